"""The conv kernel choice (csrc/igemm_launch.h choose_kernel and the FWD / DGRAD / WGRAD routes) without
a GPU: ``torch.ops.pcmp.conv_kernel_choice`` and ``set_knob`` are host code.  The tag formats the same
choice value the launch switches on and the partial-statistics buffers are sized from, so these tests
hold the launch policy itself; tests/test_image_truth_gpu.py checks on the GPU that the rows a launch
writes are the rows that choice sized."""
import collections
import pathlib

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import truth_image as T, truth_image_run as R

TABLE = pathlib.Path(__file__).parent / "data" / "conv_kernel_choice.txt"
KNOBSETS = {"default": {}, "static": {"gemm_plan": 0, "wgrad_wgs": 1024}}   # tools/conv_choice_table.py


@pytest.fixture(scope="module")
def ops():
    from pcmp.ops import _lib
    if not _lib.load():
        pytest.skip(f"native library not built: {_lib.load_error()}")
    return torch.ops.pcmp


def test_committed_tags(ops):
    """Every tag the conv cases of ops/truth_image.py commit, under the case's knobs: the assertion each
    GPU conv test opens with.  The knobs are back at their defaults afterwards."""
    def peek(n):   # set_knob returns the value it replaces
        v = ops.set_knob(n, 0)
        ops.set_knob(n, v)
        return v

    names = sorted({n for cases in (T.CONV_CASES, T.WGRAD_CASES, T.FWD_FOLD_CASES, T.BNR_STREAM_CASES)
                    for c in cases.values() for n in c["knobs"]})
    before = {n: peek(n) for n in names}
    rows = R.committed_tags(ops)
    assert len(rows) >= 114
    bad = [r for r in rows if r[1] != r[2]]
    assert not bad, bad
    assert before == {n: peek(n) for n in names}, "a case left a knob changed"


def test_production_shapes_against_table(ops):
    """The ResNet-50 / ResNet-18 conv shapes at N = 256, 64, 1 and BERT-base's Linear shapes, every
    operand combination the steps use, under the default knobs and the static set: the current library
    reproduces every line of the table recorded from the parent of the change that introduced
    choose_kernel (tools/conv_choice_table.py)."""
    by_set = collections.defaultdict(list)
    for line in TABLE.read_text().splitlines():
        if line and not line.startswith("#"):
            f = line.split()
            by_set[f[0]].append(([int(v) for v in f[1:11]], f[11]))
    assert set(by_set) == set(KNOBSETS) and sum(map(len, by_set.values())) >= 2880
    families, bad = set(), []
    for ks, rows in by_set.items():
        with R.knobs(ops, KNOBSETS[ks]):
            for args, want in rows:
                got = ops.conv_kernel_choice(*args)
                families.update(t.split("/")[0] for t in want.split("+"))
                if got != want:
                    bad.append((ks, args, want, got))
    assert not bad, f"{len(bad)} of the table's lines differ, the first: {bad[:5]}"
    assert len(families) >= 14, families
