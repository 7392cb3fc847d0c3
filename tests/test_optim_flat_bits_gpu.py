"""The flat optimizer ops against their recorded bits: every case of tools/optim_flat_bits.py is run again
and the sha256 of each output buffer compared with tests/data/optim_flat_bits_mi355x.txt, recorded on
the MI355X from the parent of the change that gave the grouped and the ungrouped kernels one element
update.  Since that change "grouped equals ungrouped" (tests/test_optim_groups_gpu.py) holds by
construction; this file is what holds the one definition to the arithmetic of the kernels before it."""
import importlib.util
import pathlib

import pytest

import pcmp  # noqa: F401

_spec = importlib.util.spec_from_file_location(
    "optim_flat_bits", pathlib.Path(__file__).parent.parent / "tools" / "optim_flat_bits.py")
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("op", bits.OPS)
def test_bits_are_the_recorded_ones(gpu, op):
    recorded = {k: h for k, h in bits.read().items() if k[0].split("/")[0] == op}
    assert recorded, "no recorded digest for " + op
    seen, wrong = set(), []
    for case, buf, h in bits.digests(gpu, op):
        assert (case, buf) in recorded, f"{case} {buf}: not in the recorded file"
        seen.add((case, buf))
        if h != recorded[case, buf]:
            wrong.append(f"{case} {buf}")
    assert not wrong, f"{len(wrong)} of {len(seen)} buffers differ from the recorded bits: " + ", ".join(wrong[:20])
    assert seen == set(recorded), f"recorded but not visited: {sorted(set(recorded) - seen)[:20]}"
