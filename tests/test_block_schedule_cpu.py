"""The residual-block / stem schedule as data, without a GPU.

``replay`` runs one configuration of tools/block_schedule_table.py in this process and compares the op
trace -- every dispatched op with its argument shapes and scalars, in host order, with the side-stream
calls marked -- line for line with tests/data/block_schedule_cpu.txt, recorded from the parent of the
change that introduced ``plan_backward``.  tests/test_block_schedule_gpu.py does the same on the GPU.
The plan functions are also asked directly for the combinations their comments promise."""
import importlib.util
import itertools
import pathlib

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import conv_blocks as CB, kernels, params

_spec = importlib.util.spec_from_file_location(
    "block_schedule_table", pathlib.Path(__file__).parent.parent / "tools" / "block_schedule_table.py")
table = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(table)


def replay(name, device, monkeypatch):
    """Trace lines of configuration ``name`` on ``device`` and the recorded ones."""
    recorded = table.read_table(table.table_path(device))
    assert name in recorded, f"no recorded trace for {name}"
    try:
        with monkeypatch.context() as mp:
            for k in table.SWITCHES:
                mp.delenv(k, raising=False)
            for k, v in table.CONFIGS[name][1].items():
                mp.setenv(k, v)
            mp.setattr(kernels, "TRACE", [])
            params.refresh_env()
            lines, _ = table.trace_lines(name, device)
    finally:
        params.refresh_env()   # the cached side-stream switches follow the restored environment
    return lines, recorded[name]


@pytest.mark.parametrize("name", list(table.CONFIGS))
def test_schedule_matches_recorded_cpu(name, monkeypatch):
    lines, want = replay(name, torch.device("cpu"), monkeypatch)
    assert len(lines) == len(want)
    bad = [(i, a, b) for i, (a, b) in enumerate(zip(lines, want)) if a != b]
    assert not bad, f"{len(bad)} trace lines differ, the first: {bad[:3]}"


# ---- the plan function alone (conditions, not measurements: on_gpu=True needs no GPU) ---------------
def _bottleneck(cin, planes, stride, keras=False):   # keras: the stride on the first 1x1, not on the 3x3
    convs = [CB.Conv(1, 1, stride if keras else 1, 0, cin, planes),
             CB.Conv(3, 3, 1 if keras else stride, 1, planes, planes), CB.Conv(1, 1, 1, 0, planes, 4 * planes)]
    down = CB.Conv(1, 1, stride, 0, cin, 4 * planes) if (stride != 1 or cin != 4 * planes) else None
    return convs, down


def _basic(cin, planes, stride):
    convs = [CB.Conv(3, 3, stride, 1, cin, planes), CB.Conv(3, 3, 1, 1, planes, planes)]
    return convs, CB.Conv(1, 1, stride, 0, cin, planes) if (stride != 1 or cin != planes) else None


# (convs, down, input [N, H, W, C]) at B = 256, 224x224 images: ResNet-50 layers 1-4, first block (with
# downsample) and a later one (without); the Keras variant's downsampling blocks; ResNet-18 likewise
BLOCKS = [(*_bottleneck(cin, pl, st), (256, hw, hw, cin))
          for cin, pl, st, hw in [(64, 64, 1, 56), (256, 64, 1, 56), (256, 128, 2, 56), (512, 128, 1, 28),
                                  (512, 256, 2, 28), (1024, 256, 1, 14), (1024, 512, 2, 14), (2048, 512, 1, 7)]]
BLOCKS += [(*_bottleneck(cin, pl, 2, keras=True), (256, hw, hw, cin))
           for cin, pl, hw in [(256, 128, 56), (512, 256, 28), (1024, 512, 14)]]
BLOCKS += [(*_basic(cin, pl, st), (256, hw, hw, cin))
           for cin, pl, st, hw in [(64, 64, 1, 56), (64, 128, 2, 56), (128, 128, 1, 28), (128, 256, 2, 28),
                                   (256, 256, 1, 14), (256, 512, 2, 14), (512, 512, 1, 7)]]


def _switches(monkeypatch, minrows0, **over):
    for k in table.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if minrows0:
        for k, v in table.MIN0.items():
            monkeypatch.setenv(k, v)
    return CB.read_switches()._replace(**{"side_stream": True, **over})


@pytest.mark.parametrize("minrows0", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_plan_combinations(dtype, minrows0, monkeypatch):
    sw = _switches(monkeypatch, minrows0)
    seen = set()
    for (convs, down, xshape), need_dx, prev, reduced, sync, sink in itertools.product(
            BLOCKS, (False, True), (False, True), (False, True), (False, True), (False, True)):
        n = len(convs)
        fp = CB.plan_forward(convs, down, xshape, dtype, True, True, True, sync, sw)
        act = [False] + list(fp.act_fold)
        nw = n + (down is not None)
        bp = CB.plan_backward(convs, down, xshape, dtype, True, need_dx, prev, reduced, sync, act, [True] * nw,
                              [sink] * nw, sw)
        assert len(bp.dgrad) == len(bp.dz_fold) == n and len(bp.wgrad_side) == nw and len(fp.act_fold) == n - 1
        # the fused conv3 kernel: only with a folded 64-channel input and 256 output channels
        for i, form in enumerate(bp.dgrad):
            assert (form in (CB.Dgrad.INTO_PREV, CB.Dgrad.NONE)) <= (i == 0)
            if form is CB.Dgrad.FUSED:
                assert act[i] and convs[i].cin == 64 and convs[i].cout == 256 and dtype == torch.bfloat16
                seen.add("fused")
        # the first conv's DGRAD: none without an input gradient, into the previous tail only if linked
        assert (bp.dgrad[0] is CB.Dgrad.NONE) == (not need_dx)
        assert (bp.dgrad[0] is CB.Dgrad.INTO_PREV) <= prev
        # conv1's dz folded only with no input gradient or the DGRAD into the previous tail
        if bp.dz_fold[0]:
            assert bp.dgrad[0] in (CB.Dgrad.NONE, CB.Dgrad.INTO_PREV) and convs[0].is_1x1s1
            seen.add("fold0")
        assert bp.dz_fold[-1] <= reduced and not any(bp.dz_fold[1:-1])
        seen.update(["fold_tail"] * bp.dz_fold[-1])
        if dtype == torch.float32:
            assert not any(bp.dz_fold) and CB.Dgrad.FUSED not in bp.dgrad
        # the downsample: compact only on the side stream, into a stride-1 conv1; nothing forked with SyncBN
        assert bp.down_compact <= (bp.down_side and convs[0].stride == 1 and down.stride == 2)
        assert bp.down_side <= (down is not None and bp.dgrad[0] is CB.Dgrad.INTO_PREV)
        seen.update(["compact"] * bp.down_compact)
        if convs[0].stride == 2 and convs[0].R == 1:   # no BN-reduce epilogue on a 1x1 stride-2 DGRAD
            assert bp.dgrad[0] is not CB.Dgrad.INTO_PREV and not bp.down_side
        if sync:
            assert not (fp.down_side or bp.down_side or bp.down_compact)
        assert bp.wgrad_side == (sink,) * nw and fp.mbits
    # layer 1 at B = 256 has 802,816 rows: every bf16 path occurs at the default thresholds already
    want = {"compact", "fold0", "fold_tail", "fused"} if dtype == torch.bfloat16 else set()
    assert seen == want, (want, seen)


def test_plan_switches_off(monkeypatch):
    """Every switch at 0 takes its path out of every plan; the eval fork follows EVAL_FORK_MAX_ROWS."""
    sw = _switches(monkeypatch, True, act_fold=False, dz_fold=False, compact_down=False, down_stream=False,
                   side_stream=False)
    for convs, down, xshape in BLOCKS:
        nw = len(convs) + (down is not None)
        fp = CB.plan_forward(convs, down, xshape, torch.bfloat16, True, True, True, False, sw)
        bp = CB.plan_backward(convs, down, xshape, torch.bfloat16, True, True, True, True, False,
                              [False] * len(convs), [True] * nw, [True] * nw, sw)
        assert not (any(fp.act_fold) or fp.down_side or any(bp.dz_fold) or bp.down_side or bp.down_compact
                    or any(bp.wgrad_side)) and CB.Dgrad.FUSED not in bp.dgrad
    convs, down, xshape = BLOCKS[0]
    sw = _switches(monkeypatch, False)
    assert not CB.plan_forward(convs, down, (1, 56, 56, 64), torch.bfloat16, True, False, False, False, sw).down_side
    monkeypatch.setattr(CB, "EVAL_FORK_MAX_ROWS", 56 * 56)
    assert CB.plan_forward(convs, down, (1, 56, 56, 64), torch.bfloat16, True, False, False, False, sw).down_side
    assert not CB.plan_forward(convs, down, (2, 56, 56, 64), torch.bfloat16, True, False, False, False, sw).down_side
