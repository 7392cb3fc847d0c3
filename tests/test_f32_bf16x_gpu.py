"""The split-bf16 fp32 matmul mode on the GPU (csrc/f32_bf16x.h: igemm_f32x_kernel under the knob
``f32_bf16x`` = 6 / 3, ``--f32-matmul bf16x6 / bf16x3``), through the cases, inputs, fp64 truths and runners of
the exact fp32 path (``pcmp.ops.truth_image_f32`` / ``truth_image_f32_run``).

Every conv case runs under both parts counts: the launch plan reads ``f32x6`` / ``f32x3`` wherever it read
``f32_big`` (but for the short reductions that stay exact at 6, ``STAYS_EXACT_X6`` of the CPU test); the grid
inputs -- every operand equals its bf16 hi part, tests/test_f32_bf16x_cpu.py -- still give the fp64 truth *bit for bit* in every tile shape and split; the random inputs stay below ``BOUNDS_X[parts]``
(4 x the floor of the CPU emulation, ``pcmp.ops.truth_f32x``); the statistics rows keep ``BOUNDS_F32``.  Then:
conv_dgrad_bnr, invariance under per-channel powers of two (bf16 parts carry fp32's exponent range), one inf
among the inputs, the exact path before and after the mode was used, and one training step of ResNet-18 and a
1-layer BERT through the public switch."""
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import truth_f32x as X, truth_image_f32 as TF, truth_image_f32_run as RF, truth_image_run as R

from test_f32_bf16x_cpu import BOUNDS_X, bounds_for, expected_tag
from test_image_truth_f32_cpu import BOUNDS_F32

pytestmark = pytest.mark.gpu
F32 = torch.float32
PARTS = [3, 2]


def ops():
    return torch.ops.pcmp


def knobs(kn, parts=None):
    return R.knobs(ops(), {**kn, "f32_bf16x": X.KNOB[parts] if parts else 0})


def _finite(ts):
    for t in ts:
        if t is not None and t.is_floating_point():
            assert torch.isfinite(t).all()


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y), "run-to-run bitwise equality"


def _runner(key, shape, gpu, rows_per):
    if key == "fwd":
        return "conv_fwd", lambda: RF.run_conv_fwd(ops(), shape, gpu, rows_per)
    if key == "fwd_fold":
        return "conv_fwd_fold", lambda: RF.run_conv_fwd_fold(ops(), shape, gpu, rows_per)
    if key == "dgrad":
        return "conv_dgrad", lambda: RF.run_conv_dgrad(ops(), shape, gpu)
    return ("conv_wgrad_fold" if key == "wgrad_fold" else "conv_wgrad"), \
        lambda: RF.run_conv_wgrad(ops(), shape, gpu, fold=key == "wgrad_fold")


# ------------------------------------------------------------------------------ 1. every conv case
@pytest.mark.parametrize("parts", PARTS)
@pytest.mark.parametrize("name", list(TF.F32_CONV_CASES))
def test_conv(gpu, name, parts):
    """Every op the case commits a tag for, in the mode: the tag, two runs bitwise equal, everything finite,
    the grid outputs exact (y_epi, y_fold, dx, dx + resid, dw, dw + dw0, also behind the fold), the random
    outputs below BOUNDS_X[parts], the statistics rows below BOUNDS_F32 with the row count the tag implies."""
    case = TF.F32_CONV_CASES[name]
    shape, tags = case["shape"], case["tags"]
    bounds = bounds_for(parts)
    with knobs(case["knobs"], parts):
        for key, committed in tags.items():
            want = expected_tag(committed, parts, name, key)
            assert RF.tag(ops(), case, key) == want, key
            gm = TF.gemm_dims(shape, RF.TAG_MODE[key][0])[0]
            rows_per = TF.stat_rows_per(want)
            op, run = _runner(key, shape, gpu, rows_per)
            exact, res, raw = run()
            _same(raw, run()[2])
            _finite(raw)
            if key == "fwd":
                assert raw[2].shape[0] == RF.expected_part_rows(gm, rows_per), (want, tuple(raw[2].shape))
            if key == "fwd_fold":
                for st in (raw[1], raw[3]):
                    assert st.shape[0] == RF.expected_part_rows(gm, rows_per), (want, tuple(st.shape))
            RF.check_exact(exact, f"{name} {key} {want}")
            RF.check_rel(bounds, op, res, f"{name} {key} {want}")
            if name == "down" and key == "dgrad":   # 1x1 stride 2: no tap reaches an odd pixel
                d = TF.conv_inputs(shape)
                for dx in (raw[0], raw[2]):
                    assert float(dx[:, 1::2].abs().max()) == 0.0 and float(dx[:, :, 1::2].abs().max()) == 0.0
                for dxr, dres in ((raw[1], d["dresq"]), (raw[3], d["dres"])):
                    assert torch.equal(dxr[:, 1::2].cpu(), dres[:, 1::2]) and torch.equal(dxr[:, :, 1::2].cpu(), dres[:, :, 1::2])


# ------------------------------------------------------------------------------ 2. conv_dgrad_bnr
@pytest.mark.parametrize("name", TF.BNR_F32_CASES)
def test_conv_dgrad_bnr(gpu, name):
    """conv_dgrad_bnr in fp32 at f32_bf16x = 6: g held to the conv_dgrad bound of BOUNDS_X[3] and exactly 0 where
    the mask is off, the bit-mask results bitwise the tensor-mask ones, part / part2 row by row (BOUNDS_F32)."""
    case = TF.F32_CONV_CASES[name]
    shape = case["shape"]
    N, H, W, C, K, Rf, s, p = shape
    rows_per = TF.reduce_rows_per(N * H * W)
    bounds = {**BOUNDS_F32, ("conv_dgrad_bnr", "g"): BOUNDS_X[3][("conv_dgrad", "dx")]}
    got = {}
    with knobs(case["knobs"], 3):
        assert RF.tag(ops(), case, "dgrad") == expected_tag(case["tags"]["dgrad"], 3, name, "dgrad")
        for form in TF.BNR_F32_FORMS:
            res, raw, mask = RF.run_conv_dgrad_bnr(ops(), shape, form, gpu, rows_per)
            _same(raw, RF.run_conv_dgrad_bnr(ops(), shape, form, gpu, rows_per)[1])
            _finite(raw)
            for part in raw[1:]:
                assert tuple(part.shape) == (RF.expected_part_rows(N * H * W, rows_per), 2, C), tuple(part.shape)
            RF.check_rel(bounds, "conv_dgrad_bnr", res, f"{name} {form}")
            g = raw[0].cpu()
            assert bool((~mask).any()) and float(g[~mask].abs().max()) == 0.0, "g where the mask is off"
            got[form] = raw
        for a, b in zip(got["tensor"], got["bits"]):
            assert torch.equal(a, b), "the bit mask gives exactly the tensor-mask result"


# ------------------------------------------------------------------------------ 3. powers of two
@pytest.mark.parametrize("parts", PARTS)
def test_power_of_two_invariance(gpu, parts):
    """t128 (128x128 tiles in all three modes): channel c of the activation times 2^e(c), channel c of the
    weights times 2^-e(c), e in [-30, 30].  The FWD output is unchanged, the DGRAD's channel c comes out times
    2^-e(c) and the WGRAD's times 2^e(c), all bit for bit: every part of a scaled operand is the scaled part.
    A split that rounds through a format of narrower exponent range shows here."""
    case = TF.F32_CONV_CASES["t128"]
    shape = case["shape"]
    N, H, W, C, K, Rf, s, p = shape
    d = TF.conv_inputs(shape)
    gen = torch.Generator().manual_seed(11)
    sc = (2.0 ** torch.randint(-30, 31, (C,), generator=gen).float())
    x, w, dy, xs, ws = R.to(gpu, d["x"], d["w"], d["dy"], d["x"] * sc, d["w"] / sc)
    sc = sc.to(gpu)
    with knobs(case["knobs"], parts):
        for key in ("fwd", "dgrad", "wgrad"):
            assert RF.tag(ops(), case, key) == expected_tag(case["tags"][key], parts, "t128", key)
        y0, y1 = (ops().conv_fwd(a, b, s, p, None, None, False, False)[0] for a, b in ((x, w), (xs, ws)))
        assert torch.equal(y0, y1), "FWD"
        dx0, dx1 = (ops().conv_dgrad(dy, b, H, W, s, p, None) for b in (w, ws))
        assert torch.equal(dx0, dx1 * sc), "DGRAD"
        dw0, dw1 = torch.empty_like(w), torch.empty_like(w)
        ops().conv_wgrad(dy, x, dw0, Rf, Rf, s, p, False)
        ops().conv_wgrad(dy, xs, dw1, Rf, Rf, s, p, False)
        assert torch.equal(dw0, dw1 / sc), "WGRAD"
        assert float(y0.abs().max()) > 0 and float(dx0.abs().max()) > 0 and float(dw0.abs().max()) > 0


# ------------------------------------------------------------------------------ 4. one non-finite input
@pytest.mark.parametrize("parts", PARTS)
def test_single_inf(gpu, parts):
    """One +inf in x on k144 FWD: exactly the outputs whose receptive field holds it are +inf, every other output
    is bitwise what it is without the inf.  The weights are strictly positive, and so is each of their bf16
    parts (bits 15 and 6 cleared, 14 and 5 set: both roundings go down and leave a residual; asserted below):
    a weight with a negative mid part would meet the inf as inf * mid = -inf, and the sum of the part products
    would be NaN where exact fp32 gives +inf.  That is the mode's contract for a non-finite operand: the split
    of the operand itself never produces inf - inf; a product of an inf with the other operand's residuals can."""
    case = TF.F32_CONV_CASES["k144"]
    shape = case["shape"]
    N, H, W, C, K, Rf, s, p = shape
    d = TF.conv_inputs(shape)
    w = ((d["w"].abs() + 0.01).view(torch.int32) & ~0x8040 | 0x4020).view(F32)
    assert all(bool((q > 0).all()) for q in X.split_bf16(w, 3))
    x1 = d["x"].clone()
    n0, h0, w0, c0 = 1, 2, 0, 5
    x1[n0, h0, w0, c0] = float("inf")
    hit = torch.zeros(N, H, W, K, dtype=torch.bool)   # 3x3 stride 1 pad 1: P = H, Q = W
    hit[n0, max(h0 - 1, 0):h0 + 2, max(w0 - 1, 0):w0 + 2] = True
    x0g, x1g, wg = R.to(gpu, d["x"], x1, w)
    with knobs(case["knobs"], parts):
        assert RF.tag(ops(), case, "fwd") == expected_tag(case["tags"]["fwd"], parts, "k144", "fwd")
        y0 = ops().conv_fwd(x0g, wg, s, p, None, None, False, False)[0].cpu()
        y1 = ops().conv_fwd(x1g, wg, s, p, None, None, False, False)[0].cpu()
    assert bool(torch.isfinite(y0).all())
    assert torch.equal(y1 == float("inf"), hit), "+inf exactly over the receptive field"
    assert torch.equal(y1[~hit], y0[~hit]), "every other output unchanged"


# ------------------------------------------------------------------------------ 5. the exact path
def test_exact_path_untouched(gpu):
    """f32_bf16x = 0 before and after the mode was used in the process: the same bits."""
    def run_all():
        out = []
        for name in ("t128", "split", "k144"):
            case = TF.F32_CONV_CASES[name]
            with knobs(case["knobs"]):
                for key in ("fwd", "dgrad", "wgrad"):
                    assert RF.tag(ops(), case, key) == case["tags"][key]
                    out += _runner(key, case["shape"], gpu, TF.stat_rows_per(case["tags"][key]))[1]()[2]
        return out

    before = run_all()
    for parts in PARTS:
        case = TF.F32_CONV_CASES["t128"]
        with knobs(case["knobs"], parts):
            _runner("fwd", case["shape"], gpu, 128)[1]()
    _same(before, run_all())


# ------------------------------------------------------------------------------ 6. model level
def test_resnet18_step_matches_exact(gpu):
    """One fp32 training step of ResNet-18 (10 classes, 2x3x64x64) under set_f32_matmul("bf16x6") against the
    step the exact kernels give from the same seed: the loss and every parameter gradient, by the comparator
    and at the constant of the fp32 model test of tests/test_f32_gpu.py (rel_close at its default)."""
    from test_f32_gpu import rel_close
    from pcmp.models import resnet
    from pcmp.ops import _lib, cross_entropy

    def step(mode):
        _lib.set_f32_matmul(mode)
        torch.manual_seed(5)
        m = resnet.resnet18(10).to(gpu).train()
        x = torch.rand(2, 3, 64, 64, device=gpu)
        y = torch.randint(0, 10, (2,), device=gpu)
        loss = cross_entropy(m.forward_logits(x), y)
        loss.backward()
        return loss.detach(), {n: q.grad for n, q in m.named_parameters() if q.grad is not None}

    _lib.set_precision("fp32")
    try:
        l0, g0 = step("exact")
        l1, g1 = step("bf16x6")
        assert ops().set_knob("f32_bf16x", 6) == 6
    finally:
        _lib.set_f32_matmul("exact")
        _lib.set_precision("bf16")
    assert l0.dtype == F32 and len(g0) > 20 and set(g0) == set(g1)
    rel_close(l1, l0)
    for n in g0:
        assert torch.isfinite(g1[n]).all(), n
        rel_close(g1[n], g0[n])


def test_bert_entrypoint(gpu, tmp_path):
    """A 1-layer fp32 BERT through --f32-matmul bf16x6: it finishes with finite losses and records the field."""
    import pytorch_on_language_distr as entry
    from pcmp.ops import _lib
    out = tmp_path / "rec.json"
    try:
        rc = entry.main(["--model", "bert", "--dtype", "fp32", "--f32-matmul", "bf16x6", "--layers", "1", "--max-len", "64",
                         "--batch-size", "8", "--train-size", "16", "--test-size", "8", "--epochs", "1", "--json", str(out)])
        assert ops().set_knob("f32_bf16x", 6) == 6, "the switch reached the native library"
    finally:
        _lib.set_f32_matmul("exact")
        _lib.set_precision("bf16")
    assert rc == 0
    rec = json.loads(out.read_text().strip().splitlines()[-1])
    assert rec["f32_matmul"] == "bf16x6" and rec["dtype"] == "fp32" and len(rec["train_loss"]) == 1
    assert all(l == l and abs(l) < 1e3 for l in rec["train_loss"]), rec["train_loss"]
