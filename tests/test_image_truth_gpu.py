"""The image-path HIP kernels (csrc/igemm*.hip, bnr_stream.h, wgrad32.h, bwd_fused.h, bn.hip,
elementwise.hip's pooling, optim.hip) against the fp64 autograd truths of ``pcmp.ops.truth_image``,
element by element, at the smallest shapes that reach each kernel.  Every case runs the forward, then
the backward on the forward's own saved outputs, through the runners of ``pcmp.ops.truth_image_run``
(the same cases tests/test_image_truth_cpu.py puts ``ops/ref.py`` through), and is held to ``BOUNDS``
of that file: k times ``1e-2*|t| + 5e-3*max_seg|t|`` for every element.  Every conv case first asserts
the kernel it takes (``torch.ops.pcmp.conv_kernel_choice``), so a policy change that moves a case off
its kernel fails loudly; it also asserts finite outputs, the exact zeros of masked gradients, the
bitwise invariants between equivalent forms, and run-to-run bitwise equality."""
import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import ref, truth_image as T, truth_image_run as R

from test_image_truth_cpu import BN_VARIANTS, BOUNDS, OPT_GS, bnr_forms, check_masked, conv_ops

pytestmark = pytest.mark.gpu


def ops():
    return torch.ops.pcmp


def knobs(kn):
    return R.knobs(ops(), kn)


def _finite(ts):
    for t in ts:
        if t is not None and t.is_floating_point():
            assert torch.isfinite(t.float()).all()


def _same(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y), "run-to-run bitwise equality"


def _tag(case, key, flags=None):
    return R.tag(ops(), case, key, flags)


def _rows(part, tag, case, mode):
    """The launch wrote what the choice sized: a partial-statistics tensor has one row per BM-row tile
    of every GEMM of its tag (the streaming kernels, one row per workgroup group, aside)."""
    want = R.part_rows(tag, case["shape"], mode)
    assert want is None or part.shape[0] == want, (tag, tuple(part.shape), want)


def _names(op_keys, cases=T.CONV_CASES):
    return [n for n, c in cases.items() if set(op_keys) & set(conv_ops(c))]


# ------------------------------------------------------------------------------ convolution
@pytest.mark.parametrize("name", _names(("fwd", "fwd_stats", "fwd_epi")))
def test_conv_fwd(gpu, name):
    """With statistics, with bias + residual + ReLU, and (the halo cases, whose kernel takes no bias)
    with residual + ReLU alone."""
    case = T.CONV_CASES[name]
    o = conv_ops(case)
    stats, epi, res_only = "fwd_epi" not in o, "fwd_stats" not in o, "fwd_res" in o
    with knobs(case["knobs"]):
        if stats:
            assert _tag(case, "fwd") == case["tags"]["fwd"]
        if epi:
            assert _tag(case, "fwd_epi") == case["tags"]["fwd_epi"]
        if res_only:
            assert _tag(case, "fwd_res") == case["tags"]["fwd_res"]
        res, raw = R.run_conv_fwd(ops(), name, gpu, stats, epi, res_only)
        _, raw2 = R.run_conv_fwd(ops(), name, gpu, stats, epi, res_only)
    if stats:
        _rows(raw[1], case["tags"]["fwd"], case, 0)
    _finite(raw)
    R.check(BOUNDS, "conv_fwd", res, name)
    _same(raw, raw2)


@pytest.mark.parametrize("name", list(T.FWD_FOLD_CASES))
def test_conv_fwd_fold(gpu, name):
    """conv_fwd behind the BatchNorm-forward fold (in_scale / in_shift), with statistics: the fold's
    register-staged tiles and the streaming FWD's fold form."""
    case = T.FWD_FOLD_CASES[name]
    with knobs(case["knobs"]):
        assert ops().conv_kernel_choice(0, *case["shape"], 1 | 16) == case["tags"]
        res, raw = R.run_conv_fwd_fold(ops(), name, gpu)
        _, raw2 = R.run_conv_fwd_fold(ops(), name, gpu)
    _rows(raw[1], case["tags"], case, 0)
    _finite(raw)
    R.check(BOUNDS, "conv_fwd_fold", res, name)
    _same(raw, raw2)


@pytest.mark.parametrize("name", _names(("dgrad",)))
def test_conv_dgrad(gpu, name):
    case = T.CONV_CASES[name]
    with knobs(case["knobs"]):
        assert _tag(case, "dgrad") == case["tags"]["dgrad"]
        res, raw = R.run_conv_dgrad(ops(), name, gpu)
        _, raw2 = R.run_conv_dgrad(ops(), name, gpu)
    _finite(raw)
    R.check(BOUNDS, "conv_dgrad", res, name)
    _same(raw, raw2)
    if name == "down":   # 1x1 stride 2: no tap reaches an odd pixel
        dx = raw[0]
        assert float(dx[:, 1::2].float().abs().max()) == 0.0 and float(dx[:, :, 1::2].float().abs().max()) == 0.0
        assert torch.equal(raw[1][:, 1::2], T.conv_inputs(name)["dres"].to(gpu)[:, 1::2])


@pytest.mark.parametrize("name", _names(("bnr", "bnr_halo")) + list(T.BNR_STREAM_CASES))
def test_conv_dgrad_bnr(gpu, name):
    """Every form of conv_dgrad_bnr the case's kernel has (test_image_truth_cpu.bnr_forms); the single
    and dual BN-reduce epilogues at epilogue depth 2 and 4."""
    case = R.all_cases()[name]
    forms = ("recompute", "tensor") if name == "halo" else bnr_forms(name)
    got = {}
    with knobs(case["knobs"]):
        for form in forms:
            f = T.BNR_FORMS[form]
            depth_knob = "epi_depth_bnr2" if f.get("dual") else "epi_depth"
            for depth in ((2, 4) if form in ("recompute", "dual_resid", "dual_bits") else (None,)):
                with knobs({depth_knob: depth} if depth else {}):
                    assert _tag(case, "bnr", f["flags"]) == R.bnr_tag(name, case, form), form
                    res, raw, mask = R.run_conv_dgrad_bnr(ops(), name, form, gpu)
                    _, raw2, _ = R.run_conv_dgrad_bnr(ops(), name, form, gpu)
                for part in raw[1:]:
                    _rows(part, R.bnr_tag(name, case, form), case, 1)
                _finite(raw)
                R.check(BOUNDS, "conv_dgrad_bnr_fold" if form == "fold" else "conv_dgrad_bnr", res, f"{name} {form} depth={depth}")
                _same(raw, raw2)
                g = raw[0].cpu()
                assert float(g[~mask].float().abs().max() if (~mask).any() else 0.0) == 0.0, "g where the mask is off"
                got[form] = raw
    if "tensor" in got and "bits" in got:
        for a, b in zip(got["tensor"], got["bits"]):
            assert torch.equal(a, b), "the bit mask gives exactly the tensor-mask result"


@pytest.mark.parametrize("name", _names(("wgrad",)) + list(T.WGRAD_CASES))
def test_conv_wgrad(gpu, name):
    if name in T.WGRAD_CASES:
        case = T.WGRAD_CASES[name]
        with knobs(case["knobs"]):
            assert ops().conv_kernel_choice(2, *case["shape"], R.WGRAD_FOLD_FLAGS[case.get("fold")]) == case["tags"]
            op, res, raw = R.run_wgrad_case(ops(), name, gpu)
            _, _, raw2 = R.run_wgrad_case(ops(), name, gpu)
    else:
        case = T.CONV_CASES[name]
        op = "conv_wgrad"
        with knobs(case["knobs"]):
            assert _tag(case, "wgrad") == case["tags"]["wgrad"]
            res, raw = R.run_conv_wgrad(ops(), name, gpu)
            _, raw2 = R.run_conv_wgrad(ops(), name, gpu)
    _finite(raw)
    R.check(BOUNDS, op, res, name)
    _same(raw, raw2)


@pytest.mark.parametrize("M,fold", R.FUSED_SHAPES)
def test_conv1x1_bwd_fused(gpu, M, fold):
    res, raw, mask = R.run_bwd_fused(ops(), M, fold, gpu)
    _, raw2, _ = R.run_bwd_fused(ops(), M, fold, gpu)
    _finite(raw)
    R.check(BOUNDS, "conv1x1_bwd_fused", res, f"M={M} fold={fold}")
    _same(raw, raw2)
    assert float(raw[0].cpu()[~mask].float().abs().max()) == 0.0, "g where the recomputed mask is off"


# ------------------------------------------------------------------------------ BatchNorm
@pytest.mark.parametrize("M,C", T.BN_SHAPES)
def test_batchnorm_chain(gpu, M, C):
    """Every x2 mode / ReLU / accumulate variant under the default knobs; the ReLU variants again with
    bn_apply_v = 1 (generic kernels), ew_unroll = 4 (unrolled body + remainder) and bn_wide_rows on
    both sides of the partial-row count.  The mask bits are bitwise pack_mask_bits of the kernel's
    own y, and y does not depend on whether they are asked for."""
    for kn in ({}, {"bn_apply_v": 1}, {"ew_unroll": 4}, {"bn_wide_rows": 1}, {"bn_wide_rows": 1 << 20}):
        for mode, relu, acc in BN_VARIANTS:
            if kn and not (relu and acc):
                continue
            with knobs(kn):
                res, raw = R.run_bn(ops(), M, C, mode, relu, acc, gpu, mbits=True)
                _, raw2 = R.run_bn(ops(), M, C, mode, relu, acc, gpu, mbits=False)
            _finite([raw["y"], *raw["outs"], *raw["stats"]])
            R.check(BOUNDS, R.bn_op(M), res, f"{(M, C)} {mode} relu={relu} acc={acc} {kn}")
            assert torch.equal(raw["mbits"], ref.pack_mask_bits(raw["y"])), "mask bits of the kernel's own y"
            _same([raw["y"], *raw["outs"], *raw["stats"]], [raw2["y"], *raw2["outs"], *raw2["stats"]])
            if relu:
                off = raw["y"] <= 0
                for t in raw["outs"][-1:]:
                    assert float(t[off].float().abs().max() if off.any() else 0.0) == 0.0, "g where y is off"


# ------------------------------------------------------------------------------ pooling
@pytest.mark.parametrize("shape", T.POOL_SHAPES)
def test_pooling(gpu, shape):
    """pool3s2 / pool_quad on and off.  maxpool_bwd_bnr takes channel counts whose 8-wide vectors divide
    a 256-thread block; C = 72 must be refused loudly, not computed wrongly."""
    if not R.pool_bnr_ok(shape[3]):
        d = T.pool_case(shape)
        a = R.to(gpu, d["dy"], d["x"], d["mean"], d["invstd"], d["scale"], d["shift"])
        idx = ops().maxpool_fwd(a[1], 3, 2, 1, True, a[4], a[5])[1]
        with pytest.raises(RuntimeError, match="channel layout"):
            ops().maxpool_bwd_bnr(a[0], idx, a[1], a[2], a[3], a[4], a[5], 3, 2, 1)
    first = None
    for p3, pq in ((1, 1), (0, 1), (1, 0), (0, 0)):
        with knobs({"pool3s2": p3, "pool_quad": pq}):
            res, raw, mask = R.run_pool(ops(), shape, gpu)
        _finite(raw)
        R.check(BOUNDS, "pool", res, f"{shape} pool3s2={p3} pool_quad={pq}")
        if R.pool_bnr_ok(shape[3]):
            assert float(raw[5].cpu()[~mask].float().abs().max()) == 0.0, "g where the prologue's ReLU is off"
        if first is None:
            first = raw
        else:   # the maximum and its index are exact: the variants agree bitwise
            _same([first[i] for i in (0, 1, 3, 4)], [raw[i] for i in (0, 1, 3, 4)])


# ------------------------------------------------------------------------------ optimizers
@pytest.mark.parametrize("n", T.OPT_SIZES)
def test_optimizers(gpu, n):
    """Every gscale / shadow / variant combination at the two small sizes; at the size that needs the
    second trip of the grid-stride loop one combination per kernel (the loop is all that differs)."""
    big = n > (1 << 20)
    for gs in (OPT_GS[1:] if big else OPT_GS):
        for sh in ((True,) if big else (True, False)):
            for v in range(1 if big else len(R.SGD_VARIANTS)):
                res, (w, mom, s) = R.run_sgd(ops(), n, v, gs, sh, gpu)
                R.check(BOUNDS, "sgd", res, f"n={n} variant={v} gscale={gs} shadow={sh}")
                assert s is None or torch.equal(s, w.to(torch.bfloat16)), "shadow == bf16(w)"
            for dec in (False, True):
                res, (w, m1, m2, s) = R.run_adam(ops(), n, dec, gs, sh, gpu)
                R.check(BOUNDS, "adam", res, f"n={n} decoupled={dec} gscale={gs} shadow={sh}")
                assert s is None or torch.equal(s, w.to(torch.bfloat16)), "shadow == bf16(w)"
    for dec in ((False,) if big else (False, True)):
        res, (w, m1, m2, s) = R.run_adam_late(ops(), n, dec, gpu)
        R.check(BOUNDS, "adam", res, f"n={n} t=10000 decoupled={dec}")
        assert torch.equal(s, w.to(torch.bfloat16))
    for v in R.clip_variants(n)[:1 if big else 3]:
        res, (norm, coef, part) = R.run_clip(ops(), n, v, gpu)
        R.check(BOUNDS, "clip", res, f"n={n} {v}")
        assert torch.isfinite(part).all(), "every partial-sum row of the NaN-filled buffer is written"


def test_optimizer_mask_semantics(gpu):
    """The kernels' ``mask`` as test_image_truth_cpu.test_optimizer_mask_semantics pins it on the
    reference: masked elements keep w; Adam keeps its moments; SGD's momentum still advances."""
    check_masked(R.run_masked(ops(), 4 * 257, gpu))
