"""The distance of ``ops/ref.py`` from the fp64 truths of ``pcmp.ops.truth_image`` (convolutions,
BatchNorm, pooling, optimizers), the input conditions of the committed cases, and the defects the
element-wise comparator must reject, on the CPU.

``BOUNDS`` holds, per (op, output), the worst ``norm_err`` of ``ops/ref.py`` against the truth over
every case of tests/test_image_truth_gpu.py (the *floor*) and the bound ``k`` the GPU tests hold the
kernels to.  The rule is that of tests/test_text_truth_cpu.py: outputs with a floor <= 1e-4 (fp32
statistics, sums, weight gradients without a fold, optimizer state) get k = 0.01; every other output
k = 2 * floor rounded up to a multiple of 0.5, at least 1 and never above max(1, 4 * floor).
``test_reference_floors`` recomputes every floor and enforces the rule.
"""
import math

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import ref, truth_image as T, truth_image_run as R

# (op, output): (floor of ops/ref.py on the CPU, bound k of the GPU tests)
BOUNDS = {
    ("adam", "m1"): (1.4e-05, 0.01), ("adam", "m2"): (1.6e-05, 0.01), ("adam", "shadow"): (0.240, 1.0),
    ("adam", "w"): (1.5e-05, 0.01),
    ("bn", "bwd_part"): (2.0e-05, 0.01), ("bn", "bwd_part2"): (2.2e-05, 0.01), ("bn", "dbeta"): (6.7e-06, 0.01),
    ("bn", "dbeta2"): (4.7e-06, 0.01), ("bn", "dgamma"): (2.3e-05, 0.01), ("bn", "dgamma2"): (2.3e-05, 0.01),
    ("bn", "dx"): (0.259, 1.0), ("bn", "dx2"): (0.257, 1.0), ("bn", "invstd"): (9.1e-06, 0.01),
    ("bn", "invstd2"): (7.2e-06, 0.01), ("bn", "mean"): (9.7e-06, 0.01), ("bn", "mean2"): (5.3e-06, 0.01),
    ("bn", "part"): (1.2e-05, 0.01), ("bn", "running_mean"): (1.0e-05, 0.01),
    ("bn", "running_mean2"): (6.0e-06, 0.01), ("bn", "running_var"): (8.1e-06, 0.01),
    ("bn", "running_var2"): (7.6e-06, 0.01), ("bn", "y"): (0.257, 1.0),
    ("bn_one_row", "bwd_part"): (0.0, 0.01), ("bn_one_row", "bwd_part2"): (0.0, 0.01),
    ("bn_one_row", "dbeta"): (0.0, 0.01), ("bn_one_row", "dbeta2"): (0.0, 0.01),
    ("bn_one_row", "dgamma"): (0.0, 0.01), ("bn_one_row", "dgamma2"): (0.0, 0.01),
    ("bn_one_row", "dx2"): (0.0, 0.01), ("bn_one_row", "invstd"): (2.8e-06, 0.01),
    ("bn_one_row", "invstd2"): (2.8e-06, 0.01), ("bn_one_row", "mean"): (0.0, 0.01),
    ("bn_one_row", "mean2"): (0.0, 0.01), ("bn_one_row", "part"): (0.0, 0.01),
    ("bn_one_row", "running_mean"): (6.2e-06, 0.01), ("bn_one_row", "running_mean2"): (5.8e-06, 0.01),
    ("bn_one_row", "running_var"): (4.8e-06, 0.01), ("bn_one_row", "running_var2"): (5.0e-06, 0.01),
    ("bn_one_row", "y"): (0.241, 1.0),
    ("clip", "coef"): (5.5e-06, 0.01), ("clip", "norm"): (2.3e-06, 0.01),
    ("conv1x1_bwd_fused", "dw"): (0.589, 1.5), ("conv1x1_bwd_fused", "g"): (0.571, 1.5),
    ("conv1x1_bwd_fused", "part"): (8.1e-06, 0.01),
    ("conv_dgrad", "dx"): (0.259, 1.0), ("conv_dgrad", "dx_resid"): (0.251, 1.0),
    ("conv_dgrad_bnr", "g"): (0.257, 1.0), ("conv_dgrad_bnr", "part"): (2.2e-05, 0.01),
    ("conv_dgrad_bnr", "part2"): (1.9e-05, 0.01),
    ("conv_dgrad_bnr_fold", "g"): (0.776, 2.0), ("conv_dgrad_bnr_fold", "part"): (1.5e-05, 0.01),
    ("conv_fwd", "stats"): (1.2e-05, 0.01), ("conv_fwd", "y"): (0.257, 1.0), ("conv_fwd", "y_epi"): (0.259, 1.0),
    ("conv_fwd_fold", "stats"): (9.0e-06, 0.01), ("conv_fwd_fold", "y"): (0.258, 1.0),
    ("conv_wgrad", "dw"): (4.0e-05, 0.01), ("conv_wgrad", "dw_acc"): (4.2e-05, 0.01),
    ("conv_wgrad_fold", "dw"): (0.708, 1.5), ("conv_wgrad_fold", "dw_acc"): (0.651, 1.5),
    ("pool", "dx"): (0.250, 1.0), ("pool", "g"): (0.250, 1.0), ("pool", "gap_dx"): (0.231, 1.0),
    ("pool", "gap_y"): (0.229, 1.0), ("pool", "part"): (1.1e-05, 0.01), ("pool", "y"): (0.0, 0.01),
    ("pool", "y_bn"): (0.259, 1.0),
    ("sgd", "mom"): (1.4e-05, 0.01), ("sgd", "shadow"): (0.237, 1.0), ("sgd", "w"): (1.0e-05, 0.01),
}


def conv_ops(case):
    return case.get("ops", ("fwd", "dgrad", "bnr", "wgrad"))


def bnr_forms(name):
    """The conv_dgrad_bnr forms a case runs: the dual form has no 8-wave instantiation, the halo
    kernel takes one BatchNorm, the dz fold a 1x1 stride-1 conv with K % 64 == 0 (and, on the stream,
    2*K < C), the sub-sampled residual a stride-1 DGRAD."""
    N, H, W, C, K, Rf, s, p = R.all_cases()[name]["shape"]
    forms = ["recompute", "tensor", "bits", "resid_bits"]
    if name in T.BNR_STREAM_CASES:
        forms = ["recompute", "bits", "dual_bits", "resid_bits", "resid_sub"] + (["fold"] if 2 * K < C else [])
    elif name not in ("igemm8_dgrad",):
        forms += ["dual_resid"]
        if s == 1:
            forms += ["resid_sub"]
    if name not in T.BNR_STREAM_CASES and Rf == 1 and s == 1 and K % 64 == 0:
        forms += ["fold"]
    return forms


BN_VARIANTS = [(mode, relu, acc) for mode in T.BN_MODES for relu in (False, True) for acc in (False, True)
               if not (mode == "none" and relu and acc)]
OPT_GS = [None, 0.5]


def collect_results(small_only=False):
    """{(op, output): [(got, truth, seg_dims), ...]} of ops/ref.py over every case (``small_only``
    leaves out the two halo cases)."""
    out = {}

    def upd(op, res):
        for n, v in res.items():
            out.setdefault((op, n), []).extend(R.chunks(v))

    for name, case in R.all_cases().items():
        if name in ("halo", "halo_s2d") and small_only:
            continue
        ops = conv_ops(case) if name in T.CONV_CASES else ("bnr",)
        if "fwd" in ops or "fwd_stats" in ops or "fwd_epi" in ops:
            upd("conv_fwd", R.run_conv_fwd(ref, name, stats="fwd_epi" not in ops, epi="fwd_stats" not in ops,
                                           res_only="fwd_res" in ops)[0])
        if "dgrad" in ops:
            upd("conv_dgrad", R.run_conv_dgrad(ref, name)[0])
        if "bnr" in ops:
            for form in bnr_forms(name):
                upd("conv_dgrad_bnr_fold" if form == "fold" else "conv_dgrad_bnr", R.run_conv_dgrad_bnr(ref, name, form)[0])
        if "bnr_halo" in ops:
            for form in ("recompute", "tensor"):
                upd("conv_dgrad_bnr", R.run_conv_dgrad_bnr(ref, name, form)[0])
        if "wgrad" in ops:
            upd("conv_wgrad", R.run_conv_wgrad(ref, name)[0])
    for name in T.WGRAD_CASES:
        op, res, _ = R.run_wgrad_case(ref, name)
        upd(op, res)
    for name in T.FWD_FOLD_CASES:
        upd("conv_fwd_fold", R.run_conv_fwd_fold(ref, name)[0])
    for M, fold in R.FUSED_SHAPES:
        upd("conv1x1_bwd_fused", R.run_bwd_fused(ref, M, fold)[0])
    for M, C in T.BN_SHAPES:
        for mode, relu, acc in BN_VARIANTS:
            upd(R.bn_op(M), R.run_bn(ref, M, C, mode, relu, acc)[0])
    for shape in T.POOL_SHAPES:
        upd("pool", R.run_pool(ref, shape)[0])
    for n in T.OPT_SIZES:
        for gs in OPT_GS:
            for v in range(len(R.SGD_VARIANTS)):
                upd("sgd", R.run_sgd(ref, n, v, gs, True)[0])
            for dec in (False, True):
                upd("adam", R.run_adam(ref, n, dec, gs, True)[0])
        for dec in (False, True):
            upd("adam", R.run_adam_late(ref, n, dec)[0])
        for v in R.clip_variants(n):
            upd("clip", R.run_clip(ref, n, v)[0])
    return out


def measure_floors():
    return {key: max([float(T.norm_err(a, t, s).max()) for a, t, s in v if a.numel()], default=0.0)
            for key, v in collect_results().items()}


# ------------------------------------------------------------------------------ tests
def test_reference_floors():
    fl = measure_floors()
    print({k: float("%.3g" % v) for k, v in fl.items()})
    assert set(fl) == set(BOUNDS), set(fl) ^ set(BOUNDS)
    bad = []
    for key, f in fl.items():
        rec, k = BOUNDS[key]
        # the recorded floor is this measurement (summation order of the CPU BLAS may move it a little:
        # 10 % + 0.02 of a bf16 floor, half of an fp32 floor + 2e-6)
        if abs(f - rec) > (0.1 * rec + 0.02 if rec > 1e-4 else 0.5 * rec + 2e-6):
            bad.append((key, "floor moved", f, rec))
        # k is not chosen: 0.01 for a floor <= 1e-4, else 2 * floor rounded up to the next multiple of
        # 0.5 and at least 1 (which never exceeds max(1, 4 * floor))
        want = 0.01 if rec <= 1e-4 else max(1.0, math.ceil(4 * rec) / 2)
        if k != want or (f <= 1e-4) != (rec <= 1e-4) or (f > 1e-4 and not (2 * f <= k <= max(1.0, 4 * f))):
            bad.append((key, "k must be the rule's value for the floor", f, rec, k, want))
    assert not bad, bad


def _near_zero(pre, terms):
    return int((pre.abs() < 1e-5 * terms).sum())


def test_input_conditions():
    """No ReLU and no recomputed mask within fp32 rounding of zero (min |pre| >= 1e-5 * sum |terms|), no
    pooling window tied at a positive maximum, no truth segment identically zero -- for every
    committed case, so that no test has to leave an element out."""
    for name, case in R.all_cases().items():
        d = T.conv_inputs(name)
        N, H, W, C, K, Rf, s, p = case["shape"]
        ops = conv_ops(case) if name in T.CONV_CASES else ("bnr",)
        if "fwd" in ops or "fwd_epi" in ops:
            pre = T.conv_truth(name, "fwd_epi")["pre"]
            terms = T.conv(d["xq"].abs(), d["wq"].abs(), s, p, d["biasq"].abs(), d["residq"].abs())["pre"]
            assert _near_zero(pre, terms) == 0, name
        if "fwd_res" in ops:
            pre = T.conv_truth(name, "fwd_res")["pre"]
            terms = T.conv(d["xq"].abs(), d["wq"].abs(), s, p, None, d["residq_odd"].abs())["pre"]
            assert _near_zero(pre, terms) == 0, name
        if "bnr" in ops or "bnr_halo" in ops:
            a, b = d["bx"].double() * d["msc"].double(), d["msh"].double().expand(d["bx"].shape)
            assert _near_zero(a + b, a.abs() + b.abs()) == 0, name
    for M, fold in R.FUSED_SHAPES:
        d = R.fused_case(M, fold)
        a, b = d["z"].double() * d["scale"].double(), d["shift"].double().expand(d["z"].shape)
        assert _near_zero(a + b, a.abs() + b.abs()) == 0, (M, fold)
    for name in T.FWD_FOLD_CASES:
        d = T.fwd_fold_inputs(name)
        a, b = d["z"].double() * d["scale"].double(), d["shift"].double().expand(d["z"].shape)
        assert _near_zero(a + b, a.abs() + b.abs()) == 0, name
    for name in T.WGRAD_CASES:      # the activation fold's ReLU
        if T.WGRAD_CASES[name].get("fold") in ("act", "both"):
            d = T.wgrad_inputs(name)
            a, b = d["x"].double() * d["asc"].double(), d["ash"].double().expand(d["x"].shape)
            assert _near_zero(a + b, a.abs() + b.abs()) == 0, name
    for M, C in T.BN_SHAPES:
        for mode in T.BN_MODES:
            t = T.bn_case(M, C, mode, True)["truth"]
            assert _near_zero(t["pre"], t["terms"]) == 0, (M, C, mode)
    for shape in T.POOL_SHAPES:
        d = T.pool_case(shape)
        assert T.pool_ties(d["x"]) == 0 and T.pool_ties(T.prologue_bf16(d["x"], d["scale"], d["shift"])) == 0, shape
        a, b = d["x"].double() * d["scale"].double(), d["shift"].double().expand(d["x"].shape)
        assert _near_zero(a + b, a.abs() + b.abs()) == 0, shape


def test_no_truth_segment_is_zero():
    """Every segment of every truth has a non-zero element (a zero segment takes nothing but exact
    zeros and has no noise floor).  Stated exception: a channel of a ReLU'd or masked output (y_epi,
    g) of the 5-row Linear case, where the ReLU / mask can be off for all five rows, and the single-row
    BatchNorm cases -- there exact zeros are what any implementation must give.  The exact zeros inside segments (masked gradients,
    the odd pixels of the 1x1 stride-2 DGRAD) are asserted bitwise by the GPU tests."""
    zero = []
    for (op, n), chunks in collect_results(small_only=True).items():
        for a, t, seg in chunks:
            rows = t.numel() // max(1, t.abs().amax(dim=seg).numel())
            if not (t.numel() and bool((t.abs().amax(dim=seg) == 0).any())) or (n in ("y_epi", "g") and rows <= 5):
                continue
            if op in ("bn", "bn_one_row") and (rows == 1 or n in ("dgamma", "dgamma2", "bwd_part", "bwd_part2")):
                # the single-row BatchNorm: a channel is one element (ReLU'd y, masked dx2), and xhat = 0
                # makes dgamma and sum g*xhat exactly zero -- in the truth and in any implementation
                assert n in ("y", "dx2") or float(t.reshape(-1, t.shape[-1])[-1].abs().max()) == 0.0
                continue
            zero.append((op, n, tuple(t.shape)))
    assert not zero, zero


def old_close(a, b, rtol=2e-2, atol=2e-2):
    """The whole-tensor bound of tests/test_kernels_gpu.py."""
    a, b = a.float(), b.float()
    return (a - b).abs().max().item() <= atol + rtol * b.abs().max().item()


def _rejects(a, t, seg, k):
    with pytest.raises(AssertionError):
        T.assert_elementwise(a, t, seg, k)


def test_comparator_rejects_image_defects():
    """Five synthetic defects on copies of truth tensors, each rejected at the k of its output; the
    first three are accepted by the whole-tensor ``close()`` of tests/test_kernels_gpu.py at the
    tolerances it is called with there (a, b: the large-shape tests' rtol 1e-2 / atol 1e-1 for dw and
    rtol 2e-2 / atol 5e-1 for the statistics; c: test_bn_forward_backward's 1e-2 / 1e-1)."""
    # a. one border tap of dw dropped: the product of one output pixel (image 0, p = q = 1) with the
    #    corner input pixel it reads through tap (0, 0), on the layer-1 3x3 shape of the halo case
    #    (59584 reduction rows)
    d = T.conv_inputs("halo")
    dw = T.conv(d["x"], d["w"], 1, 1, dy=d["dy"])["dw"]
    T.assert_elementwise(dw.clone(), dw, T.seg_k(dw)[1], BOUNDS[("conv_wgrad", "dw")][1])
    v = dw.clone()
    v[:, 0, 0, :] -= d["dy"][0, 1, 1, :].double().view(-1, 1) * d["x"][0, 0, 0, :].double().view(1, -1)
    _rejects(v, dw, T.seg_k(dw)[1], BOUNDS[("conv_wgrad", "dw")][1])
    assert old_close(v, dw, 1e-2, 1e-1)
    # b. one 16-row tile tail missing from the statistics of that shape's y
    y = T.conv_truth("halo", "fwd")["y"]
    st = T.stats_of(y)
    v = st - T.stats_of(y.reshape(-1, y.shape[-1])[-16:])
    _rejects(v, st, (1,), BOUNDS[("conv_fwd", "stats")][1])
    assert old_close(v, st, 2e-2, 5e-1)
    # c. one channel's dgamma scaled by 1.05 (the channel at the lower quartile of magnitude)
    t = T.bn_case(2040, 64, "none", True)["truth"]["dgamma"]
    v = t.clone()
    v[int(t.abs().argsort()[t.numel() // 4])] *= 1.05
    _rejects(v, t, (0,), BOUNDS[("bn", "dgamma")][1])
    assert old_close(v, t, 1e-2, 1e-1)
    # d. one sub-pixel class of a stride-2 dx shifted by a pixel
    dx = T.conv_truth("s2", "dx")
    v = dx.clone()
    v[:, 1::2, 1::2] = torch.roll(dx[:, 1::2, 1::2], 1, 2)
    _rejects(v, dx, T.seg_ch(dx)[1], BOUNDS[("conv_dgrad", "dx")][1])
    # e. Adam's m2 left at its old value
    c = T.opt_case(4 * 257)
    steps = T.optimizer_steps("adam", c["w"], c["grads"], R.LR, None, betas=(0.9, 0.999), eps=1e-8, weight_decay=R.WD)
    _rejects(steps[0]["m2"], steps[1]["m2"], (0,), BOUNDS[("adam", "m2")][1])


def test_optimizer_mask_semantics():
    """``mask`` (unused by pcmp/optim.py) as the kernels implement it, pinned on the reference: a
    masked element keeps w under both optimizers; Adam also keeps its moments, while SGD's momentum
    buffer still advances (the asymmetry is historical: sgd_flat masks the update, adam_flat the
    whole element).  The GPU test asserts the same of the kernels."""
    check_masked(R.run_masked(ref, 4 * 257))


def check_masked(out):
    off = out["mask"] == 0
    assert bool(off.any()) and bool((~off).any())
    for k in ("sgd_w", "adam_w", "adam_m1", "adam_m2"):
        assert torch.equal(out[k][off], out[k + "_0"][off]), k
        assert not torch.equal(out[k][~off], out[k + "_0"][~off]), k
    assert bool((out["sgd_mom"][off] != out["sgd_mom_0"][off]).all()), "SGD's momentum advances under the mask"
    assert torch.equal(out["sgd_mom"], out["sgd_mom_free"]), "the mask does not enter SGD's momentum"
    for k in ("sgd_w", "adam_w", "adam_m1", "adam_m2"):
        assert torch.equal(out[k][~off], out[k + "_free"][~off]), k


if __name__ == "__main__":
    import time
    t0 = time.time()
    for k, v in sorted(measure_floors().items()):
        print(k, "%.3g" % v)
    print("seconds", time.time() - t0)
