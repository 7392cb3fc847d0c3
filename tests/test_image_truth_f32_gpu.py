"""The fp32 image path (csrc/f32.hip: the fp32 convolutions, BatchNorm, pooling and element-wise kernels
of ``--dtype fp32``) against the fp64 autograd truths of ``pcmp.ops.truth_image``, through the runners
of ``pcmp.ops.truth_image_f32_run`` (the same cases tests/test_image_truth_f32_cpu.py puts ``ops/ref.py``
through).  Every conv case first asserts its launch plan (``torch.ops.pcmp.conv_f32_plan``); its grid
inputs must then give the fp64 truth *bit for bit* in every tile shape and split count, and its random
fp32 inputs stay below ``seg_rel`` 1e-5 per channel / output-channel row / statistics row
(``BOUNDS_F32``), the statistics partials compared row by row with the row count the tag implies.  Every
run is done twice and compared with ``torch.equal``; every output is finite."""
import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import ref, truth_image as T, truth_image_f32 as TF, truth_image_f32_run as RF, truth_image_run as R

from test_image_truth_cpu import BN_VARIANTS
from test_image_truth_f32_cpu import BOUNDS_F32

pytestmark = pytest.mark.gpu
F32 = torch.float32


def ops():
    return torch.ops.pcmp


def knobs(kn):
    return R.knobs(ops(), kn)


def _finite(ts):
    for t in ts:
        if t is not None and t.is_floating_point():
            assert torch.isfinite(t).all()


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y), "run-to-run bitwise equality"


# ------------------------------------------------------------------------------ convolution
@pytest.mark.parametrize("name", list(TF.F32_CONV_CASES))
def test_conv(gpu, name):
    """Every op the case commits a tag for: FWD (bias + residual + ReLU exact; y and the statistics rows),
    FWD and WGRAD behind the input fold, DGRAD plain and into a residual, WGRAD written and accumulated."""
    case = TF.F32_CONV_CASES[name]
    shape, tags = case["shape"], case["tags"]
    with knobs(case["knobs"]):
        for key, want in tags.items():
            assert RF.tag(ops(), case, key) == want, key
            gm = TF.gemm_dims(shape, RF.TAG_MODE[key][0])[0]
            rows_per = TF.stat_rows_per(want)
            if key == "fwd":
                op, run = "conv_fwd", lambda: RF.run_conv_fwd(ops(), shape, gpu, rows_per)
            elif key == "fwd_fold":
                op, run = "conv_fwd_fold", lambda: RF.run_conv_fwd_fold(ops(), shape, gpu, rows_per)
            elif key == "dgrad":
                op, run = "conv_dgrad", lambda: RF.run_conv_dgrad(ops(), shape, gpu)
            else:
                op, run = ("conv_wgrad_fold" if key == "wgrad_fold" else "conv_wgrad"), \
                    lambda: RF.run_conv_wgrad(ops(), shape, gpu, fold=key == "wgrad_fold")  # noqa: B023
            exact, res, raw = run()
            _same(raw, run()[2])
            _finite(raw)
            if key == "fwd":
                assert raw[2].shape[0] == RF.expected_part_rows(gm, rows_per), (want, tuple(raw[2].shape))
            if key == "fwd_fold":
                for st in (raw[1], raw[3]):
                    assert st.shape[0] == RF.expected_part_rows(gm, rows_per), (want, tuple(st.shape))
            RF.check_exact(exact, f"{name} {key} {want}")
            RF.check_rel(BOUNDS_F32, op, res, f"{name} {key} {want}")
            if name == "down" and key == "dgrad":   # 1x1 stride 2: no tap reaches an odd pixel
                d = TF.conv_inputs(shape)
                for dx, dres in ((raw[0], d["dresq"]), (raw[2], d["dres"])):
                    assert float(dx[:, 1::2].abs().max()) == 0.0 and float(dx[:, :, 1::2].abs().max()) == 0.0
                for dxr, dres in ((raw[1], d["dresq"]), (raw[3], d["dres"])):
                    assert torch.equal(dxr[:, 1::2].cpu(), dres[:, 1::2]) and torch.equal(dxr[:, :, 1::2].cpu(), dres[:, :, 1::2])


@pytest.mark.parametrize("name", TF.BNR_F32_CASES)
def test_conv_dgrad_bnr(gpu, name):
    """conv_dgrad_bnr in fp32: the mask as tensor, as bits and recomputed, one and two BatchNorms, with and
    without the residual; g exactly 0 where the mask is off; the bit-mask results bitwise the tensor-mask
    ones; part / part2 row by row.  The sub-sampled residual and the dz fold are bf16 only."""
    case = TF.F32_CONV_CASES[name]
    shape = case["shape"]
    N, H, W, C, K, Rf, s, p = shape
    rows_per = TF.reduce_rows_per(N * H * W)
    got = {}
    with knobs(case["knobs"]):
        assert RF.tag(ops(), case, "dgrad") == case["tags"]["dgrad"]
        for form in TF.BNR_F32_FORMS:
            res, raw, mask = RF.run_conv_dgrad_bnr(ops(), shape, form, gpu, rows_per)
            _same(raw, RF.run_conv_dgrad_bnr(ops(), shape, form, gpu, rows_per)[1])
            _finite(raw)
            for part in raw[1:]:
                assert tuple(part.shape) == (RF.expected_part_rows(N * H * W, rows_per), 2, C), tuple(part.shape)
            RF.check_rel(BOUNDS_F32, "conv_dgrad_bnr", res, f"{name} {form}")
            g = raw[0].cpu()
            assert bool((~mask).any()) and float(g[~mask].abs().max()) == 0.0, "g where the mask is off"
            got[form] = raw
        for a, b in zip(got["tensor"], got["bits"]):
            assert torch.equal(a, b), "the bit mask gives exactly the tensor-mask result"
        d = TF.conv_inputs(shape)
        a = R.to(gpu, d["dy"], d["wd"], d["dres"][:, ::2, ::2].contiguous(), d["bx"], d["mean"], d["invstd"], d["msc"],
                 d["msh"], d["dy"], torch.ones(3, K))
        with pytest.raises(RuntimeError, match="sub-sampled residual is bf16 only"):
            ops().conv_dgrad_bnr(a[0], a[1], H, W, s, p, a[2], None, a[3], a[4], a[5], None, None, None, a[6], a[7], None,
                                 None, None, None, True)
        with pytest.raises(RuntimeError, match="fold is bf16 only"):
            ops().conv_dgrad_bnr(a[0], a[1], H, W, s, p, None, None, a[3], a[4], a[5], None, None, None, a[6], a[7], None,
                                 None, a[8], a[9], False)


# ------------------------------------------------------------------------------ BatchNorm
@pytest.mark.parametrize("M,C", T.BN_SHAPES)
def test_batchnorm_chain(gpu, M, C):
    """Every x2 mode / ReLU / accumulate variant in fp32.  The mask bits are bitwise pack_mask_bits of the
    kernel's own y, y does not depend on whether they are asked for, and bn_partials' rows -- ceil(M /
    rows_per) of them: 8 at M = 2040, one at M = 1 -- are each the sums of their own rows of x."""
    for mode, relu, acc in BN_VARIANTS:
        res, raw = R.run_bn(ops(), M, C, mode, relu, acc, gpu, mbits=True, dtype=F32)
        _, raw2 = R.run_bn(ops(), M, C, mode, relu, acc, gpu, mbits=False, dtype=F32)
        outs = [raw["y"], *raw["outs"], *raw["stats"]]
        assert all(t.dtype == F32 for t in outs)
        _finite(outs)
        RF.check_rel(BOUNDS_F32, R.bn_op(M), res, f"{(M, C)} {mode} relu={relu} acc={acc}")
        assert torch.equal(raw["mbits"], ref.pack_mask_bits(raw["y"])), "mask bits of the kernel's own y"
        _same(outs, [raw2["y"], *raw2["outs"], *raw2["stats"]])
        if relu:
            off = raw["y"] <= 0
            assert float(raw["outs"][-1][off].abs().max() if off.any() else 0.0) == 0.0, "g where y is off"
    x = T.bn_case(M, C, "none", False, F32)["x"]
    part = ops().bn_partials(x.to(gpu))
    rows_per = TF.reduce_rows_per(M)
    assert tuple(part.shape) == (RF.expected_part_rows(M, rows_per), 2, C)
    assert part.shape[0] == {2040: 8, 1: 1}.get(M, part.shape[0])
    RF.check_rel(BOUNDS_F32, R.bn_op(M), {"part": RF.row_chunks(part, rows_per, lambda a, b: T.stats_of(x[a:b]))}, f"{(M, C)} rows")


# ------------------------------------------------------------------------------ pooling
@pytest.mark.parametrize("shape", T.POOL_SHAPES)
def test_pooling(gpu, shape):
    """maxpool_fwd / maxpool_bwd alone and behind the BN + ReLU prologue, maxpool_bwd_bnr, GAP.  The window
    argmax equals the truth's wherever it is unique (no window of x ties; behind the prologue the windows
    whose maximum is 0 tie among their zeros, and their gradient is masked off)."""
    res, raw, mask = R.run_pool(ops(), shape, gpu, dtype=F32)
    _same([t for t in raw], [t for t in R.run_pool(ops(), shape, gpu, dtype=F32)[1]])
    _finite(raw)
    y, idx, dx, y2, idx2, g, part = raw
    assert all(t.dtype == F32 for t in (y, dx, y2, g, part))
    RF.check_rel(BOUNDS_F32, "pool", res, str(shape))
    d = T.pool_case(shape, F32)
    RF.check_exact({"y": (y, T.maxpool(d["x"])["y"]), "y_bn": (y2, T.maxpool(d["x"], None, d["scale"], d["shift"])["y"])})
    ti, ti2 = RF.pool_truth_idx(shape)
    assert torch.equal(idx.cpu(), ti), "argmax"
    on = (y2 > 0).cpu()
    assert bool(on.any()) and torch.equal(idx2.cpu()[on], ti2[on]), "argmax behind the prologue"
    assert bool((~mask).any()) and float(g.cpu()[~mask].abs().max()) == 0.0, "g where the prologue's ReLU is off"
    N, H, W, C = shape
    rows_per = TF.reduce_rows_per(N * H * W)
    assert tuple(part.shape) == (RF.expected_part_rows(N * H * W, rows_per), 2, C)
    RF.check_rel(BOUNDS_F32, "pool", {"part": RF._bnr_rows(part, g, d["x"], d["mean"], d["invstd"], rows_per)}, f"{shape} rows")


def test_pooling_c6(gpu):
    """C = 6 (C % 4 != 0): the generic maxpool_fwd_kernel.  Only maxpool_fwd / maxpool_bwd run there;
    maxpool_bwd_bnr refuses the channel count loudly."""
    exact, res, raw, (ti, ti2) = RF.run_pool_c6(ops(), gpu)
    _same(raw, RF.run_pool_c6(ops(), gpu)[2])
    _finite(raw)
    RF.check_exact(exact, "C = 6")
    RF.check_rel(BOUNDS_F32, "pool_c6", res)
    assert torch.equal(raw[1].cpu(), ti), "argmax"
    on = (raw[3] > 0).cpu()
    assert bool(on.any()) and torch.equal(raw[4].cpu()[on], ti2[on]), "argmax behind the prologue"
    d = T.pool_case(TF.POOL_C6, F32)
    a = R.to(gpu, d["dy"], d["x"], d["mean"], d["invstd"], d["scale"], d["shift"])
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops().maxpool_bwd_bnr(a[0], raw[4], a[1], a[2], a[3], a[4], a[5], 3, 2, 1)


# ------------------------------------------------------------------------------ element-wise
@pytest.mark.parametrize("n", TF.EW_SIZES)
def test_dropout_relu_bwd(gpu, n):
    """dropout: the keep mask is bitwise the reference RNG's (seed, 64-bit offset, salt), the kept values
    x / (1 - p) within 1e-6; the fp32 op takes any n (one element, with and without a multiple of 4, a
    second trip of the grid-stride loop).  relu_bwd: exact."""
    kept, keep, res, raw = RF.run_dropout(ops(), n, gpu)
    assert torch.equal(kept, keep), "keep mask"
    RF.check_rel(BOUNDS_F32, "dropout", res, f"n={n}")
    _same(raw, RF.run_dropout(ops(), n, gpu)[3])
    exact, raw = RF.run_relu_bwd(ops(), n, gpu)
    RF.check_exact(exact, f"relu_bwd n={n}")
    _same(raw, RF.run_relu_bwd(ops(), n, gpu)[1])


@pytest.mark.parametrize("M,C", TF.COLSUM_SHAPES)
def test_colsum(gpu, M, C):
    """fp32 column sums (bias gradients), written into a NaN-filled vector and accumulated onto a non-zero one."""
    res, raw = RF.run_colsum(ops(), M, C, gpu)
    _finite(raw)
    RF.check_rel(BOUNDS_F32, "colsum", res, f"{(M, C)}")
    _same(raw, RF.run_colsum(ops(), M, C, gpu)[1])
