"""The loss-head kernels (csrc/elementwise.hip: xent_kernel, loss_mean_kernel, xent_grad_scale_kernel,
log_softmax_bwd_kernel, colsum_partial_kernel + col_reduce_kernel), fp32 and bf16, against the fp64
truths of ``pcmp.ops.truth_loss`` -- the cases tests/test_loss_truth_cpu.py puts ``ops/ref.py`` through,
held to its ``BOUNDS_LOSS``.  Rows without a valid label must be exact zeros, every output is finite, and
two runs are bitwise equal."""
import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import truth_loss as L

from test_loss_truth_cpu import BOUNDS_LOSS, _sfx

pytestmark = pytest.mark.gpu
F32, BF = L.F32, L.BF
DTYPES = [pytest.param(F32, id="fp32"), pytest.param(BF, id="bf16")]


def ops():
    return torch.ops.pcmp


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x, y), "run-to-run bitwise equality"


def _finite(ts):
    for t in ts:
        assert torch.isfinite(t.float()).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", L.XENT_V)
@pytest.mark.parametrize("B", L.XENT_B)
def test_softmax_xent(gpu, B, V, dtype):
    """Every grad_scale, label vector (mixed valid / ignored / out of range, all ignored, None) and
    want_logp / want_grad combination; at B = 1 every row kind."""
    for k0, gs, lk, wl, wg in L.xent_variants(B):
        res, zero, raw = L.run_xent(ops(), B, V, dtype, gs, lk, wl, wg, gpu, k0)
        _same(raw, L.run_xent(ops(), B, V, dtype, gs, lk, wl, wg, gpu, k0)[2])
        _finite(raw)
        for z in zero:
            assert float(z.float().abs().max() if z.numel() else 0.0) == 0.0, "a row without a valid label"
        L.check(BOUNDS_LOSS, L.xent_op(dtype), res, f"B={B} V={V} {k0} gs={gs:.3g} {lk} logp={wl} grad={wg}")


@pytest.mark.parametrize("B", L.LOSS_MEAN_B)
def test_loss_mean(gpu, B):
    """The mean over the valid rows and their exact count on both sides of the 256-thread loop; an
    all-ignored batch gives [0, 0]."""
    res, got, want, raw = L.run_loss_mean(ops(), B, False, gpu)
    assert got == want > 0
    L.check(BOUNDS_LOSS, "loss_mean", res, f"B={B}")
    _same(raw, L.run_loss_mean(ops(), B, False, gpu)[3])
    _, got, want, raw = L.run_loss_mean(ops(), B, True, gpu)
    assert got == want == 0.0 and float(raw[0][0]) == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_xent_grad_scale(gpu, dtype):
    """valid = 0 divides by 1; n below, at and off a multiple of the 256-thread block."""
    for n in L.GRAD_SCALE_N:
        for valid in (0, 1, 29):
            res, raw = L.run_grad_scale(ops(), n, dtype, valid, gpu)
            _finite(raw)
            L.check(BOUNDS_LOSS, "xent_grad_scale" + _sfx(dtype), res, f"n={n} valid={valid}")
            _same(raw, L.run_grad_scale(ops(), n, dtype, valid, gpu)[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,V", L.LSM_BWD_SHAPES)
def test_log_softmax_bwd(gpu, B, V, dtype):
    res, raw, _ = L.run_lsm_bwd(ops(), B, V, dtype, gpu)
    _finite(raw)
    L.check(BOUNDS_LOSS, "log_softmax_bwd" + _sfx(dtype), res, f"B={B} V={V}")
    _same(raw, L.run_lsm_bwd(ops(), B, V, dtype, gpu)[1])
    if dtype == F32:   # g on a grid, every row summing to exactly zero: dz is g bitwise
        _, raw, g = L.run_lsm_bwd(ops(), B, V, F32, gpu, grid=True)
        assert torch.equal(raw[0].cpu(), g)


@pytest.mark.parametrize("M,C", L.COLSUM_SHAPES)
def test_colsum_bf16(gpu, M, C):
    res, raw = L.run_colsum(ops(), M, C, gpu)
    _finite(raw)
    L.check(BOUNDS_LOSS, "colsum_bf16", res, f"{(M, C)}")
    _same(raw, L.run_colsum(ops(), M, C, gpu)[1])
