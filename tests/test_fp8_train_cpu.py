"""The fp8 training matmul mode on the CPU (``ops/ref.py`` only): the E5M2 rule on planted values, and the
distance of the reference's DGRAD / WGRAD from fp64 -- on the operands it quantised (``gemm``: what the GPU GEMM
tests are held to) and on the unquantised operands (``mode``: the quantisation error, docs/PARITY.md).

``BOUNDS`` holds (floor of ``ops/ref.py``, bound k) per output, k by the rule of tests/test_image_truth_cpu.py:
0.01 for a floor <= 1e-4, otherwise 2 * floor rounded up to a multiple of 0.5, at least 1 and never above
max(1, 4 * floor).  Every output is judged per row (``norm_err`` segments of one row).
"""
import math

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import ref, truth as T

GEMM_CASES = [(32, 32, 32), (144, 144, 400), (272, 1040, 272)]     # (M, N, K)
BOUNDS = {("gemm", "gw"): (9.2e-06, 0.01), ("mode", "dx"): (16.6, 33.5), ("mode", "gw"): (16.4, 33.0)}
# per format: v / amax of a value that lands on a normal, on a subnormal tie and below half the smallest subnormal
EDGE = {0: (2.0 ** -12, 2.0 ** -16, 2.0 ** -19), 1: (2.0 ** -12, 2.0 ** -30, 2.0 ** -33)}


def planted(n, fmt):
    """[3, n] fp32: zeros; one non-zero, the maximum; amax 3 with the rest at the format's edges (EDGE), mixed signs."""
    a, b, c = EDGE[fmt]
    v = torch.zeros(3, n)
    v[1, 0] = -3.0
    v[2] = 3.0 * a
    v[2, 0], v[2, 3::4], v[2, 5::4] = 3.0, -3.0 * b, 3.0 * c
    return v


def gemm_case(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    return (torch.randn(M, K, generator=g).bfloat16(), torch.randn(N, K, generator=g) * 0.05,
            torch.randn(M, N, generator=g).bfloat16())


def ref_backward(x, w, dy):
    """(dx, gw) of ops/ref.py and the quantised operands they came from."""
    dyq, sdy, dytq, sn = ref.fp8_quant_both(dy, 1)
    wtq, swt = ref.fp8_quant_cols(w, 0)
    xtq, sk = ref.fp8_quant_cols(x, 0)
    gw = torch.empty(w.shape)
    ref.linear_fp8_wgrad(dytq, sn, xtq, sk, gw, False)
    return ref.linear_fp8_dgrad(dyq, sdy, wtq, swt), gw, (dyq, sdy, wtq, swt, dytq, sn, xtq, sk)


def scaled(q, s):
    return q.double() * s.double()[:, None]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_e5m2_rule(dtype):
    vals = torch.arange(256, dtype=torch.uint8).view(torch.float8_e5m2).double()
    vals = vals[vals.isfinite()].unique()
    v = planted(16, 1).to(dtype)
    v[2, 1] = 3.0 - 2.0 ** -6                      # just below amax: rounds up to the largest value, not past it
    qT, s = ref.fp8_quant_cols(v.t().contiguous(), 1)
    q, s_row = ref.fp8_quant_rows(v, 1)
    assert qT.dtype == torch.float8_e5m2 and torch.equal(qT.view(torch.uint8), q.view(torch.uint8))
    assert torch.equal(s.view(torch.int32), s_row.view(torch.int32))
    amax, top = v.float().abs().amax(1), torch.full((3,), 57344.0)
    assert torch.equal(s.view(torch.int32), torch.where(amax > 0, amax / top, torch.ones(3)).view(torch.int32))
    t = (v.float() * torch.where(amax > 0, top / amax.clamp_min(1e-30), torch.zeros(3))[:, None]).double()
    dist = (t[..., None] - vals).abs()
    best, got = dist.amin(-1), q.double()
    assert bool(got.isfinite().all()) and torch.equal((got - t).abs(), best), "decoded q is a nearest e5m2 value"
    tie = (dist == best[..., None]).sum(-1) > 1
    assert bool(tie[2, 3]) and bool(((q.view(torch.uint8) & 1) == 0)[tie].all()), "ties go to the even code"
    assert got[0].abs().max() == 0 and got[1, 0] == -57344 and got[1, 1:].abs().max() == 0
    assert got[2, 0] == 57344 and got[2, 1] == 57344 and got[2, 2] == 14 and got[2, 3] == -2.0 ** -14 and got[2, 5] == 0


def test_reference_floors():
    """The floors of BOUNDS, recomputed, and the rule that turns each into its k."""
    fl = {key: 0.0 for key in BOUNDS}
    for M, N, K in GEMM_CASES:
        x, w, dy = gemm_case(M, N, K)
        dx, gw, (dyq, sdy, wtq, swt, dytq, sn, xtq, sk) = ref_backward(x, w, dy)
        exact = {"dx": scaled(dyq, sdy) @ scaled(wtq, swt).t(), "gw": scaled(dytq, sn) @ scaled(xtq, sk).t()}
        plain = {"dx": dy.double() @ w.double(), "gw": dy.double().t() @ x.double()}
        for kind, truth in (("gemm", exact), ("mode", plain)):
            for n, a in (("dx", dx), ("gw", gw)):
                if (kind, n) in fl:
                    fl[(kind, n)] = max(fl[(kind, n)], float(T.norm_err(a, truth[n], (1,)).max()))
    print({k: float("%.3g" % v) for k, v in fl.items()})
    bad = []
    for key, f in fl.items():
        rec, k = BOUNDS[key]
        if abs(f - rec) > 0.1 * rec + 0.02:   # (the summation order of the CPU BLAS may move it a little)
            bad.append((key, "floor moved", f, rec))
        want = 0.01 if rec <= 1e-4 else max(1.0, math.ceil(4 * rec) / 2)
        if k != want or (f <= 1e-4) != (rec <= 1e-4) or (f > 1e-4 and not (2 * f <= k <= max(1.0, 4 * f))):
            bad.append((key, "k must be the rule's value for the floor", f, rec, k, want))
    assert not bad, bad
