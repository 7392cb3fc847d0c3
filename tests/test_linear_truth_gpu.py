"""The Linear GEMMs with the GELU / GELU' epilogues (``linear_gelu_fwd``, ``linear_dgrad_gelu``) and the
planned Linear DGRAD (``conv_dgrad`` through ``run_plan<MODE_DGRAD>``) against the fp64 truths of
``pcmp.ops.truth_linear``, element by element, at the smallest shapes that reach each kernel, held to
``BOUNDS`` of tests/test_linear_truth_cpu.py.  Every case first asserts the kernel it takes
(``torch.ops.pcmp.conv_kernel_choice``), then checks: random full-mantissa inputs within norm_err <= k;
grid inputs (every fp32 partial sum exact) bit for bit against the rounded fp64 truth, for u, dx and
dx + resid, whatever the kernel and the split count; g bitwise equal to the standalone GELU kernel on
the stored u; and every DGRAD form bitwise the same with a transposed weight passed in."""
import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import truth_linear as T, truth_linear_run as R

from test_linear_truth_cpu import BOUNDS

pytestmark = pytest.mark.gpu


def ops():
    return torch.ops.pcmp


def _run(gpu, name, case):
    """Tags first; then every launch of the case under its knobs; then the figures are printed, and only
    then anything about the outputs is asserted."""
    fs = T.forms(case)
    res, grid, raws, same = {}, {}, [], {}

    def wt_same(raw, raw_wt, what):
        for f in raw:
            same[f"{f}{what}: a transposed weight passed in changes nothing"] = torch.equal(raw[f], raw_wt[f])

    with R.knobs(ops(), case["knobs"]):
        for f in fs:
            assert R.tag(ops(), case, f) == case["tags"][f], (name, f)
        for g in ((False,) if T.is_tails(case) else (False, True)):
            what = " (grid)" if g else ""
            if "fwd" in fs:
                r, raw = R.run_fwd(ops(), case, gpu, grid=g)
                (grid if g else res).update(r)
                raws += raw
                same[f"g == gelu_fwd(u), bitwise{what}"] = torch.equal(raw[0], raw[2])
            if [f for f in fs if f != "fwd" and not (g and f == "du")]:   # (the grid has no du)
                r, raw, raw_wt = R.run_dgrad(ops(), case, gpu, grid=g)
                (grid if g else res).update(r)
                raws += list(raw.values())
                wt_same(raw, raw_wt, what)
    print("norm_err linear", name, {n: float("%.3g" % e) for n, e in R.worst(res).items()})
    diff = {n: int((a != t).sum()) for n, (a, t) in grid.items()}
    print("grid", name, "elements that differ from bf16(truth):", diff, "bitwise invariants broken:",
          [k for k, v in same.items() if not v])
    for t in raws:
        assert torch.isfinite(t.float()).all()
    for n, v in res.items():
        for a, t, s in R.chunks(v):
            T.assert_elementwise(a, t, s, BOUNDS[("linear", n)][1], f"linear {n} {name}")
    assert not any(diff.values()), f"{name}: grid inputs must give the rounded fp64 truth bit for bit: {diff}"
    assert all(same.values()), [k for k, v in same.items() if not v]


@pytest.mark.parametrize("name", list(T.STATIC_CASES))
def test_linear_static(gpu, name):
    """Static dispatch: the register-staged igemm_kernel at every tile on both tap walks,
    igemm_dma_kernel at 128x128 / 128x64 / 8-wave 256x256 with EPI_GELU, and FWD_SPLIT into
    splitk_epilogue_kernel with relu == 2."""
    _run(gpu, name, T.STATIC_CASES[name])


@pytest.mark.parametrize("name", list(T.SMALL_CASES))
def test_linear_plan_small_m(gpu, name):
    """The small-M plan's kinds 3 and 4, unsplit and with 4 splits reduced by splitk_epilogue_kernel
    (relu == 2).  Kind 6 refuses a GELU call: its tag must read plan/auto, and it is not run."""
    case = T.SMALL_REFUSED
    with R.knobs(ops(), case["knobs"]):
        assert R.tag(ops(), case, "fwd") == "plan/auto"
    _run(gpu, name, T.SMALL_CASES[name])


@pytest.mark.parametrize("name", list(T.LARGE_CASES))
def test_linear_plan_large_m(gpu, name):
    """run_plan in both modes for kinds 1, 2, 5, 9 and 10 with 1 and 3 splits (5 + 5 + 3 K-tiles):
    FWD + GELU, DGRAD plain, into a residual, and * GELU'."""
    _run(gpu, name, T.LARGE_CASES[name])


@pytest.mark.parametrize("name", list(T.TAILS_CASES))
def test_linear_tails(gpu, name):
    """Rows scaled by 1, 2, 4: |u| past the point where 1 + erf cancels and __expf underflows; judged
    per row."""
    _run(gpu, name, T.TAILS_CASES[name])
