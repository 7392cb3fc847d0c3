"""Runners shared by tests/test_linear_truth_cpu.py and tests/test_linear_truth_gpu.py: each evaluates
one case of ``ops/truth_linear.py`` with an implementation of the op set (``ops/ref.py`` on the CPU,
``torch.ops.pcmp`` on the GPU) and returns ``({output: (got, truth, seg_dims)}, raw outputs)``.  Inputs
go to ``dev``; everything is compared on the CPU, where the truths live."""
from __future__ import annotations

from . import truth_linear as T
from .truth_image_run import _ch, _cpu, check, chunks, knobs, to, worst  # noqa: F401  (re-exported for the tests)


def _seg(case):
    """Per channel, as the conv cases; the tails case per row (a saturated row on its own scale)."""
    if T.is_tails(case):
        return lambda a, t: (_cpu(a), t, T.seg_rows(t)[1])
    return _ch


def tag(impl, case, form):
    """conv_kernel_choice of one form of a case: the FWD of x [M, 1, 1, C] * w [N, 1, 1, C], or the DGRAD
    of the case's dshape."""
    mode, flags = T.TAG_FLAGS[form]
    M, C, N = case["shape"] if form == "fwd" else case["dshape"]
    return impl.conv_kernel_choice(mode, M, 1, 1, C, N, 1, 1, 0, flags)


def committed_tags(impl):
    """(what, committed tag, conv_kernel_choice now) for every tag the cases commit, each under its
    case's knobs, the refused small-M kind included."""
    out = []
    for name, case in {**T.ALL_CASES, "small_refused": T.SMALL_REFUSED}.items():
        with knobs(impl, case["knobs"]):
            out += [(f"{name} {form}", want, tag(impl, case, form)) for form, want in case["tags"].items()]
    return out


def _wt(w, dev):
    """The transposed weight [C, N] built on the host."""
    return w.t().contiguous().to(dev)


def run_fwd(impl, case, dev="cpu", grid=False):
    """linear_gelu_fwd -> ({"u", "g"} against the fp64 truths, [g, u, gelu_fwd(u)]): g must be bitwise what
    the standalone GELU kernel gives for the stored u (the epilogue's promise; the caller compares).
    ``grid``: the grid inputs -- (u, the fp64 truth rounded to bf16) for the bitwise comparison instead of
    a result triple."""
    tails = T.is_tails(case)
    d = T.fwd_inputs(case["shape"], tails)
    t = T.fwd_truth(case["shape"], tails, grid)
    x, w, bias = to(dev, *((d["xq"], d["wq"], d["biasq"]) if grid else (d["x"], d["w"], d["bias"])))
    g, u = impl.linear_gelu_fwd(x, w, bias)
    raw = [g, u, impl.gelu_fwd(u)]
    if grid:
        return {"u": (_cpu(u), t["u"].to(T.BF))}, raw
    seg = _seg(case)
    return {"u": seg(u, t["u"]), "g": seg(g, t["g"])}, raw


def _dgrad_call(impl, form, dy, w, resid, u_in, wt):
    M, N = dy.shape
    C = w.shape[1]
    if form == "du":
        return impl.linear_dgrad_gelu(dy, w, u_in, wt)
    r = resid.clone().view(M, 1, 1, C) if form == "dx_resid" else None
    wt4 = wt.view(C, 1, 1, N) if wt is not None else None
    return impl.conv_dgrad(dy.view(M, 1, 1, N), w.view(N, 1, 1, C), 1, 1, 1, 0, r, wt4).view(M, C)


def run_dgrad(impl, case, dev="cpu", grid=False):
    """The DGRAD forms of a case ("du", "dx", "dx_resid"), each with the transposed weight made per
    call and again with one passed in: returns (res, raw, raw with wt).  ``grid``: the grid inputs, dx
    and dx_resid only, as (got, bf16 of the fp64 truth) pairs."""
    tails = T.is_tails(case)
    d = T.dgrad_inputs(case["dshape"], tails)
    t = T.dgrad_truth(case["dshape"], tails, grid)
    fs = [f for f in T.forms(case) if f != "fwd" and not (grid and f == "du")]
    dy, w, resid, u_in = to(dev, *((d["dyq"], d["wq"], d["residq"], None) if grid else (d["dy"], d["w"], d["resid"], d["u_in"])))
    wt = _wt(d["wq"] if grid else d["w"], dev)
    raw = {f: _dgrad_call(impl, f, dy, w, resid, u_in, None) for f in fs}
    raw_wt = {f: _dgrad_call(impl, f, dy, w, resid, u_in, wt) for f in fs}
    if grid:
        return {f: (_cpu(raw[f]), t[f].to(T.BF)) for f in fs}, raw, raw_wt
    seg = _seg(case)
    return {f: seg(raw[f], t[f]) for f in fs}, raw, raw_wt
