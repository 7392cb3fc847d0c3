"""Runners shared by tests/test_image_truth_f32_cpu.py and tests/test_image_truth_f32_gpu.py: each
evaluates one case of ``ops/truth_image_f32.py`` with an implementation of the op set (``ops/ref.py`` in
fp32 on the CPU, ``torch.ops.pcmp`` on the GPU).  A runner returns ``(exact, res, raw)``: ``exact`` maps
an output to ``(got, truth cast to fp32)`` and must be ``torch.equal``; ``res`` maps an output to
``(got, truth, seg_dims)`` chunks held to ``seg_rel``; ``raw`` are the implementation's tensors (run-to-run
equality, finiteness).  Everything is compared on the CPU, where the truths live."""
from __future__ import annotations

import torch

from . import ref
from . import truth_image as T
from . import truth_image_f32 as TF
from .truth import seg_rel
from .truth_image_run import _all, _ch, _cpu, _rows, chunks, knobs, to  # noqa: F401  (re-exported)

F32 = torch.float32
# mode and flags of torch.ops.pcmp.conv_f32_plan per tag key
TAG_MODE = {"fwd": (0, 0), "fwd_fold": (0, 1), "dgrad": (1, 0), "wgrad": (2, 0), "wgrad_fold": (2, 1)}


def tag(impl, case, key):
    mode, flags = TAG_MODE[key]
    return impl.conv_f32_plan(mode, *case["shape"], flags)


def committed_tags(impl):
    """(what, committed tag, conv_f32_plan now) for every tag of F32_CONV_CASES, each under its case's knobs."""
    out = []
    for name, case in TF.F32_CONV_CASES.items():
        with knobs(impl, case["knobs"]):
            out += [(f"{name} {key}", want, tag(impl, case, key)) for key, want in case["tags"].items()]
    return out


# ------------------------------------------------------------------------------ comparators
def worst_rel(res):
    return {n: max([float(seg_rel(a, t, s).max()) for a, t, s in chunks(v) if a.numel()], default=0.0)
            for n, v in res.items()}


def check_rel(bounds, op, res, what=""):
    """Every segment of every output of one case below its bound bounds[(op, output)][1]; the worst seg_rel
    per output is printed first, so a failing run still reports its figures."""
    w = worst_rel(res)
    print("seg_rel", op, what, {n: float("%.3g" % e) for n, e in w.items()})
    for n, e in w.items():
        assert e < bounds[(op, n)][1], f"{op} {n} {what}: seg_rel {e:.3g} >= {bounds[(op, n)][1]:g}"
    return w


def check_exact(exact, what=""):
    for n, (a, t) in exact.items():
        a, t = _cpu(a), t.to(F32)
        assert a.dtype == F32 and a.shape == t.shape, (what, n, a.dtype, tuple(a.shape), tuple(t.shape))
        if not torch.equal(a, t):
            bad = a != t
            idx = tuple(int(i) for i in torch.nonzero(bad)[0])
            raise AssertionError(f"{what} {n}: {int(bad.sum())} of {a.numel()} elements differ from the fp64 truth "
                                 f"(first at {idx}: got {float(a[idx])!r}, truth {float(t[idx])!r})")


def row_chunks(part, rows_per, sums):
    """The statistics partials ``part`` [T, 2, C] row by row: row t against ``sums(r0, r1)``, the fp64 [2, C]
    sums over rows [r0, r1) of the implementation's own output.  ``rows_per`` None: one row covers all."""
    part = _cpu(part)
    if rows_per is None:
        assert part.shape[0] == 1, tuple(part.shape)
        return [(part[0], sums(0, None), (1,))]
    return [(part[t], sums(t * rows_per, (t + 1) * rows_per), (1,)) for t in range(part.shape[0])]


def _stats_rows(part, y, rows_per):
    yr = _cpu(y).reshape(-1, y.shape[-1])
    return row_chunks(part, rows_per, lambda a, b: T.stats_of(yr[a:b]))


def _bnr_rows(part, g, x, mean, invstd, rows_per):
    C = x.shape[-1]
    gr, xr = _cpu(g).reshape(-1, C), x.reshape(-1, C)
    return row_chunks(part, rows_per, lambda a, b: T.bnr_sums(gr[a:b], xr[a:b], mean, invstd))


def expected_part_rows(gm, rows_per):
    return -(-gm // rows_per)


# ------------------------------------------------------------------------------ convolution
def run_conv_fwd(impl, shape, dev="cpu", rows_per=None):
    """Exact: bias + residual + ReLU on the grids.  Random: y with statistics, row by row."""
    N, H, W, C, K, R, s, p = shape
    d = TF.conv_inputs(shape)
    x, w, xq, wq, bias, resid = to(dev, d["x"], d["w"], d["xq"], d["wq"], d["biasq"], d["residq"])
    y2 = impl.conv_fwd(xq, wq, s, p, bias, resid, True, False)[0]
    y, st = impl.conv_fwd(x, w, s, p, None, None, False, True)
    exact = {"y_epi": (y2, TF.conv_truth(shape, "y_epi"))}
    res = {"y": _ch(y, TF.conv_truth(shape, "y")), "stats": _stats_rows(st, y, rows_per)}
    return exact, res, [y2, y, st]


def run_conv_fwd_fold(impl, shape, dev="cpu", rows_per=None):
    """conv_fwd behind the input fold (in_scale / in_shift) with statistics: exact on the grids (the
    padding ring must stay zero), random with the statistics row by row."""
    N, H, W, C, K, R, s, p = shape
    d = TF.conv_inputs(shape)
    zq, wq, fsc, fsh, z, w, asc, ash = to(dev, d["zq"], d["wq"], d["fsc"], d["fsh"], d["z"], d["w"], d["asc"], d["ash"])
    yq, stq = impl.conv_fwd(zq, wq, s, p, None, None, False, True, fsc, fsh)
    y, st = impl.conv_fwd(z, w, s, p, None, None, False, True, asc, ash)
    exact = {"y_fold": (yq, TF.conv_truth(shape, "y_fold_q"))}
    res = {"y": _ch(y, TF.conv_truth(shape, "y_fold")),
           "stats": _stats_rows(stq, yq, rows_per) + _stats_rows(st, y, rows_per)}
    return exact, res, [yq, stq, y, st]


def run_conv_dgrad(impl, shape, dev="cpu"):
    """conv_dgrad plain and into a residual: exact on the grids, random."""
    N, H, W, C, K, R, s, p = shape
    d = TF.conv_inputs(shape)
    dyq, wq, dresq, dy, wd, dres = to(dev, d["dyq"], d["wq"], d["dresq"], d["dy"], d["wd"], d["dres"])
    dxq = impl.conv_dgrad(dyq, wq, H, W, s, p, None)
    dxrq = impl.conv_dgrad(dyq, wq, H, W, s, p, dresq.clone())
    dx = impl.conv_dgrad(dy, wd, H, W, s, p, None)
    dxr = impl.conv_dgrad(dy, wd, H, W, s, p, dres.clone())
    tq, t = TF.conv_truth(shape, "dx_q"), TF.conv_truth(shape, "dx")
    exact = {"dx": (dxq, tq), "dx_resid": (dxrq, tq + d["dresq"].double())}
    res = {"dx": _ch(dx, t), "dx_resid": _ch(dxr, t + d["dres"].double())}
    return exact, res, [dxq, dxrq, dx, dxr]


def _wgrad(impl, dy, x, dw0, shape, fold=(None, None)):
    N, H, W, C, K, R, s, p = shape
    out = torch.full((K, R, R, C), float("nan"), device=dy.device)
    impl.conv_wgrad(dy, x, out, R, R, s, p, False, None, None, *fold)
    acc = dw0.clone()
    impl.conv_wgrad(dy, x, acc, R, R, s, p, True, None, None, *fold)
    return out, acc


def run_conv_wgrad(impl, shape, dev="cpu", fold=False):
    """conv_wgrad written and accumulated onto a non-zero buffer: exact on the grids, random; ``fold``:
    behind the input fold (x stands for z)."""
    d = TF.conv_inputs(shape)
    xk, sk, hk, xqk = ("z", "asc", "ash", "zq") if fold else ("x", None, None, "xq")
    dyq, xq, dw0q, dy, x, dw0 = to(dev, d["dyq"], d[xqk], d["dw0q"], d["dy"], d[xk], d["dw0"])
    fq = tuple(to(dev, d["fsc"], d["fsh"])) if fold else (None, None)
    fr = tuple(to(dev, d[sk], d[hk])) if fold else (None, None)
    outq, accq = _wgrad(impl, dyq, xq, dw0q, shape, fq)
    out, acc = _wgrad(impl, dy, x, dw0, shape, fr)
    tq, t = TF.conv_truth(shape, "dw_fold_q" if fold else "dw_q"), TF.conv_truth(shape, "dw_fold" if fold else "dw")
    exact = {"dw": (outq, tq), "dw_acc": (accq, tq + d["dw0q"].double())}
    res = {"dw": _rows(out, t), "dw_acc": _rows(acc, t + d["dw0"].double())}
    return exact, res, [outq, accq, out, acc]


def bnr_mask(shape, form):
    d = TF.conv_inputs(shape)
    if T.BNR_FORMS[form]["mask"] == "recompute":
        return (d["bx"].double() * d["msc"].double() + d["msh"].double()) > 0
    return d["ymask"].double() > 0


def run_conv_dgrad_bnr(impl, shape, form, dev="cpu", rows_per=None):
    """conv_dgrad_bnr in one of TF.BNR_F32_FORMS on the random inputs: g against the masked fp64 dx
    (+ residual), part / part2 row by row against the fp64 sums of the implementation's own g.  Returns
    (res, raw, mask)."""
    N, H, W, C, K, R, s, p = shape
    f = T.BNR_FORMS[form]
    d = TF.conv_inputs(shape)
    resid = d["dres"] if f.get("resid") else None
    dual = f.get("dual", False)
    ymask = d["ymask"] if f["mask"] == "tensor" else None
    bits = ref.pack_mask_bits(d["ymask"]) if f["mask"] == "bits" else None
    msc, msh = (d["msc"], d["msh"]) if f["mask"] == "recompute" else (None, None)
    a = to(dev, d["dy"], d["wd"], resid, ymask, d["bx"], d["mean"], d["invstd"], d["bx2"] if dual else None,
           d["mean2"] if dual else None, d["invstd2"] if dual else None, msc, msh, bits)
    dy, wd, resid_d, ymask_d, bx, mean, invstd, bx2, mean2, invstd2, msc_d, msh_d, bits_d = a
    out = impl.conv_dgrad_bnr(dy, wd, H, W, s, p, resid_d.clone() if resid_d is not None else None, ymask_d, bx, mean,
                              invstd, bx2, mean2, invstd2, msc_d, msh_d, None, bits_d)
    assert len(out) == (3 if dual else 2)
    mask = bnr_mask(shape, form)
    t = TF.conv_truth(shape, "dx")
    if resid is not None:
        t = t + resid.double()
    t = torch.where(mask, t, torch.zeros_like(t))
    g = _cpu(out[0])
    res = {"g": _ch(g, t), "part": _bnr_rows(out[1], g, d["bx"], d["mean"], d["invstd"], rows_per)}
    if dual:
        res["part2"] = _bnr_rows(out[2], g, d["bx2"], d["mean2"], d["invstd2"], rows_per)
    return res, list(out), mask


# ------------------------------------------------------------------------------ element-wise ops
def run_dropout(impl, n, dev="cpu"):
    """(keep mask of the implementation, the reference RNG's, res) of dropout(p = 0.1) with a salt."""
    d = TF.ew_case(n)
    salt = torch.tensor([3], dtype=torch.int64)
    y = impl.dropout(d["x"].to(dev), TF.DROP_P, TF.DROP_SEED, TF.DROP_OFF, salt.to(dev))
    idx = torch.arange(n, dtype=torch.int64) + TF.DROP_OFF
    keep = ref.hash_uniform(ref._salted(TF.DROP_SEED, salt), idx) >= TF.DROP_P
    t = torch.where(keep, d["x"].double() / (1.0 - TF.DROP_P), torch.zeros((), dtype=torch.float64))
    return _cpu(y) != 0, keep, {"y": _all(y, t)}, [y]


def run_relu_bwd(impl, n, dev="cpu"):
    d = TF.ew_case(n)
    dx = impl.relu_bwd(d["dy"].to(dev), d["y"].to(dev))
    return {"dx": (dx, torch.where(d["y"] > 0, d["dy"], torch.zeros_like(d["dy"])).double())}, [dx]


def run_colsum(impl, M, C, dev="cpu"):
    d = TF.colsum_case(M, C)
    x = d["x"].to(dev)
    out = torch.full((C,), float("nan"), device=dev)
    impl.colsum(x, out, False)
    acc = d["out0"].clone().to(dev)
    impl.colsum(x, acc, True)
    t = d["x"].double().sum(0)
    return {"sum": _all(out, t), "sum_acc": _all(acc, t + d["out0"].double())}, [out, acc]


def run_pool_c6(impl, dev="cpu"):
    """maxpool_fwd / maxpool_bwd at C = 6 (the generic forward kernel), alone and behind the prologue:
    values, indices (against ``ops/ref.py`` on the fp64 values: no window ties) and dx."""
    shape = TF.POOL_C6
    N, H, W, C = shape
    d = T.pool_case(shape, F32)
    x, dy, scale, shift = to(dev, d["x"], d["dy"], d["scale"], d["shift"])
    y, idx = impl.maxpool_fwd(x, 3, 2, 1, True)
    dx = impl.maxpool_bwd(dy, idx, H, W, 3, 2, 1)
    y2, idx2 = impl.maxpool_fwd(x, 3, 2, 1, True, scale, shift)
    dx2 = impl.maxpool_bwd(dy, idx2, H, W, 3, 2, 1)
    t, t2 = T.maxpool(d["x"], d["dy"]), T.maxpool(d["x"], d["dy"], d["scale"], d["shift"])
    ti = ref.maxpool_fwd(d["x"].double(), 3, 2, 1, True)[1]
    ti2 = ref.maxpool_fwd(d["x"].double(), 3, 2, 1, True, d["scale"].double(), d["shift"].double())[1]
    exact = {"y": (y, t["y"]), "y_bn": (y2, t2["y"])}
    res = {"dx": _ch(dx, t["dx"]), "dx_bn": _ch(dx2, t2["dx"])}
    return exact, res, [y, idx, dx, y2, idx2, dx2], (ti, ti2)


def pool_truth_idx(shape):
    """The window argmax of a pooling case, alone and behind the prologue (``ops/ref.py`` on fp64 values)."""
    d = T.pool_case(shape, F32)
    return (ref.maxpool_fwd(d["x"].double(), 3, 2, 1, True)[1],
            ref.maxpool_fwd(d["x"].double(), 3, 2, 1, True, d["scale"].double(), d["shift"].double())[1])
