"""Runners shared by tests/test_image_truth_cpu.py and tests/test_image_truth_gpu.py: each evaluates
one case of ``ops/truth_image.py`` with an implementation of the op set (``ops/ref.py`` on the CPU,
``torch.ops.pcmp`` on the GPU), forward and then backward on the forward's own saved outputs, and
returns ``({output: (got, truth, seg_dims)}, raw outputs)``.  Inputs go to ``dev``; everything is
compared on the CPU, where the truths live."""
from __future__ import annotations

import contextlib

import torch

from . import ref
from . import truth_image as T
from .truth_run import chunks, worst  # noqa: F401  (re-exported for the tests)


def to(dev, *ts):
    return [t.to(dev) if t is not None else None for t in ts]


def _cpu(t):
    return t.detach().cpu()


def _ch(a, t):      # per channel (last dimension)
    return _cpu(a), t, T.seg_ch(t)[1]


def _rows(a, t):    # per leading index: statistics rows [2, C], dw [K, ...]
    return _cpu(a), t, T.seg_k(t)[1]


def _all(a, t):
    a = _cpu(a).reshape(-1)
    return a, t.reshape(-1), (0,)


def check(bounds, op, res, what=""):
    """Every output of one case within its bound k = bounds[(op, output)][1] of the truth; the worst
    norm_err per output is printed first (three significant digits: the fp32 outputs sit near 1e-5),
    so a failing run still reports its figures."""
    print("norm_err", op, what, {n: float("%.3g" % e) for n, e in worst(res).items()})
    for n, v in res.items():
        for a, t, s in chunks(v):
            T.assert_elementwise(a, t, s, bounds[(op, n)][1], f"{op} {n} {what}")


def all_cases():
    return {**T.CONV_CASES, **T.BNR_STREAM_CASES}


# flags of torch.ops.pcmp.conv_kernel_choice per tag key of a case
TAG_FLAGS = {"fwd": (0, 1), "fwd_epi": (0, 2 | 4 | 8), "fwd_res": (0, 4 | 8), "dgrad": (1, 0), "bnr": (1, 1 | 32), "bnr_mask": (1, 1 | 8),
             "wgrad": (2, 0)}
WGRAD_FOLD_FLAGS = {None: 0, "dz": 1, "act": 2, "both": 3}


@contextlib.contextmanager
def knobs(impl, kn):
    """Set the knobs of a case; restore every one of them whatever happens."""
    old = {}
    try:
        for n, v in kn.items():
            old[n] = impl.set_knob(n, v)
        yield
    finally:
        for n, v in old.items():
            impl.set_knob(n, v)


def tag(impl, case, key, flags=None):
    """conv_kernel_choice of a conv case for one of its tag keys (TAG_FLAGS), or for explicit flags."""
    mode, fl = TAG_FLAGS[key]
    return impl.conv_kernel_choice(mode, *case["shape"], fl if flags is None else flags)


def bnr_tag(name, case, form):
    """The committed tag of a conv_dgrad_bnr form of a case."""
    N, H, W, C, K, Rf, s, p = case["shape"]
    if form == "fold" and name not in T.BNR_STREAM_CASES:
        return "fold/128x64" if C <= 64 else "fold/128x128"
    if name == "halo" and form != "recompute":
        return case["tags"]["bnr_mask"]
    return case["tags"]["bnr"]


def gemm_rows(shape, mode):
    """gm of each GEMM of a conv call: N*P*Q (FWD, mode 0); DGRAD (mode 1) N*H*W at stride 1 and, at
    stride 2, the sub-pixel classes some tap reaches, in launch order."""
    N, H, W, C, K, Rf, s, p = shape
    if mode == 0:
        P, Q = T.conv_shapes(shape)
        return [N * P * Q]
    if s == 1:
        return [N * H * W]
    cls = [((H - oph + 1) // 2, (W - opw + 1) // 2, (oph + p) & 1, (opw + p) & 1) for oph in (0, 1) for opw in (0, 1)]
    return [N * dH * dW for dH, dW, r0, s0 in cls if dH > 0 and dW > 0 and r0 < Rf and s0 < Rf]


def part_rows(tag_, shape, mode):
    """The partial-statistics rows of a call with the tag ``tag_``: one per BM-row tile of every GEMM
    ('+'-joined), BM read from the tag.  None for the streaming kernels (one row per workgroup group)."""
    tags = tag_.split("+")
    if tags[0].startswith(("fwd_stream/", "bnr_stream/")):
        return None
    gms = gemm_rows(shape, mode)
    assert len(tags) == len(gms), (tag_, gms)
    return sum(-(-gm // int(t.split("/")[1].split("x")[0])) for t, gm in zip(tags, gms))


def committed_tags(impl):
    """(what, committed tag, conv_kernel_choice now) for every tag the conv cases of truth_image.py
    commit, each under its case's knobs: what the GPU tests assert before they run a case."""
    out = []
    for name, case in T.CONV_CASES.items():
        with knobs(impl, case["knobs"]):
            out += [(f"{name} {key}", want, tag(impl, case, key)) for key, want in case["tags"].items()]
    for name, case in T.WGRAD_CASES.items():
        with knobs(impl, case["knobs"]):
            out.append((name, case["tags"], impl.conv_kernel_choice(2, *case["shape"], WGRAD_FOLD_FLAGS[case.get("fold")])))
    for name, case in T.FWD_FOLD_CASES.items():
        with knobs(impl, case["knobs"]):
            out.append((name, case["tags"], impl.conv_kernel_choice(0, *case["shape"], 1 | 16)))
    for name, case in T.BNR_STREAM_CASES.items():
        with knobs(impl, case["knobs"]):
            out += [(f"{name} {key}", want, tag(impl, case, key)) for key, want in case["tags"].items()]
    return out


# ------------------------------------------------------------------------------ convolution
def run_conv_fwd(impl, name, dev="cpu", stats=True, epi=True, res_only=False):
    """conv_fwd with statistics (y, and the partials against the fp64 sums of that y), with the
    bias + residual + ReLU epilogue (y_epi) and, ``res_only``, with residual + ReLU and no bias."""
    case = all_cases()[name]
    N, H, W, C, K, R, s, p = case["shape"]
    d = T.conv_inputs(name)
    x, w, xq, wq, bias, resid = to(dev, d["x"], d["w"], d["xq"], d["wq"], d["biasq"], d["residq"])
    res, raw = {}, []
    if stats:
        y, st = impl.conv_fwd(x, w, s, p, None, None, False, True)
        res["y"] = _ch(y, T.conv_truth(name, "fwd")["y"])
        res["stats"] = _rows(st.double().sum(0), T.stats_of(_cpu(y)))
        raw += [y, st]
    if epi:
        y2 = impl.conv_fwd(xq, wq, s, p, bias, resid, True, False)[0]
        res["y_epi"] = _ch(y2, T.conv_truth(name, "fwd_epi")["y"])
        raw.append(y2)
    if res_only:
        y3 = impl.conv_fwd(xq, wq, s, p, None, d["residq_odd"].to(dev), True, False)[0]
        res["y_epi"] = chunks(res.get("y_epi", [])) + [_ch(y3, T.conv_truth(name, "fwd_res")["y"])]
        raw.append(y3)
    return res, raw


def run_conv_fwd_fold(impl, name, dev="cpu"):
    """conv_fwd with statistics behind the BatchNorm-forward fold (a case of T.FWD_FOLD_CASES)."""
    N, H, W, C, K, R, s, p = T.FWD_FOLD_CASES[name]["shape"]
    d = T.fwd_fold_inputs(name)
    z, w, sc, sh = to(dev, d["z"], d["w"], d["scale"], d["shift"])
    y, st = impl.conv_fwd(z, w, s, p, None, None, False, True, sc, sh)
    t = T.conv(d["z"], d["w"], s, p, in_scale=d["scale"], in_shift=d["shift"])["y"]
    return {"y": _ch(y, t), "stats": _rows(st.double().sum(0), T.stats_of(_cpu(y)))}, [y, st]


def run_conv_dgrad(impl, name, dev="cpu"):
    """conv_dgrad plain and into a residual (a clone: the stride-2 form consumes the buffer)."""
    case = all_cases()[name]
    N, H, W, C, K, R, s, p = case["shape"]
    d = T.conv_inputs(name)
    dy, wd, dres = to(dev, d["dy"], d["wd"], d["dres"])
    dx = impl.conv_dgrad(dy, wd, H, W, s, p, None)
    dxr = impl.conv_dgrad(dy, wd, H, W, s, p, dres.clone())
    t = T.conv_truth(name, "dx")
    return {"dx": _ch(dx, t), "dx_resid": _ch(dxr, t + d["dres"].double())}, [dx, dxr]


def bnr_mask(name, form):
    """The fp64 ReLU mask (bool) of a conv_dgrad_bnr form."""
    d = T.conv_inputs(name)
    if T.BNR_FORMS[form]["mask"] == "recompute":
        return (d["bx"].double() * d["msc"].double() + d["msh"].double()) > 0
    return d["ymask"].double() > 0


def run_conv_dgrad_bnr(impl, name, form, dev="cpu"):
    """conv_dgrad_bnr in one of T.BNR_FORMS: g against the masked fp64 dx (+ residual), the partial
    sums against the fp64 sums of the implementation's own g.  Returns (res, raw, mask)."""
    case = all_cases()[name]
    N, H, W, C, K, R, s, p = case["shape"]
    f = T.BNR_FORMS[form]
    d = T.conv_inputs(name)
    sub = f.get("resid_sub", False)
    resid = (d["dres_sub"] if sub else d["dres"]) if f.get("resid") else None
    dual, fold = f.get("dual", False), f.get("fold", False)
    ymask = d["ymask"] if f["mask"] == "tensor" else None
    bits = ref.pack_mask_bits(d["ymask"]) if f["mask"] == "bits" else None
    msc, msh = (d["msc"], d["msh"]) if f["mask"] == "recompute" else (None, None)
    a = to(dev, d["dy"], d["wd"], resid, ymask, d["bx"], d["mean"], d["invstd"], d["bx2"] if dual else None,
           d["mean2"] if dual else None, d["invstd2"] if dual else None, msc, msh, bits, d["fx"] if fold else None,
           d["fcoef"] if fold else None)
    dy, wd, resid_d, ymask_d, bx, mean, invstd, bx2, mean2, invstd2, msc_d, msh_d, bits_d, fx, fcoef = a
    out = impl.conv_dgrad_bnr(dy, wd, H, W, s, p, resid_d.clone() if resid_d is not None else None, ymask_d, bx, mean,
                              invstd, bx2, mean2, invstd2, msc_d, msh_d, None, bits_d, fx, fcoef, sub)
    assert len(out) == (3 if dual else 2)
    mask = bnr_mask(name, form)
    t = T.conv_truth(name, "dx_fold" if fold else "dx")
    if resid is not None:
        t = t + (T.expand_sub_resid(resid, H, W) if sub else resid).double()
    t = torch.where(mask, t, torch.zeros_like(t))
    g = _cpu(out[0])
    res = {"g": _ch(g, t), "part": _rows(out[1].double().sum(0), T.bnr_sums(g, d["bx"], d["mean"], d["invstd"]))}
    if dual:
        res["part2"] = _rows(out[2].double().sum(0), T.bnr_sums(g, d["bx2"], d["mean2"], d["invstd2"]))
    return res, list(out), mask


def _wgrad(impl, shape, d, dev, fold=None):
    N, H, W, C, K, R, s, p = shape
    dy, x, dw0, fx, fcoef, asc, ash = to(dev, d["dy"], d["x"], d["dw0"], d["fx"], d["fcoef"], d["asc"], d["ash"])
    fa = (fx, fcoef) if fold in ("dz", "both") else (None, None)
    aa = (asc, ash) if fold in ("act", "both") else (None, None)
    out = torch.empty(K, R, R, C, device=dev)
    impl.conv_wgrad(dy, x, out, R, R, s, p, False, *fa, *aa)
    acc = dw0.clone()
    impl.conv_wgrad(dy, x, acc, R, R, s, p, True, *fa, *aa)
    return out, acc


def run_conv_wgrad(impl, name, dev="cpu"):
    """conv_wgrad of a conv case: written, and accumulated into a non-zero buffer (truth dw0 + dw)."""
    case = all_cases()[name]
    d = T.conv_inputs(name)
    out, acc = _wgrad(impl, case["shape"], d, dev)
    t = T.conv_truth(name, "dw")
    return {"dw": _rows(out, t), "dw_acc": _rows(acc, t + d["dw0"].double())}, [out, acc]


def run_wgrad_case(impl, name, dev="cpu"):
    """A case of T.WGRAD_CASES; returns (op, res, raw): the folded forms are their own op (their floor
    carries the operand's bf16 rounding)."""
    case = T.WGRAD_CASES[name]
    N, H, W, C, K, R, s, p = case["shape"]
    d = T.wgrad_inputs(name)
    fold = case.get("fold")
    out, acc = _wgrad(impl, case["shape"], d, dev, fold)
    t = T.conv(d["x"], torch.zeros(K, R, R, C), s, p, dy=d["dy"],
               in_scale=d["asc"] if fold in ("act", "both") else None, in_shift=d["ash"] if fold in ("act", "both") else None,
               fold_x=d["fx"] if fold in ("dz", "both") else None, fold_coef=d["fcoef"] if fold in ("dz", "both") else None)["dw"]
    op = "conv_wgrad_fold" if fold else "conv_wgrad"
    return op, {"dw": _rows(out, t), "dw_acc": _rows(acc, t + d["dw0"].double())}, [out, acc]


FUSED_SHAPES = [(32, 1), (96, 0), (160, 1)]    # (rows % 32 == 0, fold): 1, 3 and 5 row groups


def fused_case(M, fold):
    """conv1x1_bwd_fused: K = 256 -> C = 64 (the only compiled geometry), M rows as [M, 1, 1, .]."""
    gen = T._gen(M + fold)
    K, C = 256, 64
    rn = lambda *sh, scale=1.0: (torch.randn(*sh, generator=gen) * scale).to(T.BF)  # noqa: E731
    d = dict(g=rn(M, 1, 1, K), fx=rn(M, 1, 1, K), fcoef=torch.stack([torch.rand(K, generator=gen) + 0.5,
             torch.randn(K, generator=gen) * 0.2, torch.randn(K, generator=gen) * 0.1]),
             w=rn(K, 1, 1, C, scale=(2.0 / K) ** 0.5), z=T._grid((M, 1, 1, C), gen), dw0=torch.randn(K, 1, 1, C, generator=gen),
             mean=torch.randn(C, generator=gen) * 0.1, invstd=torch.rand(C, generator=gen) + 0.5)
    d["scale"] = torch.tensor([1.0, -1.0, 2.0, -2.0])[torch.randint(0, 4, (C,), generator=gen)]
    d["shift"] = (2 * torch.randint(-8, 8, (C,), generator=gen) + 1).float() / 16      # |scale*z + shift| >= 1/16
    return d


def run_bwd_fused(impl, M, fold, dev="cpu"):
    """All three outputs: g_in (masked by relu(scale*z + shift) > 0), its BN partials, dw accumulated
    into a non-zero buffer."""
    d = fused_case(M, fold)
    K, C = 256, 64
    g, fx, fcoef, w, z, sc, sh, mean, invstd, dw0 = to(dev, d["g"], d["fx"], d["fcoef"], d["w"], d["z"], d["scale"],
                                                        d["shift"], d["mean"], d["invstd"], d["dw0"])
    wt = w.reshape(K, C).t().contiguous().reshape(C, 1, 1, K)
    dw = dw0.clone()
    gin, part = impl.conv1x1_bwd_fused(g, fx if fold else None, fcoef if fold else None, wt, z, sc, sh, mean, invstd, dw, True)
    t = T.conv(d["z"], d["w"], 1, 0, dy=d["g"], in_scale=d["scale"], in_shift=d["shift"],
               fold_x=d["fx"] if fold else None, fold_coef=d["fcoef"] if fold else None)
    mask = (d["z"].double() * d["scale"].double() + d["shift"].double()) > 0
    tg = torch.where(mask, t["dx"], torch.zeros_like(t["dx"]))
    gc = _cpu(gin)
    res = {"g": _ch(gc, tg), "part": _rows(part.double().sum(0), T.bnr_sums(gc, d["z"], d["mean"], d["invstd"])),
           "dw": _rows(dw, t["dw"] + d["dw0"].double())}
    return res, [gin, part, dw], mask


# ------------------------------------------------------------------------------ BatchNorm
def bn_op(M):
    """The single-row cases are an op of their own in the bound table: their y = scale*x + shift
    cancels two terms ~1e3 times its size, a noise the other shapes' floor must not inherit."""
    return "bn" if M > 1 else "bn_one_row"


def run_bn(impl, M, C, mode, relu, accumulate, dev="cpu", mbits=False, dtype=T.BF):
    """bn_partials -> bn_finalize (running buffers) -> bn_apply, then bn_bwd_reduce -> bn_bwd_finalize
    -> bn_bwd_apply on the forward's own y / mean / invstd.  An accumulating call starts dgamma / dbeta
    from 0.5.  Returns (res, raw); raw["mbits"] with ``mbits``."""
    d = T.bn_case(M, C, mode, relu, dtype)
    t = d["truth"]
    x, gamma, beta, dy, x2, gamma2, beta2 = to(dev, d["x"], d["gamma"], d["beta"], d["dy"], d["x2"], d["gamma2"], d["beta2"])
    rm, rv = to(dev, d["rm"].clone(), d["rv"].clone())
    bn2 = mode == "bn2"
    part = impl.bn_partials(x)
    mean, invstd, sc, sh = impl.bn_finalize(part, M, gamma, beta, rm, rv, 0.1, 1e-5)
    res = {"part": _rows(part.double().sum(0), T.stats_of(d["x"])), "mean": _all(mean, t["mean"]),
           "invstd": _all(invstd, t["invstd"]), "running_mean": _all(rm, t["running_mean"]),
           "running_var": _all(rv, t["running_var"])}
    sc2 = sh2 = mean2 = invstd2 = None
    if bn2:
        rm2, rv2 = to(dev, d["rm2"].clone(), d["rv2"].clone())
        mean2, invstd2, sc2, sh2 = impl.bn_finalize(impl.bn_partials(x2), M, gamma2, beta2, rm2, rv2, 0.1, 1e-5)
        res.update(mean2=_all(mean2, t["mean2"]), invstd2=_all(invstd2, t["invstd2"]),
                   running_mean2=_all(rm2, t["running_mean2"]), running_var2=_all(rv2, t["running_var2"]))
    mb = torch.empty(M * C // 8, dtype=torch.uint8, device=dev) if mbits else None
    y = impl.bn_apply(x, sc, sh, x2, sc2, sh2, relu, mb)
    res["y"] = _ch(y, t["y"])
    ymask = y if relu else None
    parts = impl.bn_bwd_reduce(dy, ymask, x, mean, invstd, x2 if bn2 else None, mean2, invstd2)
    gm = _cpu(dy).double() * ((_cpu(y).double() > 0) if relu else 1.0)
    res["bwd_part"] = _rows(parts[0].double().sum(0), T.bnr_sums(gm, d["x"], _cpu(mean), _cpu(invstd)))
    init = 0.5 if accumulate else float("nan")
    dg, db = (torch.full((C,), init, device=dev) for _ in range(2))
    coef = impl.bn_bwd_finalize(parts[0], M, gamma, mean, invstd, dg, db, accumulate)
    off = 0.5 if accumulate else 0.0
    res.update(dgamma=_all(dg, t["dgamma"] + off), dbeta=_all(db, t["dbeta"] + off))
    coef2 = None
    if bn2:
        res["bwd_part2"] = _rows(parts[1].double().sum(0), T.bnr_sums(gm, d["x2"], _cpu(mean2), _cpu(invstd2)))
        dg2, db2 = (torch.full((C,), init, device=dev) for _ in range(2))
        coef2 = impl.bn_bwd_finalize(parts[1], M, gamma2, mean2, invstd2, dg2, db2, accumulate)
        res.update(dgamma2=_all(dg2, t["dgamma2"] + off), dbeta2=_all(db2, t["dbeta2"] + off))
    outs = impl.bn_bwd_apply(dy, ymask, x, coef, x2 if bn2 else None, coef2, True)
    if M == 1:
        # dx = k1*g + k2*x + k3 with k2 = 0 and k3 = -k1*g: the truth is exactly 0 and has no noise floor.
        # What is left is the cancellation of two fp32 terms of size |gamma*invstd*g|, each rounded twice
        # (k1 and its product; k3 and the sum): at most 4 * 2^-24 of that size, then one bf16 rounding
        for o, gam in ((outs[0], d["gamma"]),) + (((outs[1], d["gamma2"]),) if bn2 else ()):
            lim = 4 * 2.0 ** -24 * (gam.double() * t["invstd"] * gm.abs()) * (1 + 2.0 ** -8)
            assert bool((_cpu(o).double().abs() <= lim).all()), "dx of a single row"
    else:
        res["dx"] = _ch(outs[0], t["dx"])
    if bn2:
        if M > 1:
            res["dx2"] = _ch(outs[1], t["dx2"])
    elif mode == "resid":
        res["dx2"] = _ch(outs[-1], t["dx2"])      # the residual branch takes the masked gradient g
    return res, {"y": y, "mbits": mb, "outs": list(outs), "stats": [mean, invstd, rm, rv, dg, db]}


# ------------------------------------------------------------------------------ pooling
def pool_bnr_ok(C):
    """maxpool_bwd_bnr's channel layout (csrc/elementwise.hip): C / 8 vectors dividing a 256-thread
    block; other channel counts are refused (C = 72 among the cases)."""
    return C % 8 == 0 and 256 % (C // 8) == 0


def run_pool(impl, shape, dev="cpu", dtype=T.BF):
    """maxpool_fwd / maxpool_bwd alone and behind the stem's BN + ReLU prologue, maxpool_bwd_bnr's
    masked gradient and partial sums, GAP forward and backward."""
    N, H, W, C = shape
    d = T.pool_case(shape, dtype)
    x, dy, scale, shift, mean, invstd, gdy = to(dev, d["x"], d["dy"], d["scale"], d["shift"], d["mean"], d["invstd"], d["gdy"])
    y, idx = impl.maxpool_fwd(x, 3, 2, 1, True)
    dx = impl.maxpool_bwd(dy, idx, H, W, 3, 2, 1)
    t = T.maxpool(d["x"], d["dy"])
    y2, idx2 = impl.maxpool_fwd(x, 3, 2, 1, True, scale, shift)
    t2 = T.maxpool(d["x"], d["dy"], d["scale"], d["shift"])
    mask = (d["x"].double() * d["scale"].double() + d["shift"].double()) > 0
    tgap = T.gap(d["x"], d["gdy"])
    res = {"y": _ch(y, t["y"]), "dx": _ch(dx, t["dx"]), "y_bn": _ch(y2, t2["y"]),
           "gap_y": _ch(impl.gap_fwd(x), tgap["y"]), "gap_dx": _ch(impl.gap_bwd(gdy, H, W), tgap["dx"])}
    g = part = None
    if pool_bnr_ok(C) if dtype == T.BF else C % 4 == 0:   # (the fp32 kernels: float4 = 4 channels)
        g, part = impl.maxpool_bwd_bnr(dy, idx2, x, mean, invstd, scale, shift, 3, 2, 1)
        gc = _cpu(g)
        res["g"] = _ch(gc, torch.where(mask, t2["dx"], torch.zeros_like(t2["dx"])))
        res["part"] = _rows(part.double().sum(0), T.bnr_sums(gc, d["x"], d["mean"], d["invstd"]))
    return res, [y, idx, dx, y2, idx2, g, part], mask


# ------------------------------------------------------------------------------ optimizers
LR, WD = 0.05, 0.01
SGD_VARIANTS = [dict(momentum=0.9, nesterov=True, weight_decay=WD), dict(momentum=0.9, nesterov=False, weight_decay=0.0)]


def _scalar(v, dev):
    return torch.tensor([float(v)], device=dev)


def run_sgd(impl, n, variant, gscale, with_shadow, dev="cpu"):
    """Three consecutive sgd_flat steps from zero state (first_step true, then false); every state
    tensor of every step is compared.  Returns (res, last raw state)."""
    d = T.opt_case(n)
    kw = SGD_VARIANTS[variant]
    truth = T.optimizer_steps("sgd", d["w"], d["grads"], LR, gscale, **kw)
    w, mom = d["w"].clone().to(dev), torch.zeros(n, device=dev)
    sh = torch.empty(n, dtype=T.BF, device=dev) if with_shadow else None
    gs = _scalar(gscale, dev) if gscale is not None else None
    res = {"w": [], "mom": [], "shadow": []}
    for i, g in enumerate(d["grads"]):
        impl.sgd_flat(w, g.to(dev), mom, sh, None, _scalar(LR, dev), gs, kw["momentum"], 0.0, kw["weight_decay"],
                      kw["nesterov"], i == 0)
        res["w"].append(_all(w.clone(), truth[i]["w"]))
        res["mom"].append(_all(mom.clone(), truth[i]["mom"]))
        if with_shadow:
            res["shadow"].append(_all(sh.clone(), truth[i]["w"]))
    return res, (w, mom, sh)


def run_adam(impl, n, decoupled, gscale, with_shadow, dev="cpu"):
    """Three consecutive adam_flat steps from zero state (t = 1, 2, 3)."""
    d = T.opt_case(n)
    truth = T.optimizer_steps("adamw" if decoupled else "adam", d["w"], d["grads"], LR, gscale, betas=(0.9, 0.999),
                              eps=1e-8, weight_decay=WD)
    w, m1, m2 = d["w"].clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    sh = torch.empty(n, dtype=T.BF, device=dev) if with_shadow else None
    gs = _scalar(gscale, dev) if gscale is not None else None
    res = {"w": [], "m1": [], "m2": [], "shadow": []}
    for i, g in enumerate(d["grads"]):
        impl.adam_flat(w, g.to(dev), m1, m2, sh, None, _scalar(LR, dev), gs, _scalar(i + 1, dev), 0.9, 0.999, 1e-8, WD,
                       decoupled)
        for k, v in (("w", w), ("m1", m1), ("m2", m2)):
            res[k].append(_all(v.clone(), truth[i][k]))
        if with_shadow:
            res["shadow"].append(_all(sh.clone(), truth[i]["w"]))
    return res, (w, m1, m2, sh)


def run_adam_late(impl, n, decoupled, dev="cpu"):
    """One step at t = 10000 from a given state (bias corrections 1 - 0.9^t = 1, 1 - 0.999^t = 0.99995)."""
    d = T.opt_case(n)
    truth = T.adam_step_from(d["w"], d["grads"][0], d["m1"], d["m2"], 10000, LR, 0.9, 0.999, 1e-8, WD, decoupled)
    w, m1, m2, g = to(dev, d["w"].clone(), d["m1"].clone(), d["m2"].clone(), d["grads"][0])
    sh = torch.empty(n, dtype=T.BF, device=dev)
    impl.adam_flat(w, g, m1, m2, sh, None, _scalar(LR, dev), None, _scalar(10000, dev), 0.9, 0.999, 1e-8, WD, decoupled)
    return {"w": _all(w, truth["w"]), "m1": _all(m1, truth["m1"]), "m2": _all(m2, truth["m2"]),
            "shadow": _all(sh, truth["w"])}, (w, m1, m2, sh)


def clip_variants(n):
    """(pre_scale, max_norm, post_scale): the norm (about sqrt(n)) above and below max_norm, and no clip."""
    r = float(n) ** 0.5
    return [(1.0, 0.5 * r, 0.25), (0.5, 2.0 * r, 0.25), (1.0, 0.0, 0.5)]


def run_clip(impl, n, variant, dev="cpu"):
    """grad_clip_coef, and the two-phase form over three uneven buckets into a NaN-filled buffer."""
    d = T.opt_case(n)
    g = d["grads"][0]
    pre, mx, post = variant
    tn, tc = T.clip_coef(g, pre, mx, post)
    gd = g.to(dev)
    norm, coef = impl.grad_clip_coef(gd, pre, mx, post)
    cuts = [0, 4 * (n // 12), 4 * (n // 12) + 4 * (n // 6), n] if n >= 24 else [0, n]
    cuts = [c for i, c in enumerate(cuts) if i == 0 or c > cuts[i - 1]]
    nb = [ref.sumsq_blocks(cuts[i + 1] - cuts[i]) for i in range(len(cuts) - 1)]
    part = torch.full((sum(nb),), float("nan"), device=dev)
    off = 0
    for i, b in enumerate(nb):
        impl.grad_sumsq_parts(gd[cuts[i]:cuts[i + 1]], part, off)
        off += b
    norm2, coef2 = impl.clip_coef_parts(part, pre, mx, post)
    return {"norm": [_all(norm, tn), _all(norm2, tn)], "coef": [_all(coef, tc), _all(coef2, tc)]}, (norm, coef, part)


def run_masked(impl, n, dev="cpu"):
    """One sgd_flat and one adam_flat step from a non-zero state with and without ``mask`` (uint8, 0 =
    frozen).  Returns the tensors before (``_0``), after the masked step, and after the unmasked one
    (``_free``), on the CPU."""
    d = T.opt_case(n)
    g, mask = d["grads"][0].to(dev), d["mask"].to(dev)
    out = {"mask": d["mask"]}
    for tag, m in (("", mask), ("_free", None)):
        w, mom = d["w"].clone().to(dev), d["m1"].clone().to(dev)
        impl.sgd_flat(w, g, mom, None, m, _scalar(LR, dev), None, 0.9, 0.0, WD, False, False)
        out.update({"sgd_w" + tag: _cpu(w), "sgd_mom" + tag: _cpu(mom)})
        w, m1, m2 = d["w"].clone().to(dev), d["m1"].clone().to(dev), d["m2"].clone().to(dev)
        impl.adam_flat(w, g, m1, m2, None, m, _scalar(LR, dev), None, _scalar(5, dev), 0.9, 0.999, 1e-8, WD, False)
        out.update({"adam_w" + tag: _cpu(w), "adam_m1" + tag: _cpu(m1), "adam_m2" + tag: _cpu(m2)})
    out.update(sgd_w_0=d["w"], sgd_mom_0=d["m1"], adam_w_0=d["w"], adam_m1_0=d["m1"], adam_m2_0=d["m2"])
    return out
