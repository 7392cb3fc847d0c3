"""Runners shared by tests/test_text_truth_cpu.py and tests/test_text_truth_gpu.py: each evaluates one
case of ``ops/truth.py`` with an implementation of the op set (``ops/ref.py`` on the CPU,
``torch.ops.pcmp`` on the GPU), forward and then backward on the forward's own saved outputs, and
returns ``{output: (got, truth, seg_dims)}`` (or a list of such chunks) in the views the segments
are defined on."""
from __future__ import annotations

import torch

from . import truth as T

LN_SEED, LN_OFF = 77, 1 << 32
AT_SEED, AT_OFF = 99, 5 << 32


def _salt(dev, v=3):
    return torch.tensor([v], device=dev, dtype=torch.int64)


def to(dev, *ts):
    return [t.to(dev) if t is not None else None for t in ts]


def seg_view(a, t, seg):
    """(got, truth, seg_dims) in the view the segment function gives."""
    return seg(a)[0], seg(t)[0], seg(a)[1]


# ------------------------------------------------------------------------------ runners
def run_lstm(impl, case, dev="cpu", guard=None, truth=None, bwd=True):
    """Forward, then (``bwd``) the backward on the forward's own gates / c (as production does).
    ``guard`` is called with the sync words right after each launch (the GPU tests stop there on a
    barrier timeout); ``truth`` takes a T.lstm() result computed before."""
    gx, whh, ids, dh = to(dev, *case)
    H = whh.shape[2]
    h, g, c, sync = impl.lstm_seq_fwd(gx, whh, ids)
    if guard:
        guard(sync)
    th, tg, tc, tdg = truth if truth is not None else T.lstm(gx, whh, ids, dh)
    out = {"hout": seg_view(h, th, lambda x: T.seg_hout(x, H)), "gates": seg_view(g, tg, lambda x: T.seg_gates(x, H)),
           "c": seg_view(c, tc, T.seg_c)}
    if not bwd:
        return out, (h, g, c)
    dg, sync2 = impl.lstm_seq_bwd(dh, g, c, whh, ids)
    if guard:
        guard(sync2)
    out["dgates"] = seg_view(dg, tdg, lambda x: T.seg_gates(x, H))
    return out, (h, g, c, dg)


def run_attention(impl, case, S, p, H=2, dev="cpu"):
    """Returns (res, one_key, raw).  A sequence with a single valid key has P = 1 for that key, so
    the truth's dQ and dK are identically zero there by cancellation (dP - D), not by masking: those
    segments have no noise floor (their bound is exact zero, whatever k) and come back apart in
    ``one_key`` for the tests that ask for the exact zeros; ``res`` holds everything else."""
    qkv, ids, dctx, B, lens = case
    qkv, ids, dctx = to(dev, qkv, ids, dctx)
    salt = _salt(dev, 2) if p > 0 else None
    ctx, lse = impl.attention_fwd(qkv, ids, B, S, H, p, AT_SEED, AT_OFF, salt)
    dq = impl.attention_bwd(dctx, qkv, ctx, lse, ids, B, S, H, p, AT_SEED, AT_OFF, salt)
    tctx, tlse, tdq = T.attention(qkv, ids, B, S, H, p, AT_SEED, AT_OFF, salt, dctx)
    one = [b for b in range(B) if ids is not None and lens[b] == 1]
    rest = [b for b in range(B) if b not in one]
    a, t, sd = seg_view(dq, tdq, lambda x: T.seg_dqkv(x, B, S, H))
    res = {"ctx": seg_view(ctx, tctx, lambda x: T.seg_ctx(x, B, S, H)), "lse": seg_view(lse, tlse, lambda x: T.seg_lse(x, B, H)),
           "dqkv": [(a[rest], t[rest], sd), (a[one][:, :, 2:], t[one][:, :, 2:], sd)]}
    one_key = {"dqk": (a[one][:, :, :2], t[one][:, :, :2], sd)}
    return res, one_key, (ctx, lse, dq)


def ln_variants(M, D):
    """(with_r, p, accumulate, fused, accmask) of one LayerNorm shape."""
    v = [(wr, p, acc, False, 0) for wr in (True, False) for p in (0.0, 0.1) for acc in (False, True)]
    if D % 256 == 0 and D <= 1024:
        v += [(wr, p, False, True, am) for wr in (True, False) for p in (0.0, 0.1) for am in (0, 0b111)]
    return v


def run_layernorm(impl, case, variant, dev="cpu"):
    """layernorm_fwd, then layernorm_bwd (or layernorm_bwd_fused with a bias gradient) on the
    forward's own xs / mean / rstd.  The gradient vectors start at 0.5, so an accumulating call
    must give truth + 0.5.  A constant last row (M >= 3, p == 0) has rstd = 1e6: it is left out of
    the dx / dxd / rstd comparison (the caller checks it on its own)."""
    with_r, p, acc, fused, accmask = variant
    x, r, g, b, dy = to(dev, *case)
    M, D = x.shape
    salt = _salt(dev) if p > 0 else None
    y, xs, mean, rstd = impl.layernorm_fwd(x, r, g, b, 1e-12, p, LN_SEED, LN_OFF, salt)
    txs = T.ln_input(x, r, p, LN_SEED, LN_OFF, salt)
    keep = T.keep_mask((M, D), p, LN_SEED, LN_OFF, salt, x.device)
    t = T.layernorm(txs, g, b, 1e-12, dy, keep)
    dgo, dbo, dbi = (torch.full((D,), 0.5, device=x.device) for _ in range(3))
    if fused:
        dx, dxd = impl.layernorm_bwd_fused(dy, xs, mean, rstd, g, dgo, dbo, dbi, accmask, p, LN_SEED, LN_OFF, salt)
        accs = [(accmask >> w) & 1 for w in range(3)]
    else:
        dx = impl.layernorm_bwd(dy, xs, mean, rstd, g, dgo, dbo, acc)
        dxd = None
        accs = [int(acc)] * 2
    rows = slice(0, M - 1) if (M >= 3 and p == 0) else slice(0, M)
    out = {"y": seg_view(y, t["y"], T.seg_rows), "xs": seg_view(xs, txs, T.seg_rows), "mean": seg_view(mean, t["mean"], T.seg_all),
           "rstd": seg_view(rstd[rows], t["rstd"][rows], T.seg_all), "dx": seg_view(dx[rows], t["dx"][rows], T.seg_rows),
           "dgamma": seg_view(dgo, t["dgamma"] + 0.5 * accs[0], T.seg_all), "dbeta": seg_view(dbo, t["dbeta"] + 0.5 * accs[1], T.seg_all)}
    if fused:
        out["dxd"] = seg_view(dxd[rows], t["dxd"][rows], T.seg_rows)
        out["dbias"] = seg_view(dbi, t["dbias"] + 0.5 * accs[2], T.seg_all)
    return out, (y, xs, mean, rstd, dx, dxd)


def run_embed_layernorm(impl, case, dev="cpu"):
    x, pos, tt, g, b = to(dev, *case)
    y, xs, mean, rstd = impl.embed_layernorm_fwd(x, pos, tt, g, b, 1e-12)
    txs = T.embed_ln_input(x, pos, tt)
    t = T.layernorm(txs, g, b, 1e-12)
    return {"y": seg_view(y, t["y"], T.seg_rows), "xs": seg_view(xs, txs, T.seg_rows), "mean": seg_view(mean, t["mean"], T.seg_all),
            "rstd": seg_view(rstd, t["rstd"], T.seg_all)}


def run_activations(impl, case, dev="cpu"):
    x, dy = to(dev, *case)
    gy, gdx = T.gelu(x, dy)
    ty, tdx = T.tanh(x, dy)
    y = impl.tanh_fwd(x)
    got = {"gelu_y": impl.gelu_fwd(x), "gelu_dx": impl.gelu_bwd(dy, x), "tanh_y": y, "tanh_dx": impl.tanh_bwd(dy, y),
           "add": impl.add_bf16(x, dy)}
    tr = {"gelu_y": gy, "gelu_dx": gdx, "tanh_y": ty, "tanh_dx": tdx, "add": T.add(x, dy)}
    return {n: (got[n], tr[n], (0,)) for n in got}, got


def run_embedding(impl, case, accumulate, dev="cpu"):
    _, ids, W, dy, dW0 = case
    ids, W, dy, dW0 = to(dev, ids, W, dy, dW0)
    y = impl.embedding_fwd(ids, W)
    dW = dW0.clone()
    impl.embedding_bwd(ids, dy, dW, 0, accumulate)
    ty, tdW = T.embedding(ids, W, dy, 0, dW0 if accumulate else None)
    return {"y": (y, ty, (0, 1, 2)), "dW": (dW, tdW, (0, 1))}, (y, dW)


def run_masked_mean(impl, case, dev="cpu"):
    x, ids, dy = to(dev, *case)
    y = impl.masked_mean_fwd(x, ids)
    dx = impl.masked_mean_bwd(dy, ids, x.shape[1])
    ty, tdx = T.masked_mean(x, ids, dy)
    return {"y": (y, ty, (0, 1)), "dx": (dx, tdx, (0, 1, 2))}, (y, dx)


def chunks(v):
    return v if isinstance(v, list) else [v]


def worst(res):
    return {n: max([float(T.norm_err(a, t, s).max()) for a, t, s in chunks(v) if a.numel()], default=0.0)
            for n, v in res.items()}


def check(bounds, op, res, what=""):
    """Every output of one case within its bound k = bounds[(op, output)][1] of the truth; the worst
    norm_err per output is printed first, so a failing run still reports its figures."""
    print(op, what, {n: round(e, 3) for n, e in worst(res).items()})
    for n, v in res.items():
        for a, t, s in chunks(v):
            T.assert_elementwise(a, t, s, bounds[(op, n)][1], f"{op} {n} {what}")


def attn_op(p):
    return "attention_p0" if p == 0 else "attention_drop"
