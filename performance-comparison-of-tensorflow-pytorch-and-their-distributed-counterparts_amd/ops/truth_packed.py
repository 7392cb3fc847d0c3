"""fp64 truth of the packed (padding-free) attention ops and the case their tests share.

The truth is the padded one: the packed rows are scattered to the [B, max_s] rectangle (zeros
outside the segments, a key valid when it lies in its sequence's segment and, with ``ids``, carries
an id > 0), ``truth.attention`` runs on the rectangle in fp64 with the padded dropout keep-mask, and
the segments' rows are gathered back; rows that belong to no segment are zero.  ``dctx`` is zero
outside the segments, so the rectangle's extra queries contribute nothing to dK / dV.  The index
helpers are ``ref.packed_rows`` (part of the layout's definition); no arithmetic is shared with
``ops/ref.py``.

The case (tests/test_attention_packed_cpu.py measures the floors of ``ops/ref.py`` on it,
tests/test_attention_packed_gpu.py holds the kernels to the bounds): H = 2, max_s = 512, eleven
sequences of ``PACKED_TOKENS`` tokens (segments of 32 .. 512 rows, 1728 in all, plus 64 rows that
belong to no sequence at ``rows_multiple`` = 256), random bf16 qkv, dctx zero outside the segments.
"""
from __future__ import annotations

import torch

from . import ref, truth as T, truth_run as R
from ..data.imdb import pack_batch

PACKED_TOKENS = [1, 17, 31, 32, 33, 64, 65, 130, 200, 449, 512]
PACKED_MAX_S, PACKED_H, PACKED_ROWS_MULTIPLE = 512, 2, 256
PACKED_SEED = 0     # the draw of qkv / dctx (tests/test_attention_packed_cpu.py says how it was chosen)


def attention_packed(qkv, cu, ids, B, max_s, H, p_drop=0.0, seed=0, offset=0, salt=None, dctx=None):
    """-> fp64 [ctx [T, D], lse [H, T], dqkv [T, 3D] or None]."""
    Tn, D = qkv.shape[0], qkv.shape[1] // 3
    rows, inside = ref.packed_rows(cu, B, max_s, Tn)
    flat = rows.reshape(-1)

    def padded(x):
        return torch.cat([x.detach().double(), x.new_zeros(1, x.shape[1], dtype=torch.float64)], 0)[flat]

    kid = inside.long() if ids is None else torch.cat([ids.long(), ids.new_zeros(1, dtype=torch.long)])[rows] * inside
    ctx, lse, dq = T.attention(padded(qkv), kid, B, max_s, H, p_drop, seed, offset, salt,
                               None if dctx is None else padded(dctx))
    sel = rows[inside]

    def packed(xp):
        out = xp.new_zeros(Tn, xp.shape[-1])
        out[sel] = xp.reshape(B, max_s, -1)[inside]
        return out

    lse_p = lse.new_zeros(H, Tn)
    lse_p[:, sel] = lse.view(B, H, max_s).transpose(0, 1)[:, inside]
    return [packed(ctx), lse_p, None if dq is None else packed(dq)]


def packed_lens(p):
    """The one-key sequence is a p = 0 case only (truth.attn_lens)."""
    return [5 if p > 0 else PACKED_TOKENS[0]] + PACKED_TOKENS[1:]


def packed_case(p, with_ids=True, seed=PACKED_SEED, lens=None, max_s=PACKED_MAX_S, rows_multiple=PACKED_ROWS_MULTIPLE,
                H=PACKED_H, dtype=torch.bfloat16):
    """-> (qkv [T, 3*64*H], PackedBatch, ids [T] or None, dctx [T, 64*H], lens)."""
    gen = T._gen(1009 * seed + int(100 * p) + (0 if with_ids else 5))
    lens = packed_lens(p) if lens is None else list(lens)
    pad_ids = T.attn_ids(max_s, lens, gen)
    pb = pack_batch(pad_ids, (pad_ids > 0).long(), 32, rows_multiple)
    qkv = torch.randn(pb.rows, 3 * 64 * H, generator=gen).to(dtype)
    dctx = torch.randn(pb.rows, 64 * H, generator=gen).to(dtype)
    dctx[int(pb.cu[-1]):] = 0
    return qkv, pb, (pb.ids if with_ids else None), dctx, lens


def run_attention_packed(impl, case, p, H=PACKED_H, dev="cpu", truth=None):
    """The packed twin of ``truth_run.run_attention``: (res, one_key, raw, truth).  One segment per
    sequence x head (x {q, k, v}) over that sequence's rows; the one-key sequence's dQ / dK come back
    apart in ``one_key`` (exact zeros in the truth)."""
    qkv, pb, ids, dctx, lens = case
    qkv, ids, dctx, cu = R.to(dev, qkv, ids, dctx, pb.cu)
    B, max_s = pb.B, pb.max_s
    salt = R._salt(dev, 2) if p > 0 else None
    ctx, lse = impl.attention_fwd(qkv, ids, B, max_s, H, p, R.AT_SEED, R.AT_OFF, salt, cu)
    dq = impl.attention_bwd(dctx, qkv, ctx, lse, ids, B, max_s, H, p, R.AT_SEED, R.AT_OFF, salt, cu)
    if truth is None:
        truth = attention_packed(qkv.cpu(), pb.cu, None if ids is None else ids.cpu(), B, max_s, H, p, R.AT_SEED,
                                 R.AT_OFF, None if salt is None else salt.cpu(), dctx.cpu())
    tctx, tlse, tdq = R.to(dev, *truth)
    c = pb.cu.tolist()
    res = {"ctx": [], "lse": [], "dqkv": []}
    one_key = {"dqk": []}
    for b in range(B):
        r = slice(c[b], c[b + 1])
        n = c[b + 1] - c[b]
        res["ctx"].append((ctx[r].reshape(n, H, 64), tctx[r].reshape(n, H, 64), (0, 2)))
        res["lse"].append((lse[:, r], tlse[:, r], (0, 1)))
        a, t = dq[r].reshape(n, 3, H, 64), tdq[r].reshape(n, 3, H, 64)
        if ids is not None and lens[b] == 1:
            res["dqkv"].append((a[:, 2:], t[:, 2:], (0, 3)))
            one_key["dqk"].append((a[:, :2], t[:, :2], (0, 3)))
        else:
            res["dqkv"].append((a, t, (0, 3)))
    return res, one_key, (ctx, lse, dq), truth
