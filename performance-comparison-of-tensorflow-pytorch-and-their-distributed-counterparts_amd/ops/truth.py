"""fp64 truths of the text-path ops and the element-wise comparator the tests judge them with.

``ops/ref.py`` mirrors the kernels' roundings by hand; the functions here do not.  Every truth is
plain fp64 torch on the values the bf16 / fp32 inputs hold, with no intermediate rounding, and every
backward comes from ``torch.autograd``.  The only thing shared with ``ref.py`` is the counter-based
dropout keep-mask (``ref.hash_uniform`` / ``ref._attn_drop`` / ``ref._salted``), which is part of
the ops' contract.

Comparator: ``norm_err`` divides the error of each element by ``1e-2*|t| + 5e-3*max_seg|t|`` (the
``close_el`` constants of the conv-path tests), the maximum taken per *segment* so that one head,
one gate or one row cannot hide behind a larger neighbour.  ``assert_elementwise`` requires
``norm_err <= k`` for every element.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import ref

REL, ABS_FRAC = 1e-2, 5e-3     # close_el's constants (tests/test_kernels_gpu.py)


# ------------------------------------------------------------------------------ comparator
def norm_err(a, t, seg_dims):
    """|a - t| / (REL*|t| + ABS_FRAC*max_seg|t|) per element; ``seg_dims`` are the dimensions one
    segment spans (the maximum is taken over them and kept for every other index).  Elements with
    a == t count as 0; any other element of a segment whose truth is identically zero is inf."""
    a, t = a.detach().double(), t.detach().double()
    assert a.shape == t.shape, (tuple(a.shape), tuple(t.shape))
    seg_dims = tuple(d % t.dim() for d in seg_dims)
    if t.numel() == 0:
        return torch.zeros_like(t)
    at = t.abs()
    den = REL * at + ABS_FRAC * (at.amax(dim=seg_dims, keepdim=True) if seg_dims else at)
    err = (a - t).abs()
    same = (a == t)
    out = err / torch.where(den > 0, den, torch.ones_like(den))
    out = torch.where((den > 0) | same, out, torch.full_like(out, float("inf")))
    out = torch.where(same, torch.zeros_like(out), out)
    return torch.where(torch.isnan(out), torch.full_like(out, float("inf")), out)   # NaN never passes


def assert_elementwise(a, t, seg_dims, k, what=""):
    """Every element of ``a`` within ``k`` of the truth ``t`` (see ``norm_err``); where a segment's
    truth is identically zero ``a`` must be exactly zero.  Returns the worst normalised error."""
    e = norm_err(a, t, seg_dims)
    worst = float(e.max()) if e.numel() else 0.0
    if not worst <= k:
        bad = e > k
        idx = tuple(int(i) for i in torch.nonzero(e == e.max())[0])
        raise AssertionError(
            f"{what or 'tensor'}: {int(bad.sum())} of {e.numel()} elements beyond norm_err {k} "
            f"(worst {worst:.3g} at {idx}: got {float(a.detach().double()[idx]):.6g}, "
            f"truth {float(t.detach().double()[idx]):.6g})")
    return worst


def seg_rel(a, t, seg_dims):
    """Norm-relative error per segment (the fp32 tests' criterion): ||a - t|| / ||t|| over
    ``seg_dims``; a segment whose truth is zero gives 0 when ``a`` is zero there too, else inf."""
    a, t = a.detach().double(), t.detach().double()
    assert a.shape == t.shape, (tuple(a.shape), tuple(t.shape))
    seg_dims = tuple(d % t.dim() for d in seg_dims)
    if t.numel() == 0:
        return torch.zeros(())
    num = (a - t).pow(2).sum(dim=seg_dims).sqrt()
    den = t.pow(2).sum(dim=seg_dims).sqrt()
    out = num / torch.where(den > 0, den, torch.ones_like(den))
    out = torch.where((den > 0) | (num == 0), out, torch.full_like(out, float("inf")))
    return torch.where(torch.isnan(out), torch.full_like(out, float("inf")), out)


# The segment of every compared tensor: (view it is judged in, dimensions one segment spans).
def seg_hout(x, H):          # [B, S, 2H] -> one segment per direction
    return x.reshape(x.shape[0], x.shape[1], 2, H), (0, 1, 3)


def seg_c(x):                # [B, S, 2, H] -> per direction
    return x, (0, 1, 3)


def seg_gates(x, H):         # [B, S, 2, 4H] -> per direction x gate
    return x.reshape(x.shape[0], x.shape[1], 2, 4, H), (0, 1, 4)


def seg_ctx(x, B, S, H):     # [B*S, D] -> per sequence x head
    return x.reshape(B, S, H, -1), (1, 3)


def seg_dqkv(x, B, S, H):    # [B*S, 3D] -> per sequence x {q, k, v} x head
    return x.reshape(B, S, 3, H, -1), (1, 4)


def seg_lse(x, B, H):        # [B*H, S] -> per sequence
    return x.reshape(B, H, -1), (1, 2)


def seg_rows(x):             # [M, D] -> per row
    return x.reshape(-1, x.shape[-1]), (1,)


def seg_all(x):              # one segment
    return x, tuple(range(x.dim()))


# ------------------------------------------------------------------------------ LSTM
def lstm(gx, whh, ids, dh=None):
    """BiLSTM recurrence over the per-step mask ids > 0 (state carried at masked steps, the gates
    of a masked step still evaluated, as in ``ref.lstm_seq_fwd``).  Returns fp64
    [hout [B,S,2H], gates [B,S,2,4H], c [B,S,2,H], dgates [B,S,2,4H] or None] with
    dgates = d(sum(hout * dh)) / d(gx) by autograd."""
    B, S, _, G4 = gx.shape
    H = G4 // 4
    gx64 = gx.detach().double().requires_grad_(dh is not None)
    W = whh.detach().double()
    valid = ids > 0
    hs, gs, cs = [], [], []
    for d in range(2):
        h = gx64.new_zeros(B, H)
        c = gx64.new_zeros(B, H)
        ho, go, co = [None] * S, [None] * S, [None] * S
        for t in (range(S) if d == 0 else range(S - 1, -1, -1)):
            pre = gx64[:, t, d] + h @ W[d].t()
            i, f, g, o = pre.split(H, dim=1)
            i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
            cn = f * c + i * g
            hn = o * torch.tanh(cn)
            v = valid[:, t].unsqueeze(1)
            c = torch.where(v, cn, c)
            h = torch.where(v, hn, h)
            ho[t], go[t], co[t] = h, torch.cat([i, f, g, o], 1), c
        hs.append(torch.stack(ho, 1))
        gs.append(torch.stack(go, 1))
        cs.append(torch.stack(co, 1))
    hout = torch.cat(hs, 2)
    gates = torch.stack(gs, 2)
    cst = torch.stack(cs, 2)
    dgates = None
    if dh is not None:
        dgates, = torch.autograd.grad((hout * dh.detach().double()).sum(), gx64)
    return [hout.detach(), gates.detach(), cst.detach(), dgates]


# ------------------------------------------------------------------------------ attention
def attention(qkv, ids, B, S, H, p_drop=0.0, seed=0, offset=0, salt=None, dctx=None):
    """softmax(q k^T / 8 + mask) v per head (head dim 64), the keep-mask of the counter-based RNG
    applied to the probabilities.  Returns fp64 [ctx [B*S, D], lse [B*H, S], dqkv [B*S, 3D] or
    None], dqkv = d(sum(ctx * dctx)) / d(qkv) by autograd.  A sequence without a valid key has no
    softmax: its rows are outside the contract (see ``ref.attention_fwd``)."""
    D = qkv.shape[-1] // 3
    x = qkv.detach().double().requires_grad_(dctx is not None)
    t = x.view(B, S, 3, H, D // H)
    q, k, v = t[:, :, 0].transpose(1, 2), t[:, :, 1].transpose(1, 2), t[:, :, 2].transpose(1, 2)
    s = q @ k.transpose(-1, -2) * 0.125
    if ids is not None:
        s = s + torch.where((ids > 0).view(B, 1, 1, S), 0.0, -1e30).to(s)
    lse = torch.logsumexp(s, -1)
    P = torch.softmax(s, -1)
    dm = ref._attn_drop(B, H, S, p_drop, ref._salted(seed, salt), offset, qkv.device)
    if dm is not None:
        P = P * dm.double()
    ctx = (P @ v).transpose(1, 2).reshape(B * S, D)
    dqkv = None
    if dctx is not None:
        dqkv, = torch.autograd.grad((ctx * dctx.detach().double().reshape(B * S, D)).sum(), x)
    return [ctx.detach(), lse.detach().reshape(B * H, S), dqkv]


# ------------------------------------------------------------------------------ LayerNorm
def keep_mask(shape, p, seed, offset, salt, device):
    """The hidden-dropout keep-mask scaled by 1 / (1 - p), fp64; None when p == 0."""
    if p <= 0:
        return None
    n = 1
    for s in shape:
        n *= s
    idx = torch.arange(n, device=device, dtype=torch.int64) + offset
    return (ref.hash_uniform(ref._salted(seed, salt), idx).view(shape) >= p).double() / (1.0 - p)


def ln_input(x, r, p=0.0, seed=0, offset=0, salt=None):
    """xs = drop(x) + r rounded once to the activation dtype: the tensor LayerNorm normalises."""
    xf = x.float()
    if p > 0:
        idx = torch.arange(x.numel(), device=x.device, dtype=torch.int64) + offset
        keep = ref.hash_uniform(ref._salted(seed, salt), idx).view(x.shape) >= p
        xf = torch.where(keep, xf / (1.0 - p), torch.zeros((), device=x.device))
    if r is not None:
        xf = xf + r.float()
    return xf.to(x.dtype)


def layernorm(xs, g, b, eps, dy=None, keep=None):
    """F.layer_norm of the (already rounded) input ``xs`` in fp64.  Returns a dict with y, mean,
    rstd and, given dy, dx / dgamma / dbeta by autograd, plus dxd = dx * keep (the gradient of the
    dropped branch) and dbias = its column sum."""
    D = xs.shape[-1]
    x = xs.detach().double().reshape(-1, D).requires_grad_(dy is not None)
    g64 = g.detach().double().requires_grad_(dy is not None)
    b64 = b.detach().double().requires_grad_(dy is not None)
    y = F.layer_norm(x, (D,), g64, b64, eps)
    out = {"y": y.detach(), "mean": x.detach().mean(-1),
           "rstd": torch.rsqrt(x.detach().var(-1, unbiased=False) + eps)}
    if dy is not None:
        dx, dg, db = torch.autograd.grad((y * dy.detach().double().reshape(-1, D)).sum(), (x, g64, b64))
        dxd = dx * keep.reshape(-1, D) if keep is not None else dx
        out.update(dx=dx, dgamma=dg, dbeta=db, dxd=dxd, dbias=dxd.sum(0))
    return out


def embed_ln_input(x, pos, tt):
    """(x + pos[row % S]) + tt in fp32, rounded once (csrc/transformer.hip embed_layernorm_fwd)."""
    D = x.shape[-1]
    S = pos.numel() // D
    xs = x.float().reshape(-1, S, D) + pos.float().reshape(1, S, D) + tt.float().reshape(1, 1, D)
    return xs.reshape(x.shape).to(x.dtype)


# ------------------------------------------------------------------------------ element-wise ops
def gelu(x, dy=None):
    """erf GELU in fp64: [y, dx or None] (dx by autograd)."""
    x64 = x.detach().double().requires_grad_(dy is not None)
    y = 0.5 * x64 * (1.0 + torch.erf(x64 * 0.7071067811865476))
    dx = torch.autograd.grad((y * dy.detach().double()).sum(), x64)[0] if dy is not None else None
    return [y.detach(), dx]


def tanh(x, dy=None):
    x64 = x.detach().double().requires_grad_(dy is not None)
    y = torch.tanh(x64)
    dx = torch.autograd.grad((y * dy.detach().double()).sum(), x64)[0] if dy is not None else None
    return [y.detach(), dx]


def add(a, b):
    return a.double() + b.double()


def embedding(ids, W, dy=None, padding_idx=0, dW0=None):
    """Gather W[ids]; with dy, the scatter-add of dy into dW0 (zeros when None) by autograd, rows
    of ``padding_idx`` skipped."""
    W64 = W.detach().double().requires_grad_(dy is not None)
    y = W64[ids]
    dW = None
    if dy is not None:
        keep = (ids != padding_idx).unsqueeze(-1).double()
        dW, = torch.autograd.grad((y * dy.detach().double() * keep).sum(), W64)
        if dW0 is not None:
            dW = dW + dW0.double()
    return [y.detach(), dW]


def masked_mean(x, ids, dy=None):
    """Mean over the steps with ids > 0 (0 for a row without one); dx by autograd."""
    x64 = x.detach().double().requires_grad_(dy is not None)
    m = (ids > 0).double().unsqueeze(-1)
    y = (x64 * m).sum(1) / m.sum(1).clamp_min(1.0)
    dx = torch.autograd.grad((y * dy.detach().double()).sum(), x64)[0] if dy is not None else None
    return [y.detach(), dx]


# ------------------------------------------------------------------------------ shared test cases
# The shapes, masks and inputs of tests/test_text_truth_cpu.py (reference floors) and
# tests/test_text_truth_gpu.py (kernels): built on the CPU from a fixed seed so both judge the same
# numbers.
LSTM_SHAPES = [(1, 1, 64), (32, 2, 64), (5, 7, 32), (17, 33, 96), (3, 9, 192), (8, 16, 512)]
LSTM_SHAPES_F32 = LSTM_SHAPES + [(9, 5, 1)]
ATTN_S = [32, 64, 96, 128]
ATTN_S_F32 = [1, 33, 256]
LN_SHAPES = [(1, 8), (3, 64), (5, 256), (13, 520), (13, 768), (5, 1024), (3, 1280), (5, 2048)]
EMBED_LN_SHAPES = [(1, 1, 256), (3, 5, 520)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def lstm_ids(B, S, gen):
    """Tail padding S - (7i) % S; row 2 all pad, row 3 a leading pad, row 4 a hole in the middle
    (rows the batch does not have are skipped)."""
    ids = torch.randint(1, 1000, (B, S), generator=gen)
    for i in range(B):
        ids[i, max(1, S - (7 * i) % S):] = 0
    if B > 2:
        ids[2] = 0
    if B > 3:
        ids[3, :max(1, S // 3)] = 0
        ids[3, -1] = 7
    if B > 4:
        ids[4] = 5
        ids[4, S // 2:S // 2 + max(1, S // 4)] = 0
    return ids


def lstm_case(B, S, H, dtype=torch.bfloat16):
    gen = _gen(1000 * B + 10 * S + H)
    ids = lstm_ids(B, S, gen)
    gx = (torch.randn(B, S, 2, 4 * H, generator=gen) * 0.5).to(dtype)
    whh = (torch.randn(2, 4 * H, H, generator=gen) / H ** 0.5).to(dtype)
    dh = torch.randn(B, S, 2 * H, generator=gen).to(dtype)
    return gx, whh, ids, dh


def attn_ids(S, lens, gen):
    ids = torch.randint(1, 30522, (len(lens), S), generator=gen)
    for i, l in enumerate(lens):
        ids[i, l:] = 0
    return ids


def attn_lens(S, p):
    """Sequence lengths of one case.  The one-key sequence is a p = 0 case only: under dropout its
    dQ / dK cancel to exactly 0 in the truth while any bf16 evaluation leaves rounding noise."""
    return [S, max(1, S - 1), min(S, 17), 1 if p == 0 else min(S, 5)]


def attn_case(S, p, with_ids=True, H=2, dtype=torch.bfloat16):
    gen = _gen(77 * S + int(100 * p) + (0 if with_ids else 5))
    lens = attn_lens(S, p)
    B = len(lens)
    ids = attn_ids(S, lens, gen) if with_ids else None
    qkv = torch.randn(B * S, 3 * 64 * H, generator=gen).to(dtype)
    dctx = torch.randn(B * S, 64 * H, generator=gen).to(dtype)
    return qkv, ids, dctx, B, lens


# Long sequences (128 < S <= 512, the key-tiled bf16 kernels, 64-key tiles): 160 ends in a partial
# tile and leaves half of its last 64-query block idle, 192 is an odd number of tiles, 256 / 384 /
# 512 are four to eight whole ones.
ATTN_S_LONG = [160, 192, 256, 384, 512]
# The key-tiled fp32 kernels (256 < S <= 512, any length): 257 spills one query and one key into a
# fifth tile, 300 ends in a partial tile, 320 is five whole tiles, 384 / 512 six and eight, 509 is odd
# and leaves the last 4-key MFMA k-group partial.
ATTN_S_F32_LONG = [257, 300, 320, 384, 509, 512]


def attn_case_long(S, p, with_ids=True, H=2, dtype=torch.bfloat16):
    """Five sequences: ``attn_lens(S, p)`` and a fifth whose valid keys are [136, S - 3) only, so
    its first 128 keys (two whole key tiles) are padding (the online softmax must forget those
    tiles' provisional probabilities) and a short tail pad follows.  Its length is reported as S - 3: the runners
    only ask whether a sequence has exactly one key."""
    gen = _gen(91 * S + int(100 * p) + (0 if with_ids else 5))
    lens = attn_lens(S, p) + [S - 3]
    B = len(lens)
    ids = None
    if with_ids:
        ids = attn_ids(S, lens, gen)
        ids[4, :136] = 0
    qkv = torch.randn(B * S, 3 * 64 * H, generator=gen).to(dtype)
    dctx = torch.randn(B * S, 64 * H, generator=gen).to(dtype)
    return qkv, ids, dctx, B, lens


def ln_case(M, D, with_r, dtype=torch.bfloat16):
    """When M >= 3 the last row is constant (x = 1.5, r = 0.25: every partial sum is exact)."""
    gen = _gen(31 * M + D + (1 if with_r else 0))
    x = torch.randn(M, D, generator=gen).to(dtype)
    r = torch.randn(M, D, generator=gen).to(dtype) if with_r else None
    if M >= 3:
        x[-1] = 1.5
        if r is not None:
            r[-1] = 0.25
    g = torch.rand(D, generator=gen) + 0.5
    b = torch.randn(D, generator=gen)
    dy = torch.randn(M, D, generator=gen).to(dtype)
    return x, r, g, b, dy


def embed_ln_case(B, S, D, dtype=torch.bfloat16):
    gen = _gen(B + 10 * S + D)
    x = torch.randn(B * S, D, generator=gen).to(dtype)
    pos = torch.randn(S, D, generator=gen).to(dtype)
    tt = torch.randn(D, generator=gen).to(dtype)
    return x, pos, tt, torch.rand(D, generator=gen) + 0.5, torch.randn(D, generator=gen)


def act_case(n, dtype=torch.bfloat16):
    gen = _gen(n)
    x = (torch.randn(n, generator=gen) * 2).to(dtype)
    x[:8] = torch.tensor([0.0, -0.0, 10.0, -10.0, 40.0, -40.0, 1.0, -1.0]).to(dtype)
    dy = torch.randn(n, generator=gen).to(dtype)
    return x, dy


def embedding_cases(E, dtype=torch.bfloat16):
    """(name, ids, W, dy, dW0): random ids with padding, every row the same token, all padding."""
    gen = _gen(E)
    V, B, S = 50, 3, 11
    W = torch.randn(V, E, generator=gen).to(dtype)
    dy = torch.randn(B, S, E, generator=gen).to(dtype)
    dW0 = torch.randn(V, E, generator=gen)
    rnd = torch.randint(0, V, (B, S), generator=gen)
    rnd[:, 8:] = 0
    return [("random", rnd, W, dy, dW0), ("one-token", torch.full((B, S), 7), W, dy, dW0),
            ("all-pad", torch.zeros(B, S, dtype=torch.int64), W, dy, dW0)]


def masked_mean_case(D, S, dtype=torch.bfloat16):
    """Row 1 is all pad; row 0 full; row 2 keeps its first ceil(S/2) steps."""
    gen = _gen(D + S)
    B = 3
    ids = torch.randint(1, 100, (B, S), generator=gen)
    ids[1] = 0
    ids[2, (S + 1) // 2:] = 0
    x = torch.randn(B, S, D, generator=gen).to(dtype)
    dy = torch.randn(B, D, generator=gen).to(dtype)
    return x, ids, dy
