"""The text-path HIP kernels (csrc/rnn.hip, transformer.hip, embed.h, text_f32.hip) against the fp64
autograd truths of ``pcmp.ops.truth``, element by element, at the smallest shapes that reach each
code path.  Every case runs the forward kernel, then the backward kernel on the forward's own saved
outputs.  bf16 outputs are held to ``BOUNDS`` of tests/test_text_truth_cpu.py (k times
``1e-2*|t| + 5e-3*max_seg|t|`` for every element); fp32 outputs to the norm-relative criterion of
tests/test_text_f32_gpu.py, per segment, against the fp64 truth."""
import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import truth as T, truth_run as R

from test_text_truth_cpu import BOUNDS     # the floor / bound table lives with the test that checks it

pytestmark = pytest.mark.gpu


def ops():
    return torch.ops.pcmp


def _guard(sync):
    torch.cuda.synchronize()
    assert int(sync[2].item()) == 0, "barrier timeout"


def _finite(*ts):
    for t in ts:
        if t is not None:
            assert torch.isfinite(t.float()).all()


# ------------------------------------------------------------------------------ LSTM
@pytest.mark.parametrize("B,S,H", T.LSTM_SHAPES)
def test_lstm(gpu, B, S, H):
    """lstm_v2 = 0 (round-1 kernels), 1 (role-split) and 2 (default: v2 forward, partial-exchange
    backward).  The forward takes the v2 kernel only when H is a multiple of 64; (5, 7, 32) and
    (17, 33, 96) fall back to the round-1 forward at every knob.  The round-1 backward keeps the
    whole [32][4H] dgates tile in LDS (384*H + 6 KB <= 160 KB: H <= 384), so at H = 512 lstm_v2 = 0
    has a forward only and its backward must refuse with the LDS-budget error."""
    case = T.lstm_case(B, S, H)
    gx, whh, ids, dh = R.to(gpu, *case)
    truth = T.lstm(gx, whh, ids, dh)
    pad = (ids <= 0)
    runs = {}
    old = ops().set_knob("lstm_v2", 0)
    try:
        for v in (0, 1, 2, 2):
            ops().set_knob("lstm_v2", v)
            has_bwd = v != 0 or H <= 384
            res, raw = R.run_lstm(ops(), case, gpu, _guard, truth, has_bwd)
            runs.setdefault(v, []).append(raw)
            R.check(BOUNDS, "lstm", res, f"{(B, S, H)} lstm_v2={v}")
            if not has_bwd:
                with pytest.raises(RuntimeError, match="LDS budget"):
                    ops().lstm_seq_bwd(dh, raw[1], raw[2], whh, ids)
                continue
            h, g, c, dg = raw
            assert float(dg[pad].float().abs().max() if pad.any() else 0.0) == 0.0, "dgates at padded steps"
            if B > 2:
                assert float(h[2].float().abs().max()) == 0.0 and float(dg[2].float().abs().max()) == 0.0
    finally:
        ops().set_knob("lstm_v2", old)
    for a, b in zip(*runs[2]):
        assert torch.equal(a, b), "lstm_v2 = 2 must be run-to-run deterministic"
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b), "lstm_v2 = 1 runs the round-1 arithmetic"


# ------------------------------------------------------------------------------ attention
def _attention(gpu, S, p, with_ids):
    case = T.attn_case(S, p, with_ids)
    B, lens = case[3], case[4]
    res, one_key, raw = R.run_attention(ops(), case, S, p, dev=gpu)
    torch.cuda.synchronize()
    _finite(*raw)
    R.check(BOUNDS, R.attn_op(p), res, f"S={S} p={p} ids={with_ids}")
    dq = T.seg_dqkv(raw[2], B, S, 2)[0]
    if with_ids:
        for b, l in enumerate(lens):
            assert float(dq[b, l:, 1:].float().abs().max() if l < S else 0.0) == 0.0, "dK / dV at padded keys"
    _, _, raw2 = R.run_attention(ops(), case, S, p, dev=gpu)
    for a, b in zip(raw, raw2):
        assert torch.equal(a, b)
    return one_key


@pytest.mark.parametrize("S", T.ATTN_S)
@pytest.mark.parametrize("p,with_ids", [(0.0, True), (0.1, True), (0.0, False)])
def test_attention(gpu, S, p, with_ids):
    """H = 2; lengths [S, S-1, 17, 1] at p = 0 and [S, S-1, 17, 5] at p = 0.1, and ids = None.  The
    dQ / dK of the one-key sequence are judged in test_attention_one_key_sequence."""
    _attention(gpu, S, p, with_ids)


@pytest.mark.parametrize("dtype,S", [(torch.bfloat16, S) for S in T.ATTN_S] + [(torch.float32, S) for S in T.ATTN_S_F32],
                         ids=[f"bf16-{S}" for S in T.ATTN_S] + [f"f32-{S}" for S in T.ATTN_S_F32])
def test_attention_one_key_sequence(gpu, dtype, S):
    """With one valid key P = 1, and the truth's dQ and dK are identically zero by the cancellation
    dP - D: the comparator takes nothing but exact zeros for a segment whose truth is zero (in fp32
    the norm-relative error of such a segment is likewise 0 or infinite).  The backward kernels form
    D = sum_j P_j dP_j from the very P and dP that dS uses (and the fp32 scores by the same explicit
    fused multiply-adds in forward and backward, so that P is exactly 1), which makes the
    cancellation exact."""
    case = T.attn_case(S, 0.0, True, 2, dtype)
    res, one_key, raw = R.run_attention(ops(), case, S, 0.0, dev=gpu)
    a, t, s = one_key["dqk"]
    print("one-key dQ/dK: max |kernel|", float(a.float().abs().max()), "nonzero", int((a != 0).sum()), "of", a.numel())
    if dtype == torch.float32:
        assert float(T.seg_rel(a, t, s).max()) < 1e-5
    else:
        T.assert_elementwise(a, t, s, 1.0, f"one-key dQ / dK S={S}")


def test_attention_all_pad_sequence(gpu):
    """A sequence with no valid key is outside the contract (``ref.attention_fwd``): its outputs are
    finite and the other sequences are bitwise what a batch without it gives."""
    S, H = 64, 2
    qkv, ids, dctx, B, _ = T.attn_case(S, 0.0)
    qkv, ids, dctx = R.to(gpu, qkv, ids, dctx)
    ids3 = torch.stack([ids[0], torch.zeros_like(ids[0]), ids[2]])

    def run(sel, idsel):
        n = len(sel)
        q = qkv.view(B, S, -1)[sel].reshape(n * S, -1).contiguous()
        d = dctx.view(B, S, -1)[sel].reshape(n * S, -1).contiguous()
        ctx, lse = ops().attention_fwd(q, idsel, n, S, H, 0.0, 0, 0)
        dq = ops().attention_bwd(d, q, ctx, lse, idsel, n, S, H, 0.0, 0, 0)
        return ctx.view(n, S, -1), lse.view(n, H, S), dq.view(n, S, -1)

    r3 = run([0, 1, 2], ids3)
    r2 = run([0, 2], ids3[[0, 2]].contiguous())
    torch.cuda.synchronize()
    _finite(*r3)
    for a, b in zip(r3, r2):
        assert torch.equal(a[[0, 2]], b)


# ------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("M,D", T.LN_SHAPES)
def test_layernorm(gpu, M, D):
    """KC = 1..4 of the lane-dense kernels (D = 256, 520 -> generic, 768, 1024), the generic kernels
    with one lane (D = 8), a partial vector (64, 520, 1280) and a full one (2048); row tails of the
    4-row forward and 8-row backward blocks; with and without the residual, p in {0, 0.1},
    layernorm_bwd accumulating or not, layernorm_bwd_fused with dbias where it exists."""
    for v in R.ln_variants(M, D):
        with_r, p, acc, fused, accmask = v
        case = T.ln_case(M, D, with_r)
        res, raw = R.run_layernorm(ops(), case, v, gpu)
        torch.cuda.synchronize()
        R.check(BOUNDS, "layernorm", res, f"{(M, D)} r={with_r} p={p} acc={acc} fused={fused} accmask={accmask}")
        y, xs, mean, rstd, dx, dxd = raw
        if M >= 3 and p == 0:     # the constant row: xhat = 0 exactly, so y = beta rounded
            assert torch.equal(y[-1], case[3].to(gpu).to(torch.bfloat16)), "constant row: y != bf16(beta)"
            _finite(dx[-1])
        if fused and p == 0:
            assert dxd.data_ptr() == dx.data_ptr()


@pytest.mark.parametrize("B,S,D", T.EMBED_LN_SHAPES)
def test_embed_layernorm(gpu, B, S, D):
    res = R.run_embed_layernorm(ops(), T.embed_ln_case(B, S, D), gpu)
    torch.cuda.synchronize()
    R.check(BOUNDS, "embed_layernorm", res, f"{(B, S, D)}")
    a, t, _ = res["xs"]
    assert torch.equal(a.double(), t.double())      # (x + pos) + tt in fp32, rounded once


# ------------------------------------------------------------------------------ element-wise, pooling
@pytest.mark.parametrize("n", [8, 8 * 257])
def test_activations(gpu, n):
    case = T.act_case(n)
    res, got = R.run_activations(ops(), case, gpu)
    torch.cuda.synchronize()
    _finite(*got.values())
    R.check(BOUNDS, "act", res, f"n={n}")
    x = case[0].to(gpu)
    assert float(got["gelu_y"][x == -40].float().abs().max()) == 0.0
    assert torch.equal(got["tanh_y"][x.abs() == 40].float(), torch.sign(x[x.abs() == 40].float()))


@pytest.mark.parametrize("E", [8, 136])
def test_embedding(gpu, E):
    for case in T.embedding_cases(E):
        for acc in (False, True):
            res, raw = R.run_embedding(ops(), case, acc, gpu)
            _, raw2 = R.run_embedding(ops(), case, acc, gpu)
            torch.cuda.synchronize()
            R.check(BOUNDS, "embedding", res, f"E={E} {case[0]} acc={acc}")
            assert torch.equal(raw[0].cpu(), case[2][case[1]])            # the gather is a copy
            assert torch.equal(raw[0], raw2[0]) and torch.equal(raw[1], raw2[1])
            if case[0] == "all-pad":
                assert torch.equal(raw[1].cpu(), case[4] if acc else torch.zeros_like(case[4]))


@pytest.mark.parametrize("D", [8, 264])
@pytest.mark.parametrize("S", [1, 40])
def test_masked_mean(gpu, D, S):
    res, (y, dx) = R.run_masked_mean(ops(), T.masked_mean_case(D, S), gpu)
    torch.cuda.synchronize()
    R.check(BOUNDS, "masked_mean", res, f"D={D} S={S}")
    assert float(y[1].float().abs().max()) == 0.0 and float(dx[1].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------ fp32 variants
def _check_f32(res, tol, what, tols=None):
    for n, v in res.items():
        for a, t, s in R.chunks(v):
            assert a.dtype == torch.float32, (n, a.dtype)
            e = float(T.seg_rel(a, t, s).max()) if a.numel() else 0.0
            lim = (tols or {}).get(n, tol)
            print("f32", what, n, "%.3g" % e)
            assert e < lim, f"{what} {n}: segment norm-relative error {e:.3g} >= {lim}"


@pytest.mark.parametrize("B,S,H", T.LSTM_SHAPES_F32)
def test_lstm_f32(gpu, B, S, H):
    res, raw = R.run_lstm(ops(), T.lstm_case(B, S, H, torch.float32), gpu, _guard)
    _check_f32(res, 1e-5, f"lstm {(B, S, H)}")
    ids = T.lstm_case(B, S, H, torch.float32)[2].to(gpu)
    assert float(raw[3][ids <= 0].abs().max() if (ids <= 0).any() else 0.0) == 0.0


@pytest.mark.parametrize("S,p", [(1, 0.0), (33, 0.0), (33, 0.1), (256, 0.0), (256, 0.1)])
def test_attention_f32(gpu, S, p):
    """S = 1 (every softmax is one key; p = 0 only, like every one-key sequence), 33 (odd) and 256
    (the fp32 kernels' limit).  dQ / dK of one-key sequences: test_attention_one_key_sequence."""
    case = T.attn_case(S, p, True, 2, torch.float32)
    res, one_key, raw = R.run_attention(ops(), case, S, p, dev=gpu)
    torch.cuda.synchronize()
    _finite(*raw)
    _check_f32(res, 1e-5, f"attention S={S} p={p}", {"lse": 1e-6})


@pytest.mark.parametrize("M,D", T.LN_SHAPES)
def test_layernorm_f32(gpu, M, D):
    for v in R.ln_variants(M, D):
        case = T.ln_case(M, D, v[0], torch.float32)
        res, raw = R.run_layernorm(ops(), case, v, gpu)
        torch.cuda.synchronize()
        _check_f32(res, 1e-5, f"layernorm {(M, D)} {v}")
        if M >= 3 and v[1] == 0:
            assert torch.equal(raw[0][-1], case[3].to(gpu)), "constant row: y != beta"
            _finite(raw[4][-1])


def test_elementwise_f32(gpu):
    for n in (8, 8 * 257):
        res, got = R.run_activations(ops(), T.act_case(n, torch.float32), gpu)
        _finite(*got.values())
        _check_f32(res, 1e-6, f"act n={n}")
    for case in T.embedding_cases(136, torch.float32):
        _check_f32(R.run_embedding(ops(), case, True, gpu)[0], 1e-6, f"embedding {case[0]}")
    _check_f32(R.run_masked_mean(ops(), T.masked_mean_case(264, 40, torch.float32), gpu)[0], 1e-6, "masked_mean")
