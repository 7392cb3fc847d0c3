"""The key-tiled fp32 attention kernels (csrc/attn_tiled_f32.h, 256 < S <= 512, any length) against
the fp64 truth of ``pcmp.ops.truth`` on ``attn_case_long(S, p, with_ids, 2, torch.float32)`` (B = 5,
H = 2; the fifth sequence's first 128 keys are padding), held per segment to the project's fp32
attention bounds (``F32_LONG_BOUNDS`` of tests/test_attention_f32_long_cpu.py: seg_rel < 1e-5 for ctx
and dqkv, < 1e-6 for lse); the contracts of docs/PARITY.md (exact zeros at padded keys and for the
one-key sequence, bitwise run-to-run determinism, an all-pad sequence that stays finite and invisible
to its neighbours, the salt); the same kernels on the short shapes through the knob
``attn_f32_tiled``; the host's length check; a 2-layer fp32 BERT at S = 384 against the torch fp32
backend and the entry point at ``--dtype fp32 --max-len 300`` (S = 320)."""
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import truth as T, truth_run as R

from test_attention_f32_long_cpu import F32_LONG_BOUNDS, F32_LONG_VARIANTS
from test_text_f32_gpu import _check_model

pytestmark = pytest.mark.gpu

SHORT_S = (33, 64, 137, 256)


def ops():
    return torch.ops.pcmp


def _finite(*ts):
    for t in ts:
        assert t.dtype == torch.float32, t.dtype
        assert torch.isfinite(t).all()


def _check(res, p, what):
    """Every segment of every output below its bound; each figure is printed before it is judged."""
    for n, v in res.items():
        for a, t, s in R.chunks(v):
            assert a.dtype == torch.float32, (n, a.dtype)
            e = float(T.seg_rel(a, t, s).max()) if a.numel() else 0.0
            lim = F32_LONG_BOUNDS[(R.attn_op(p), n)][1]
            print("f32", what, n, "%.3g" % e)
            assert e < lim, f"{what} {n}: segment norm-relative error {e:.3g} >= {lim}"


def _padded_keys_zero(raw, ids, B, S, gpu):
    dq = T.seg_dqkv(raw[2], B, S, 2)[0]                  # [B, S, 3, H, 64]
    pad = (ids <= 0).to(gpu)
    assert pad.any()
    assert float(dq[:, :, 1:][pad].abs().max()) == 0.0, "dK / dV at padded keys"


def _one_key_zero(one_key, what):
    a, t, s = one_key["dqk"]
    assert a.shape[0] >= 1 and a.numel() > 0      # S = 1: every sequence is a one-key sequence
    print(what, "one-key dQ/dK: max |kernel|", float(a.abs().max()), "nonzero", int((a != 0).sum()), "of", a.numel())
    assert float(a.abs().max()) == 0.0, what
    T.assert_elementwise(a, t, s, 1.0, what)


@pytest.mark.parametrize("S", T.ATTN_S_F32_LONG)
@pytest.mark.parametrize("p,with_ids", F32_LONG_VARIANTS)
def test_attention_f32_long(gpu, S, p, with_ids):
    case = T.attn_case_long(S, p, with_ids, 2, torch.float32)
    ids, B = case[1], case[3]
    res, _, raw = R.run_attention(ops(), case, S, p, dev=gpu)
    torch.cuda.synchronize()
    _finite(*raw)
    _check(res, p, f"S={S} p={p} ids={with_ids}")
    if with_ids:
        assert (ids[4, :128] <= 0).all()
        _padded_keys_zero(raw, ids, B, S, gpu)
    _, _, raw2 = R.run_attention(ops(), case, S, p, dev=gpu)
    for a, b in zip(raw, raw2):
        assert torch.equal(a, b), "run-to-run determinism"


@pytest.mark.parametrize("S", T.ATTN_S_F32_LONG)
def test_attention_f32_long_one_key_sequence(gpu, S):
    """P = 1 for the lone key in forward and backward (the same score bits) and D is formed from the
    same dP bits that dS subtracts it from: dQ and dK are exact zeros."""
    _, one_key, _ = R.run_attention(ops(), T.attn_case_long(S, 0.0, True, 2, torch.float32), S, 0.0, dev=gpu)
    _one_key_zero(one_key, f"one-key dQ / dK S={S}")


@pytest.mark.parametrize("S", [300, 320])
def test_attention_f32_long_all_pad_sequence(gpu, S):
    """S = 320 is five whole tiles; at S = 300 the all-pad sequence's last tile holds -1e30 keys next
    to the -inf keys beyond S."""
    H = 2
    qkv, ids, dctx, B, _ = T.attn_case_long(S, 0.0, True, 2, torch.float32)
    qkv, ids, dctx = R.to(gpu, qkv, ids, dctx)
    ids3 = torch.stack([ids[0], torch.zeros_like(ids[0]), ids[4]])

    def run(sel, idsel):
        n = len(sel)
        q = qkv.view(B, S, -1)[sel].reshape(n * S, -1).contiguous()
        d = dctx.view(B, S, -1)[sel].reshape(n * S, -1).contiguous()
        ctx, lse = ops().attention_fwd(q, idsel, n, S, H, 0.0, 0, 0)
        dq = ops().attention_bwd(d, q, ctx, lse, idsel, n, S, H, 0.0, 0, 0)
        return ctx.view(n, S, -1), lse.view(n, H, S), dq.view(n, S, -1)

    r3 = run([0, 1, 4], ids3)
    r2 = run([0, 4], ids3[[0, 2]].contiguous())
    torch.cuda.synchronize()
    _finite(*r3)
    for a, b in zip(r3, r2):
        assert torch.equal(a[[0, 2]], b)


def test_attention_f32_long_salt(gpu):
    S, p, H = 320, 0.1, 2
    qkv, ids, _, B, _ = T.attn_case_long(S, p, True, 2, torch.float32)
    qkv, ids = R.to(gpu, qkv, ids)

    def fwd(v):
        return ops().attention_fwd(qkv, ids, B, S, H, p, R.AT_SEED, R.AT_OFF, torch.tensor([v], device=gpu))[0]

    a, b, c = fwd(2), fwd(3), fwd(2)
    assert not torch.equal(a, b) and torch.equal(a, c)


def test_f32_tiled_kernels_on_short_shapes(gpu):
    """attn_f32_tiled = 1 sends S <= 256 through the tiled kernels: judged on the short fp32 cases with
    the same bounds.  At 0 (the default) the whole-sequence-in-LDS kernels run, bit for bit what they
    gave before the knob was touched."""
    shapes = [(1, 0.0, True)] + [(S, p, wi) for p, wi in F32_LONG_VARIANTS for S in SHORT_S]

    def run(S, p, wi):
        return R.run_attention(ops(), T.attn_case(S, p, wi, 2, torch.float32), S, p, dev=gpu)

    before = {k: run(*k)[2] for k in shapes}
    old = ops().set_knob("attn_f32_tiled", 1)
    try:
        differs = False
        for S, p, wi in shapes:
            case = T.attn_case(S, p, wi, 2, torch.float32)
            res, one_key, raw = run(S, p, wi)
            torch.cuda.synchronize()
            _finite(*raw)
            _check(res, p, f"tiled S={S} p={p} ids={wi}")
            if wi and (case[1] <= 0).any():
                _padded_keys_zero(raw, case[1], case[3], S, gpu)
            if wi and p == 0:
                _one_key_zero(one_key, f"tiled one-key dQ / dK S={S}")
            differs |= not all(torch.equal(a, b) for a, b in zip(raw, before[(S, p, wi)]))
        assert differs, "attn_f32_tiled = 1 must reach other kernels than the default"
    finally:
        ops().set_knob("attn_f32_tiled", old)
    assert old == 0
    for k in shapes:
        for a, b in zip(run(*k)[2], before[k]):
            assert torch.equal(a, b), f"default path changed at {k}"


def test_attention_f32_rejected_lengths(gpu):
    B, H, S = 1, 2, 513
    qkv = torch.zeros(B * S, 3 * 64 * H, device=gpu)
    with pytest.raises(RuntimeError, match=r"attention \(fp32\): S <= 512"):
        ops().attention_fwd(qkv, None, B, S, H, 0.0, 0, 0)
    ctx = torch.zeros(B * S, 64 * H, device=gpu)
    lse = torch.zeros(B * H, S, device=gpu)
    with pytest.raises(RuntimeError, match=r"attention_bwd \(fp32\): head dim 64, S <= 512"):
        ops().attention_bwd(ctx, qkv, ctx, lse, None, B, S, H, 0.0, 0, 0)


@pytest.mark.parametrize("drop", [0.0, 0.1])
def test_bert2_fp32_long_grads_match_torch_fp32(gpu, drop):
    """The criterion of test_bert2_fp32_grads_match_torch_fp32 (worst gradient error < 1e-4) at
    S = 384, lengths [384, 300, 131, 9].  Measured on an MI355X: 1.08e-6 (dropout 0) and 9.8e-7
    (dropout 0.1), both at a qkv weight."""
    from pcmp.models.bert import BertConfig, BertForSequenceClassification
    torch.manual_seed(0)
    m = BertForSequenceClassification(BertConfig(num_hidden_layers=2, hidden_dropout_prob=drop,
                                                 attention_probs_dropout_prob=drop)).to(gpu).train()
    g = torch.Generator(device=gpu).manual_seed(2)
    ids = torch.randint(1000, 30522, (4, 384), device=gpu, generator=g)
    for i, L in enumerate([384, 300, 131, 9]):
        ids[i, L:] = 0
    y = torch.randint(0, 2, (4,), device=gpu, generator=g)
    _check_model(m, lambda: m(ids, None, (ids > 0).long(), y)[0], f"bert2 fp32 S=384 drop={drop}")


def test_entrypoint_fp32_max_len_300(gpu, tmp_path, monkeypatch):
    """--dtype fp32 --max-len 300 pads to S = 320: the fused bert_attn_fwd path with dropout on the tiled
    fp32 kernels."""
    import pytorch_on_language_distr as entry
    from pcmp.ops.kernels import K
    seen = set()   # (op, S, dtype) of every attention the run dispatches, fused or not

    def spy(name, s_at):
        real = getattr(K, name)

        def call(*args):
            seen.add((name, int(args[s_at]), args[0].dtype))
            return real(*args)

        monkeypatch.setattr(K, name, call)

    spy("bert_attn_fwd", 9)    # (h, ids, wq, bq, wo, bo, g, b, B, S, ...)
    spy("attention_fwd", 3)    # (qkv, ids, B, S, ...)
    out = tmp_path / "rec.json"
    rc = entry.main(["--model", "bert", "--dtype", "fp32", "--layers", "2", "--max-len", "300", "--batch-size", "8",
                     "--train-size", "64", "--test-size", "16", "--epochs", "1", "--json", str(out)])
    assert rc == 0
    rec = json.loads(out.read_text().strip().splitlines()[-1])
    assert seen and {(s, dt) for _, s, dt in seen} == {(320, torch.float32)}, seen
    assert rec["model"] == "bert" and rec["dtype"] == "fp32" and len(rec["train_loss"]) == 1
    assert all(l == l and abs(l) < 1e3 for l in rec["train_loss"]), rec["train_loss"]
