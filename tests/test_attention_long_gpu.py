"""The key-tiled bf16 attention kernels (csrc/attn_tiled.h, 128 < S <= 512) against the fp64 truth
of ``pcmp.ops.truth`` on ``attn_case_long`` (B = 5, H = 2; the fifth sequence's first 128 keys are
padding), held element by element to ``LONG_BOUNDS`` of tests/test_attention_long_cpu.py; the
contracts of docs/PARITY.md (exact zeros at padded keys and for the one-key sequence, bitwise
run-to-run determinism, an all-pad sequence that stays finite and invisible to its neighbours, the
salt); the same kernels on the short shapes through the knob ``attn_tiled``; the host's length
check; a 2-layer BERT at S = 256 and the entry point at ``--max-len 200`` (S = 224)."""
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import truth as T, truth_run as R

from test_attention_long_cpu import LONG_BOUNDS, LONG_VARIANTS
from test_model_parity_gpu import _bf16_noise_check
from test_text_truth_cpu import BOUNDS

pytestmark = pytest.mark.gpu


def ops():
    return torch.ops.pcmp


def _finite(*ts):
    for t in ts:
        assert torch.isfinite(t.float()).all()


@pytest.mark.parametrize("S", T.ATTN_S_LONG)
@pytest.mark.parametrize("p,with_ids", LONG_VARIANTS)
def test_attention_long(gpu, S, p, with_ids):
    case = T.attn_case_long(S, p, with_ids)
    ids, B = case[1], case[3]
    res, _, raw = R.run_attention(ops(), case, S, p, dev=gpu)
    torch.cuda.synchronize()
    _finite(*raw)
    R.check(LONG_BOUNDS, R.attn_op(p), res, f"S={S} p={p} ids={with_ids}")
    if with_ids:
        dq = T.seg_dqkv(raw[2], B, S, 2)[0]                  # [B, S, 3, H, 64]
        pad = (ids <= 0).to(gpu)
        assert pad[4, :128].all() and pad.any(1).sum() >= 4
        assert float(dq[:, :, 1:][pad].float().abs().max()) == 0.0, "dK / dV at padded keys"
    _, _, raw2 = R.run_attention(ops(), case, S, p, dev=gpu)
    for a, b in zip(raw, raw2):
        assert torch.equal(a, b), "run-to-run determinism"


@pytest.mark.parametrize("S", T.ATTN_S_LONG)
def test_attention_long_one_key_sequence(gpu, S):
    """P = 1 for the lone key in forward and backward (the same score bits) and D is formed from the
    same dP bits that dS subtracts it from: dQ and dK are exact zeros."""
    _, one_key, _ = R.run_attention(ops(), T.attn_case_long(S, 0.0), S, 0.0, dev=gpu)
    a, t, s = one_key["dqk"]
    assert a.shape[0] == 1 and a.numel() > 0
    print("one-key dQ/dK: max |kernel|", float(a.float().abs().max()), "nonzero", int((a != 0).sum()), "of", a.numel())
    T.assert_elementwise(a, t, s, 1.0, f"one-key dQ / dK S={S}")


def test_attention_long_all_pad_sequence(gpu):
    S, H = 256, 2
    qkv, ids, dctx, B, _ = T.attn_case_long(S, 0.0)
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


def test_tiled_kernels_on_short_shapes(gpu):
    """attn_tiled = 1 sends S <= 128 through the tiled kernels: judged on the short cases with the
    short bounds.  At 0 (the default) the register-resident kernels run, bit for bit what they gave
    before the knob was touched."""
    shapes = [(S, p, wi) for S in (32, 96, 128) for p, wi in LONG_VARIANTS]

    def run(S, p, wi):
        return R.run_attention(ops(), T.attn_case(S, p, wi), S, p, dev=gpu)

    before = {k: run(*k)[2] for k in shapes}
    old = ops().set_knob("attn_tiled", 1)
    try:
        differs = False
        for S, p, wi in shapes:
            case = T.attn_case(S, p, wi)
            res, one_key, raw = run(S, p, wi)
            torch.cuda.synchronize()
            _finite(*raw)
            R.check(BOUNDS, R.attn_op(p), res, f"tiled S={S} p={p} ids={wi}")
            if wi:
                dq = T.seg_dqkv(raw[2], case[3], S, 2)[0]
                assert float(dq[:, :, 1:][(case[1] <= 0).to(gpu)].float().abs().max()) == 0.0
            if wi and p == 0:
                T.assert_elementwise(*one_key["dqk"], 1.0, f"tiled one-key dQ / dK S={S}")
            differs |= not all(torch.equal(a, b) for a, b in zip(raw, before[(S, p, wi)]))
        assert differs, "attn_tiled = 1 must reach other kernels than the default"
    finally:
        ops().set_knob("attn_tiled", old)
    assert old == 0
    for k in shapes:
        for a, b in zip(run(*k)[2], before[k]):
            assert torch.equal(a, b), f"default path changed at {k}"


def test_attention_long_salt(gpu):
    S, p, H = 256, 0.1, 2
    qkv, ids, _, B, _ = T.attn_case_long(S, p)
    qkv, ids = R.to(gpu, qkv, ids)

    def fwd(v):
        return ops().attention_fwd(qkv, ids, B, S, H, p, R.AT_SEED, R.AT_OFF, torch.tensor([v], device=gpu))[0]

    a, b, c = fwd(2), fwd(3), fwd(2)
    assert not torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("S", [544, 200])
def test_attention_rejected_lengths(gpu, S):
    B, H = 1, 2
    qkv = torch.zeros(B * S, 3 * 64 * H, device=gpu, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="attention: S must be a multiple of 32 and <= 512"):
        ops().attention_fwd(qkv, None, B, S, H, 0.0, 0, 0)
    ctx = torch.zeros(B * S, 64 * H, device=gpu, dtype=torch.bfloat16)
    lse = torch.zeros(B * H, S, device=gpu)
    with pytest.raises(RuntimeError, match="attention_bwd: S must be a multiple of 32 and <= 512"):
        ops().attention_bwd(ctx, qkv, ctx, lse, None, B, S, H, 0.0, 0, 0)


def test_bert_long_grads_at_bf16_noise_level(gpu):
    """The criterion of test_bert_grads_at_bf16_noise_level at S = 256."""
    from pcmp.models.bert import BertConfig, BertForSequenceClassification
    torch.manual_seed(0)
    m = BertForSequenceClassification(BertConfig(num_hidden_layers=2, hidden_dropout_prob=0.0,
                                                 attention_probs_dropout_prob=0.0)).to(gpu).train()
    g = torch.Generator(device=gpu).manual_seed(2)
    ids = torch.randint(1000, 30522, (4, 256), device=gpu, generator=g)
    for i, L in enumerate([256, 200, 131, 9]):
        ids[i, L:] = 0
    y = torch.randint(0, 2, (4,), device=gpu, generator=g)
    _bf16_noise_check(m, lambda: m(ids, None, (ids > 0).long(), y)[0], "bert S=256")


def test_entrypoint_max_len_200(gpu, tmp_path):
    """--max-len 200 pads to S = 224: the fused bert_attn_fwd path with dropout on the tiled kernels."""
    import pytorch_on_language_distr as entry
    out = tmp_path / "rec.json"
    rc = entry.main(["--model", "bert", "--layers", "2", "--max-len", "200", "--batch-size", "8", "--train-size", "64",
                     "--test-size", "16", "--epochs", "1", "--json", str(out)])
    assert rc == 0
    rec = json.loads(out.read_text().strip().splitlines()[-1])
    assert rec["model"] == "bert" and len(rec["train_loss"]) == 1
    assert all(l == l and abs(l) < 1e3 for l in rec["train_loss"]), rec["train_loss"]
