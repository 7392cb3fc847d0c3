"""The packed (padding-free) attention kernels (csrc/attn_tiled.h over a cu_seqlens table) against the
fp64 truth of ``pcmp.ops.truth_packed`` on ``packed_case`` (11 sequences of 1 .. 512 tokens, H = 2,
max_s = 512, 64 rows of no sequence), held element by element to ``PACKED_BOUNDS`` of
tests/test_attention_packed_cpu.py; the exact zeros; bitwise equality with the padded tiled kernels on
the [B, max_s] rectangle of the same sequences (same seed, offset and salt, so the same dropout draw);
isolation of the segments; ``max_s`` as a mere bound; run-to-run determinism and the salt; the host
checks; a packed 2-layer BERT and the entry point's ``--pack``."""
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.data.imdb import pack_batch
from pcmp.ops import ref, truth as T, truth_packed as TP, truth_run as R

from test_attention_packed_cpu import PACKED_BOUNDS, PACKED_VARIANTS
from test_model_parity_gpu import _bf16_noise_check, _text_grads

pytestmark = pytest.mark.gpu
H = TP.PACKED_H


def ops():
    return torch.ops.pcmp


def _finite(*ts):
    for t in ts:
        assert torch.isfinite(t.float()).all()


def _run(gpu, case, p, max_s=None, salt=2):
    """(ctx, lse, dqkv) of the packed ops on one case."""
    qkv, pb, ids, dctx, _ = case
    qkv, ids, dctx, cu = R.to(gpu, qkv, ids, dctx, pb.cu)
    max_s = max_s or pb.max_s
    st = R._salt(gpu, salt) if p > 0 else None
    ctx, lse = ops().attention_fwd(qkv, ids, pb.B, max_s, H, p, R.AT_SEED, R.AT_OFF, st, cu)
    dq = ops().attention_bwd(dctx, qkv, ctx, lse, ids, pb.B, max_s, H, p, R.AT_SEED, R.AT_OFF, st, cu)
    return ctx, lse, dq


@pytest.mark.parametrize("p,with_ids", PACKED_VARIANTS)
def test_attention_packed_truth(gpu, p, with_ids):
    case = TP.packed_case(p, with_ids)
    res, one_key, raw, _ = TP.run_attention_packed(ops(), case, p, dev=gpu)
    torch.cuda.synchronize()
    _finite(*raw)
    R.check(PACKED_BOUNDS, R.attn_op(p), res, f"packed p={p} ids={with_ids}")
    ctx, lse, dq = raw
    pb, ids = case[1], case[2]
    used = int(pb.cu[-1])
    assert used == 1728 and pb.rows == 1792
    for name, x in (("ctx", ctx[used:]), ("lse", lse[:, used:]), ("dqkv", dq[used:])):
        assert float(x.float().abs().max()) == 0.0, f"{name} at the rows of no sequence"
    if with_ids:
        masked = (ids <= 0)[:used].to(gpu)
        assert int(masked.sum()) == 1728 - sum(case[4])
        kv = dq[:used].reshape(used, 3, H * 64)[:, 1:]
        assert float(kv[masked].float().abs().max()) == 0.0, "dK / dV at masked keys"
    if with_ids and p == 0:
        (a, t, s), = one_key["dqk"]
        assert a.shape[0] == 32
        print("one-key dQ/dK: max |kernel|", float(a.float().abs().max()))
        T.assert_elementwise(a, t, s, 1.0, "one-key dQ / dK")
    for a, b in zip(raw, _run(gpu, case, p)):
        assert torch.equal(a, b), "run-to-run determinism"


def _padded_twin(gpu, case, p, max_s):
    """The padded [B, max_s] call on the same sequences (dctx zero outside the segments), gathered
    back to the packed rows: (ctx, lse, dqkv, inside rows)."""
    qkv, pb, ids, dctx, _ = case
    Tn = qkv.shape[0]
    rows, inside = ref.packed_rows(pb.cu, pb.B, max_s, Tn)
    pq, pd = ref._to_padded(qkv, rows).to(gpu), ref._to_padded(dctx, rows).to(gpu)
    pid = ref._packed_key_ids(ids, rows, inside).to(gpu)
    st = R._salt(gpu, 2) if p > 0 else None
    old = ops().set_knob("attn_tiled", 1)
    try:
        ctx, lse = ops().attention_fwd(pq, pid, pb.B, max_s, H, p, R.AT_SEED, R.AT_OFF, st)
        dq = ops().attention_bwd(pd, pq, ctx, lse, pid, pb.B, max_s, H, p, R.AT_SEED, R.AT_OFF, st)
        torch.cuda.synchronize()
    finally:
        ops().set_knob("attn_tiled", old)
    rows, inside = rows.to(gpu), inside.to(gpu)
    lse_p = lse.new_zeros(H, Tn)
    lse_p[:, rows[inside]] = lse.view(pb.B, H, max_s).transpose(0, 1)[:, inside]
    return ref._to_packed(ctx, rows, inside, Tn), lse_p, ref._to_packed(dq, rows, inside, Tn)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("max_s,lens", [(512, None), (128, [1, 33, 64, 128])])
def test_packed_is_bitwise_the_padded_tiled_kernels(gpu, p, max_s, lens):
    """A masked key tile contributes probabilities of exactly 0 once a valid key has been seen and a pad
    query contributes dO = 0, so both layouts add the same non-zero terms in the same order."""
    case = TP.packed_case(p, True, lens=lens, max_s=max_s)
    got = _run(gpu, case, p)
    want = _padded_twin(gpu, case, p, max_s)
    for name, a, b in zip(("ctx", "lse", "dqkv"), got, want):
        assert a.shape == b.shape
        print(name, "differing elements", int((a != b).sum()), "of", a.numel())
        assert torch.equal(a, b), f"{name}: packed differs from the padded tiled kernels"


def test_packed_segments_are_isolated(gpu):
    """Other values in one middle segment's rows leave every other segment's results bit for bit."""
    p = 0.1
    qkv, pb, ids, dctx, lens = TP.packed_case(p, True)
    c = pb.cu.tolist()
    b = 7                                                      # 130 tokens, rows 352 .. 512
    assert c[b + 1] - c[b] == 160
    qkv2 = qkv.clone()
    qkv2[c[b]:c[b + 1]] = (torch.randn(160, qkv.shape[1], generator=T._gen(11)) * 3).to(qkv.dtype)
    r1 = _run(gpu, (qkv, pb, ids, dctx, lens), p)
    r2 = _run(gpu, (qkv2, pb, ids, dctx, lens), p)
    keep = torch.ones(pb.rows, dtype=torch.bool, device=gpu)
    keep[c[b]:c[b + 1]] = False
    for name, x, y in zip(("ctx", "lse", "dqkv"), r1, r2):
        if name == "lse":
            x, y = x.t(), y.t()
        assert torch.equal(x[keep], y[keep]), f"{name} of another segment changed"
        assert not torch.equal(x[~keep], y[~keep])


def test_packed_max_s_is_a_bound(gpu):
    """Without dropout max_s only sizes the grid: 480 (>= the longest segment here) gives the bits of 512."""
    lens = TP.PACKED_TOKENS[:-1] + [470]
    case = TP.packed_case(0.0, True, lens=lens)
    assert int((case[1].cu[1:] - case[1].cu[:-1]).max()) == 480
    for a, b in zip(_run(gpu, case, 0.0, 512), _run(gpu, case, 0.0, 480)):
        assert torch.equal(a, b)


def test_packed_salt(gpu):
    case = TP.packed_case(0.1, True)
    a, b, c = _run(gpu, case, 0.1, salt=2)[0], _run(gpu, case, 0.1, salt=3)[0], _run(gpu, case, 0.1, salt=2)[0]
    assert not torch.equal(a, b) and torch.equal(a, c)


def test_packed_host_checks(gpu):
    B, Tn = 2, 64
    qkv = torch.zeros(Tn, 3 * 64 * H, device=gpu, dtype=torch.bfloat16)
    cu = torch.tensor([0, 32, 64], device=gpu, dtype=torch.int32)
    ctx = torch.zeros(Tn, 64 * H, device=gpu, dtype=torch.bfloat16)
    lse = torch.zeros(H, Tn, device=gpu)

    def both(match, q, c, max_s, cx=ctx, ls=lse):
        with pytest.raises(RuntimeError, match=match):
            ops().attention_fwd(q, None, B, max_s, H, 0.0, 0, 0, None, c)
        with pytest.raises(RuntimeError, match=match):
            ops().attention_bwd(cx, q, cx, ls, None, B, max_s, H, 0.0, 0, 0, None, c)

    both("attention_packed: bf16 only", qkv.float(), cu, 64, ctx.float())
    both("T must be a multiple of 32", qkv[:48].contiguous(), cu, 64, ctx[:48].contiguous(), lse[:, :48].contiguous())
    both("max_s must be a multiple of 32 and <= 512", qkv, cu, 544)
    both("cu must have B \\+ 1 entries", qkv, cu[:2].contiguous(), 64)
    ops().attention_fwd(qkv, None, B, 64, H, 0.0, 0, 0, None, cu)       # the well-formed call runs
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,S,D", [(3, 32, 768), (3, 5, 520)])
def test_embed_layernorm_packed(gpu, B, S, D):
    """The position row comes from pos_ids[row]: with pos_ids = row % S the lane-dense (D = 768) and the
    generic (D = 520) kernels give the bits of embed_layernorm_fwd; with a packed batch's positions
    every row is the padded op's row of the same token."""
    x, pos, tt, g, b = R.to(gpu, *T.embed_ln_case(B, S, D))
    want = ops().embed_layernorm_fwd(x, pos, tt, g, b, 1e-12)
    table = torch.cat([pos.reshape(S, D), torch.full((3, D), 7.0, device=gpu, dtype=pos.dtype)]).contiguous()
    pos_ids = (torch.arange(B * S, device=gpu) % S).contiguous()
    got = ops().embed_layernorm_fwd(x, table, tt, g, b, 1e-12, pos_ids)
    for a, w in zip(got, want):
        assert torch.equal(a, w)
    perm = torch.randperm(B * S, generator=T._gen(4)).to(gpu)        # any row order: a gather of the rows
    got2 = ops().embed_layernorm_fwd(x[perm].contiguous(), table, tt, g, b, 1e-12, pos_ids[perm].contiguous())
    for a, w in zip(got2, want):
        assert torch.equal(a, w[perm])
    with pytest.raises(RuntimeError, match="embed_layernorm_packed: bf16 only"):
        ops().embed_layernorm_fwd(x.float(), table.float(), tt.float(), g, b, 1e-12, pos_ids)


def test_bert_attn_fused_packed_matches_op_sequence(gpu):
    """bert_attn_fwd(..., cu) (one native dispatch) == Linear, attention_fwd(..., cu), Linear, dropout +
    residual + LayerNorm issued one op at a time, bitwise, with dropout 0.1: the packed counterpart of
    test_bert_fused_sublayer_ops_match_op_sequence (tests/test_text_kernels_gpu.py)."""
    Hb, D = 12, 768
    pad_ids = T.attn_ids(128, [1, 33, 64, 128], T._gen(8))
    pb = pack_batch(pad_ids, (pad_ids > 0).long(), 32, 32)
    assert (pb.cu[1:] - pb.cu[:-1]).tolist() == [32, 64, 64, 128] and pb.rows == 288 and pb.max_s == 128
    pb = pb.to(gpu)
    Tn, o = pb.rows, ops()
    torch.manual_seed(6)
    h = (torch.randn(Tn, D, device=gpu) * 0.5).bfloat16()
    wq, bq = (torch.randn(3 * D, D, device=gpu) * 0.02).bfloat16(), torch.randn(3 * D, device=gpu) * 0.02
    wo, bo = (torch.randn(D, D, device=gpu) * 0.02).bfloat16(), torch.randn(D, device=gpu) * 0.02
    g, b = torch.rand(D, device=gpu) + 0.5, torch.randn(D, device=gpu) * 0.1

    def lin(x, w, bias):
        return o.conv_fwd(x.view(Tn, 1, 1, -1), w.view(w.shape[0], 1, 1, -1), 1, 0, bias, None, False, False)[0].view(Tn, -1)

    fa = o.bert_attn_fwd(h, pb.ids, wq, bq, wo, bo, g, b, pb.B, pb.max_s, Hb, 0.1, 11, 3 << 32, 0.1, 11, 4 << 32, 1e-12,
                         None, pb.cu)
    qkv = lin(h, wq, bq)
    ctx, lse = o.attention_fwd(qkv, pb.ids, pb.B, pb.max_s, Hb, 0.1, 11, 3 << 32, None, pb.cu)
    y = o.layernorm_fwd(lin(ctx, wo, bo), h, g, b, 1e-12, 0.1, 11, 4 << 32)
    assert ctx.shape == (Tn, D) and lse.shape == (Hb, Tn)
    _finite(*fa)
    for name, u, v in zip(("h1", "qkv", "ctx", "lse", "xs", "mean", "rstd"), fa, [y[0], qkv, ctx, lse] + list(y[1:])):
        assert torch.equal(u, v), name


def test_cu_none_changes_nothing(gpu):
    """attention_fwd / attention_bwd with an explicit trailing cu = None are the 9- and 12-argument calls,
    bitwise, on the padded shape of test_bert_fused_sublayer_ops_match_op_sequence with B = 2 (dropout and
    salt on); an fp32 qkv with cu is rejected before the fp32 dispatch."""
    B, S, Hb, D, p = 2, 128, 12, 768, 0.1
    gen = T._gen(9)
    qkv = torch.randn(B * S, 3 * D, generator=gen).bfloat16().to(gpu)
    dctx = torch.randn(B * S, D, generator=gen).bfloat16().to(gpu)
    ids = T.attn_ids(S, [128, 90], gen).to(gpu)
    st = R._salt(gpu, 2)
    ctx, lse = ops().attention_fwd(qkv, ids, B, S, Hb, p, R.AT_SEED, R.AT_OFF, st)
    dq = ops().attention_bwd(dctx, qkv, ctx, lse, ids, B, S, Hb, p, R.AT_SEED, R.AT_OFF, st)
    ctx2, lse2 = ops().attention_fwd(qkv, ids, B, S, Hb, p, R.AT_SEED, R.AT_OFF, st, None)
    dq2 = ops().attention_bwd(dctx, qkv, ctx, lse, ids, B, S, Hb, p, R.AT_SEED, R.AT_OFF, st, None)
    _finite(ctx, lse, dq)
    assert torch.equal(ctx, ctx2) and torch.equal(lse, lse2) and torch.equal(dq, dq2)
    cu = torch.tensor([0, S, 2 * S], device=gpu, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="attention_packed: bf16 only"):
        ops().attention_fwd(qkv.float(), ids, B, S, Hb, 0.0, 0, 0, None, cu)
    with pytest.raises(RuntimeError, match="attention_packed: bf16 only"):
        ops().attention_bwd(dctx.float(), qkv.float(), ctx.float(), lse, ids, B, S, Hb, 0.0, 0, 0, None, cu)


def _bert2(gpu):
    from pcmp.models.bert import BertConfig, BertForSequenceClassification
    torch.manual_seed(0)
    return BertForSequenceClassification(BertConfig(num_hidden_layers=2, hidden_dropout_prob=0.0,
                                                    attention_probs_dropout_prob=0.0)).to(gpu).train()


def test_bert_packed_grads_at_bf16_noise_level(gpu):
    """The criterion of test_bert_long_grads_at_bf16_noise_level on a PackedBatch of the same batch, and
    the packed fp32 reference loss against the padded one."""
    m = _bert2(gpu)
    g = torch.Generator(device=gpu).manual_seed(2)
    ids = torch.randint(1000, 30522, (4, 256), device=gpu, generator=g)
    for i, L in enumerate([256, 200, 131, 9]):
        ids[i, L:] = 0
    y = torch.randint(0, 2, (4,), device=gpu, generator=g)
    pb = pack_batch(ids.cpu(), (ids > 0).long().cpu(), 32, 256).to(gpu)
    assert pb.rows == 768 and pb.max_s == 256
    _bf16_noise_check(m, lambda: m(pb, None, None, y)[0], "bert packed")
    l_packed, _ = _text_grads(m, lambda: m(pb, None, None, y)[0], "torch", fp32=True)
    l_padded, _ = _text_grads(m, lambda: m(ids, None, (ids > 0).long(), y)[0], "torch", fp32=True)
    print("fp32 reference loss: packed %.7f padded %.7f" % (l_packed, l_padded))
    assert abs(l_packed - l_padded) <= 1e-5 * abs(l_padded)


def test_entrypoint_pack(gpu, tmp_path):
    """--pack with dropout on: the fused packed path in training, validation and test through the packed
    eval."""
    import pytorch_on_language_distr as entry
    out = tmp_path / "rec.json"
    rc = entry.main(["--model", "bert", "--layers", "2", "--max-len", "200", "--pack", "--batch-size", "8",
                     "--train-size", "64", "--test-size", "16", "--epochs", "1", "--json", str(out)])
    assert rc == 0
    rec = json.loads(out.read_text().strip().splitlines()[-1])
    assert rec["model"] == "bert" and len(rec["train_loss"]) == 1
    assert all(l == l and abs(l) < 1e3 for l in rec["train_loss"]), rec["train_loss"]
    pk = rec["packing"]
    assert pk["rows"] > 0 and pk["rows"] % 1024 == 0 and 0 < pk["tokens"] <= pk["rows"] and pk["padded_rows"] == 57 * 224
