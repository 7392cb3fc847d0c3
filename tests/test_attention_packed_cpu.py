"""Packed (padding-free) BERT batches on the CPU: ``data.imdb.pack_batch``'s invariants, the floors of
``ops/ref.py`` against the fp64 truth on ``truth_packed.packed_case`` and the bounds the packed kernels
are held to in tests/test_attention_packed_gpu.py, the exact zeros of the one-key sequence and of the
masked keys, a packed BERT against the padded one, and the entry point's ``--pack``.

``PACKED_BOUNDS`` follows the rule of ``LONG_BOUNDS`` (tests/test_attention_long_cpu.py): per (op,
output) the floor is the worst ``norm_err`` of ``ref.py`` in bf16 over p in {0, 0.1}, with and without
``ids``, and the bound k satisfies 2 * floor <= k <= max(1, 4 * floor).  The bounds are the
existing attention rows' (1 for ctx / dqkv, 0.01 for the fp32 lse); ``truth_packed.PACKED_SEED`` is
the first draw of the case (seeds tried from 0 up; seed 1 gives a dqkv floor of 0.556) whose floors
are <= 0.5, so that k = 1 satisfies the rule.  No element is left out but the one-key sequence's
dQ / dK, exact zeros here.
"""
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.data.imdb import PackedBatch, pack_batch
from pcmp.ops import ref, truth as T, truth_packed as TP, truth_run as R

PACKED_VARIANTS = ((0.0, True), (0.1, True), (0.0, False), (0.1, False))

# (op, output): (floor of ops/ref.py on the CPU, bound k of the GPU tests)
PACKED_BOUNDS = {
    ("attention_p0", "ctx"): (0.371, 1.0), ("attention_p0", "lse"): (6.7e-6, 0.01), ("attention_p0", "dqkv"): (0.460, 1.0),
    ("attention_drop", "ctx"): (0.392, 1.0), ("attention_drop", "lse"): (6.5e-6, 0.01),
    ("attention_drop", "dqkv"): (0.432, 1.0),
}

_RUNS = {}


def ref_run(p, with_ids, seed=TP.PACKED_SEED):
    """run_attention_packed of ops/ref.py on the case, computed once per session."""
    key = (p, with_ids, seed)
    if key not in _RUNS:
        _RUNS[key] = TP.run_attention_packed(ref, TP.packed_case(p, with_ids, seed), p)
    return _RUNS[key]


def measure_packed_floors(seed=TP.PACKED_SEED):
    fl = {}
    for p, with_ids in PACKED_VARIANTS:
        for n, e in R.worst(ref_run(p, with_ids, seed)[0]).items():
            key = (R.attn_op(p), n)
            fl[key] = max(fl.get(key, 0.0), e)
    return fl


def _padded_case():
    """The case's lengths plus a full-width row, as a padded [B, 512] batch."""
    lens = TP.PACKED_TOKENS + [512]
    ids = T.attn_ids(512, lens, T._gen(5))
    return ids, (ids > 0).long(), lens


def test_pack_batch_invariants():
    ids, mask, lens = _padded_case()
    for rows_multiple in (256, 1024):
        pb = pack_batch(ids, mask, 32, rows_multiple)
        assert isinstance(pb, PackedBatch) and pb.B == len(lens) and pb.max_s == 512
        cu = pb.cu
        assert cu.dtype == torch.int32 and cu.shape == (len(lens) + 1,) and int(cu[0]) == 0
        seg = (cu[1:] - cu[:-1]).tolist()
        assert seg == [max(32, -(-l // 32) * 32) for l in lens]
        assert all(s >= 32 and s % 32 == 0 and s <= 512 for s in seg) and not bool((cu % 32).any())
        assert pb.rows % rows_multiple == 0 and pb.rows >= int(cu[-1]) and pb.rows - int(cu[-1]) < rows_multiple
        assert pb.ids.shape == (pb.rows,) and pb.ids.dtype == torch.int64
        assert pb.pos.shape == (pb.rows,) and pb.pos.dtype == torch.int64
        for b, s in enumerate(seg):
            assert torch.equal(pb.pos[int(cu[b]):int(cu[b + 1])], torch.arange(s))
        assert int(pb.pos[int(cu[-1]):].abs().sum()) == 0 and int(pb.ids[int(cu[-1]):].abs().sum()) == 0
        assert torch.equal(pb.unpack(), ids * mask)       # the ids at every valid token, 0 elsewhere
        assert pb.tokens == int(mask.sum()) == sum(lens)
    assert pack_batch(ids, mask, 32, 256).rows == 2304 and TP.packed_case(0.0)[1].rows == 1792
    assert int(TP.packed_case(0.0)[1].cu[-1]) == 1728
    # a narrower batch: max_s is the width rounded up to 32
    pb = pack_batch(ids[:5, :200], mask[:5, :200], 32, 256)
    assert pb.max_s == 224 and pb.rows == 256 and (pb.cu[1:] - pb.cu[:-1]).tolist() == [32, 32, 32, 32, 64]
    holed = mask.clone()
    holed[7, 3] = 0
    with pytest.raises(ValueError, match="holes"):
        pack_batch(ids, holed, 32, 256)
    lead = mask.clone()
    lead[9, 0] = 0
    with pytest.raises(ValueError, match="holes"):
        pack_batch(ids, lead, 32, 256)


def test_packed_reference_floors():
    fl = measure_packed_floors()
    print({k: float("%.3g" % v) for k, v in fl.items()})
    assert set(fl) == set(PACKED_BOUNDS), set(fl) ^ set(PACKED_BOUNDS)
    bad = []
    for key, f in fl.items():
        rec, k = PACKED_BOUNDS[key]
        if abs(f - rec) > 0.1 * rec + 0.02:
            bad.append((key, "floor moved", f, rec))
        if not (2 * f <= k and k <= max(1.0, 4 * f)) or not (2 * rec <= k and k <= max(1.0, 4 * rec)):
            bad.append((key, "2*floor <= k <= max(1, 4*floor) violated", f, k))
    assert not bad, bad


def test_ref_attention_with_cu_is_scatter_padded_gather():
    """ref.attention_fwd / attention_bwd given ``cu`` on packed_case(0.0) return, bit for bit, the definition
    spelled out here: scatter to the [B, max_s] rectangle, the same ops without ``cu``, gather back (what
    test_packed_reference_floors holds to the fp64 truth)."""
    qkv, pb, ids, dctx, _ = TP.packed_case(0.0)
    B, S, H, Tn = pb.B, pb.max_s, TP.PACKED_H, qkv.shape[0]
    ctx, lse, dq = ref_run(0.0, True)[2]
    rows, inside = ref.packed_rows(pb.cu, B, S, Tn)
    kid = ref._packed_key_ids(ids, rows, inside)
    pq = ref._to_padded(qkv, rows)
    pctx, plse = ref.attention_fwd(pq, kid, B, S, H, 0.0, R.AT_SEED, R.AT_OFF)
    pdq = ref.attention_bwd(ref._to_padded(dctx, rows), pq, ref._to_padded(ctx, rows), ref._lse_to_padded(lse, rows, B, H),
                            kid, B, S, H, 0.0, R.AT_SEED, R.AT_OFF)
    want_lse = plse.new_zeros(H, Tn)
    want_lse[:, rows[inside]] = plse.view(B, H, S).transpose(0, 1)[:, inside]
    assert ctx.shape == (Tn, 64 * H) and lse.shape == (H, Tn) and dq.shape == qkv.shape
    assert torch.equal(ctx, ref._to_packed(pctx, rows, inside, Tn)) and torch.equal(lse, want_lse)
    assert torch.equal(dq, ref._to_packed(pdq, rows, inside, Tn))


def test_packed_exact_zeros_reference():
    """dQ / dK of the one-key sequence, dK / dV at masked keys and every row of no sequence are exact
    zeros in the truth and in ops/ref.py."""
    res, one_key, (ctx, lse, dq), (tctx, tlse, tdq) = ref_run(0.0, True)
    (a, t, s), = one_key["dqk"]
    assert a.shape[0] == 32 and float(t.abs().max()) == 0.0
    print("one-key dQ / dK: max |ref|", float(a.float().abs().max()))
    T.assert_elementwise(a, t, s, 1.0, "one-key dQ / dK")
    _, pb, ids, _, _ = TP.packed_case(0.0, True)
    used = int(pb.cu[-1])
    masked = (ids <= 0)[:used]
    H = TP.PACKED_H
    for name, x in (("ref", dq), ("truth", tdq)):
        kv = x[:used].reshape(used, 3, H * 64)[:, 1:]
        print(name, "max |dK, dV| at masked keys", float(kv[masked].float().abs().max()))
        assert float(kv[masked].float().abs().max()) == 0.0
    for x in (ctx, dq, tctx, tdq):
        assert float(x[used:].float().abs().max()) == 0.0
    assert float(lse[:, used:].abs().max()) == 0.0 and float(tlse[:, used:].abs().max()) == 0.0


def test_embed_layernorm_packed_reference():
    """ref.embed_layernorm_fwd with pos_ids = row % S is ref.embed_layernorm_fwd without."""
    for B, S, D in T.EMBED_LN_SHAPES:
        x, pos, tt, g, b = T.embed_ln_case(B, S, D)
        want = ref.embed_layernorm_fwd(x, pos, tt, g, b, 1e-12)
        got = ref.embed_layernorm_fwd(x, pos, tt, g, b, 1e-12, torch.arange(B * S) % S)
        for a, w in zip(got, want):
            assert torch.equal(a, w)


def _small_bert():
    from pcmp.models.bert import BertConfig, BertForSequenceClassification
    torch.manual_seed(0)
    return BertForSequenceClassification(BertConfig(
        vocab_size=500, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256,
        hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)).train()


@pytest.mark.parametrize("fused", [True, False])
def test_bert_packed_matches_padded_on_cpu(monkeypatch, fused):
    """One layer, dropout 0, fp32 on the CPU: the packed forward / backward is the padded one up to the
    order of the fp32 sums over rows (the bound of the fp32 tests: 1e-5 of each tensor's norm), through
    the fused sublayer nodes and through the op-by-op layer (AttentionFn with cu, eager position gather)."""
    import pcmp.models.bert as bert_mod
    monkeypatch.setattr(bert_mod, "_FUSED", fused)
    monkeypatch.setattr(bert_mod, "_EMB_FUSED", fused)
    m = _small_bert()
    lens = [96, 70, 33, 9, 1]
    ids = T.attn_ids(96, lens, T._gen(3)) % 499 + 1
    ids = ids * (torch.arange(96).view(1, -1) < torch.tensor(lens).view(-1, 1))
    mask = (ids > 0).long()
    y = torch.tensor([0, 1, 1, 0, 1])
    out = {}
    for name, batch in (("padded", (ids, mask)), ("packed", (pack_batch(ids, mask, 32, 128), None))):
        m.zero_grad(set_to_none=True)
        loss = m(batch[0], None, batch[1], y)[0]
        loss.backward()
        out[name] = (float(loss.detach()), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    (lp, gp), (lk, gk) = out["padded"], out["packed"]
    print("loss padded %.8f packed %.8f" % (lp, lk))
    assert abs(lp - lk) <= 1e-5 * abs(lp)
    assert set(gp) == set(gk) and len(gp) > 10
    for n in gp:
        err = float((gp[n] - gk[n]).norm()) / max(float(gp[n].norm()), 1e-30)
        assert err <= 1e-5, (n, err)
    assert float(gp["position"][96:].abs().max()) == 0.0 and float(gk["position"][96:].abs().max()) == 0.0


def test_synthetic_lognormal_profile():
    from pcmp.data.synthetic import SyntheticIMDB
    idx = torch.arange(4000)
    base = SyntheticIMDB(4000, 128)
    assert torch.equal(base.lengths(idx), SyntheticIMDB(4000, 128, lengths="truncated").lengths(idx))
    assert float((base.lengths(idx) == 128).float().mean()) > 0.7
    L = SyntheticIMDB(4000, 512, lengths="lognormal").lengths(idx).float()
    assert 8 <= float(L.min()) and float(L.max()) == 512
    assert 215 <= float(L.median()) <= 245 and 245 <= float(L.mean()) <= 275, (float(L.median()), float(L.mean()))
    assert 0.09 <= float((L == 512).float().mean()) <= 0.16
    pb, none, y = SyntheticIMDB(64, 200, lengths="lognormal", pack=(32, 256)).get_batch(list(range(8)))
    assert isinstance(pb, PackedBatch) and none is None and y.shape == (8,) and pb.max_s == 224 and pb.B == 8
    with pytest.raises(ValueError, match="lengths must be one of"):
        SyntheticIMDB(8, 128, lengths="uniform")


def test_entrypoint_pack(tmp_path):
    import pytorch_on_language_distr as entry
    out = tmp_path / "rec.json"
    base = ["--device", "cpu", "--model", "bert", "--layers", "1", "--max-len", "200", "--pack", "--len-profile",
            "lognormal"]
    small = ["--train-size", "40", "--test-size", "8", "--epochs", "1", "--batch-size", "16", "--pack-rows", "256"]
    assert entry.main(base + small + ["--json", str(out)]) == 0
    rec = json.loads(out.read_text().strip().splitlines()[-1])
    assert rec["model"] == "bert" and all(l == l and abs(l) < 1e3 for l in rec["train_loss"])
    pk = rec["packing"]
    assert set(pk) == {"rows", "tokens", "padded_rows"}
    assert 0 < pk["tokens"] <= pk["rows"] < pk["padded_rows"] == 36 * 224, pk
    for extra, why in ((["--model", "bilstm"], "--pack needs --model bert"), (["--dtype", "fp32"], "bf16 only"),
                       (["--graph"], "not capturable")):
        with pytest.raises(SystemExit, match=why):
            entry.main(base + small + extra)


if __name__ == "__main__":
    for seed in (0, 1, 2, 3):
        print(seed, {k: float("%.3g" % v) for k, v in sorted(measure_packed_floors(seed).items())})
