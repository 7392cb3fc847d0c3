"""Long-sequence attention (128 < S <= 512) on the CPU: the floors of ``ops/ref.py`` against the fp64
truth on ``truth.attn_case_long`` and the bounds the tiled kernels are held to in
tests/test_attention_long_gpu.py, the exact zeros of the one-key sequence, the entry point's
padding to a multiple of 32 and its ``--max-len`` limit.

``LONG_BOUNDS`` follows the rule of ``BOUNDS`` in tests/test_text_truth_cpu.py: per (op, output) the
worst ``norm_err`` of ``ref.py`` over ``ATTN_S_LONG`` x {(p = 0, ids), (p = 0.1, ids), (p = 0, no
ids)} (the floor) and k = 2 * floor rounded up to a multiple of 0.5, at least 1 and at most
max(1, 4 * floor); ``lse`` (fp32) gets 0.01.
"""
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.data.imdb import pad_to_multiple
from pcmp.ops import ref, truth as T, truth_run as R

LONG_VARIANTS = ((0.0, True), (0.1, True), (0.0, False))

# (op, output): (floor of ops/ref.py on the CPU, bound k of the GPU tests)
LONG_BOUNDS = {
    ("attention_p0", "ctx"): (0.391, 1.0), ("attention_p0", "lse"): (1.4e-5, 0.01), ("attention_p0", "dqkv"): (0.479, 1.0),
    ("attention_drop", "ctx"): (0.394, 1.0), ("attention_drop", "lse"): (7.7e-6, 0.01),
    ("attention_drop", "dqkv"): (0.491, 1.0),
}

_RUNS = {}


def ref_run(S, p, with_ids):
    """run_attention of ops/ref.py on one long case, computed once per session."""
    key = (S, p, with_ids)
    if key not in _RUNS:
        _RUNS[key] = R.run_attention(ref, T.attn_case_long(S, p, with_ids), S, p)
    return _RUNS[key]


def measure_long_floors():
    fl = {}
    for S in T.ATTN_S_LONG:
        for p, with_ids in LONG_VARIANTS:
            for n, e in R.worst(ref_run(S, p, with_ids)[0]).items():
                key = (R.attn_op(p), n)
                fl[key] = max(fl.get(key, 0.0), e)
    return fl


def test_long_case_shape():
    """Five sequences; the fifth has its valid keys in [136, S - 3) only."""
    for S in T.ATTN_S_LONG:
        qkv, ids, dctx, B, lens = T.attn_case_long(S, 0.0)
        assert B == 5 and lens[:4] == T.attn_lens(S, 0.0) and lens[4] != 1
        valid = (ids > 0)
        assert [int(v.sum()) for v in valid[:4]] == lens[:4]
        assert not valid[4, :136].any() and valid[4, 136:S - 3].all() and not valid[4, S - 3:].any()
        assert qkv.shape == (B * S, 384) and dctx.shape == (B * S, 128)
        assert T.attn_case_long(S, 0.0, with_ids=False)[1] is None
    assert T.ATTN_S_LONG == [160, 192, 256, 384, 512]


def test_long_reference_floors():
    fl = measure_long_floors()
    print({k: round(v, 3) for k, v in fl.items()})
    assert set(fl) == set(LONG_BOUNDS), set(fl) ^ set(LONG_BOUNDS)
    bad = []
    for key, f in fl.items():
        rec, k = LONG_BOUNDS[key]
        if abs(f - rec) > 0.1 * rec + 0.02:
            bad.append((key, "floor moved", f, rec))
        if not (2 * f <= k and k <= max(1.0, 4 * f)) or not (2 * rec <= k and k <= max(1.0, 4 * rec)):
            bad.append((key, "2*floor <= k <= max(1, 4*floor) violated", f, k))
    assert not bad, bad


def test_long_one_key_sequence_reference():
    """dQ / dK of the one-key sequence are exact zeros in ref.attention_bwd at every long S."""
    for S in T.ATTN_S_LONG:
        _, one_key, _ = ref_run(S, 0.0, True)
        a, t, s = one_key["dqk"]
        assert a.shape[0] == 1 and a.numel() > 0
        T.assert_elementwise(a, t, s, 1.0, f"one-key dQ / dK S={S}")


def test_pad_to_multiple():
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(1, 1000, (3, 200), generator=g)
    ids[1, 150:] = 0
    mask = (ids > 0).long()
    pi, pm = pad_to_multiple(ids, mask, 32)
    assert pi.shape == (3, 224) and pm.shape == (3, 224)
    assert pi.dtype == ids.dtype and pm.dtype == mask.dtype
    assert torch.equal(pi[:, :200], ids) and torch.equal(pm[:, :200], mask)
    assert int(pi[:, 200:].abs().sum()) == 0 and int(pm[:, 200:].abs().sum()) == 0
    for L in (32, 128, 192):
        i2, m2 = pad_to_multiple(ids[:, :L].contiguous(), mask[:, :L].contiguous(), 32)
        assert i2.shape == (3, L) and torch.equal(i2, ids[:, :L]) and torch.equal(m2, mask[:, :L])
    assert pad_to_multiple(ids[:, :1], mask[:, :1], 32)[0].shape == (3, 32)


def test_entrypoint_pads_and_limits_max_len(tmp_path, capsys):
    """--max-len 200 trains BERT at S = 224 (200 tokens + 24 masked columns); --max-len 600 is
    refused with both numbers before any model is built."""
    import pytorch_on_language_distr as entry
    out = tmp_path / "rec.json"
    rc = entry.main(["--device", "cpu", "--model", "bert", "--layers", "1", "--max-len", "200", "--train-size", "24",
                     "--test-size", "8", "--epochs", "1", "--batch-size", "8", "--json", str(out)])
    assert rc == 0
    rec = json.loads(out.read_text().strip().splitlines()[-1])
    assert rec["model"] == "bert" and all(l == l and abs(l) < 1e3 for l in rec["train_loss"])
    with pytest.raises(SystemExit, match=r"--max-len 600 exceeds BERT's max_position_embeddings \(512\)"):
        entry.main(["--device", "cpu", "--model", "bert", "--layers", "1", "--max-len", "600", "--train-size", "24",
                    "--test-size", "8", "--epochs", "1", "--batch-size", "8"])


if __name__ == "__main__":
    for k, v in sorted(measure_long_floors().items()):
        print(k, "%.3g" % v)
