"""The mxfp8 inference attention mode on the CPU: the reference ops' contract (docs/PARITY.md), the chained layer's op
sequence, the switch and its flag, and the cases the GPU tests share."""
import functools
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.models.bert import BertConfig, BertForSequenceClassification
from pcmp.ops import _lib, kernels, ref, truth as T
from test_mxfp8_linear_cpu import block_scaled

K_CTX = 1.0   # BOUNDS[("attention_p0", "ctx")][1] of tests/test_text_truth_cpu.py
# (B, S, H): one tile with idle waves and scale-row pad bytes; a partial query block with head / batch offsets; a full
# tile; the online rescale with a 32-key last tile; four tiles
ATTN_CASES = [(1, 32, 1), (2, 96, 2), (3, 128, 1), (2, 160, 2), (1, 512, 2)]


@functools.lru_cache(maxsize=None)
def attn_mx_case(B, S, H):
    """(q, e, ids, fp64 truth of ctx): every 32-block with its own scale, an all-zero Q block and an all-zero V block,
    sequences of S, S - 19 and 1 + S // 3 valid keys, and c such that the scores are neither flat nor one-hot."""
    gen = torch.Generator().manual_seed(100 * S + 10 * B + H)
    D = 64 * H
    x = block_scaled(B * S, 3 * D, gen)
    x[1, :32] = 0
    x[2, 2 * D + 32: 2 * D + 64] = 0
    heads = x.double().view(B, S, 3, H, 64)
    std = float((heads[:, :, 0].transpose(1, 2) @ heads[:, :, 1].permute(0, 2, 3, 1) / 8).std())
    q, e = ref.mxfp8_quant(x * (2.0 / std) ** 0.5)     # scores scale with c^2: std 2 before the e4m3 rounding
    xd = ref.mxfp8_dequant(q, e, torch.float64)
    heads = xd.view(B, S, 3, H, 64)
    std = float((heads[:, :, 0].transpose(1, 2) @ heads[:, :, 1].permute(0, 2, 3, 1) / 8).std())
    assert 1.0 <= std <= 4.0, std
    ids = T.attn_ids(S, [S, S - 19, 1 + S // 3][:B], gen)
    return q, e, ids, T.attention(xd, ids, B, S, H)[0]


def mx_bert(layers=2):
    torch.manual_seed(5)
    return BertForSequenceClassification(BertConfig(num_hidden_layers=layers), compute_dtype=torch.bfloat16).eval()


def mx_ids(B=2, S=64):
    return T.attn_ids(S, [S, S - 19][:B], torch.Generator().manual_seed(3))


def traced_forward(model, ids, matmul):
    """Op names of one no_grad forward in the attention mode (the second: the weight caches are warm)."""
    _lib.set_infer_matmul(matmul)
    _lib.set_infer_attn("mxfp8")
    try:
        with torch.no_grad():
            model(ids)
            kernels.TRACE = []
            model(ids)
            return list(kernels.TRACE)
    finally:
        kernels.TRACE = None
        _lib.set_infer_matmul("bf16")
        _lib.set_infer_attn("bf16")


def assert_chained_trace(trace, B, S, layers, gemm):
    """One attention_mx_fwd per layer and no bf16 attention; the only quantiser on [B*S, .] rows is layer 0's (the
    pooler and the classifier quantise their [B, 768] inputs as in the parent)."""
    names = [n for n, _ in trace]
    assert names.count("attention_mx_fwd") == layers and "attention_fwd" not in names and "bert_attn_fwd" not in names
    assert [a[0] for n, a in trace if n == "mxfp8_quant"] == [(B * S, 768), (B, 768), (B, 768)]
    assert names.count(gemm) == 4 * layers + 2 and names.count("layernorm_fwd") == 2 * layers


@pytest.mark.parametrize("matmul,gemm", [("mxfp8", "linear_mxfp8_fwd"), ("mxfp4", "linear_mxfp4_fwd")])
def test_chained_layer_on_cpu(matmul, gemm):
    ids = mx_ids()
    assert_chained_trace(traced_forward(mx_bert(), ids, matmul), *ids.shape, 2, gemm)


@pytest.mark.parametrize("B,S,H", ATTN_CASES[:2])
def test_reference_against_truth(B, S, H):
    q, e, ids, truth = attn_mx_case(B, S, H)
    ctx, = ref.attention_mx_fwd(q, e, ids, B, S, H, False)
    print("norm_err", T.assert_elementwise(*[T.seg_ctx(t, B, S, H)[0] for t in (ctx, truth)], T.seg_ctx(ctx, B, S, H)[1], K_CTX))
    cq, ce = ref.attention_mx_fwd(q, e, ids, B, S, H, True)
    rq, re = ref.mxfp8_quant(ctx)
    assert torch.equal(cq.view(torch.uint8), rq.view(torch.uint8)) and torch.equal(ce, re)


def test_reference_layernorm_pair():
    x, r, g, b, _ = T.ln_case(33, 96, True)
    y, xs, mean, rstd, yq, ye = ref.layernorm_fwd(x, r, g, b, 1e-12, 0.0, 0, 0, None, True)
    assert torch.equal(y, ref.layernorm_fwd(x, r, g, b, 1e-12)[0]) and ye.shape == (33, 4)
    rq, re = ref.mxfp8_quant(y)
    assert torch.equal(yq.view(torch.uint8), rq.view(torch.uint8)) and torch.equal(ye, re)


def test_switch(tmp_path):
    import another_neural_net as entry
    with pytest.raises(ValueError, match="inference attention mode"):
        _lib.set_infer_attn("fp8")
    assert _lib.infer_attn() == "bf16"
    small = ["--preset", "mlp-cpu"]
    for bad in (["--infer-attn", "mxfp8"], ["--infer-attn", "mxfp8", "--infer-matmul", "fp8"],
                ["--infer-attn", "mxfp8", "--infer-matmul", "mxfp8", "--dtype", "fp32"]):
        with pytest.raises(SystemExit, match="--infer-"):
            entry.main(small + bad)
    out = tmp_path / "rec.json"
    try:
        assert entry.main(small + ["--infer-matmul", "mxfp8", "--infer-attn", "mxfp8", "--json", str(out)]) == 0
    finally:
        _lib.set_infer_matmul("bf16")
        _lib.set_infer_attn("bf16")
        _lib.set_precision("bf16")
    assert json.loads(out.read_text().strip().splitlines()[-1])["infer_attn"] == "mxfp8"
