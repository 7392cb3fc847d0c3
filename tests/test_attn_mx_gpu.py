"""The mxfp8 inference attention mode on the GPU (csrc/attn_mx.hip, layernorm_fwd's out_mx): the kernel against the fp64
truth of its decoded operands, the pair contracts bit for bit, the chained layer as the composition of its ops, the
end-to-end error against the unchained mode and one entry-point run."""
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import _lib, kernels, params, truth as T
from pcmp.ops._lib import ops
from test_attn_mx_cpu import ATTN_CASES, K_CTX, assert_chained_trace, attn_mx_case, mx_bert, mx_ids, traced_forward

pytestmark = pytest.mark.gpu


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("B,S,H", ATTN_CASES)
def test_kernel_against_fp64_and_pair_contract(gpu, B, S, H):
    q, e, ids, truth = attn_mx_case(B, S, H)
    q, e, ids = q.to(gpu), e.to(gpu), ids.to(gpu)
    ctx, = ops().attention_mx_fwd(q, e, ids, B, S, H, False)
    view, seg = T.seg_ctx(ctx.cpu(), B, S, H)
    print("norm_err", T.assert_elementwise(view, T.seg_ctx(truth, B, S, H)[0], seg, K_CTX, "ctx"))
    assert torch.equal(ctx, ops().attention_mx_fwd(q, e, ids, B, S, H, False)[0]), "two runs are bitwise equal"
    cq, ce = ops().attention_mx_fwd(q, e, ids, B, S, H, True)
    rq, re = ops().mxfp8_quant(ctx)
    assert same_bytes(cq, rq) and same_bytes(ce, re), "out_mx is mxfp8_quant of the bf16 context, pad bytes included"


@pytest.mark.parametrize("with_r", [False, True])
@pytest.mark.parametrize("M", [1, 33])
@pytest.mark.parametrize("D", [256, 768, 1024])
def test_layernorm_pair(gpu, D, M, with_r):
    x, r, g, b, _ = [t.to(gpu) if t is not None else None for t in T.ln_case(M, D, with_r)]
    plain = ops().layernorm_fwd(x, r, g, b, 1e-12)
    y, xs, mean, rstd, yq, ye = ops().layernorm_fwd(x, r, g, b, 1e-12, 0.0, 0, 0, None, True)
    assert torch.equal(y, plain[0]) and torch.equal(mean, plain[2]) and torch.equal(rstd, plain[3])
    rq, re = ops().mxfp8_quant(y)
    assert same_bytes(yq, rq) and same_bytes(ye, re)


def test_chained_layer_is_the_composition_of_its_ops(gpu):
    model, ids = mx_bert().to(gpu), mx_ids().to(gpu)
    B, S = ids.shape
    assert_chained_trace(traced_forward(model, ids, "mxfp8"), B, S, 2, "linear_mxfp8_fwd")
    assert_chained_trace(traced_forward(model, ids, "mxfp4"), B, S, 2, "linear_mxfp4_fwd")
    L = model.layers[0]
    h = torch.randn(B * S, 768, generator=torch.Generator().manual_seed(9)).bfloat16().to(gpu)
    _lib.set_infer_matmul("mxfp8")
    _lib.set_infer_attn("mxfp8")
    try:
        with torch.no_grad():
            h2, (h2q, h2e) = L(h, ids, B, S)
            lin = lambda x, l, act, mx: ops().linear_mxfp8_fwd(*x, *params.mxfp8_weight(l.weight), l.bias.float(), act, mx)
            qkv = lin(ops().mxfp8_quant(h), L.qkv, 0, True)
            a, = lin(ops().attention_mx_fwd(*qkv, ids, B, S, L.heads, True), L.attn_out, 0, False)
            ln1 = ops().layernorm_fwd(a, h, L.ln1.weight, L.ln1.bias, L.ln1.eps, 0.0, 0, 0, None, True)
            f, = lin(lin(ln1[4:], L.ffn1, 2, True), L.ffn2, 0, False)
            ln2 = ops().layernorm_fwd(f, ln1[0], L.ln2.weight, L.ln2.bias, L.ln2.eps, 0.0, 0, 0, None, True)
    finally:
        _lib.set_infer_matmul("bf16")
        _lib.set_infer_attn("bf16")
    assert torch.equal(h2, ln2[0]) and same_bytes(h2q, ln2[4]) and same_bytes(h2e, ln2[5])


def test_logits_against_the_unchained_mode(gpu):
    """The attention mode adds one e4m3 rounding each to Q, K and V, errors of the size the mxfp8 matmul mode already
    carries: its deviation from the bf16 logits is at most twice the unchained mode's."""
    model, ids = mx_bert().to(gpu), mx_ids().to(gpu)
    z = {}
    try:
        with torch.no_grad():
            for name, mm, at in (("bf16", "bf16", "bf16"), ("off", "mxfp8", "bf16"), ("on", "mxfp8", "mxfp8")):
                _lib.set_infer_matmul(mm)
                _lib.set_infer_attn(at)
                z[name] = model(ids)[0].float()
    finally:
        _lib.set_infer_matmul("bf16")
        _lib.set_infer_attn("bf16")
    d_off, d_on = float((z["off"] - z["bf16"]).abs().max()), float((z["on"] - z["bf16"]).abs().max())
    print("d_off", d_off, "d_on", d_on)
    assert d_on <= 2 * d_off


def test_bert_entrypoint(gpu, tmp_path):
    """A 1-layer BERT through --infer-matmul mxfp8 --infer-attn mxfp8: evaluation runs the chained layer."""
    import pytorch_on_language_distr as entry
    out = tmp_path / "rec.json"
    kernels.TRACE = []
    try:
        rc = entry.main(["--model", "bert", "--infer-matmul", "mxfp8", "--infer-attn", "mxfp8", "--layers", "1", "--max-len", "64",
                         "--batch-size", "8", "--train-size", "16", "--test-size", "8", "--epochs", "1", "--json", str(out)])
        seen = {n for n, _ in kernels.TRACE}
    finally:
        kernels.TRACE = None
        _lib.set_infer_matmul("bf16")
        _lib.set_infer_attn("bf16")
    assert rc == 0 and "attention_mx_fwd" in seen
    rec = json.loads(out.read_text().strip().splitlines()[-1])
    assert rec["infer_attn"] == "mxfp8" and rec["infer_matmul"] == "mxfp8" and len(rec["train_loss"]) == 1
    assert all(l == l and abs(l) < 1e3 for l in rec["train_loss"]) and 0.0 <= rec["test_accuracy"] <= 1.0
