"""The mxfp4 inference matmul mode on the GPU (csrc/mxfp4.hip): the weight quantiser against the CPU reference, bit for
bit; the W4A8 GEMMs against fp64 under the bf16 Linear forward's bound; the ``out_mx`` epilogue; the public path; one
entry-point run.  Every operand's 32-blocks carry different scales (test_mxfp8_linear_cpu.block_scaled)."""
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import _lib, kernels, params, ref, truth as T
from pcmp.ops._lib import ops
from test_mxfp4_linear_cpu import OUT_MX_CASES, mx4_truth, out_mx_case, quant_bound, special_blocks
from test_mxfp8_linear_cpu import LAYER_CASES, block_scaled, layer_case, rule_scale
from test_mxfp8_linear_gpu import GEMM_CASES, K_FWD, with_knobs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("R,K", [(1, 32), (5, 160), (33, 768), (2, 4128)])
def test_quantiser_matches_reference(gpu, R, K, dtype):
    v = block_scaled(R, K, torch.Generator().manual_seed(R * K)) * 3
    sp = special_blocks()[: K // 32 * R]                       # spliced in as the leading blocks, row-major
    v.view(-1, 32)[: len(sp)] = sp
    v = v.to(dtype)   # the CPU reference and the kernel see the same rounded input
    q0, e0 = ref.mxfp4_quant(v)
    q, e = ops().mxfp4_quant(v.to(gpu))
    assert q.dtype == torch.uint8 and q.shape == (R, K // 2) and e.dtype == torch.uint8
    assert torch.equal(e.cpu(), e0), "scale bytes, pad bytes included"
    assert torch.equal(q.cpu(), q0), "nibbles, the sign of a value that rounds to zero included"


@pytest.mark.parametrize("name", list(GEMM_CASES))
def test_gemm_against_fp64(gpu, name):
    """The shapes, biases, activations and knobs of the mxfp8 GEMM test: products of E4M3 by E2M1 are exact and the sums
    run in fp32, so the same bound applies."""
    M, K, N, has_b, act, knobs = GEMM_CASES[name]
    gen = torch.Generator().manual_seed(M + K + N)
    xq, ex = ref.mxfp8_quant(block_scaled(M, K, gen).bfloat16())
    wq4, ew = ref.mxfp4_quant(block_scaled(N, K, gen, 0.05))
    b = torch.randn(N, generator=gen) * 0.5 if has_b else None
    t = mx4_truth(xq, ex, wq4, ew, b, act)
    args = [a.to(gpu) for a in (xq, ex, wq4, ew)] + [b.to(gpu) if has_b else None, act, False]
    (y,), (y2,) = with_knobs(knobs, lambda: (ops().linear_mxfp4_fwd(*args), ops().linear_mxfp4_fwd(*args)))
    worst = T.assert_elementwise(y.cpu(), t, (1,), K_FWD, f"linear_mxfp4_fwd {name}")
    print(f"mxfp4 gemm {name}: worst norm_err {worst:.4f}")
    assert y.dtype == torch.bfloat16 and torch.equal(y, y2), "two runs are bitwise equal"


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("M,K,N,act,seed", OUT_MX_CASES)
def test_out_mx_epilogue(gpu, M, K, N, act, seed, tile):
    """The pair emitted is MXFP8.  Scale bytes: the mxfp8 rule on the fp64 truth (test_out_mx_case_conditions keeps it clear
    of the thresholds).  Decoded output: the bound of test_mxfp8_linear_gpu.test_out_mx_epilogue."""
    xq, ex, wq4, ew, b, t = out_mx_case(M, K, N, act, seed)
    args = [a.to(gpu) for a in (xq, ex, wq4, ew, b)] + [act, True]
    (yq, ye), (yq2, ye2) = with_knobs({"fp8_tile": tile}, lambda: (ops().linear_mxfp4_fwd(*args), ops().linear_mxfp4_fwd(*args)))
    assert yq.dtype == torch.float8_e4m3fn and yq.shape == (M, N) and ye.shape == (M, 4 * ((N + 127) // 128))
    assert torch.equal(yq.view(torch.uint8), yq2.view(torch.uint8)) and torch.equal(ye, ye2)
    amax = t.abs().view(M, N // 32, 32).amax(2)
    want_e = torch.nn.functional.pad(rule_scale(amax), (0, ye.shape[1] - N // 32), value=127)
    assert torch.equal(ye.cpu(), want_e)
    scale = 2.0 ** (want_e[:, : N // 32].double() - 127).repeat_interleave(32, 1)
    allow = K_FWD * (T.REL * t.abs() + T.ABS_FRAC * t.abs().amax(1, keepdim=True))
    err = (ref.mxfp8_dequant(yq.cpu(), ye.cpu(), torch.float64) - t).abs()
    bound = 2.0 ** -4 * t.abs() + 2.0 ** -10 * scale + allow
    print(f"mxfp4 out_mx {(M, K, N)} act {act} tile {tile}: worst err / bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("fin,fout,M", LAYER_CASES)
def test_linear_public_path(gpu, fin, fout, M):
    lin, x = layer_case(fin, fout, M)
    t, bound = quant_bound(x, lin.weight.detach(), lin.bias.detach())
    lin, x = lin.to(gpu), x.to(gpu)
    try:
        _lib.set_infer_matmul("mxfp4")
        with torch.no_grad():
            y = lin(x)
            wq4, ew = params.mxfp4_weight(lin.weight)
            xq, ex = ops().mxfp8_quant(x)
            assert torch.equal(y, ops().linear_mxfp4_fwd(xq, ex, wq4, ew, lin.bias, 0, False)[0]), "the mxfp4 path is taken"
            err = (y.cpu().double() - t).abs()
            print(f"mxfp4 Linear({fin}, {fout}) M={M}: worst err / bound {float((err / bound).max()):.4f}")
            assert bool((err <= bound).all())
            lin.weight.data.mul_(-1.5)          # no version bump: what a fused optimizer step looks like
            params.bump_weight_gen()
            assert not torch.equal(lin(x), y), "the weight cache follows WEIGHT_GEN"
            kernels.TRACE = []                  # K = 144 is no multiple of 32: that layer stays on bf16
            type(lin)(144, 72).to(gpu)(torch.randn(M, 144, device=gpu).bfloat16())
            assert [n for n, _ in kernels.TRACE] == ["conv_fwd"]
    finally:
        kernels.TRACE = None
        _lib.set_infer_matmul("bf16")


def test_bert_entrypoint(gpu, tmp_path):
    """A 1-layer BERT through --infer-matmul mxfp4: ffn1 runs with GELU and out_mx, ffn2 consumes the pair."""
    import pytorch_on_language_distr as entry
    out = tmp_path / "rec.json"
    kernels.TRACE = []
    try:
        rc = entry.main(["--model", "bert", "--infer-matmul", "mxfp4", "--layers", "1", "--max-len", "64", "--batch-size", "8",
                         "--train-size", "16", "--test-size", "8", "--epochs", "1", "--json", str(out)])
        calls = [(n, a) for n, a in kernels.TRACE if n in ("linear_mxfp4_fwd", "linear_mxfp8_fwd", "mxfp8_quant")]
    finally:
        kernels.TRACE = None
        _lib.set_infer_matmul("bf16")
    fwd = [a for n, a in calls if n == "linear_mxfp4_fwd"]
    i = next(i for i, a in enumerate(fwd) if a[-2:] == [2, True])
    M = fwd[i][0][0]                     # ffn2's x is ffn1's [M, 3072] pair; nothing quantised an [M, 3072] activation
    assert rc == 0 and fwd[i + 1][0] == (M, 3072) and fwd[i + 1][2] == (768, 1536) and fwd[i + 1][-2:] == [0, False]
    assert not any(n == "linear_mxfp8_fwd" or (n == "mxfp8_quant" and a[0] == (M, 3072)) for n, a in calls)
    rec = json.loads(out.read_text().strip().splitlines()[-1])
    assert rec["infer_matmul"] == "mxfp4" and rec["dtype"] == "bf16" and len(rec["train_loss"]) == 1
    assert all(l == l and abs(l) < 1e3 for l in rec["train_loss"]) and 0.0 <= rec["test_accuracy"] <= 1.0
