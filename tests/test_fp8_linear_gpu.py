"""The fp8 (E4M3) inference matmul mode on the GPU (csrc/fp8.hip): the row quantiser against the CPU reference, bit
for bit; the GEMMs against fp64 on operands the CPU reference quantised, under the bound of the bf16 Linear forward
(tests/test_linear_truth_gpu.py: norm_err <= 1 per row); the public path through ``Linear``; one entry-point run."""
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import _lib, kernels, params, ref, truth as T
from pcmp.ops._lib import ops
from test_fp8_linear_cpu import LAYER_CASES, layer_case, quant_bound, special_rows

pytestmark = pytest.mark.gpu
K_FWD = 1.0   # BOUNDS[("linear", "u" / "g")][1] of tests/test_linear_truth_cpu.py


# (2, 4112): the first row length the quantiser reads twice instead of keeping in registers (K > 4096)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M,K", [(1, 16), (5, 144), (33, 768), (3, 3072), (2, 4112)])
def test_quantiser_matches_reference(gpu, M, K, dtype):
    torch.manual_seed(M * K)
    v = torch.randn(M, K) * 3
    idx = [1, 0, 2][: min(M, 3)]
    v[: len(idx)] = special_rows(K)[idx]
    v = v.to(dtype)   # the CPU reference and the kernel see the same rounded input
    q0, s0 = ref.fp8_quant_rows(v)
    q, s = ops().fp8_quant_rows(v.to(gpu))
    assert q.dtype == torch.float8_e4m3fn and torch.equal(s.cpu().view(torch.int32), s0.view(torch.int32))
    assert torch.equal(q.cpu().float(), q0.float())


# (M, K, N, bias, act, knobs)
GEMM_CASES = {
    "skinny_min": (1, 16, 8, True, 0, {}),
    "skinny_m16_tails": (16, 144, 72, False, 1, {}),
    "skinny_split_auto": (4, 4096, 64, True, 1, {"fp8_skinny_ns": 0}),
    "skinny_split1": (4, 4096, 64, True, 2, {"fp8_skinny_ns": 1}),
    "skinny_split4": (4, 4096, 64, False, 0, {"fp8_skinny_ns": 4}),
    "tiled_first_m_64": (17, 128, 64, False, 2, {"fp8_tile": 64}),
    "tiled_first_m_128": (17, 128, 64, True, 0, {"fp8_tile": 128}),
    "tiled_tails_64": (129, 400, 136, True, 1, {"fp8_tile": 64}),
    "tiled_tails_128": (129, 400, 136, True, 2, {"fp8_tile": 128}),
    "tiled_multi_64": (260, 1040, 264, True, 0, {"fp8_tile": 64}),
    "tiled_multi_128": (260, 1040, 264, False, 1, {"fp8_tile": 128}),
    "tiled_auto": (260, 1040, 264, True, 2, {}),
}


@pytest.mark.parametrize("name", list(GEMM_CASES))
def test_gemm_against_fp64(gpu, name):
    M, K, N, has_b, act, knobs = GEMM_CASES[name]
    torch.manual_seed(M + K + N)
    xq, sx = ref.fp8_quant_rows(torch.randn(M, K).bfloat16())
    wq, sw = ref.fp8_quant_rows(torch.randn(N, K) * 0.05)
    b = torch.randn(N) * 0.5 if has_b else None
    t = (sx[:, None] * sw[None, :]).double() * (xq.double() @ wq.double().t()) + (b.double() if has_b else 0)
    t = torch.relu(t) if act == 1 else torch.nn.functional.gelu(t) if act == 2 else t
    args = [a.to(gpu) for a in (xq, sx, wq, sw)] + [b.to(gpu) if has_b else None, act]
    old = {k: ops().set_knob(k, v) for k, v in knobs.items()}   # set_knob returns the previous value
    try:
        y, y2 = ops().linear_fp8_fwd(*args), ops().linear_fp8_fwd(*args)
    finally:
        for k, v in old.items():
            ops().set_knob(k, v)
    worst = T.assert_elementwise(y.cpu(), t, (1,), K_FWD, f"linear_fp8_fwd {name}")
    print(f"fp8 gemm {name}: worst norm_err {worst:.4f}")
    assert y.dtype == torch.bfloat16 and torch.equal(y, y2), "two runs are bitwise equal"


@pytest.mark.parametrize("fin,fout,M", LAYER_CASES)
def test_linear_public_path(gpu, fin, fout, M):
    lin, x = layer_case(fin, fout, M)
    t, bound = quant_bound(x, lin.weight.detach(), lin.bias.detach())
    lin, x = lin.to(gpu), x.to(gpu)
    try:
        _lib.set_infer_matmul("fp8")
        with torch.no_grad():
            y = lin(x)
            wq, sw = params.fp8_weight(lin.weight)
            xq, sx = ops().fp8_quant_rows(x)
            assert torch.equal(y, ops().linear_fp8_fwd(xq, sx, wq, sw, lin.bias, 0)), "the fp8 path is taken"
            err = (y.cpu().double() - t).abs()
            print(f"fp8 Linear({fin}, {fout}) M={M}: worst err / bound {float((err / bound).max()):.4f}")
            assert bool((err <= bound).all())
            lin.weight.data.mul_(-1.5)          # no version bump: what a fused optimizer step looks like
            params.bump_weight_gen()
            y3 = lin(x)
        assert not torch.equal(y3, y), "the weight cache follows WEIGHT_GEN"
    finally:
        _lib.set_infer_matmul("bf16")


def test_bert_entrypoint(gpu, tmp_path):
    """A 1-layer BERT through --infer-matmul fp8: evaluation runs the fp8 GEMMs (GELU in the ffn1 epilogue)."""
    import pytorch_on_language_distr as entry
    out = tmp_path / "rec.json"
    kernels.TRACE = []
    try:
        rc = entry.main(["--model", "bert", "--infer-matmul", "fp8", "--layers", "1", "--max-len", "64", "--batch-size", "8",
                         "--train-size", "16", "--test-size", "8", "--epochs", "1", "--json", str(out)])
        acts = [a[-1] for n, a in kernels.TRACE if n == "linear_fp8_fwd"]
    finally:
        kernels.TRACE = None
        _lib.set_infer_matmul("bf16")
    assert rc == 0 and 2 in acts and 0 in acts
    rec = json.loads(out.read_text().strip().splitlines()[-1])
    assert rec["infer_matmul"] == "fp8" and rec["dtype"] == "bf16" and len(rec["train_loss"]) == 1
    assert all(l == l and abs(l) < 1e3 for l in rec["train_loss"]) and 0.0 <= rec["test_accuracy"] <= 1.0
