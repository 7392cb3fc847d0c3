"""The mxfp8 training matmul mode on the CPU (``ops/ref.py`` only): the switch and the CLI flag, the fp32 floor of the
reference's WGRAD that bounds the GPU GEMM tests, and the CPU ``Linear`` path against the composed reference ops.
``BOUNDS`` holds (floor of ``ops/ref.py``, bound k) by the rule of tests/test_fp8_train_cpu.py, judged per row."""
import json
import math

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import _lib, ref, truth as T
from test_fp8_train_gpu import layer_run
from test_mxfp8_linear_cpu import block_scaled, special_blocks

GEMM_CASES = [(32, 32, 32), (160, 96, 416), (1056, 288, 160)]      # (M, N, K)
QUANT_CASES = [(32, 32), (96, 160), (160, 96), (288, 416)]          # (R, C)
BOUNDS = {("gemm", "gw"): (3.2e-05, 0.01)}


def planted(R, C, dtype):
    """``block_scaled`` data with the first five ``special_blocks`` (zero, amax 448 / 449, mantissa 1.75 and the next
    fp32) along a row block and along a column block; they are zero where the two meet at 32 x 32, so both hold."""
    v = block_scaled(R, C, torch.Generator().manual_seed(R * C))
    sb = special_blocks()[:5]
    v[8:13, C - 32:] = sb
    v[R - 32:, 8:13] = sb.t()
    return v.to(dtype)


def graded(R, C, gen, std=1.0):
    """[R, C] fp32 randn, each 32 x 32 tile times 2^j, j from -3..3: cut into blocks along rows or along columns, a
    scale applied to the wrong block shows, and no block has a spread inside (the quantiser's matter, docs/PARITY.md)."""
    j = torch.randint(-3, 4, (R // 32, 1, C // 32, 1), generator=gen)
    return (torch.randn(R // 32, 32, C // 32, 32, generator=gen) * std * 2.0 ** j).reshape(R, C)


def gemm_case(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    return graded(M, K, g).bfloat16(), graded(N, K, g, 0.05), graded(M, N, g).bfloat16()


def ref_backward(x, w, dy):
    """(dx, gw) of ops/ref.py, the DGRAD and WGRAD operands they came from, and the fp64 products of exactly those."""
    dyq, edy, dytq, edyt = ref.mxfp8_quant_both(dy)
    dgrad, wgrad = (dyq, edy, *ref.mxfp8_quant_both(w)[2:]), (dytq, edyt, *ref.mxfp8_quant_both(x)[2:])
    gw = torch.empty(w.shape)
    ref.linear_mxfp8_wgrad(*wgrad, gw, False)
    dq = lambda q, e: ref.mxfp8_dequant(q, e, torch.float64)
    return (ref.linear_mxfp8_fwd(*dgrad)[0], gw, dgrad, wgrad, dq(*dgrad[:2]) @ dq(*dgrad[2:]).t(),
            dq(*wgrad[:2]) @ dq(*wgrad[2:]).t())


def test_switch_and_cli_flag(tmp_path):
    import another_neural_net as entry
    out = tmp_path / "rec.json"
    assert _lib.train_matmul() == "bf16"
    try:
        _lib.set_train_matmul("mxfp8")
        assert _lib.train_matmul() == "mxfp8" and _lib.infer_matmul() == "bf16"
        _lib.set_train_matmul("bf16")
        assert entry.main(["--preset", "mlp-cpu", "--train-matmul", "mxfp8", "--json", str(out)]) == 0
        assert json.loads(out.read_text().strip().splitlines()[-1])["train_matmul"] == "mxfp8"
        with pytest.raises(SystemExit, match="--train-matmul mxfp8 needs --dtype bf16"):
            entry.main(["--preset", "mlp-cpu", "--train-matmul", "mxfp8", "--dtype", "fp32", "--json", str(out)])
    finally:
        _lib.set_train_matmul("bf16")
        _lib.set_precision("bf16")


def test_reference_floor():
    """The floor of BOUNDS, recomputed on GEMM_CASES, and the rule that turns it into k."""
    f = 0.0
    for M, N, K in GEMM_CASES:
        _, gw, _, _, _, t_gw = ref_backward(*gemm_case(M, N, K))
        f = max(f, float(T.norm_err(gw, t_gw, (1,)).max()))
    rec, k = BOUNDS[("gemm", "gw")]
    assert abs(f - rec) <= 0.1 * rec + 0.02, ("floor moved", f, rec)   # (the summation order of the CPU BLAS may move it)
    assert k == (0.01 if rec <= 1e-4 else max(1.0, math.ceil(4 * rec) / 2)) and (f <= 1e-4) == (rec <= 1e-4)


def test_linear_cpu_path():
    """Grad enabled + mxfp8 mode on the CPU: ``LinearMxfp8TrainFn`` over ops/ref.py equals the composed reference ops."""
    from pcmp.models.layers import Linear
    torch.manual_seed(5)
    lin, x, dy = Linear(160, 96, relu=True), torch.randn(64, 160).bfloat16(), torch.randn(64, 96).bfloat16()
    base = layer_run(lin, x, dy)
    try:
        _lib.set_train_matmul("mxfp8")
        y, gx, gw = layer_run(lin, x, dy)
    finally:
        _lib.set_train_matmul("bf16")
    xq, ex, xtq, ext = ref.mxfp8_quant_both(x)
    wq, ew, wtq, ewt = ref.mxfp8_quant_both(lin.weight.detach())
    assert torch.equal(y, ref.linear_mxfp8_fwd(xq, ex, wq, ew, lin.bias.detach(), 1)[0]) and not torch.equal(y, base[0])
    dyq, edy, dytq, edyt = ref.mxfp8_quant_both(ref.relu_bwd(dy, y))
    want = torch.empty_like(gw)
    ref.linear_mxfp8_wgrad(dytq, edyt, xtq, ext, want, False)
    assert torch.equal(gx, ref.linear_mxfp8_fwd(dyq, edy, wtq, ewt)[0]) and torch.equal(gw, want)
