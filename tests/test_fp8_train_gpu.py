"""The fp8 training matmul mode on the GPU (csrc/fp8_train.hip, csrc/fp8.hip): the quantisers against the CPU
reference, bit for bit; DGRAD and WGRAD against fp64 on operands the CPU reference quantised; the public path
through ``Linear``; one entry-point run."""
import functools
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import _lib, kernels, params, ref, truth as T
from pcmp.ops._lib import ops
from test_fp8_train_cpu import BOUNDS, GEMM_CASES, gemm_case, planted, ref_backward, scaled
from test_linear_truth_cpu import BOUNDS as LINEAR_BOUNDS

pytestmark = pytest.mark.gpu
K_DX, K_GW = LINEAR_BOUNDS[("linear", "dx")][1], BOUNDS[("gemm", "gw")][1]


def same(got, want):
    """fp8 payload bytes and the bit patterns of fp32 scales."""
    view = torch.uint8 if want.element_size() == 1 else torch.int32
    return got.dtype == want.dtype and torch.equal(got.cpu().view(view), want.view(view))


# tiles of 128 rows x 64 columns, amax slabs of 256 rows: (144, 72) passes the tile by one 16-row / 8-column step,
# (272, 72) the slab; (1040, 24) has a fifth slab (the partials are reduced four slabs at a time)
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("R,C", [(16, 16), (80, 144), (272, 72), (144, 72), (1040, 24)])
def test_quantisers_match_reference(gpu, R, C, dtype, fmt):
    torch.manual_seed(R * C)
    v = torch.randn(R, C) * 3
    v[:3], v[:, C - 3:] = 0, 0
    v[:3, : C - 3] = planted(C - 3, fmt)           # rows: zero, a lone maximum, the format's subnormal edge
    v[3:, C - 3:] = planted(R - 3, fmt).t()        # the same three as columns
    v = v.to(dtype)
    d = v.to(gpu)
    cols, both, rows = ops().fp8_quant_cols(d, fmt), ops().fp8_quant_both(d, fmt), ops().fp8_quant_rows(d, fmt)
    for got, want in ((cols, ref.fp8_quant_cols(v, fmt)), (both, ref.fp8_quant_both(v, fmt)), (rows, ref.fp8_quant_rows(v, fmt))):
        assert len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(both, rows + cols))


@functools.lru_cache(maxsize=None)
def backward_case(M, N, K):
    """Operands quantised by the CPU reference, the fp64 products of exactly those, and a gradient to accumulate onto."""
    x, w, dy = gemm_case(M, N, K)
    dyq, sdy, wtq, swt, dytq, sn, xtq, sk = ref_backward(x, w, dy)[2]
    g0 = torch.randn(N, K, generator=torch.Generator().manual_seed(K))
    return ((dyq, sdy, wtq, swt), (dytq, sn, xtq, sk), scaled(dyq, sdy) @ scaled(wtq, swt).t(),
            scaled(dytq, sn) @ scaled(xtq, sk).t(), g0)


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("M,N,K", GEMM_CASES)
def test_gemms_against_fp64(gpu, M, N, K, tile):
    dgrad_args, wgrad_args, t_dx, t_gw, g0 = backward_case(M, N, K)
    dgrad_args, wgrad_args = [a.to(gpu) for a in dgrad_args], [a.to(gpu) for a in wgrad_args]
    old = ops().set_knob("fp8_tile", tile)
    try:
        dx = [ops().linear_fp8_dgrad(*dgrad_args) for _ in range(2)]
        gw = {}
        for acc in (False, True):
            gw[acc] = [g0.to(gpu), g0.to(gpu)]
            for out in gw[acc]:
                ops().linear_fp8_wgrad(*wgrad_args, out, acc)
    finally:
        ops().set_knob("fp8_tile", old)
    worst = [T.assert_elementwise(dx[0].cpu(), t_dx, (1,), K_DX, "linear_fp8_dgrad"),
             T.assert_elementwise(gw[False][0].cpu(), t_gw, (1,), K_GW, "linear_fp8_wgrad"),
             T.assert_elementwise(gw[True][0].cpu(), t_gw + g0.double(), (1,), K_GW, "linear_fp8_wgrad acc")]
    print(f"fp8 train gemms ({M}, {N}, {K}) tile {tile}: worst norm_err dx {worst[0]:.4f} gw {worst[1]:.2e} acc {worst[2]:.2e}")
    assert dx[0].dtype == torch.bfloat16 and torch.equal(dx[0], dx[1]), "two runs are bitwise equal"
    assert torch.equal(gw[False][0], gw[False][1]) and torch.equal(gw[True][0], gw[True][1])


def layer_run(lin, x, dy):
    x = x.clone().requires_grad_(True)
    lin.weight.grad = None
    y = lin(x)
    y.backward(dy[:, : y.shape[1]])
    return y.detach(), x.grad, lin.weight.grad


@pytest.mark.parametrize("sink", [False, True])
@pytest.mark.parametrize("fin,fout,M,relu", [(144, 80, 48, True), (768, 3072, 64, False)])
def test_linear_public_path(gpu, fin, fout, M, relu, sink):
    from pcmp.models.layers import Linear
    torch.manual_seed(fin + M)
    lin, x, dy = Linear(fin, fout, relu=relu).to(gpu), torch.randn(M, fin).bfloat16().to(gpu), torch.randn(M, fout).bfloat16().to(gpu)
    w = lin.weight
    try:
        _lib.set_train_matmul("fp8")
        if sink:
            w.main_grad, w._grad_fresh = torch.full_like(w, 7.0), True
        y, gx, gw = layer_run(lin, x, dy)
        wq, sw = params.fp8_weight(w)
        wtq, swt = params.fp8_weight_t(w)
        assert torch.equal(y, ops().linear_fp8_fwd(*ops().fp8_quant_rows(x), wq, sw, lin.bias.detach(), int(relu))), "the fp8 forward is taken"
        g = ops().relu_bwd(dy, y) if relu else dy
        dyq, sdy, dytq, sn = ops().fp8_quant_both(g, 1)
        want = torch.empty_like(w)
        ops().linear_fp8_wgrad(dytq, sn, *ops().fp8_quant_cols(x, 0), want, False)
        assert torch.equal(gx, ops().linear_fp8_dgrad(dyq, sdy, wtq, swt)), "the fp8 DGRAD is taken"
        assert torch.equal(w.main_grad if sink else gw, want) and (gw is None) == sink, "the fp8 WGRAD is taken"
        if sink:                                   # the second backward of a step accumulates into the sink
            layer_run(lin, x, dy)
            ops().linear_fp8_wgrad(dytq, sn, *ops().fp8_quant_cols(x, 0), want, True)
            assert torch.equal(w.main_grad, want)
        w.data.mul_(-1.5)                          # no version bump: what a fused optimizer step looks like
        params.bump_weight_gen()
        assert not torch.equal(params.fp8_weight(w)[1], sw) and not torch.equal(params.fp8_weight_t(w)[1], swt)
    finally:
        _lib.set_train_matmul("bf16")


def test_ineligible_shape_keeps_bf16(gpu):
    """Linear(144, 2): N pads to 8, below the 16 the mode needs -- the call is LinearFn's, bit for bit."""
    from pcmp.models.layers import Linear
    torch.manual_seed(2)
    lin, x, dy = Linear(144, 2).to(gpu), torch.randn(48, 144).bfloat16().to(gpu), torch.randn(48, 2).bfloat16().to(gpu)
    base = layer_run(lin, x, dy)
    try:
        _lib.set_train_matmul("fp8")
        got = layer_run(lin, x, dy)
    finally:
        _lib.set_train_matmul("bf16")
    assert all(torch.equal(a, b) for a, b in zip(got, base))


def test_bert_entrypoint(gpu, tmp_path):
    """A 1-layer BERT through --train-matmul fp8: training runs all three fp8 GEMMs."""
    import pytorch_on_language_distr as entry
    out = tmp_path / "rec.json"
    kernels.TRACE = []
    try:
        rc = entry.main(["--model", "bert", "--train-matmul", "fp8", "--layers", "1", "--max-len", "64", "--batch-size", "16",
                         "--train-size", "32", "--test-size", "16", "--epochs", "1", "--json", str(out)])
        seen = {n for n, _ in kernels.TRACE}
    finally:
        kernels.TRACE = None
        _lib.set_train_matmul("bf16")
    assert rc == 0 and {"linear_fp8_fwd", "linear_fp8_dgrad", "linear_fp8_wgrad"} <= seen
    rec = json.loads(out.read_text().strip().splitlines()[-1])
    assert rec["train_matmul"] == "fp8" and rec["dtype"] == "bf16" and len(rec["train_loss"]) == 1
    assert all(l == l and abs(l) < 1e3 for l in rec["train_loss"])
