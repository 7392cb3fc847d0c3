"""The mxfp8 training matmul mode on the GPU (csrc/mxfp8_train.hip, csrc/mxfp8.hip): the two-way quantiser against
the CPU reference, bit for bit; WGRAD and DGRAD against fp64 on operands the CPU reference quantised; the public
path through ``Linear``; one entry-point run.

Measured on one MI355X (docs/PARITY.md): ``dx`` norm_err 0.24 / 0.23 / 0.25 under k = 1, ``gw`` 7.2e-3 / 7.7e-3 / 7.6e-3
under k = 0.01 on the three GEMM cases, tiles 64 and 128 alike."""
import functools
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import _lib, kernels, params, ref, truth as T
from pcmp.ops._lib import ops
from test_linear_truth_cpu import BOUNDS as LINEAR_BOUNDS
from test_fp8_train_gpu import layer_run
from test_mxfp8_train_cpu import BOUNDS, GEMM_CASES, QUANT_CASES, gemm_case, planted, ref_backward

pytestmark = pytest.mark.gpu
K_DX, K_GW = LINEAR_BOUNDS[("linear", "dx")][1], BOUNDS[("gemm", "gw")][1]


# tiles of 128 rows x 64 columns: (96, 160) and (160, 96) end inside a tile in one direction each, (288, 416) in both,
# with a second scale dword in the transposed rows; no R / 32 or C / 32 is a multiple of 4: every scale row is padded
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("R,C", QUANT_CASES)
def test_quantiser_matches_reference(gpu, R, C, dtype):
    v = planted(R, C, dtype)
    d = v.to(gpu)
    got = ops().mxfp8_quant_both(d)
    own = ops().mxfp8_quant(d) + ops().mxfp8_quant(d.t().contiguous())
    for want in (ref.mxfp8_quant(v) + ref.mxfp8_quant(v.t().contiguous()), own):
        assert len(got) == 4 and all(g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu().view(torch.uint8), w.cpu().view(torch.uint8))
                                     for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def backward_case(M, N, K):
    _, _, dgrad, wgrad, t_dx, t_gw = ref_backward(*gemm_case(M, N, K))
    return dgrad, wgrad, t_dx, t_gw, torch.randn(N, K, generator=torch.Generator().manual_seed(K))


# (1056, 288, 160): 9 K-steps over the tokens in 2 splits of 5 and 4, the last step 32 tokens deep; 15 (64x64) or 6 tiles
@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("M,N,K", GEMM_CASES)
def test_gemms_against_fp64(gpu, M, N, K, tile):
    dgrad, wgrad, t_dx, t_gw, g0 = backward_case(M, N, K)
    dgrad, wgrad = [a.to(gpu) for a in dgrad], [a.to(gpu) for a in wgrad]
    old = ops().set_knob("fp8_tile", tile)
    try:
        dx = [ops().linear_mxfp8_fwd(*dgrad, None, 0, False)[0] for _ in range(2)]
        gw = {}
        for acc in (False, True):
            gw[acc] = [g0.to(gpu), g0.to(gpu)]
            for out in gw[acc]:
                ops().linear_mxfp8_wgrad(*wgrad, out, acc)
    finally:
        ops().set_knob("fp8_tile", old)
    pairs = ((dx[0], t_dx, K_DX), (gw[False][0], t_gw, K_GW), (gw[True][0], t_gw + g0.double(), K_GW))
    print(f"mxfp8 train gemms ({M}, {N}, {K}) tile {tile}: worst norm_err dx / gw / gw acc",
          ["%.2e" % float(T.norm_err(a.cpu(), t, (1,)).max()) for a, t, _ in pairs])
    for a, t, k in pairs:
        T.assert_elementwise(a.cpu(), t, (1,), k, "mxfp8 DGRAD / WGRAD / WGRAD acc")
    assert dx[0].dtype == torch.bfloat16 and torch.equal(dx[0], dx[1]), "two runs are bitwise equal"
    assert torch.equal(gw[False][0], gw[False][1]) and torch.equal(gw[True][0], gw[True][1])


@pytest.mark.parametrize("sink", [False, True])
@pytest.mark.parametrize("fin,fout,M,relu", [(160, 96, 64, True), (768, 3072, 64, False)])
def test_linear_public_path(gpu, fin, fout, M, relu, sink):
    from pcmp.models.layers import Linear
    torch.manual_seed(fin + M)
    lin, x, dy = Linear(fin, fout, relu=relu).to(gpu), torch.randn(M, fin).bfloat16().to(gpu), torch.randn(M, fout).bfloat16().to(gpu)
    w = lin.weight
    try:
        _lib.set_train_matmul("mxfp8")
        if sink:
            w.main_grad, w._grad_fresh = torch.full_like(w, 7.0), True
        y, gx, gw = layer_run(lin, x, dy)
        (wq, ew), (wtq, ewt) = params.mxfp8_weight(w), params.mxfp8_weight_t(w)
        xq, ex, xtq, ext = ops().mxfp8_quant_both(x)
        assert torch.equal(y, ops().linear_mxfp8_fwd(xq, ex, wq, ew, lin.bias.detach(), int(relu), False)[0]), "the mxfp8 forward is taken"
        dyq, edy, dytq, edyt = ops().mxfp8_quant_both(ops().relu_bwd(dy, y) if relu else dy)
        want = torch.empty_like(w)
        ops().linear_mxfp8_wgrad(dytq, edyt, xtq, ext, want, False)
        assert torch.equal(gx, ops().linear_mxfp8_fwd(dyq, edy, wtq, ewt, None, 0, False)[0]), "the mxfp8 DGRAD is taken"
        assert torch.equal(w.main_grad if sink else gw, want) and (gw is None) == sink, "the mxfp8 WGRAD is taken"
        if sink:                                   # the second backward of a step accumulates into the sink
            layer_run(lin, x, dy)
            ops().linear_mxfp8_wgrad(dytq, edyt, xtq, ext, want, True)
            assert torch.equal(w.main_grad, want)
        w.data.mul_(-1.5)                          # no version bump: what a fused optimizer step looks like
        params.bump_weight_gen()
        new = params.mxfp8_weight(w)[0], params.mxfp8_weight_t(w)[0]
        assert not any(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(new, (wq, wtq)))
    finally:
        _lib.set_train_matmul("bf16")


@pytest.mark.parametrize("fout,M", [(2, 64), (96, 48)])
def test_ineligible_call_keeps_bf16(gpu, fout, M):
    """Linear(160, 2) pads N to 8, and M = 48 is no multiple of 32: the call is LinearFn's, bit for bit."""
    from pcmp.models.layers import Linear
    torch.manual_seed(2)
    lin, x, dy = Linear(160, fout).to(gpu), torch.randn(M, 160).bfloat16().to(gpu), torch.randn(M, fout).bfloat16().to(gpu)
    base = layer_run(lin, x, dy)
    try:
        _lib.set_train_matmul("mxfp8")
        got = layer_run(lin, x, dy)
    finally:
        _lib.set_train_matmul("bf16")
    assert all(torch.equal(a, b) for a, b in zip(got, base))


def test_bert_entrypoint(gpu, tmp_path):
    """A 1-layer BERT through --train-matmul mxfp8: training runs the quantiser and both block-scaled GEMM ops."""
    import pytorch_on_language_distr as entry
    out = tmp_path / "rec.json"
    kernels.TRACE = []
    try:
        rc = entry.main(["--model", "bert", "--train-matmul", "mxfp8", "--layers", "1", "--max-len", "64", "--batch-size", "32",
                         "--train-size", "32", "--test-size", "16", "--epochs", "1", "--json", str(out)])
        seen = {n for n, _ in kernels.TRACE}
    finally:
        kernels.TRACE = None
        _lib.set_train_matmul("bf16")
    assert rc == 0 and {"mxfp8_quant_both", "linear_mxfp8_fwd", "linear_mxfp8_wgrad"} <= seen
    rec = json.loads(out.read_text().strip().splitlines()[-1])
    assert rec["train_matmul"] == "mxfp8" and len(rec["train_loss"]) == 1 and all(l == l and abs(l) < 1e3 for l in rec["train_loss"])
