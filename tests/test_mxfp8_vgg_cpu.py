"""The pooled mxfp8 conv and VGG16's chain on the CPU: ``ref.conv_mxfp8_fwd(..., pool=2)`` against the pooled fp64 truth,
the conditions of the pair cases, the path VGG takes, and the cases and checks the GPU tests share."""
from unittest import mock

import pytest
import torch
import torch.nn.functional as F

import pcmp  # noqa: F401
from pcmp.models.layers import Conv2d, MaxPool2d
from pcmp.models.vgg import CFG16, vgg16
from pcmp.ops import _lib, kernels, params, ref, truth as T
from pcmp.ops.functions import linear_mxfp8
from test_mxfp8_conv_cpu import CONV_CASES, K_FWD, check_out_mx, conv_case

# conv_case rows (N, H, W, C, Cout, kernel, stride, pad, bias, resid, relu): bias + ReLU, the only form VGG uses
POOL_CASES = {
    "odd_extents": (2, 5, 7, 64, 96, 3, 1, 1, True, False, True),     # floor in both axes; two images in one tile; N tail
    "one_window": (1, 2, 2, 32, 32, 3, 1, 1, True, False, True),      # M' = 4; all taps but the centre partly padded
    "row_tiles": (3, 10, 10, 128, 128, 3, 1, 1, True, False, True),   # M' = 300: row tiles, a partial last one
    "slab_tail": (1, 6, 6, 160, 64, 3, 1, 1, True, False, True),      # slab 128 + 32
}
# (case, seed) of the pair tests: the first seeds that pass test_pool_pair_case_conditions (conv_case zeroes image 0, so
# the single-image cases would hold nothing but the bias)
POOL_MX_CASES = [("odd_extents", 0), ("row_tiles", 0)]


def pool_case(name, seed=0, out_mx=False, dev="cpu"):
    """``conv_case`` of a pooled case, and ``max_pool2d`` of its fp64 truth, [N, OH/2, OW/2, Cout]."""
    with mock.patch.dict(CONV_CASES, POOL_CASES):
        args, t = conv_case(name, None, seed, out_mx, dev)
    return args, F.max_pool2d(t.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()


def vgg_by_hand(m, x, op, fc_pair):
    """VGG16's mxfp8 chain composed from the ops and ``params.mxfp8_conv_weight``: logits."""
    f = list(m.features)
    h = f[0](m.prepare_input(x))
    q, e = op.mxfp8_quant(h.view(-1, h.shape[-1]))
    h = (q.view(h.shape), e)
    convs = [(c, isinstance(n, MaxPool2d)) for c, n in zip(f[1:], f[2:] + [None]) if isinstance(c, Conv2d)]
    for k, (c, pool) in enumerate(convs):
        bf = k == len(convs) - 1 and not fc_pair
        wq, ew, b = params.mxfp8_conv_weight(c)
        h = op.conv_mxfp8_fwd(*h, wq, ew, 1, 1, b, None, True, bf, not bf, 2 if pool else 0)
    fc, z = m.classifier[0], h[0].reshape(len(x), -1)
    if fc_pair:
        z = linear_mxfp8((z, h[1].view(len(x), -1)), fc.weight, fc.bias, 1)
    return m.classifier[1 if fc_pair else 0:](z)


def check_vgg_paths(dev, op):
    """Mode on: the trace, and logits bitwise the hand-composed ops'; with the mxfp8 matmul mode the last conv's pair goes
    straight to classifier[0].  Mode off or grad enabled: the unchanged path.  The cache follows WEIGHT_GEN."""
    torch.manual_seed(5)
    m = vgg16(10, compute_dtype=torch.bfloat16).to(dev).eval()
    x = torch.rand(2, 3, 224, 224, device=dev)

    def trace_ops(fn):   # (result, [(op, args)] of every op dispatched)
        kernels.TRACE = tr = []
        try:
            return fn(), tr
        finally:
            kernels.TRACE = None

    def names(tr):   # conv, quantiser and pool ops; a Linear on the bf16 path is a conv_fwd on [B, 1, 1, K]: left out
        return [n for n, a in tr if any(k in n for k in ("conv", "quant", "pool")) and not (n == "conv_fwd" and a[0][1:3] == (1, 1))]

    with torch.no_grad():
        y_off, tr_off = trace_ops(lambda: m(x))
    try:
        _lib.set_infer_conv("mxfp8")
        y_grad, tr_grad = trace_ops(lambda: m(x))
        with torch.no_grad():
            want = vgg_by_hand(m, x, op, False)      # composed first: it fills the weight cache
            out, tr = trace_ops(lambda: m(x))
            _lib.set_infer_matmul("mxfp8")
            want_mm = vgg_by_hand(m, x, op, True)    # fills classifier[0]'s cache too
            out_mm, tr_mm = trace_ops(lambda: m.forward_logits(x))
            _lib.set_infer_matmul("bf16")
            m.features[1].weight.data.mul_(-1.5)     # no version bump: what a fused optimizer step looks like
            params.bump_weight_gen()
            out2 = m(x)
    finally:
        _lib.set_infer_conv("bf16")
        _lib.set_infer_matmul("bf16")
    today = ["maxpool_fwd" if v == "M" else "conv_fwd" for v in CFG16]
    assert names(tr_off) == today == names(tr_grad) and torch.equal(y_grad, y_off)
    assert names(tr) == ["conv_fwd", "mxfp8_quant"] + ["conv_mxfp8_fwd"] * 12
    mx = [a for n, a in tr if n == "conv_mxfp8_fwd"]
    pools = [2 if n == "M" else 0 for v, n in zip(CFG16[1:], CFG16[2:] + [0]) if v != "M"]   # behind convs 2 .. 13
    assert [a[-1] for a in mx] == pools and sum(pools) == 10 and [tuple(a[-3:-1]) for a in mx] == [(False, True)] * 11 + [(True, False)]
    assert torch.equal(out, want) and not torch.equal(out, y_off) and not torch.equal(out2, out)
    after = [n for n, _ in tr_mm][[n for n, _ in tr_mm].index("conv_fwd") + 2:]   # behind layer 0 and its quantiser
    assert after[:13] == ["conv_mxfp8_fwd"] * 12 + ["linear_mxfp8_fwd"] and torch.equal(out_mm, want_mm)
    return out, y_off


@pytest.mark.parametrize("name", list(POOL_CASES))
def test_ref_pooled_conv_against_fp64(name):
    args, t = pool_case(name)
    (y,) = ref.conv_mxfp8_fwd(*args, True, False, 2)
    assert y.shape == t.shape
    T.assert_elementwise(y.view(-1, y.shape[-1]), t.view(-1, t.shape[-1]), (1,), K_FWD, f"ref pooled conv {name}")


@pytest.mark.parametrize("name,seed", POOL_MX_CASES)
def test_pool_pair_case_conditions(name, seed):
    """No block amax of the pooled truth within relative 2^-10 of a threshold 1.75 * 2^j; an all-zero block; the reference's pair."""
    args, t = pool_case(name, seed, out_mx=True)
    amax = t.abs().view(-1, t.shape[-1] // 32, 32).amax(2)
    f = torch.frexp(amax[amax > 0])[0]
    assert bool(((f - 0.875).abs() > 0.875 * 2.0 ** -10).all()) and bool((amax == 0).any())
    y, yq, ye = ref.conv_mxfp8_fwd(*args, True, True, 2)
    check_out_mx(yq, ye, t)
    assert torch.equal(y, ref.conv_mxfp8_fwd(*args, True, False, 2)[0])


def test_vgg_cpu_paths():
    check_vgg_paths("cpu", ref)
