"""The mxfp8 inference conv mode on the CPU: ``ref.conv_mxfp8_fwd`` against the contract's formula in fp64, the switch
and its flag, the path residual blocks take, and the cases and conditions the GPU tests share."""
import json

import pytest
import torch
import torch.nn.functional as F

import pcmp  # noqa: F401
from pcmp.models.resnet import BasicBlock, Bottleneck
from pcmp.ops import _lib, kernels, params, ref, truth as T
from pcmp.ops.conv_blocks import MxAct
from test_mxfp8_linear_cpu import block_scaled, rule_scale

K_FWD = 1.0   # the bf16 Linear forward's bound, as in tests/test_mxfp8_linear_gpu.py
# name: (N, H, W, C, Cout, kernel, stride, pad, bias, resid, relu); each the smallest shape reaching one failure mode
CONV_CASES = {
    "tiny_1x1": (1, 3, 3, 32, 8, 1, 1, 0, False, False, False),       # M = 9 < any tile; one partial slab
    "half_slab_3x3": (2, 5, 7, 64, 72, 3, 1, 1, True, False, True),   # N tail; every border; rows cross images
    "slab_tail_s2": (2, 7, 7, 160, 64, 3, 2, 1, True, False, False),  # slab 128 + 32; odd extent under stride
    "downsample": (5, 8, 8, 128, 256, 1, 2, 0, True, False, False),
    "resid_tiles": (3, 10, 10, 128, 128, 3, 1, 1, True, True, True),  # M = 300: several row tiles, residual
    "zero_image": (1, 4, 4, 96, 32, 3, 1, 1, False, False, False),    # image 0 all zero: zero blocks next to padding
}
# (case, Cout, seed) of the out_mx tests: the first seeds that pass test_out_mx_case_conditions
OUT_MX_CASES = [("half_slab_3x3", 96, 0), ("slab_tail_s2", 64, 0), ("resid_tiles", 128, 7)]


def conv_case(name, cout=None, seed=0, out_mx=False, dev="cpu"):
    """(op arguments up to relu on ``dev``, fp64 truth [N, OH, OW, Cout]).  ``out_mx``: ReLU, image 0 zero and a
    non-positive bias / residual on the first 32 channels, so an all-zero block exists."""
    N, H, W, C, Co, R, stride, pad, has_b, has_r, relu = CONV_CASES[name]
    Co, relu = cout or Co, relu or out_mx
    gen = torch.Generator().manual_seed(seed + N * H * W + C + Co)
    x = block_scaled(N * H * W, C, gen).bfloat16()
    if out_mx or name == "zero_image":
        x[: H * W] = 0
    xq, ex = ref.mxfp8_quant(x)
    wq, ew = ref.mxfp8_quant(block_scaled(Co * R * R, C, gen, 0.05))
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    b = torch.randn(Co, generator=gen) * 0.5 if has_b or out_mx else None
    r = torch.randn(N, OH, OW, Co, generator=gen).bfloat16() if has_r else None
    if out_mx:
        b[:32] = -b[:32].abs() - 0.01
        if r is not None:
            r[..., :32] = -r[..., :32].abs()
    xd = ref.mxfp8_dequant(xq, ex, torch.float64).view(N, H, W, C).permute(0, 3, 1, 2)
    wd = ref.mxfp8_dequant(wq, ew, torch.float64).view(Co, R, R, C).permute(0, 3, 1, 2)
    t = F.conv2d(xd, wd, None, stride, pad).permute(0, 2, 3, 1)
    t = t + b.double() if b is not None else t
    t = t + r.double() if r is not None else t
    t = (torch.relu(t) if relu else t).contiguous()
    args = [xq.view(N, H, W, C), ex, wq.view(Co, R, R, C), ew, stride, pad, b, r, relu]
    return [a.to(dev) if isinstance(a, torch.Tensor) else a for a in args], t


def check_out_mx(yq, ye, t):
    """Scale bytes: the rule on the fp64 truth's block amax, pad bytes included.  Decoded values: within 2^-4 |t| +
    2^-10 2^(e-127) + the bf16 allowance (test_mxfp8_linear_gpu.test_out_mx_epilogue).  Returns worst err / bound."""
    Co, t = t.shape[-1], t.reshape(-1, t.shape[-1])
    amax = t.abs().view(len(t), Co // 32, 32).amax(2)
    want_e = F.pad(rule_scale(amax), (0, ye.shape[1] - Co // 32), value=127)
    assert yq.dtype == torch.float8_e4m3fn and ye.shape == (len(t), 4 * ((Co + 127) // 128))
    assert torch.equal(ye, want_e), "scale bytes, pad bytes included"
    scale = 2.0 ** (want_e[:, : Co // 32].double() - 127).repeat_interleave(32, 1)
    allow = K_FWD * (T.REL * t.abs() + T.ABS_FRAC * t.abs().amax(1, keepdim=True))
    err = (ref.mxfp8_dequant(yq.reshape(-1, Co), ye, torch.float64) - t).abs()
    bound = 2.0 ** -4 * t.abs() + 2.0 ** -10 * scale + allow
    assert bool((err <= bound).all())
    return float((err / bound).max())


def block_case(kind):
    """Bottleneck (64 -> 32 -> 128, stride 2, downsample) or BasicBlock, moved BN statistics, eval; a stem-like input."""
    torch.manual_seed(11)
    blk = (Bottleneck(64, 32, 2) if kind == "bottleneck" else BasicBlock(64, 64)).eval()
    with torch.no_grad():
        for L in blk.main_layers() + ([blk.downsample] if blk.downsample is not None else []):
            L.running_mean.normal_(0, 0.1), L.beta.normal_(0, 0.2), L.running_var.uniform_(0.5, 1.5), L.gamma.uniform_(0.5, 1.5)
    return blk, torch.relu(torch.randn(2, 9, 9, 64)).bfloat16()


def traced(fn):
    """(result, [(op, args)] of the conv and quantiser ops ``fn`` dispatched)."""
    kernels.TRACE = tr = []
    try:
        return fn(), [c for c in tr if "conv" in c[0] or "quant" in c[0]]
    finally:
        kernels.TRACE = None


def check_block_paths(kind, dev, op):
    """The chain is bitwise the hand-composed ops; grad enabled or mode off: the unchanged path; the cache follows WEIGHT_GEN."""
    blk, x = (t.to(dev) for t in block_case(kind))
    main, down = blk.main_layers(), blk.downsample
    with torch.no_grad():
        y_off, tr_off = traced(lambda: blk(x))
        xq, ex = op.mxfp8_quant(x.view(-1, 64))
        xin = MxAct(x, xq.view(x.shape), ex)
    try:
        _lib.set_infer_conv("mxfp8")
        y_grad, tr_grad = traced(lambda: blk(x))
        with torch.no_grad():
            h = (xin.q, xin.e)             # composed first: it fills the weight cache, so the trace shows no quantiser
            for L in main[:-1]:
                wq, ew, b = params.mxfp8_conv_weight(L)
                h = op.conv_mxfp8_fwd(*h, wq, ew, L.stride, L.pad, b, None, True, False, True)
            r = x
            if down is not None:
                wq, ew, b = params.mxfp8_conv_weight(down)
                r = op.conv_mxfp8_fwd(xin.q, xin.e, wq, ew, down.stride, down.pad, b, None, False, True, False)[0]
            wq, ew, b = params.mxfp8_conv_weight(main[-1])
            want = op.conv_mxfp8_fwd(*h, wq, ew, 1, main[-1].pad, b, r, True, True, True)
            out, tr = traced(lambda: blk(xin))
            main[0].weight.data.mul_(-1.5)      # no version bump: what a fused optimizer step looks like
            params.bump_weight_gen()
            out2 = blk(xin)
    finally:
        _lib.set_infer_conv("bf16")
    assert isinstance(out, MxAct) and all(torch.equal(a.view(torch.uint8), w.view(torch.uint8)) for a, w in zip(out, want))
    flags = [(False, True)] * (len(main) - 1) + ([(True, False)] if down is not None else []) + [(True, True)]
    assert [n for n, _ in tr] == ["conv_mxfp8_fwd"] * len(flags) and [tuple(a[-2:]) for _, a in tr] == flags
    assert {n for n, _ in tr_off} == {"conv_fwd"} == {n for n, _ in tr_grad}
    assert torch.equal(y_grad, y_off) and not torch.equal(out.y, y_off) and not torch.equal(out2.y, out.y)


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_ref_conv_against_fp64(name):
    args, t = conv_case(name)
    (y,) = ref.conv_mxfp8_fwd(*args, True, False)
    T.assert_elementwise(y.view(-1, y.shape[-1]), t.view(-1, t.shape[-1]), (1,), K_FWD, f"ref.conv_mxfp8_fwd {name}")
    assert name != "zero_image" or float(y.abs().max()) == 0


@pytest.mark.parametrize("name,cout,seed", OUT_MX_CASES)
def test_out_mx_case_conditions(name, cout, seed):
    """No block amax of the truth within relative 2^-10 of a threshold 1.75 * 2^j; an all-zero block; the reference's pair."""
    args, t = conv_case(name, cout, seed, out_mx=True)
    amax = t.abs().view(-1, cout // 32, 32).amax(2)
    f = torch.frexp(amax[amax > 0])[0]                           # threshold: mantissa 1.75 = 0.875 * 2
    assert bool(((f - 0.875).abs() > 0.875 * 2.0 ** -10).all()) and bool((amax == 0).any())
    y, yq, ye = ref.conv_mxfp8_fwd(*args, True, True)
    check_out_mx(yq, ye, t)
    assert torch.equal(y, ref.conv_mxfp8_fwd(*args, True, False)[0])


def test_switch_and_cli_flag(tmp_path):
    import another_neural_net as entry
    out = tmp_path / "rec.json"
    try:
        with pytest.raises(ValueError):
            _lib.set_infer_conv("fp8")
        assert _lib.infer_conv() == "bf16"
        assert entry.main(["--preset", "mlp-cpu", "--infer-conv", "mxfp8", "--json", str(out)]) == 0
        rec = json.loads(out.read_text().strip().splitlines()[-1])
        assert _lib.infer_conv() == "mxfp8" and rec["infer_conv"] == "mxfp8" and rec["infer_matmul"] == "bf16"
        with pytest.raises(SystemExit, match="--infer-conv mxfp8 needs --dtype bf16"):
            entry.main(["--preset", "mlp-cpu", "--infer-conv", "mxfp8", "--dtype", "fp32", "--json", str(out)])
        assert len(out.read_text().strip().splitlines()) == 1
    finally:
        _lib.set_infer_conv("bf16")
        _lib.set_precision("bf16")


@pytest.mark.parametrize("kind", ["bottleneck", "basic"])
def test_block_cpu_paths(kind):
    check_block_paths(kind, "cpu", ref)
