"""The split-bf16 fp32 matmul mode (csrc/f32_bf16x.h, knob ``f32_bf16x``, ``--f32-matmul bf16x6 / bf16x3``)
on the CPU, in plain torch: the operand split the kernel performs at staging time and an emulation of the
product it forms, on the cases, inputs and fp64 truths of ``ops/truth_image_f32.py``.

``split_bf16(x, parts)``: hi = bf16_rne(x), mid = bf16_rne(x - hi), lo = bf16_rne(x - hi - mid).  Both
subtractions are exact in fp32 and three 8-bit significands with signed residuals hold fp32's 24 bits, so
with three parts hi + mid + lo == x; with two, |x - hi - mid| <= 2^-17 |x|.  A part below a non-finite hi
is 0 (an inf stays an inf).

``emulate(shape, what, parts)``: the sum of the kept part products (i, j), i + j <= parts - 1, each one
fp32 convolution of the fp32-held bf16 parts, added smallest first: (2,0) (1,1) (0,2) (1,0) (0,1) (0,0).
The kernel adds the same products in another order (per 16-deep slab of the reduction), so the emulation
gives the mode's accuracy *floor* -- the distance from the fp64 truth that the dropped products and the
fp32 accumulation leave -- not its bits.  tests/test_f32_bf16x_cpu.py commits the floors and derives the
kernel's bounds from them.
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F
from torch.nn import grad as G

from . import truth_image as T
from . import truth_image_f32 as TF

F32 = torch.float32
KNOB = {2: 3, 3: 6}                    # parts -> knob f32_bf16x (the number of products)
KERNEL = {2: "f32x3", 3: "f32x6"}      # parts -> kernel name of the conv_f32_plan tag
OUTPUTS = ("y", "y_fold", "dx", "dw", "dw_fold")


def split_bf16(x, parts):
    """[hi, mid(, lo)] of an fp32 tensor, each an fp32 tensor holding bf16 values."""
    assert x.dtype == F32 and parts in (2, 3)
    out, rest = [], x
    dead = torch.zeros_like(x, dtype=torch.bool)
    for i in range(parts):
        part = torch.where(dead, torch.zeros_like(x), rest.to(torch.bfloat16).to(F32))
        out.append(part)
        dead = dead | ~torch.isfinite(part)
        if i + 1 < parts:
            rest = torch.where(dead, torch.zeros_like(x), rest - part)   # exact in fp32
    return out


def products(parts):
    """The kept part products (i, j) in the order they are added: smallest first."""
    return [(i, d - i) for d in range(parts - 1, -1, -1) for i in range(d, -1, -1)]


def fold_f32(z, scale, shift):
    """relu(fma(z, scale, shift)) in fp32, the kernel's input fold: one rounding (the product is exact in
    fp64; the second rounding of the fp64 sum to fp32 differs from the fma's only in a double-rounding tie)."""
    return torch.relu(z.double() * scale.double() + shift.double()).to(F32)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def matmul_operands(shape, what, grid=False):
    """(a, b) of one output: the two matmul operands as the kernel sees them, NHWC / KRSC, fp32.  ``grid``:
    the operands of the exact cases (y_epi, y_fold_q, dx_q, dw_q, dw_fold_q)."""
    d = TF.conv_inputs(shape)
    if grid:
        fz = fold_f32(d["zq"], d["fsc"], d["fsh"])
        return {"y": (d["xq"], d["wq"]), "y_fold": (fz, d["wq"]), "dx": (d["dyq"], d["wq"]), "dw": (d["dyq"], d["xq"]),
                "dw_fold": (d["dyq"], fz)}[what]
    fz = fold_f32(d["z"], d["asc"], d["ash"])
    return {"y": (d["x"], d["w"]), "y_fold": (fz, d["w"]), "dx": (d["dy"], d["wd"]), "dw": (d["dy"], d["x"]),
            "dw_fold": (d["dy"], fz)}[what]


@functools.lru_cache(maxsize=None)
def emulate(shape, what, parts):
    """The mode's product for one random output of ``truth_image_f32.conv_truth`` (fp32, NHWC / KRSC)."""
    N, H, W, C, K, R, s, p = shape
    a, b = matmul_operands(shape, what)
    pa, pb = split_bf16(a, parts), split_bf16(b, parts)
    if what in ("y", "y_fold"):
        one = lambda u, v: _nhwc(F.conv2d(_nchw(u), _nchw(v), None, s, p))  # noqa: E731
    elif what == "dx":
        one = lambda u, v: _nhwc(G.conv2d_input((N, C, H, W), _nchw(v), _nchw(u), s, p))  # noqa: E731
    else:
        one = lambda u, v: _nhwc(G.conv2d_weight(_nchw(v), (K, C, R, R), _nchw(u), s, p))  # noqa: E731
    out = None
    for i, j in products(parts):
        t = one(pa[i], pb[j])
        out = t if out is None else out + t
    assert out.dtype == F32
    return out


# (op, output) of BOUNDS_X -> (the emulated product, the fp32 tensor the op adds to it, the tag key whose cases run it)
BOUND_KEYS = {
    ("conv_fwd", "y"): ("y", None, "fwd"),
    ("conv_fwd_fold", "y"): ("y_fold", None, "fwd_fold"),
    ("conv_dgrad", "dx"): ("dx", None, "dgrad"),
    ("conv_dgrad", "dx_resid"): ("dx", "dres", "dgrad"),
    ("conv_wgrad", "dw"): ("dw", None, "wgrad"),
    ("conv_wgrad", "dw_acc"): ("dw", "dw0", "wgrad"),
    ("conv_wgrad_fold", "dw"): ("dw_fold", None, "wgrad_fold"),
    ("conv_wgrad_fold", "dw_acc"): ("dw_fold", "dw0", "wgrad_fold"),
}


def floors(parts):
    """{(op, output): worst seg_rel of ``emulate`` (plus, in fp32, the residual / the accumulated-onto buffer)
    against the fp64 truth over every case of F32_CONV_CASES that runs that op}, segmented as the GPU tests
    segment them: per channel for the activations, per output-channel row for dw."""
    from .truth import seg_rel
    out = {}
    for bkey, (what, add, key) in BOUND_KEYS.items():
        worst = 0.0
        for shape in sorted({c["shape"] for c in TF.F32_CONV_CASES.values() if key in c["tags"]}):
            e, t = emulate(shape, what, parts), TF.conv_truth(shape, what)
            if add:
                e, t = e + TF.conv_inputs(shape)[add], t + TF.conv_inputs(shape)[add].double()
            seg = T.seg_k(t)[1] if what.startswith("dw") else T.seg_ch(t)[1]
            worst = max(worst, float(seg_rel(e, t, seg).max()))
        out[bkey] = worst
    return out
