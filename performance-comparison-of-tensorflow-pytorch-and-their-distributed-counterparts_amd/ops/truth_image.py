"""fp64 truths of the image-path ops (implicit-GEMM convolutions, BatchNorm, pooling, the flat
optimizers) and the cases tests/test_image_truth_cpu.py and tests/test_image_truth_gpu.py judge.

As in ``ops/truth.py``: every truth is plain fp64 torch on the values the bf16 / fp32 inputs hold,
with no intermediate rounding, and every backward comes from ``torch.autograd``.  The BatchNorm folds
are exact math on the unrounded operand (the activation fold is ``relu(scale*z + shift)``, the
backward fold ``k1*g + k2*x + k3``), so the floor of a folded output carries the operand's bf16
rounding.  The statistics the conv epilogues emit are, by contract, those of the *stored, rounded*
output: their truth is the fp64 sum of the implementation's own output (``stats_of`` / ``bnr_sums``),
which is what catches a tile tail missing from the partials.

Everything here lives on the CPU: the cases are built from fixed seeds and the truths computed once
per case (``functools.lru_cache``), so the CPU and GPU tests judge the same numbers.
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

from .truth import ABS_FRAC, REL, assert_elementwise, norm_err, seg_all  # noqa: F401  (re-exported)

BF = torch.bfloat16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# segments of the compared tensors
def seg_ch(x):        # [..., C] -> one segment per (last-dimension) channel
    return x, tuple(range(x.dim() - 1))


def seg_k(x):         # dw [K, R, S, C] / statistics [2, C] -> one segment per leading index
    return x, tuple(range(1, x.dim()))


# ------------------------------------------------------------------------------ convolution
def fold_act(z, scale, shift):
    return torch.relu(z.double() * scale.double() + shift.double())


def fold_dz(g, x, coef):
    c = coef.double().reshape(3, -1)
    return c[0] * g.double() + c[1] * x.double() + c[2]


def conv(x, w, stride, pad, bias=None, resid=None, relu=False, dy=None, dx_resid=None, in_scale=None,
         in_shift=None, fold_x=None, fold_coef=None):
    """NHWC x [N,H,W,C] * KRSC w -> {"y", "pre"} and, given dy, {"dx", "dw"}: dx the gradient of the
    conv's (folded) input plus ``dx_resid``, dw that of w, both for the output gradient dy (folded:
    k1*dy + k2*fold_x + k3).  ``pre`` is y before the ReLU."""
    xe = fold_act(x, in_scale, in_shift) if in_scale is not None else x.double()
    xe = xe.detach().requires_grad_(dy is not None)
    w64 = w.detach().double().requires_grad_(dy is not None)
    lin = F.conv2d(xe.permute(0, 3, 1, 2), w64.permute(0, 3, 1, 2), None, stride, pad).permute(0, 2, 3, 1)
    pre = lin
    if bias is not None:
        pre = pre + bias.double()
    if resid is not None:
        pre = pre + resid.double().reshape(pre.shape)
    out = {"pre": pre.detach(), "y": (torch.relu(pre) if relu else pre).detach().contiguous()}
    if dy is not None:
        d = fold_dz(dy, fold_x, fold_coef) if fold_x is not None else dy.double()
        dx, dw = torch.autograd.grad((lin * d.reshape(lin.shape)).sum(), (xe, w64))
        if dx_resid is not None:
            dx = dx + dx_resid.double()
        out.update(dx=dx.contiguous(), dw=dw.contiguous())
    return out


def stats_of(y):
    """[2, K]: per-channel sum and sum of squares of an implementation's own stored output."""
    yr = y.detach().double().reshape(-1, y.shape[-1])
    return torch.stack([yr.sum(0), (yr * yr).sum(0)])


def bnr_sums(g, x, mean, invstd):
    """[2, C]: sum g and sum g * (x - mean) * invstd of an implementation's own masked gradient g,
    the given fp32 mean / invstd taken as doubles."""
    C = x.shape[-1]
    gr = g.detach().double().reshape(-1, C)
    xh = (x.double().reshape(-1, C) - mean.double()) * invstd.double()
    return torch.stack([gr.sum(0), (gr * xh).sum(0)])


def expand_sub_resid(r, H, W):
    full = torch.zeros(r.shape[0], H, W, r.shape[-1], dtype=r.dtype)
    full[:, 0::2, 0::2] = r
    return full


# ------------------------------------------------------------------------------ BatchNorm chain
def batchnorm(x, gamma, beta, rm, rv, momentum, eps, x2=None, gamma2=None, beta2=None, rm2=None, rv2=None,
              relu=False, dy=None):
    """y = [relu](BN(x) [+ x2 | + BN2(x2)]) by F.batch_norm(training=True) in fp64 (x: [M, C]).  The
    running buffers are updated in place (fp64 copies are returned).  With dy: dx, dx2 (the gradient
    of the residual branch), dgamma / dbeta (and dgamma2 / dbeta2) by autograd."""
    need = dy is not None
    x64 = x.detach().double().requires_grad_(need)
    g64 = gamma.detach().double().requires_grad_(need)
    b64 = beta.detach().double().requires_grad_(need)
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    pre = F.batch_norm(x64, rm64, rv64, g64, b64, True, momentum, eps)
    out = {"mean": x64.detach().mean(0), "invstd": torch.rsqrt(x64.detach().var(0, unbiased=False) + eps),
           "running_mean": rm64, "running_var": rv64}
    terms = (out["invstd"] * g64.detach() * x64.detach()).abs() + (b64.detach() - out["mean"] * out["invstd"] * g64.detach()).abs()
    leaves = [x64, g64, b64]
    names = ["dx", "dgamma", "dbeta"]
    if x2 is not None:
        x2_64 = x2.detach().double().requires_grad_(need)
        leaves.append(x2_64)
        names.append("dx2")
        if gamma2 is not None:
            g2, b2 = gamma2.detach().double().requires_grad_(need), beta2.detach().double().requires_grad_(need)
            rm2_64, rv2_64 = rm2.double().clone(), rv2.double().clone()
            pre = pre + F.batch_norm(x2_64, rm2_64, rv2_64, g2, b2, True, momentum, eps)
            m2, i2 = x2_64.detach().mean(0), torch.rsqrt(x2_64.detach().var(0, unbiased=False) + eps)
            out.update(mean2=m2, invstd2=i2, running_mean2=rm2_64, running_var2=rv2_64)
            terms = terms + (i2 * g2.detach() * x2_64.detach()).abs() + (b2.detach() - m2 * i2 * g2.detach()).abs()
            leaves += [g2, b2]
            names += ["dgamma2", "dbeta2"]
        else:
            pre = pre + x2_64
            terms = terms + x2_64.detach().abs()
    y = torch.relu(pre) if relu else pre
    out.update(y=y.detach(), pre=pre.detach(), terms=terms)
    if need:
        out.update(zip(names, torch.autograd.grad((y * dy.detach().double()).sum(), leaves)))
    return out


def batchnorm_one_row(x, gamma, beta, rm, rv, momentum, eps, x2=None, gamma2=None, beta2=None, rm2=None, rv2=None,
                      relu=False, dy=None):
    """``batchnorm`` for a single row (M = 1), written out by hand: F.batch_norm refuses one value per
    channel in training mode, the op does not.  mean = x, var = 0, invstd = rsqrt(eps), the normalised
    value is 0, so y = [relu](beta [+ x2 | + beta2]); the running buffers take mean and var = 0 with
    *no* unbiased correction (count == 1: ops/ref.py bn_finalize).  Backward: xhat = 0 makes dgamma
    = 0, dbeta = g (the masked dy) and dx = gamma*invstd*(g - mean(g)) = 0; a plain residual takes g."""
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    C = x.shape[-1]
    istd = torch.full((C,), eps, dtype=torch.float64).rsqrt()
    out = {"mean": x64[0].clone(), "invstd": istd, "running_mean": (1 - momentum) * rm.double() + momentum * x64[0],
           "running_var": (1 - momentum) * rv.double()}
    pre = b64.expand(1, C).clone()
    terms = (istd * g64 * x64).abs() + (b64 - x64 * istd * g64).abs()
    if x2 is not None:
        x2_64 = x2.double()
        if gamma2 is not None:
            pre = pre + beta2.double()
            out.update(mean2=x2_64[0].clone(), invstd2=istd.clone(),
                       running_mean2=(1 - momentum) * rm2.double() + momentum * x2_64[0],
                       running_var2=(1 - momentum) * rv2.double())
            terms = terms + (istd * gamma2.double() * x2_64).abs() + (beta2.double() - x2_64 * istd * gamma2.double()).abs()
        else:
            pre = pre + x2_64
            terms = terms + x2_64.abs()
    y = torch.relu(pre) if relu else pre
    out.update(y=y, pre=pre, terms=terms)
    if dy is not None:
        g = dy.double() * ((pre > 0).double() if relu else 1.0)
        z = torch.zeros(C, dtype=torch.float64)
        out.update(dx=torch.zeros_like(g), dgamma=z.clone(), dbeta=g[0].clone())
        if x2 is not None:
            out["dx2"] = torch.zeros_like(g) if gamma2 is not None else g.clone()
            if gamma2 is not None:
                out.update(dgamma2=z.clone(), dbeta2=g[0].clone())
    return out


# ------------------------------------------------------------------------------ pooling
def maxpool(x, dy=None, scale=None, shift=None):
    """max_pool2d(k 3, s 2, pad 1) of NHWC x, optionally behind y = relu(scale*x + shift) (the stem's
    fused prologue); with dy, the gradient of the pooled tensor's input (after the prologue)."""
    xe = x.double() if scale is None else torch.relu(x.double() * scale.double() + shift.double())
    xe = xe.detach().requires_grad_(dy is not None)
    y = F.max_pool2d(xe.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    dx = torch.autograd.grad((y * dy.double()).sum(), xe)[0] if dy is not None else None
    return {"y": y.detach().contiguous(), "dx": dx, "in": xe.detach()}


def gap(x, dy=None):
    x64 = x.detach().double().requires_grad_(dy is not None)
    y = x64.reshape(x.shape[0], -1, x.shape[-1]).mean(1)
    dx = torch.autograd.grad((y * dy.double()).sum(), x64)[0] if dy is not None else None
    return {"y": y.detach(), "dx": dx}


# ------------------------------------------------------------------------------ optimizers
def optimizer_steps(kind, w, grads, lr, gscale=None, **kw):
    """``len(grads)`` consecutive steps of torch.optim.SGD / Adam / AdamW from zero state on an fp64
    copy of w; returns per step the dict of w and the state tensors (mom | m1, m2)."""
    p = torch.nn.Parameter(w.detach().double().clone())
    cls = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "adamw": torch.optim.AdamW}[kind]
    opt = cls([p], lr=lr, **kw)
    out = []
    for g in grads:
        p.grad = g.double() * (1.0 if gscale is None else float(gscale))
        opt.step()
        st = opt.state[p]
        if kind == "sgd":
            out.append({"w": p.detach().clone(), "mom": st["momentum_buffer"].detach().clone()})
        else:
            out.append({"w": p.detach().clone(), "m1": st["exp_avg"].detach().clone(),
                        "m2": st["exp_avg_sq"].detach().clone()})
    return out


def adam_step_from(w, g, m1, m2, t, lr, beta1, beta2, eps, wd, decoupled):
    """One Adam / AdamW step number t from a given state, through torch.optim on fp64 tensors."""
    p = torch.nn.Parameter(w.detach().double().clone())
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([p], lr=lr, betas=(beta1, beta2), eps=eps,
                                                               weight_decay=wd)
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": m1.double().clone(),
                    "exp_avg_sq": m2.double().clone()}
    p.grad = g.double()
    opt.step()
    st = opt.state[p]
    return {"w": p.detach().clone(), "m1": st["exp_avg"].clone(), "m2": st["exp_avg_sq"].clone()}


def clip_coef(g, pre_scale, max_norm, post_scale):
    norm = g.double().pow(2).sum().sqrt() * pre_scale
    c = torch.clamp(max_norm / (norm + 1e-6), max=1.0) if max_norm > 0 else torch.ones_like(norm)
    return norm.reshape(()), (c * post_scale).reshape(())


# ==============================================================================  cases
# A convolution case: shape (N, H, W, C, K, R, stride, pad), the knobs it runs under (restored by the
# tests in ``finally``) and the kernel tags torch.ops.pcmp.conv_kernel_choice must report for it --
# "fwd" with statistics, "fwd_epi" with bias + residual + ReLU, "dgrad" plain, "bnr" with the
# BN-reduce epilogue in the form the runner uses first (mask recomputed from x), "wgrad".  The
# derivations quote csrc/igemm_launch.h (BK = 64, BM8 = 256, HALO_BM = 224), bnr_stream.h, wgrad32.h
# and igemm_fwd.hip / igemm_wgrad.hip.  Every conv case pins gemm_plan = 0 (static dispatch) and
# wgrad_wgs = 1024 (no timed split count) unless it says otherwise.
BASE_KNOBS = {"gemm_plan": 0, "wgrad_wgs": 1024, "fwd_split_target": 1}


def _case(shape, tags, knobs=None, **kw):
    k = dict(BASE_KNOBS)
    k.update(knobs or {})
    return dict(shape=shape, tags=tags, knobs=k, **kw)


CONV_CASES = {
    # stem 7x7/2: gm = 2*5*5 = 50 (<= 64), gn = 64, gk = 392 (C = 8: no uniform tap walk, no DMA)
    # -> register-staged 64x64.  DGRAD: four sub-pixel classes of gm = 2*5*5 / 2*5*4 / 2*4*5 / 2*4*4
    # rows (<= 64 and <= 32), gn = 8 -> 64x64, 64x64, 64x64, 32x64.  WGRAD: gm = K = 64, gn = 392 >=
    # 256, C = 8 -> the 64x256 stem tile; N*P*Q = 50 rows -> 1 K-step, one split.
    "stem7": _case((2, 9, 9, 8, 64, 7, 2, 3),
                   dict(fwd="reg/64x64", fwd_epi="reg/64x64", dgrad="reg/64x64+reg/64x64+reg/64x64+reg/32x64",
                        bnr="reg/64x64+reg/64x64+reg/64x64+reg/32x64", wgrad="wgrad_m32/64x256/ns1")),
    # the same tile for the space-to-depth stem's C = 16 (4x4 stride 1): WGRAD gm = 64, gn = 256
    "stem16": _case((2, 8, 8, 16, 64, 4, 1, 2), dict(fwd="reg/128x64", fwd_epi="reg/128x64", wgrad="wgrad_m32/64x256/ns1"),
                    ops=("fwd", "wgrad")),
    # Linear, tiny M and N: gm = 5 (<= 32), gn = 16 -> 32x64; DGRAD gn = 256 -> 32x128; WGRAD gm = 16
    # (<= 32), gn = 256 -> 32x128 (32x32 wave tiles: the 32x32x16 form)
    "lin5": _case((5, 1, 1, 256, 16, 1, 1, 0),
                  dict(fwd="reg/32x64", fwd_epi="reg/32x64", dgrad="reg/32x128", bnr="reg/32x128", wgrad="wgrad_m32/32x128/ns1")),
    # gm = 33 rows (one past the 32-row tile), gn = 72 -> 64x128; DGRAD gn = 64 -> 64x64; WGRAD gm = 72
    # (> 64) x gn = 64 -> 128x64 (gm < 256: not the 256x64 wide tile)
    "gm33": _case((33, 1, 1, 64, 72, 1, 1, 0),
                  dict(fwd="reg/64x128", fwd_epi="reg/64x128", dgrad="reg/64x64", bnr="reg/64x64", wgrad="wgrad_m32/128x64/ns1")),
    # gm = 65 rows, gn = 64 -> 128x64 (gk = 64: one K-tile, no DMA kernel); WGRAD gm = gn = 64 -> 64x64
    "gm65": _case((65, 1, 1, 64, 64, 1, 1, 0),
                  dict(fwd="reg/128x64", fwd_epi="reg/128x64", dgrad="reg/128x64", bnr="reg/128x64", wgrad="wgrad_m32/64x64/ns1")),
    # gm = 129 rows (a second 128-row tile of one row), gn = 136 (a second column tile of 8): with
    # statistics 128x128; the plain epilogues (1 x 2 < 256 tiles of 128x128) take bm64_smallgrid's
    # 64x128; wgrad_m32 = 0 puts the 128x128 WGRAD (gm = 136, gn = 64 -> 128x64) on 16x16x32 MFMAs
    "gm129": _case((129, 1, 1, 64, 136, 1, 1, 0),
                   dict(fwd="reg/128x128", fwd_epi="reg_smallgrid/64x128", dgrad="reg/128x64", bnr="reg/128x64",
                        wgrad="wgrad/128x64/ns1"), knobs={"wgrad_m32": 0}),
    # channel counts off the tile grid: C = 24 (no uniform tap walk), K = 136; gm = 392 (a 4th row
    # tile of 8 rows).  WGRAD gm = 136, gn = 216 -> 128x128 with tails both ways
    "offgrid": _case((2, 14, 14, 24, 136, 3, 1, 1),
                     dict(fwd="reg/128x128", fwd_epi="reg_smallgrid/64x128", dgrad="reg/128x64", bnr="reg/128x64",
                          wgrad="wgrad_m32/128x128/ns1")),
    # bm64_smallgrid 64x128, plain epilogue: gm = 392, gn = 136, 4 x 2 tiles < 256 (with statistics the
    # shape stays on the LDS-DMA kernel: C = 64, 9 K-tiles, dma4_small_n64 -> 128x64 on the 32x32x16 kernel)
    "smallgrid": _case((2, 14, 14, 64, 136, 3, 1, 1), dict(fwd="dma32/128x64", fwd_epi="reg_smallgrid/64x128"),
                       ops=("fwd",)),
    # LDS-DMA 128x64: gm = 147 (> 64; a second row tile of 19), gn = 64, gk = 576 = 9 K-tiles -> use_dma4
    # case 2; FWD on the 32x32x16 kernel (dma32 = 1, >= dma32_mink = 3 K-tiles), DGRAD on igemm_dma_kernel
    # (dma32_modes = 1: FWD only).  WGRAD: gm = 64, gn = 576 but C = 64: 64x128
    "dma64": _case((3, 7, 7, 64, 64, 3, 1, 1),
                   dict(fwd="dma32/128x64", fwd_epi="dma32/128x64", dgrad="dma4/128x64", bnr="dma4/128x64",
                        wgrad="wgrad_m32/64x128/ns1")),
    "dma64_old": _case((3, 7, 7, 64, 64, 3, 1, 1),
                       dict(fwd="dma4/128x64", fwd_epi="dma4/128x64", dgrad="dma4/128x64", bnr="dma4/128x64"),
                       knobs={"dma32": 0}, ops=("fwd", "dgrad", "bnr")),
    # ... and its DGRAD on the 32x32x16 kernel: dma32_modes = 3 (3x3: R*S > 1)
    "dma64_dgrad32": _case((3, 7, 7, 64, 64, 3, 1, 1), dict(dgrad="dma32/128x64", bnr="dma32/128x64"),
                           knobs={"dma32_modes": 3, "dma32_dgrad_mink": 1}, ops=("dgrad", "bnr")),
    # LDS-DMA 128x128 (bm64_smallgrid = 0, dma4_small_n64 = 0): gm = 147 (row tail), gn = 192 (a
    # half-empty second column tile), 18 K-tiles.  DGRAD: gn = 128, K = 192 -> 27 K-tiles
    "dma128": _case((3, 7, 7, 128, 192, 3, 1, 1),
                    dict(fwd="dma32/128x128", fwd_epi="dma32/128x128", dgrad="dma4/128x128", bnr="dma4/128x128",
                         wgrad="wgrad_m32/128x128/ns1"), knobs={"bm64_smallgrid": 0, "dma4_small_n64": 0}),
    # stride-2 3x3: FWD gm = 2*7*7 = 98, 18 K-tiles.  DGRAD runs four sub-pixel classes of 98 rows each
    # with 1x1 / 1x2 / 2x1 / 2x2 taps = 2 / 4 / 4 / 8 K-tiles of K = 128: the first (< 3 K-tiles) stays
    # register-staged, the others take the LDS-DMA kernel (launch order: (oph, opw) = (0,0) is 1x1)
    "s2": _case((2, 14, 14, 128, 128, 3, 2, 1),
                dict(fwd="dma32/128x128", fwd_epi="dma32/128x128", dgrad="reg/128x128+dma4/128x128+dma4/128x128+dma4/128x128",
                     bnr="reg/128x128+dma4/128x128+dma4/128x128+dma4/128x128", wgrad="wgrad_m32/128x128/ns1"),
                knobs={"bm64_smallgrid": 0, "dma4_small_n64": 0}),
    # ... on an odd H, W: classes of 8x8, 8x7, 7x8 and 7x7 pixels
    "s2_odd": _case((2, 15, 15, 128, 128, 3, 2, 1),
                    dict(dgrad="reg/128x128+dma4/128x128+dma4/128x128+dma4/128x128",
                         bnr="reg/128x128+dma4/128x128+dma4/128x128+dma4/128x128"),
                    knobs={"bm64_smallgrid": 0, "dma4_small_n64": 0}, ops=("dgrad", "bnr")),
    # 1x1 stride-2 downsample: one covered class (even pixels), the truth's dx is exactly 0 at the odd
    # ones.  C = 192 gives the FWD 3 K-tiles (gm = 5*4*4 = 80 > 64): LDS-DMA 128x128; DGRAD gn = 192,
    # K = 256 -> 4 K-tiles, 1x1 with < dma32_dgrad_mink K-tiles: igemm_dma_kernel
    "down": _case((5, 8, 8, 192, 256, 1, 2, 0),
                  dict(fwd="dma32/128x128", fwd_epi="dma32/128x128", dgrad="dma4/128x128", wgrad="wgrad_m32/128x128/ns1"),
                  knobs={"bm64_smallgrid": 0, "dma4_small_n64": 0}, ops=("fwd", "dgrad", "wgrad")),
    # 8-wave 256x256 (igemm8_min_tiles = 1): gn = 256, 9 K-tiles (>= 8), gm = 392 is not a multiple of 256
    "igemm8": _case((2, 14, 14, 64, 256, 3, 1, 1), dict(fwd="dma8/256x256", fwd_epi="dma8/256x256"),
                    knobs={"igemm8_min_tiles": 1}, ops=("fwd",)),
    # ... and the DGRAD of the mirrored shape (gn = C = 256, K = 64 -> 9 K-tiles)
    "igemm8_dgrad": _case((2, 14, 14, 256, 64, 3, 1, 1), dict(dgrad="dma8/256x256", bnr="dma8/256x256"),
                          knobs={"igemm8_min_tiles": 1}, ops=("dgrad", "bnr")),
    # split-K forward at batch 1 (no statistics, < 128 tiles, >= 8 K-steps): gm = 49 -> 64-row tiles,
    # 1 x 16 tiles, 8 K-steps -> min(16, 8/4, 32) = 2 splits; gm = 196, 2 x 2 tiles, 36 K-steps ->
    # min(64, 9, 32) = 9 splits of 4 K-steps
    "splitk_1x1": _case((1, 7, 7, 512, 2048, 1, 1, 0), dict(fwd_epi="reg/64x128/ns2"), knobs={"fwd_split_target": 256}, ops=("fwd_epi",)),
    "splitk_3x3": _case((1, 14, 14, 256, 256, 3, 1, 1), dict(fwd_epi="reg/128x128/ns9"), knobs={"fwd_split_target": 256}, ops=("fwd_epi",)),
    # streaming FWD + statistics (bnr_stream.h use_fwd_stream): 1x1, gk = 64 / 128 < gn, gn % 128 == 0,
    # gm = 32 rows (% 32 == 0); gn = 256 with gk = 64 takes the 256-column form
    "fwd_stream64": _case((2, 4, 4, 64, 256, 1, 1, 0), dict(fwd="fwd_stream/32x256"), ops=("fwd_stats",)),
    "fwd_stream128": _case((2, 4, 4, 128, 384, 1, 1, 0), dict(fwd="fwd_stream/32x128"), ops=("fwd_stats",)),
    # halo kernel: layer-1 3x3 at 56 wide, 19 * 56 / 4 = 266 tiles of 224 rows (>= 256).  FWD with
    # statistics overlaps its stores; halo = 7 enables the DGRAD: the overlapped form needs the mask
    # recomputed from x and no residual, a mask tensor takes the plain one
    # residual + ReLU (no bias: the halo kernel takes none) runs the FWD without the overlapped stores
    "halo": _case((19, 56, 56, 64, 64, 3, 1, 1), dict(fwd="halo_ovl/224x64", fwd_res="halo/224x64", bnr="halo_ovl/224x64",
                                                      bnr_mask="halo/224x64"),
                  knobs={"halo": 7}, ops=("fwd_stats", "fwd_res", "bnr_halo")),
    # ... and the space-to-depth stem (C = 16, 4x4, no padding, 112 wide: tiles of two output rows) at
    # its smallest eligible batch: 5 * 112 / 2 = 280 tiles >= 256
    "halo_s2d": _case((5, 115, 115, 16, 64, 4, 1, 0), dict(fwd="halo_ovl/224x64", fwd_res="halo/224x64"),
                      ops=("fwd_stats", "fwd_res")),
}

# C = 576 = 4.5 column tiles of 128 is not for the stream (it covers gn / 128 whole tiles: the last 64
# channels came back unwritten before use_bnr_stream asked for whole tiles): gm = 32 -> 32x128
CONV_CASES["bnr_gn576"] = _case((2, 4, 4, 576, 256, 1, 1, 0), dict(bnr="reg/32x128"), ops=("bnr",))

# Planner kinds (igemm_plan.h), each through plan_force with gemm_plan = 1, the split count pinned to 1
# and to one that does not divide the K-steps.  Large M (plain_gemm_eligible: 1x1, gm = 1030 >= 1024,
# 13 K-tiles, gn = 264 >= 256): kinds 1 (dma128x128), 2 (dma256x256), 5 (dma128x64), 9 / 10 (the
# 32x32x16 GEMMs) with 1 and 2 splits (7 + 6 K-tiles).  Small M (gm = 49, 1 x 2 tiles, 13 K-steps):
# kinds 3 (reg64x64), 4 (reg32x64), 6 (skinny, 26 K-steps of 32) with 1 and 4 splits (4+4+4+1 / 7+7+7+5).
PLAN_KINDS = {1: "dma128x128", 2: "dma256x256", 5: "dma128x64", 9: "m32_128x128", 10: "m32_256x256",
              3: "reg64x64", 4: "reg32x64", 6: "skinny64x64"}
for _k, _n in PLAN_KINDS.items():
    _small = _k in (3, 4, 6)
    for _ns in ((1, 4) if _small else (1, 2)):
        CONV_CASES[f"plan_{_n}_ns{_ns}"] = _case(
            (1, 7, 7, 832, 136, 1, 1, 0) if _small else (1030, 1, 1, 832, 264, 1, 1, 0), dict(fwd_epi=f"plan/{_n}/ns{_ns}"),
            knobs={"gemm_plan": 1, "plan_force": _k, "plan_nsplit": _ns, "fwd_split_target": 256}, ops=("fwd_epi",))

# streaming DGRAD + BN-reduce (bnr_stream.h use_bnr_stream): 1x1, gk = K in {64, 128, 256} < gn = C
# (64, or whole 128-column tiles), gm = 32 rows, the mask as bits or recomputed (never a tensor); the
# dz fold doubles the operand: 2*K < C.
BNR_STREAM_CASES = {
    "bnr_stream64": _case((2, 4, 4, 256, 64, 1, 1, 0), dict(bnr="bnr_stream/32x128")),
    "bnr_stream128": _case((2, 4, 4, 384, 128, 1, 1, 0), dict(bnr="bnr_stream/32x128")),
    "bnr_stream256": _case((2, 4, 4, 640, 256, 1, 1, 0), dict(bnr="bnr_stream/32x128")),
}

# forms of conv_dgrad_bnr (the runner's ``form``): how the ReLU mask arrives, one or two BatchNorms,
# the residual, the dz fold.  flags are conv_kernel_choice's DGRAD flags.
BNR_FORMS = {
    "recompute": dict(mask="recompute", flags=1 | 32),
    "tensor": dict(mask="tensor", flags=1 | 8),
    "bits": dict(mask="bits", flags=1 | 16),
    "dual_resid": dict(mask="tensor", dual=True, resid=True, flags=1 | 2 | 4 | 8),
    "dual_bits": dict(mask="bits", dual=True, flags=1 | 2 | 16),
    "resid_bits": dict(mask="bits", resid=True, flags=1 | 4 | 16),
    "resid_sub": dict(mask="bits", resid=True, resid_sub=True, flags=1 | 4 | 16 | 128),
    "fold": dict(mask="recompute", fold=True, flags=1 | 32 | 64),
}


def conv_shapes(shape):
    N, H, W, C, K, R, s, p = shape
    return (H + 2 * p - R) // s + 1, (W + 2 * p - R) // s + 1


def _grid(shape, gen, lo=-32, hi=32, step=0.125):
    """bf16-exact values on a coarse grid (multiples of ``step``)."""
    return (torch.randint(lo, hi + 1, shape, generator=gen).float() * step).to(BF)


@functools.lru_cache(maxsize=None)
def conv_inputs(name):
    """The tensors of one conv case (CPU, fixed seed).  x / w / dy are unit normals scaled so that
    outputs are O(1) (xq / wq / biasq / residq: see below).  The BN-reduce operands: bx (the BatchNorm input the mask is recomputed from)
    lies on a grid of 1/8 with msc in {+-1, +-2} and msh an odd multiple of 1/16, so that
    |bx*msc + msh| >= 1/16 for every element -- no recomputed mask is anywhere near zero (the input
    condition of tests/test_image_truth_cpu.py holds by construction, also for the 3.8 M elements of
    the halo case)."""
    case = {**CONV_CASES, **BNR_STREAM_CASES}[name]
    N, H, W, C, K, R, s, p = case["shape"]
    P, Q = conv_shapes(case["shape"])
    gen = _gen(sum(ord(c) * (i + 1) for i, c in enumerate(name)))
    rn = lambda *sh, scale=1.0: (torch.randn(*sh, generator=gen) * scale).to(BF)  # noqa: E731
    d = dict(x=rn(N, H, W, C), w=rn(K, R, R, C, scale=(2.0 / (R * R * C)) ** 0.5), bias=torch.randn(K, generator=gen),
             resid=rn(N, P, Q, K), dy=rn(N, P, Q, K), wd=rn(K, R, R, C, scale=(2.0 / (R * R * K)) ** 0.5),
             dres=rn(N, H, W, C), dres_sub=rn(N, (H + 1) // 2, (W + 1) // 2, C), dw0=torch.randn(K, R, R, C, generator=gen))
    # the bias + residual + ReLU forward runs on coarse grids: x on 1/2 in [-2, 2], w on 1/4 in [-1, 1],
    # the residual on 1/8, the bias on odd multiples of 1/16.  Every partial sum is then exact in fp32
    # in any order (multiples of 1/16 below 2^24 of them), and the pre-activation is an odd multiple of
    # 1/16: never zero, never within rounding of it, whatever the reduction length
    d["xq"], d["wq"] = _grid((N, H, W, C), gen, -4, 4, 0.5), _grid((K, R, R, C), gen, -4, 4, 0.25)
    d["residq"] = _grid((N, P, Q, K), gen)
    d["biasq"] = (2 * torch.randint(-16, 16, (K,), generator=gen) + 1).float() / 16
    if "fwd_res" in case.get("ops", ()):   # residual + ReLU without a bias: the residual itself on odd multiples of 1/16
        d["residq_odd"] = ((2 * torch.randint(-32, 32, (N, P, Q, K), generator=gen) + 1).float() / 16).to(BF)
    d["bx"] = _grid((N, H, W, C), gen)
    d["bx2"] = rn(N, H, W, C)
    d["mean"], d["invstd"] = torch.randn(C, generator=gen) * 0.1, torch.rand(C, generator=gen) + 0.5
    d["mean2"], d["invstd2"] = torch.randn(C, generator=gen) * 0.1, torch.rand(C, generator=gen) + 0.5
    d["msc"] = torch.tensor([1.0, -1.0, 2.0, -2.0])[torch.randint(0, 4, (C,), generator=gen)]
    d["msh"] = (2 * torch.randint(-8, 8, (C,), generator=gen) + 1).float() / 16
    d["ymask"] = torch.relu(rn(N, H, W, C))
    # the dz fold's operands (1x1 stride-1 only): dy stands for g, fx for the BatchNorm input
    d["fx"] = rn(N, P, Q, K)
    d["fcoef"] = torch.stack([torch.rand(K, generator=gen) + 0.5, torch.randn(K, generator=gen) * 0.2,
                              torch.randn(K, generator=gen) * 0.1])
    # the activation fold's operands (WGRAD / FWD): x stands for z
    d["asc"], d["ash"] = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.5
    return d


@functools.lru_cache(maxsize=None)
def conv_truth(name, what):
    """Cached truths of a conv case: "fwd" (y, plain), "fwd_epi" (bias + residual + ReLU), "bwd"
    (dx and dw for dy, weights wd for dx / x for dw), "bwd_resid" (dx + dres), "bwd_sub" (dx + the
    sub-sampled residual), "bwd_fold" (dy folded)."""
    case = {**CONV_CASES, **BNR_STREAM_CASES}[name]
    N, H, W, C, K, R, s, p = case["shape"]
    d = conv_inputs(name)
    if what == "fwd":
        return conv(d["x"], d["w"], s, p)
    if what == "fwd_epi":
        return conv(d["xq"], d["wq"], s, p, d["biasq"], d["residq"], True)
    if what == "fwd_res":
        return conv(d["xq"], d["wq"], s, p, None, d["residq_odd"], True)
    if what == "dw":
        return conv(d["x"], d["w"], s, p, dy=d["dy"])["dw"]
    if what == "dx":
        return conv(d["x"], d["wd"], s, p, dy=d["dy"])["dx"]
    if what == "dx_fold":
        return conv(d["x"], d["wd"], s, p, dy=d["dy"], fold_x=d["fx"], fold_coef=d["fcoef"])["dx"]
    raise KeyError(what)


# WGRAD cases beyond the conv cases' own: (shape, knobs, tag, fold) -- fold in {None, "dz", "act", "both"}
WGRAD_CASES = {
    # 256x64 wide tile: gn = C = 64 (1x1), gm = K = 256; N*P*Q = 98 rows -> 2 K-steps, one split
    "w256x64": _case((2, 7, 7, 64, 256, 1, 1, 0), "wgrad_m32/256x64/ns1"),
    # several splits, the last short: N*P*Q = 3*19*19 = 1083 rows = 17 K-steps (the last of 59 rows);
    # gm = 64, gn = 576 -> 1 x 5 tiles of 64x128, min(ceil(1024/5), 17/8, 256) = 2 splits of 9 and 8
    "w_split": _case((3, 19, 19, 64, 64, 3, 1, 1), "wgrad_m32/64x128/ns2"),
    # the LDS-DMA 32x32x16 WGRAD (wgrad32.h): N = 64 images, C, K in {64, 128}; 2x2 and 3x3 outputs
    # (N*P*Q = 256 / 576 rows -> 4 / 9 K-steps, one split); the knob off gives the register-staged tiles
    "w_dma32_a": _case((64, 2, 2, 64, 128, 3, 1, 1), "wgrad_dma32/128x128/ns1"),
    "w_dma32_b": _case((64, 3, 3, 128, 64, 1, 1, 0), "wgrad_dma32/64x128/ns1"),
    "w_dma32_a_off": _case((64, 2, 2, 64, 128, 3, 1, 1), "wgrad_m32/128x128/ns1", knobs={"wgrad_dma32": 0}),
    "w_dma32_b_off": _case((64, 3, 3, 128, 64, 1, 1, 0), "wgrad_m32/64x128/ns1", knobs={"wgrad_dma32": 0}),
    # folds (1x1 stride 1, K % 8 == C % 8 == 0): dz on the A operand, the activation on B (needs
    # gm = K > 64: 128-row tiles), and both
    "w_fold_dz": _case((2, 7, 7, 64, 64, 1, 1, 0), "fold_wgrad_m32/64x64/ns1", fold="dz"),
    "w_fold_act": _case((2, 7, 7, 64, 136, 1, 1, 0), "fold_wgrad_m32/128x64/ns1", fold="act"),
    "w_fold_both": _case((2, 7, 7, 136, 72, 1, 1, 0), "fold_wgrad_m32/128x128/ns1", fold="both"),
    # wgrad_m32 = 0: the 16x16x32 form of the stem tile, the wide tile, 64x64 / 128x128 and of two fold tiles
    "w_stem_m16": _case((2, 9, 9, 8, 64, 7, 2, 3), "wgrad/64x256/ns1", knobs={"wgrad_m32": 0}),
    "w256x64_m16": _case((2, 7, 7, 64, 256, 1, 1, 0), "wgrad/256x64/ns1", knobs={"wgrad_m32": 0}),
    "w64x64_m16": _case((65, 1, 1, 64, 64, 1, 1, 0), "wgrad/64x64/ns1", knobs={"wgrad_m32": 0}),
    "w128x128_m16": _case((2, 14, 14, 24, 136, 3, 1, 1), "wgrad/128x128/ns1", knobs={"wgrad_m32": 0}),
    "w_fold_dz_m16": _case((2, 7, 7, 64, 64, 1, 1, 0), "fold_wgrad/64x64/ns1", knobs={"wgrad_m32": 0}, fold="dz"),
    "w_fold_both_m16": _case((2, 7, 7, 136, 72, 1, 1, 0), "fold_wgrad/128x128/ns1", knobs={"wgrad_m32": 0}, fold="both"),
}

# conv_fwd behind the BatchNorm-forward fold (in_scale / in_shift; 1x1 stride 1, C % 64 == 0), with
# statistics: gn = 64 -> the fold's 128x64 tile, gn = 136 -> 128x128, and the expanding 64 -> 256 conv
# at 32 rows, which the streaming FWD takes in its fold form.
FWD_FOLD_CASES = {
    "ffold64": _case((2, 7, 7, 64, 64, 1, 1, 0), "fold/128x64"),
    "ffold136": _case((2, 7, 7, 128, 136, 1, 1, 0), "fold/128x128"),
    "ffold_stream": _case((2, 4, 4, 64, 256, 1, 1, 0), "fwd_stream/32x256"),
}


@functools.lru_cache(maxsize=None)
def fwd_fold_inputs(name):
    """z on a grid of 1/8, scale in {+-1, +-2}, shift an odd multiple of 1/16: |scale*z + shift| >= 1/16
    and relu(scale*z + shift) is exact in bf16 (multiples of 1/16 below 16)."""
    N, H, W, C, K, R, s, p = FWD_FOLD_CASES[name]["shape"]
    gen = _gen(11 + sum(ord(c) * (i + 1) for i, c in enumerate(name)))
    return dict(z=_grid((N, H, W, C), gen), w=(torch.randn(K, R, R, C, generator=gen) * (2.0 / C) ** 0.5).to(BF),
                scale=torch.tensor([1.0, -1.0, 2.0, -2.0])[torch.randint(0, 4, (C,), generator=gen)],
                shift=(2 * torch.randint(-8, 8, (C,), generator=gen) + 1).float() / 16)


@functools.lru_cache(maxsize=None)
def wgrad_inputs(name):
    case = WGRAD_CASES[name]
    N, H, W, C, K, R, s, p = case["shape"]
    P, Q = conv_shapes(case["shape"])
    gen = _gen(7 + sum(ord(c) * (i + 1) for i, c in enumerate(name)))
    rn = lambda *sh, scale=1.0: (torch.randn(*sh, generator=gen) * scale).to(BF)  # noqa: E731
    return dict(x=rn(N, H, W, C), dy=rn(N, P, Q, K), dw0=torch.randn(K, R, R, C, generator=gen), fx=rn(N, P, Q, K),
                fcoef=torch.stack([torch.rand(K, generator=gen) + 0.5, torch.randn(K, generator=gen) * 0.2,
                                   torch.randn(K, generator=gen) * 0.1]),
                asc=torch.rand(C, generator=gen) + 0.5, ash=torch.randn(C, generator=gen) * 0.5)


# ------------------------------------------------------------------------------ BatchNorm cases
# (M, C): C in {8, 64, 2048} takes the vector kernels (256 % (C/8) == 0: ew2_ok), 24 and 136 the
# generic ones.  With ew_unroll = 4 the vector kernels run ceil8(ceil(nvec / 1024)) blocks of 256
# threads over nvec = M*C/8 vectors: at nvec = 16320 (C = 64) and 16128 (C = 2048) that is T = 4096
# threads of which nvec - 3T take the 4-deep unrolled body once and the others the remainder loop.
# M = 1 (a single-row launch: empty unrolled body, one partial row, var = 0) on a vector (64) and a
# generic (24) channel count; its truth is batchnorm_one_row.
BN_SHAPES = [(1, 64), (1, 24), (50, 8), (37, 24), (2040, 64), (300, 136), (63, 2048)]
BN_MODES = ["none", "resid", "bn2"]


@functools.lru_cache(maxsize=None)
def bn_case(M, C, mode, relu, dtype=BF):
    """``dtype``: the activation type x / x2 / dy are stored in (bf16 rounds them; fp32 keeps the full
    mantissa of the same draws).  The fp32 single-row case scales x (and x2) by 2^-18: y = scale*x + shift
    then cancels two terms of about 0.005 instead of 1e3, whose fp32 rounding (6e-8 relative) stays below a
    quarter of the fp32 criterion even where beta + beta2 leaves a y of 1e-3; x^2, inexact in fp32, then
    is nothing against eps in var + eps.  Resamples the seed until no ReLU pre-activation is within 1e-5 of its terms of zero and no
    channel is switched off as a whole (beta is small against the unit-variance BN output; at M = 1 a
    channel is its one element, and the ReLU switches about half of them off)."""
    for seed in range(100 * M + C, 100 * M + C + 50):
        gen = _gen(seed + 7 * BN_MODES.index(mode) + (3 if relu else 0))
        rn = lambda *sh: torch.randn(*sh, generator=gen)  # noqa: E731
        # (M = 1: y is beta itself against terms of gamma*rsqrt(eps)*|x| ~ 1e3, so |beta| >= 0.2)
        beta = rn(C) * 0.3 if M > 1 else (torch.rand(C, generator=gen) * 0.5 + 0.2) * (2 * torch.randint(0, 2, (C,), generator=gen) - 1)
        xs = 2.0 ** -18 if (M == 1 and dtype == torch.float32) else 1.0
        d = dict(x=((rn(M, C) * 2 + 0.5) * xs).to(dtype), gamma=torch.rand(C, generator=gen) + 0.5, beta=beta,
                 rm=rn(C) * 0.1, rv=torch.rand(C, generator=gen) + 0.5, dy=rn(M, C).to(dtype), x2=None, gamma2=None,
                 beta2=None, rm2=None, rv2=None)
        if mode != "none":
            d["x2"] = (rn(M, C) * xs).to(dtype)
        if mode == "bn2":
            d.update(gamma2=torch.rand(C, generator=gen) + 0.5, beta2=rn(C) * 0.3, rm2=rn(C) * 0.1,
                     rv2=torch.rand(C, generator=gen) + 0.5)
        t = (batchnorm if M > 1 else batchnorm_one_row)(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"], 0.1, 1e-5, d["x2"],
                                                        d["gamma2"], d["beta2"], d["rm2"], d["rv2"], relu, d["dy"])
        # (M = 1 also without a ReLU: y = scale*x + shift is then beta plus the cancellation noise of two
        # fp32 terms of size gamma*rsqrt(eps)*|x|, and the same condition keeps every y well above it)
        if not (relu or M == 1) or (bool((t["pre"].abs() >= 1e-5 * t["terms"]).all())
                                    and (M == 1 or bool((t["y"].amax(0) > 0).all()))):
            d["truth"] = t
            return d
    raise AssertionError("bn_case: no seed satisfies the ReLU condition")


# ------------------------------------------------------------------------------ pooling cases
POOL_SHAPES = [(2, 17, 17, 64), (1, 28, 28, 8), (3, 17, 23, 72)]


def pool_ties(xe):
    """Number of 3x3 / stride-2 / pad-1 windows of NHWC ``xe`` whose maximum is positive and attained
    more than once (the argmax, hence the backward, is then a matter of convention)."""
    N, H, W, C = xe.shape
    xp = F.pad(xe.double().permute(0, 3, 1, 2).reshape(N * C, 1, H, W), (1, 1, 1, 1), value=float("-inf"))
    u = F.unfold(xp, 3, stride=2)
    m = u.amax(1, keepdim=True)
    return int((((u == m).sum(1, keepdim=True) > 1) & (m > 0)).sum())


def prologue_bf16(x, scale, shift):
    """The pooled tensor as an implementation sees it: relu(scale*x + shift) in fp32, rounded to bf16
    (scale a power of two: one rounding whether or not the multiply-add is fused)."""
    return torch.relu(x.float() * scale + shift).to(BF)


@functools.lru_cache(maxsize=None)
def pool_case(shape, dtype=BF):
    """``dtype``: the activation type (x is integer-valued and exact in both; dy / gdy keep their full
    mantissa in fp32).  x = 8*l + j - 36 with l a per-plane permutation of 0..8 indexed by (h % 3, w % 3) and j a random
    0..7 per pixel: any 3x3 window holds nine different l, hence nine distinct bf16-exact integers in
    [-36, 35] -- no window ties.  The prologue's scale is 0.5, 1 or 2 and its shift an integer in
    [-12, 12] plus 1/4: scale*x + shift is never within 1/4 of zero, is exact in bf16 below 64 and
    keeps distinct inputs distinct above (even integers + 1/4 on a grid of 1/2).  The seed is
    resampled should a window of the rounded prologue output still tie at a positive maximum (zeros
    tie only where the maximum is not positive)."""
    N, H, W, C = shape
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    cls = (3 * (torch.arange(H) % 3).view(H, 1) + (torch.arange(W) % 3).view(1, W)).reshape(-1)
    for seed in range(50):
        gen = _gen(N * 1000 + H * 10 + W + C + 7919 * seed)
        lv = torch.stack([torch.randperm(9, generator=gen)[cls] for _ in range(N * C)]).reshape(N, C, H, W)
        x = (8 * lv + torch.randint(0, 8, (N, C, H, W), generator=gen) - 36).float()
        x = x.permute(0, 2, 3, 1).contiguous().to(dtype)
        d = dict(x=x, dy=torch.randn(N, P, Q, C, generator=gen).to(dtype),
                 scale=torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=gen)],
                 shift=torch.randint(-12, 13, (C,), generator=gen).float() + 0.25,
                 mean=torch.randn(C, generator=gen) * 0.1, invstd=torch.rand(C, generator=gen) + 0.5,
                 gdy=torch.randn(N, C, generator=gen).to(dtype))
        if pool_ties(x) == 0 and pool_ties(prologue_bf16(x, d["scale"], d["shift"]).to(dtype)) == 0:
            return d
    raise AssertionError("pool_case: no seed without window ties")


# ------------------------------------------------------------------------------ optimizer cases
# n = 4 (one vector), 4*257 (a second block of one vector), 4*(256*2048) + 12 (flat_grid caps at 2048
# blocks of 256 threads: three vectors make a second trip of the grid-stride loop)
OPT_SIZES = [4, 4 * 257, 4 * (256 * 2048) + 12]


@functools.lru_cache(maxsize=None)
def opt_case(n):
    gen = _gen(n)
    return dict(w=torch.randn(n, generator=gen), grads=[torch.randn(n, generator=gen) for _ in range(3)],
                m1=torch.randn(n, generator=gen) * 0.1, m2=torch.rand(n, generator=gen) * 0.01 + 1e-4,
                mask=(torch.rand(n, generator=gen) < 0.5).to(torch.uint8))
