"""fp64 truths of the Linear GEMMs (``linear_gelu_fwd``, ``linear_dgrad_gelu`` and the plain / residual
DGRAD of a Linear layer through ``conv_dgrad``) and the cases tests/test_linear_truth_cpu.py and
tests/test_linear_truth_gpu.py judge.

As in ``ops/truth_image.py``: every truth is plain fp64 torch on the values the bf16 inputs hold, with
no intermediate rounding -- ``u = x W^T + b``, ``g = gelu(u)`` with erf, ``dx = dy W (+ resid)`` and
``du = (dy W) * gelu'(u_in)`` for a given bf16 ``u_in``.  Everything lives on the CPU, built from fixed
seeds and cached per *shape*: the planner cases, which differ only in the kernel they force, share one
set of inputs and truths.

Shapes are ``(M, C, N)``: the FWD reads x [M, C] and w [N, C] (gm = M, gn = N, gk = C); the DGRAD reads
dy [M, N] and w [N, C] and reduces over N (gm = M, gn = C, gk = N).
"""
from __future__ import annotations

import functools

import torch

from .truth import assert_elementwise, gelu, norm_err, seg_rows  # noqa: F401  (re-exported)
from .truth_image import BASE_KNOBS, BF, _case, _gen, _grid, seg_ch  # noqa: F401  (re-exported)

# the outputs a case runs and commits a tag for: "fwd" (linear_gelu_fwd: u and g), "du"
# (linear_dgrad_gelu), "dx" / "dx_resid" (conv_dgrad of the [M, 1, 1, N] views, plain / into a residual)
FORMS = ("fwd", "du", "dx", "dx_resid")
# conv_kernel_choice (mode, flags) of each form: FWD bias + GELU; DGRAD GELU', plain, residual
TAG_FLAGS = {"fwd": (0, 2 | 32), "du": (1, 256), "dx": (1, 0), "dx_resid": (1, 4)}


def _lin(shape, tags, knobs=None, dshape=None, **kw):
    return _case(shape, tags, knobs, dshape=dshape or shape, **kw)


# Static dispatch (BASE_KNOBS: gemm_plan = 0, fwd_split_target = 1 -> fwd_route returns FWD_PLAIN,
# dgrad_route DGRAD_DISPATCH, both choose_kernel; csrc/igemm_launch.h, BK = 64).  With a GELU epilogue
# p.relu >= 2: use_dma32 and halo_geom refuse, so a dma4 case stays on igemm_dma_kernel.  Each runs
# FWD + GELU and DGRAD * GELU' unless its tags say otherwise.
STATIC_CASES = {
    # FWD gm = 5 (<= 32), gn = 16 (<= 64): default_bm / default_bn -> 32x64, C = 256: uniform walk.
    # DGRAD gn = 256, gk = 16: K % 64 != 0 -> no DMA kernel, per-element walk over less than one K-tile;
    # gm <= 32 -> 32x128
    "g5": _lin((5, 256, 16), dict(fwd="reg/32x64", du="reg/32x128")),
    # FWD gm = 33 (one past the 32-row tile: 32 < gm <= 64 -> 64 rows), gn = 72 (> 64 -> 128 columns, a
    # tail of 8 behind the first 64), one K-tile (use_dma4 asks for 3).  DGRAD gn = 64, gk = 72 -> 64x64
    "g33": _lin((33, 64, 72), dict(fwd="reg/64x128", du="reg/64x64")),
    # FWD gm = 129 > 64, gn = 136 > 64, 2 x 2 tiles of 128x128 < 256: use_bm64_smallgrid (no statistics)
    # -> 64x128, the third row tile holds one row.  DGRAD gn = 64 (not > 64: no small-grid tile), gk = 136
    # (K % 64 != 0: no DMA) -> 128x64 with a second row tile of one row
    "g129": _lin((129, 64, 136), dict(fwd="reg_smallgrid/64x128", du="reg/128x64")),
    # C = 24 and a DGRAD reduction of 136: neither a multiple of 64 -> the per-element tap walk both ways.
    # FWD gm = 392, gn = 136: 4 x 2 tiles < 256 -> small-grid 64x128; DGRAD gn = 24 <= 64 -> 128x64
    "goff": _lin((392, 24, 136), dict(fwd="reg_smallgrid/64x128", du="reg/128x64")),
    # gm = 147 (> 64; row tail of 19), gn = 192 (a half-empty second column tile), 3 K-tiles.  At the
    # default knobs use_bm64_smallgrid (2 x 2 tiles < 256) comes before use_dma4 in choose_kernel, in
    # both modes: 64x128 with three K-tiles on the uniform walk ...
    "gdma_default": _lin((147, 192, 192), dict(fwd="reg_smallgrid/64x128", du="reg_smallgrid/64x128")),
    # ... so igemm_dma_kernel takes bm64_smallgrid = 0: use_dma4 (cin % 64 == 0, gk / 64 = 3 >= 3, gm > 64,
    # gn > 64) gives a FWD grid of fewer than 256 tiles case 2 (dma4_small_n64 = 1: 128x64) and a DGRAD
    # case 1 (128x128); use_dma32 refuses p.relu >= 2
    "gdma": _lin((147, 192, 192), dict(fwd="dma4/128x64", du="dma4/128x128"), knobs={"bm64_smallgrid": 0}),
    # dma4_small_n64 = 0: the FWD on 128x128 as well
    "gdma_128": _lin((147, 192, 192), dict(fwd="dma4/128x128"), knobs={"bm64_smallgrid": 0, "dma4_small_n64": 0}),
    # gn <= 64 (no small-grid tile: it asks for gn > 64): use_dma4's dma4_n64 = 1 -> case 2, 128x64, in
    # both modes (FWD gn = N = 64; the mirrored DGRAD gn = C = 64, gk = 192)
    "gdma_n64": _lin((147, 192, 64), dict(fwd="dma4/128x64", du="dma4/128x64"), dshape=(147, 64, 192)),
    # 8-wave 256x256: use_igemm8 with igemm8_min_tiles = 1: gn = 256 (>= 256), gk = 512 = 8 K-tiles (>= 8),
    # gm = 300 -> 2 x 1 tiles, the second with 44 rows; it precedes the small-grid tile in choose_kernel
    "g8w": _lin((300, 512, 256), dict(fwd="dma8/256x256", du="dma8/256x256"), knobs={"igemm8_min_tiles": 1},
                dshape=(300, 256, 512)),
    # FWD_SPLIT: gm = 49 -> 1 x 2 tiles of 64x128 (< 128), 13 K-steps (>= 8), fwd_split_target = 256 ->
    # min(ceil(256 / 2), 13 / fwd_split_mink = 3, 32) = 3 splits, set_split: ceil(13 / 3) = 5 K-steps each
    # -> 5 + 5 + 3; choose_kernel with nsplit = 3 keeps the register-staged default tile; the partials go
    # through splitk_epilogue_kernel with relu == 2
    "gsplit": _lin((49, 832, 136), dict(fwd="reg/64x128/ns3"), knobs={"fwd_split_target": 256, "fwd_split_mink": 4}),
}

# Planner (csrc/igemm_plan.h; gemm_plan = 1, plan_force, plan_nsplit).  Small M: (49, 832, 136) is
# fwd_route's FWD_PLAN_SMALL_M (the split heuristic above; gm < 1024 keeps it off plain_gemm_eligible);
# plan_candidate_list offers kinds 3 and 4 (gm <= 256) at ns in {1, 2, 4} (13 / 8 < 2 ends the list):
# 1 split, and 4 splits of 4 + 4 + 4 + 1 K-steps into splitk_epilogue_kernel.
SMALL_KINDS = {3: "reg64x64", 4: "reg32x64"}
SMALL_CASES = {
    f"plan_{_n}_ns{_ns}": _lin((49, 832, 136), dict(fwd=f"plan/{_n}/ns{_ns}"),
                               knobs={"gemm_plan": 1, "plan_force": _k, "plan_nsplit": _ns, "fwd_split_target": 256,
                                      "fwd_split_mink": 4})
    for _k, _n in SMALL_KINDS.items() for _ns in (1, 4)}
# kind 6 (skinny) asks for p.relu < 2 in plan_candidate_list: a GELU call has no such candidate, the
# forced list stays unrestricted and the tag is "plan/auto" -- a timed choice, asserted and not run
SMALL_REFUSED = _lin((49, 832, 136), dict(fwd="plan/auto"),
                     knobs={"gemm_plan": 1, "plan_force": 6, "plan_nsplit": 1, "fwd_split_target": 256, "fwd_split_mink": 4})

# Large M: plain_gemm_eligible in both modes (1x1, gm = 1030 >= 1024, 13 K-tiles of a reduction of 832,
# gn = 264: % 8 == 0 and >= 256 for kinds 2 and 10, <= 1024 for kind 5).  1 split, and 3 (13 / 3 >= 4)
# of 5 + 5 + 3 K-tiles: the last one short.  The DGRAD is that of the mirrored layer: dy [1030, 832],
# w [832, 264].  A residual or the GELU' operand does not enter the plan's candidates: one tag per case.
LARGE_KINDS = {1: "dma128x128", 2: "dma256x256", 5: "dma128x64", 9: "m32_128x128", 10: "m32_256x256"}
LARGE_CASES = {
    f"plan_{_n}_ns{_ns}": _lin((1030, 832, 264), {f: f"plan/{_n}/ns{_ns}" for f in FORMS},
                               knobs={"gemm_plan": 1, "plan_force": _k, "plan_nsplit": _ns}, dshape=(1030, 264, 832))
    for _k, _n in LARGE_KINDS.items() for _ns in (1, 3)}

# Tails: the g33 shape with the rows of x and u_in scaled by 1, 2, 4 in turn (|u| up to about 17): the
# region where 1 + erf cancels and __expf underflows in gelu_fast / dgelu_fast.  Judged per row.
TAILS_CASES = {"gtails": _lin((33, 64, 72), dict(fwd="reg/64x128", du="reg/64x64"), tails=True)}

ALL_CASES = {**STATIC_CASES, **{"small_" + n: c for n, c in SMALL_CASES.items()},
             **{"large_" + n: c for n, c in LARGE_CASES.items()}, **TAILS_CASES}


def forms(case):
    return tuple(f for f in FORMS if f in case["tags"])


def is_tails(case):
    return bool(case.get("tails"))


# ------------------------------------------------------------------------------ inputs
def _row_scale(M):
    return torch.tensor([1.0, 2.0, 4.0])[torch.arange(M) % 3].view(M, 1)


# |u| beyond which exp(-u^2 / 2) is below 2^-149, the smallest fp32 denormal: __expf gives 0 there and
# 1 + erf has cancelled completely long before (1 - y*t*e rounds to 1 from |u| = 5.55 on in fp32)
TAILS_REACH = 14.5


@functools.lru_cache(maxsize=None)
def fwd_inputs(shape, tails=False):
    """x a unit normal, w scaled by fan_in ** -0.5, the bias 0.5 * N(0, 1) (fp32).  Grid inputs: xq on a
    grid of 1/2 in [-2, 2], wq on 1/4 in [-1, 1], biasq on 1/8 in [-4, 4]: every product and every
    partial sum is a multiple of 1/8 far below 2^24 of them, hence exact in fp32 in any order.
    ``tails``: the rows of x scaled by 1, 2, 4 in turn; the seed is resampled until the fp64 u falls
    below -TAILS_REACH (an input condition, about one seed in eight meets it; beyond +5.55 the GELU is the
    identity in fp32 whatever __expf gives, so the positive side asks for nothing)."""
    M, C, N = shape
    for seed in range(50 if tails else 1):
        gen = _gen(1000003 * M + 1009 * C + N + (5 + 7919 * seed if tails else 0))
        x = torch.randn(M, C, generator=gen).to(BF)
        if tails:
            x = x * _row_scale(M).to(BF)      # powers of two: exact
        d = dict(x=x, w=(torch.randn(N, C, generator=gen) * C ** -0.5).to(BF), bias=0.5 * torch.randn(N, generator=gen),
                 xq=_grid((M, C), gen, -4, 4, 0.5), wq=_grid((N, C), gen, -4, 4, 0.25),
                 biasq=torch.randint(-32, 33, (N,), generator=gen).float() * 0.125)
        u = linear(d["x"], d["w"], d["bias"])["u"]
        if not tails or float(u.min()) < -TAILS_REACH:
            return d
    raise AssertionError("fwd_inputs: no seed reaches the tails")


@functools.lru_cache(maxsize=None)
def dgrad_inputs(dshape, tails=False):
    """dy a unit normal, w [N, C] scaled by the DGRAD's fan_in N ** -0.5, u_in 1.5 * N(0, 1), the residual
    a unit normal.  Grid inputs as in ``fwd_inputs``, the residual on 1/8 in [-4, 4].  ``tails``: the
    rows of u_in scaled by 1, 2, 4 in turn, resampled until u_in passes TAILS_REACH on both sides."""
    M, C, N = dshape
    for seed in range(50 if tails else 1):
        gen = _gen(7 + 1000003 * M + 1009 * C + N + (5 + 7919 * seed if tails else 0))
        u_in = (1.5 * torch.randn(M, C, generator=gen)).to(BF)
        if tails:
            u_in = u_in * _row_scale(M).to(BF)
        d = dict(dy=torch.randn(M, N, generator=gen).to(BF), w=(torch.randn(N, C, generator=gen) * N ** -0.5).to(BF),
                 u_in=u_in, resid=torch.randn(M, C, generator=gen).to(BF),
                 dyq=_grid((M, N), gen, -4, 4, 0.5), wq=_grid((N, C), gen, -4, 4, 0.25), residq=_grid((M, C), gen, -32, 32, 0.125))
        if not tails or (float(u_in.min()) < -TAILS_REACH and float(u_in.max()) > TAILS_REACH):
            return d
    raise AssertionError("dgrad_inputs: no seed reaches the tails")


# ------------------------------------------------------------------------------ truths
def linear(x, w, bias=None):
    """{"u": x W^T + b, "g": gelu(u)} in fp64."""
    u = x.double() @ w.double().t()
    if bias is not None:
        u = u + bias.double()
    return {"u": u, "g": gelu(u)[0]}


def linear_dgrad(dy, w, resid=None, u_in=None):
    """{"dx": dy W, "dx_resid": dx + resid, "du": dx * gelu'(u_in)} in fp64 (gelu' by autograd)."""
    dx = dy.double() @ w.double()
    out = {"dx": dx}
    if resid is not None:
        out["dx_resid"] = dx + resid.double()
    if u_in is not None:
        out["du"] = gelu(u_in, dx)[1]
    return out


@functools.lru_cache(maxsize=None)
def fwd_truth(shape, tails=False, grid=False):
    d = fwd_inputs(shape, tails)
    return linear(d["xq"], d["wq"], d["biasq"]) if grid else linear(d["x"], d["w"], d["bias"])


@functools.lru_cache(maxsize=None)
def dgrad_truth(dshape, tails=False, grid=False):
    d = dgrad_inputs(dshape, tails)
    if grid:
        return linear_dgrad(d["dyq"], d["wq"], d["residq"])
    return linear_dgrad(d["dy"], d["w"], d["resid"], d["u_in"])


def grid_terms(case):
    """The largest sum of |terms| of a grid output of the case, in units of the grid step 1/8: below
    2^24 every fp32 partial sum is exact in any order."""
    worst = 0.0
    if "fwd" in case["tags"]:
        d = fwd_inputs(case["shape"], is_tails(case))
        worst = max(worst, float((d["xq"].double().abs() @ d["wq"].double().abs().t() + d["biasq"].double().abs()).max()))
    if "dx" in case["tags"] or "dx_resid" in case["tags"]:
        d = dgrad_inputs(case["dshape"], is_tails(case))
        worst = max(worst, float((d["dyq"].double().abs() @ d["wq"].double().abs() + d["residq"].double().abs()).max()))
    return worst / 0.125


def tanh_gelu(u):
    """The tanh approximation of GELU, fp64 (what the tests do *not* tell from erf-GELU)."""
    u = u.double()
    return 0.5 * u * (1.0 + torch.tanh(0.7978845608028654 * (u + 0.044715 * u ** 3)))
