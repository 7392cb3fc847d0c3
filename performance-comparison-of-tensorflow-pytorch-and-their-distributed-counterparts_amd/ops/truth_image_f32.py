"""The fp32 image path (csrc/f32.hip, ``--dtype fp32``) against the fp64 truths of ``ops/truth_image.py``:
the conv cases tests/test_image_truth_f32_cpu.py and tests/test_image_truth_f32_gpu.py judge, their
inputs and their truths.  The BatchNorm and pooling cases are those of ``truth_image.py`` with
``dtype=torch.float32``.

Every conv case has two sets of inputs:

* *grid* inputs, the grids of the bf16 harness cast to fp32: x and dy on multiples of 1/2 in [-2, 2], w
  on 1/4 in [-1, 1], the residuals and dw0 on 1/8 in [-4, 4], the bias on odd multiples of 1/16; the
  folded activation z on 1/8 with scale in {+-1, +-2} and shift an odd multiple of 1/16, so that
  relu(scale*z + shift) is a multiple of 1/16 below 9.  Every product and every partial sum is then a
  small multiple of a power of two and exact in fp32 in any order (``exact_units`` bounds the worst
  output element by 2^24 units of the finest grid step; the CPU test asserts it).  The fp32 kernels are
  exact-fp32 fma chains, so whatever the tile shape and the split count they must return the fp64
  truth *bit for bit*: these cases carry no tolerance.
* *random* inputs, fp32 normals with their full mantissa (not rounded through bf16), held to
  ``seg_rel < 1e-5`` per segment (one channel of an activation, one output-channel row of dw, one
  [C] row of the statistics).

The statistics partials are compared row by row: row t of ``part`` against the fp64 sums of the
implementation's own y over the rows that tile covers (``rows_per`` rows: BM without a split, 16 after
one -- csrc/f32.hip splitk_epilogue_kernel; everything in one row for ``ops/ref.py``).
"""
from __future__ import annotations

import functools

import torch

from . import truth_image as T

F32 = torch.float32

# ==============================================================================  cases
# shape (N, H, W, C, K, R, stride, pad); FWD gm = N*P*Q, gn = K, gk = R*R*C; DGRAD gm = N*H*W, gn = C,
# gk = R*R*K; WGRAD gm = K, gn = R*R*C, gk = N*P*Q.  The derivations quote plan_f32 (csrc/f32.hip),
# nk = ceil(gk / 32):
#   big      igemm_f32_big_kernel if f32_big and (FWD: C % 16 == 0; DGRAD: K % 16 == 0; WGRAD: always),
#            else igemm_f32_kernel (64x64)
#   tiles    bm = 64 if gm <= 64 else 128, bn likewise; shortk = FWD / DGRAD with nk <= f32_shortk (4);
#            tt = f32_blocks (256) or, WGRAD, f32_wgrad_blocks (2048; 1x1: f32_wgrad_blocks_1x1, 512);
#            bn, then bm, drop to 64 while shortk or ceil(gm/bm)*ceil(gn/bn) < tt
#   split    WGRAD: ns = min(ceil(tt / tiles), ceil(nk / 32)); FWD / DGRAD with tiles < f32_blocks:
#            ns = min(ceil(f32_blocks / tiles), nk // f32_split_steps (4)), at least 1; with tiles >=
#            f32_blocks on the big kernel and nk >= f32_qsplit_mink: the s <= f32_qsplit (5) with nk // s
#            >= 4 that fills whole waves of f32_blocks best, if it gains f32_qgain percent
#   ksplit = 32 * ceil(ceil(gk / ns) / 32), nsplit = ceil(gk / ksplit)
# Every shape this small has fewer than 256 tiles, so the default knobs give 64x64 tiles and a split
# wherever nk >= 8; BIG128 (every block target 1: nothing is below it) keeps the 128-wide tiles of every
# dimension above 64 and never splits.  Tag keys: "fwd", "fwd_fold" (flags 1), "dgrad", "wgrad",
# "wgrad_fold" (flags 1).
BIG128 = {"f32_blocks": 1, "f32_wgrad_blocks": 1, "f32_wgrad_blocks_1x1": 1}
QSPLIT = {"f32_blocks": 3, "f32_qsplit_mink": 1, "f32_qgain": 0}
# every f32 knob a case may set, with its default (the CPU test asserts they are back afterwards)
KNOB_DEFAULTS = {"f32_big": 1, "f32_split": 1, "f32_blocks": 256, "f32_split_steps": 4, "f32_shortk": 4,
                 "f32_wgrad_blocks": 2048, "f32_wgrad_blocks_1x1": 512, "f32_qsplit": 5, "f32_qgain": 10,
                 "f32_qsplit_mink": 64, "f32_fold": 1}


def _case(shape, tags, knobs=None):
    return dict(shape=shape, tags=tags, knobs=dict(knobs or {}))


F32_CONV_CASES = {
    # Linear, 5 rows: FWD gm = 5, gn = 12, nk = 2 -> big (C = 64), one 64x64 tile, nk // 4 = 0 -> ns1.
    # DGRAD K = 12 (% 16 != 0): the small kernel's natural fallback, gk = 12 (% 16 != 0), ns1.  WGRAD gm = 12,
    # gn = 64, gk = 5 (odd): 64x64, ceil(1 / 32) = 1 -> ns1
    "lin5": _case((5, 1, 1, 64, 12, 1, 1, 0),
                  dict(fwd="f32_big/64x64/ns1", fwd_fold="f32_big/64x64/ns1/fold", dgrad="f32_small/64x64/ns1",
                       wgrad="f32_big/64x64/ns1", wgrad_fold="f32_big/64x64/ns1/apply")),
    # gm = 33 (<= 64), gn = 72 (> 64), nk = 5 (> shortk) under BIG128 -> 64x128.  DGRAD K = 72 -> small,
    # gk = 72 (% 16 = 8).  WGRAD gm = 72, gn = 160 -> 128x128, gk = 33 (odd)
    "gm33": _case((33, 1, 1, 160, 72, 1, 1, 0),
                  dict(fwd="f32_big/64x128/ns1", dgrad="f32_small/64x64/ns1", wgrad="f32_big/128x128/ns1"), BIG128),
    # gm = 65 (a second 64-row half of one row), gn = 64 -> 128x64.  DGRAD gm = 65, gn = 160 would take
    # 128x128, but gk = 64 -> nk = 2 <= f32_shortk -> 64x64 (the shortk rule).  WGRAD gm = 64, gn = 160 -> 64x128
    "gm65": _case((65, 1, 1, 160, 64, 1, 1, 0),
                  dict(fwd="f32_big/128x64/ns1", dgrad="f32_big/64x64/ns1", wgrad="f32_big/64x128/ns1"), BIG128),
    # gm = 129 (a second 128-row tile of one row), gn = 136 (a second column tile of 8) -> 128x128.  DGRAD
    # K = 136 (% 16 = 8) -> small.  WGRAD gm = 136, gn = 160, gk = 129 -> 128x128
    "gm129": _case((129, 1, 1, 160, 136, 1, 1, 0),
                   dict(fwd="f32_big/128x128/ns1", dgrad="f32_small/64x64/ns1", wgrad="f32_big/128x128/ns1"), BIG128),
    # 128x128 in all three modes, 3x3: FWD gm = 162, gn = 80, nk = 41; DGRAD gm = 162, gn = 144, nk = 23;
    # WGRAD gm = 80, gn = 1296, gk = 162
    "t128": _case((2, 9, 9, 144, 80, 3, 1, 1),
                  dict(fwd="f32_big/128x128/ns1", fwd_fold="f32_big/128x128/ns1/fold", dgrad="f32_big/128x128/ns1",
                       wgrad="f32_big/128x128/ns1"), BIG128),
    # 128x64 FWD (gm = 162, gn = 64, nk = 9) and DGRAD (gn = 32, nk = 18); WGRAD gm = 64, gn = 288 -> 64x128
    "t128x64": _case((2, 9, 9, 32, 64, 3, 1, 1),
                     dict(fwd="f32_big/128x64/ns1", dgrad="f32_big/128x64/ns1", wgrad="f32_big/64x128/ns1"), BIG128),
    # 128x64 WGRAD: gm = K = 80, gn = C = 64 (1x1).  FWD gm = 162, gn = 80 would take 128x128, but nk = 2 ->
    # the shortk rule's 64x64; DGRAD nk = 3 likewise
    "w128x64": _case((2, 9, 9, 64, 80, 1, 1, 0),
                     dict(fwd="f32_big/64x64/ns1", dgrad="f32_big/64x64/ns1", wgrad="f32_big/128x64/ns1"), BIG128),
    # 64x128 DGRAD: gm = 49, gn = 80, nk = 14.  FWD gm = 49, gn = 48 -> 64x64; WGRAD gm = 48, gn = 720 -> 64x128
    "d64x128": _case((1, 7, 7, 80, 48, 3, 1, 1),
                     dict(fwd="f32_big/64x64/ns1", dgrad="f32_big/64x128/ns1", wgrad="f32_big/64x128/ns1"), BIG128),
    # stride-2 3x3 through the 128x128 tiles: FWD gm = 98, gn = 128, nk = 36; DGRAD gm = 392 (a 4th row tile
    # of 8), gn = 128, nk = 36; WGRAD gm = 128, gn = 1152, gk = 98
    "s2": _case((2, 14, 14, 128, 128, 3, 2, 1),
                dict(fwd="f32_big/128x128/ns1", fwd_fold="f32_big/128x128/ns1/fold", dgrad="f32_big/128x128/ns1",
                     wgrad="f32_big/128x128/ns1"), BIG128),
    # default knobs, a split with a short last part: FWD / DGRAD gm = 98, gn = 48 -> 2 tiles of 64x64,
    # gk = 432, nk = 14 -> min(128, 3) = 3 splits of ksplit = 160: 160 + 160 + 112.  WGRAD gk = 98 -> ns1
    "split": _case((2, 7, 7, 48, 48, 3, 1, 1),
                   dict(fwd="f32_big/64x64/ns3", fwd_fold="f32_big/64x64/ns3/fold", dgrad="f32_big/64x64/ns3",
                        wgrad="f32_big/64x64/ns1")),
    # ... the same FWD / DGRAD unsplit (f32_split = 0; nk = 14 < f32_qsplit_mink: no quantisation split either)
    "split_ns1": _case((2, 7, 7, 48, 48, 3, 1, 1), dict(fwd="f32_big/64x64/ns1", dgrad="f32_big/64x64/ns1"),
                       {"f32_split": 0}),
    # ... and the same through f32_big = 0: the small kernel in all three modes, FWD / DGRAD ns3
    "split_small": _case((2, 7, 7, 48, 48, 3, 1, 1),
                         dict(fwd="f32_small/64x64/ns3", fwd_fold="f32_small/64x64/ns3/apply", dgrad="f32_small/64x64/ns3",
                              wgrad="f32_small/64x64/ns1", wgrad_fold="f32_small/64x64/ns1/apply"), {"f32_big": 0}),
    # DGRAD's natural fallback with a split: K = 40 (% 16 = 8), gk = 360, nk = 12 -> 3 splits of 128: 128 +
    # 128 + 104.  FWD (C = 48) big, gk = 432 -> ns3; WGRAD gm = 40, gn = 432, gk = 98
    "k40": _case((2, 7, 7, 48, 40, 3, 1, 1),
                 dict(fwd="f32_big/64x64/ns3", dgrad="f32_small/64x64/ns3", wgrad="f32_big/64x64/ns1")),
    # WGRAD split, gk = N*P*Q = 1083 odd: nk = 34 -> min(ceil(2048 / 9), ceil(34 / 32)) = 2 splits of 544:
    # 544 + 539 (gm = 64, gn = 576 -> 1 x 9 tiles of 64x64).  FWD / DGRAD gm = 1083 -> 17 tiles, gk = 576, nk = 18
    # -> min(16, 4) = 4 splits of 160: 160 * 3 + 96
    "w_split": _case((3, 19, 19, 64, 64, 3, 1, 1),
                     dict(fwd="f32_big/64x64/ns4", dgrad="f32_big/64x64/ns4", wgrad="f32_big/64x64/ns2",
                          wgrad_fold="f32_big/64x64/ns2/apply")),
    # ... and the small kernel's WGRAD split (f32_big = 0)
    "w_split_small": _case((3, 19, 19, 64, 64, 3, 1, 1), dict(wgrad="f32_small/64x64/ns2"), {"f32_big": 0}),
    # gk % 32 == 16: C = K = 16, 3x3, gk = 144, nk = 5 -> nk // 4 = 1 -> ns1 (FWD / DGRAD gm = 72: a second
    # tile of 8 rows); the FWD fold on a 3x3 with padding (the ring must stay zero, not relu(shift))
    "k144": _case((2, 6, 6, 16, 16, 3, 1, 1),
                  dict(fwd="f32_big/64x64/ns1", fwd_fold="f32_big/64x64/ns1/fold", dgrad="f32_big/64x64/ns1",
                       wgrad="f32_big/64x64/ns1", wgrad_fold="f32_big/64x64/ns1/apply")),
    # ... with f32_fold = 0: the folded activation is materialised through bn_apply
    "k144_nofold": _case((2, 6, 6, 16, 16, 3, 1, 1), dict(fwd_fold="f32_big/64x64/ns1/apply"), {"f32_fold": 0}),
    # ... and through f32_big = 0: the small kernel, ns1, in all three modes
    "k144_small": _case((2, 6, 6, 16, 16, 3, 1, 1),
                        dict(fwd="f32_small/64x64/ns1", dgrad="f32_small/64x64/ns1", wgrad="f32_small/64x64/ns1"),
                        {"f32_big": 0}),
    # FWD's natural fallback: C = 20 (% 16 != 0), gk = 180 (% 16 = 4), nk = 6 -> ns1.  DGRAD K = 24 -> small,
    # gk = 216 (% 16 = 8), nk = 7 -> ns1.  WGRAD gm = 24, gn = 180, gk = 72
    "c20": _case((2, 6, 6, 20, 24, 3, 1, 1),
                 dict(fwd="f32_small/64x64/ns1", dgrad="f32_small/64x64/ns1", wgrad="f32_big/64x64/ns1")),
    # the stem, 7x7 stride 2 pad 3 with C = 8: FWD small (C % 16), gm = 50, gk = 392, nk = 13 -> 3 splits of
    # 160: 160 + 160 + 72; its fold goes through bn_apply.  DGRAD K = 64 big, gm = 162 (3 tiles), gn = 8, gk =
    # 3136, nk = 98 -> min(86, 24) = 24 -> ksplit = 160 -> 20 splits (the last 96).  WGRAD gm = 64, gn = 392, gk = 50
    "stem7": _case((2, 9, 9, 8, 64, 7, 2, 3),
                   dict(fwd="f32_small/64x64/ns3", fwd_fold="f32_small/64x64/ns3/apply", dgrad="f32_big/64x64/ns20",
                        wgrad="f32_big/64x64/ns1")),
    # the space-to-depth stem, C = 16 4x4 stride 1: two taps per 32-deep K-step.  FWD gm = 162 (3 tiles),
    # gk = 256, nk = 8 -> min(86, 2) = 2 splits of 128.  DGRAD gm = 128, gn = 16, gk = 1024, nk = 32 -> min(128, 8)
    # = 8 splits of 128.  WGRAD gm = 64, gn = 256, gk = 162
    "stem16": _case((2, 8, 8, 16, 64, 4, 1, 2),
                    dict(fwd="f32_big/64x64/ns2", fwd_fold="f32_big/64x64/ns2/fold", dgrad="f32_big/64x64/ns8",
                         wgrad="f32_big/64x64/ns1")),
    # 3x3 stride 2 pad 1 on odd H, W = 15: FWD gm = 128, gk = 288, nk = 9 -> 2 splits of 160: 160 + 128 (the
    # stride-2 fold).  DGRAD gm = 450 (8 tiles), gn = 32, nk = 9 -> min(32, 2) = 2.  WGRAD gm = 32, gn = 288, gk = 128
    "s2_odd": _case((2, 15, 15, 32, 32, 3, 2, 1),
                    dict(fwd="f32_big/64x64/ns2", fwd_fold="f32_big/64x64/ns2/fold", dgrad="f32_big/64x64/ns2",
                         wgrad="f32_big/64x64/ns1")),
    # 1x1 stride-2 downsample: dx is exactly 0 at odd pixels and dx + resid is resid bitwise there.  FWD gm =
    # 80, gk = 64, nk = 2 -> ns1; DGRAD gm = 320, gn = 64, gk = 64; WGRAD gm = gn = 64, gk = 80
    "down": _case((5, 8, 8, 64, 64, 1, 2, 0),
                  dict(fwd="f32_big/64x64/ns1", dgrad="f32_big/64x64/ns1", wgrad="f32_big/64x64/ns1")),
    # the smallest channel counts the path accepts, C = K = 4: FWD / DGRAD small (gn = 4, gk = 36, nk = 2);
    # WGRAD big, gm = 4, gn = 36, gk = 50
    "c4": _case((2, 5, 5, 4, 4, 3, 1, 1),
                dict(fwd="f32_small/64x64/ns1", dgrad="f32_small/64x64/ns1", wgrad="f32_big/64x64/ns1")),
    # the wave-quantisation split (QSPLIT: f32_blocks = 3): FWD / DGRAD gm = 98, gn = 128 shrink to 64x64 (1, 2
    # < 3 tiles) -> 4 tiles >= 3, nk = 36; efficiency 4/6 at s = 1, 8/9 at 2, 12/12 at 3 -> 3 splits of 384.  The
    # WGRAD plan has no such rule (gk = 98 -> ns1)
    "qsplit": _case((2, 7, 7, 128, 128, 3, 1, 1),
                    dict(fwd="f32_big/64x64/ns3", dgrad="f32_big/64x64/ns3", wgrad="f32_big/64x64/ns1"), QSPLIT),
}

# the largest case, by the elements of x, w and y together
MAX_ELEMENTS = 2 * 14 * 14 * 128 + 128 * 9 * 128 + 2 * 7 * 7 * 128


def elements(shape):
    N, H, W, C, K, R, s, p = shape
    P, Q = T.conv_shapes(shape)
    return N * H * W * C + K * R * R * C + N * P * Q * K


def gemm_dims(shape, mode):
    """(gm, gn, gk) of the GEMM a conv call runs: mode 0 FWD, 1 DGRAD, 2 WGRAD."""
    N, H, W, C, K, R, s, p = shape
    P, Q = T.conv_shapes(shape)
    return [(N * P * Q, K, R * R * C), (N * H * W, C, R * R * K), (K, R * R * C, N * P * Q)][mode]


def parse_tag(tag):
    """(kernel, BM, BN, ns, fold) of a conv_f32_plan tag; fold in {None, "fold", "apply"}."""
    f = tag.split("/")
    bm, bn = (int(v) for v in f[1].split("x"))
    return f[0], bm, bn, int(f[2][2:]), (f[3] if len(f) > 3 else None)


def last_split_short(gk, ns):
    """True if the last of a tag's ``ns`` splits is certainly shorter than the others.  ksplit is a
    multiple of 32 with ceil(gk / ksplit) == ns; gk == ns * ksplit would make gk a multiple of 32 * ns."""
    return ns > 1 and gk % (32 * ns) != 0


def stat_rows_per(tag):
    """Rows of y one row of the statistics partials covers under a tag: BM, or 16 after a split."""
    _, bm, _, ns, _ = parse_tag(tag)
    return 16 if ns > 1 else bm


def reduce_rows_per(M):
    """Rows one partial row of the fp32 channel reductions covers (csrc/f32.hip launch_reduce: bn_partials,
    bn_bwd_reduce, the masked reduction of conv_dgrad_bnr / maxpool_bwd_bnr, colsum)."""
    t = max(1, min(1024, (M + 255) // 256))
    return (M + t - 1) // t


# ==============================================================================  inputs and truths
def _gen(name, salt=0):
    return T._gen(salt + sum(ord(c) * (i + 1) for i, c in enumerate(name)))


def _grid(shape, gen, lo, hi, step):
    return torch.randint(lo, hi + 1, shape, generator=gen).float() * step


@functools.lru_cache(maxsize=None)
def conv_inputs(shape):
    """The tensors of one conv shape (CPU, fp32, fixed seed; cases that share a shape share them)."""
    N, H, W, C, K, R, s, p = shape
    P, Q = T.conv_shapes(shape)
    gen = _gen(repr(shape))
    rn = lambda *sh, scale=1.0: torch.randn(*sh, generator=gen) * scale  # noqa: E731
    d = dict(x=rn(N, H, W, C), w=rn(K, R, R, C, scale=(2.0 / (R * R * C)) ** 0.5), dy=rn(N, P, Q, K),
             wd=rn(K, R, R, C, scale=(2.0 / (R * R * K)) ** 0.5), dres=rn(N, H, W, C), dw0=rn(K, R, R, C))
    # grids (module docstring): exact in fp32 in any summation order
    d["xq"], d["wq"] = _grid((N, H, W, C), gen, -4, 4, 0.5), _grid((K, R, R, C), gen, -4, 4, 0.25)
    d["residq"] = _grid((N, P, Q, K), gen, -32, 32, 0.125)
    d["biasq"] = (2 * torch.randint(-16, 16, (K,), generator=gen) + 1).float() / 16
    d["dyq"], d["dresq"] = _grid((N, P, Q, K), gen, -4, 4, 0.5), _grid((N, H, W, C), gen, -32, 32, 0.125)
    d["dw0q"] = _grid((K, R, R, C), gen, -32, 32, 0.125)
    # the input fold: z on 1/8, scale in {+-1, +-2}, shift an odd multiple of 1/16 -> |scale*z + shift| >= 1/16
    d["zq"] = _grid((N, H, W, C), gen, -32, 32, 0.125)
    d["fsc"] = torch.tensor([1.0, -1.0, 2.0, -2.0])[torch.randint(0, 4, (C,), generator=gen)]
    d["fsh"] = (2 * torch.randint(-8, 8, (C,), generator=gen) + 1).float() / 16
    # the random fold: scale / shift such that about half of relu(scale*z + shift) is on
    d["z"], d["asc"], d["ash"] = rn(N, H, W, C), torch.rand(C, generator=gen) + 0.5, rn(C, scale=0.5)
    # conv_dgrad_bnr: the BatchNorm input on 1/8 with the recomputed mask's scale / shift as above, a second
    # BatchNorm's input, the saved statistics, a mask tensor
    d["bx"], d["bx2"] = _grid((N, H, W, C), gen, -32, 32, 0.125), rn(N, H, W, C)
    d["mean"], d["invstd"] = rn(C, scale=0.1), torch.rand(C, generator=gen) + 0.5
    d["mean2"], d["invstd2"] = rn(C, scale=0.1), torch.rand(C, generator=gen) + 0.5
    d["msc"] = torch.tensor([1.0, -1.0, 2.0, -2.0])[torch.randint(0, 4, (C,), generator=gen)]
    d["msh"] = (2 * torch.randint(-8, 8, (C,), generator=gen) + 1).float() / 16
    d["ymask"] = torch.relu(rn(N, H, W, C))
    assert all(v.dtype == F32 for v in d.values())
    return d


@functools.lru_cache(maxsize=None)
def conv_truth(shape, what):
    """fp64 truths of a conv shape.  Exact (grid) cases: "y_epi", "y_fold_q", "dx_q", "dw_q"; random cases:
    "y", "y_fold", "dx", "dw"."""
    N, H, W, C, K, R, s, p = shape
    d = conv_inputs(shape)
    if what == "y_epi":
        return T.conv(d["xq"], d["wq"], s, p, d["biasq"], d["residq"], True)["y"]
    if what == "y_fold_q":
        return T.conv(d["zq"], d["wq"], s, p, in_scale=d["fsc"], in_shift=d["fsh"])["y"]
    if what == "dx_q":
        return T.conv(d["xq"], d["wq"], s, p, dy=d["dyq"])["dx"]
    if what == "dw_q":
        return T.conv(d["xq"], d["wq"], s, p, dy=d["dyq"])["dw"]
    if what == "dw_fold_q":
        return T.conv(d["zq"], d["wq"], s, p, dy=d["dyq"], in_scale=d["fsc"], in_shift=d["fsh"])["dw"]
    if what == "y":
        return T.conv(d["x"], d["w"], s, p)["y"]
    if what == "y_fold":
        return T.conv(d["z"], d["w"], s, p, in_scale=d["asc"], in_shift=d["ash"])["y"]
    if what == "dx":
        return T.conv(d["x"], d["wd"], s, p, dy=d["dy"])["dx"]
    if what == "dw":
        return T.conv(d["x"], d["w"], s, p, dy=d["dy"])["dw"]
    if what == "dw_fold":
        return T.conv(d["z"], d["w"], s, p, dy=d["dy"], in_scale=d["asc"], in_shift=d["ash"])["dw"]
    raise KeyError(what)


def exact_units(shape):
    """{output: the largest sum of |terms| of one element of an exact case, in units of the finest grid step
    among its terms}.  Below 2^24 every partial sum, in any order and under any split, is an integer number
    of units that fp32 holds exactly."""
    N, H, W, C, K, R, s, p = shape
    d = conv_inputs(shape)
    ab = lambda t: t.abs()  # noqa: E731
    fz = T.fold_act(d["zq"], d["fsc"], d["fsh"])
    out = {
        # products on 1/8, residual on 1/8, bias on 1/16
        "y_epi": T.conv(ab(d["xq"]), ab(d["wq"]), s, p, ab(d["biasq"]), ab(d["residq"]))["pre"].max() * 16,
        # relu(scale*z + shift) on 1/16 times w on 1/4
        "y_fold": T.conv(fz, ab(d["wq"]), s, p)["pre"].max() * 64,
        # dy on 1/2 times w on 1/4, residual on 1/8
        "dx": (T.conv(ab(d["xq"]), ab(d["wq"]), s, p, dy=ab(d["dyq"]))["dx"] + ab(d["dresq"]).double()).max() * 8,
        # dy on 1/2 times x on 1/2, dw0 on 1/8
        "dw": (T.conv(ab(d["xq"]), ab(d["wq"]), s, p, dy=ab(d["dyq"]))["dw"] + ab(d["dw0q"]).double()).max() * 8,
        "dw_fold": (T.conv(fz, ab(d["wq"]), s, p, dy=ab(d["dyq"]))["dw"] + ab(d["dw0q"]).double()).max() * 32,
    }
    return {k: float(v) for k, v in out.items()}


# conv_dgrad_bnr in fp32 (f32::conv_dgrad, then the masked channel reduction): the forms of
# truth_image.BNR_FORMS the fp32 path has, at a 3x3 stride-1, a 3x3 stride-2 and a 1x1 shape
BNR_F32_CASES = ["split", "s2_odd", "down"]
BNR_F32_FORMS = ["recompute", "tensor", "bits", "resid_bits", "dual_resid", "dual_bits"]


# ------------------------------------------------------------------------------ element-wise ops
# dropout / relu_bwd sizes: one element, a multiple of 4, not a multiple of 4, a second block, a second
# trip of the grid-stride loop (grid_n caps at 8192 blocks of 256 threads)
EW_SIZES = [1, 1024, 1027, 256 * 8192 + 5]
COLSUM_SHAPES = [(M, C) for M in (1, 17, 300) for C in (4, 520)]
DROP_P, DROP_SEED, DROP_OFF = 0.1, 1234, 3 << 32
# C = 6: the generic maxpool_fwd_kernel (C % 4 != 0)
POOL_C6 = (2, 9, 11, 6)


@functools.lru_cache(maxsize=None)
def ew_case(n):
    """x without zeros (so that the kept elements of a dropout are exactly its non-zero outputs), y with
    about half of its elements off."""
    gen = T._gen(n)
    x = torch.randn(n, generator=gen)
    x = torch.where(x == 0, torch.ones_like(x), x)
    return dict(x=x, dy=torch.randn(n, generator=gen), y=torch.relu(torch.randn(n, generator=gen)))


@functools.lru_cache(maxsize=None)
def colsum_case(M, C):
    gen = T._gen(1000 * M + C)
    return dict(x=torch.randn(M, C, generator=gen) + 0.25, out0=torch.randn(C, generator=gen))
