// Host side of the implicit-GEMM kernels (igemm_kernels.h): one launcher per kernel family, the
// eligibility predicates with the measurements behind them, choose_kernel(), which makes the kernel
// and tile choice of a GEMM once as a KernelChoice value, and what reads that value: dispatch<> (the
// launch), choice_tag() (its name) and the callers' partial-statistics sizing (its bm).  The
// plain-GEMM planner on top of these is igemm_plan.h.
#pragma once
#include "igemm_kernels.h"

namespace pcmp {

// epilogue kind of a launch
template <int MODE>
static int epi_of(const IgemmParams& p) {
  if (MODE == MODE_FWD && p.stats) return EPI_STATS;
  if (MODE == MODE_DGRAD && p.bn_x) return p.bn_x2 ? EPI_BNR2 : EPI_BNR;
  return MODE != MODE_WGRAD && p.relu >= 2 ? EPI_GELU : EPI_PLAIN;
}

// epilogue column-sum scratch of the BN-statistics / BN-backward-reduce epilogues (0 for the others):
// NW waves x [16][NS*WTN+4] + [WM][NS][BN] floats
template <int MODE, int BN, int WM, int WN, int NW = 4>
static size_t epi_scratch_bytes(const IgemmParams& p) {
  if (!((MODE == MODE_FWD && p.stats) || (MODE == MODE_DGRAD && p.bn_x))) return 0;
  const int NS = MODE == MODE_DGRAD && p.bn_x2 ? 3 : 2;
  return (size_t)(NW * 16 * (NS * (BN / WN) + 4) + WM * NS * BN) * sizeof(float);
}

// igemm_kernel with epilogue E at epilogue depth D, on the block-uniform tap walk where the shape has
// it; the fold form (FOLD != 0) is compiled for that walk only
template <int MODE, int BM, int BN, int WM, int WN, int FOLD, int E, int D = 2>
static void launch_igemm(bool unif, int grid, size_t smem, hipStream_t st, const IgemmParams& p) {
  if constexpr (FOLD != 0) {
    launch_lds<igemm_kernel<MODE, BM, BN, WM, WN, true, E, D, NT, FOLD>>(dim3(grid), dim3(NT), smem, st, p);
  } else {
    if (unif) launch_lds<igemm_kernel<MODE, BM, BN, WM, WN, true, E, D>>(dim3(grid), dim3(NT), smem, st, p);
    else launch_lds<igemm_kernel<MODE, BM, BN, WM, WN, false, E, D>>(dim3(grid), dim3(NT), smem, st, p);
  }
}

// Register-staged igemm_kernel.  FOLD != 0 are the BatchNorm fold launches (IgemmParams::fold_x /
// act_sc): register-staged kernel only -- the LDS-DMA kernels move operands straight into LDS with no
// register pass in which the operand could be formed -- and without the GELU and plain DGRAD epilogues.
template <int MODE, int BM, int BN, int WM, int WN, int FOLD = 0>
static void launch_cfg(IgemmParams& p, hipStream_t st) {
  p.tiles_m = ceil_div(p.gm, BM);
  p.tiles_n = ceil_div(p.gn, BN);
  TORCH_CHECK(MODE == MODE_WGRAD || !p.stats || p.tiles_m <= p.stats_cap,
              FOLD ? "igemm fold: partial-stats buffer too small" : "igemm: partial-stats buffer too small");
  const int grid = p.tiles_m * p.tiles_n * p.nsplit;
  const int nk = ceil_div(std::min(p.ksplit, p.gk), BK);
  size_t smem = std::max((size_t)(nk > 1 ? 2 : 1) * (BM + BN) * BK * 2, epi_scratch_bytes<MODE, BN, WM, WN>(p));
  if (FOLD != 0 && MODE != MODE_WGRAD) {   // the coefficient copy sits after every buffer the kernel uses
    p.fold_lds = (int)((smem + 15) / 16 * 16);
    smem = (size_t)p.fold_lds + (MODE == MODE_FWD ? (size_t)2 * p.C : (size_t)3 * p.K) * sizeof(float);
  }
  const int cin = MODE == MODE_FWD ? p.C : p.K;
  const bool unif = MODE != MODE_WGRAD && cin % BK == 0 && p.ksplit % BK == 0;
  const int epi = epi_of<MODE>(p);
  if constexpr (MODE == MODE_WGRAD) {
    if constexpr ((BM / WM) % 32 == 0 && (BN / WN) % 32 == 0) {
      if (kn_wgrad_m32.get()) {
        launch_lds<igemm_kernel<MODE, BM, BN, WM, WN, false, EPI_PLAIN, 2, NT, FOLD, true>>(dim3(grid), dim3(NT), smem, st, p);
        return;
      }
    }
    launch_lds<igemm_kernel<MODE, BM, BN, WM, WN, false, EPI_PLAIN, 2, NT, FOLD>>(dim3(grid), dim3(NT), smem, st, p);
  } else if constexpr (MODE == MODE_FWD) {
    if (epi == EPI_STATS) return launch_igemm<MODE, BM, BN, WM, WN, FOLD, EPI_STATS>(unif, grid, smem, st, p);
    if constexpr (FOLD == 0) {
      if (epi == EPI_GELU) return launch_igemm<MODE, BM, BN, WM, WN, FOLD, EPI_GELU>(unif, grid, smem, st, p);
    }
    launch_igemm<MODE, BM, BN, WM, WN, FOLD, EPI_PLAIN>(unif, grid, smem, st, p);
  } else {
    if constexpr (FOLD != 0) {
      TORCH_CHECK(p.bn_x, "igemm fold: DGRAD only with the fused BN-backward-reduce epilogue");
    }
    if (epi == EPI_BNR) {
      if (kn_epi_depth.get() >= 4) launch_igemm<MODE, BM, BN, WM, WN, FOLD, EPI_BNR, 4>(unif, grid, smem, st, p);
      else launch_igemm<MODE, BM, BN, WM, WN, FOLD, EPI_BNR>(unif, grid, smem, st, p);
    } else if (epi == EPI_BNR2) {
      if (kn_epi_depth_bnr2.get() >= 4) launch_igemm<MODE, BM, BN, WM, WN, FOLD, EPI_BNR2, 4>(unif, grid, smem, st, p);
      else launch_igemm<MODE, BM, BN, WM, WN, FOLD, EPI_BNR2>(unif, grid, smem, st, p);
    } else if constexpr (FOLD == 0) {
      if (epi == EPI_GELU) launch_igemm<MODE, BM, BN, WM, WN, FOLD, EPI_GELU>(unif, grid, smem, st, p);
      else launch_igemm<MODE, BM, BN, WM, WN, FOLD, EPI_PLAIN>(unif, grid, smem, st, p);
    }
  }
}

// A/B knobs (torch.ops.pcmp.set_knob; tools/gemm_knob_ab.py)

inline Knob kn_wgrad_wgs("wgrad_wgs", 0);   // > 0: fixed split-K workgroup target (side-stream WGRADs)
inline Knob kn_igemm8("igemm8", 1);
static int igemm8_mode() { return kn_igemm8.get(); }

// minimum 256x256 tile count for the 8-wave kernel (knob igemm8_min_tiles, A/B runs)
inline Knob kn_igemm8_min_tiles("igemm8_min_tiles", 160);
static int igemm8_min_tiles() { return kn_igemm8_min_tiles.get(); }

// igemm_dma_kernel with epilogue E; the BN-backward-reduce epilogues of the 4-wave kernel run at the
// epilogue depth of their knob.  (A plain `if`: every epilogue keeps its depth-4 instantiation.)
template <int MODE, int BM, int BN, int WM, int WN, int NTHR, int MINB, int E>
static void launch_dma_epi(int grid, size_t smem, hipStream_t st, const IgemmParams& p) {
  constexpr bool can_deep = (E == EPI_BNR || E == EPI_BNR2) && NTHR == 256;
  if (can_deep && (E == EPI_BNR2 ? kn_epi_depth_bnr2 : kn_epi_depth).get() >= 4)
    launch_lds<igemm_dma_kernel<MODE, BM, BN, WM, WN, NTHR, MINB, E, 4>>(dim3(grid), dim3(NTHR), smem, st, p);
  else
    launch_lds<igemm_dma_kernel<MODE, BM, BN, WM, WN, NTHR, MINB, E, 2>>(dim3(grid), dim3(NTHR), smem, st, p);
}

template <int MODE, int BM, int BN, int WM, int WN, int NTHR, int MINB>
static void launch_dma(IgemmParams& p, hipStream_t st) {
  p.tiles_m = ceil_div(p.gm, BM);
  p.tiles_n = ceil_div(p.gn, BN);
  TORCH_CHECK(!p.stats || p.tiles_m <= p.stats_cap, "igemm_dma: partial-stats buffer too small");
  TORCH_CHECK(p.gk % BK == 0 && (MODE == MODE_FWD ? p.C : p.K) % BK == 0 && p.ksplit % BK == 0,
              "igemm_dma: needs the block-uniform tap walk");
  TORCH_CHECK(p.nsplit == 1 || (!p.stats && !p.bn_x), "igemm_dma: split-K only with the plain epilogue");
  const int grid = p.tiles_m * p.tiles_n * p.nsplit;
  const size_t smem = std::max((size_t)2 * (BM + BN) * BK * 2, epi_scratch_bytes<MODE, BN, WM, WN, NTHR / 64>(p));
  const int epi = epi_of<MODE>(p);
  if constexpr (MODE == MODE_FWD) {
    if (epi == EPI_STATS) launch_dma_epi<MODE, BM, BN, WM, WN, NTHR, MINB, EPI_STATS>(grid, smem, st, p);
    else if (epi == EPI_GELU) launch_dma_epi<MODE, BM, BN, WM, WN, NTHR, MINB, EPI_GELU>(grid, smem, st, p);
    else launch_dma_epi<MODE, BM, BN, WM, WN, NTHR, MINB, EPI_PLAIN>(grid, smem, st, p);
  } else {
    if (epi == EPI_BNR) launch_dma_epi<MODE, BM, BN, WM, WN, NTHR, MINB, EPI_BNR>(grid, smem, st, p);
    else if (epi == EPI_BNR2) {
      if constexpr (NTHR == 256) launch_dma_epi<MODE, BM, BN, WM, WN, NTHR, MINB, EPI_BNR2>(grid, smem, st, p);
      else TORCH_CHECK(false, "igemm8: dual BN-reduce epilogue not instantiated");
    } else if (epi == EPI_GELU) launch_dma_epi<MODE, BM, BN, WM, WN, NTHR, MINB, EPI_GELU>(grid, smem, st, p);
    else launch_dma_epi<MODE, BM, BN, WM, WN, NTHR, MINB, EPI_PLAIN>(grid, smem, st, p);
  }
}

// igemm_dma32_kernel in place of igemm_dma_kernel for the 4-wave 128x128 / 128x64 FWD and DGRAD
// GEMMs (use_dma4 cases 1 and 2) with at least dma32_mink K-tiles; not for the GELU epilogues (the
// planner's Linear GEMMs keep their own kernels).  Per-shape A/B on the ResNet-50 B=256 conv shapes
// with their training epilogues (profiles/r5_knob_dma32.txt): every FWD + BN-statistics GEMM gains or
// ties (l2 3x3 85.5 -> 72.4 us, l3 1x1 256->1024 60.4 -> 47.3, l4 3x3 73.3 -> 65.3, l4 1x1 2048->512
// 37.4 -> 32.8), so do the 3x3 DGRAD + BN-reduce GEMMs (l1 157.7 -> 151.0, l2 107.2 -> 102.8, l4 85.5
// -> 81.0); the short-K 1x1 DGRADs into wide outputs lose 4-30 % (l3 1x1 1024->256 125.6 -> 139.8, its
// dual-BN form 153 -> 200) and stay on igemm_dma_kernel: DGRAD takes the new kernel for filters wider
// than 1x1 or >= dma32_dgrad_mink K-tiles.  Knob dma32 = 0 restores igemm_dma_kernel (A/B).
inline Knob kn_dma32("dma32", 1);
inline Knob kn_dma32_modes("dma32_modes", 1);   // bit 0: FWD, bit 1: DGRAD (whole-step A/B: FWD only, profiles/r5_bench_ab_dma32_modes.txt)
inline Knob kn_dma32_mink("dma32_mink", 3);
inline Knob kn_dma32_dgrad_mink("dma32_dgrad_mink", 16);
static bool use_dma32(int mode, const IgemmParams& p) {
  if (!kn_dma32.get() || mode == MODE_WGRAD || p.nsplit != 1 || p.relu >= 2 || p.gn % 8 != 0 ||
      p.gk / BK < kn_dma32_mink.get())
    return false;
  if (!(kn_dma32_modes.get() & (mode == MODE_FWD ? 1 : 2))) return false;
  return mode == MODE_FWD || p.R * p.S > 1 || p.gk / BK >= kn_dma32_dgrad_mink.get();
}

template <int MODE, int BM, int BN, int WM, int WN>
static void launch_dma32(IgemmParams& p, hipStream_t st) {
  p.tiles_m = ceil_div(p.gm, BM);
  p.tiles_n = ceil_div(p.gn, BN);
  TORCH_CHECK(!p.stats || p.tiles_m <= p.stats_cap, "igemm_dma32: partial-stats buffer too small");
  TORCH_CHECK(p.gk % BK == 0 && (MODE == MODE_FWD ? p.C : p.K) % BK == 0 && p.ksplit >= p.gk && p.nsplit == 1,
              "igemm_dma32: needs the block-uniform tap walk and no split-K");
  TORCH_CHECK(p.relu < 2 && p.gn % 8 == 0, "igemm_dma32: conv epilogues with 8-channel groups only");
  TORCH_CHECK(p.gk / BK >= 2, "igemm_dma32: at least two K-tiles");
  const dim3 grid(p.tiles_m * p.tiles_n), block(256);
  constexpr size_t smem = (size_t)2 * (BM + BN) * BK * 2 + (size_t)(6 * BN + WM * 3 * BN) * sizeof(float);
  static_assert(2 * smem <= 160 * 1024, "igemm_dma32: two blocks per CU");
  const int epi = epi_of<MODE>(p);
  if constexpr (MODE == MODE_FWD) {
    if (epi == EPI_STATS) launch_lds<igemm_dma32_kernel<MODE, BM, BN, WM, WN, EPI_STATS, 2>>(grid, block, smem, st, p);
    else launch_lds<igemm_dma32_kernel<MODE, BM, BN, WM, WN, EPI_PLAIN, 2>>(grid, block, smem, st, p);
  } else {
    if (epi == EPI_BNR) {
      if (kn_epi_depth.get() >= 4) launch_lds<igemm_dma32_kernel<MODE, BM, BN, WM, WN, EPI_BNR, 4>>(grid, block, smem, st, p);
      else launch_lds<igemm_dma32_kernel<MODE, BM, BN, WM, WN, EPI_BNR, 2>>(grid, block, smem, st, p);
    } else if (epi == EPI_BNR2) {
      if (kn_epi_depth_bnr2.get() >= 4) launch_lds<igemm_dma32_kernel<MODE, BM, BN, WM, WN, EPI_BNR2, 4>>(grid, block, smem, st, p);
      else launch_lds<igemm_dma32_kernel<MODE, BM, BN, WM, WN, EPI_BNR2, 2>>(grid, block, smem, st, p);
    } else {
      launch_lds<igemm_dma32_kernel<MODE, BM, BN, WM, WN, EPI_PLAIN, 2>>(grid, block, smem, st, p);
    }
  }
}

// 4-wave LDS-DMA kernel (2 blocks per CU) in place of the register-staged 4-wave kernel for the
// FWD/DGRAD GEMMs with the block-uniform tap walk and >= 3 K-tiles (measured
// profiles/r1_dma4_ab.txt: 3x3 layers 10-16 % faster, e.g. layer4 3x3 DGRAD 97 -> 84 us; GEMMs
// of 2 K-tiles ran up to 9 % slower).  Knob dma4 = 0 disables it (A/B runs); knob dma4_n64 picks
// the narrow-output (gn <= 64) tile: 1 = 128x64 (2x2 waves of 64x32, the default: 6 % faster than
// 256x64 on the layer1 3x3), 2 = 256x64 (4x1 waves of 64x64), 0 = register-staged kernel.
inline Knob kn_dma4("dma4", 1);
inline Knob kn_dma4_n64("dma4_n64", 1);
static int dma4_mode() { return kn_dma4.get(); }
static int dma4_n64() { return kn_dma4_n64.get(); }
// 0: register-staged kernel; 1: 128x128; 2: 128x64; 3: 256x64
// FWD grids with fewer 128x128 tiles than CUs (the B=64 transfer-learning step's layer-3/4 convs:
// 100-196 tiles) take 128x64 tiles: twice the workgroups (dma4_small_n64 = 0: 128x128)
inline Knob kn_dma4_small_n64("dma4_small_n64", 1);   // TL step 2.43 -> 2.38 ms (profiles/r6_tl_small_n64_ab.txt)
static int use_dma4(int mode, const IgemmParams& p) {
  if (!dma4_mode() || mode == MODE_WGRAD || p.nsplit != 1) return 0;
  const int cin = mode == MODE_FWD ? p.C : p.K;
  if (cin % BK != 0 || p.gk % BK != 0 || p.gk / BK < 3 || p.gm <= 64) return 0;
  if (p.gn <= 64) {
    const int v = dma4_n64();
    return v == 1 ? 2 : (v == 2 ? 3 : 0);
  }
  if (mode == MODE_FWD && kn_dma4_small_n64.get() && ceil_div(p.gm, 128) * ceil_div(p.gn, 128) < 256) return 2;
  return 1;
}

// halo-tiled direct conv for the layer-1 3x3 / stem shapes: bit 0 FWD, bit 1 every DGRAD variant,
// bit 2 the overlapped BN-backward DGRAD.  DGRAD is off by default: its BN-backward epilogue loads
// stall the one wave per SIMD (profiles/r2_halo_conv.txt)
inline Knob kn_halo("halo", 1);
inline Knob kn_halo_ovl("halo_ovl", 1);   // output stores overlapped with the next tile's MFMAs

static bool halo_dgrad_ovl(const IgemmParams& p) {
  return kn_halo_ovl.get() && p.bn_x && !p.bn_x2 && !p.resid && !p.relu && !p.bn_mask && !p.bn_mbits && p.bn_msc &&
         p.bn_msh;
}

// Eligibility + geometry of halo_conv_kernel: stride 1, square filter, 64 output channels and
// (C, R) = (64, 3) [layer-1 3x3, FWD and DGRAD] or (16, 4) [space-to-depth stem, FWD]; the output
// width divides 224 (a tile = whole rows) and the grid has at least one tile per CU.
static bool halo_geom(int mode, const IgemmParams& p, HaloGeom& g) {
  const int hk = kn_halo.get();
  if ((mode == MODE_FWD && !(hk & 1)) || (mode == MODE_DGRAD && !(hk & 6)) || mode == MODE_WGRAD || p.nsplit != 1 || p.stride != 1 || p.R != p.S || p.gn != 64 ||
      p.sub || p.relu >= 2)
    return false;
  int CS, pad;
  if (mode == MODE_FWD) {
    CS = p.C; g.Hs = p.H; g.Ws = p.W; g.Ho = p.P; g.Wo = p.Q; pad = p.pad;
    if (p.bias) return false;
  } else {
    CS = p.K; g.Hs = p.P; g.Ws = p.Q; g.Ho = p.H; g.Wo = p.W; pad = p.R - 1 - p.pad;
    if (p.bn_x2 || pad < 0) return false;
    // bit 1 enables every DGRAD variant, bit 2 only the overlapped BN-backward form (mask
    // recomputed from x, no residual)
    if (!(hk & 2) && !((hk & 4) && halo_dgrad_ovl(p))) return false;
  }
  // compiled geometries: layer-1 3x3 at 56 wide, the space-to-depth stem at 112 wide
  if (!((CS == 64 && p.R == 3 && g.Wo == 56) || (CS == 16 && p.R == 4 && g.Wo == 112 && mode == MODE_FWD)))
    return false;
  g.TR = HALO_BM / g.Wo;
  if (g.Ho % g.TR != 0 || g.Ho != g.Hs + 2 * pad - p.R + 1 || g.Wo != g.Ws + 2 * pad - p.S + 1) return false;
  g.tiles_img = g.Ho / g.TR;
  g.tiles = p.N * g.tiles_img;
  if (g.tiles < 256 || (int64_t)g.tiles * HALO_BM != (int64_t)p.gm) return false;
  g.padT = pad; g.padL = pad;
  g.HWd = g.Wo + p.S - 1;
  g.HWp = (g.HWd + 15 + 15) / 16 * 16;    // room for the 0..15-slot row skew, multiple of 16
  g.HR = g.TR + p.R - 1;
  g.ninstr = ceil_div(g.HR * (CS / 8) * g.HWp * 16, 1024);
  g.lds_bytes = g.ninstr * 1024;
  if (2 * g.lds_bytes + HALO_BM * 64 * 2 + 768 * (int)sizeof(float) > 160 * 1024) return false;
  g.src = p.a; g.src_bytes = p.a_bytes; g.wsrc = p.b;
  g.fd_HWp = make_fastdiv(g.HWp);
  g.fd_Wo = make_fastdiv(g.Wo);
  g.fd_timg = make_fastdiv(g.tiles_img);
  return true;
}
static bool use_halo(int mode, const IgemmParams& p) {
  HaloGeom g;
  return halo_geom(mode, p, g);
}

// halo_conv_kernel<MODE, E, CS, RS, FLIP, WO, OVL> for one compiled FWD geometry
template <int CS, int RS, int WO>
static void launch_halo_fwd(bool ovl, dim3 grid, size_t smem, hipStream_t st, const IgemmParams& p, const HaloGeom& g) {
  const dim3 block(NT);
  if (ovl) {
    if (p.stats) launch_lds<halo_conv_kernel<MODE_FWD, EPI_STATS, CS, RS, false, WO, true>>(grid, block, smem, st, p, g);
    else launch_lds<halo_conv_kernel<MODE_FWD, EPI_PLAIN, CS, RS, false, WO, true>>(grid, block, smem, st, p, g);
  } else {
    if (p.stats) launch_lds<halo_conv_kernel<MODE_FWD, EPI_STATS, CS, RS, false, WO, false>>(grid, block, smem, st, p, g);
    else launch_lds<halo_conv_kernel<MODE_FWD, EPI_PLAIN, CS, RS, false, WO, false>>(grid, block, smem, st, p, g);
  }
}

// ovl: the choice's halo_ovl bit (output stores overlapped with the next tile's MFMAs)
template <int MODE>
static void launch_halo(IgemmParams& p, bool ovl, hipStream_t st) {
  HaloGeom g;
  TORCH_CHECK(halo_geom(MODE, p, g), "halo_conv: shape not eligible");
  p.tiles_m = g.tiles;
  p.tiles_n = 1;
  TORCH_CHECK(!p.stats || p.tiles_m <= p.stats_cap, "halo_conv: partial-stats buffer too small");
  const dim3 grid(std::min(g.tiles, 256)), block(NT);
  size_t smem = (size_t)2 * g.lds_bytes + 768 * sizeof(float);
  if constexpr (MODE == MODE_FWD) {
    if (ovl) smem += (size_t)HALO_BM * 64 * 2;
    if (p.C == 64) launch_halo_fwd<64, 3, 56>(ovl, grid, smem, st, p, g);
    else launch_halo_fwd<16, 4, 112>(ovl, grid, smem, st, p, g);
  } else if constexpr (MODE == MODE_DGRAD) {
    if (ovl) {
      smem += (size_t)HALO_BM * 64 * 2;
      launch_lds<halo_conv_kernel<MODE, EPI_BNR, 64, 3, true, 56, true>>(grid, block, smem, st, p, g);
    } else if (p.bn_x) {
      launch_lds<halo_conv_kernel<MODE, EPI_BNR, 64, 3, true, 56, false>>(grid, block, smem, st, p, g);
    } else {
      launch_lds<halo_conv_kernel<MODE, EPI_PLAIN, 64, 3, true, 56, false>>(grid, block, smem, st, p, g);
    }
  }
}

// 8-wave LDS-DMA kernel eligibility: FWD/DGRAD with the block-uniform tap walk (source channels a
// multiple of BK), no split-K, enough K-tiles for the phase pipeline, and a grid that still covers
// most CUs with BM = 256 tiles: >= 160 tiles (ResNet-50 layer3 at B=256 has 196 and runs 20-28 %
// faster than on the 4-wave kernel's 784 tiles; layer4's 98 tiles run 25-35 % slower, measured
// profiles/r1_igemm8_mintiles_ab.txt), and >= 8 K-tiles: with one block per CU a short main loop
// cannot hide the load / epilogue latency that two 4-wave blocks per CU overlap (1x1 convs over
// 256 input channels ran 6-12 % faster on the 4-wave kernel, profiles/r1_igemm8_ab_v2.txt).
// PCMP_IGEMM8=0 disables it (A/B runs).
static int use_igemm8(int mode, const IgemmParams& p) {
  if (!igemm8_mode() || mode == MODE_WGRAD || p.nsplit != 1) return 0;
  const int cin = mode == MODE_FWD ? p.C : p.K;
  if (cin % BK != 0 || p.gk % BK != 0 || p.gk / BK < 8 || p.gn < 256) return 0;
  // (measured: the BN=128 variant does not beat the 4-wave 128x128 kernel; the dual BN-reduce
  //  epilogue of a 128x64 wave tile spills)
  if (mode == MODE_DGRAD && p.bn_x2) return 0;
  if (ceil_div(p.gm, BM8) * ceil_div(p.gn, 256) < igemm8_min_tiles()) return 0;
  return 256;
}

// WGRAD tiles with 64x64 wave tiles where one GEMM side is narrow: RSC <= 64 (gn) -> 256x64 with
// the 4 waves along M; cout <= 64 (gm) -> 64x256 with the waves along N, only for the Cin=8 stem
// (measured profiles/r1_wgrad_wide_ab.txt: stem -7 %, 1x1 64->256 -5 %, but the layer1 3x3 and
// 1x1 256->64 WGRADs ran 5-16 % slower on 64x256).  Knob wg64 = 0 disables them (A/B runs).
inline Knob kn_wg64("wg64", 1);
static int wgrad_wide(const IgemmParams& p) {
  if (!kn_wg64.get()) return 0;
  if (p.gm > 32 && p.gm <= 64 && p.gn >= 256 && (p.C == 8 || p.C == 16)) return 1;   // 64 x 256 (stem)
  if (p.gn > 32 && p.gn <= 64 && p.gm >= 256) return 2;   // 256 x 64
  return 0;
}

// wgrad_dma32_kernel (wgrad32.h) in place of the register-staged WGRAD: no BatchNorm fold (those
// operands are formed in registers), a batch of whole 64-image groups, 64-multiple channel counts (a
// 64-column block is one tap / one 128-B row run).  Knob wgrad_dma32 = 0 disables it (A/B runs).
inline Knob kn_wgrad_dma32("wgrad_dma32", 1);
static bool use_wgrad_dma32(const IgemmParams& p) {
  if (!kn_wgrad_dma32.get() || p.fold_x || p.act_sc) return false;
  if (p.N % 64 || p.C % 64 || p.K % 64 || p.gk % 64) return false;
  // 32-bit offsets: per-lane parts and the block-uniform parts stay below 2^31 bytes
  return (int64_t)p.N * p.P * p.Q * p.K * 2 < (1ll << 31) && (int64_t)p.N * p.H * p.W * p.C * 2 < (1ll << 31);
}

// FWD/DGRAD grids of fewer 128x128 tiles than CUs (BERT-base's M=4096 token GEMMs with N=768:
// 192 tiles) run 64x128 tiles instead: twice the workgroups, every CU busy.  Knob bm64_smallgrid =
// 0 disables it (A/B runs).  FWD convs with BN statistics keep the LDS-DMA tiles (bm64_smallgrid = 1):
// the ResNet-50 transfer-learning step at B=64 (layer-3/4 convs: 100-196 tiles) ran 2.41 -> 2.38
// ms/step without the 64x128 register-staged form (profiles/r6_tl_bm64_ab.txt, r6_tl_bm64_ab2.txt); 2 = every GEMM.
inline Knob kn_bm64_smallgrid("bm64_smallgrid", 1);
static bool use_bm64_smallgrid(int mode, const IgemmParams& p, bool stats) {
  if (!(mode != MODE_WGRAD && p.nsplit == 1 && p.gm > 64 && p.gn > 64)) return false;
  const int k = kn_bm64_smallgrid.get();
  if (k == 0 || (k == 1 && mode == MODE_FWD && stats)) return false;
  return ceil_div(p.gm, 128) * ceil_div(p.gn, 128) < 256;
}

// ---- the kernel choice of one GEMM: made once by choose_kernel(), then read by the launch
// (dispatch<>), by the tag (choice_tag) and by the callers that size per-row-tile partial statistics
// (ceil(gm / bm) rows).
enum KernelFamily {
  KF_REG,             // igemm_kernel, register-staged ("reg"; WGRAD "wgrad" / "wgrad_m32")
  KF_REG_SMALLGRID,   // its 64x128 tile for FWD/DGRAD grids below one 128x128 tile per CU
  KF_FOLD,            // its BatchNorm fold forms ("fold"; WGRAD "fold_wgrad[_m32]")
  KF_DMA4,            // igemm_dma_kernel, 4 waves
  KF_DMA32,           // igemm_dma32_kernel
  KF_DMA8,            // igemm_dma_kernel, 8 waves, 256x256
  KF_HALO,            // halo_conv_kernel ("halo" / "halo_ovl")
  KF_WGRAD_DMA32,     // wgrad_dma32_kernel (wgrad32.h)
};
struct KernelChoice {
  int family, bm, bn;
  bool halo_ovl;   // KF_HALO: output stores overlapped with the next tile's MFMAs
  bool m32;        // WGRAD, register-staged: the 32x32x16 MFMA form
};

// wave grid WM x WN of the register-staged tiles: four waves along N for 32-row tiles and the 64x256
// stem tile, along M for 256x64, 2x2 otherwise
constexpr int reg_wm(int bm, int bn) { return bm == 32 || bn == 256 ? 1 : (bm == 256 ? 4 : 2); }
constexpr int reg_wn(int bm, int bn) { return bm == 32 || bn == 256 ? 4 : (bm == 256 ? 1 : 2); }
template <int MODE, int BM, int BN, int FOLD = 0>
static void launch_reg(IgemmParams& p, hipStream_t st) {
  launch_cfg<MODE, BM, BN, reg_wm(BM, BN), reg_wn(BM, BN), FOLD>(p, st);
}
template <int MODE, int BM, int FOLD = 0>   // BN = 64 (n64) or 128
static void launch_reg_bn(bool n64, IgemmParams& p, hipStream_t st) {
  if (n64) launch_reg<MODE, BM, 64, FOLD>(p, st); else launch_reg<MODE, BM, 128, FOLD>(p, st);
}

// default register-staged tile: BN = 64 for narrow outputs, BM = 32 / 64 for short M (linear at small batch)
static int default_bm(const IgemmParams& p) { return p.gm <= 32 ? 32 : (p.gm <= 64 ? 64 : 128); }
static int default_bn(const IgemmParams& p) { return p.gn <= 64 ? 64 : 128; }

// The one evaluation of the eligibility predicates, in order of precedence.  Depends on the geometry,
// p.nsplit, the presence of the optional operands and the knobs; `stats` says whether a FWD call
// produces BN statistics (its buffer is sized from the choice, so it need not exist yet).
static KernelChoice choose_kernel(int mode, const IgemmParams& p, bool stats) {
  // launch_cfg runs WGRAD in the 32x32x16 form where the wave tile is a multiple of 32 both ways
  auto reg = [&](int family, int bm, int bn) {
    const bool m32 = mode == MODE_WGRAD && kn_wgrad_m32.get() && (bm / reg_wm(bm, bn)) % 32 == 0 &&
                     (bn / reg_wn(bm, bn)) % 32 == 0;
    return KernelChoice{family, bm, bn, false, m32};
  };
  if (p.fold_x || p.act_sc) {
    // BatchNorm folds: 128-row tiles; WGRAD's dz-only fold also takes 64-row tiles and the 64x256 stem
    // tile (no 256x64 wide tile: with the fold's x chunks and coefficients it spills; the stem tile
    // reads the folded operand once instead of once per 128-column tile)
    if (mode != MODE_WGRAD) return reg(KF_FOLD, 128, default_bn(p));
    if (!p.act_sc && wgrad_wide(p) == 1) return reg(KF_FOLD, 64, 256);
    return reg(KF_FOLD, p.gm <= 64 ? 64 : 128, default_bn(p));   // (the activation fold needs gm > 64: launch_fold)
  }
  if (mode == MODE_WGRAD) {
    if (use_wgrad_dma32(p)) return {KF_WGRAD_DMA32, p.gm <= 64 ? 64 : 128, default_bn(p), false, false};
    const int w = wgrad_wide(p);
    if (w == 1) return reg(KF_REG, 64, 256);
    if (w == 2) return reg(KF_REG, 256, 64);
    return reg(KF_REG, default_bm(p), default_bn(p));
  }
  if (use_halo(mode, p)) {
    const bool ovl = mode == MODE_DGRAD ? halo_dgrad_ovl(p) : !p.resid && !p.relu && !p.bias && kn_halo_ovl.get();
    return {KF_HALO, HALO_BM, 64, ovl, false};
  }
  if (use_igemm8(mode, p) == 256) return {KF_DMA8, BM8, 256, false, false};
  if (use_bm64_smallgrid(mode, p, stats)) return reg(KF_REG_SMALLGRID, 64, 128);
  switch (use_dma4(mode, p)) {
    case 1: return {use_dma32(mode, p) ? KF_DMA32 : KF_DMA4, 128, 128, false, false};
    case 2: return {use_dma32(mode, p) ? KF_DMA32 : KF_DMA4, 128, 64, false, false};
    case 3: return {KF_DMA4, 256, 64, false, false};
    default: return reg(KF_REG, default_bm(p), default_bn(p));
  }
}
static KernelChoice choose_kernel(int mode, const IgemmParams& p) { return choose_kernel(mode, p, p.stats != nullptr); }

// "<family>/<BM>x<BN>" of a choice (the conv_kernel_choice op; tests pin every case to its kernel with it)
static std::string choice_tag(int mode, const KernelChoice& c) {
  const bool wg = mode == MODE_WGRAD;
  const char* fam = "";
  switch (c.family) {
    case KF_REG: fam = !wg ? "reg" : (c.m32 ? "wgrad_m32" : "wgrad"); break;
    case KF_REG_SMALLGRID: fam = "reg_smallgrid"; break;
    case KF_FOLD: fam = !wg ? "fold" : (c.m32 ? "fold_wgrad_m32" : "fold_wgrad"); break;
    case KF_DMA4: fam = "dma4"; break;
    case KF_DMA32: fam = "dma32"; break;
    case KF_DMA8: fam = "dma8"; break;
    case KF_HALO: fam = c.halo_ovl ? "halo_ovl" : "halo"; break;
    case KF_WGRAD_DMA32: fam = "wgrad_dma32"; break;
  }
  return std::string(fam) + "/" + std::to_string(c.bm) + "x" + std::to_string(c.bn);
}

// split-K over whole K-steps of kq reduction elements: at most nsplit splits, none of them empty
static void set_split(IgemmParams& p, int nsplit, int kq) {
  const int ksteps = ceil_div(p.gk, kq);
  const int steps_per = ceil_div(ksteps, std::max(1, nsplit));
  p.nsplit = ceil_div(ksteps, steps_per);
  p.ksplit = steps_per * kq;
}

// BatchNorm fold launches (fold_x / act_sc): operand checks, then the choice's tile with igemm_kernel's
// FOLD bitmask (1 = the A operand is formed while staging, 2 = WGRAD's B operand is)
template <int MODE>
static void launch_fold(IgemmParams& p, const KernelChoice& c, hipStream_t st) {
  const bool n64 = c.bn == 64;
  if constexpr (MODE == MODE_DGRAD) {
    TORCH_CHECK(p.fold_x && !p.act_sc, "igemm fold: DGRAD folds only the BatchNorm-backward dz");
    TORCH_CHECK(p.R == 1 && p.S == 1 && p.stride == 1 && p.K % BK == 0 && p.nsplit == 1 && p.ksplit % BK == 0,
                "igemm fold: DGRAD of a 1x1 stride-1 conv with K % 64 == 0, no split");
    launch_reg_bn<MODE, 128, 1>(n64, p, st);
  } else if constexpr (MODE == MODE_FWD) {
    TORCH_CHECK(p.act_sc && p.act_sh && !p.fold_x, "igemm fold: FWD folds only the BatchNorm-forward activation");
    TORCH_CHECK(p.R == 1 && p.S == 1 && p.stride == 1 && p.C % BK == 0 && p.nsplit == 1 && p.ksplit % BK == 0,
                "igemm fold: FWD of a 1x1 stride-1 conv with C % 64 == 0, no split");
    launch_reg_bn<MODE, 128, 1>(n64, p, st);
  } else {
    TORCH_CHECK(p.K % 8 == 0 && p.C % 8 == 0, "igemm fold: WGRAD needs K % 8 == 0 and C % 8 == 0");
    if (p.act_sc) {   // B-operand fold (optionally with the A-operand dz fold): 128-row tiles
      TORCH_CHECK(p.gm > 64, "igemm fold: WGRAD activation fold needs >= 65 output channels");
      if (p.fold_x) launch_reg_bn<MODE, 128, 3>(n64, p, st); else launch_reg_bn<MODE, 128, 2>(n64, p, st);
    } else if (c.bn == 256) {
      launch_reg<MODE, 64, 256, 1>(p, st);
    } else if (c.bm == 64) {
      launch_reg_bn<MODE, 64, 1>(n64, p, st);
    } else {
      launch_reg_bn<MODE, 128, 1>(n64, p, st);
    }
  }
}

// The launch of a choice: a switch to the template instantiations of this mode, nothing decided here.
template <int MODE>
static void dispatch(IgemmParams& p, const KernelChoice& c, hipStream_t st) {
  const bool n64 = c.bn == 64;
  if (c.family == KF_FOLD) return launch_fold<MODE>(p, c, st);
  if (c.family == KF_REG) {
    if constexpr (MODE == MODE_WGRAD) {
      if (c.bn == 256) return launch_reg<MODE, 64, 256>(p, st);
      if (c.bm == 256) return launch_reg<MODE, 256, 64>(p, st);
    }
    if (c.bm == 32) return launch_reg_bn<MODE, 32>(n64, p, st);
    if (c.bm == 64) return launch_reg_bn<MODE, 64>(n64, p, st);
    return launch_reg_bn<MODE, 128>(n64, p, st);
  }
  if constexpr (MODE != MODE_WGRAD) {
    switch (c.family) {
      case KF_HALO: return launch_halo<MODE>(p, c.halo_ovl, st);
      case KF_DMA8: return launch_dma<MODE, 256, 256, 2, 4, NT8, 1>(p, st);
      case KF_REG_SMALLGRID: return launch_reg<MODE, 64, 128>(p, st);
      case KF_DMA32:
        if (n64) launch_dma32<MODE, 128, 64, 2, 2>(p, st); else launch_dma32<MODE, 128, 128, 2, 2>(p, st);
        return;
      case KF_DMA4:
        if (c.bm == 256) launch_dma<MODE, 256, 64, 4, 1, NT, 2>(p, st);
        else if (n64) launch_dma<MODE, 128, 64, 2, 2, NT, 2>(p, st);
        else launch_dma<MODE, 128, 128, 2, 2, NT, 2>(p, st);
        return;
      default: break;
    }
  }
  TORCH_CHECK(false, "igemm dispatch: kernel family ", c.family, " has no launch in mode ", MODE);
}
// choose and launch (the planner's default kind, whose split count is its own)
template <int MODE>
static void dispatch(IgemmParams& p, hipStream_t st) { dispatch<MODE>(p, choose_kernel(MODE, p), st); }

template <int BM, int BN, int WM, int WN, int MINB>
static void launch_gemm32(IgemmParams& p, hipStream_t st) {
  TORCH_CHECK(p.R == 1 && p.S == 1 && p.stride == 1 && p.pad == 0 && p.gk % BK == 0 && p.ksplit % BK == 0 &&
                  !p.stats && !p.bn_x && !p.fold_x && !p.act_sc && p.gn % 4 == 0,
              "gemm32: plain 1x1 GEMMs only");
  p.tiles_m = ceil_div(p.gm, BM);
  p.tiles_n = ceil_div(p.gn, BN);
  const int grid = p.tiles_m * p.tiles_n * p.nsplit;
  constexpr size_t smem = (size_t)2 * (BM + BN) * BK * 2;
  static_assert(smem <= 160 * 1024, "gemm32: LDS budget");
  launch_lds<gemm32_kernel<BM, BN, WM, WN, MINB>>(dim3(grid), dim3(WM * WN * 64), smem, st, p);
}

// splitk_reduce2_kernel: dst[i] (+)= sum_s ws[s][i] over n4 float4 columns, with the split dimension
// over 1 / 4 / 16 thread lanes by the split count.  (A template so that only the translation units
// that call it instantiate the three kernels.)
template <class T>
static void launch_splitk_reduce2(const T* ws, T* out, int n4, int nsplit, bool accumulate, hipStream_t st) {
  const int SL = nsplit <= 8 ? 1 : (nsplit <= 32 ? 4 : 16);
  const dim3 grid(ceil_div(n4, 256 / SL)), block(256);
  if (SL == 1) hipLaunchKernelGGL(splitk_reduce2_kernel<1>, grid, block, 0, st, ws, out, n4, nsplit, (int)accumulate);
  else if (SL == 4) hipLaunchKernelGGL(splitk_reduce2_kernel<4>, grid, block, 0, st, ws, out, n4, nsplit, (int)accumulate);
  else hipLaunchKernelGGL(splitk_reduce2_kernel<16>, grid, block, 0, st, ws, out, n4, nsplit, (int)accumulate);
  PCMP_LAUNCH_CHECK();
}

}  // namespace pcmp
