// What the block-scaled kernels share (mxfp8.hip: Linear layers; mxfp8_conv.hip: convolutions; mxfp4.hip: Linear
// layers with MXFP4 weights): the E8M0 scale rule of a 32-element E4M3 block, the operand / result record of a
// block-scaled GEMM, its bias + activation step and the epilogue of the tiled Linear GEMMs.
#pragma once
#include "fp8_common.h"

namespace pcmp {

constexpr unsigned kE8M0One = 127u, kE8M0OneX4 = 0x7f7f7f7fu;

// biased E8M0 scale of a block from its fp32 amax (no division, no log)
__device__ __forceinline__ unsigned mx_scale_of(float amax) {
  const unsigned u = __float_as_uint(amax);
  const int e = (int)(u >> 23) - 8 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
  return amax > 0.f ? (unsigned)max(e, 0) : kE8M0One;
}
// 2^-t = 2^(127 - e): e <= 247, so the exponent field 254 - e is that of a normal number
__device__ __forceinline__ float mx_inv_scale(unsigned e) { return __uint_as_float((254u - e) << 23); }

struct MxParams {
  const uint8_t* x;    // [M][K] e4m3
  const uint8_t* w;    // [N][K] e4m3, or [N][K / 2] e2m1 pairs (mxfp4.hip)
  const uint8_t* ex;   // [M][eb] E8M0
  const uint8_t* ew;   // [N][eb] E8M0
  const float* bias;   // [N] or null
  __bf16* y;           // [M][N]                 (!out_mx)
  uint8_t* yq;         // [M][N] e4m3            (out_mx)
  uint8_t* ye;         // [M][ebn] E8M0          (out_mx)
  float* ws;           // split-K partials [ns][M][N] (skinny kernels, WGRAD)
  float* yf;           // [M][N] fp32 output of the WGRAD epilogue
  int accum;           // WGRAD: add to yf instead of overwriting it
  int M, N, K, act;
  int eb, ebn;         // bytes per scale row of the operands / of ye
  int tiles_m, tiles_n;
  int kper, ns;        // skinny: K bytes per split (multiple of 256), splits; WGRAD: 128-byte K-steps per split, splits
};

// bias + activation of four consecutive channels n .. n+3
__device__ __forceinline__ void mx_bias_act(const MxParams& p, int n, const f32x4& acc, float (&v)[4]) {
  const f32x4 b4 = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = acc[e] + b4[e];
    if (p.act == 1) v[e] = fmaxf(v[e], 0.f);
    else if (p.act == 2) v[e] = gelu_fast(v[e]);
  }
}

__device__ __forceinline__ void mx_store4(const MxParams& p, int m, int n, const f32x4& acc) {
  float v[4];
  mx_bias_act(p, n, acc, v);
  *reinterpret_cast<uint2*>(p.y + (size_t)m * p.N + n) = uint2{f2bf2(v[0], v[1]), f2bf2(v[2], v[3])};
}

// Epilogue of the tiled GEMMs (4 waves as 2 x 2, wave (wr, wc); the MFMA ran W x X): bf16 rows, or (OUT_MX) the
// result quantised to (yq, ye) from registers.
template <int BM, int BN, bool OUT_MX>
__device__ __forceinline__ void mx_tile_epilogue(const MxParams& p, const f32x4 (&acc)[BN / 32][BM / 32], int m0, int n0, int wr,
                                                 int wc, int fr, int g) {
  constexpr int WTM = BM / 2, WTN = BN / 2, TM = WTM / 16, TN = WTN / 16;
  const int M = p.M, N = p.N;
  // epilogue: lane holds row m = .. + fr, channels n = .. + 4g .. 4g+3 of every 16x16 tile
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = m0 + wr * WTM + i * 16 + fr;
    if constexpr (!OUT_MX) {
      if (m >= M) continue;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + wc * WTN + j * 16 + 4 * g;
        if (n < N) mx_store4(p, m, n, acc[j][i]);   // N % 8 == 0: all four channels are in range
      }
    } else {
      // a 32-channel block is the tile pair (2jp, 2jp+1) times the four lane groups of row fr: amax over this
      // lane's 8 values, then over g (lanes xor 16, xor 32).  N % 32 == 0: a block is in range or out as a whole,
      // and the lanes that exchange values share m and the block, so they take the branches together.
#pragma unroll
      for (int jp = 0; jp < TN / 2; ++jp) {
        const int nb0 = n0 + wc * WTN + jp * 32;
        const bool ok = m < M && nb0 < N;
        float v[2][4];
        float amax = 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int n = nb0 + h * 16 + 4 * g;
          if (ok) mx_bias_act(p, n, acc[2 * jp + h][i], v[h]);
          else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[h][e] = 0.f;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fabsf(v[h][e]));
        }
        amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
        amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
        if (!ok) continue;
        const unsigned sc = mx_scale_of(amax);
        const float r = mx_inv_scale(sc);
#pragma unroll
        for (int h = 0; h < 2; ++h)
          *reinterpret_cast<unsigned*>(p.yq + (size_t)m * N + nb0 + h * 16 + 4 * g) = quant4(v[h][0], v[h][1], v[h][2], v[h][3], r);
        if (g == 0) {
          uint8_t* er = p.ye + (size_t)m * p.ebn;
          const int cb = nb0 >> 5;
          er[cb] = (uint8_t)sc;
          if (nb0 + 32 == N)                   // the row's last block: pad the scale row to whole dwords
            for (int c = cb + 1; c < p.ebn; ++c) er[c] = (uint8_t)kE8M0One;
        }
      }
    }
  }
}

}  // namespace pcmp
