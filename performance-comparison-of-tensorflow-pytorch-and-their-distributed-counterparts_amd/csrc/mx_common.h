// What the MXFP8 kernels share (mxfp8.hip: Linear layers; mxfp8_conv.hip: convolutions): the E8M0 scale rule
// of a 32-element block, the operand / result record of a block-scaled GEMM and its bias + activation step.
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
  const uint8_t* w;    // [N][K] e4m3
  const uint8_t* ex;   // [M][eb] E8M0
  const uint8_t* ew;   // [N][eb] E8M0
  const float* bias;   // [N] or null
  __bf16* y;           // [M][N]                 (!out_mx)
  uint8_t* yq;         // [M][N] e4m3            (out_mx)
  uint8_t* ye;         // [M][ebn] E8M0          (out_mx)
  float* ws;           // skinny split-K partials [ns][M][N]
  int M, N, K, act;
  int eb, ebn;         // bytes per scale row of the operands / of ye
  int tiles_m, tiles_n;
  int kper, ns;        // skinny: K bytes per split (multiple of 256), splits
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

}  // namespace pcmp
