// What the fp8 matmul families share (fp8.hip: one scale per row; fp8_train.hip: the column quantisers of
// the training mode; mxfp8.hip: one E8M0 scale per 32-element block): the 8-element loads and the fp8 packs
// of the quantisers, the knobs, the split-K plan of the skinny (M <= 16) kernels and the operand checks of
// the GEMM ops.
#pragma once
#include "igemm_kernels.h"

namespace pcmp {

inline Knob kn_fp8_skinny_ns("fp8_skinny_ns", 0);   // K-split of the skinny kernel; 0: automatic
inline Knob kn_fp8_tile("fp8_tile", 0);             // tiled kernel: 0 automatic, 64 / 128 force the tile

typedef long i64x2 __attribute__((ext_vector_type(2)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
constexpr float kE4M3Max = 448.f;
// Element formats of the row-scaled family.  The numbers are the format fields of the scaled MFMA (cbsz / blgp).
constexpr int kFmtE4M3 = 0, kFmtE5M2 = 1;
template <int FMT>
constexpr float fp8_max() { return FMT == kFmtE5M2 ? 57344.f : kE4M3Max; }
inline at::ScalarType fp8_dtype(int64_t fmt) {
  TORCH_CHECK(fmt == kFmtE4M3 || fmt == kFmtE5M2, "fp8 format: 0 (E4M3) or 1 (E5M2)");
  return fmt == kFmtE5M2 ? at::kFloat8_e5m2 : at::kFloat8_e4m3fn;
}

template <typename T>
__device__ __forceinline__ void load8(const T* p, float (&v)[8]);
template <>
__device__ __forceinline__ void load8<__bf16>(const __bf16* p, float (&v)[8]) {
  const uint4 u = *reinterpret_cast<const uint4*>(p);
  const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[2 * e] = __uint_as_float(w[e] << 16);
    v[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
  }
}
template <>
__device__ __forceinline__ void load8<float>(const float* p, float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
}
__device__ __forceinline__ float amax8(const float (&v)[8], float m) {
#pragma unroll
  for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(v[e]));
  return m;
}
// four scaled floats -> four fp8 bytes (v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32, round to nearest even)
template <int FMT = kFmtE4M3>
__device__ __forceinline__ unsigned pack4(float a, float b, float c, float d) {
  int u = 0;
  if constexpr (FMT == kFmtE5M2) {
    u = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, u, false);
    u = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, u, true);
  } else {
    u = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, u, false);
    u = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, u, true);
  }
  return (unsigned)u;
}
// four floats times r -> four fp8 bytes
template <int FMT = kFmtE4M3>
__device__ __forceinline__ unsigned quant4(float a, float b, float c, float d, float r) {
  return pack4<FMT>(a * r, b * r, c * r, d * r);
}
// eight floats times r -> eight fp8 bytes
template <int FMT = kFmtE4M3>
__device__ __forceinline__ uint2 quant8(const float (&v)[8], float r) {
  return uint2{quant4<FMT>(v[0], v[1], v[2], v[3], r), quant4<FMT>(v[4], v[5], v[6], v[7], r)};
}
// s = amax / max, r = max / amax, both correctly rounded; a zero row or column: s = 1, r = 0 (q = 0)
template <int FMT>
__device__ __forceinline__ void fp8_scales(float amax, float& s, float& r) {
  s = amax > 0.f ? __fdiv_rn(amax, fp8_max<FMT>()) : 1.f;
  r = amax > 0.f ? __fdiv_rn(fp8_max<FMT>(), amax) : 0.f;
}

// Split-K plan of a skinny kernel: K bytes per split (a multiple of `step`, at most kper_max so the x rows
// of a split fit in LDS) and the number of splits.  Automatic (knob 0): at least two workgroups per CU
// (256 CUs), K ranges of at most kper_auto bytes.
constexpr int kSkinnyKperAuto = 4096, kSkinnyKperMax = 8192;
inline void skinny_split_plan(int N, int K, int step, int& kper, int& ns_out) {
  const int cg = ceil_div(N, 64);
  int ns = kn_fp8_skinny_ns.get();
  if (ns <= 0) ns = std::max(ceil_div(512, cg), ceil_div(K, kSkinnyKperAuto));
  ns = std::max(ns, ceil_div(K, kSkinnyKperMax));
  kper = ceil_div(ceil_div(K, ns), step) * step;
  ns_out = ceil_div(K, kper);
}

// operand checks shared by linear_fp8_fwd, linear_mxfp8_fwd and linear_mxfp4_fwd
// (xfmt: the format of xq; the training GEMMs take E5M2 gradients there.  w4: wq is uint8 [N, K / 2], two E2M1
// elements per byte, the weight of linear_mxfp4_fwd)
inline void fp8_gemm_checks(const char* op, const at::Tensor& xq, const at::Tensor& wq, const c10::optional<at::Tensor>& bias,
                           int64_t kmul, int64_t act, int xfmt = kFmtE4M3, bool w4 = false) {
  TORCH_CHECK(xq.is_cuda() && wq.is_cuda() && xq.is_contiguous() && wq.is_contiguous(), op, ": xq / wq must be contiguous GPU tensors");
  TORCH_CHECK(xq.scalar_type() == fp8_dtype(xfmt) && wq.scalar_type() == (w4 ? at::kByte : at::kFloat8_e4m3fn), op,
              w4 ? ": xq must be float8_e4m3fn and wq uint8 (two E2M1 elements per byte)"
                 : xfmt == kFmtE5M2 ? ": xq must be float8_e5m2 and wq float8_e4m3fn" : ": xq / wq must be float8_e4m3fn");
  TORCH_CHECK(xq.dim() == 2 && wq.dim() == 2 && xq.size(1) == (w4 ? 2 : 1) * wq.size(1), op,
              w4 ? ": xq [M, K], wq [N, K / 2]" : ": xq [M, K], wq [N, K]");
  const int64_t M = xq.size(0), K = xq.size(1), N = wq.size(0);
  TORCH_CHECK(K > 0 && K % kmul == 0 && N % 8 == 0, op, ": K must be a multiple of ", kmul, " and N of 8 (got K = ", K,
              ", N = ", N, ")");
  TORCH_CHECK(M * K < (1ll << 31) && N * K < (1ll << 31) && M * N < (1ll << 31), op, ": operand beyond 2 GiB");
  TORCH_CHECK(act >= 0 && act <= 2, op, ": act 0 (none), 1 (ReLU) or 2 (GELU)");
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(bias->is_cuda() && bias->scalar_type() == at::kFloat && bias->is_contiguous() && bias->numel() == N, op,
                ": bias fp32 [N]");
  }
}
inline int fp8_forced_tile() {
  const int tile = kn_fp8_tile.get();
  TORCH_CHECK(tile == 0 || tile == 64 || tile == 128, "knob fp8_tile: 0, 64 or 128");
  return tile;
}

}  // namespace pcmp
