// Operand quantisers of the fp8 training matmul mode of the Linear layers (docs/PARITY.md "The fp8 training
// matmul mode"): E4M3 forward, E5M2 output gradients.  For y = x W^T the two backward GEMMs reduce over N
// (DGRAD, dx = dy W) and over M (WGRAD, gw = dy^T x).  The MFMA kernel (fp8.hip: fp8_gemm_kernel) wants both
// operands contiguous along the reduction with one scale per operand row, so the backward needs transposed
// images whose scale belongs to a *column* of the source: a scale can only leave the sum if it does not depend
// on the summation index, and WGRAD sums over m -- per-row (per-m) scales of dy or x would stay inside it.
//
//   fp8_quant_cols(x [R,C] bf16 | fp32, fmt)  -> (qT [C,R] fp8, scale [C])                  x^T, W^T, dy^T
//   fp8_quant_both(dy [M,N] bf16 | fp32, fmt) -> (q [M,N], s_row [M], qT [N,M], s_col [N])  dy for DGRAD and WGRAD
//       fmt 0: E4M3 (max 448), 1: E5M2 (max 57344).  R % 16 == 0, C % 8 == 0.
//
// Rule (the one of fp8.hip, over a column instead of a row): amax = max |v|, s = amax / max, r = max / amax, both
// correctly rounded, q = rne(float(v) * r); a zero column gets s = 1, q = 0.  fp8_quant_both's row image is
// fp8_quant_rows's and its column image is fp8_quant_cols's, bit for bit.
//
// No saturation in E5M2.  |v| <= amax and r <= (57344 / amax)(1 + 2^-24), so |v| r <= 57344 (1 + 2^-24) before the
// product is rounded; 57344 (1 + 2^-24) = 57344 + 0.0034 lies within one fp32 step (2^-8 at 2^15 .. 2^16) of 57344,
// so the fp32 product is at most 57344 + 2^-8.  E5M2's spacing up there is 8192: the value after 57344 would be
// 65536 (not finite in the format) and the rounding boundary is 61440, four thousand away.  The E4M3 argument is
// the same with a spacing of 32 (boundary 464) and an fp32 step of 2^-15: E5M2 has the wider margin of the two.
//
// Two launches, no atomics, no buffer that needs clearing:
//   fp8_amax_kernel     block = 64 columns x a slab of 256 rows.  A lane owns 8 consecutive columns (one 16-byte
//                       load of bf16), 8 lanes cover the 64 columns of one row (128 contiguous bytes), a wave 8
//                       rows, the block 32 rows per step.  Running maxima per lane; the 8 row-lanes of a column
//                       group combine by shuffles, the 4 waves through LDS; one partial per (slab, column).  With
//                       ROWS the 8 lanes of a row combine too: one partial per (column block, row).
//   fp8_quant_t_kernel  block = 128 rows x 64 columns.  Prologue: the maxima of its 64 columns over the slabs
//                       (and of its 128 rows over the column blocks) from the partials, then s and r in LDS.
//                       A thread loads 4 rows x 8 columns, scales, and converts column-wise: one packed
//                       conversion pair makes the 4 row-bytes of a column, i.e. one dword of the transposed
//                       tile.  The tile sits in LDS as [64 columns][128 rows + 4] bytes: the stride of 33 dwords
//                       sends the 64 dword stores of a wave (8 column groups x 8 row groups) to 64 different
//                       banks.  It is read back as 16-byte chunks along R (four dword reads: the stride is not
//                       16-byte aligned), 8 lanes writing 128 contiguous bytes of one output row.
// Slabs combine through the partials buffer, not through an integer atomic max: a maximum is order-independent
// either way, but the atomic needs a cleared buffer -- a third launch, or a memset node a captured training step
// must not contain -- while the partials ([R / 256, C] floats, L2-resident) cost a block 64 x R / 256 loads
// beside the 8192 elements of its tile.
#include "fp8_common.h"

namespace pcmp {

constexpr int kTC = 64;               // columns of an amax block and of a transpose tile
constexpr int kSlab = 256;            // rows of an amax slab
constexpr int kTR = 128;              // rows of a transpose tile
constexpr int kTStride = kTR + 4;     // bytes between the columns of the LDS tile: 33 dwords

template <typename T, bool ROWS>
__global__ void __launch_bounds__(256) fp8_amax_kernel(const T* __restrict__ x, float* __restrict__ cpart,
                                                      float* __restrict__ rpart, int R, int C) {
  __shared__ float red[4][kTC];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int cg = lane & 7, rl = lane >> 3;
  const int c = blockIdx.x * kTC + cg * 8;
  const int r0 = blockIdx.y * kSlab;
  float m[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) m[e] = 0.f;
  for (int it = 0; it < kSlab / 32 && r0 + it * 32 < R; ++it) {
    const int r = r0 + it * 32 + wid * 8 + rl;
    float v[8];
    if (c < C && r < R) load8<T>(x + (size_t)r * C + c, v);
    else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], fabsf(v[e]));
    if constexpr (ROWS) {
      float a = amax8(v, 0.f);
      a = fmaxf(a, __shfl_xor(a, 1));
      a = fmaxf(a, __shfl_xor(a, 2));
      a = fmaxf(a, __shfl_xor(a, 4));
      if (cg == 0 && r < R) rpart[(size_t)blockIdx.x * R + r] = a;
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    m[e] = fmaxf(m[e], __shfl_xor(m[e], 8));
    m[e] = fmaxf(m[e], __shfl_xor(m[e], 16));
    m[e] = fmaxf(m[e], __shfl_xor(m[e], 32));
  }
  if (rl == 0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) red[wid][cg * 8 + e] = m[e];
  }
  __syncthreads();
  const int col = blockIdx.x * kTC + tid;
  if (tid < kTC && col < C)
    cpart[(size_t)blockIdx.y * C + col] = fmaxf(fmaxf(red[0][tid], red[1][tid]), fmaxf(red[2][tid], red[3][tid]));
}

// BOTH: also the row image q [R][C] with the row scales srow (fp8_quant_both)
template <typename T, int FMT, bool BOTH>
__global__ void __launch_bounds__(256) fp8_quant_t_kernel(const T* __restrict__ x, const float* __restrict__ cpart,
                                                         const float* __restrict__ rpart, uint8_t* __restrict__ qT,
                                                         float* __restrict__ scol, uint8_t* __restrict__ q,
                                                         float* __restrict__ srow, int R, int C, int nslab, int ncb) {
  __shared__ float red[4][kTC], rcol[kTC];
  __shared__ float redr[BOTH ? 2 : 1][kTR], rrow[kTR];
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTC * kTStride];
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * kTC, r0 = blockIdx.y * kTR;
  {   // column maxima over the slabs: 4 threads per column
    const int col = tid & 63, g = tid >> 6;
    float a = 0.f;
    if (c0 + col < C)
      for (int s = g; s < nslab; s += 4) a = fmaxf(a, cpart[(size_t)s * C + c0 + col]);
    red[g][col] = a;
  }
  if constexpr (BOTH) {   // row maxima over the column blocks: 2 threads per row
    const int row = tid & 127, g = tid >> 7;
    float a = 0.f;
    if (r0 + row < R)
      for (int b = g; b < ncb; b += 2) a = fmaxf(a, rpart[(size_t)b * R + r0 + row]);
    redr[g][row] = a;
  }
  __syncthreads();
  if (tid < kTC) {
    float s, r;
    fp8_scales<FMT>(fmaxf(fmaxf(red[0][tid], red[1][tid]), fmaxf(red[2][tid], red[3][tid])), s, r);
    rcol[tid] = r;
    if (blockIdx.y == 0 && c0 + tid < C) scol[c0 + tid] = s;
  }
  if constexpr (BOTH) {
    if (tid >= 128) {
      const int row = tid - 128;
      float s, r;
      fp8_scales<FMT>(fmaxf(redr[0][row], redr[1][row]), s, r);
      rrow[row] = r;
      if (blockIdx.x == 0 && r0 + row < R) srow[r0 + row] = s;
    }
  }
  __syncthreads();
  // 4 rows x 8 columns per thread (R % 4 == 0, C % 8 == 0: a group is inside or outside as a whole)
  const int cg = tid & 7, rg = tid >> 3;
  const int c = c0 + cg * 8, rb = r0 + rg * 4;
  const bool live = c < C && rb < R;
  float v[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (live) load8<T>(x + (size_t)(rb + i) * C + c, v[i]);
    else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float r = rcol[cg * 8 + e];
    *reinterpret_cast<unsigned*>(tile + (cg * 8 + e) * kTStride + rg * 4) = quant4<FMT>(v[0][e], v[1][e], v[2][e], v[3][e], r);
  }
  if constexpr (BOTH) {
    if (live) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<uint2*>(q + (size_t)(rb + i) * C + c) = quant8<FMT>(v[i], rrow[rg * 4 + i]);
    }
  }
  __syncthreads();
  // 16 rows of one column per chunk (R % 16 == 0); 8 lanes write the 128 bytes of one tile row of qT
#pragma unroll
  for (int pass = 0; pass < kTC / 32; ++pass) {
    const int col = (tid >> 3) + 32 * pass, r = r0 + (tid & 7) * 16;
    if (c0 + col >= C || r >= R) continue;
    const unsigned* src = reinterpret_cast<const unsigned*>(tile + col * kTStride + (tid & 7) * 16);
    *reinterpret_cast<uint4*>(qT + (size_t)(c0 + col) * R + r) = uint4{src[0], src[1], src[2], src[3]};
  }
}

template <typename T, int FMT, bool BOTH>
static void launch_quant_t(const at::Tensor& x, std::vector<at::Tensor>& o, int R, int C) {
  const int nslab = ceil_div(R, kSlab), ncb = ceil_div(C, kTC);
  at::Tensor cpart = torch::empty({nslab, C}, x.options().dtype(at::kFloat));
  at::Tensor rpart = BOTH ? torch::empty({ncb, R}, x.options().dtype(at::kFloat)) : at::Tensor();
  float* rp = BOTH ? ptr<float>(rpart) : nullptr;
  hipLaunchKernelGGL((fp8_amax_kernel<T, BOTH>), dim3(ncb, nslab), dim3(256), 0, cur_stream(), ptr<const T>(x),
                     ptr<float>(cpart), rp, R, C);
  PCMP_LAUNCH_CHECK();
  // o: {qT, scol} or {q, srow, qT, scol}
  hipLaunchKernelGGL((fp8_quant_t_kernel<T, FMT, BOTH>), dim3(ncb, ceil_div(R, kTR)), dim3(256), 0, cur_stream(),
                     ptr<const T>(x), ptr<const float>(cpart), (const float*)rp, ptr<uint8_t>(o[BOTH ? 2 : 0]),
                     ptr<float>(o[BOTH ? 3 : 1]), BOTH ? ptr<uint8_t>(o[0]) : nullptr, BOTH ? ptr<float>(o[1]) : nullptr, R, C,
                     nslab, ncb);
  PCMP_LAUNCH_CHECK();
}

template <bool BOTH>
static std::vector<at::Tensor> quant_t(const char* op, const at::Tensor& x, int64_t fmt) {
  PCMP_CHECK_CUDA(x);
  PCMP_CHECK_CONTIG(x);
  TORCH_CHECK(x.dim() == 2, op, ": x must be [R, C]");
  const int64_t R = x.size(0), C = x.size(1);
  TORCH_CHECK(R > 0 && C > 0 && R % 16 == 0 && C % 8 == 0 && R * C < (1ll << 31), op,
              ": R must be a multiple of 16 and C of 8 (got R = ", R, ", C = ", C, "), below 2^31 elements");
  const bool bf = x.scalar_type() == at::kBFloat16, e5 = fmt == kFmtE5M2;
  TORCH_CHECK(bf || x.scalar_type() == at::kFloat, op, ": x must be bf16 or fp32");
  const auto o8 = x.options().dtype(fp8_dtype(fmt)), of = x.options().dtype(at::kFloat);
  std::vector<at::Tensor> o;
  if (BOTH) o = {torch::empty({R, C}, o8), torch::empty({R}, of)};
  o.push_back(torch::empty({C, R}, o8));
  o.push_back(torch::empty({C}, of));
  if (bf && !e5) launch_quant_t<__bf16, kFmtE4M3, BOTH>(x, o, (int)R, (int)C);
  else if (bf) launch_quant_t<__bf16, kFmtE5M2, BOTH>(x, o, (int)R, (int)C);
  else if (!e5) launch_quant_t<float, kFmtE4M3, BOTH>(x, o, (int)R, (int)C);
  else launch_quant_t<float, kFmtE5M2, BOTH>(x, o, (int)R, (int)C);
  return o;
}

std::vector<at::Tensor> fp8_quant_cols(const at::Tensor& x, int64_t fmt) { return quant_t<false>("fp8_quant_cols", x, fmt); }
std::vector<at::Tensor> fp8_quant_both(const at::Tensor& dy, int64_t fmt) { return quant_t<true>("fp8_quant_both", dy, fmt); }

}  // namespace pcmp

TORCH_LIBRARY_FRAGMENT(pcmp, m) {
  m.def("fp8_quant_cols(Tensor x, int fmt=0) -> Tensor[]", &pcmp::fp8_quant_cols);
  m.def("fp8_quant_both(Tensor dy, int fmt=1) -> Tensor[]", &pcmp::fp8_quant_both);
}
