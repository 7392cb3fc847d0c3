// MXFP4-weight (W4A8) inference path of the Linear layers: the weights are OCP MXFP4 (E2M1 elements, two per byte,
// one E8M0 scale per 32 consecutive K elements), the activations stay MXFP8 as mxfp8_quant makes them, and both meet
// on the gfx950 block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz:4: an E2M1 first operand in four
// registers against an E4M3 second operand in eight).
//
//   mxfp4_quant(w [R,K] bf16 | fp32)                              -> (q [R,K/2] uint8, e [R, 4*ceil(K/128)] uint8)
//   linear_mxfp4_fwd(xq, ex, wq4 [N,K/2], ew, bias?, act, out_mx) -> [y bf16 [M,N]]  or  [yq, ye] (out_mx, MXFP8)
//       y[m,n] = act(sum_b 2^(ex[m,b] + ew[n,b] - 254) * sum_{k in b} xq[m,k] * e2m1(wq4[n,k]) + bias[n])
//
// Contract (docs/PARITY.md "The mxfp4 inference matmul mode"): K % 32 == 0; block amax = m * 2^E (1 <= m < 2) gives
// t = E - 2 if m <= 1.5 else E - 1, clamped below at -127; e = t + 127; code = e2m1_rne(v * 2^-t) on the grid
// {0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the even code, sign << 3 | magnitude; the multiply is exact and the scaled
// amax lies in (3, 6], so nothing saturates.  The sign bit is the value's own, also where the magnitude rounds to
// zero (what v_cvt_scalef32_pk_fp4_f32 produces).  Element k sits in byte k / 2, even k in the low nibble.  A zero
// block gets e = 127; the scale row is padded with 127 to whole dwords.  Products of E4M3 by E2M1 are exact, sums
// run in fp32, split-K partials are reduced in a fixed order: two runs are bitwise equal.
//
// Operand layout of the E2M1 operand, as measured: lane (fr, g) supplies, for row fr, k = 32g .. 32g+31 in its four
// registers in memory order (nibble p of the 16 bytes is k = 32g + p), and in byte 0 of its scale register the E8M0
// scale of that same block g.  So a lane reads the 16-byte chunk g of a row's 64-byte K-step and byte g of the
// row's scale dword: unlike the E4M3 operand (mxfp8.hip), whose chunks g and 4+g straddle blocks, data and scale
// of a lane belong together here.
//
// Kernels:
//   mxfp4_quant_kernel     mxfp8_quant_kernel's work split (8 elements per lane, a quad per block, amax by two
//                          quad DPP moves); a lane emits one dword of eight nibbles
//   mxfp4w_gemm_kernel     M > 16: mxfp8_gemm_kernel's pipeline (LDS-DMA, two stages, one barrier per K-step,
//                          scale dwords behind the tile) with a B tile of 64-byte rows in an LDS image of its own
//   mxfp4w_skinny_kernel   M <= 16: x rows and x scale dwords of the K split in LDS; per trip of four K-steps
//                          (512 elements) a lane streams four 16-byte weight chunks and one 16-byte load of its
//                          row's sixteen scales into four scaled MFMAs; split-K partials + reduce kernel
#include "mx_common.h"

namespace pcmp {

// biased E8M0 scale of an E2M1 block from its fp32 amax: the smallest t with amax / 2^t <= 6
__device__ __forceinline__ unsigned mx4_scale_of(float amax) {
  const unsigned u = __float_as_uint(amax);
  const int e = (int)(u >> 23) - 2 + ((u & 0x7fffffu) > 0x400000u ? 1 : 0);
  return amax > 0.f ? (unsigned)max(e, 0) : kE8M0One;
}
// eight floats times r -> eight E2M1 nibbles, element 0 in the lowest (the convert's own scale stays 1)
__device__ __forceinline__ unsigned quant8_e2m1(const float (&v)[8], float r) {
  unsigned u = 0;
  u = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(u, v[0] * r, v[1] * r, 1.f, 0);
  u = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(u, v[2] * r, v[3] * r, 1.f, 1);
  u = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(u, v[4] * r, v[5] * r, 1.f, 2);
  u = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(u, v[6] * r, v[7] * r, 1.f, 3);
  return u;
}

// ------------------------------------------------------------------------------------------------
// Block quantiser.  Thread i of the grid holds elements 8i .. 8i+7 of the flat [R * K] operand (K % 32 == 0:
// a block never straddles rows) and writes dword i of q; its quad holds block i >> 2.
template <typename T>
__global__ void __launch_bounds__(256) mxfp4_quant_kernel(const T* __restrict__ x, unsigned* __restrict__ q,
                                                         uint8_t* __restrict__ e, int nblk, int bpr, int ew) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int blk = i >> 2;
  const bool live = blk < nblk;               // uniform over a quad
  float v[8];
  if (live) load8<T>(x + (size_t)i * 8, v);
  else {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = 0.f;
  }
  float amax = amax8(v, 0.f);
  amax = fmaxf(amax, dpp_mov<0xB1>(amax));    // quad_perm(1,0,3,2)
  amax = fmaxf(amax, dpp_mov<0x4E>(amax));    // quad_perm(2,3,0,1)
  const unsigned sc = mx4_scale_of(amax);
  if (!live) return;
  q[i] = quant8_e2m1(v, mx_inv_scale(sc));    // sc <= 253: 254 - sc is the exponent field of a normal number
  if ((i & 3) == 0) {
    const int row = blk / bpr, cb = blk - row * bpr;
    uint8_t* er = e + (size_t)row * ew;
    er[cb] = (uint8_t)sc;
    if (cb == bpr - 1)                        // the owner of the row's last block pads the row to whole dwords
      for (int c = bpr; c < ew; ++c) er[c] = (uint8_t)kE8M0One;
  }
}

std::vector<at::Tensor> mxfp4_quant(const at::Tensor& x) {
  PCMP_CHECK_CUDA(x);
  PCMP_CHECK_CONTIG(x);
  TORCH_CHECK(x.dim() == 2, "mxfp4_quant: x must be [R, K]");
  const int64_t R = x.size(0), K = x.size(1);
  TORCH_CHECK(K > 0 && K % 32 == 0 && R * K < (1ll << 31), "mxfp4_quant: K must be a multiple of 32 (got ", K, ")");
  const int64_t ew = 4 * ((K + 127) / 128);
  at::Tensor q = torch::empty({R, K / 2}, x.options().dtype(at::kByte));
  at::Tensor e = torch::empty({R, ew}, x.options().dtype(at::kByte));
  if (R == 0) return {q, e};
  const int nblk = (int)(R * K / 32);
  const dim3 grid(ceil_div(nblk, 64)), block(256);
  if (x.scalar_type() == at::kBFloat16)
    hipLaunchKernelGGL(mxfp4_quant_kernel<__bf16>, grid, block, 0, cur_stream(), ptr<const __bf16>(x), ptr<unsigned>(q),
                       ptr<uint8_t>(e), nblk, (int)(K / 32), (int)ew);
  else if (x.scalar_type() == at::kFloat)
    hipLaunchKernelGGL(mxfp4_quant_kernel<float>, grid, block, 0, cur_stream(), ptr<const float>(x), ptr<unsigned>(q),
                       ptr<uint8_t>(e), nblk, (int)(K / 32), (int)ew);
  else TORCH_CHECK(false, "mxfp4_quant: x must be bf16 or fp32");
  PCMP_LAUNCH_CHECK();
  return {q, e};
}

// the E2M1 operand rides in the low four registers of the builtin's eight-register argument
__device__ __forceinline__ f32x4 mfma_w4a8(const i32x4& w, const i32x8& x, const f32x4& acc, int sw, int sx) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(__builtin_shufflevector(w, w, 0, 1, 2, 3, -1, -1, -1, -1), x, acc,
                                                          4 /* E2M1 */, 0 /* E4M3 */, 0, sw, 0, sx);
}

// ------------------------------------------------------------------------------------------------
// LDS image of the B tile: [rows][64 bytes], four 16-byte chunks per row.  A wave's ds_read_b128 of a B fragment
// takes rows 16j .. 16j+15 (lane fr) at one chunk per lane group g.  The LDS has 64 four-byte banks, 256 bytes,
// so four consecutive rows fill the banks once and rows r, r+4, r+8, r+12 start at the same bank: unswizzled,
// sixteen lanes of one g would hit each bank group four times.  With the chunk stored at slot chunk ^ ((row >> 2) & 3)
// the sixteen rows of one g land on sixteen different 16-byte bank groups ((row & 3) picks the 64-byte quarter,
// the xor makes the four rows of a quarter take four different slots), whether the hardware serves the 64 lanes
// in groups of 8 or of 16 consecutive lanes.  (rr_off is the same idea for 128-byte rows.)  The LDS-DMA writes
// lane l's 16 bytes at l * 16, row l >> 2, slot l & 3, so the lane fetches chunk (l & 3) ^ ((l >> 4) & 3).
__device__ __forceinline__ int b4_off(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }

// Tiled GEMM, M > 16.  4 waves as 2 x 2; W x X as in mxfp8_gemm_kernel.  LDS stage: [A tile BM x 128][B tile
// BN x 64][scale dwords of the BM A rows, then of the BN B rows].  p.K counts elements: an A row has K bytes,
// a B row K / 2.
template <int BM, int BN, bool OUT_MX>
__global__ void __launch_bounds__(256, 2) mxfp4w_gemm_kernel(const MxParams p) {
  constexpr int WTM = BM / 2, WTN = BN / 2, TM = WTM / 16, TN = WTN / 16;
  constexpr int KB = 128;
  constexpr int A_BYTES = BM * KB, T_BYTES = A_BYTES + BN * (KB / 2), STAGE = T_BYTES + (BM + BN) * 4;
  constexpr int NA = BM / 8 / 4, NB = BN / 16 / 4;
  static_assert(NA >= 1 && NB >= 1 && TM >= 1 && TN >= 1 && TN % 2 == 0 && BM % 64 == 0 && BN % 64 == 0, "mxfp4w tile");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int M = p.M, N = p.N, K = p.K, K2 = K >> 1;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_m = lin / p.tiles_n, tile_n = lin - tile_m * p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int nk = (K + KB - 1) / KB;
  const __amdgpu_buffer_rsrc_t rsA = make_rsrc(p.x, (unsigned)((size_t)M * K)), rsB = make_rsrc(p.w, (unsigned)((size_t)N * K2));
  const int gch = (lane & 7) ^ (lane >> 3);          // A: rr_off image, 8 rows of 8 chunks per DMA
  const int gch4 = (lane & 3) ^ ((lane >> 4) & 3);   // B: b4_off image, 16 rows of 4 chunks per DMA
  unsigned a_vo[NA], b_vo[NB];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int m = m0 + (wid * NA + i) * 8 + (lane >> 3);
    a_vo[i] = m < M ? (unsigned)((size_t)m * K + gch * 16) : kOOB;
  }
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int n = n0 + (wid * NB + i) * 16 + (lane >> 2);
    b_vo[i] = n < N ? (unsigned)((size_t)n * K2 + gch4 * 16) : kOOB;
  }
  // scale dwords: this wave's 64 rows of the (A rows, B rows) list all belong to one operand
  constexpr bool kScaleWave4 = (BM + BN) / 64 >= 4;          // 128x128: every wave; 64x64: waves 0 and 1
  const int uwid = __builtin_amdgcn_readfirstlane(wid);
  const bool sc_wave = kScaleWave4 || uwid < (BM + BN) / 64;
  const bool sc_is_a = uwid * 64 < BM;
  const __amdgpu_buffer_rsrc_t rsE = sc_is_a ? make_rsrc(p.ex, (unsigned)((size_t)M * p.eb))
                                             : make_rsrc(p.ew, (unsigned)((size_t)N * p.eb));
  unsigned e_vo;
  {
    const int r = sc_is_a ? m0 + wid * 64 + lane : n0 + wid * 64 - BM + lane;
    e_vo = r < (sc_is_a ? M : N) ? (unsigned)((size_t)r * p.eb) : kOOB;
  }
  auto issue = [&](int s, int t) {
    const int k0 = t * KB;
    const bool live = k0 + gch * 16 < K;     // K tail: this lane's chunk lies inside the row (16 elements of A,
    const bool live4 = k0 + gch4 * 32 < K;   // 32 of B)
#pragma unroll
    for (int i = 0; i < NA; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(smem + s * STAGE + (wid * NA + i) * 1024), 16,
                                               (int)(live && a_vo[i] != kOOB ? a_vo[i] + k0 : kOOB), 0, 0, 0);
#pragma unroll
    for (int i = 0; i < NB; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(smem + s * STAGE + A_BYTES + (wid * NB + i) * 1024), 16,
                                               (int)(live4 && b_vo[i] != kOOB ? b_vo[i] + (k0 >> 1) : kOOB), 0, 0, 0);
    if (sc_wave)   // wave-uniform
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsE, (__attribute__((address_space(3))) void*)(smem + s * STAGE + T_BYTES + wid * 256), 4,
                                               (int)(e_vo != kOOB ? e_vo + 4 * t : kOOB), 0, 0, 0);
  };
  f32x4 acc[TN][TM];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int i = 0; i < TM; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, g = lane >> 4;
  issue(0, 0);
  for (int t = 0; t < nk; ++t) {
    const int s = t & 1;
    // stage t has landed (this wave's DMA, then everyone's); every wave is past its reads of the other stage
    wait_vm_b<0>();
    lds_sync();
    if (t + 1 < nk) issue(s ^ 1, t + 1);
    const char* sA = smem + s * STAGE;
    const char* sB = sA + A_BYTES;
    const unsigned* sEA = reinterpret_cast<const unsigned*>(sA + T_BYTES);
    const unsigned* sEB = sEA + BM;
    i32x8 fa[TM];
    i32x4 fb[TN];
    int ea[TM], eb[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row = wr * WTM + i * 16 + fr;
      const i32x4 lo = *reinterpret_cast<const i32x4*>(sA + rr_off(row, g));
      const i32x4 hi = *reinterpret_cast<const i32x4*>(sA + rr_off(row, 4 + g));
      fa[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      ea[i] = (int)__builtin_amdgcn_ubfe(sEA[row], 8 * g, 8);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int row = wc * WTN + j * 16 + fr;
      fb[j] = *reinterpret_cast<const i32x4*>(sB + b4_off(row, g));
      eb[j] = (int)__builtin_amdgcn_ubfe(sEB[row], 8 * g, 8);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int i = 0; i < TM; ++i) acc[j][i] = mfma_w4a8(fb[j], fa[i], acc[j][i], eb[j], ea[i]);
  }
  mx_tile_epilogue<BM, BN, OUT_MX>(p, acc, m0, n0, wr, wc, fr, g);
}

// ------------------------------------------------------------------------------------------------
// Skinny GEMM, M <= 16: a weight stream.  Block = 64 output channels x one K split; wave w owns channels 16w ..
// 16w+15.  LDS as in mxfp8_skinny_kernel: the x rows of the split (16 rows, zero beyond M and beyond K, 16-byte row
// pad), then their scale dwords.  A weight row's K-step is 64 bytes and lane group g owns its chunk g, so one load
// instruction of the four groups of a row covers 64 contiguous bytes.  Per trip of four K-steps (512 elements,
// 256 bytes of the row) a lane issues four 16-byte weight loads and one 16-byte load of the row's sixteen scale
// bytes of the trip (dword u = K-step u, byte g = this lane's block; a split's partial last trip loads its dwords
// one by one; rows past N read zeros through the buffer descriptor, next to weight registers that are zero), then
// feeds four MFMAs.
constexpr int kMx4SkinnyStep = 512;
__global__ void __launch_bounds__(256) mxfp4w_skinny_kernel(const MxParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int M = p.M, N = p.N, K = p.K;
  const int cg = blockIdx.x % p.tiles_n, split = blockIdx.x / p.tiles_n;
  const int kb = split * p.kper;                                              // multiple of 512
  const int klen = min(K - kb, p.kper);                                       // elements of this split, multiple of 32
  const int kpad = (klen + kMx4SkinnyStep - 1) / kMx4SkinnyStep * kMx4SkinnyStep;   // <= p.kper
  const int rs = p.kper + 16;                                                 // LDS row stride of x
  const int cpr = kpad >> 4;                                                  // 16-byte chunks per LDS row
  const int dpr = p.kper >> 7;                                                // scale dwords per LDS row
  unsigned* sE = reinterpret_cast<unsigned*>(smem + 16 * rs);
  for (int idx = tid; idx < 16 * cpr; idx += 256) {
    const int m = idx / cpr, c = idx - m * cpr;
    uint4 v = {0u, 0u, 0u, 0u};
    if (m < M && c * 16 < klen) v = *reinterpret_cast<const uint4*>(p.x + (size_t)m * K + kb + c * 16);
    *reinterpret_cast<uint4*>(smem + m * rs + c * 16) = v;
  }
  for (int idx = tid; idx < 16 * (kpad >> 7); idx += 256) {
    const int m = idx / (kpad >> 7), d = idx - m * (kpad >> 7);
    unsigned v = kE8M0OneX4;
    if (m < M && d * 128 < klen) v = *reinterpret_cast<const unsigned*>(p.ex + (size_t)m * p.eb + (kb >> 5) + 4 * d);
    sE[m * dpr + d] = v;
  }
  __syncthreads();
  const int fr = lane & 15, g = lane >> 4;
  const int nrow = cg * 64 + wid * 16 + fr;
  const bool nok = nrow < N;
  const uint8_t* wrow = p.w + ((size_t)(nok ? nrow : 0) * K + kb) / 2 + 16 * g;
  const __amdgpu_buffer_rsrc_t rsE = make_rsrc(p.ew, (unsigned)((size_t)N * p.eb));
  const unsigned e_vo = nok ? (unsigned)((size_t)nrow * p.eb + (kb >> 5)) : kOOB;
  const char* xrow = smem + fr * rs;
  const uint8_t* xe = reinterpret_cast<const uint8_t*>(sE + fr * dpr);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < kpad; k0 += kMx4SkinnyStep) {
    i32x4 fw[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)   // klen % 32 == 0: a lane's chunk is one whole block, inside the split or outside
      fw[u] = nok && k0 + 128 * u + 32 * g < klen ? *reinterpret_cast<const i32x4*>(wrow + (k0 >> 1) + 64 * u) : i32x4{0, 0, 0, 0};
    unsigned se[4];
    if (k0 + kMx4SkinnyStep <= klen) {   // block-uniform: the sixteen bytes lie inside the scale row
      const uint4 se4 = bload16(rsE, e_vo != kOOB ? e_vo + (k0 >> 5) : kOOB);
      se[0] = se4.x, se[1] = se4.y, se[2] = se4.z, se[3] = se4.w;
    } else {                             // the split's last, partial trip: a dword per K-step that has data
#pragma unroll
      for (int u = 0; u < 4; ++u)
        se[u] = k0 + 128 * u < klen ? (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rsE, (int)(e_vo != kOOB ? e_vo + (k0 >> 5) + 4 * u : kOOB), 0, 0)
                                    : kE8M0OneX4;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kk = k0 + 128 * u + 16 * g;
      const i32x4 lo = *reinterpret_cast<const i32x4*>(xrow + kk), hi = *reinterpret_cast<const i32x4*>(xrow + kk + 64);
      const i32x8 fx = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      acc = mfma_w4a8(fw[u], fx, acc, (int)__builtin_amdgcn_ubfe(se[u], 8 * g, 8), (int)xe[(k0 >> 5) + 4 * u + g]);
    }
  }
  // lane holds row m = fr, channels n .. n+3
  const int m = fr, n = cg * 64 + wid * 16 + 4 * g;
  if (m >= M || n >= N) return;
  if (p.ns == 1) mx_store4(p, m, n, acc);
  else *reinterpret_cast<f32x4*>(p.ws + ((size_t)split * M + m) * N + n) = acc;
}

// split-K reduce + epilogue: one thread per four channels, partials summed in split order
__global__ void __launch_bounds__(256) mxfp4w_skinny_reduce_kernel(const MxParams p) {
  const int n4 = p.N >> 2;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.M * n4) return;
  const int m = idx / n4, n = (idx - m * n4) * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < p.ns; ++s) acc += *reinterpret_cast<const f32x4*>(p.ws + ((size_t)s * p.M + m) * p.N + n);
  mx_store4(p, m, n, acc);
}

static void launch_mx4_skinny(MxParams& p, const at::Tensor& like) {
  skinny_split_plan(p.N, p.K, kMx4SkinnyStep, p.kper, p.ns);   // kper in K elements = bytes of an x row
  p.tiles_n = ceil_div(p.N, 64);
  at::Tensor ws;
  if (p.ns > 1) {
    ws = torch::empty({p.ns, p.M, p.N}, like.options().dtype(at::kFloat));
    p.ws = ptr<float>(ws);
  }
  const size_t smem = (size_t)16 * (p.kper + 16) + (size_t)16 * (p.kper / 128) * 4;
  launch_lds<mxfp4w_skinny_kernel>(dim3(p.tiles_n * p.ns), dim3(256), smem, cur_stream(), p);
  if (p.ns > 1) {
    hipLaunchKernelGGL(mxfp4w_skinny_reduce_kernel, dim3(ceil_div((int64_t)p.M * (p.N / 4), 256)), dim3(256), 0, cur_stream(), p);
    PCMP_LAUNCH_CHECK();
  }
}

template <int BM, int BN>
static void launch_mx4_tiled(MxParams& p, bool out_mx) {
  p.tiles_m = ceil_div(p.M, BM);
  p.tiles_n = ceil_div(p.N, BN);
  const dim3 grid(p.tiles_m * p.tiles_n), block(256);
  const size_t smem = (size_t)2 * (BM * 128 + BN * 64 + (BM + BN) * 4);
  if (out_mx) launch_lds<mxfp4w_gemm_kernel<BM, BN, true>>(grid, block, smem, cur_stream(), p);
  else launch_lds<mxfp4w_gemm_kernel<BM, BN, false>>(grid, block, smem, cur_stream(), p);
}

std::vector<at::Tensor> linear_mxfp4_fwd(const at::Tensor& xq, const at::Tensor& ex, const at::Tensor& wq4, const at::Tensor& ew,
                                         const c10::optional<at::Tensor>& bias, int64_t act, bool out_mx) {
  fp8_gemm_checks("linear_mxfp4_fwd", xq, wq4, bias, 32, act, kFmtE4M3, true);   // the 2 GiB limits hold for the packed N * K / 2 too
  const int64_t M = xq.size(0), K = xq.size(1), N = wq4.size(0);
  const int64_t ewb = 4 * ((K + 127) / 128), ewn = 4 * ((N + 127) / 128);
  TORCH_CHECK(ex.is_cuda() && ew.is_cuda() && ex.is_contiguous() && ew.is_contiguous() && ex.scalar_type() == at::kByte &&
                  ew.scalar_type() == at::kByte && ex.dim() == 2 && ew.dim() == 2 && ex.size(0) == M && ew.size(0) == N &&
                  ex.size(1) == ewb && ew.size(1) == ewb,
              "linear_mxfp4_fwd: ex [M, ", ewb, "], ew [N, ", ewb, "] uint8");
  TORCH_CHECK(!out_mx || (M > 16 && N % 32 == 0), "linear_mxfp4_fwd: out_mx needs M > 16 and N % 32 == 0 (got M = ", M,
              ", N = ", N, ")");
  MxParams p{};
  std::vector<at::Tensor> out;
  if (out_mx) {
    out = {torch::empty({M, N}, xq.options()), torch::empty({M, ewn}, ex.options())};
    p.yq = ptr<uint8_t>(out[0]);
    p.ye = ptr<uint8_t>(out[1]);
  } else {
    out = {torch::empty({M, N}, xq.options().dtype(at::kBFloat16))};
    p.y = ptr<__bf16>(out[0]);
  }
  if (M == 0 || N == 0) return out;
  p.x = ptr<const uint8_t>(xq);
  p.w = ptr<const uint8_t>(wq4);
  p.ex = ptr<const uint8_t>(ex);
  p.ew = ptr<const uint8_t>(ew);
  p.bias = optr<const float>(bias);
  p.M = (int)M, p.N = (int)N, p.K = (int)K, p.act = (int)act;
  p.eb = (int)ewb, p.ebn = (int)ewn;
  p.ns = 1;
  if (M <= 16) {
    launch_mx4_skinny(p, xq);
    return out;
  }
  // automatic = 64x64, the convention of the fp8 and mxfp8 modes (fp8_tile = 128 forces the 128x128 tile)
  if (fp8_forced_tile() == 128) launch_mx4_tiled<128, 128>(p, out_mx);
  else launch_mx4_tiled<64, 64>(p, out_mx);
  return out;
}

}  // namespace pcmp

TORCH_LIBRARY_FRAGMENT(pcmp, m) {
  m.def("mxfp4_quant(Tensor x) -> Tensor[]", &pcmp::mxfp4_quant);
  m.def("linear_mxfp4_fwd(Tensor xq, Tensor ex, Tensor wq4, Tensor ew, Tensor? bias, int act, bool out_mx) -> Tensor[]",
        &pcmp::linear_mxfp4_fwd);
}
