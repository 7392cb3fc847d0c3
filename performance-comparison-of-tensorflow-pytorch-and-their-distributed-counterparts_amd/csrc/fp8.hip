// FP8 (OCP E4M3) inference path of the Linear layers on the gfx950 fp8 MFMA.
//
//   fp8_quant_rows(x [M,K] bf16 | fp32)            -> (q [M,K] float8_e4m3fn, scale [M] fp32)
//   linear_fp8_fwd(xq, sx, wq [N,K], sw, bias?, act) -> y [M,N] bf16
//       y[m,n] = act(sx[m] * sw[n] * sum_k xq[m,k] * wq[n,k] + b[n]),  act: 0 none, 1 ReLU, 2 erf-GELU
//
// Contract (docs/PARITY.md "FP8 inference matmul mode"): one fp32 scale per K-contiguous row,
// amax = max_k |v|, s = amax / 448, r = 448 / amax (both correctly rounded), q = e4m3_rne(float(v) * r);
// a zero row gets s = 1, q = 0.  v * r exceeds 448 by at most two fp32 roundings, which round back to
// 448, so the conversion never saturates.  Every e4m3 x e4m3 product is exact in fp32; sums run in
// fp32 on the MFMA; split-K partials are reduced in a fixed order (no float atomics): two runs are
// bitwise equal.
//
// The fp8 training mode (csrc/fp8_train.hip, docs/PARITY.md "The fp8 training matmul mode") reuses both kernels:
//   fp8_quant_rows(x, fmt = 1)                       the same rule in E5M2 (largest finite value 57344)
//   linear_fp8_dgrad(dyq, sdy, wtq, swt)             -> dx [M,K] bf16      E5M2 x E4M3
//   linear_fp8_wgrad(dytq, sn, xtq, sk, out, acc)    out [N,K] fp32 = (acc ? out : 0) + ...
// as template variants of fp8_gemm_kernel (the format field of the scaled MFMA; an fp32 epilogue).  Why E5M2
// never saturates either is worked out in the header of fp8_train.hip.
//
// Three kernels:
//   fp8_quant_rows_kernel  one wave per row; rows of K <= 4096 stay in registers between the amax pass
//                          and the convert pass, longer rows are read twice
//   fp8_gemm_kernel        M > 16: 256 threads, BM x BN tile (64x64, or 128x128 on request), 128-byte K-steps staged by
//                          LDS-DMA into the XOR-swizzled 128-byte row image of the bf16 kernels
//                          (igemm_kernels.h rr_off / gemm32_kernel), two stages, one barrier per K-step
//   fp8_skinny_kernel      M <= 16 (batch-1 inference): bandwidth-bound; the x rows of the block's K range
//                          sit in LDS, each wave streams 16 weight rows straight from global memory into
//                          MFMA fragments; split-K partials + fp8_skinny_reduce_kernel
//
// Both operands are K-contiguous, so an MFMA fragment is consecutive bytes of one row.  A lane reads 16-byte
// chunks (skinny: two 8-byte fragments; tiled: two chunks per 32-byte fragment); which k a fragment byte carries does not matter as long as
// the x and w fragments of one MFMA carry the same k, and they do: both sides use one address rule.
#include "fp8_common.h"

namespace pcmp {

// ------------------------------------------------------------------------------------------------
// Row quantiser (load8 / amax8 / quant8: fp8_common.h)
constexpr int kQuantNI = 8;                       // 8-element chunks a lane keeps in registers
constexpr int kQuantRegK = 64 * 8 * kQuantNI;     // 4096: longest row held in registers

// REG: the row (K <= kQuantRegK) is loaded once and kept in registers; otherwise it is read twice
template <typename T, bool REG, int FMT>
__global__ void __launch_bounds__(256) fp8_quant_rows_kernel(const T* __restrict__ x, uint8_t* __restrict__ q,
                                                            float* __restrict__ scale, int M, int K) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const T* xr = x + (size_t)m * K;
  uint8_t* qr = q + (size_t)m * K;
  const int nc = K >> 3;
  float v[REG ? kQuantNI : 1][8];
  float amax = 0.f;
  if constexpr (REG) {
#pragma unroll
    for (int i = 0; i < kQuantNI; ++i) {
      const int c = lane + 64 * i;
      if (c < nc) load8<T>(xr + c * 8, v[i]);
      else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
      }
      amax = amax8(v[i], amax);
    }
  } else {
    for (int c = lane; c < nc; c += 64) {
      load8<T>(xr + c * 8, v[0]);
      amax = amax8(v[0], amax);
    }
  }
  amax = warp_max(amax);
  float s, r;
  fp8_scales<FMT>(amax, s, r);
  if (lane == 0) scale[m] = s;
  if constexpr (REG) {
#pragma unroll
    for (int i = 0; i < kQuantNI; ++i) {
      const int c = lane + 64 * i;
      if (c < nc) *reinterpret_cast<uint2*>(qr + c * 8) = quant8<FMT>(v[i], r);
    }
  } else {
    for (int c = lane; c < nc; c += 64) {
      load8<T>(xr + c * 8, v[0]);
      *reinterpret_cast<uint2*>(qr + c * 8) = quant8<FMT>(v[0], r);
    }
  }
}

template <typename T, int FMT>
static void launch_quant(const at::Tensor& x, at::Tensor& q, at::Tensor& s, int M, int K) {
  const dim3 grid(ceil_div(M, 4)), block(256);
  if (K <= kQuantRegK)
    hipLaunchKernelGGL((fp8_quant_rows_kernel<T, true, FMT>), grid, block, 0, cur_stream(), ptr<const T>(x), ptr<uint8_t>(q),
                       ptr<float>(s), M, K);
  else
    hipLaunchKernelGGL((fp8_quant_rows_kernel<T, false, FMT>), grid, block, 0, cur_stream(), ptr<const T>(x), ptr<uint8_t>(q),
                       ptr<float>(s), M, K);
  PCMP_LAUNCH_CHECK();
}

std::vector<at::Tensor> fp8_quant_rows(const at::Tensor& x, int64_t fmt) {
  PCMP_CHECK_CUDA(x);
  PCMP_CHECK_CONTIG(x);
  TORCH_CHECK(x.dim() == 2, "fp8_quant_rows: x must be [M, K]");
  const int64_t M = x.size(0), K = x.size(1);
  TORCH_CHECK(K % 8 == 0 && K > 0 && M < (1ll << 31) && K < (1ll << 31), "fp8_quant_rows: K must be a multiple of 8");
  at::Tensor q = torch::empty({M, K}, x.options().dtype(fp8_dtype(fmt)));
  at::Tensor s = torch::empty({M}, x.options().dtype(at::kFloat));
  if (M == 0) return {q, s};
  const bool bf = x.scalar_type() == at::kBFloat16, e5 = fmt == kFmtE5M2;
  TORCH_CHECK(bf || x.scalar_type() == at::kFloat, "fp8_quant_rows: x must be bf16 or fp32");
  if (bf && !e5) launch_quant<__bf16, kFmtE4M3>(x, q, s, (int)M, (int)K);
  else if (bf) launch_quant<__bf16, kFmtE5M2>(x, q, s, (int)M, (int)K);
  else if (!e5) launch_quant<float, kFmtE4M3>(x, q, s, (int)M, (int)K);
  else launch_quant<float, kFmtE5M2>(x, q, s, (int)M, (int)K);
  return {q, s};
}

// ------------------------------------------------------------------------------------------------
// Shared epilogue: four consecutive output channels n .. n+3 of row m
struct Fp8Params {
  const uint8_t* x;    // [M][K] e4m3 (e5m2 in the training GEMMs: template parameter XFMT)
  const uint8_t* w;    // [N][K] e4m3
  const float* sx;     // [M]
  const float* sw;     // [N]
  const float* bias;   // [N] or null
  __bf16* y;           // [M][N]
  float* yf;           // [M][N] fp32 output of the F32OUT epilogue (WGRAD)
  int accum;           // F32OUT: add to yf instead of overwriting it
  float* ws;           // skinny split-K partials [ns][M][N]
  int M, N, K, act;
  int tiles_m, tiles_n;
  int kper, ns;        // skinny: K bytes per split (multiple of 256), splits
};

__device__ __forceinline__ void fp8_store4(const Fp8Params& p, int m, int n, const f32x4& acc) {
  const float sm = p.sx[m];
  const f32x4 sn = *reinterpret_cast<const f32x4*>(p.sw + n);
  const f32x4 b4 = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = (sm * sn[e]) * acc[e] + b4[e];
    if (p.act == 1) v[e] = fmaxf(v[e], 0.f);
    else if (p.act == 2) v[e] = gelu_fast(v[e]);
  }
  *reinterpret_cast<uint2*>(p.y + (size_t)m * p.N + n) = uint2{f2bf2(v[0], v[1]), f2bf2(v[2], v[3])};
}

// The fp32 epilogue of the weight-gradient GEMM: out = (accum ? out : 0) + sx * sw * sum, no bias, no act
__device__ __forceinline__ void fp8_store4_f32(const Fp8Params& p, int m, int n, const f32x4& acc) {
  const float sm = p.sx[m];
  const f32x4 sn = *reinterpret_cast<const f32x4*>(p.sw + n);
  f32x4* out = reinterpret_cast<f32x4*>(p.yf + (size_t)m * p.N + n);
  f32x4 v = p.accum ? *out : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] += (sm * sn[e]) * acc[e];
  *out = v;
}

// ------------------------------------------------------------------------------------------------
// Tiled GEMM, M > 16.  4 waves as 2 x 2, wave tile (BM/2) x (BN/2) of 16x16 MFMA tiles.  A K-step is
// 128 bytes of every row: one LDS-DMA instruction moves 8 rows x 128 B, lane l fetching global chunk
// (l & 7) ^ (l >> 3) of row l >> 3 into LDS slot l & 7 -- the image rr_off addresses.  The K tail is
// predicated per 16-byte chunk (a chunk past K would read the next row, not out of range): such a
// chunk takes the out-of-range offset and lands as zeros.  The MFMA runs W x X, so a lane ends with
// four consecutive channels of one output row.
// Instruction: v_mfma_f32_16x16x128_f8f6f4 with unit block scales, one per 128-byte K-step and tile pair; lane
// group g owns chunks 2g, 2g+1 of a row.  Measured against four v_mfma_f32_16x16x32_fp8_fp8 per K-step in
// the same loop it was 2-14 % faster on the M = 4096 BERT shapes (docs/PERF_NOTES.md), so it stays.
// XFMT: the element format of x, which goes into the instruction's format field of its second operand
// (E5M2 output gradients against E4M3 weights / activations in DGRAD and WGRAD; w is always E4M3).
// F32OUT: the fp32 overwrite / accumulate epilogue instead of the bf16 one.
template <int BM, int BN, int XFMT = kFmtE4M3, bool F32OUT = false>
__global__ void __launch_bounds__(256, 2) fp8_gemm_kernel(const Fp8Params p) {
  constexpr int WTM = BM / 2, WTN = BN / 2, TM = WTM / 16, TN = WTN / 16;
  constexpr int KB = 128;                                   // bytes (= elements) per K-step
  constexpr int A_BYTES = BM * KB, STAGE = (BM + BN) * KB;
  constexpr int NA = BM / 8 / 4, NB = BN / 8 / 4;
  static_assert(NA >= 1 && NB >= 1 && TM >= 1 && TN >= 1, "fp8 tile");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int M = p.M, N = p.N, K = p.K;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_m = lin / p.tiles_n, tile_n = lin - tile_m * p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int nk = (K + KB - 1) / KB;
  const __amdgpu_buffer_rsrc_t rsA = make_rsrc(p.x, (unsigned)((size_t)M * K)), rsB = make_rsrc(p.w, (unsigned)((size_t)N * K));
  const int gch = (lane & 7) ^ (lane >> 3);
  unsigned a_vo[NA], b_vo[NB];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int m = m0 + (wid * NA + i) * 8 + (lane >> 3);
    a_vo[i] = m < M ? (unsigned)((size_t)m * K + gch * 16) : kOOB;
  }
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int n = n0 + (wid * NB + i) * 8 + (lane >> 3);
    b_vo[i] = n < N ? (unsigned)((size_t)n * K + gch * 16) : kOOB;
  }
  auto issue = [&](int s, int k0) {
    const bool live = k0 + gch * 16 < K;   // K tail: this lane's chunk lies inside the row
#pragma unroll
    for (int i = 0; i < NA; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(smem + s * STAGE + (wid * NA + i) * 1024), 16,
                                               (int)(live && a_vo[i] != kOOB ? a_vo[i] + k0 : kOOB), 0, 0, 0);
#pragma unroll
    for (int i = 0; i < NB; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(smem + s * STAGE + A_BYTES + (wid * NB + i) * 1024), 16,
                                               (int)(live && b_vo[i] != kOOB ? b_vo[i] + k0 : kOOB), 0, 0, 0);
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
    if (t + 1 < nk) issue(s ^ 1, (t + 1) * KB);
    const char* sA = smem + s * STAGE;
    const char* sB = sA + A_BYTES;
    i32x8 fa[TM], fb[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row = wr * WTM + i * 16 + fr;
      const i32x4 lo = *reinterpret_cast<const i32x4*>(sA + rr_off(row, 2 * g));
      const i32x4 hi = *reinterpret_cast<const i32x4*>(sA + rr_off(row, 2 * g + 1));
      fa[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int row = wc * WTN + j * 16 + fr;
      const i32x4 lo = *reinterpret_cast<const i32x4*>(sB + rr_off(row, 2 * g));
      const i32x4 hi = *reinterpret_cast<const i32x4*>(sB + rr_off(row, 2 * g + 1));
      fb[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int i = 0; i < TM; ++i)   // w (e4m3) x x (XFMT), both block scales E8M0 127 = 2^0
        acc[j][i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[j], fa[i], acc[j][i], kFmtE4M3, XFMT, 0, 127, 0, 127);
  }
  // epilogue: lane holds row m = .. + fr, channels n = .. + 4g .. 4g+3 of every 16x16 tile
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = m0 + wr * WTM + i * 16 + fr;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + wc * WTN + j * 16 + 4 * g;
      if (n >= N) continue;   // N % 8 == 0: all four channels are in range
      if constexpr (F32OUT) fp8_store4_f32(p, m, n, acc[j][i]);
      else fp8_store4(p, m, n, acc[j][i]);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Skinny GEMM, M <= 16.  Block = 64 output channels x one K split; wave w owns channels 16w .. 16w+15.
// The x rows of the split (padded to 16 rows, zero beyond M and beyond K) sit in LDS with a 16-byte row
// pad; per 256-byte K-step a lane issues four 16-byte global loads of its weight row (lanes g = 0..3 of
// a row cover 64 contiguous bytes per load, 256 per step) and feeds eight 16x16x32 MFMAs.
constexpr int kSkinnyStep = 256;
__global__ void __launch_bounds__(256) fp8_skinny_kernel(const Fp8Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int M = p.M, N = p.N, K = p.K;
  const int cg = blockIdx.x % p.tiles_n, split = blockIdx.x / p.tiles_n;
  const int kb = split * p.kper;
  const int klen = min(K - kb, p.kper);                                  // bytes of this split, multiple of 16
  const int kpad = (klen + kSkinnyStep - 1) / kSkinnyStep * kSkinnyStep;   // <= p.kper
  const int rs = p.kper + 16;                                            // LDS row stride
  const int cpr = kpad >> 4;                                             // 16-byte chunks per LDS row
  for (int idx = tid; idx < 16 * cpr; idx += 256) {
    const int m = idx / cpr, c = idx - m * cpr;
    uint4 v = {0u, 0u, 0u, 0u};
    if (m < M && c * 16 < klen) v = *reinterpret_cast<const uint4*>(p.x + (size_t)m * K + kb + c * 16);
    *reinterpret_cast<uint4*>(smem + m * rs + c * 16) = v;
  }
  __syncthreads();
  const int fr = lane & 15, g = lane >> 4;
  const int nrow = cg * 64 + wid * 16 + fr;
  const bool nok = nrow < N;
  const uint8_t* wrow = p.w + (size_t)(nok ? nrow : 0) * K + kb;
  const char* xrow = smem + fr * rs;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < kpad; k0 += kSkinnyStep) {
    i64x2 fw[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kk = k0 + 64 * u + 16 * g;
      fw[u] = (nok && kk < klen) ? *reinterpret_cast<const i64x2*>(wrow + kk) : i64x2{0, 0};
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const i64x2 fx = *reinterpret_cast<const i64x2*>(xrow + k0 + 64 * u + 16 * g);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(fw[u][0], fx[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(fw[u][1], fx[1], acc, 0, 0, 0);
    }
  }
  // lane holds row m = fr, channels n .. n+3
  const int m = fr, n = cg * 64 + wid * 16 + 4 * g;
  if (m >= M || n >= N) return;
  if (p.ns == 1) fp8_store4(p, m, n, acc);
  else *reinterpret_cast<f32x4*>(p.ws + ((size_t)split * M + m) * N + n) = acc;
}

// split-K reduce + epilogue: one thread per four channels, partials summed in split order
__global__ void __launch_bounds__(256) fp8_skinny_reduce_kernel(const Fp8Params p) {
  const int n4 = p.N >> 2;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.M * n4) return;
  const int m = idx / n4, n = (idx - m * n4) * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < p.ns; ++s) acc += *reinterpret_cast<const f32x4*>(p.ws + ((size_t)s * p.M + m) * p.N + n);
  fp8_store4(p, m, n, acc);
}

static void launch_skinny(Fp8Params& p, const at::Tensor& like) {   // LDS: 16 rows x (kper + 16) bytes
  const int cg = ceil_div(p.N, 64);
  skinny_split_plan(p.N, p.K, kSkinnyStep, p.kper, p.ns);
  p.tiles_n = cg;
  at::Tensor ws;
  if (p.ns > 1) {
    ws = torch::empty({p.ns, p.M, p.N}, like.options().dtype(at::kFloat));
    p.ws = ptr<float>(ws);
  }
  launch_lds<fp8_skinny_kernel>(dim3(cg * p.ns), dim3(256), (size_t)16 * (p.kper + 16), cur_stream(), p);
  if (p.ns > 1) {
    hipLaunchKernelGGL(fp8_skinny_reduce_kernel, dim3(ceil_div((int64_t)p.M * (p.N / 4), 256)), dim3(256), 0, cur_stream(), p);
    PCMP_LAUNCH_CHECK();
  }
}

template <int BM, int BN, int XFMT = kFmtE4M3, bool F32OUT = false>
static void launch_tiled(Fp8Params& p) {
  p.tiles_m = ceil_div(p.M, BM);
  p.tiles_n = ceil_div(p.N, BN);
  launch_lds<fp8_gemm_kernel<BM, BN, XFMT, F32OUT>>(dim3(p.tiles_m * p.tiles_n), dim3(256), (size_t)2 * (BM + BN) * 128, cur_stream(), p);
}
// the tile choice of linear_fp8_fwd (below), for every variant of the tiled kernel
template <int XFMT, bool F32OUT>
static void launch_tiled_auto(Fp8Params& p) {
  if (fp8_forced_tile() == 128) launch_tiled<128, 128, XFMT, F32OUT>(p);
  else launch_tiled<64, 64, XFMT, F32OUT>(p);
}

at::Tensor linear_fp8_fwd(const at::Tensor& xq, const at::Tensor& sx, const at::Tensor& wq, const at::Tensor& sw,
                          const c10::optional<at::Tensor>& bias, int64_t act) {
  fp8_gemm_checks("linear_fp8_fwd", xq, wq, bias, 16, act);
  PCMP_CHECK_CONTIG(sx);
  PCMP_CHECK_CONTIG(sw);
  PCMP_CHECK_F32(sx);
  PCMP_CHECK_F32(sw);
  const int64_t M = xq.size(0), K = xq.size(1), N = wq.size(0);
  TORCH_CHECK(sx.numel() == M && sw.numel() == N && sx.is_cuda() && sw.is_cuda(), "linear_fp8_fwd: sx [M], sw [N]");
  at::Tensor y = torch::empty({M, N}, xq.options().dtype(at::kBFloat16));
  if (M == 0 || N == 0) return y;
  Fp8Params p{};
  p.x = ptr<const uint8_t>(xq);
  p.w = ptr<const uint8_t>(wq);
  p.sx = ptr<const float>(sx);
  p.sw = ptr<const float>(sw);
  p.bias = optr<const float>(bias);
  p.y = ptr<__bf16>(y);
  p.M = (int)M, p.N = (int)N, p.K = (int)K, p.act = (int)act;
  p.ns = 1;
  if (M <= 16) {
    launch_skinny(p, xq);
    return y;
  }
  // 64x64 tiles (8 waves / SIMD hide the DMA latency of the one-barrier loop) beat 128x128 tiles on every
  // measured shape, the 576-tile M = 4096 BERT grids included (docs/PERF_NOTES.md): automatic = 64x64,
  // the 128x128 tile runs under fp8_tile = 128
  launch_tiled_auto<kFmtE4M3, false>(p);
  return y;
}

// The two backward GEMMs of the fp8 training mode (fp8_train.hip quantises their operands).  Both are the
// forward's form, C[i, j] = sa[i] * sb[j] * sum_r A[i, r] * B[j, r] with A in E5M2, on the tiled kernel:
//   DGRAD  dx[m, k] = sdy[m] * swt[k] * sum_n dyq[m, n] * wtq[k, n]              bf16
//   WGRAD  gw[n, k] = sn[n] * sk[k] * sum_m dytq[n, m] * xtq[k, m]               fp32, overwrite / accumulate
static Fp8Params fp8_train_params(const char* op, const at::Tensor& a, const at::Tensor& sa, const at::Tensor& b,
                                  const at::Tensor& sb) {
  fp8_gemm_checks(op, a, b, c10::nullopt, 16, 0, kFmtE5M2);
  const int64_t M = a.size(0), K = a.size(1), N = b.size(0);
  TORCH_CHECK(sa.is_cuda() && sb.is_cuda() && sa.is_contiguous() && sb.is_contiguous() && sa.scalar_type() == at::kFloat &&
              sb.scalar_type() == at::kFloat && sa.numel() == M && sb.numel() == N, op, ": fp32 scales, one per operand row");
  Fp8Params p{};
  p.x = ptr<const uint8_t>(a);
  p.w = ptr<const uint8_t>(b);
  p.sx = ptr<const float>(sa);
  p.sw = ptr<const float>(sb);
  p.M = (int)M, p.N = (int)N, p.K = (int)K;
  p.ns = 1;
  return p;
}

at::Tensor linear_fp8_dgrad(const at::Tensor& dyq, const at::Tensor& sdy, const at::Tensor& wtq, const at::Tensor& swt) {
  Fp8Params p = fp8_train_params("linear_fp8_dgrad", dyq, sdy, wtq, swt);
  at::Tensor dx = torch::empty({p.M, p.N}, dyq.options().dtype(at::kBFloat16));
  if (p.M == 0 || p.N == 0) return dx;
  p.y = ptr<__bf16>(dx);
  launch_tiled_auto<kFmtE5M2, false>(p);
  return dx;
}

void linear_fp8_wgrad(const at::Tensor& dytq, const at::Tensor& sn, const at::Tensor& xtq, const at::Tensor& sk, at::Tensor out,
                      bool acc) {
  Fp8Params p = fp8_train_params("linear_fp8_wgrad", dytq, sn, xtq, sk);
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.scalar_type() == at::kFloat && out.dim() == 2 && out.size(0) == p.M &&
              out.size(1) == p.N, "linear_fp8_wgrad: out must be contiguous fp32 [N, K]");
  if (p.M == 0 || p.N == 0) return;
  p.yf = ptr<float>(out);
  p.accum = acc ? 1 : 0;
  launch_tiled_auto<kFmtE5M2, true>(p);
}

}  // namespace pcmp

TORCH_LIBRARY_FRAGMENT(pcmp, m) {
  m.def("fp8_quant_rows(Tensor x, int fmt=0) -> Tensor[]", &pcmp::fp8_quant_rows);
  m.def("linear_fp8_dgrad(Tensor dyq, Tensor sdy, Tensor wtq, Tensor swt) -> Tensor", &pcmp::linear_fp8_dgrad);
  m.def("linear_fp8_wgrad(Tensor dytq, Tensor sn, Tensor xtq, Tensor sk, Tensor(a!) out, bool acc) -> ()", &pcmp::linear_fp8_wgrad);
  m.def("linear_fp8_fwd(Tensor xq, Tensor sx, Tensor wq, Tensor sw, Tensor? bias, int act) -> Tensor", &pcmp::linear_fp8_fwd);
}
