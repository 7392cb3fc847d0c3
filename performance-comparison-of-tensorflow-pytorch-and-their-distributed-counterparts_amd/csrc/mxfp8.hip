// MXFP8 inference path of the Linear layers: e4m3 elements with one power-of-two (E8M0) scale per 32
// consecutive K elements, multiplied on the gfx950 block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4).
//
//   mxfp8_quant(x [R,K] bf16 | fp32)                         -> (q [R,K] float8_e4m3fn, e [R, 4*ceil(K/128)] uint8)
//   linear_mxfp8_fwd(xq, ex, wq [N,K], ew, bias?, act, out_mx) -> [y bf16 [M,N]]  or  [yq, ye] (out_mx)
//       y[m,n] = act(sum_b 2^(ex[m,b] + ew[n,b] - 254) * sum_{k in b} xq[m,k] * wq[n,k] + bias[n])
//   linear_mxfp8_wgrad(dytq [N,M], edyt, xtq [K,M], ext, out [N,K] fp32, acc)   (the mxfp8 training mode)
//       out[n,k] = (acc ? out : 0) + sum_b 2^(edyt[n,b] + ext[k,b] - 254) * sum_{m in b} dytq[n,m] * xtq[k,m]
//
// Contract (docs/PARITY.md "The mxfp8 inference matmul mode"): K % 32 == 0; block amax = m * 2^E (1 <= m < 2)
// gives t = E - 8 if m <= 1.75 else E - 7, clamped below at -127; e = t + 127; q = e4m3_rne(v * 2^-t): the
// multiply is exact and the scaled amax lies in (224, 448], so nothing saturates.  A zero block gets e = 127.
// The scale row is padded with 127 to whole dwords: the four scales of a 128-byte K-step are one aligned
// dword, in the K tail too.  The scales are applied by the MFMA; sums run in fp32; split-K partials are
// reduced in a fixed order (no float atomics): two runs are bitwise equal.
//
// Kernels:
//   mxfp8_quant_kernel     the work unit is a block: a lane holds 8 elements, a quad one block (amax by two
//                          quad DPP moves), a wave 16 blocks; the grid covers R * K / 32 blocks
//   mxfp8_gemm_kernel      M > 16: fp8_gemm_kernel's staging (LDS-DMA of 128-byte K-steps into the rr_off image,
//                          two stages, one barrier per K-step) plus the scale dwords of the stage's rows, moved
//                          by one 4-byte LDS-DMA per wave into (BM + BN) * 4 bytes behind the tile; a lane reads
//                          its row's dword from LDS and extracts byte g (one v_bfe per K-step and row tile).  OUT_MX: the epilogue quantises the
//                          fp32 result to (yq, ye) from registers
//   mxfp8_skinny_kernel    M <= 16: x rows and x scale dwords of the K split in LDS; per 128-byte K-step a lane
//                          streams two 16-byte weight chunks and its weight scale byte from global memory into
//                          one scaled 16x16x128 MFMA; split-K partials + mxfp8_skinny_reduce_kernel
//
// Operand layout of the 16x16x128 MFMA, as measured (a lane's scale does NOT cover the lane's own 32 values):
// lane (fr, g) supplies, for row fr, k = 16g .. 16g+15 in registers 0-3 and k = 64+16g .. 64+16g+15 in registers
// 4-7, and in byte 0 of its scale register (op_sel 0) the E8M0 scale of block g, k = 32g .. 32g+31, of row fr.
// So a lane reads the 16-byte chunks g and 4+g of a row's 128-byte K-step and byte g of the row's scale dword.
#include "mx_common.h"

namespace pcmp {

// ------------------------------------------------------------------------------------------------
// Block quantiser.  Thread i of the grid holds elements 8i .. 8i+7 of the flat [R * K] operand (K % 32 == 0:
// a block never straddles rows); its quad holds block i >> 2.
template <typename T>
__global__ void __launch_bounds__(256) mxfp8_quant_kernel(const T* __restrict__ x, uint8_t* __restrict__ q,
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
  const unsigned sc = mx_scale_of(amax);
  if (!live) return;
  *reinterpret_cast<uint2*>(q + (size_t)i * 8) = quant8(v, mx_inv_scale(sc));
  if ((i & 3) == 0) {
    const int row = blk / bpr, cb = blk - row * bpr;
    uint8_t* er = e + (size_t)row * ew;
    er[cb] = (uint8_t)sc;
    if (cb == bpr - 1)                        // the owner of the row's last block pads the row to whole dwords
      for (int c = bpr; c < ew; ++c) er[c] = (uint8_t)kE8M0One;
  }
}

std::vector<at::Tensor> mxfp8_quant(const at::Tensor& x) {
  PCMP_CHECK_CUDA(x);
  PCMP_CHECK_CONTIG(x);
  TORCH_CHECK(x.dim() == 2, "mxfp8_quant: x must be [R, K]");
  const int64_t R = x.size(0), K = x.size(1);
  TORCH_CHECK(K > 0 && K % 32 == 0 && R * K < (1ll << 31), "mxfp8_quant: K must be a multiple of 32 (got ", K, ")");
  const int64_t ew = 4 * ((K + 127) / 128);
  at::Tensor q = torch::empty({R, K}, x.options().dtype(at::kFloat8_e4m3fn));
  at::Tensor e = torch::empty({R, ew}, x.options().dtype(at::kByte));
  if (R == 0) return {q, e};
  const int nblk = (int)(R * K / 32);
  const dim3 grid(ceil_div(nblk, 64)), block(256);
  if (x.scalar_type() == at::kBFloat16)
    hipLaunchKernelGGL(mxfp8_quant_kernel<__bf16>, grid, block, 0, cur_stream(), ptr<const __bf16>(x), ptr<uint8_t>(q),
                       ptr<uint8_t>(e), nblk, (int)(K / 32), (int)ew);
  else if (x.scalar_type() == at::kFloat)
    hipLaunchKernelGGL(mxfp8_quant_kernel<float>, grid, block, 0, cur_stream(), ptr<const float>(x), ptr<uint8_t>(q),
                       ptr<uint8_t>(e), nblk, (int)(K / 32), (int)ew);
  else TORCH_CHECK(false, "mxfp8_quant: x must be bf16 or fp32");
  PCMP_LAUNCH_CHECK();
  return {q, e};
}

// ------------------------------------------------------------------------------------------------
// fp32 epilogue of the WGRAD variant (wave (wr, wc) of 2 x 2, lane = row fr, channels 4g .. 4g+3 of every 16x16
// tile; N % 4 == 0).  One split: yf = (accum ? yf : 0) + acc.  Several: the bare partial goes to slab `split` of
// the workspace and the reduce applies accum.
template <int BM, int BN>
__device__ __forceinline__ void mx_tile_store_f32(const MxParams& p, const f32x4 (&acc)[BN / 32][BM / 32], int m0, int n0, int wr,
                                                  int wc, int fr, int g, int split) {
  constexpr int WTM = BM / 2, WTN = BN / 2, TM = WTM / 16, TN = WTN / 16;
  const bool part = p.ns > 1;
  float* dst = part ? p.ws + (size_t)split * p.M * p.N : p.yf;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = m0 + wr * WTM + i * 16 + fr;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + wc * WTN + j * 16 + 4 * g;
      if (n >= p.N) continue;
      f32x4* o = reinterpret_cast<f32x4*>(dst + (size_t)m * p.N + n);
      *o = !part && p.accum ? *o + acc[j][i] : acc[j][i];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Tiled GEMM, M > 16.  4 waves as 2 x 2; the MFMA runs W x X, so a lane ends with four consecutive channels
// 4g .. 4g+3 of output row fr per 16x16 tile.  LDS stage: [A tile BM x 128][B tile BN x 128][scale dwords of
// the BM A rows, then of the BN B rows].  Wave w moves the scale dwords of rows 64w .. 64w+63 of that list
// (one 4-byte LDS-DMA, lane = row; rows past the operand and K-steps past the row read as zero, next to
// operand bytes that are zero too).
// WGRAD: the weight-gradient variant.  The reduction (the tokens) is long and the output small, so blockIdx.y
// splits the K-steps: split s runs steps s * kper .. min(nk, (s + 1) * kper) - 1 and stores its fp32 tile to
// yf (ns == 1, overwrite or accumulate) or to slab s of the workspace, which mxfp8_wgrad_reduce_kernel sums.
template <int BM, int BN, bool OUT_MX, bool WGRAD = false>
__global__ void __launch_bounds__(256, 2) mxfp8_gemm_kernel(const MxParams p) {
  constexpr int WTM = BM / 2, WTN = BN / 2, TM = WTM / 16, TN = WTN / 16;
  constexpr int KB = 128;
  constexpr int A_BYTES = BM * KB, T_BYTES = (BM + BN) * KB, STAGE = T_BYTES + (BM + BN) * 4;
  constexpr int NA = BM / 8 / 4, NB = BN / 8 / 4;
  static_assert(NA >= 1 && NB >= 1 && TM >= 1 && TN >= 1 && TN % 2 == 0 && BM % 64 == 0 && BN % 64 == 0, "mxfp8 tile");
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
    const bool live = k0 + gch * 16 < K;   // K tail: this lane's chunk lies inside the row
#pragma unroll
    for (int i = 0; i < NA; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(smem + s * STAGE + (wid * NA + i) * 1024), 16,
                                               (int)(live && a_vo[i] != kOOB ? a_vo[i] + k0 : kOOB), 0, 0, 0);
#pragma unroll
    for (int i = 0; i < NB; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(smem + s * STAGE + A_BYTES + (wid * NB + i) * 1024), 16,
                                               (int)(live && b_vo[i] != kOOB ? b_vo[i] + k0 : kOOB), 0, 0, 0);
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
  const int t0 = WGRAD ? (int)blockIdx.y * p.kper : 0, t1 = WGRAD ? min(nk, t0 + p.kper) : nk;
  issue(0, t0);
  for (int t = t0; t < t1; ++t) {
    const int s = (t - t0) & 1;
    // stage t has landed (this wave's DMA, then everyone's); every wave is past its reads of the other stage
    wait_vm_b<0>();
    lds_sync();
    if (t + 1 < t1) issue(s ^ 1, t + 1);
    const char* sA = smem + s * STAGE;
    const char* sB = sA + A_BYTES;
    const unsigned* sEA = reinterpret_cast<const unsigned*>(sA + T_BYTES);
    const unsigned* sEB = sEA + BM;
    i32x8 fa[TM], fb[TN];
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
      const i32x4 lo = *reinterpret_cast<const i32x4*>(sB + rr_off(row, g));
      const i32x4 hi = *reinterpret_cast<const i32x4*>(sB + rr_off(row, 4 + g));
      fb[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      eb[j] = (int)__builtin_amdgcn_ubfe(sEB[row], 8 * g, 8);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int i = 0; i < TM; ++i)   // fp8 x fp8; byte 0 of lane (fr, g)'s scale register scales block g of row fr
        acc[j][i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[j], fa[i], acc[j][i], 0, 0, 0, eb[j], 0, ea[i]);
  }
  if constexpr (WGRAD) mx_tile_store_f32<BM, BN>(p, acc, m0, n0, wr, wc, fr, g, (int)blockIdx.y);
  else mx_tile_epilogue<BM, BN, OUT_MX>(p, acc, m0, n0, wr, wc, fr, g);
}

// ------------------------------------------------------------------------------------------------
// Skinny GEMM, M <= 16.  Block = 64 output channels x one K split; wave w owns channels 16w .. 16w+15.  LDS:
// the x rows of the split (16 rows, zero beyond M and beyond K, 16-byte row pad), then their scale dwords
// (16 rows x kper / 128, unit scales where there is no data).  Per 256-byte step a lane issues four 16-byte
// loads of its weight row (two 128-byte K-steps; lane group g owns chunks g and 4+g of each, so the four groups
// of a row cover 64 contiguous bytes per load) and two byte loads of its scales (block g of each K-step), then
// feeds two scaled MFMAs.
constexpr int kMxSkinnyStep = 256;
__global__ void __launch_bounds__(256) mxfp8_skinny_kernel(const MxParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int M = p.M, N = p.N, K = p.K;
  const int cg = blockIdx.x % p.tiles_n, split = blockIdx.x / p.tiles_n;
  const int kb = split * p.kper;                                            // multiple of 256
  const int klen = min(K - kb, p.kper);                                     // bytes of this split, multiple of 32
  const int kpad = (klen + kMxSkinnyStep - 1) / kMxSkinnyStep * kMxSkinnyStep;   // <= p.kper
  const int rs = p.kper + 16;                                               // LDS row stride of x
  const int cpr = kpad >> 4;                                                // 16-byte chunks per LDS row
  const int dpr = p.kper >> 7;                                              // scale dwords per LDS row
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
  const uint8_t* wrow = p.w + (size_t)(nok ? nrow : 0) * K + kb;
  const uint8_t* erow = p.ew + (size_t)(nok ? nrow : 0) * p.eb + (kb >> 5);
  const char* xrow = smem + fr * rs;
  const uint8_t* xe = reinterpret_cast<const uint8_t*>(sE + fr * dpr);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < kpad; k0 += kMxSkinnyStep) {
    i32x4 fw[2][2];
    int sw[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int kk = k0 + 128 * u + 16 * g, kb32 = k0 + 128 * u + 32 * g;   // klen % 32 == 0: chunks and blocks are whole
      fw[u][0] = nok && kk < klen ? *reinterpret_cast<const i32x4*>(wrow + kk) : i32x4{0, 0, 0, 0};
      fw[u][1] = nok && kk + 64 < klen ? *reinterpret_cast<const i32x4*>(wrow + kk + 64) : i32x4{0, 0, 0, 0};
      sw[u] = nok && kb32 < klen ? (int)erow[kb32 >> 5] : (int)kE8M0One;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int kk = k0 + 128 * u + 16 * g;
      const i32x4 lo = *reinterpret_cast<const i32x4*>(xrow + kk), hi = *reinterpret_cast<const i32x4*>(xrow + kk + 64);
      const i32x8 fx = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      const i32x8 fwu = __builtin_shufflevector(fw[u][0], fw[u][1], 0, 1, 2, 3, 4, 5, 6, 7);
      acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fwu, fx, acc, 0, 0, 0, sw[u], 0, (int)xe[(k0 >> 5) + 4 * u + g]);
    }
  }
  // lane holds row m = fr, channels n .. n+3
  const int m = fr, n = cg * 64 + wid * 16 + 4 * g;
  if (m >= M || n >= N) return;
  if (p.ns == 1) mx_store4(p, m, n, acc);
  else *reinterpret_cast<f32x4*>(p.ws + ((size_t)split * M + m) * N + n) = acc;
}

// split-K reduce + epilogue: one thread per four channels, partials summed in split order
__global__ void __launch_bounds__(256) mxfp8_skinny_reduce_kernel(const MxParams p) {
  const int n4 = p.N >> 2;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.M * n4) return;
  const int m = idx / n4, n = (idx - m * n4) * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < p.ns; ++s) acc += *reinterpret_cast<const f32x4*>(p.ws + ((size_t)s * p.M + m) * p.N + n);
  mx_store4(p, m, n, acc);
}

static void launch_mx_skinny(MxParams& p, const at::Tensor& like) {
  skinny_split_plan(p.N, p.K, kMxSkinnyStep, p.kper, p.ns);
  p.tiles_n = ceil_div(p.N, 64);
  at::Tensor ws;
  if (p.ns > 1) {
    ws = torch::empty({p.ns, p.M, p.N}, like.options().dtype(at::kFloat));
    p.ws = ptr<float>(ws);
  }
  const size_t smem = (size_t)16 * (p.kper + 16) + (size_t)16 * (p.kper / 128) * 4;
  launch_lds<mxfp8_skinny_kernel>(dim3(p.tiles_n * p.ns), dim3(256), smem, cur_stream(), p);
  if (p.ns > 1) {
    hipLaunchKernelGGL(mxfp8_skinny_reduce_kernel, dim3(ceil_div((int64_t)p.M * (p.N / 4), 256)), dim3(256), 0, cur_stream(), p);
    PCMP_LAUNCH_CHECK();
  }
}

template <int BM, int BN>
static void launch_mx_tiled(MxParams& p, bool out_mx) {
  p.tiles_m = ceil_div(p.M, BM);
  p.tiles_n = ceil_div(p.N, BN);
  const dim3 grid(p.tiles_m * p.tiles_n), block(256);
  const size_t smem = (size_t)2 * (BM + BN) * (128 + 4);
  if (out_mx) launch_lds<mxfp8_gemm_kernel<BM, BN, true>>(grid, block, smem, cur_stream(), p);
  else launch_lds<mxfp8_gemm_kernel<BM, BN, false>>(grid, block, smem, cur_stream(), p);
}

std::vector<at::Tensor> linear_mxfp8_fwd(const at::Tensor& xq, const at::Tensor& ex, const at::Tensor& wq, const at::Tensor& ew,
                                         const c10::optional<at::Tensor>& bias, int64_t act, bool out_mx) {
  fp8_gemm_checks("linear_mxfp8_fwd", xq, wq, bias, 32, act);
  const int64_t M = xq.size(0), K = xq.size(1), N = wq.size(0);
  const int64_t ewb = 4 * ((K + 127) / 128), ewn = 4 * ((N + 127) / 128);
  TORCH_CHECK(ex.is_cuda() && ew.is_cuda() && ex.is_contiguous() && ew.is_contiguous() && ex.scalar_type() == at::kByte &&
                  ew.scalar_type() == at::kByte && ex.dim() == 2 && ew.dim() == 2 && ex.size(0) == M && ew.size(0) == N &&
                  ex.size(1) == ewb && ew.size(1) == ewb,
              "linear_mxfp8_fwd: ex [M, ", ewb, "], ew [N, ", ewb, "] uint8");
  TORCH_CHECK(!out_mx || (M > 16 && N % 32 == 0), "linear_mxfp8_fwd: out_mx needs M > 16 and N % 32 == 0 (got M = ", M,
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
  p.w = ptr<const uint8_t>(wq);
  p.ex = ptr<const uint8_t>(ex);
  p.ew = ptr<const uint8_t>(ew);
  p.bias = optr<const float>(bias);
  p.M = (int)M, p.N = (int)N, p.K = (int)K, p.act = (int)act;
  p.eb = (int)ewb, p.ebn = (int)ewn;
  p.ns = 1;
  if (M <= 16) {
    launch_mx_skinny(p, xq);
    return out;
  }
  // automatic = 64x64, the convention of the fp8 mode (fp8_tile = 128 forces the 128x128 tile)
  if (fp8_forced_tile() == 128) launch_mx_tiled<128, 128>(p, out_mx);
  else launch_mx_tiled<64, 64>(p, out_mx);
  return out;
}

// ------------------------------------------------------------------------------------------------
// WGRAD of the mxfp8 training mode: out [N, K] fp32 = (acc ? out : 0) + dy^T x on the transposed images
// (mxfp8_train.hip: mxfp8_quant_both), whose blocks run along the tokens.  In the kernel's terms M = N_out,
// N = K_out and the reduction K = the tokens.
//
// Split rule, static in (tiles, K-steps): floor(256 / tiles) splits -- the grid grows only while it still fits the
// 256 CUs once -- and no split shorter than 4 K-steps (512 tokens).  Measured (docs/PERF_NOTES.md, 1 / 2 / 4 / 8
// splits at 4096 tokens): with 144 tiles (768 x 768, 64x64 tiles) splitting is a wash at best, with 432 tiles and
// more every split loses to the partial stores and the reduce launch, so BERT-base's shapes all run unsplit; small
// outputs (256 x 256: 16 tiles) are where the splits pay.
// Partials are summed in split order by one thread per four outputs: two runs are bitwise equal.
static Knob kn_mxfp8_wgrad_ns("mxfp8_wgrad_ns", 0);   // splits of linear_mxfp8_wgrad; 0: the rule

__global__ void __launch_bounds__(256) mxfp8_wgrad_reduce_kernel(const MxParams p) {
  const size_t mn = (size_t)p.M * p.N, i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= mn) return;
  f32x4 s = *reinterpret_cast<const f32x4*>(p.ws + i);
  for (int sp = 1; sp < p.ns; ++sp) s += *reinterpret_cast<const f32x4*>(p.ws + sp * mn + i);
  f32x4* o = reinterpret_cast<f32x4*>(p.yf + i);
  *o = p.accum ? *o + s : s;
}

template <int BM, int BN>
static void launch_mx_wgrad(MxParams& p, const at::Tensor& like) {
  p.tiles_m = ceil_div(p.M, BM);
  p.tiles_n = ceil_div(p.N, BN);
  const int tiles = p.tiles_m * p.tiles_n, nk = ceil_div(p.K, 128);
  int ns = kn_mxfp8_wgrad_ns.get();
  if (ns <= 0) ns = std::min(256 / tiles, nk / 4);
  p.kper = ceil_div(nk, std::max(1, std::min(ns, nk)));
  p.ns = ceil_div(nk, p.kper);                              // every split owns at least one K-step
  at::Tensor ws;
  if (p.ns > 1) {
    ws = torch::empty({p.ns, p.M, p.N}, like.options().dtype(at::kFloat));
    p.ws = ptr<float>(ws);
  }
  launch_lds<mxfp8_gemm_kernel<BM, BN, false, true>>(dim3(tiles, p.ns), dim3(256), (size_t)2 * (BM + BN) * (128 + 4), cur_stream(), p);
  if (p.ns > 1) {
    hipLaunchKernelGGL(mxfp8_wgrad_reduce_kernel, dim3(ceil_div((int64_t)p.M * p.N / 4, 256)), dim3(256), 0, cur_stream(), p);
    PCMP_LAUNCH_CHECK();
  }
}

void linear_mxfp8_wgrad(const at::Tensor& dytq, const at::Tensor& edyt, const at::Tensor& xtq, const at::Tensor& ext, at::Tensor out,
                        bool acc) {
  fp8_gemm_checks("linear_mxfp8_wgrad", dytq, xtq, c10::nullopt, 32, 0);
  const int64_t N = dytq.size(0), M = dytq.size(1), K = xtq.size(0), eb = 4 * ((M + 127) / 128);
  TORCH_CHECK(edyt.is_cuda() && ext.is_cuda() && edyt.is_contiguous() && ext.is_contiguous() && edyt.scalar_type() == at::kByte &&
                  ext.scalar_type() == at::kByte && edyt.dim() == 2 && ext.dim() == 2 && edyt.size(0) == N && ext.size(0) == K &&
                  edyt.size(1) == eb && ext.size(1) == eb,
              "linear_mxfp8_wgrad: edyt [N, ", eb, "], ext [K, ", eb, "] uint8");
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.scalar_type() == at::kFloat && out.dim() == 2 && out.size(0) == N &&
                  out.size(1) == K, "linear_mxfp8_wgrad: out must be contiguous fp32 [N, K]");
  if (N == 0 || K == 0) return;
  MxParams p{};
  p.x = ptr<const uint8_t>(dytq);
  p.w = ptr<const uint8_t>(xtq);
  p.ex = ptr<const uint8_t>(edyt);
  p.ew = ptr<const uint8_t>(ext);
  p.yf = ptr<float>(out);
  p.accum = acc ? 1 : 0;
  p.M = (int)N, p.N = (int)K, p.K = (int)M;
  p.eb = (int)eb;
  if (fp8_forced_tile() == 128) launch_mx_wgrad<128, 128>(p, dytq);
  else launch_mx_wgrad<64, 64>(p, dytq);
}

}  // namespace pcmp

TORCH_LIBRARY_FRAGMENT(pcmp, m) {
  m.def("mxfp8_quant(Tensor x) -> Tensor[]", &pcmp::mxfp8_quant);
  m.def("linear_mxfp8_fwd(Tensor xq, Tensor ex, Tensor wq, Tensor ew, Tensor? bias, int act, bool out_mx) -> Tensor[]",
        &pcmp::linear_mxfp8_fwd);
  m.def("linear_mxfp8_wgrad(Tensor dytq, Tensor edyt, Tensor xtq, Tensor ext, Tensor(a!) out, bool acc) -> ()",
        &pcmp::linear_mxfp8_wgrad);
}
