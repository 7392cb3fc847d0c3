// MXFP8 inference convolutions: NHWC implicit GEMM on the gfx950 block-scaled MFMA, chained.
//
//   conv_mxfp8_fwd(xq [N,H,W,C], ex, wq [Cout,R,S,C], ew, stride, pad, bias?, resid?, relu, out_bf16, out_mx, pool = 0)
//       -> [y bf16 [N,OH,OW,Cout]] and / or [yq e4m3 [N,OH,OW,Cout], ye [N*OH*OW, 4*ceil(Cout/128)]], in that order
//          (pool = 2: MaxPool2d(2, 2) of the activated value, the outputs over [N, OH/2, OW/2]; no resid)
//       y[m,n] = act(sum_{tap, b} 2^(ex[pix(m,tap), b] + ew[n*R*S + tap, b] - 254) * sum_{c in b} xq * wq
//                    + bias[n] + resid[m,n])
//
// Contract (docs/PARITY.md "The mxfp8 inference conv mode").  Both operands are rows of C bytes with a
// dword-aligned E8M0 scale row, exactly what mxfp8_quant yields on the [N*H*W, C] activation view and on the
// [Cout*R*S, C] view of the weight: a 32-channel block of NHWC is a 32-block of the GEMM's K = tap x channel
// axis, and every (output channel, tap) is one row of an MX matrix whose scale dwords are aligned per tap.
// C % 32 == 0, Cout % 8 == 0 (% 32 for the pair).  A padding tap contributes exactly zero: its element chunks
// and its scale dword are sent out of range (zero bytes, scale byte 0 = 2^-127).  Sums run in fp32 in a fixed
// order; there is no split-K, no atomic and no cross-workgroup hand-off: two runs are bitwise equal.
//
// mxfp8_conv_kernel is mxfp8_gemm_kernel's tile and pipeline (256 threads as 2 x 2 waves, 64x64 or 128x128,
// LDS-DMA of 16-byte chunks into the rr_off image, two stages, one barrier per K-step, the stage's scale
// dwords behind the tile) with a gathered A operand:
//   * a K-step is (tap, 128-channel slab); the last slab of a tap may hold 32, 64 or 96 live bytes, whose dead
//     chunks are out of range on both operands.  A step never straddles taps, so the A scale dword of a tile
//     row is one aligned dword of one input pixel's scale row;
//   * every thread decodes the tile rows it stages, m -> (n, oh, ow), once before the K loop and keeps the
//     row's first input pixel and its (ih, iw) origin; per tap the pixel is origin + (r, s), valid when both
//     coordinates lie inside the image.  Validity is an explicit mask: a column left or right of the image
//     lands inside the buffer on a neighbouring row, so the buffer range check alone is no padding;
//   * the (tap, slab) of the step being issued is carried, not divided out, per step;
//   * lane (fr, g) supplies chunks g and 4+g of the 128-byte step and scale byte g (mxfp8.hip, header);
//   * epilogue per 16x16 tile: four consecutive channels of one output pixel per lane; the bf16 residual
//     joins the accumulator, then the shared bias + activation step; the bf16 store and / or the MX pair
//     (quad / xor 16 / xor 32 amax of the 32-channel block) come from the same fp32 values.
//
// The pooled variant (POOL) is the same K loop on window-major tile rows: row m is (pooled pixel m >> 2, window
// position m & 3), oh = 2 ph + (pos >> 1), ow = 2 pw + (pos & 1), M' = NB * (OH / 2) * (OW / 2) * 4.  The division
// floors: an odd last row or column of the conv output is never computed, as MaxPool2d(2, 2) drops it.  Only the
// row decode differs; masks, carried (tap, slab) and scale addressing work from the decoded (pix, ih, iw).  BM % 4
// == 0, so a window is the four lanes fr = 4q .. 4q+3 of one 16-lane group and never straddles tiles or waves.
// Epilogue: bias + activation per lane, then the window max by two quad exchanges (DPP xor 1, xor 2), after which
// the four lanes of a quad hold the same pooled values for every tile column j.  The stores are spread over the
// quad: lane pos packs (or quantises) every column, keeps column j = pos and stores it, so a wave issues one
// full-width store per 16 rows where one lane per quad would issue TN quarter-width ones (at 64x64, TN = 2, lanes
// pos 2 and 3 sit out); the scale byte of block jp is written by lane pos = jp of group g = 0.  The block amax is
// the unpooled epilogue's exchange on the pooled values.  Nothing crosses a workgroup: runs stay bitwise equal.
#include "mx_common.h"

namespace pcmp {

struct MxConvParams {
  MxParams g;            // x [NB*H*W][C], w [Cout*R*S][C]; M = NB*OH*OW, N = Cout, K = C; act 0 / 1
  const __bf16* resid;   // [M][Cout] or null
  int NB, H, W, OH, OW, R, S, stride, pad;
  int PH, PW;            // pooled extent OH / 2, OW / 2 (POOL; then M = NB*PH*PW*4, window-major)
};

constexpr int kNoRow = -0x40000000;   // ih origin of a tile row past M: no tap is ever valid

// residual (four bf16 of this lane's pixel), then bias + activation
__device__ __forceinline__ void mx_conv_epi4(const MxConvParams& q, int m, int n, f32x4 acc, float (&v)[4]) {
  if (q.resid) {
    const uint2 r = *reinterpret_cast<const uint2*>(q.resid + (size_t)m * q.g.N + n);
    acc[0] += __uint_as_float(r.x << 16);
    acc[1] += __uint_as_float(r.x & 0xffff0000u);
    acc[2] += __uint_as_float(r.y << 16);
    acc[3] += __uint_as_float(r.y & 0xffff0000u);
  }
  mx_bias_act(q.g, n, acc, v);
}
__device__ __forceinline__ void mx_conv_store_bf16(const MxParams& p, int m, int n, const float (&v)[4]) {
  *reinterpret_cast<uint2*>(p.y + (size_t)m * p.N + n) = uint2{f2bf2(v[0], v[1]), f2bf2(v[2], v[3])};
}

// OUT: 1 bf16 result, 2 the MX pair, 3 both.  POOL: 2x2 / stride-2 max-pool of the activated value (header)
template <int BM, int BN, int OUT, bool POOL>
__global__ void __launch_bounds__(256, 2) mxfp8_conv_kernel(const MxConvParams q) {
  constexpr int WTM = BM / 2, WTN = BN / 2, TM = WTM / 16, TN = WTN / 16;
  constexpr int KB = 128;
  constexpr int A_BYTES = BM * KB, T_BYTES = (BM + BN) * KB, STAGE = T_BYTES + (BM + BN) * 4;
  constexpr int NA = BM / 8 / 4, NB = BN / 8 / 4;
  static_assert(NA >= 1 && NB >= 1 && TM >= 1 && TN >= 1 && TN % 2 == 0 && BM % 64 == 0 && BN % 64 == 0, "mxfp8 tile");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const MxParams& p = q.g;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int M = p.M, N = p.N, C = p.K;
  const int H = q.H, W = q.W, S = q.S;
  const int taps = q.R * S, slabs = (C + KB - 1) / KB, nk = taps * slabs;
  const int HW = H * W, OHW = q.OH * q.OW;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_m = lin / p.tiles_n, tile_n = lin - tile_m * p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const __amdgpu_buffer_rsrc_t rsA = make_rsrc(p.x, (unsigned)((size_t)q.NB * HW * C)),
                               rsB = make_rsrc(p.w, (unsigned)((size_t)N * taps * C));
  // tile row m -> its first input pixel (tap (0, 0); may lie outside the image) and that pixel's (ih, iw)
  auto decode = [&](int m, int& pix, int& ih, int& iw) {
    if (m >= M) {
      pix = 0, ih = kNoRow, iw = 0;
      return;
    }
    int n, oh, ow;
    if constexpr (POOL) {   // window-major: four rows per pooled pixel
      const int w = m >> 2, pos = m & 3, PHW = q.PH * q.PW;
      n = w / PHW;
      const int rem = w - n * PHW, ph = rem / q.PW;
      oh = 2 * ph + (pos >> 1), ow = 2 * (rem - ph * q.PW) + (pos & 1);
    } else {
      n = m / OHW;
      const int rem = m - n * OHW;
      oh = rem / q.OW, ow = rem - oh * q.OW;
    }
    ih = oh * q.stride - q.pad;
    iw = ow * q.stride - q.pad;
    pix = n * HW + ih * W + iw;
  };
  const int gch = (lane & 7) ^ (lane >> 3);
  int a_pix[NA], a_ih[NA], a_iw[NA];
  unsigned b_vo[NB];
#pragma unroll
  for (int i = 0; i < NA; ++i) decode(m0 + (wid * NA + i) * 8 + (lane >> 3), a_pix[i], a_ih[i], a_iw[i]);
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int n = n0 + (wid * NB + i) * 8 + (lane >> 3);
    b_vo[i] = n < N ? (unsigned)((size_t)n * taps * C + gch * 16) : kOOB;
  }
  // scale dwords: this wave's 64 rows of the (A rows, B rows) list all belong to one operand; lane = row
  constexpr bool kScaleWave4 = (BM + BN) / 64 >= 4;          // 128x128: every wave; 64x64: waves 0 and 1
  const int uwid = __builtin_amdgcn_readfirstlane(wid);
  const bool sc_wave = kScaleWave4 || uwid < (BM + BN) / 64;
  const bool sc_is_a = uwid * 64 < BM;
  const __amdgpu_buffer_rsrc_t rsE = sc_is_a ? make_rsrc(p.ex, (unsigned)((size_t)q.NB * HW * p.eb))
                                             : make_rsrc(p.ew, (unsigned)((size_t)N * taps * p.eb));
  int e_pix = 0, e_ih = kNoRow, e_iw = 0;
  unsigned e_vo = kOOB;
  if (sc_is_a) decode(m0 + wid * 64 + lane, e_pix, e_ih, e_iw);
  else {
    const int n = n0 + wid * 64 - BM + lane;
    if (n < N) e_vo = (unsigned)((size_t)n * taps * p.eb);
  }
  // the K-step being issued: tap (i_r, i_s), slab i_slab; steps are issued in order
  int i_r = 0, i_s = 0, i_slab = 0;
  auto issue = [&](int s) {
    const int c0 = i_slab * KB;
    const bool live = c0 + gch * 16 < C;   // slab tail: this lane's chunk lies inside the pixel's channels
    const int dpix = i_r * W + i_s, wtap = i_r * S + i_s;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const bool ok = live && (unsigned)(a_ih[i] + i_r) < (unsigned)H && (unsigned)(a_iw[i] + i_s) < (unsigned)W;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(smem + s * STAGE + (wid * NA + i) * 1024), 16,
                                               (int)(ok ? (unsigned)((a_pix[i] + dpix) * C + c0 + gch * 16) : kOOB), 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(smem + s * STAGE + A_BYTES + (wid * NB + i) * 1024), 16,
                                               (int)(live && b_vo[i] != kOOB ? b_vo[i] + (unsigned)(wtap * C + c0) : kOOB), 0, 0, 0);
    if (sc_wave) {   // wave-uniform
      unsigned vo;
      if (sc_is_a) {
        const bool ok = (unsigned)(e_ih + i_r) < (unsigned)H && (unsigned)(e_iw + i_s) < (unsigned)W;
        vo = ok ? (unsigned)((e_pix + dpix) * p.eb + 4 * i_slab) : kOOB;
      } else {
        vo = e_vo != kOOB ? e_vo + (unsigned)(wtap * p.eb + 4 * i_slab) : kOOB;
      }
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsE, (__attribute__((address_space(3))) void*)(smem + s * STAGE + T_BYTES + wid * 256), 4,
                                               (int)vo, 0, 0, 0);
    }
    if (++i_slab == slabs) {
      i_slab = 0;
      if (++i_s == S) i_s = 0, ++i_r;
    }
  };
  f32x4 acc[TN][TM];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int i = 0; i < TM; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, g = lane >> 4;
  issue(0);
  for (int t = 0; t < nk; ++t) {
    const int s = t & 1;
    // stage t has landed (this wave's DMA, then everyone's); every wave is past its reads of the other stage
    wait_vm_b<0>();
    lds_sync();
    if (t + 1 < nk) issue(s ^ 1);
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
      for (int i = 0; i < TM; ++i)   // W x X: a lane ends with four consecutive channels of one output pixel
        acc[j][i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[j], fa[i], acc[j][i], 0, 0, 0, eb[j], 0, ea[i]);
  }
  // epilogue: lane holds pixel m = .. + fr, channels n = .. + 4g .. 4g+3 of every 16x16 tile
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = m0 + wr * WTM + i * 16 + fr;
    if constexpr (POOL) {
      // every lane runs the exchanges; the lanes of a quad share the window (so m < M) and the channels (so n < N)
      const int pos = fr & 3;
      const size_t w = (size_t)(m >> 2);
      const int nq = n0 + wc * WTN + pos * 16 + 4 * g;   // the tile column this lane stores: j = pos
      const bool st = m < M && pos < TN && nq < N;       // M % 4 == 0: a window is in range or out as a whole
      float v[TN][4];
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + wc * WTN + j * 16 + 4 * g;
        if (n < N) mx_conv_epi4(q, m, n, acc[j][i], v[j]);   // resid is null: m is not read
        else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[j][e] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[j][e] = fmaxf(v[j][e], dpp_mov<0xB1>(v[j][e]));    // quad_perm(1,0,3,2)
          v[j][e] = fmaxf(v[j][e], dpp_mov<0x4E>(v[j][e]));    // quad_perm(2,3,0,1)
        }
      }
      if constexpr ((OUT & 1) != 0) {
        uint2 pk{0u, 0u};
#pragma unroll
        for (int j = 0; j < TN; ++j)
          if (pos == j) pk = uint2{f2bf2(v[j][0], v[j][1]), f2bf2(v[j][2], v[j][3])};
        if (st) *reinterpret_cast<uint2*>(p.y + w * N + nq) = pk;
      }
      if constexpr ((OUT & 2) != 0) {
        unsigned qd = 0u, sc_q = 0u;   // this lane's column, quantised; the scale of block jp = pos
#pragma unroll
        for (int jp = 0; jp < TN / 2; ++jp) {
          float amax = 0.f;
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fabsf(v[2 * jp + h][e]));
          amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
          amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
          const unsigned sc = mx_scale_of(amax);
          const float r = mx_inv_scale(sc);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const unsigned d = quant4(v[2 * jp + h][0], v[2 * jp + h][1], v[2 * jp + h][2], v[2 * jp + h][3], r);
            if (pos == 2 * jp + h) qd = d;
          }
          if (pos == jp) sc_q = sc;
        }
        if (st) *reinterpret_cast<unsigned*>(p.yq + w * N + nq) = qd;
        const int nb0 = n0 + wc * WTN + pos * 32;
        if (g == 0 && m < M && pos < TN / 2 && nb0 < N) {
          uint8_t* er = p.ye + w * p.ebn;
          const int cb = nb0 >> 5;
          er[cb] = (uint8_t)sc_q;
          if (nb0 + 32 == N)                   // the pixel's last block: pad the scale row to whole dwords
            for (int c = cb + 1; c < p.ebn; ++c) er[c] = (uint8_t)kE8M0One;
        }
      }
    } else if constexpr (OUT == 1) {
      if (m >= M) continue;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + wc * WTN + j * 16 + 4 * g;
        if (n >= N) continue;   // N % 8 == 0: all four channels are in range or none
        float v[4];
        mx_conv_epi4(q, m, n, acc[j][i], v);
        mx_conv_store_bf16(p, m, n, v);
      }
    } else {
      // a 32-channel block is the tile pair (2jp, 2jp+1) times the four lane groups of pixel fr (N % 32 == 0:
      // a block is in range or out as a whole; the lanes that exchange values share m and the block)
#pragma unroll
      for (int jp = 0; jp < TN / 2; ++jp) {
        const int nb0 = n0 + wc * WTN + jp * 32;
        const bool ok = m < M && nb0 < N;
        float v[2][4];
        float amax = 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int n = nb0 + h * 16 + 4 * g;
          if (ok) {
            mx_conv_epi4(q, m, n, acc[2 * jp + h][i], v[h]);
            if constexpr (OUT == 3) mx_conv_store_bf16(p, m, n, v[h]);
          } else {
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
          if (nb0 + 32 == N)                   // the pixel's last block: pad the scale row to whole dwords
            for (int c = cb + 1; c < p.ebn; ++c) er[c] = (uint8_t)kE8M0One;
        }
      }
    }
  }
}

template <int BM, int BN, bool POOL>
static void launch_mx_conv(MxConvParams& q, int out) {
  q.g.tiles_m = ceil_div(q.g.M, BM);
  q.g.tiles_n = ceil_div(q.g.N, BN);
  const dim3 grid(q.g.tiles_m * q.g.tiles_n), block(256);
  const size_t smem = (size_t)2 * (BM + BN) * (128 + 4);
  if (out == 1) launch_lds<mxfp8_conv_kernel<BM, BN, 1, POOL>>(grid, block, smem, cur_stream(), q);
  else if (out == 2) launch_lds<mxfp8_conv_kernel<BM, BN, 2, POOL>>(grid, block, smem, cur_stream(), q);
  else launch_lds<mxfp8_conv_kernel<BM, BN, 3, POOL>>(grid, block, smem, cur_stream(), q);
}

std::vector<at::Tensor> conv_mxfp8_fwd(const at::Tensor& xq, const at::Tensor& ex, const at::Tensor& wq, const at::Tensor& ew,
                                       int64_t stride, int64_t pad, const c10::optional<at::Tensor>& bias,
                                       const c10::optional<at::Tensor>& resid, bool relu, bool out_bf16, bool out_mx,
                                       int64_t pool) {
  const char* op = "conv_mxfp8_fwd";
  TORCH_CHECK(xq.is_cuda() && wq.is_cuda() && xq.is_contiguous() && wq.is_contiguous(), op, ": xq / wq must be contiguous GPU tensors");
  TORCH_CHECK(xq.scalar_type() == at::kFloat8_e4m3fn && wq.scalar_type() == at::kFloat8_e4m3fn, op,
              ": xq / wq must be float8_e4m3fn");
  TORCH_CHECK(xq.dim() == 4 && wq.dim() == 4 && xq.size(3) == wq.size(3), op, ": xq [N, H, W, C], wq [Cout, R, S, C]");
  TORCH_CHECK(out_bf16 || out_mx, op, ": at least one of out_bf16 / out_mx");
  const int64_t NB = xq.size(0), H = xq.size(1), W = xq.size(2), C = xq.size(3);
  const int64_t Co = wq.size(0), R = wq.size(1), S = wq.size(2);
  TORCH_CHECK(stride >= 1 && pad >= 0 && H + 2 * pad >= R && W + 2 * pad >= S, op, ": stride / pad / kernel extent");
  const int64_t OH = (H + 2 * pad - R) / stride + 1, OW = (W + 2 * pad - S) / stride + 1;
  TORCH_CHECK(pool == 0 || pool == 2, op, ": pool must be 0 or 2 (MaxPool2d(2, 2)); got ", pool);
  const bool has_resid = resid.has_value() && resid->defined();
  TORCH_CHECK(!pool || (OH >= 2 && OW >= 2 && !has_resid), op, ": pool needs OH >= 2, OW >= 2 and no resid");
  // the extent of the outputs, and the GEMM's rows: with pool, four window positions per pooled pixel
  const int64_t YH = pool ? OH / 2 : OH, YW = pool ? OW / 2 : OW;
  const int64_t M = NB * YH * YW * (pool ? 4 : 1), ewb = 4 * ((C + 127) / 128), ewn = 4 * ((Co + 127) / 128);
  TORCH_CHECK(C > 0 && C % 32 == 0 && Co % 8 == 0 && (!out_mx || Co % 32 == 0), op,
              ": C must be a multiple of 32 and Cout of 8 (of 32 with out_mx); got C = ", C, ", Cout = ", Co);
  TORCH_CHECK(NB * H * W * C < (1ll << 31) && Co * R * S * C < (1ll << 31) && M * Co * 2 < (1ll << 31), op, ": operand beyond 2 GiB");
  TORCH_CHECK(ex.is_cuda() && ew.is_cuda() && ex.is_contiguous() && ew.is_contiguous() && ex.scalar_type() == at::kByte &&
                  ew.scalar_type() == at::kByte && ex.dim() == 2 && ew.dim() == 2 && ex.size(0) == NB * H * W &&
                  ew.size(0) == Co * R * S && ex.size(1) == ewb && ew.size(1) == ewb,
              op, ": ex [N*H*W, ", ewb, "], ew [Cout*R*S, ", ewb, "] uint8");
  if (bias.has_value() && bias->defined())
    TORCH_CHECK(bias->is_cuda() && bias->scalar_type() == at::kFloat && bias->is_contiguous() && bias->numel() == Co, op,
                ": bias fp32 [Cout]");
  if (has_resid)
    TORCH_CHECK(resid->is_cuda() && resid->scalar_type() == at::kBFloat16 && resid->is_contiguous() && resid->numel() == M * Co,
                op, ": resid bf16 [N, OH, OW, Cout]");
  MxConvParams q{};
  MxParams& p = q.g;
  std::vector<at::Tensor> out;
  if (out_bf16) {
    out.push_back(torch::empty({NB, YH, YW, Co}, xq.options().dtype(at::kBFloat16)));
    p.y = ptr<__bf16>(out.back());
  }
  if (out_mx) {
    out.push_back(torch::empty({NB, YH, YW, Co}, xq.options()));
    p.yq = ptr<uint8_t>(out.back());
    out.push_back(torch::empty({NB * YH * YW, ewn}, ex.options()));
    p.ye = ptr<uint8_t>(out.back());
  }
  if (M == 0 || Co == 0) return out;
  p.x = ptr<const uint8_t>(xq);
  p.w = ptr<const uint8_t>(wq);
  p.ex = ptr<const uint8_t>(ex);
  p.ew = ptr<const uint8_t>(ew);
  p.bias = optr<const float>(bias);
  q.resid = optr<const __bf16>(resid);
  p.M = (int)M, p.N = (int)Co, p.K = (int)C, p.act = relu ? 1 : 0;
  p.eb = (int)ewb, p.ebn = (int)ewn;
  q.NB = (int)NB, q.H = (int)H, q.W = (int)W, q.OH = (int)OH, q.OW = (int)OW;
  q.R = (int)R, q.S = (int)S, q.stride = (int)stride, q.pad = (int)pad;
  q.PH = (int)YH, q.PW = (int)YW;
  const int mode = (out_bf16 ? 1 : 0) | (out_mx ? 2 : 0);
  // automatic = 64x64, the convention of the fp8 modes (fp8_tile = 128 forces the 128x128 tile)
  const bool big = fp8_forced_tile() == 128;
  if (pool) big ? launch_mx_conv<128, 128, true>(q, mode) : launch_mx_conv<64, 64, true>(q, mode);
  else big ? launch_mx_conv<128, 128, false>(q, mode) : launch_mx_conv<64, 64, false>(q, mode);
  return out;
}

}  // namespace pcmp

TORCH_LIBRARY_FRAGMENT(pcmp, m) {
  m.def("conv_mxfp8_fwd(Tensor xq, Tensor ex, Tensor wq, Tensor ew, int stride, int pad, Tensor? bias, Tensor? resid, "
        "bool relu, bool out_bf16, bool out_mx, int pool=0) -> Tensor[]",
        &pcmp::conv_mxfp8_fwd);
}
