// Split-bf16 fp32 matmul mode (knob f32_bf16x = 3 / 6): the fp32 implicit GEMM of igemm_f32_big_kernel
// with its matrix instruction replaced.  gfx950 has no xf32 MFMA and v_mfma_f32_32x32x2_f32 runs at
// 1/16 of the bf16 MFMA rate, so each fp32 operand element is written as a sum of PARTS bf16 parts
//
//   hi = bf16_rne(x),  mid = bf16_rne(x - hi),  lo = bf16_rne(x - hi - mid)        (PARTS == 3)
//
// (both subtractions are exact in fp32; three 8-bit significands with signed residuals hold all 24
// bits, so hi + mid + lo == x) and the product is formed on v_mfma_f32_32x32x16_bf16 from the part
// products (i, j) with i + j <= PARTS - 1 -- 6 at PARTS == 3 (what is dropped is below 2^-24 of the
// term), 3 at PARTS == 2 (2^-17 class) -- accumulated in fp32.  A part below a non-finite hi is 0, so
// an inf operand stays an inf instead of turning into inf - inf.
//
// Everything else is igemm_f32_big_kernel's: the GEMM views, the 32-deep K-steps, the per-thread tap
// walks and zero-padding buffer loads, the FWD input fold (applied before the split, to in-bounds rows
// only), the single LDS stage with two barriers per K-step, the split-K contract (p.raw) and the
// epilogue on the 32x32 accumulator (same lane map as the f32 MFMA), so splitk_epilogue_kernel /
// splitk_sum_kernel and the statistics rows are shared as they are.
//
// Split at staging time, once per element, in the thread that loaded it; LDS holds PARTS bf16 images
// per operand (64 B per row or column and part: 48 KB at 128x128, PARTS == 3):
//   * row-k operands (A of FWD / DGRAD, B of FWD: a thread holds 8 or 16 consecutive k of one row):
//     [row][32 k], 64-B rows of four 16-B chunks, chunk ^ ((row >> 2) & 3); the fragment of lane l is
//     one ds_read_b128: row l & 31, k 8 * (l >> 5) .. + 7 of a 16-deep slab.
//   * k-col operands (B of DGRAD, A and B of WGRAD arrive reduction-major: a thread holds 4 consecutive
//     columns of one k): wgrad32.h's transposed-read image [cols / 64][32 k][64 cols], 128-B rows with
//     the 16-B chunk ^ 4 * ((k >> 1) & 1), read with ds_read_b64_tr_b16 into the same lane map.
// Both paths give lane l the k order 8 * (l >> 5) + e, e = 0 .. 7, so A and B always agree.
// The part products of a 16-deep slab are added smallest first -- (2,0) (1,1) (0,2) (1,0) (0,1), summed
// from zero, then (0,0) onto the running sum, then the small sum -- in every instantiation: two runs
// are bitwise equal.
//
// Included by f32.hip inside namespace pcmp::f32, after igemm_f32_big_kernel (ConvP, GBK, bld4, ...).
#pragma once

constexpr int XIMG_ROW = 64;   // bytes of one row (row-k) or column (k-col) of one part image

// byte offset of 16-B chunk c (8 k) of a row in a row-k image
__device__ __forceinline__ int xrk_off(int row, int c) { return row * XIMG_ROW + ((c ^ ((row >> 2) & 3)) << 4); }
// byte offset of element (k, col) in a k-col image [cols / 64][32][64], col % 4 == 0
__device__ __forceinline__ int xkc_off(int k, int col) {
  return (col >> 6) * 4096 + k * 128 + ((((col & 63) >> 3) ^ (((k >> 1) & 1) << 2)) << 4) + ((col & 7) << 1);
}

// the bf16 parts of two fp32 values, packed (low half = a): out[i] = part i
template <int PARTS>
__device__ __forceinline__ void xsplit2(float a, float b, unsigned (&out)[PARTS]) {
#pragma unroll
  for (int i = 0; i < PARTS; ++i) {
    const unsigned u = f2bf2(a, b);
    out[i] = u;
    if (i + 1 < PARTS) {
      const float ha = __uint_as_float(u << 16), hb = __uint_as_float(u & 0xffff0000u);
      // exact in fp32; the parts below a non-finite hi are 0 (an inf stays an inf, a NaN a NaN) -- mid
      // is finite whenever hi is
      a = i > 0 || fabsf(ha) < __builtin_inff() ? a - ha : 0.f;
      b = i > 0 || fabsf(hb) < __builtin_inff() ? b - hb : 0.f;
    }
  }
}

template <int MODE, int BM, int BN, int PARTS>
__global__ __launch_bounds__(256, 2) void igemm_f32x_kernel(const ConvP p) {
  static_assert(GBK == 32, "igemm_f32x: 32-deep K-steps");
  static_assert(PARTS == 2 || PARTS == 3, "igemm_f32x: two or three bf16 parts");
  constexpr int WM = BM / 2, TM = WM / 32;
  constexpr int WN = BN / 2, TN = WN / 32;
  constexpr int BMV = BM * GBK / 1024, BNV = BN * GBK / 1024;   // float4s per thread of the A / B tile
  constexpr int KCT = 256 / GBK, KCS = 4 * KCT;                 // k-col role: threads per k row, column stride
  constexpr int A_IMG = BM * XIMG_ROW, B_IMG = BN * XIMG_ROW;   // bytes of one part image
  constexpr bool A_RK = MODE != F_WGRAD, B_RK = MODE == F_FWD;  // row-k operands; the others are k-col
  __shared__ __attribute__((aligned(16))) char As[PARTS * A_IMG];
  __shared__ __attribute__((aligned(16))) char Bs[PARTS * B_IMG];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1;
  const int tiles_mn = p.tiles_m * p.tiles_n;
  const int split = blockIdx.x / tiles_mn, tl = blockIdx.x - split * tiles_mn;
  const int tile_m = tl / p.tiles_n, tile_n = tl - (tl / p.tiles_n) * p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int kbeg = split * p.ksplit, kend = min(p.gk, kbeg + p.ksplit);
  const int nk = (kend - kbeg + GBK - 1) / GBK;
  const __amdgpu_buffer_rsrc_t rsA = f32_rsrc(p.a, p.a_bytes), rsB = f32_rsrc(p.b, p.b_bytes);

  // ---- operand loads: igemm_f32_big_kernel's loader roles and tap walks
  const int ra_row = tid % BM, ra_k = (tid / BM) * (4 * BMV);          // A row-k: 4 * BMV k
  const int rb_row = tid % BN, rb_k = (tid / BN) * (4 * BNV);          // B row-k: 4 * BNV k
  const int kc_k = tid / KCT, kc_c = (tid % KCT) * 4;                 // k-col: cols kc_c + KCS * h
  const int CIN = MODE == F_FWD ? p.C : p.K;
  struct Walk { int c, s, r; };
  auto walk_at = [&](int k) {
    Walk w;
    w.c = k % CIN;
    const int rs = k / CIN;
    w.s = rs % p.S;
    w.r = rs / p.S;
    return w;
  };
  auto walk_next = [&](Walk& w) {
    w.c += GBK;
    while (w.c >= CIN) {
      w.c -= CIN;
      if (++w.s == p.S) { w.s = 0; ++w.r; }
    }
  };
  Walk wa{0, 0, 0}, wbk{0, 0, 0};
  int a_n = 0, a_y = 0, a_x = 0;
  bool a_ok = false;
  if constexpr (MODE != F_WGRAD) {
    wa = walk_at(kbeg + ra_k);
    if constexpr (MODE == F_DGRAD) wbk = walk_at(kbeg + kc_k);
    const int m = m0 + ra_row;
    a_ok = m < p.gm;
    const int mm = a_ok ? m : 0;
    if constexpr (MODE == F_FWD) {
      a_n = mm / (p.P * p.Q);
      const int rem = mm - a_n * p.P * p.Q;
      const int pp = rem / p.Q, qq = rem - (rem / p.Q) * p.Q;
      a_y = pp * p.stride - p.pad;
      a_x = qq * p.stride - p.pad;
    } else {
      a_n = mm / (p.H * p.W);
      const int rem = mm - a_n * p.H * p.W;
      a_y = rem / p.W + p.pad;
      a_x = rem - (rem / p.W) * p.W + p.pad;
    }
  }
  int wb_y[BNV], wb_x[BNV], wb_c[BNV];
  if constexpr (MODE == F_WGRAD) {
#pragma unroll
    for (int h = 0; h < BNV; ++h) {
      const int j = n0 + kc_c + KCS * h;
      const int jj = j < p.gn ? j : 0;
      wb_c[h] = jj % p.C;
      const int rs = jj / p.C;
      wb_x[h] = rs % p.S - p.pad;
      wb_y[h] = j < p.gn ? rs / p.S - p.pad : -(1 << 20);
    }
  }

  float4 ra[BMV], rb[BNV];
  // input fold (FWD, p.isc): a wave's A chunk covers the same 4 * BMV channels for all its rows, so the
  // coefficients are scalar loads from a wave-uniform channel index -- issued at split time, not held
  // in registers across the MFMAs
  bool fold_ok = false;
  int fold_c = 0;
  auto load = [&](int k0) {
    if constexpr (MODE == F_FWD) {
      const int y = a_y + wa.r, x = a_x + wa.s;
      const bool kok = k0 + ra_k < kend;
      const bool ok = a_ok && kok && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
      const unsigned off = ok ? 4u * (unsigned)((((a_n * p.H + y) * p.W + x) * p.C) + wa.c) : F32_OOB;
#pragma unroll
      for (int h = 0; h < BMV; ++h) ra[h] = bld4(rsA, off + 16 * h);
      if (p.isc) {
        fold_ok = ok;
        fold_c = __builtin_amdgcn_readfirstlane(wa.c);
      }
      const int n = n0 + rb_row;
      const unsigned offb = n < p.gn && k0 + rb_k < kend ? 4u * (unsigned)(n * p.gk + k0 + rb_k) : F32_OOB;
#pragma unroll
      for (int h = 0; h < BNV; ++h) rb[h] = bld4(rsB, offb + 16 * h);
    } else if constexpr (MODE == F_DGRAD) {
      const int ph = a_y - wa.r, pw = a_x - wa.s;
      bool ok = a_ok && k0 + ra_k < kend && ph >= 0 && pw >= 0;
      int py = ph, px = pw;
      if (p.stride != 1) {
        ok = ok && (ph % p.stride) == 0 && (pw % p.stride) == 0;
        py = ph / p.stride;
        px = pw / p.stride;
      }
      ok = ok && py < p.P && px < p.Q;
      const unsigned off = ok ? 4u * (unsigned)((((a_n * p.P + py) * p.Q + px) * p.K) + wa.c) : F32_OOB;
#pragma unroll
      for (int h = 0; h < BMV; ++h) ra[h] = bld4(rsA, off + 16 * h);
      const bool kokb = k0 + kc_k < kend;
      const int wrow = ((wbk.c * p.R + wbk.r) * p.S + wbk.s) * p.C;
#pragma unroll
      for (int h = 0; h < BNV; ++h) {
        const int c = n0 + kc_c + KCS * h;
        rb[h] = bld4(rsB, kokb && c < p.gn ? 4u * (unsigned)(wrow + c) : F32_OOB);
      }
    } else {
      const int m = k0 + kc_k;
      const bool mok = m < kend;
#pragma unroll
      for (int h = 0; h < BMV; ++h) {
        const int co = m0 + kc_c + KCS * h;
        ra[h] = bld4(rsA, mok && co < p.gm ? 4u * (unsigned)(m * p.K + co) : F32_OOB);
      }
      const int mm = mok ? m : 0;
      const int n = mm / (p.P * p.Q);
      const int rem = mm - n * p.P * p.Q;
      const int pp = rem / p.Q, qq = rem - (rem / p.Q) * p.Q;
      const int y0 = pp * p.stride, x0 = qq * p.stride;
#pragma unroll
      for (int h = 0; h < BNV; ++h) {
        const int y = y0 + wb_y[h], x = x0 + wb_x[h];
        const bool okb = mok && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
        rb[h] = bld4(rsB, okb ? 4u * (unsigned)(((n * p.H + y) * p.W + x) * p.C + wb_c[h]) : F32_OOB);
      }
    }
    if constexpr (MODE != F_WGRAD) walk_next(wa);
    if constexpr (MODE == F_DGRAD) walk_next(wbk);
  };

  // ---- staging in two steps: split_parts() folds and splits the loaded K-step into packed bf16 pairs in
  // registers before the barrier that retires the stage's readers, stage() stores them after it
  unsigned qa[2 * BMV][PARTS], qb[2 * BNV][PARTS];   // [pair of consecutive elements][part]
  auto split_parts = [&]() {
    if (MODE == F_FWD && p.isc) {
#pragma unroll
      for (int h = 0; h < BMV; ++h) {
        const float4 sc = ld4(p.isc + fold_c + 4 * h), sh = ld4(p.ish + fold_c + 4 * h);
        float4& v = ra[h];
        v.x = fold_ok ? fmaxf(fmaf(v.x, sc.x, sh.x), 0.f) : 0.f;
        v.y = fold_ok ? fmaxf(fmaf(v.y, sc.y, sh.y), 0.f) : 0.f;
        v.z = fold_ok ? fmaxf(fmaf(v.z, sc.z, sh.z), 0.f) : 0.f;
        v.w = fold_ok ? fmaxf(fmaf(v.w, sc.w, sh.w), 0.f) : 0.f;
      }
    }
#pragma unroll
    for (int h = 0; h < BMV; ++h) {
      xsplit2<PARTS>(ra[h].x, ra[h].y, qa[2 * h]);
      xsplit2<PARTS>(ra[h].z, ra[h].w, qa[2 * h + 1]);
    }
#pragma unroll
    for (int h = 0; h < BNV; ++h) {
      xsplit2<PARTS>(rb[h].x, rb[h].y, qb[2 * h]);
      xsplit2<PARTS>(rb[h].z, rb[h].w, qb[2 * h + 1]);
    }
  };
  // row-k: V float4s = 4 * V consecutive k of one row -> V / 2 16-B chunks per part
  auto stage_rk = [&](char* img0, int img_bytes, const auto& q, int row, int k, auto nv) {
    constexpr int V = decltype(nv)::value;
#pragma unroll
    for (int h = 0; h < V; h += 2) {
      const int off = xrk_off(row, (k >> 3) + (h >> 1));
#pragma unroll
      for (int i = 0; i < PARTS; ++i)
        *reinterpret_cast<uint4*>(img0 + i * img_bytes + off) =
            make_uint4(q[2 * h][i], q[2 * h + 1][i], q[2 * h + 2][i], q[2 * h + 3][i]);
    }
  };
  // k-col: V float4s = 4 consecutive columns each of one k -> one 8-B store per float4 and part
  auto stage_kc = [&](char* img0, int img_bytes, const auto& q, auto nv) {
    constexpr int V = decltype(nv)::value;
#pragma unroll
    for (int h = 0; h < V; ++h) {
      const int off = xkc_off(kc_k, kc_c + KCS * h);
#pragma unroll
      for (int i = 0; i < PARTS; ++i)
        *reinterpret_cast<uint2*>(img0 + i * img_bytes + off) = make_uint2(q[2 * h][i], q[2 * h + 1][i]);
    }
  };
  using NA = std::integral_constant<int, BMV>;
  using NB = std::integral_constant<int, BNV>;
  auto stage = [&]() {
    if constexpr (A_RK) stage_rk(As, A_IMG, qa, ra_row, ra_k, NA{});
    else stage_kc(As, A_IMG, qa, NA{});
    if constexpr (B_RK) stage_rk(Bs, B_IMG, qb, rb_row, rb_k, NB{});
    else stage_kc(Bs, B_IMG, qb, NB{});
  };

  // ---- fragments: lane l holds row / column (l & 31) and k 8 * (l >> 5) .. + 7 of a 16-deep slab
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4_t;
  const int g4 = lane >> 4, q4 = (lane >> 2) & 3, pc = (lane & 3) * 4;
  const int frow = 8 * (g4 >> 1) + q4;   // k-col: the k row this lane reads (and + 4)
  int fa_off[TM], fb_off[TN];            // byte offsets of slab 0 within a part image
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int c0 = wr * WM + i * 32;
    fa_off[i] = A_RK ? xrk_off(c0 + (lane & 31), lane >> 5) : xkc_off(frow, c0 + 16 * (g4 & 1) + pc);
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int c0 = wc * WN + j * 32;
    fb_off[j] = B_RK ? xrk_off(c0 + (lane & 31), lane >> 5) : xkc_off(frow, c0 + 16 * (g4 & 1) + pc);
  }
  // slab kk: row-k chunk + 2 * kk -> chunk index bit 1, untouched by the lane's own ^; k-col k + 16 * kk
  auto frag_rk = [&](const char* img, int off, int kk) {
    return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(img + (off ^ (kk << 5))));
  };
  auto frag_kc = [&](const char* img, int off, int kk) {
    const char* q = img + off + kk * 16 * 128;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(q));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(q + 512));   // k + 4: same swizzle
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // one 16-deep slab of the K-step: the small part products (sa + sb >= 1, 2^-8 of the term and below)
  // are summed from zero, smallest first, the hi * hi product is added to the running sum by its MFMA
  // and the small sum after it -- two roundings at the running sum's magnitude per slab instead of six.
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto slab = [&](int kk) {
    bf16x8 fb[PARTS][TN];
#pragma unroll
    for (int s = 0; s < PARTS; ++s)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        fb[s][j] = B_RK ? frag_rk(Bs + s * B_IMG, fb_off[j], kk) : frag_kc(Bs + s * B_IMG, fb_off[j], kk);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      bf16x8 fa[PARTS];
#pragma unroll
      for (int s = 0; s < PARTS; ++s)
        fa[s] = A_RK ? frag_rk(As + s * A_IMG, fa_off[i], kk) : frag_kc(As + s * A_IMG, fa_off[i], kk);
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        // part products (sa, sb), sa + sb = d, smallest terms (largest d) first
        f32x16 sm = zero16;
#pragma unroll
        for (int d = PARTS - 1; d >= 1; --d)
#pragma unroll
          for (int sa = d; sa >= 0; --sa)
            sm = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[sa], fb[d - sa][j], sm, 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0], fb[0][j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] += sm[r];
        __builtin_amdgcn_sched_barrier(0);   // one small sum alive at a time (registers)
      }
    }
  };

  if (nk > 0) {
    load(kbeg);
    split_parts();
    stage();
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
      const bool nxt = t + 1 < nk;
      if (nxt) load(kbeg + (t + 1) * GBK);
      slab(0);
      slab(1);
      // the split after the last fragment read, not under the MFMAs: the kernel is bound by its operand
      // fetch, and the registers the parts would hold across a slab cost the small tiles their occupancy
      __builtin_amdgcn_sched_barrier(0);
      if (nxt) split_parts();
      if (nxt) {
        __syncthreads();   // every wave is done reading the single stage
        stage();
      }
      __syncthreads();
    }
  }

  // ---- epilogue: igemm_f32_big_kernel's (the 32x32 accumulator map is that of the f32 MFMA)
  if (MODE == F_WGRAD || p.raw) {
    float* o = p.out + (size_t)split * p.gm * p.gn;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + wc * WN + j * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wr * WM + i * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
          if (m < p.gm && n < p.gn) o[(size_t)m * p.gn + n] = acc[i][j][r];
        }
      }
  } else {
    float cs[TN], cq[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      cs[j] = 0.f;
      cq[j] = 0.f;
      const int n = n0 + wc * WN + j * 32 + (lane & 31);
      const bool nok = n < p.gn;
      const float bv = (p.bias && nok) ? p.bias[n] : 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wr * WM + i * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
          if (m < p.gm && nok) {
            float v = acc[i][j][r] + bv;
            if (p.resid) v += p.resid[(size_t)m * p.gn + n];
            if (p.relu) v = fmaxf(v, 0.f);
            p.out[(size_t)m * p.gn + n] = v;
            cs[j] += v;
            cq[j] += v * v;
          }
        }
    }
    if (p.stats) {
      float(*red)[2][BN] = reinterpret_cast<float(*)[2][BN]>(As);   // main loop is done
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        cs[j] += __shfl_xor(cs[j], 32, 64);
        cq[j] += __shfl_xor(cq[j], 32, 64);
        if (lane < 32) {
          red[wr][0][wc * WN + j * 32 + lane] = cs[j];
          red[wr][1][wc * WN + j * 32 + lane] = cq[j];
        }
      }
      __syncthreads();
      if (tid < 2 * BN) {
        const int q = tid / BN, c = tid % BN, n = n0 + c;
        if (n < p.gn) p.stats[((size_t)tile_m * 2 + q) * p.gn + n] = red[0][q][c] + red[1][q][c];
      }
    }
  }
}
