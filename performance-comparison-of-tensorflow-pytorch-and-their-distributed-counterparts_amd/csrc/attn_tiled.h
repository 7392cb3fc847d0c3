// Key-tiled ("flash") bf16 attention for 128 < S <= 512 (head dim 64); included by transformer.hip
// after the register-resident kernels, whose AttnParams contract, fragment helpers and register
// layouts it shares.  With the knob attn_tiled = 1 these kernels also take S <= 128.  Each kernel is
// a template over its parameter block: AttnParams is the padded [B, S] batch, AttnPackedParams a
// padding-free batch whose sequences of every length (32 .. 512 rows) lie back to back (attn_seg below).
//
// Forward: block = 4 waves x 16 queries of one (batch, head), grid = B*H*ceil(S/64).  K and V stream
// through LDS in tiles of 64 keys (the next tile's global loads wait in registers while the
// current one is used); per tile each wave forms S^T = K Q^T (the short kernel's MFMA shape and
// reduction order, so forward and backward see the same score bits), so a lane holds one query's scores of the tile and the same query's four
// head dims of O^T: the online-softmax running max m and running sum l are per lane, and the
// rescale exp(m_old - m_new) of the accumulators is lane-local.  l stays a per-lane partial (the
// four 16-lane groups hold different keys) and is reduced once at the end, where O is normalised.
// A tile whose keys are all masked leaves m = -1e30 and p = 1; the first tile with a valid key
// rescales that by exp(-1e30 - m) = 0 exactly.
//
// Backward: two kernels, no floating-point atomics, every sum in a fixed order.
//   dq kernel  (query-parallel, the forward's layout and K / V tiles): sweep 1 over the key tiles
//              forms D[q] = sum_j P_j dP_j from the recomputed P and dP = drop * (V dO^T) and writes
//              it to a workspace; sweep 2 recomputes both, forms dS = P (dP - D) / 8 and accumulates
//              dQ^T = K^T dS^T with K transposed out of the LDS tile.
//   dkv kernel (key-parallel, the short backward's layout): block = 4 waves x 16 keys, Q and dO
//              stream through LDS in tiles of 64 queries; P and dP are recomputed with the MFMA
//              shapes of the dq kernel, D comes from the workspace, dV^T += dO^T Pd and
//              dK^T += Q^T dS accumulate in registers over the query tiles.
// 64-row tiles keep the kernels at 4 / 3 / 2 waves per SIMD (forward / dq / dkv); 128-row tiles cost
// the dkv kernel its second wave (docs/PERF_NOTES.md).
// P = 1 and dP - D = 0 exactly for a sequence with one valid key (the same dP bits in both kernels);
// P = 0 exactly at padded keys.
#pragma once

namespace pcmp {

constexpr int ATS = 512;    // max sequence of the tiled kernels
constexpr int AKT = 64;     // keys (forward, dq) or queries (dkv) per LDS tile (a multiple of 32)
constexpr int ANT = AKT / 16;

// A rows x 64 bf16 tile goes from global rows of pitch ld to an LDS tile of pitch ADP in two halves, so
// that the global loads of the next tile are in flight while the current one is computed on: one
// thread's share is AKT / 32 16-byte pieces (rows % 32 == 0, so the row test is uniform over the block).
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
struct AttnTileRegs { u32x4 v[AKT / 32]; };
__device__ __forceinline__ void attn_tile_load(AttnTileRegs& r, const __bf16* src, size_t ld, int rows) {
#pragma unroll
  for (int u = 0; u < AKT / 32; ++u) {
    const int rr = (threadIdx.x >> 3) + 32 * u, c8 = threadIdx.x & 7;
    if (rr < rows) r.v[u] = *reinterpret_cast<const u32x4*>(src + (size_t)rr * ld + c8 * 8);
  }
}
__device__ __forceinline__ void attn_tile_store(__bf16* dst, const AttnTileRegs& r, int rows) {
#pragma unroll
  for (int u = 0; u < AKT / 32; ++u) {
    const int rr = (threadIdx.x >> 3) + 32 * u, c8 = threadIdx.x & 7;
    if (rr < rows) *reinterpret_cast<u32x4*>(dst + rr * ADP + c8 * 8) = r.v[u];
  }
}

// B operand over the permuted 32-row order of frag_tr_perm from two C tiles
__device__ __forceinline__ bf16x8 attn_pack(const f32x4& a, const f32x4& b) {
  return __builtin_bit_cast(bf16x8, uint4{f2bf2(a[0], a[1]), f2bf2(a[2], a[3]), f2bf2(b[0], b[1]), f2bf2(b[2], b[3])});
}

// Where the rows of one (batch, head) live.  Padded (AttnParams): sequence b is rows b*S .. of the
// [B, S] rectangle and lse / D are [B*H][S].  Packed (AttnPackedParams): sequence b owns rows
// cu[b] .. cu[b+1] of the [T, .] matrices (a multiple of 32 rows, at most p.S = max_s), lse / D are
// [H][T]; b is uniform over the block, so cu is read with scalar loads.  Everything else -- the
// dropout index ((b*H + h)*p.S + q)*p.S + k with q, k local to the sequence included -- is shared, so
// a packed batch computes bit for bit what the padded [B, max_s] batch of its sequences computes.
struct AttnSeg {
  int S;         // rows of the sequence
  size_t row0;   // its first row in qkv / ids / ctx / dctx / dqkv
  size_t lse0;   // its first element in lse / D for head h
};
template <class P>
constexpr bool attn_is_packed = std::is_same<P, AttnPackedParams>::value;
template <class P>
__device__ __forceinline__ AttnSeg attn_seg(const P& p, int bh, int b, int h) {
  if constexpr (attn_is_packed<P>) {
    // the host cannot look at cu's values without a synchronisation (data/imdb.py pack_batch asserts
    // them): a table that breaks the contract is cut to rows inside [0, T) and to max_s, never followed
    const int r0 = min(max(p.cu[b], 0), p.T);
    const int n = min(min(p.cu[b + 1] - r0, p.S), p.T - r0);
    return AttnSeg{max(n, 0) & ~31, (size_t)r0, (size_t)h * p.T + r0};
  } else {
    return AttnSeg{p.S, (size_t)b * p.S, (size_t)bh * p.S};
  }
}

template <class P>   // AttnParams (padded) or AttnPackedParams
__global__ void __launch_bounds__(256) attention_fwd_tiled_kernel(const P p) {
  __shared__ __attribute__((aligned(16))) __bf16 sK[AKT * ADP];
  __shared__ __attribute__((aligned(16))) __bf16 sV[AKT * ADP];
  __shared__ __attribute__((aligned(16))) float sMask[ATS];
  const int QB = (p.S + 63) / 64;
  const int bh = blockIdx.x / QB, qb = blockIdx.x - bh * QB;
  const int b = bh / p.H, h = bh - b * p.H;
  const AttnSeg sg = attn_seg(p, bh, b, h);
  const int S = sg.S;
  if constexpr (attn_is_packed<P>)   // the grid is sized for max_s: block-uniform, before any barrier
    if (qb * 64 >= S) return;
  const int D3 = 3 * p.D;
  const __bf16* base = p.qkv + sg.row0 * D3 + h * AD;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, g = lane >> 4;
  const int q0 = qb * 64 + w * 16;
  const bool act = q0 < S;      // S % 64 == 32: the last block's upper waves only help staging
  const int q = q0 + fr;
  for (int sr = tid; sr < S; sr += 256) sMask[sr] = (p.ids && p.ids[sg.row0 + sr] <= 0) ? -1e30f : 0.f;
  bf16x8 qf[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
    qf[kk] = *reinterpret_cast<const bf16x8*>(base + (size_t)(act ? q : 0) * D3 + kk * 32 + 8 * g);
  float m = -INFINITY, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  AttnTileRegs rk, rv;
  attn_tile_load(rk, base + p.D, D3, min(AKT, S));
  attn_tile_load(rv, base + 2 * p.D, D3, min(AKT, S));
  for (int k0 = 0; k0 < S; k0 += AKT) {
    const int nt = min(AKT, S - k0) / 16;   // even: S % 32 == 0
    if (k0) __syncthreads();                // every wave is done with the previous tile
    attn_tile_store(sK, rk, 16 * nt);
    attn_tile_store(sV, rv, 16 * nt);
    __syncthreads();
    if (k0 + AKT < S) {   // the next tile loads while this one is used
      attn_tile_load(rk, base + p.D + (size_t)(k0 + AKT) * D3, D3, min(AKT, S - k0 - AKT));
      attn_tile_load(rv, base + 2 * p.D + (size_t)(k0 + AKT) * D3, D3, min(AKT, S - k0 - AKT));
    }
    if (!act) continue;
    // S^T = K Q^T: lane = query q, keys k0 + 16j + 4g + e
    f32x4 st[ANT];
#pragma unroll
    for (int j = 0; j < ANT; ++j) {
      st[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (j < nt) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          st[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row(sK, ADP, 16 * j + fr, kk * 32 + 8 * g), qf[kk], st[j], 0, 0, 0);
        }
      }
    }
    float mt = -INFINITY;
#pragma unroll
    for (int j = 0; j < ANT; ++j)
      if (j < nt) {
        const f32x4 mk = *reinterpret_cast<const f32x4*>(sMask + k0 + 16 * j + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = st[j][e] * p.scale + mk[e];
          st[j][e] = v;
          mt = fmaxf(mt, v);
        }
      }
    mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float mn = fmaxf(m, mt);          // >= -1e30: finite from the first tile on
    const float alpha = __expf(m - mn);     // 0 for the first tile (m = -inf) and after all-masked tiles
    m = mn;
    float ps = 0.f;
#pragma unroll
    for (int j = 0; j < ANT; ++j)
      if (j < nt) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float ev = __expf(st[j][e] - mn); st[j][e] = ev; ps += ev; }
      }
    l = l * alpha + ps;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) o[t][e] *= alpha;
    // O^T += V^T Pd^T over the permuted key order of each 32-key chunk
#pragma unroll
    for (int c = 0; c < ANT / 2; ++c)
      if (2 * c < nt) {
        f32x4 v2[2];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v2[hh][e] = st[2 * c + hh][e] * drop_scale(p, bh, q, k0 + 16 * (2 * c + hh) + 4 * g + e);
        const bf16x8 pb = attn_pack(v2[0], v2[1]);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr_perm(sV, ADP, 32 * c, 16 * t), pb, o[t], 0, 0, 0);
      }
  }
  if (!act) return;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const float inv = 1.f / l;
  if (g == 0) p.lse[sg.lse0 + q] = m + __logf(l);
  __bf16* orow = p.out + (sg.row0 + q) * p.D + h * AD;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    *reinterpret_cast<uint2*>(orow + 16 * t + 4 * g) =
        uint2{f2bf2(o[t][0] * inv, o[t][1] * inv), f2bf2(o[t][2] * inv, o[t][3] * inv)};
}

// D[bh][q] (workspace, fp32) and dQ; see the header comment
template <class P>
__global__ void __launch_bounds__(256) attention_bwd_dq_tiled_kernel(const P p, float* __restrict__ Dws) {
  __shared__ __attribute__((aligned(16))) __bf16 sK[AKT * ADP];
  __shared__ __attribute__((aligned(16))) __bf16 sV[AKT * ADP];
  __shared__ __attribute__((aligned(16))) float sMask[ATS];
  const int QB = (p.S + 63) / 64;
  const int bh = blockIdx.x / QB, qb = blockIdx.x - bh * QB;
  const int b = bh / p.H, h = bh - b * p.H;
  const AttnSeg sg = attn_seg(p, bh, b, h);
  const int S = sg.S;
  if constexpr (attn_is_packed<P>)
    if (qb * 64 >= S) return;
  const int D3 = 3 * p.D;
  const __bf16* base = p.qkv + sg.row0 * D3 + h * AD;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, g = lane >> 4;
  const int q0 = qb * 64 + w * 16;
  const bool act = q0 < S;
  const int q = act ? q0 + fr : 0;
  AttnTileRegs rk, rv;
  attn_tile_load(rk, base + p.D, D3, min(AKT, S));
  attn_tile_load(rv, base + 2 * p.D, D3, min(AKT, S));
  for (int sr = tid; sr < S; sr += 256) sMask[sr] = (p.ids && p.ids[sg.row0 + sr] <= 0) ? -1e30f : 0.f;
  bf16x8 qf[2], dof[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    qf[kk] = *reinterpret_cast<const bf16x8*>(base + (size_t)q * D3 + kk * 32 + 8 * g);
    dof[kk] = *reinterpret_cast<const bf16x8*>(p.dout + (sg.row0 + q) * p.D + h * AD + kk * 32 + 8 * g);
  }
  const float lq = p.lse[sg.lse0 + q];
  float Dq = 0.f;
  f32x4 dq[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) dq[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int pass = 0; pass < 2; ++pass) {
    for (int k0 = 0; k0 < S; k0 += AKT) {
      const int nt = min(AKT, S - k0) / 16;
      if (pass | k0) __syncthreads();
      attn_tile_store(sK, rk, 16 * nt);
      attn_tile_store(sV, rv, 16 * nt);
      __syncthreads();
      {   // the next tile (the first one again when sweep 2 follows) loads while this one is used
        const int kn = k0 + AKT < S ? k0 + AKT : 0;
        if (kn || pass == 0) {
          attn_tile_load(rk, base + p.D + (size_t)kn * D3, D3, min(AKT, S - kn));
          attn_tile_load(rv, base + 2 * p.D + (size_t)kn * D3, D3, min(AKT, S - kn));
        }
      }
      if (!act) continue;
      // S^T = K Q^T (the forward's operands and order), dPd^T = V dO^T: lane = query q, keys k0 + 16j + 4g + e
      f32x4 st[ANT], dp[ANT];
#pragma unroll
      for (int j = 0; j < ANT; ++j) {
        st[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        dp[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (j < nt) {
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            st[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row(sK, ADP, 16 * j + fr, kk * 32 + 8 * g), qf[kk], st[j], 0, 0, 0);
            dp[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row(sV, ADP, 16 * j + fr, kk * 32 + 8 * g), dof[kk], dp[j], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < ANT; ++j)
        if (j < nt) {
          const f32x4 mk = *reinterpret_cast<const f32x4*>(sMask + k0 + 16 * j + 4 * g);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float pr = __expf(st[j][e] * p.scale + mk[e] - lq);
            const float dpv = dp[j][e] * drop_scale(p, bh, q, k0 + 16 * j + 4 * g + e);   // dP
            if (pass == 0) Dq += pr * dpv;
            else st[j][e] = pr * (dpv - Dq) * p.scale;                                    // dS
          }
        }
      if (pass == 0) continue;
      // dQ^T += K^T dS^T over the permuted key order
#pragma unroll
      for (int c = 0; c < ANT / 2; ++c)
        if (2 * c < nt) {
          const bf16x8 dsb = attn_pack(st[2 * c], st[2 * c + 1]);
#pragma unroll
          for (int t = 0; t < 4; ++t)
            dq[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr_perm(sK, ADP, 32 * c, 16 * t), dsb, dq[t], 0, 0, 0);
        }
    }
    if (pass == 0) {   // the four key groups of the query, in a fixed order
      Dq += __shfl_xor(Dq, 16, 64);
      Dq += __shfl_xor(Dq, 32, 64);
      if (act && g == 0) Dws[sg.lse0 + q] = Dq;
    }
  }
  if (!act) return;
  __bf16* qrow = p.dqkv + (sg.row0 + q) * D3 + h * AD;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    *reinterpret_cast<uint2*>(qrow + 16 * t + 4 * g) = uint2{f2bf2(dq[t][0], dq[t][1]), f2bf2(dq[t][2], dq[t][3])};
}

// dK, dV for 64 keys per block over all queries; D from the dq kernel's workspace
template <class P>
__global__ void __launch_bounds__(256) attention_bwd_dkv_tiled_kernel(const P p, const float* __restrict__ Dws) {
  __shared__ __attribute__((aligned(16))) __bf16 sQ[AKT * ADP];
  __shared__ __attribute__((aligned(16))) __bf16 sdO[AKT * ADP];
  __shared__ __attribute__((aligned(16))) float sL[ATS];
  __shared__ __attribute__((aligned(16))) float sD[ATS];
  const int KB = (p.S + 63) / 64;
  const int bh = blockIdx.x / KB, kb = blockIdx.x - bh * KB;
  const int b = bh / p.H, h = bh - b * p.H;
  const AttnSeg sg = attn_seg(p, bh, b, h);
  const int S = sg.S;
  if constexpr (attn_is_packed<P>)
    if (kb * 64 >= S) return;
  const int D3 = 3 * p.D;
  const __bf16* base = p.qkv + sg.row0 * D3 + h * AD;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, g = lane >> 4;
  const int key0 = kb * 64 + w * 16;
  const bool act = key0 < S;
  const int key = act ? key0 + fr : 0;
  for (int r = tid; r < S; r += 256) {
    sL[r] = p.lse[sg.lse0 + r];
    sD[r] = Dws[sg.lse0 + r];
  }
  bf16x8 kf[2], vf[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    kf[kk] = *reinterpret_cast<const bf16x8*>(base + p.D + (size_t)key * D3 + kk * 32 + 8 * g);
    vf[kk] = *reinterpret_cast<const bf16x8*>(base + 2 * p.D + (size_t)key * D3 + kk * 32 + 8 * g);
  }
  const float mk = (p.ids && p.ids[sg.row0 + key] <= 0) ? -1e30f : 0.f;
  f32x4 dv[4], dk[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) { dv[t] = f32x4{0.f, 0.f, 0.f, 0.f}; dk[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  const __bf16* dobase = p.dout + sg.row0 * p.D + h * AD;
  AttnTileRegs rq, rdo;
  attn_tile_load(rq, base, D3, min(AKT, S));
  attn_tile_load(rdo, dobase, p.D, min(AKT, S));
  for (int qt = 0; qt < S; qt += AKT) {
    const int nt = min(AKT, S - qt) / 16;
    if (qt) __syncthreads();
    attn_tile_store(sQ, rq, 16 * nt);
    attn_tile_store(sdO, rdo, 16 * nt);
    __syncthreads();
    if (qt + AKT < S) {   // the next tile loads while this one is used
      attn_tile_load(rq, base + (size_t)(qt + AKT) * D3, D3, min(AKT, S - qt - AKT));
      attn_tile_load(rdo, dobase + (size_t)(qt + AKT) * p.D, p.D, min(AKT, S - qt - AKT));
    }
    if (!act) continue;
    // S = Q K^T, dPd = dO V^T: lane = key, queries qt + 16i + 4g + e
    f32x4 sc[ANT], dp[ANT];
#pragma unroll
    for (int i = 0; i < ANT; ++i) {
      sc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      dp[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i < nt) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          sc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row(sQ, ADP, 16 * i + fr, kk * 32 + 8 * g), kf[kk], sc[i], 0, 0, 0);
          dp[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row(sdO, ADP, 16 * i + fr, kk * 32 + 8 * g), vf[kk], dp[i], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < ANT; ++i)
      if (i < nt) {
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(sL + qt + 16 * i + 4 * g);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(sD + qt + 16 * i + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float pr = __expf(sc[i][e] * p.scale + mk - l4[e]);
          const float dsc = drop_scale(p, bh, qt + 16 * i + 4 * g + e, key);
          sc[i][e] = pr * dsc;                                      // Pd
          dp[i][e] = pr * (dp[i][e] * dsc - d4[e]) * p.scale;       // dS
        }
      }
    // dV^T += dO^T Pd, dK^T += Q^T dS over the permuted query order
#pragma unroll
    for (int c = 0; c < ANT / 2; ++c)
      if (2 * c < nt) {
        const bf16x8 pbv = attn_pack(sc[2 * c], sc[2 * c + 1]);
        const bf16x8 dsb = attn_pack(dp[2 * c], dp[2 * c + 1]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          dv[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr_perm(sdO, ADP, 32 * c, 16 * t), pbv, dv[t], 0, 0, 0);
          dk[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr_perm(sQ, ADP, 32 * c, 16 * t), dsb, dk[t], 0, 0, 0);
        }
      }
  }
  if (!act) return;
  __bf16* krow = p.dqkv + (sg.row0 + key) * D3 + p.D + h * AD;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    *reinterpret_cast<uint2*>(krow + 16 * t + 4 * g) = uint2{f2bf2(dk[t][0], dk[t][1]), f2bf2(dk[t][2], dk[t][3])};
    *reinterpret_cast<uint2*>(krow + p.D + 16 * t + 4 * g) = uint2{f2bf2(dv[t][0], dv[t][1]), f2bf2(dv[t][2], dv[t][3])};
  }
}

}  // namespace pcmp
