// Key-tiled ("flash") fp32 attention on the exact f32-input MFMA (v_mfma_f32_16x16x4_f32: bitwise a
// k-ordered fmaf chain) for 256 < S <= 512, head dim 64; included by text_f32.hip inside pcmp::f32,
// after the whole-sequence-in-LDS kernels whose contract it keeps (qkv [B*S][3D], ctx [B*S][D], lse
// [B*H][S], scale 1/8, additive -1e30 key mask, dropout index ((b*H+h)*S+q)*S+key).  With the knob
// attn_f32_tiled = 1 these kernels also take S <= 256.  The structure is attn_tiled.h's; S is any
// length here (not a multiple of 32).
//
// Forward: block = 4 waves x 16 queries of one (batch, head), grid = B*H*ceil(S/64).  K and V stream
// through LDS in tiles of 64 keys (the next tile's global loads wait in registers while the current
// one is used).  Per tile a wave forms S^T = K Q^T, so a lane holds one query's scores of keys
// 16j + 4g + e: the online-softmax state (running max m, partial sum l) is per lane, and the four
// probabilities of accumulator j are the B operand of O^T += V^T P^T as they stand -- MFMA step e
// takes key 16j + 4g + e at k index g from both operands (a permuted k order), so P never visits LDS.
// The A operand of that product is one 16-byte LDS read per key (head dims 4*fr .. 4*fr + 3 for the
// four output tiles), which leaves a lane with head dims 16g + 4e + t of its query: 16-byte stores.
//
// Backward: two kernels, no floating-point atomics, no [S, S] scratch, every sum in a fixed order.
//   dq kernel  (query-parallel, the forward's layout): sweep 1 over the key tiles forms
//              D[q] = sum_j P_j dP_j from the recomputed P and dP = drop * (V dO^T) and writes it to a
//              [B*H][S] workspace; sweep 2 recomputes both, forms dS = P (dP - D) and accumulates
//              dQ^T = K^T dS^T (scaled by 1/8 at the store).
//   dkv kernel (key-parallel): block = 4 waves x 16 keys, Q and dO stream through LDS in tiles of 64
//              queries; P and dP are recomputed, D and lse come from global memory,
//              dV^T += dO^T Pd and dK^T += Q^T dS accumulate in registers over the query tiles.
// Every score and every dP = dO . V is formed by tile_dot below (one MFMA shape, one k order, zero
// initial accumulator; a product's two factors may swap operands, which leaves its bits alone), so the
// forward and both backward kernels see the same score bits and both backward kernels the same dP
// bits: P = 1 and dP - D = 0 exactly for a sequence with one valid key, P = 0 exactly at padded keys.
// A tile whose keys are all padding leaves m = -1e30 and p = 1; the first tile with a valid key
// rescales that by exp(-1e30 - m) = 0 exactly.  Keys beyond S (the last tile's tail) get the mask
// -inf: probability 0 even in an all-padding sequence, whose softmax runs over its S keys as in
// ops/ref.py; rows beyond S are zeros in LDS, so 0 * them stays 0.  Queries beyond S are computed on
// row S - 1 and not stored.
//
// LDS rows are 64 floats + 4 of padding (272 B): the 16 rows a tile_dot read touches start 4 banks
// apart, and the 4 rows a transposed read touches 16 banks apart -- each 16-lane phase of a 16-byte
// read covers all 64 banks once.  36-38 KB of static LDS per block, no scratch, 3 waves per SIMD in
// all three kernels (the forward and the dkv kernel by their launch bounds): 768 blocks of the
// B = 8, S = 512, H = 12 shape are resident at once (docs/PERF_NOTES.md).
#pragma once

constexpr int TS32 = 512;    // max sequence of the tiled kernels
constexpr int TKT = 64;      // keys (forward, dq) or queries (dkv) per LDS tile
constexpr int TLP = AD32 + 4;   // LDS row pitch in floats

// a 64 x 64 fp32 tile, 4 x 16 bytes per thread; rows at or beyond `rows` are zeros
struct Tile32 { f32x4 v[4]; };
__device__ __forceinline__ void tile_load(Tile32& r, const float* src, size_t ld, int rows) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int rr = (threadIdx.x >> 4) + 16 * u, c4 = threadIdx.x & 15;
    r.v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (rr < rows) r.v[u] = *reinterpret_cast<const f32x4*>(src + (size_t)rr * ld + c4 * 4);
  }
}
__device__ __forceinline__ void tile_store(float* dst, const Tile32& r) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int rr = (threadIdx.x >> 4) + 16 * u, c4 = threadIdx.x & 15;
    *reinterpret_cast<f32x4*>(dst + rr * TLP + c4 * 4) = r.v[u];
  }
}
// one row of 64 floats as tile_dot's register operand: dims 16c + 4g + e
__device__ __forceinline__ void row_frag(f32x4 (&f)[4], const float* row, int g) {
#pragma unroll
  for (int c = 0; c < 4; ++c) f[c] = *reinterpret_cast<const f32x4*>(row + 16 * c + 4 * g);
}

// acc[e] = sum_d tile[row0 + 4g + e][d] * rf-row(fr)[d], d in the order 16c + 4g' + e' (c, e' outer to
// inner over the steps, g' the MFMA's k index): THE dot product of these kernels
__device__ __forceinline__ f32x4 tile_dot(const float* tile, int row0, int fr, int g, const f32x4 (&rf)[4]) {
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(tile + (row0 + fr) * TLP + 16 * c + 4 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], rf[c][e], acc, 0, 0, 0);
  }
  return acc;
}
// o[t][e'] += sum_e tile[row0 + 4g' + e][4i + t] * w[e] over (g', e): rows of the tile in tile_dot's
// accumulator order, output row i = 4g + e' of the MFMA, i.e. head dim 16g + 4e' + t for column fr
__device__ __forceinline__ void tile_acc_tr(f32x4 (&o)[4], const float* tile, int row0, int fr, int g, const f32x4& w) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(tile + (row0 + 4 * g + e) * TLP + 4 * fr);
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], w[e], o[t], 0, 0, 0);
  }
}
// a lane's 16 head dims 16g + 4e + t of its row
__device__ __forceinline__ void frag_store(float* row, int g, const f32x4 (&o)[4], float scale) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
    *reinterpret_cast<f32x4*>(row + 16 * g + 4 * e) = f32x4{o[0][e] * scale, o[1][e] * scale, o[2][e] * scale, o[3][e] * scale};
}
// key bias of sequence b for the keys of all tiles: -1e30 at padding, -inf beyond S
__device__ __forceinline__ void fill_mask(float* sMask, const int64_t* ids, int b, int S) {
  for (int sr = threadIdx.x; sr < (S + TKT - 1) / TKT * TKT; sr += 256)
    sMask[sr] = sr >= S ? -INFINITY : (ids && ids[(size_t)b * S + sr] <= 0) ? -1e30f : 0.f;
}
__device__ __forceinline__ float drop_mul(float p, float keep, uint64_t sd, uint64_t idx) {
  return uniform01(sd, idx) >= p ? keep : 0.f;
}

// Where a thread of any of the three kernels works: block = (batch, head) bh x 64 rows (queries in the
// forward and the dq kernel, keys in the dkv kernel), wave = 16 of them, lane = row `row` (MFMA column
// fr, k / accumulator group g).  A wave whose rows all lie beyond S only helps staging (act false); a
// lane beyond S computes on row S - 1 (rowc) and stores nothing.
struct RowPos {
  int bh, b, h, D, D3, fr, g, row, rowc;
  bool act;
  const float* base;    // qkv of sequence b at head h: q at + 0, k at + D, v at + 2D, row pitch D3
  uint64_t sd;          // dropout seed
  float keep;           // 1 / (1 - p)
};
__device__ __forceinline__ RowPos row_pos(const float* qkv, int S, int H, float p, uint64_t seed, const int64_t* salt) {
  RowPos r;
  const int NB = (S + TKT - 1) / TKT;
  r.bh = blockIdx.x / NB;
  r.b = r.bh / H;
  r.h = r.bh - r.b * H;
  r.D = H * AD32;
  r.D3 = 3 * r.D;
  r.base = qkv + (size_t)r.b * S * r.D3 + r.h * AD32;
  const int lane = threadIdx.x & 63, row0 = (blockIdx.x - r.bh * NB) * TKT + (threadIdx.x >> 6) * 16;
  r.fr = lane & 15;
  r.g = lane >> 4;
  r.act = row0 < S;
  r.row = row0 + r.fr;
  r.rowc = min(r.row, S - 1);
  r.sd = dropout_seed(seed, salt);
  r.keep = 1.f / (1.f - p);
  return r;
}
// One step of the tile stream: the two tiles waiting in registers go to LDS between two barriers (the
// first one only when a tile is in use: `busy`), then the loads of the next pair (`rows` rows left from
// nextA / nextB on; none when rows <= 0) are issued and stay in flight while the caller computes.
__device__ __forceinline__ void tiles_step(float* sA, float* sB, Tile32& ra, Tile32& rb, bool busy, const float* nextA,
                                           size_t ldA, const float* nextB, size_t ldB, int rows) {
  if (busy) __syncthreads();
  tile_store(sA, ra);
  tile_store(sB, rb);
  __syncthreads();
  if (rows > 0) {
    tile_load(ra, nextA, ldA, min(TKT, rows));
    tile_load(rb, nextB, ldB, min(TKT, rows));
  }
}

__global__ void __launch_bounds__(256, 3) attn_fwd_f32_tiled_kernel(const float* __restrict__ qkv, const int64_t* __restrict__ ids,
                                                                  float* __restrict__ ctx, float* __restrict__ lse, int B,
                                                                  int S, int H, float p, uint64_t seed, uint64_t offset,
                                                                  const int64_t* salt) {
  __shared__ __attribute__((aligned(16))) float sK[TKT * TLP];
  __shared__ __attribute__((aligned(16))) float sV[TKT * TLP];
  __shared__ __attribute__((aligned(16))) float sMask[TS32];
  const RowPos r = row_pos(qkv, S, H, p, seed, salt);
  const int bh = r.bh, b = r.b, h = r.h, D = r.D, D3 = r.D3, fr = r.fr, g = r.g, q = r.row;
  const float* kbase = r.base + D;
  const float* vbase = r.base + 2 * D;
  const bool act = r.act;
  const uint64_t sd = r.sd;
  const float keep = r.keep;
  Tile32 rk, rv;
  tile_load(rk, kbase, D3, min(TKT, S));
  tile_load(rv, vbase, D3, min(TKT, S));
  fill_mask(sMask, ids, b, S);
  f32x4 qf[4];
  row_frag(qf, r.base + (size_t)r.rowc * D3, g);
  const uint64_t rowidx = offset + ((uint64_t)bh * S + r.rowc) * S;
  float m = -INFINITY, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < S; k0 += TKT) {
    const size_t next = (size_t)(k0 + TKT) * D3;
    tiles_step(sK, sV, rk, rv, k0 != 0, kbase + next, D3, vbase + next, D3, S - k0 - TKT);
    if (!act) continue;
    // S^T = K Q^T: lane = query q, keys k0 + 16j + 4g + e
    f32x4 st[4];
    float mt = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      st[j] = tile_dot(sK, 16 * j, fr, g, qf);
      const f32x4 mk = *reinterpret_cast<const f32x4*>(sMask + k0 + 16 * j + 4 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        st[j][e] = attn_score_f32(st[j][e], mk[e]);
        mt = fmaxf(mt, st[j][e]);
      }
    }
    mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float mn = fmaxf(m, mt);          // >= -1e30: every tile has a key below S
    const float alpha = __expf(m - mn);     // 0 for the first tile (m = -inf) and after all-padding tiles
    m = mn;
    float ps = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float ev = __expf(st[j][e] - mn);
        ps += ev;
        st[j][e] = p > 0.f ? ev * drop_mul(p, keep, sd, rowidx + (k0 + 16 * j + 4 * g + e)) : ev;
      }
    l = l * alpha + ps;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) o[t][e] *= alpha;
    // O^T += V^T Pd^T, keys in the accumulators' order
#pragma unroll
    for (int j = 0; j < 4; ++j) tile_acc_tr(o, sV, 16 * j, fr, g, st[j]);
  }
  if (!act) return;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (q >= S) return;
  if (g == 0) lse[(size_t)bh * S + q] = m + logf(l);
  frag_store(ctx + ((size_t)b * S + q) * D + h * AD32, g, o, 1.f / l);
}

// D[bh][q] (workspace) and dQ; see the header comment
__global__ void __launch_bounds__(256) attn_bwd_dq_f32_tiled_kernel(const float* __restrict__ qkv, const int64_t* __restrict__ ids,
                                                                     const float* __restrict__ dctx, const float* __restrict__ lse,
                                                                     float* __restrict__ Dws, float* __restrict__ dqkv, int B, int S,
                                                                     int H, float p, uint64_t seed, uint64_t offset,
                                                                     const int64_t* salt) {
  __shared__ __attribute__((aligned(16))) float sK[TKT * TLP];
  __shared__ __attribute__((aligned(16))) float sV[TKT * TLP];
  __shared__ __attribute__((aligned(16))) float sMask[TS32];
  const RowPos r = row_pos(qkv, S, H, p, seed, salt);
  const int bh = r.bh, b = r.b, h = r.h, D = r.D, D3 = r.D3, fr = r.fr, g = r.g, q = r.row;
  const float* kbase = r.base + D;
  const float* vbase = r.base + 2 * D;
  const bool act = r.act;
  const uint64_t sd = r.sd;
  const float keep = r.keep;
  Tile32 rk, rv;
  tile_load(rk, kbase, D3, min(TKT, S));
  tile_load(rv, vbase, D3, min(TKT, S));
  fill_mask(sMask, ids, b, S);
  f32x4 qf[4], dof[4];
  row_frag(qf, r.base + (size_t)r.rowc * D3, g);
  row_frag(dof, dctx + ((size_t)b * S + r.rowc) * D + h * AD32, g);
  const float lq = lse[(size_t)bh * S + r.rowc];
  const uint64_t rowidx = offset + ((uint64_t)bh * S + r.rowc) * S;
  float Dq = 0.f;
  f32x4 dq[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) dq[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int pass = 0; pass < 2; ++pass) {
    for (int k0 = 0; k0 < S; k0 += TKT) {
      // the next tile is the first one again when sweep 2 follows
      const int kn = k0 + TKT < S ? k0 + TKT : 0;
      tiles_step(sK, sV, rk, rv, (pass | k0) != 0, kbase + (size_t)kn * D3, D3, vbase + (size_t)kn * D3, D3,
                 (kn || pass == 0) ? S - kn : 0);
      if (!act) continue;
      // S^T = K Q^T (the forward's bits), dPd^T = V dO^T: lane = query q, keys k0 + 16j + 4g + e
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f32x4 st = tile_dot(sK, 16 * j, fr, g, qf);
        const f32x4 dp = tile_dot(sV, 16 * j, fr, g, dof);
        const f32x4 mk = *reinterpret_cast<const f32x4*>(sMask + k0 + 16 * j + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float pr = __expf(attn_score_f32(st[e], mk[e]) - lq);
          // dP: a rounded product of its own, the one the dkv kernel forms
          const float dpv = p > 0.f ? __fmul_rn(dp[e], drop_mul(p, keep, sd, rowidx + (k0 + 16 * j + 4 * g + e))) : dp[e];
          if (pass == 0) Dq = fmaf(pr, dpv, Dq);
          else st[e] = pr * (dpv - Dq);                                                  // dS
        }
        if (pass) tile_acc_tr(dq, sK, 16 * j, fr, g, st);   // dQ^T += K^T dS^T
      }
    }
    if (pass == 0) {   // the four key groups of the query, in a fixed order
      Dq += __shfl_xor(Dq, 16, 64);
      Dq += __shfl_xor(Dq, 32, 64);
      if (act && g == 0 && q < S) Dws[(size_t)bh * S + q] = Dq;
    }
  }
  if (!act || q >= S) return;
  frag_store(dqkv + ((size_t)b * S + q) * D3 + h * AD32, g, dq, 0.125f);
}

// dK, dV for 64 keys per block over all queries; D from the dq kernel's workspace
__global__ void __launch_bounds__(256, 3) attn_bwd_dkv_f32_tiled_kernel(const float* __restrict__ qkv, const int64_t* __restrict__ ids,
                                                                      const float* __restrict__ dctx, const float* __restrict__ lse,
                                                                      const float* __restrict__ Dws, float* __restrict__ dqkv, int B,
                                                                      int S, int H, float p, uint64_t seed, uint64_t offset,
                                                                      const int64_t* salt) {
  __shared__ __attribute__((aligned(16))) float sQ[TKT * TLP];
  __shared__ __attribute__((aligned(16))) float sdO[TKT * TLP];
  __shared__ __attribute__((aligned(16))) float sL[TS32];
  __shared__ __attribute__((aligned(16))) float sD[TS32];
  const RowPos r = row_pos(qkv, S, H, p, seed, salt);
  const int bh = r.bh, b = r.b, h = r.h, D = r.D, D3 = r.D3, fr = r.fr, g = r.g, key = r.row;
  const float* qbase = r.base;
  const float* dobase = dctx + (size_t)b * S * D + h * AD32;
  const bool act = r.act;
  const uint64_t sd = r.sd;
  const float keep = r.keep;
  Tile32 rq, rdo;
  tile_load(rq, qbase, D3, min(TKT, S));
  tile_load(rdo, dobase, D, min(TKT, S));
  // queries beyond S: lse = +inf makes their P exactly 0
  for (int i = threadIdx.x; i < (S + TKT - 1) / TKT * TKT; i += 256) {
    sL[i] = i < S ? lse[(size_t)bh * S + i] : INFINITY;
    sD[i] = i < S ? Dws[(size_t)bh * S + i] : 0.f;
  }
  f32x4 kf[4], vf[4];
  row_frag(kf, r.base + D + (size_t)r.rowc * D3, g);
  row_frag(vf, r.base + 2 * D + (size_t)r.rowc * D3, g);
  const float mk = key >= S ? -INFINITY : (ids && ids[(size_t)b * S + key] <= 0) ? -1e30f : 0.f;
  const uint64_t colidx = offset + (uint64_t)bh * S * S + r.rowc;
  f32x4 dv[4], dk[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) { dv[t] = f32x4{0.f, 0.f, 0.f, 0.f}; dk[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  for (int qt = 0; qt < S; qt += TKT) {
    tiles_step(sQ, sdO, rq, rdo, qt != 0, qbase + (size_t)(qt + TKT) * D3, D3, dobase + (size_t)(qt + TKT) * D, D,
               S - qt - TKT);
    if (!act) continue;
    // S = Q K^T, dPd = dO V^T (the dq kernel's bits): lane = key, queries qt + 16i + 4g + e
    // (rolled: unrolled, the kernel needs 244 registers, and spills when held to 3 waves per SIMD)
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
      f32x4 sc = tile_dot(sQ, 16 * i, fr, g, kf);
      f32x4 dp = tile_dot(sdO, 16 * i, fr, g, vf);
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(sL + qt + 16 * i + 4 * g);
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(sD + qt + 16 * i + 4 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float pr = __expf(attn_score_f32(sc[e], mk) - l4[e]);
        if (p > 0.f) {
          const float dm = drop_mul(p, keep, sd, colidx + (uint64_t)(qt + 16 * i + 4 * g + e) * S);
          sc[e] = pr * dm;                                // Pd
          dp[e] = pr * (__fmul_rn(dp[e], dm) - d4[e]);    // dS
        } else {
          sc[e] = pr;
          dp[e] = pr * (dp[e] - d4[e]);
        }
      }
      tile_acc_tr(dv, sdO, 16 * i, fr, g, sc);   // dV^T += dO^T Pd
      tile_acc_tr(dk, sQ, 16 * i, fr, g, dp);    // dK^T += Q^T dS
    }
  }
  if (!act || key >= S) return;
  float* krow = dqkv + ((size_t)b * S + key) * D3 + D + h * AD32;
  frag_store(krow, g, dk, 0.125f);
  frag_store(krow + D, g, dv, 1.f);
}
