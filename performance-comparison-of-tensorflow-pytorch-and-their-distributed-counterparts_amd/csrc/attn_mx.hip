// MXFP8 attention forward of the block-scaled inference family (inference only: no dropout, no lse, no backward).
//
//   attention_mx_fwd(q [B*S, 3D] float8_e4m3fn, e [B*S, 4*ceil(3D/128)] uint8, ids?, B, S, H, out_mx)
//       -> [ctx bf16 [B*S, D]]  or  [ctxq e4m3 [B*S, D], ctxe uint8 [B*S, 4*ceil(D/128)]]  (out_mx)
//
// (q, e) is the pair linear_mxfp8_fwd(..., out_mx=True) emits for the fused QKV projection: head h of Q / K / V
// owns columns h*64 .. of its third of a row and the scale bytes 2h, 2h+1 / D/32 + 2h, .. / 2D/32 + 2h, .. (head
// dim 64 = two 32-element MX blocks).  S % 32 == 0, 32 <= S <= 512; ids is the key mask (ids > 0).
//
// Contract (docs/PARITY.md "The mxfp8 inference attention mode"): ctx = softmax(q k^T / 8 + mask) v on the decoded
// operands, scores and sums in fp32, the probabilities rounded to bf16 before P V; the out_mx pair is quantised
// from the bf16-rounded context, so it is bit for bit mxfp8_quant of the out_mx = false result.  Two runs are
// bitwise equal (no atomics, fixed reduction order).
//
// Kernel: the work split of attention_fwd2_kernel (transformer.hip).  One workgroup of 4 waves x 16 queries per
// (batch, head, 64-query block); a wave computes S^T = K Q^T, so a lane holds one query's scores for 4 keys per
// 16-key tile, the softmax reduces in registers plus two cross-group shuffles, and P^T is already the B operand
// of O^T = V^T P^T.
//   * Q K^T runs on the fp8 MFMA (16x16x32 fp8 x fp8): a 32-deep step is exactly one MX block of a head row, so a
//     key tile takes two MFMAs into two accumulators and one combining step on the VALU,
//     s = a0 * (sq0 * sk0[key]) + a1 * (sq1 * sk1[key]): products of e4m3 values are exact in fp32, the scales are
//     powers of two.  Q and K fragments are 8-byte loads straight from q (lane (fr, g): bytes 8g .. 8g+7 of each
//     block); the query's two scales are lane constants, the keys' are staged per key tile in LDS as floats with
//     1/8 folded in, next to the mask.  The scaled 16x16x128 MFMA would apply the scales in hardware, but a head
//     row fills only half of its 128-deep step (registers 4 to 7 zero): the same two fp8 passes' worth of issue
//     time for 64 useful dims, plus four zero registers per operand, against two VALU multiplies per score here.
//   * V's MX blocks run along the head dim while P V reduces over keys, so its scales cannot ride the MFMA: V is
//     decoded while it is staged (e4m3 byte times 2^(e-127) is exact in bf16) into the row-major bf16 LDS tile
//     frag_tr_perm reads, and P V runs on the bf16 MFMA over the permuted key order with P in bf16 registers.
//   * Keys are walked in tiles of 128 (32 score registers per lane, 18 KB of LDS for V) with the online-softmax
//     rescale of O^T; S <= 128 is the one-tile case, a last tile of 32, 64 or 96 keys runs its 16-key tiles only.
//   * Epilogue: O^T's C layout gives a lane 4 consecutive head dims of one query for each of four 16-dim tiles; a
//     32-dim block is two tiles times the four lane groups (amax, shfl_xor 16 / 32, quant4: mx_tile_epilogue's
//     pattern).
#include "attn_frag.h"
#include "mx_common.h"

namespace pcmp {

constexpr int AMX_KT = 128;   // keys per tile

struct AttnMxParams {
  const uint8_t* q;      // [B*S][3D] e4m3 (q | k | v, head h at cols h*64)
  const uint8_t* e;      // [B*S][eb] E8M0
  const int64_t* ids;    // [B][S] key mask = ids > 0 (nullptr: no mask)
  __bf16* out;           // [B*S][D]                  (!out_mx)
  uint8_t* oq;           // [B*S][D] e4m3             (out_mx)
  uint8_t* oe;           // [B*S][ebo] E8M0           (out_mx)
  int B, S, H, D;
  int eb, ebo;           // bytes per scale row of e / of oe
};

// 2^(e - 127) of a biased E8M0 byte (e = 0: the fp32 denormal 2^-127)
__device__ __forceinline__ float mx_scale_f(unsigned e) { return __uint_as_float(e ? e << 23 : 0x00400000u); }

template <bool OUT_MX>
__global__ void __launch_bounds__(256) attention_mx_fwd_kernel(const AttnMxParams p) {
  __shared__ __attribute__((aligned(16))) __bf16 sV[AMX_KT * ADP];
  __shared__ __attribute__((aligned(16))) float sK0[AMX_KT], sK1[AMX_KT], sMask[AMX_KT];
  const int S = p.S, QB = (S + 63) / 64;
  const int bh = blockIdx.x / QB, qb = blockIdx.x - bh * QB;
  const int b = bh / p.H, h = bh - b * p.H;
  const int D3 = 3 * p.D, nb = p.D >> 5;   // nb: scale bytes of each of Q, K, V in a row
  const uint8_t* base = p.q + (size_t)b * S * D3 + h * AD;     // the head's Q columns, first row of the sequence
  const uint8_t* ebase = p.e + (size_t)b * S * p.eb + 2 * h;   // the head's two Q scale bytes
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, g = lane >> 4;
  const int q0 = qb * 64 + w * 16;
  const bool act = q0 < S;   // S % 16 == 0: a wave's 16 queries are in range or out together
  // B operand Q^T: lane = query q0 + fr, bytes 8g .. 8g+7 of each 32-dim block; its two block scales
  long qf[2] = {0, 0};
  float sq[2] = {0.f, 0.f};
  if (act) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      qf[kk] = *reinterpret_cast<const long*>(base + (size_t)(q0 + fr) * D3 + kk * 32 + 8 * g);
      sq[kk] = mx_scale_f(ebase[(size_t)(q0 + fr) * p.eb + kk]);
    }
  }
  f32x4 o[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;   // l_run: this lane's part of the row sum (reduced over g at the end)
  for (int k0 = 0; k0 < S; k0 += AMX_KT) {
    const int nk = min(AMX_KT, S - k0);   // 32, 64, 96 or 128 keys
    if (k0) __syncthreads();              // the previous tile's V and scales have been read
    // V tile, decoded: 8 bytes of one block -> 8 bf16
    for (int i = tid; i < nk * (AD / 8); i += 256) {
      const int sr = i >> 3, c8 = i & 7;
      const size_t row = (size_t)(k0 + sr);
      const uint2 vb = *reinterpret_cast<const uint2*>(base + row * D3 + 2 * p.D + c8 * 8);
      const float sc = mx_scale_f(ebase[row * p.eb + 2 * nb + (c8 >> 2)]);
      const auto lo0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)vb.x, false), lo1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)vb.x, true);
      const auto hi0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)vb.y, false), hi1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)vb.y, true);
      *reinterpret_cast<uint4*>(sV + sr * ADP + c8 * 8) =
          uint4{f2bf2(lo0[0] * sc, lo0[1] * sc), f2bf2(lo1[0] * sc, lo1[1] * sc), f2bf2(hi0[0] * sc, hi0[1] * sc),
                f2bf2(hi1[0] * sc, hi1[1] * sc)};
    }
    for (int sr = tid; sr < nk; sr += 256) {
      const uint8_t* er = ebase + (size_t)(k0 + sr) * p.eb + nb;
      sK0[sr] = mx_scale_f(er[0]) * 0.125f;
      sK1[sr] = mx_scale_f(er[1]) * 0.125f;
      sMask[sr] = (p.ids && p.ids[(size_t)b * S + k0 + sr] <= 0) ? -1e30f : 0.f;
    }
    __syncthreads();
    if (!act) continue;
    // S^T = K Q^T: A = K rows (keys), one fp8 MFMA per MX block; lane holds keys 16j + 4g + e of query q0 + fr
    f32x4 st[AMX_KT / 16];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < AMX_KT / 16; ++j) {
      if (16 * j >= nk) continue;
      const uint8_t* kr = base + (size_t)(k0 + 16 * j + fr) * D3 + p.D + 8 * g;
      const long kf0 = *reinterpret_cast<const long*>(kr), kf1 = *reinterpret_cast<const long*>(kr + 32);
      const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
      const f32x4 a0 = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(kf0, qf[0], z, 0, 0, 0);
      const f32x4 a1 = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(kf1, qf[1], z, 0, 0, 0);
      const f32x4 c0 = *reinterpret_cast<const f32x4*>(sK0 + 16 * j + 4 * g);
      const f32x4 c1 = *reinterpret_cast<const f32x4*>(sK1 + 16 * j + 4 * g);
      const f32x4 mk = *reinterpret_cast<const f32x4*>(sMask + 16 * j + 4 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = a0[e] * (sq[0] * c0[e]) + a1[e] * (sq[1] * c1[e]) + mk[e];
        st[j][e] = v;
        mx = fmaxf(mx, v);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // online softmax: what the earlier tiles left is rescaled to the new running maximum (first tile: by 0)
    const float m_new = fmaxf(m_run, mx);
    const float alpha = __expf(m_run - m_new);
    m_run = m_new;
    l_run *= alpha;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) o[t][e] *= alpha;
    // P^T B operands per 32-key chunk c: slots i < 4 -> key 32c + 4g + i, i >= 4 -> 32c + 16 + 4g + i - 4
    bf16x8 pb[AMX_KT / 32];
#pragma unroll
    for (int c = 0; c < AMX_KT / 32; ++c) {
      if (32 * c >= nk) continue;
      unsigned pk[4];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int j = 2 * c + hh;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = __expf(st[j][e] - m_new); l_run += v[e]; }
        pk[2 * hh] = f2bf2(v[0], v[1]);
        pk[2 * hh + 1] = f2bf2(v[2], v[3]);
      }
      pb[c] = __builtin_bit_cast(bf16x8, uint4{pk[0], pk[1], pk[2], pk[3]});
    }
    // O^T[d][q] += V^T P^T over the permuted key order
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int c = 0; c < AMX_KT / 32; ++c) {
        if (32 * c >= nk) continue;
        o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr_perm(sV, ADP, 32 * c, 16 * t), pb[c], o[t], 0, 0, 0);
      }
  }
  if (!act) return;
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  const float inv = 1.f / l_run;
  // lane holds head dims 16t + 4g .. + 3 of query q0 + fr, rounded to bf16 first in both output forms
  const size_t row = (size_t)b * S + q0 + fr;
  unsigned u[4][2];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    u[t][0] = f2bf2(o[t][0] * inv, o[t][1] * inv);
    u[t][1] = f2bf2(o[t][2] * inv, o[t][3] * inv);
  }
  if constexpr (!OUT_MX) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
      *reinterpret_cast<uint2*>(p.out + row * p.D + h * AD + 16 * t + 4 * g) = uint2{u[t][0], u[t][1]};
  } else {
    // a 32-dim block is the tile pair (2jp, 2jp+1) times the four lane groups of query fr
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) {
      float v[2][4];
      float amax = 0.f;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const unsigned* uu = u[2 * jp + hh];
        v[hh][0] = __uint_as_float(uu[0] << 16); v[hh][1] = __uint_as_float(uu[0] & 0xffff0000u);
        v[hh][2] = __uint_as_float(uu[1] << 16); v[hh][3] = __uint_as_float(uu[1] & 0xffff0000u);
#pragma unroll
        for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fabsf(v[hh][e]));
      }
      amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
      amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
      const unsigned sc = mx_scale_of(amax);
      const float r = mx_inv_scale(sc);
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
        *reinterpret_cast<unsigned*>(p.oq + row * p.D + h * AD + jp * 32 + hh * 16 + 4 * g) =
            quant4(v[hh][0], v[hh][1], v[hh][2], v[hh][3], r);
      if (g == 0) {
        uint8_t* er = p.oe + row * p.ebo;
        er[2 * h + jp] = (uint8_t)sc;
        if (h == p.H - 1 && jp == 1)         // the row's last block: pad the scale row to whole dwords
          for (int c = nb; c < p.ebo; ++c) er[c] = (uint8_t)kE8M0One;
      }
    }
  }
}

std::vector<at::Tensor> attention_mx_fwd(const at::Tensor& q, const at::Tensor& e, const c10::optional<at::Tensor>& ids,
                                         int64_t B, int64_t S, int64_t H, bool out_mx) {
  TORCH_CHECK(q.is_cuda() && e.is_cuda() && q.is_contiguous() && e.is_contiguous() && q.dim() == 2 && e.dim() == 2,
              "attention_mx_fwd: q / e must be contiguous 2-D GPU tensors");
  TORCH_CHECK(q.scalar_type() == at::kFloat8_e4m3fn && e.scalar_type() == at::kByte,
              "attention_mx_fwd: q must be float8_e4m3fn and e uint8");
  const int64_t D3 = q.size(1), D = D3 / 3, rows = B * S;
  TORCH_CHECK(B > 0 && H > 0 && D3 == 3 * H * AD, "attention_mx_fwd: head dim must be 64");
  TORCH_CHECK(S >= 32 && S % 32 == 0 && S <= 512, "attention_mx_fwd: S must be a multiple of 32, 32 <= S <= 512 (got ", S, ")");
  const int64_t eb = 4 * ((D3 + 127) / 128), ebo = 4 * ((D + 127) / 128);
  TORCH_CHECK(q.size(0) == rows && e.size(0) == rows && e.size(1) == eb, "attention_mx_fwd: q [B*S, 3D], e [B*S, ", eb, "]");
  TORCH_CHECK(rows * D3 < (1ll << 31), "attention_mx_fwd: operand beyond 2 GiB");
  const bool has_ids = ids.has_value() && ids->defined();
  at::Tensor idc;
  if (has_ids) {
    TORCH_CHECK(ids->is_cuda() && ids->scalar_type() == at::kLong && ids->numel() == rows, "attention_mx_fwd: ids must be int64 [B, S]");
    idc = ids->contiguous();
  }
  AttnMxParams p{};
  std::vector<at::Tensor> out;
  if (out_mx) {
    out = {torch::empty({rows, D}, q.options()), torch::empty({rows, ebo}, e.options())};
    p.oq = ptr<uint8_t>(out[0]);
    p.oe = ptr<uint8_t>(out[1]);
  } else {
    out = {torch::empty({rows, D}, q.options().dtype(at::kBFloat16))};
    p.out = ptr<__bf16>(out[0]);
  }
  p.q = ptr<const uint8_t>(q);
  p.e = ptr<const uint8_t>(e);
  p.ids = has_ids ? idc.data_ptr<int64_t>() : nullptr;
  p.B = (int)B; p.S = (int)S; p.H = (int)H; p.D = (int)D;
  p.eb = (int)eb; p.ebo = (int)ebo;
  const dim3 grid((unsigned)(B * H * ((S + 63) / 64)));
  if (out_mx) hipLaunchKernelGGL(attention_mx_fwd_kernel<true>, grid, dim3(256), 0, cur_stream(), p);
  else hipLaunchKernelGGL(attention_mx_fwd_kernel<false>, grid, dim3(256), 0, cur_stream(), p);
  PCMP_LAUNCH_CHECK();
  return out;
}

}  // namespace pcmp

TORCH_LIBRARY_FRAGMENT(pcmp, m) {
  m.def("attention_mx_fwd(Tensor q, Tensor e, Tensor? ids, int B, int S, int H, bool out_mx) -> Tensor[]",
        &pcmp::attention_mx_fwd);
}
