// Two-way block quantiser of the mxfp8 training matmul mode of the Linear layers (docs/PARITY.md "The mxfp8
// training matmul mode").  For y = x W^T the three GEMMs reduce over K (forward), N (DGRAD, dx = dy W) and M
// (WGRAD, gw = dy^T x); the block-scaled MFMA wants both operands contiguous along the reduction with one E8M0
// scale per 32 elements of it.  So every tensor is needed in two images: blocks along its rows and blocks along
// its columns, the latter transposed.  An MX scale depends on its 32 elements only, so -- unlike the per-column
// scales of fp8_train.hip, which cost an amax sweep over the whole column first -- both images come out of one
// read of a tile: no partials, no atomics, no second pass.
//
//   mxfp8_quant_both(x [R,C] bf16 | fp32) -> (q [R,C], e [R, 4*ceil(C/128)], qt [C,R], et [C, 4*ceil(R/128)])
//       (q, e)   = mxfp8_quant(x)                     blocks of 32 consecutive columns of one row
//       (qt, et) = mxfp8_quant(x.t().contiguous())    blocks of 32 consecutive rows of one column
//       both bit for bit, scale rows padded with 127 to whole dwords (the rule of mxfp8.hip).  R % 32 == 0,
//       C % 32 == 0: a block never straddles the edge, in either direction.
//
// mxfp8_quant_both_kernel: 256 threads per tile of 128 rows x 64 columns.
//   Why this tile.  The 128 rows make one tile row of qt 128 contiguous bytes (eight 16-byte stores of eight
//   neighbouring lanes), the 64 columns make a source row 128 (bf16) or 256 (fp32) contiguous bytes to read and
//   64 bytes of q to write; the fp32 staging copy is 34 KB, so four tiles share a CU, and the M = 4096 activations
//   of BERT-base (768 .. 3072 columns) give 384 .. 1536 tiles on 256 CUs.  A 128 x 128 tile would double the LDS
//   and halve the grid for 64 more contiguous bytes of q.
//   Phase 1, the row image, from registers the way mxfp8_quant_kernel does it: a lane loads 16 consecutive
//   columns of one row (4 lanes a row, 16 rows a wave, two passes of 64 rows), parks them as fp32 in LDS, takes
//   the amax of its 16 values and of its pair lane's (one quad DPP move: two lanes are one 32-column block),
//   converts and stores 16 bytes of q; the even lane of a pair stores the block's scale byte.
//   Phase 2, the column image, from transposed LDS reads: lane (rc, c) reads rows 16rc .. 16rc+15 of tile column
//   c (16 ds_read_b32), takes the amax with its pair lane rc ^ 1 (the other half of the 32-row block), converts
//   and stores 16 bytes of qt row c.  A wave covers 8 row chunks x 8 columns, rc the fast index, so eight lanes
//   write the 128 contiguous bytes of one tile row of qt.
//   LDS layout: element (r, c) at dword 68 r + 8 (r >> 4) + c.  The row stride of 68 dwords keeps rows 16-byte
//   aligned for phase 1's ds_write_b128 and shifts neighbouring rows by four banks (the 16 lanes of four rows
//   write 64 different banks).  In a transposed read the 64 lanes are at rows 16 rc + i with one i: their
//   addresses are 1088 rc + 68 i + 8 rc + c = 8 rc + c + 4 i (mod 64) -- the 8 dwords of padding behind every 16
//   rows are what separates the row chunks -- 64 different banks.  The wave's columns are c = (lane >> 3) ^
//   (rc & 4), which also leaves each half-wave on 32 different banks modulo 32.
#include "mx_common.h"

namespace pcmp {

constexpr int kQbR = 128, kQbC = 64;                              // tile rows, columns
constexpr int kQbStride = kQbC + 4, kQbGroupPad = 8;              // dwords per tile row; behind every 16 rows
constexpr int kQbLds = kQbR * kQbStride + kQbR / 16 * kQbGroupPad;
__device__ __forceinline__ int qb_off(int r, int c) { return r * kQbStride + (r >> 4) * kQbGroupPad + c; }

// the scale byte of block `b` of a scale row, and the 127s behind the row's last block (nb blocks, w bytes)
__device__ __forceinline__ void qb_store_scale(uint8_t* row, int b, int nb, int w, unsigned sc) {
  row[b] = (uint8_t)sc;
  if (b == nb - 1)
    for (int c = nb; c < w; ++c) row[c] = (uint8_t)kE8M0One;
}

template <typename T>
__global__ void __launch_bounds__(256) mxfp8_quant_both_kernel(const T* __restrict__ x, uint8_t* __restrict__ q,
                                                              uint8_t* __restrict__ e, uint8_t* __restrict__ qt,
                                                              uint8_t* __restrict__ et, int R, int C, int ew, int etw) {
  __shared__ __attribute__((aligned(16))) float tile[kQbLds];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int c0 = blockIdx.x * kQbC, r0 = blockIdx.y * kQbR;
  {   // phase 1: rows.  C % 32 == 0: the two lanes of a block are inside or outside together
    const int cj = tid & 3, gc = c0 + 16 * cj;
#pragma unroll
    for (int pass = 0; pass < kQbR / 64; ++pass) {
      const int r = pass * 64 + (tid >> 2), gr = r0 + r;
      const bool live = gr < R && gc < C;
      float va[8], vb[8];
      if (live) {
        load8<T>(x + (size_t)gr * C + gc, va);
        load8<T>(x + (size_t)gr * C + gc + 8, vb);
      } else {   // the transposed reads of a live column meet these rows only in dead blocks; keep them defined
#pragma unroll
        for (int k = 0; k < 8; ++k) va[k] = vb[k] = 0.f;
      }
      float* dst = tile + qb_off(r, 16 * cj);
      *reinterpret_cast<f32x4*>(dst) = f32x4{va[0], va[1], va[2], va[3]};
      *reinterpret_cast<f32x4*>(dst + 4) = f32x4{va[4], va[5], va[6], va[7]};
      *reinterpret_cast<f32x4*>(dst + 8) = f32x4{vb[0], vb[1], vb[2], vb[3]};
      *reinterpret_cast<f32x4*>(dst + 12) = f32x4{vb[4], vb[5], vb[6], vb[7]};
      float amax = amax8(vb, amax8(va, 0.f));
      amax = fmaxf(amax, dpp_mov<0xB1>(amax));    // quad_perm(1,0,3,2): the other half of the block
      const unsigned sc = mx_scale_of(amax);
      if (live) {
        const float inv = mx_inv_scale(sc);
        const uint2 lo = quant8(va, inv), hi = quant8(vb, inv);
        *reinterpret_cast<uint4*>(q + (size_t)gr * C + gc) = uint4{lo.x, lo.y, hi.x, hi.y};
        if ((cj & 1) == 0) qb_store_scale(e + (size_t)gr * ew, gc >> 5, C >> 5, ew, sc);
      }
    }
  }
  __syncthreads();
  {   // phase 2: columns.  R % 32 == 0: the two lanes of a block are inside or outside together
    const int rc = lane & 7, cw = (lane >> 3) ^ (rc & 4), gr = r0 + 16 * rc;
#pragma unroll
    for (int pass = 0; pass < kQbC / 32; ++pass) {
      const int c = pass * 32 + wid * 8 + cw, gc = c0 + c;
      const bool live = gc < C && gr < R;
      float va[8], vb[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        va[i] = tile[qb_off(16 * rc + i, c)];
        vb[i] = tile[qb_off(16 * rc + 8 + i, c)];
      }
      float amax = amax8(vb, amax8(va, 0.f));
      amax = fmaxf(amax, dpp_mov<0xB1>(amax));    // lane ^ 1 is row chunk rc ^ 1 of the same column
      const unsigned sc = mx_scale_of(amax);
      if (live) {
        const float inv = mx_inv_scale(sc);
        const uint2 lo = quant8(va, inv), hi = quant8(vb, inv);
        *reinterpret_cast<uint4*>(qt + (size_t)gc * R + gr) = uint4{lo.x, lo.y, hi.x, hi.y};
        if ((rc & 1) == 0) qb_store_scale(et + (size_t)gc * etw, gr >> 5, R >> 5, etw, sc);
      }
    }
  }
}

std::vector<at::Tensor> mxfp8_quant_both(const at::Tensor& x) {
  PCMP_CHECK_CUDA(x);
  PCMP_CHECK_CONTIG(x);
  TORCH_CHECK(x.dim() == 2, "mxfp8_quant_both: x must be [R, C]");
  const int64_t R = x.size(0), C = x.size(1);
  TORCH_CHECK(R > 0 && C > 0 && R % 32 == 0 && C % 32 == 0 && R * C < (1ll << 31),
              "mxfp8_quant_both: R and C must be multiples of 32 (got R = ", R, ", C = ", C, "), below 2^31 elements");
  const int64_t ew = 4 * ((C + 127) / 128), etw = 4 * ((R + 127) / 128);
  const auto o8 = x.options().dtype(at::kFloat8_e4m3fn), ob = x.options().dtype(at::kByte);
  at::Tensor q = torch::empty({R, C}, o8), e = torch::empty({R, ew}, ob);
  at::Tensor qt = torch::empty({C, R}, o8), et = torch::empty({C, etw}, ob);
  const dim3 grid(ceil_div((int)C, kQbC), ceil_div((int)R, kQbR)), block(256);
  if (x.scalar_type() == at::kBFloat16)
    hipLaunchKernelGGL(mxfp8_quant_both_kernel<__bf16>, grid, block, 0, cur_stream(), ptr<const __bf16>(x), ptr<uint8_t>(q),
                       ptr<uint8_t>(e), ptr<uint8_t>(qt), ptr<uint8_t>(et), (int)R, (int)C, (int)ew, (int)etw);
  else if (x.scalar_type() == at::kFloat)
    hipLaunchKernelGGL(mxfp8_quant_both_kernel<float>, grid, block, 0, cur_stream(), ptr<const float>(x), ptr<uint8_t>(q),
                       ptr<uint8_t>(e), ptr<uint8_t>(qt), ptr<uint8_t>(et), (int)R, (int)C, (int)ew, (int)etw);
  else TORCH_CHECK(false, "mxfp8_quant_both: x must be bf16 or fp32");
  PCMP_LAUNCH_CHECK();
  return {q, e, qt, et};
}

}  // namespace pcmp

TORCH_LIBRARY_FRAGMENT(pcmp, m) { m.def("mxfp8_quant_both(Tensor x) -> Tensor[]", &pcmp::mxfp8_quant_both); }
