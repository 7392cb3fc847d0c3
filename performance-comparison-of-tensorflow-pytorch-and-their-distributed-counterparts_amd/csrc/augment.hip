// Batch assembly from the device-resident image cache (data/device_cache.py): shuffle (gather by
// index), augmentation (one inverse affine map per sample: crop, rotation, flip, centre crop in a
// single bilinear resampling pass), normalisation and layout in one launch -- PARITY row B5.
//
// cache : uint8 [N, Sc, Sc, 4], N decoded square images of side Sc, RGBx: one pixel is one aligned
//         dword, so a bilinear tap is one 4-byte load.  The fourth byte is never read into a result.
// idx   : int64 [B] on the device, the source image of every output sample (any order, repeats
//         allowed).  An entry outside [0, N) reads nothing and yields the all-outside sample.
// params: fp32 [B, 6] = (a, b, c, d, e, f).  Output pixel (x, y) has centre (px, py) = (x + 0.5,
//         y + 0.5) and reads the cache image at u = a*px + b*py + c, v = d*px + e*py + f, where
//         pixel i covers [i, i + 1): bilinear at (u - 0.5, v - 0.5) with x0 = floor(u - 0.5),
//         wx = (u - 0.5) - x0, taps x0 and x0 + 1 (y alike).  A tap outside [0, Sc) contributes the
//         pixel value 0 (before normalisation).  This is F.grid_sample(mode='bilinear',
//         padding_mode='zeros', align_corners=False) under the matching affine grid.
// mode 0: uint8 NCHW [B, 3, O, O] = floor(val + 0.5) clamped to 0..255 (what the loaders yield);
// mode 1 / 2: bf16 / fp32 NHWC [B, O, O, cpad] = (val*scale - mean[c]) / std[c], the expression of
//         nchw_to_nhwc_kernel (an unaugmented sample is bit-identical to that input path); pad
//         channels are exact zeros.
//
// A memory-bound gather: one thread per output pixel (grid-stride), four dword loads, neighbouring
// threads read neighbouring cache pixels (exactly so for crops and flips, within a few rows for the
// +-15 degree rotations) and store neighbouring output pixels (mode 0: one byte per channel plane;
// modes 1 / 2: one cpad-channel vector, 16 bytes at cpad = 8 bf16).  No LDS, no atomics, no host
// synchronisation.  All arithmetic is fp32 in the order of ops/ref.py:augment_batch; the build's fma
// contraction may fuse a multiply into the following add, so the two agree to fp32 rounding
// (tests/test_augment_cpu.py states the floor) and bitwise wherever the weights are exact.
#include "common.h"

#include <climits>

namespace pcmp {

namespace {

typedef unsigned short aug_u16x8 __attribute__((ext_vector_type(8)));

// the three channel values of the bilinear sample of image `img` (Sc x Sc dwords) at (u, v)
__device__ __forceinline__ void aug_sample(const uint32_t* __restrict__ img, int Sc, float u, float v, float* val) {
  const float uu = u - 0.5f, vv = v - 0.5f;
  const float fx = floorf(uu), fy = floorf(vv);
  const float wx = uu - fx, wy = vv - fy;
  val[0] = val[1] = val[2] = 0.f;
  // every tap outside the image: nothing to read (also keeps the float -> int conversion in range)
  if (!(fx >= -1.f && fx < (float)Sc && fy >= -1.f && fy < (float)Sc)) return;
  const int x0 = (int)fx, y0 = (int)fy;
  uint32_t p[4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int xx = x0 + i, yy = y0 + j;
      const bool in = xx >= 0 && xx < Sc && yy >= 0 && yy < Sc;
      p[j * 2 + i] = in ? img[(int64_t)yy * Sc + xx] : 0u;
    }
  const float ax = 1.f - wx, ay = 1.f - wy;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p00 = (float)((p[0] >> (8 * c)) & 255u), p01 = (float)((p[1] >> (8 * c)) & 255u);
    const float p10 = (float)((p[2] >> (8 * c)) & 255u), p11 = (float)((p[3] >> (8 * c)) & 255u);
    const float top = p00 * ax + p01 * wx;
    const float bot = p10 * ax + p11 * wx;
    val[c] = top * ay + bot * wy;
  }
}

__device__ __forceinline__ void aug_coords(const float* __restrict__ q, int x, int y, float& u, float& v) {
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
  u = (q[0] * px + q[1] * py) + q[2];
  v = (q[3] * px + q[4] * py) + q[5];
}

// nchw_to_nhwc_kernel's expression, statement for statement
__device__ __forceinline__ float aug_norm(float val, int c, float scale, const float* __restrict__ mean,
                                          const float* __restrict__ stdv) {
  float a = val * scale;
  if (mean) a = (a - mean[c]) / stdv[c];
  return a;
}

template <int MODE>
__global__ __launch_bounds__(256) void augment_batch_kernel(
    const uint32_t* __restrict__ cache, const int64_t* __restrict__ idx, const float* __restrict__ params,
    void* __restrict__ out, int64_t N, int B, int Sc, int O, int cpad, float scale,
    const float* __restrict__ mean, const float* __restrict__ stdv) {
  const int64_t total = (int64_t)B * O * O;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    int x, y, b;
    if (total < INT_MAX) {   // 32-bit index math (64-bit division is a long VALU sequence)
      const unsigned w = (unsigned)t, r = w / (unsigned)O;
      x = w - r * (unsigned)O; y = r % (unsigned)O; b = r / (unsigned)O;
    } else {
      const int64_t r = t / O;
      x = (int)(t - r * O); y = (int)(r % O); b = (int)(r / O);
    }
    const int64_t n = idx[b];
    float val[3] = {0.f, 0.f, 0.f};
    if (n >= 0 && n < N) {
      float u, v;
      aug_coords(params + (int64_t)b * 6, x, y, u, v);
      aug_sample(cache + n * ((int64_t)Sc * Sc), Sc, u, v, val);   // 64-bit element offset of the slot
    }
    if constexpr (MODE == 0) {
      unsigned char* o = reinterpret_cast<unsigned char*>(out);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float r = fminf(fmaxf(floorf(val[c] + 0.5f), 0.f), 255.f);
        o[(((int64_t)b * 3 + c) * O + y) * O + x] = (unsigned char)(int)r;
      }
    } else {
      float nv[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) nv[c] = aug_norm(val[c], c, scale, mean, stdv);
      if constexpr (MODE == 1) {
        unsigned short* o = reinterpret_cast<unsigned short*>(out) + t * cpad;
        if (cpad == 8) {
          aug_u16x8 w8 = {f2bf(nv[0]), f2bf(nv[1]), f2bf(nv[2]), 0, 0, 0, 0, 0};
          *reinterpret_cast<aug_u16x8*>(o) = w8;
        } else {
          for (int c = 0; c < cpad; ++c) o[c] = c < 3 ? f2bf(nv[c]) : (unsigned short)0;
        }
      } else {
        float* o = reinterpret_cast<float*>(out) + t * cpad;
        if (cpad % 4 == 0) {
          *reinterpret_cast<float4*>(o) = make_float4(nv[0], nv[1], nv[2], 0.f);
          for (int c = 4; c < cpad; c += 4) *reinterpret_cast<float4*>(o + c) = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
          for (int c = 0; c < cpad; ++c) o[c] = c < 3 ? nv[c] : 0.f;
        }
      }
    }
  }
}

}  // namespace

at::Tensor augment_batch(const at::Tensor& cache, const at::Tensor& idx, const at::Tensor& params, int64_t out_size,
                         int64_t mode, int64_t cpad, double scale, const c10::optional<at::Tensor>& mean,
                         const c10::optional<at::Tensor>& stdv) {
  PCMP_CHECK_CUDA(cache); PCMP_CHECK_CONTIG(cache);
  PCMP_CHECK_CUDA(idx); PCMP_CHECK_CONTIG(idx);
  PCMP_CHECK_CUDA(params); PCMP_CHECK_CONTIG(params);
  TORCH_CHECK(cache.scalar_type() == at::kByte && cache.dim() == 4 && cache.size(3) == 4 &&
              cache.size(1) == cache.size(2), "augment_batch: cache must be uint8 [N, Sc, Sc, 4]");
  TORCH_CHECK(cache.size(1) > 0 && cache.size(1) <= (1 << 15), "augment_batch: cache side");
  // pixels are read as dwords: a view at a storage offset that is no multiple of 4 is refused
  TORCH_CHECK(reinterpret_cast<uintptr_t>(cache.data_ptr()) % 4 == 0, "augment_batch: cache must be 4-byte aligned");
  TORCH_CHECK(idx.scalar_type() == at::kLong && idx.dim() == 1, "augment_batch: idx must be int64 [B]");
  PCMP_CHECK_F32(params);
  TORCH_CHECK(params.dim() == 2 && params.size(0) == idx.size(0) && params.size(1) == 6,
              "augment_batch: params must be fp32 [B, 6]");
  TORCH_CHECK(out_size > 0 && out_size <= (1 << 15), "augment_batch: out_size");
  TORCH_CHECK(mode >= 0 && mode <= 2, "augment_batch: mode");
  if (mode) TORCH_CHECK(cpad >= 3 && cpad <= 64, "augment_batch: cpad");
  const bool has_mean = mean.has_value() && mean->defined();
  TORCH_CHECK(has_mean == (stdv.has_value() && stdv->defined()), "augment_batch: mean and stdv go together");
  if (has_mean) {
    PCMP_CHECK_CUDA(*mean); PCMP_CHECK_CUDA(*stdv);
    PCMP_CHECK_F32(*mean); PCMP_CHECK_F32(*stdv);
    PCMP_CHECK_CONTIG(*mean); PCMP_CHECK_CONTIG(*stdv);
    TORCH_CHECK(mean->numel() >= 3 && stdv->numel() >= 3, "augment_batch: mean/std of 3 channels");
  }
  const int64_t N = cache.size(0), B = idx.size(0);
  const int Sc = (int)cache.size(1), O = (int)out_size;
  TORCH_CHECK(B <= (1 << 24), "augment_batch: batch size");
  at::Tensor out;
  if (mode == 0) out = at::empty({B, 3, O, O}, cache.options());
  else out = at::empty({B, O, O, cpad}, cache.options().dtype(mode == 1 ? at::kBFloat16 : at::kFloat));
  if (B == 0) return out;
  const dim3 grid(ew_grid(B * (int64_t)O * O));
  const float* mp = optr<float>(mean);
  const float* sp = optr<float>(stdv);
#define PCMP_AUG(M) hipLaunchKernelGGL(augment_batch_kernel<M>, grid, dim3(256), 0, cur_stream(),               \
                                       ptr<uint32_t>(cache), ptr<int64_t>(idx), ptr<float>(params), out.data_ptr(), \
                                       N, (int)B, Sc, O, (int)cpad, (float)scale, mp, sp)
  if (mode == 0) PCMP_AUG(0); else if (mode == 1) PCMP_AUG(1); else PCMP_AUG(2);
#undef PCMP_AUG
  PCMP_LAUNCH_CHECK();
  return out;
}

}  // namespace pcmp

TORCH_LIBRARY_FRAGMENT(pcmp, m) {
  m.def("augment_batch(Tensor cache, Tensor idx, Tensor params, int out_size, int mode, int cpad, float scale, "
        "Tensor? mean, Tensor? stdv) -> Tensor", &pcmp::augment_batch);
}
