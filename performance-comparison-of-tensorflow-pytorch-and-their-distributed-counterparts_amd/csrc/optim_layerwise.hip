// Layer-wise adaptive optimizers over the flat arena: LARS (You et al. 2017, the scaled-gradient form in
// front of the SGD arithmetic of optim_update.h) and LAMB (You et al. 2020, bias-corrected, decay inside
// the update).  Both scale a parameter's step by a trust ratio of two L2 norms over that parameter, so no
// element can be updated before its whole parameter has been read once.  A step is three launches on one
// stream, without host synchronisation and without float atomics:
//
//   1  lars_norms / lamb_moments   one workgroup per chunk: partial (sum w^2, sum x^2) -> part[chunk]
//                                  (x = g' for LARS; x = u, the LAMB update, formed in registers from the
//                                  moments this pass also writes -- u is never stored)
//   2  trust_ratio                 one workgroup per segment: its chunks' partials summed in a fixed order
//                                  in fp64 -> ratio[segment] (fp32, kept by the optimizer)
//   3  lars_apply / lamb_apply     the chunks again: w (LARS: and momentum) and the bf16 shadow
//
// Work split.  A segment is one parameter's arena slice with its alignment padding (zeros with zero
// gradient: they add nothing to a norm and stay exact zeros).  The host cuts every segment into chunks
// of `chunk` elements (a multiple of 16; the last chunk of a segment is short, no chunk spans two
// segments) and numbers them along the arena.  A workgroup owns one chunk and finds its segment once, by
// a binary search over the segments' first-chunk numbers in global memory (workgroup-uniform loads), so
// the learning rate, the decay and the ratio are uniform over the workgroup and the streaming loop holds
// no lookup; the number of segments is not bounded by LDS.  What remains bounded is the grid: at most
// 2^31 - 1 chunks.  With a grid-stride loop instead a workgroup's vectors would fall into many segments
// and a segmented sum would need atomics or a second table.
//
// Bits.  Per thread the squares are accumulated by __builtin_fmaf in ascending address order, then
// block_sum (xor-shuffle tree over a wave, the four waves added in order), then the fp64 sum of pass 2
// (thread t takes partials t, t + 256, ..., then a halving tree over LDS): every order is fixed, two runs
// are bitwise equal.  lamb_apply recomputes u from the stored moments and w with the same lamb_u, whose
// roundings are all spelled out (rounded(), __builtin_fmaf), and both passes take their launch scalars
// from the one out-of-line lamb_scalars, so pass 3 sees the bits pass 1 summed whatever -ffp-contract does.
#include "common.h"
#include "optim_update.h"

namespace pcmp {

constexpr int kLwThreads = 256;

struct SegTable {
  const int64_t* pos;   // [n + 1][2]: first chunk, arena offset of the segment; row n = (chunks, arena size)
  const float* par;     // [n][3]: lr_mult, weight decay, adapted (1) or ratio 1 (0)
  int n;
  int64_t chunk;        // elements per chunk
};

struct Chunk {
  int seg;
  int64_t lo, hi;       // [lo, hi) of the arena, multiples of 16
};

// the segment of chunk blockIdx.x: the last one whose first chunk is <= it (an empty segment shares its
// first chunk with the next one and is never found); the range is clamped to the arena
__device__ __forceinline__ Chunk find_chunk(const SegTable& t, int64_t n) {
  const int64_t b = blockIdx.x;
  int lo = 0, hi = t.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.pos[2 * mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  Chunk c;
  c.seg = lo;
  c.lo = t.pos[2 * lo + 1] + (b - t.pos[2 * lo]) * t.chunk;
  c.hi = c.lo + t.chunk;
  const int64_t end = t.pos[2 * lo + 3] < n ? t.pos[2 * lo + 3] : n;
  if (c.hi > end) c.hi = end;
  if (c.lo < 0) c.lo = c.hi;
  return c;
}

#define PCMP_CHUNK_LOOP(i, c) \
  for (int64_t i = ((c).lo >> 2) + threadIdx.x; i < ((c).hi >> 2); i += kLwThreads)

__device__ __forceinline__ void write_partials(float a, float b, float* __restrict__ part) {
  __shared__ float sh[16];
  a = block_sum(a, sh);
  b = block_sum(b, sh);
  if (threadIdx.x == 0) {
    part[2 * (int64_t)blockIdx.x] = a;
    part[2 * (int64_t)blockIdx.x + 1] = b;
  }
}

// ---------------------------------------------------------------------------------- LARS
//   r = trust_coef * |w| / (|g'| + wd * |w| + eps);  d = r * fma(wd, w, g');  sgd_update(d, decay 0)
// w and g are read by both passes (plain loads: a ResNet-50 arena's pair fits the last-level cache);
// everything pass 3 touches for the last time is nontemporal.
__global__ void __launch_bounds__(kLwThreads)
lars_norms_kernel(const float* __restrict__ w, const float* __restrict__ g, int64_t n, OptScalars sc, SegTable t,
                  float* __restrict__ part) {
  const Chunk c = find_chunk(t, n);
  const float gs = read_or(sc.gscale, 1.f);
  float sw = 0.f, sg = 0.f;
  PCMP_CHUNK_LOOP(i, c) {
    const f32x4 wv = reinterpret_cast<const f32x4*>(w)[i];
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float g0 = rounded(gv[e] * gs);
      sw = __builtin_fmaf(wv[e], wv[e], sw);
      sg = __builtin_fmaf(g0, g0, sg);
    }
  }
  write_partials(sw, sg, part);
}

__global__ void __launch_bounds__(kLwThreads)
lars_apply_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ mom,
                  __bf16* __restrict__ shadow, int64_t n, OptScalars sc, SegTable t, const float* __restrict__ ratio,
                  float momentum, float dampening, int nesterov, int first_step) {
  const Chunk c = find_chunk(t, n);
  const float* par = t.par + 3 * c.seg;
  const float gs = read_or(sc.gscale, 1.f), lr = rounded(*sc.lr * par[0]), wd = par[1], r = ratio[c.seg];
  const SgdScalars s{1.f, momentum, dampening, nesterov, first_step};   // d is already scaled; decay 0 below
  PCMP_CHUNK_LOOP(i, c) {
    f32x4 wv = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(w) + i);
    const f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);
    f32x4 m = momentum != 0.f ? __builtin_nontemporal_load(reinterpret_cast<f32x4*>(mom) + i) : f32x4{0, 0, 0, 0};
    u16x4 sh;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float we = wv[e], me = m[e];
      const float d = rounded(r * __builtin_fmaf(wd, we, rounded(gv[e] * gs)));
      sgd_update(we, d, me, lr, 0.f, s, true);
      wv[e] = we;
      m[e] = me;
      sh[e] = f2bf(we);
    }
    __builtin_nontemporal_store(wv, reinterpret_cast<f32x4*>(w) + i);
    if (momentum != 0.f) __builtin_nontemporal_store(m, reinterpret_cast<f32x4*>(mom) + i);
    if (shadow) __builtin_nontemporal_store(sh, reinterpret_cast<u16x4*>(shadow) + i);
  }
}

// ---------------------------------------------------------------------------------- LAMB
//   m = b1*m + (1-b1)*g';  v = b2*v + ((1-b2)*g')*g';  u = fma(wd, w, (m/bc1) / (sqrt(v)/sqrt(bc2) + eps))
//   r = |w| / |u|;  w = fma(-(lr*r), u, w)
// 1 - beta and the bias corrections are formed in fp64 (1.f - 0.999f is 4.7e-5 off, which a norm of u
// would show) and rounded once.
struct LambScalars { float gs, beta1, beta2, omb1, omb2, eps, bc1, bc2s; };

__device__ __noinline__ LambScalars lamb_scalars(OptScalars sc, double beta1, double beta2, float eps) {
  const double t = (double)read_or(sc.step, 1.f);
  return LambScalars{read_or(sc.gscale, 1.f), (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),
                     eps, (float)(1.0 - pow(beta1, t)), (float)sqrt(1.0 - pow(beta2, t))};
}

__device__ __forceinline__ void lamb_moments(float g, float& m, float& v, const LambScalars& c) {
  const float g0 = rounded(g * c.gs);
  m = rounded(c.beta1 * m) + rounded(c.omb1 * g0);
  v = rounded(c.beta2 * v) + rounded(rounded(c.omb2 * g0) * g0);
}

__device__ __forceinline__ float lamb_u(float w, float m, float v, float wd, const LambScalars& c) {
  const float denom = rounded(sqrtf(v) / c.bc2s) + c.eps;
  return __builtin_fmaf(wd, w, rounded(rounded(m / c.bc1) / denom));
}

// g and the old moments are read for the last time (nontemporal); the new moments and w come back in pass 3
__global__ void __launch_bounds__(kLwThreads)
lamb_moments_kernel(const float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m1,
                    float* __restrict__ m2, int64_t n, OptScalars sc, SegTable t, float* __restrict__ part,
                    double beta1, double beta2, float eps) {
  const Chunk c = find_chunk(t, n);
  const LambScalars ls = lamb_scalars(sc, beta1, beta2, eps);
  const float wd = t.par[3 * c.seg + 1];
  float sw = 0.f, su = 0.f;
  PCMP_CHUNK_LOOP(i, c) {
    const f32x4 wv = reinterpret_cast<const f32x4*>(w)[i];
    const f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);
    f32x4 a = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(m1) + i);
    f32x4 b = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(m2) + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float ae = a[e], be = b[e];
      lamb_moments(gv[e], ae, be, ls);
      const float u = lamb_u(wv[e], ae, be, wd, ls);
      sw = __builtin_fmaf(wv[e], wv[e], sw);
      su = __builtin_fmaf(u, u, su);
      a[e] = ae;
      b[e] = be;
    }
    reinterpret_cast<f32x4*>(m1)[i] = a;
    reinterpret_cast<f32x4*>(m2)[i] = b;
  }
  write_partials(sw, su, part);
}

__global__ void __launch_bounds__(kLwThreads)
lamb_apply_kernel(float* __restrict__ w, const float* __restrict__ m1, const float* __restrict__ m2,
                  __bf16* __restrict__ shadow, int64_t n, OptScalars sc, SegTable t, const float* __restrict__ ratio,
                  double beta1, double beta2, float eps) {
  const Chunk c = find_chunk(t, n);
  const LambScalars ls = lamb_scalars(sc, beta1, beta2, eps);
  const float* par = t.par + 3 * c.seg;
  const float wd = par[1], step = rounded(rounded(*sc.lr * par[0]) * ratio[c.seg]);
  PCMP_CHUNK_LOOP(i, c) {
    f32x4 wv = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(w) + i);
    const f32x4 a = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(m1) + i);
    const f32x4 b = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(m2) + i);
    u16x4 sh;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      wv[e] = __builtin_fmaf(-step, lamb_u(wv[e], a[e], b[e], wd, ls), wv[e]);
      sh[e] = f2bf(wv[e]);
    }
    __builtin_nontemporal_store(wv, reinterpret_cast<f32x4*>(w) + i);
    if (shadow) __builtin_nontemporal_store(sh, reinterpret_cast<u16x4*>(shadow) + i);
  }
}

// ---------------------------------------------------------------------------------- pass 2
// ratio[s] from the partial pairs of segment s's chunks; 1 when the segment is not adapted or a norm is 0
__global__ void __launch_bounds__(kLwThreads)
trust_ratio_kernel(const float* __restrict__ part, SegTable t, float* __restrict__ ratio, float trust_coef, float eps,
                   int lars) {
  __shared__ double sh[2][kLwThreads];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int64_t c0 = t.pos[2 * s], c1 = t.pos[2 * s + 2];
  double a = 0.0, b = 0.0;
  for (int64_t c = c0 + tid; c < c1; c += kLwThreads) {
    a += (double)part[2 * c];
    b += (double)part[2 * c + 1];
  }
  sh[0][tid] = a;
  sh[1][tid] = b;
  __syncthreads();
  for (int o = kLwThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      sh[0][tid] += sh[0][tid + o];
      sh[1][tid] += sh[1][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double wn = sqrt(sh[0][0]), xn = sqrt(sh[1][0]), wd = (double)t.par[3 * s + 1];
    double r = 1.0;
    if (t.par[3 * s + 2] != 0.f && wn > 0.0 && xn > 0.0)
      r = lars ? (double)trust_coef * wn / (xn + wd * wn + (double)eps) : wn / xn;
    ratio[s] = (float)r;
  }
}

// ---------------------------------------------------------------------------------- host side
// The table's values are the Python side's to assert (reading them here would synchronise); what can be
// checked without them is: shapes, devices, and a chunk count that can cover the arena and fits a grid.
static SegTable check_segs(const char* op, const at::Tensor& w, const at::Tensor& seg_pos, const at::Tensor& seg_par,
                           const at::Tensor& part, const at::Tensor& ratio, int64_t chunk, int64_t nchunks) {
  const int64_t n = w.numel(), S = ratio.numel();
  TORCH_CHECK(n % 16 == 0, op, ": the arena is 16-element slices, numel % 16 (got ", n, ")");
  TORCH_CHECK(chunk > 0 && chunk % 16 == 0, op, ": chunk must be a positive multiple of 16 (got ", chunk, ")");
  TORCH_CHECK(S >= 1 && S <= INT_MAX - 1, op, ": needs at least one segment (got ", S, ")");
  TORCH_CHECK(seg_pos.scalar_type() == at::kLong && seg_pos.is_contiguous() && seg_pos.device() == w.device() &&
                  seg_pos.numel() == 2 * (S + 1),
              op, ": seg_pos must be a contiguous int64 tensor of [", S + 1, ", 2] on w's device");
  check_flat(op, "seg_par", seg_par, w, 3 * S);
  check_flat(op, "ratio", ratio, w, S);
  TORCH_CHECK(nchunks <= INT_MAX && nchunks <= n / 16 && nchunks * chunk >= n, op, ": ", nchunks, " chunks of ", chunk,
              " cannot tile an arena of ", n, " elements in one grid");
  check_flat(op, "part", part, w, 2 * nchunks);
  return SegTable{seg_pos.data_ptr<int64_t>(), ptr<float>(seg_par), (int)S, chunk};
}

static void launch_ratio(const SegTable& t, const at::Tensor& part, at::Tensor& ratio, double trust_coef, double eps,
                         bool lars) {
  hipLaunchKernelGGL(trust_ratio_kernel, dim3(t.n), dim3(kLwThreads), 0, cur_stream(), ptr<float>(part), t,
                     ptr<float>(ratio), (float)trust_coef, (float)eps, (int)lars);
  PCMP_LAUNCH_CHECK();
}

void lars_flat(at::Tensor w, const at::Tensor& g, at::Tensor mom, const c10::optional<at::Tensor>& shadow,
               const at::Tensor& lr, const c10::optional<at::Tensor>& gscale, const at::Tensor& seg_pos,
               const at::Tensor& seg_par, at::Tensor part, at::Tensor ratio, int64_t chunk, int64_t nchunks,
               double momentum, double dampening, bool nesterov, bool first_step, double trust_coef, double eps) {
  const char* op = "lars_flat";
  const OptScalars sc = check_common(op, w, g, shadow, c10::nullopt, lr, gscale, nullptr);
  const int64_t n = w.numel();
  if (momentum != 0) check_flat(op, "mom", mom, w, n);
  const SegTable t = check_segs(op, w, seg_pos, seg_par, part, ratio, chunk, nchunks);
  if (n == 0) return;
  hipLaunchKernelGGL(lars_norms_kernel, dim3((unsigned)nchunks), dim3(kLwThreads), 0, cur_stream(), ptr<float>(w),
                     ptr<float>(g), n, sc, t, ptr<float>(part));
  PCMP_LAUNCH_CHECK();
  launch_ratio(t, part, ratio, trust_coef, eps, true);
  hipLaunchKernelGGL(lars_apply_kernel, dim3((unsigned)nchunks), dim3(kLwThreads), 0, cur_stream(), ptr<float>(w),
                     ptr<float>(g), momentum != 0 ? ptr<float>(mom) : nullptr, optr<__bf16>(shadow), n, sc, t,
                     ptr<float>(ratio), (float)momentum, (float)dampening, (int)nesterov, (int)first_step);
  PCMP_LAUNCH_CHECK();
}

void lamb_flat(at::Tensor w, const at::Tensor& g, at::Tensor m1, at::Tensor m2, const c10::optional<at::Tensor>& shadow,
               const at::Tensor& lr, const c10::optional<at::Tensor>& gscale, const at::Tensor& step,
               const at::Tensor& seg_pos, const at::Tensor& seg_par, at::Tensor part, at::Tensor ratio, int64_t chunk,
               int64_t nchunks, double beta1, double beta2, double eps) {
  const char* op = "lamb_flat";
  const OptScalars sc = check_common(op, w, g, shadow, c10::nullopt, lr, gscale, &step);
  const int64_t n = w.numel();
  check_flat(op, "m1", m1, w, n);
  check_flat(op, "m2", m2, w, n);
  const SegTable t = check_segs(op, w, seg_pos, seg_par, part, ratio, chunk, nchunks);
  if (n == 0) return;
  hipLaunchKernelGGL(lamb_moments_kernel, dim3((unsigned)nchunks), dim3(kLwThreads), 0, cur_stream(), ptr<float>(w),
                     ptr<float>(g), ptr<float>(m1), ptr<float>(m2), n, sc, t, ptr<float>(part), beta1, beta2,
                     (float)eps);
  PCMP_LAUNCH_CHECK();
  launch_ratio(t, part, ratio, 0.0, 0.0, false);
  hipLaunchKernelGGL(lamb_apply_kernel, dim3((unsigned)nchunks), dim3(kLwThreads), 0, cur_stream(), ptr<float>(w),
                     ptr<float>(m1), ptr<float>(m2), optr<__bf16>(shadow), n, sc, t, ptr<float>(ratio), beta1, beta2,
                     (float)eps);
  PCMP_LAUNCH_CHECK();
}

#undef PCMP_CHUNK_LOOP

}  // namespace pcmp

TORCH_LIBRARY_FRAGMENT(pcmp, m) {
  m.def("lars_flat(Tensor(a!) w, Tensor g, Tensor(b!) mom, Tensor(c!)? shadow, Tensor lr, Tensor? gscale, "
        "Tensor seg_pos, Tensor seg_par, Tensor(d!) part, Tensor(e!) ratio, int chunk, int nchunks, float momentum, "
        "float dampening, bool nesterov, bool first_step, float trust_coef, float eps) -> ()",
        &pcmp::lars_flat);
  m.def("lamb_flat(Tensor(a!) w, Tensor g, Tensor(b!) m1, Tensor(c!) m2, Tensor(d!)? shadow, Tensor lr, "
        "Tensor? gscale, Tensor step, Tensor seg_pos, Tensor seg_par, Tensor(e!) part, Tensor(f!) ratio, int chunk, "
        "int nchunks, float beta1, float beta2, float eps) -> ()",
        &pcmp::lamb_flat);
}
