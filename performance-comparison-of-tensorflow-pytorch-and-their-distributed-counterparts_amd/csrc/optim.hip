// Fused flat-buffer optimizers and global gradient-norm clipping.
//
// Every trainable parameter of a model lives in ONE fp32 master buffer (and its bf16 compute
// shadow in one bf16 buffer); gradients live in ONE fp32 buffer whose slices are the DDP
// all-reduce buckets.  An optimizer step is therefore a single streaming kernel over the whole
// model (ResNet-50: 25.6 M params in one launch), not a per-tensor loop:
//   sgd_flat   : torch.optim.SGD semantics (momentum, dampening, weight decay, nesterov)
//                -- Keras SGD(lr=0.001) of resnet.py:24 and the north-star SGD
//   adam_flat  : torch.optim.Adam (L2 weight decay) / AdamW (decoupled decay)
//                -- Adam(lr=3e-3) of another_neural_net.py:114,258 and HF AdamW(lr=2e-5,
//                eps=1e-8) of pytorch_on_language_distr.py:167-170
//   grad_norm  : global L2 norm over the flat gradient (clip_grad_norm_, :271-273); the clip
//                coefficient is computed ON DEVICE and consumed by the optimizer kernel through a
//                pointer, so clipping needs no host synchronisation and is graph-capturable.
// Learning rate and step count are also read through device pointers (LR schedules update a
// device scalar; hipGraph replays stay valid).  The kernels write the refreshed bf16 shadow in
// the same pass ("cast fused into the update").
#include "common.h"

namespace pcmp {

struct OptScalars {
  const float* lr;         // device scalar
  const float* gscale;     // device scalar multiplier on grads (clip coef * 1/world), may be null
  const float* step;       // device scalar (Adam bias correction), may be null
};

__device__ __forceinline__ float read_or(const float* p, float d) { return p ? *p : d; }

// ---------------------------------------------------------------------------------- the element updates
// sgd_update / adam_update are the one definition of an optimizer step's arithmetic; the ungrouped ops
// (sgd_flat / adam_flat: lr and wd of the launch, an optional uint8 mask) and the grouped ops
// (sgd_flat_groups / adam_flat_groups: lr and wd looked up per run) instantiate the same kernel
// template around them, so the two paths are bitwise equal by construction.  The build's
// -ffp-contract=fast would leave to the compiler which products fuse into an fma, so every rounding is
// spelled out: __builtin_fmaf where the step fuses, rounded() -- a value pinned in a register, which a
// later add cannot fuse with -- where the product is rounded first:
//   sgd :  d = fma(g, gs, wd*w);  m = mom*m + (1-damp)*d;  nesterov d = fma(mom, m, d);  w = fma(-lr, d, w)
//   adam:  gv = g*gs [+ wd*w];  m1 = b1*m1 + (1-b1)*gv;  m2 = b2*m2 + ((1-b2)*gv)*gv;
//          denom = sqrt(m2)/sqrt(bc2) + eps;  [w = w * fma(-wd, lr, 1)];  w = w - (step_size*m1)/denom
// tests/test_optim_flat_bits_gpu.py holds these bits to the recorded ones.  A masked-off element
// (on == false) keeps w; under SGD its momentum still advances, under Adam its state stays too.
// A pinned value is formed outside the launch-uniform choices (first_step, decoupled) and selected
// afterwards: the compiler does not speculate an asm, so a pin inside a choice is a branch per element.
__device__ __forceinline__ float rounded(float x) {
  asm("" : "+v"(x));
  return x;
}

struct SgdScalars { float gs, momentum, dampening; int nesterov, first_step; };   // of the launch

__device__ __forceinline__ void sgd_update(float& w, float g, float& m, float lr, float wd, const SgdScalars& c,
                                           bool on) {
  float d = __builtin_fmaf(g, c.gs, rounded(wd * w));
  const float blend = rounded(c.momentum * m) + rounded((1.f - c.dampening) * d);
  if (c.momentum != 0.f) {
    m = c.first_step ? d : blend;
    d = c.nesterov ? __builtin_fmaf(c.momentum, m, d) : m;
  }
  if (on) w = __builtin_fmaf(-lr, d, w);
}

struct AdamScalars {
  float gs, beta1, beta2, eps, bc1, bc2s;   // of the launch: bc1 = 1 - beta1^t, bc2s = sqrt(1 - beta2^t)
  int decoupled;
  float wd, step_size, keep;                // of (lr, wd): set_rates
};

__device__ __forceinline__ void set_rates(AdamScalars& c, float lr, float wd) {
  c.wd = wd;
  c.step_size = lr / c.bc1;
  c.keep = __builtin_fmaf(-wd, lr, 1.f);   // AdamW: 1 - lr * wd
}

__device__ __forceinline__ void adam_update(float& w, float g, float& m1, float& m2, const AdamScalars& c, bool on) {
  const float g0 = rounded(g * c.gs), l2 = rounded(g0 + rounded(c.wd * w)), kept = rounded(w * c.keep);
  const float gv = c.decoupled ? g0 : l2;
  float nw = c.decoupled ? kept : w;
  const float a = rounded(c.beta1 * m1) + rounded((1.f - c.beta1) * gv);
  const float b = rounded(c.beta2 * m2) + rounded(rounded((1.f - c.beta2) * gv) * gv);
  const float denom = rounded(sqrtf(b) / c.bc2s) + c.eps;
  nw = nw - rounded(rounded(c.step_size * a) / denom);
  w = on ? nw : w;
  m1 = on ? a : m1;
  m2 = on ? b : m2;
}

// ---------------------------------------------------------------------------------- parameter groups
// The grouped ops run the same streaming step with a per-*run* learning-rate multiplier and weight
// decay.  A run is a maximal stretch of adjacent parameters of one group; the table (run_end: absolute
// arena offsets in elements, increasing, multiples of 16; run_lr_mult; run_wd) lives on the device and
// is staged into LDS once per workgroup (a strided loop: R may exceed the 256 threads).  Every
// parameter slice starts on a 16-element boundary and a thread works on 4-element vectors, so a vector
// lies in exactly one run: one lookup per vector, by a carried cursor (arena offsets only grow along
// the grid-stride loop) with a binary search over the runs after it.  The element update then gets
// lr = rounded(lr0 * lr_mult[run]) (one rounded fp32 product) and wd = run_wd[run]; no atomics, nothing
// read from the host.
constexpr int kMaxRuns = 2048;   // 16 B of LDS per run: 32 KiB

struct RunTable {
  const int64_t* end;      // [n] arena offset at which each run ends
  const float* lr_mult;    // [n]
  const float* wd;         // [n]
  int n;
};

struct RunLds {
  int64_t* end;
  float* lr_mult;
  float* wd;
};

__device__ __forceinline__ RunLds stage_runs(const RunTable& t, unsigned char* lds) {
  RunLds s;
  s.end = reinterpret_cast<int64_t*>(lds);
  s.lr_mult = reinterpret_cast<float*>(s.end + t.n);
  s.wd = s.lr_mult + t.n;
  for (int r = threadIdx.x; r < t.n; r += blockDim.x) {
    s.end[r] = t.end[r];
    s.lr_mult[r] = t.lr_mult[r];
    s.wd[r] = t.wd[r];
  }
  __syncthreads();
  return s;
}

// the first run r >= cur with off < end[r]; the last run when there is none (an offset past the
// table never indexes outside it)
__device__ __forceinline__ int find_run(const int64_t* end, int n, int cur, int64_t off) {
  if (off < end[cur]) return cur;
  int lo = cur + 1, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off < end[mid]) hi = mid;
    else lo = mid + 1;
  }
  return lo < n ? lo : n - 1;
}

// kRuns = false: the ungrouped op (no LDS, no lookup; lr from the device scalar, wd from the launch,
// mask honoured).  kRuns = true: the grouped op over w = arena[base, base + n) (no mask).
template <bool kRuns>
__global__ void sgd_flat_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ mom,
                                __bf16* __restrict__ shadow, const uint8_t* __restrict__ mask, int64_t n, int64_t base,
                                OptScalars sc, RunTable runs, float wd0, float momentum, float dampening, int nesterov,
                                int first_step) {
  extern __shared__ __attribute__((aligned(16))) unsigned char run_lds[];
  RunLds rt;
  if constexpr (kRuns) rt = stage_runs(runs, run_lds);
  const SgdScalars c{read_or(sc.gscale, 1.f), momentum, dampening, nesterov, first_step};
  const float lr0 = *sc.lr;
  float lr = lr0, wd = wd0;
  int run = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n / 4;
       i += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (kRuns) {
      run = find_run(rt.end, runs.n, run, base + i * 4);
      lr = rounded(lr0 * rt.lr_mult[run]);
      wd = rt.wd[run];
    }
    f32x4 wv = reinterpret_cast<f32x4*>(w)[i];
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 m = momentum != 0.f ? reinterpret_cast<f32x4*>(mom)[i] : f32x4{0, 0, 0, 0};
    u16x4 sh;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float we = wv[e], me = m[e];   // a vector element does not bind to a reference
      sgd_update(we, gv[e], me, lr, wd, c, kRuns || !mask || mask[i * 4 + e]);
      wv[e] = we;
      m[e] = me;
      sh[e] = f2bf(we);
    }
    reinterpret_cast<f32x4*>(w)[i] = wv;
    if (momentum != 0.f) reinterpret_cast<f32x4*>(mom)[i] = m;
    if (shadow) reinterpret_cast<u16x4*>(shadow)[i] = sh;
  }
}

template <bool kRuns>
__global__ void adam_flat_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m1,
                                 float* __restrict__ m2, __bf16* __restrict__ shadow, const uint8_t* __restrict__ mask,
                                 int64_t n, int64_t base, OptScalars sc, RunTable runs, float wd0, float beta1,
                                 float beta2, float eps, int decoupled) {
  extern __shared__ __attribute__((aligned(16))) unsigned char run_lds[];
  RunLds rt;
  if constexpr (kRuns) rt = stage_runs(runs, run_lds);
  const float lr0 = *sc.lr, t = read_or(sc.step, 1.f);
  AdamScalars c{read_or(sc.gscale, 1.f), beta1, beta2, eps, 1.f - powf(beta1, t), sqrtf(1.f - powf(beta2, t)),
                decoupled};
  set_rates(c, lr0, wd0);
  int run = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n / 4;
       i += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (kRuns) {
      run = find_run(rt.end, runs.n, run, base + i * 4);
      set_rates(c, rounded(lr0 * rt.lr_mult[run]), rt.wd[run]);
    }
    // every operand is streamed exactly once per step: nontemporal loads / stores (5.1 -> 5.5 TB/s
    // over a 110 M-parameter buffer, profiles/r4_adam_lab.txt)
    f32x4 wv = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(w) + i);
    const f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);
    f32x4 a = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(m1) + i);
    f32x4 b = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(m2) + i);
    u16x4 sh;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float we = wv[e], ae = a[e], be = b[e];   // a vector element does not bind to a reference
      adam_update(we, gv[e], ae, be, c, kRuns || !mask || mask[i * 4 + e]);
      wv[e] = we;
      a[e] = ae;
      b[e] = be;
      sh[e] = f2bf(we);
    }
    __builtin_nontemporal_store(wv, reinterpret_cast<f32x4*>(w) + i);
    __builtin_nontemporal_store(a, reinterpret_cast<f32x4*>(m1) + i);
    __builtin_nontemporal_store(b, reinterpret_cast<f32x4*>(m2) + i);
    if (shadow) __builtin_nontemporal_store(sh, reinterpret_cast<u16x4*>(shadow) + i);
  }
}

// partial sums of squares -> part[blockIdx]
__global__ void sumsq_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part) {
  __shared__ float sh[16];
  float s = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n / 4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
    s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// norm = sqrt(sum part) * pre_scale ; coef = min(1, max_norm / (norm + 1e-6)) * post_scale
__global__ void clip_coef_kernel(const float* __restrict__ part, int np, float pre_scale, float max_norm,
                                 float post_scale, float* __restrict__ norm_out, float* __restrict__ coef_out) {
  __shared__ float sh[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < np; i += blockDim.x) s += part[i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) {
    const float norm = sqrtf(s) * pre_scale;
    *norm_out = norm;
    float c = max_norm > 0.f ? max_norm / (norm + 1e-6f) : 1.f;
    c = fminf(c, 1.f);
    *coef_out = c * post_scale;
  }
}

__global__ void cast_f32_bf16_kernel(const float* __restrict__ x, __bf16* __restrict__ y, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    reinterpret_cast<unsigned short*>(y)[i] = f2bf(x[i]);
}

static int flat_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n / 4 + 255) / 256)); }

// ---------------------------------------------------------------------------------- host side
// The four ops share one launcher per optimizer and its checks; a refused call launches nothing.
static void check_flat(const char* op, const char* name, const at::Tensor& t, const at::Tensor& like, int64_t n,
                       at::ScalarType dtype = at::kFloat, const char* dname = "fp32") {
  TORCH_CHECK(t.scalar_type() == dtype && t.is_contiguous() && t.device() == like.device() && t.numel() == n, op, ": ",
              name, " must be a contiguous ", dname, " tensor of ", n, " elements on ", like.device());
}

static const float* scalar_f32(const char* op, const char* name, const at::Tensor& t, const at::Tensor& like) {
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.numel() >= 1 && t.device() == like.device(), op, ": ", name,
              " must be an fp32 device scalar on w's device");
  return ptr<float>(t);
}

// what every op takes: w, g, the optional shadow and mask, and the device scalars (step: Adam's)
static OptScalars check_common(const char* op, const at::Tensor& w, const at::Tensor& g,
                               const c10::optional<at::Tensor>& shadow, const c10::optional<at::Tensor>& mask,
                               const at::Tensor& lr, const c10::optional<at::Tensor>& gscale, const at::Tensor* step) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.is_contiguous(), op,
              ": w must be a contiguous fp32 GPU tensor");
  const int64_t n = w.numel();
  check_flat(op, "g", g, w, n);
  if (shadow.has_value() && shadow->defined()) check_flat(op, "shadow", *shadow, w, n, at::kBFloat16, "bf16");
  if (mask.has_value() && mask->defined()) check_flat(op, "mask", *mask, w, n, at::kByte, "uint8");
  TORCH_CHECK(n % 4 == 0, op, ": numel % 4 (got ", n, ")");
  return OptScalars{scalar_f32(op, "lr", lr, w),
                    gscale.has_value() && gscale->defined() ? scalar_f32(op, "gscale", *gscale, w) : nullptr,
                    step ? scalar_f32(op, "step", *step, w) : nullptr};
}

// the run table of a grouped op and the slice [base, base + n) of its arena that w is
struct RunArgs {
  const at::Tensor& run_end;
  const at::Tensor& run_lr_mult;
  const at::Tensor& run_wd;
  int64_t base, arena_size;
};

// run_end's values are the Python side's to assert (reading them here would synchronise)
static RunTable check_runs(const char* op, const at::Tensor& w, const RunArgs& a) {
  const int64_t n = w.numel(), base = a.base;
  TORCH_CHECK(base >= 0 && base % 4 == 0, op, ": base must be a non-negative multiple of 4 (got ", base, ")");
  TORCH_CHECK(base + n <= a.arena_size, op, ": slice [", base, ", ", base + n, ") ends past the arena of ",
              a.arena_size, " elements the run table covers");
  const int64_t R = a.run_end.numel();
  TORCH_CHECK(R >= 1 && R <= kMaxRuns, op, ": the run table needs 1 to ", kMaxRuns, " runs (got ", R, ")");
  TORCH_CHECK(a.run_lr_mult.numel() == R && a.run_wd.numel() == R, op, ": run_end, run_lr_mult and run_wd must have "
              "one length (got ", R, ", ", a.run_lr_mult.numel(), ", ", a.run_wd.numel(), ")");
  TORCH_CHECK(a.run_end.scalar_type() == at::kLong && a.run_end.is_contiguous() && a.run_end.device() == w.device(),
              op, ": run_end must be a contiguous int64 tensor on w's device");
  check_flat(op, "run_lr_mult", a.run_lr_mult, w, R);
  check_flat(op, "run_wd", a.run_wd, w, R);
  return RunTable{a.run_end.data_ptr<int64_t>(), ptr<float>(a.run_lr_mult), ptr<float>(a.run_wd), (int)R};
}

static size_t run_lds_bytes(const RunTable& t) { return (size_t)t.n * (sizeof(int64_t) + 2 * sizeof(float)); }

// ra == nullptr: the ungrouped op (wd of the call); otherwise the grouped op (wd of the table, no mask)
static void sgd_launch(const char* op, at::Tensor& w, const at::Tensor& g, at::Tensor& mom,
                       const c10::optional<at::Tensor>& shadow, const c10::optional<at::Tensor>& mask,
                       const at::Tensor& lr, const c10::optional<at::Tensor>& gscale, const RunArgs* ra, double wd,
                       double momentum, double dampening, bool nesterov, bool first_step) {
  const OptScalars sc = check_common(op, w, g, shadow, mask, lr, gscale, nullptr);
  const int64_t n = w.numel();
  if (momentum != 0) check_flat(op, "mom", mom, w, n);
  const RunTable runs = ra ? check_runs(op, w, *ra) : RunTable{};
  if (n == 0) return;
  hipLaunchKernelGGL(ra ? sgd_flat_kernel<true> : sgd_flat_kernel<false>, dim3(flat_grid(n)), dim3(256),
                     run_lds_bytes(runs), cur_stream(), ptr<float>(w), ptr<float>(g),
                     momentum != 0 ? ptr<float>(mom) : nullptr, optr<__bf16>(shadow), optr<uint8_t>(mask), n,
                     ra ? ra->base : 0, sc, runs, (float)wd, (float)momentum, (float)dampening, (int)nesterov,
                     (int)first_step);
  PCMP_LAUNCH_CHECK();
}

static void adam_launch(const char* op, at::Tensor& w, const at::Tensor& g, at::Tensor& m1, at::Tensor& m2,
                        const c10::optional<at::Tensor>& shadow, const c10::optional<at::Tensor>& mask,
                        const at::Tensor& lr, const c10::optional<at::Tensor>& gscale, const at::Tensor& step,
                        const RunArgs* ra, double wd, double beta1, double beta2, double eps, bool decoupled) {
  const OptScalars sc = check_common(op, w, g, shadow, mask, lr, gscale, &step);
  const int64_t n = w.numel();
  check_flat(op, "m1", m1, w, n);
  check_flat(op, "m2", m2, w, n);
  const RunTable runs = ra ? check_runs(op, w, *ra) : RunTable{};
  if (n == 0) return;
  hipLaunchKernelGGL(ra ? adam_flat_kernel<true> : adam_flat_kernel<false>, dim3(flat_grid(n)), dim3(256),
                     run_lds_bytes(runs), cur_stream(), ptr<float>(w), ptr<float>(g), ptr<float>(m1), ptr<float>(m2),
                     optr<__bf16>(shadow), optr<uint8_t>(mask), n, ra ? ra->base : 0, sc, runs, (float)wd,
                     (float)beta1, (float)beta2, (float)eps, (int)decoupled);
  PCMP_LAUNCH_CHECK();
}

void sgd_flat(at::Tensor w, const at::Tensor& g, at::Tensor mom, const c10::optional<at::Tensor>& shadow,
              const c10::optional<at::Tensor>& mask, const at::Tensor& lr, const c10::optional<at::Tensor>& gscale,
              double momentum, double dampening, double wd, bool nesterov, bool first_step) {
  sgd_launch("sgd_flat", w, g, mom, shadow, mask, lr, gscale, nullptr, wd, momentum, dampening, nesterov, first_step);
}

void adam_flat(at::Tensor w, const at::Tensor& g, at::Tensor m1, at::Tensor m2, const c10::optional<at::Tensor>& shadow,
               const c10::optional<at::Tensor>& mask, const at::Tensor& lr, const c10::optional<at::Tensor>& gscale,
               const at::Tensor& step, double beta1, double beta2, double eps, double wd, bool decoupled) {
  adam_launch("adam_flat", w, g, m1, m2, shadow, mask, lr, gscale, step, nullptr, wd, beta1, beta2, eps, decoupled);
}

void sgd_flat_groups(at::Tensor w, const at::Tensor& g, at::Tensor mom, const c10::optional<at::Tensor>& shadow,
                     const at::Tensor& lr, const c10::optional<at::Tensor>& gscale, const at::Tensor& run_end,
                     const at::Tensor& run_lr_mult, const at::Tensor& run_wd, int64_t base, int64_t arena_size,
                     double momentum, double dampening, bool nesterov, bool first_step) {
  const RunArgs ra{run_end, run_lr_mult, run_wd, base, arena_size};
  sgd_launch("sgd_flat_groups", w, g, mom, shadow, c10::nullopt, lr, gscale, &ra, 0.0, momentum, dampening, nesterov,
             first_step);
}

void adam_flat_groups(at::Tensor w, const at::Tensor& g, at::Tensor m1, at::Tensor m2,
                      const c10::optional<at::Tensor>& shadow, const at::Tensor& lr,
                      const c10::optional<at::Tensor>& gscale, const at::Tensor& step, const at::Tensor& run_end,
                      const at::Tensor& run_lr_mult, const at::Tensor& run_wd, int64_t base, int64_t arena_size,
                      double beta1, double beta2, double eps, bool decoupled) {
  const RunArgs ra{run_end, run_lr_mult, run_wd, base, arena_size};
  adam_launch("adam_flat_groups", w, g, m1, m2, shadow, c10::nullopt, lr, gscale, step, &ra, 0.0, beta1, beta2, eps,
              decoupled);
}

// Two-phase global-norm clip for the per-bucket optimizer (parallel/ddp.py): each gradient bucket's
// block partial sums of squares go to part[offset, offset + flat_grid(n)) as soon as that bucket's
// all-reduce completes; clip_coef_parts then reduces every bucket's partials in one launch.
void grad_sumsq_parts(const at::Tensor& g, at::Tensor part, int64_t offset) {
  PCMP_CHECK_F32(g); PCMP_CHECK_F32(part);
  const int64_t n = g.numel();
  TORCH_CHECK(n % 4 == 0, "grad_sumsq_parts: numel % 4");
  const int nb = flat_grid(n);
  TORCH_CHECK(offset >= 0 && offset + nb <= part.numel(), "grad_sumsq_parts: partial buffer too small");
  hipLaunchKernelGGL(sumsq_kernel, dim3(nb), dim3(256), 0, cur_stream(), ptr<float>(g), n, ptr<float>(part) + offset);
  PCMP_LAUNCH_CHECK();
}

// returns [norm, coef] device scalars (f32)
std::vector<at::Tensor> clip_coef_parts(const at::Tensor& part, double pre_scale, double max_norm, double post_scale) {
  PCMP_CHECK_F32(part);
  auto out = at::empty({2}, part.options());
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, cur_stream(), ptr<float>(part), (int)part.numel(),
                     (float)pre_scale, (float)max_norm, (float)post_scale, ptr<float>(out), ptr<float>(out) + 1);
  PCMP_LAUNCH_CHECK();
  return {out[0], out[1]};
}

// the whole gradient as one bucket
std::vector<at::Tensor> grad_clip_coef(const at::Tensor& g, double pre_scale, double max_norm, double post_scale) {
  auto part = at::empty({flat_grid(g.numel())}, g.options());
  grad_sumsq_parts(g, part, 0);
  return clip_coef_parts(part, pre_scale, max_norm, post_scale);
}

void cast_to_bf16(const at::Tensor& x, at::Tensor y) {
  PCMP_CHECK_F32(x); PCMP_CHECK_BF16(y);
  TORCH_CHECK(x.numel() == y.numel() && x.is_contiguous() && y.is_contiguous(), "cast_to_bf16: shapes");
  const int64_t n = x.numel();
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3((int)std::min<int64_t>(4096, (n + 255) / 256)), dim3(256), 0,
                     cur_stream(), ptr<float>(x), ptr<__bf16>(y), n);
  PCMP_LAUNCH_CHECK();
}

}  // namespace pcmp

TORCH_LIBRARY_FRAGMENT(pcmp, m) {
  m.def("sgd_flat(Tensor(a!) w, Tensor g, Tensor(b!) mom, Tensor(c!)? shadow, Tensor? mask, Tensor lr, Tensor? gscale, "
        "float momentum, float dampening, float wd, bool nesterov, bool first_step) -> ()",
        &pcmp::sgd_flat);
  m.def("adam_flat(Tensor(a!) w, Tensor g, Tensor(b!) m1, Tensor(c!) m2, Tensor(d!)? shadow, Tensor? mask, Tensor lr, "
        "Tensor? gscale, Tensor step, float beta1, float beta2, float eps, float wd, bool decoupled) -> ()",
        &pcmp::adam_flat);
  m.def("sgd_flat_groups(Tensor(a!) w, Tensor g, Tensor(b!) mom, Tensor(c!)? shadow, Tensor lr, Tensor? gscale, "
        "Tensor run_end, Tensor run_lr_mult, Tensor run_wd, int base, int arena_size, float momentum, float dampening, "
        "bool nesterov, bool first_step) -> ()",
        &pcmp::sgd_flat_groups);
  m.def("adam_flat_groups(Tensor(a!) w, Tensor g, Tensor(b!) m1, Tensor(c!) m2, Tensor(d!)? shadow, Tensor lr, "
        "Tensor? gscale, Tensor step, Tensor run_end, Tensor run_lr_mult, Tensor run_wd, int base, int arena_size, "
        "float beta1, float beta2, float eps, bool decoupled) -> ()",
        &pcmp::adam_flat_groups);
  m.def("grad_clip_coef(Tensor g, float pre_scale, float max_norm, float post_scale) -> Tensor[]",
        &pcmp::grad_clip_coef);
  m.def("grad_sumsq_parts(Tensor g, Tensor(a!) part, int offset) -> ()", &pcmp::grad_sumsq_parts);
  m.def("clip_coef_parts(Tensor part, float pre_scale, float max_norm, float post_scale) -> Tensor[]",
        &pcmp::clip_coef_parts);
  m.def("cast_to_bf16(Tensor x, Tensor(a!) y) -> ()", &pcmp::cast_to_bf16);
}
