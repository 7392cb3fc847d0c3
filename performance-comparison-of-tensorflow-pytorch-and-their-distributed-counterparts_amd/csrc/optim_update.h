// The flat optimizers' shared text: the device scalars, the one definition of each element update
// (sgd_update / adam_update) and the host checks every optimizer op goes through.  Included by
// optim.hip (sgd_flat / adam_flat and their grouped forms) and optim_layerwise.hip (lars_flat /
// lamb_flat).
#pragma once
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

// ---------------------------------------------------------------------------------- host checks
// Shared by every optimizer op; a refused call launches nothing.
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

}  // namespace pcmp
