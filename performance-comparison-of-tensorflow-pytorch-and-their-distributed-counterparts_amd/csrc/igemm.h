// Implicit-GEMM convolution / Linear: the one include of the igemm translation units and of
// bnr_stream.h / wgrad32.h.  Device code (the MFMA kernels) is igemm_kernels.h, launchers, the kernel
// choice (choose_kernel) and dispatch<> are igemm_launch.h, the plain-GEMM planner is igemm_plan.h;
// below are the helpers and entry points the translation units share.
#pragma once
#include "igemm_plan.h"

namespace pcmp {

static unsigned tensor_bytes(const at::Tensor& t) {
  const int64_t b = t.numel() * t.element_size();
  TORCH_CHECK(b < (1ll << 31), "igemm: operand larger than 2 GiB (buffer-resource range)");
  return (unsigned)b;
}

static void fill_geometry(IgemmParams& p, int N, int H, int W, int C, int K, int R, int S,
                          int stride, int pad) {
  p.N = N; p.H = H; p.W = W; p.C = C; p.K = K; p.R = R; p.S = S;
  p.stride = stride; p.pad = pad;
  p.P = (H + 2 * pad - R) / stride + 1;
  p.Q = (W + 2 * pad - S) / stride + 1;
  p.fd_PQ = make_fastdiv(p.P * p.Q);
  p.fd_Q = make_fastdiv(p.Q);
  p.fd_HW = make_fastdiv(H * W);
  p.fd_W = make_fastdiv(W);
  p.dH = H; p.dW = W; p.offy = pad; p.offx = pad; p.sub = 0; p.oph = 0; p.opw = 0;
  p.bias = nullptr; p.resid = nullptr; p.aux = nullptr; p.stats = nullptr; p.stats2 = nullptr;
  p.bn_mask = nullptr; p.bn_x = nullptr; p.bn_mean = nullptr; p.bn_istd = nullptr;
  p.bn_x2 = nullptr; p.bn_mean2 = nullptr; p.bn_istd2 = nullptr; p.bn_msc = nullptr; p.bn_msh = nullptr;
  p.bn_mbits = nullptr;
  p.stats_cap = 0;
  p.relu = 0; p.alpha = 1.f; p.accumulate = 0; p.nsplit = 1;
  p.fold_x = nullptr; p.fold_coef = nullptr; p.fold_lds = 0;
  p.act_sc = nullptr; p.act_sh = nullptr;
  p.resid_sub = 0; p.rs_H2 = 0; p.rs_W2 = 0;
}

// ---- entry points (igemm_fwd.hip / igemm_dgrad.hip / igemm_wgrad.hip; registered in igemm.hip)
std::vector<at::Tensor> conv_fwd(const at::Tensor& x, const at::Tensor& w, int64_t stride, int64_t pad,
                                 const c10::optional<at::Tensor>& bias,
                                 const c10::optional<at::Tensor>& resid, bool relu, bool want_stats,
                                 const c10::optional<at::Tensor>& in_scale, const c10::optional<at::Tensor>& in_shift);
std::vector<std::string> plan_candidates(const at::Tensor& x, const at::Tensor& w, int64_t stride, int64_t pad,
                                         const c10::optional<at::Tensor>& bias, const c10::optional<at::Tensor>& resid,
                                         bool relu);
std::vector<at::Tensor> linear_gelu_fwd(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias);
at::Tensor conv_dgrad(const at::Tensor& dy, const at::Tensor& w, int64_t H, int64_t W, int64_t stride, int64_t pad,
                      const c10::optional<at::Tensor>& resid, const c10::optional<at::Tensor>& wt);
at::Tensor linear_dgrad_gelu(const at::Tensor& dy, const at::Tensor& w, const at::Tensor& u,
                             const c10::optional<at::Tensor>& wt);
std::vector<at::Tensor> conv_dgrad_bnr(const at::Tensor& dy, const at::Tensor& w, int64_t H, int64_t W,
                                       int64_t stride, int64_t pad, const c10::optional<at::Tensor>& resid,
                                       const c10::optional<at::Tensor>& ymask, const at::Tensor& x,
                                       const at::Tensor& mean, const at::Tensor& invstd,
                                       const c10::optional<at::Tensor>& x2, const c10::optional<at::Tensor>& mean2,
                                       const c10::optional<at::Tensor>& invstd2, const c10::optional<at::Tensor>& mscale,
                                       const c10::optional<at::Tensor>& mshift, const c10::optional<at::Tensor>& wt,
                                       const c10::optional<at::Tensor>& ymask_bits,
                                       const c10::optional<at::Tensor>& fold_x,
                                       const c10::optional<at::Tensor>& fold_coef, bool resid_sub);
void conv_wgrad(const at::Tensor& dy, const at::Tensor& x, at::Tensor out, int64_t R, int64_t S,
                int64_t stride, int64_t pad, bool accumulate, const c10::optional<at::Tensor>& fold_x,
                const c10::optional<at::Tensor>& fold_coef, const c10::optional<at::Tensor>& in_scale,
                const c10::optional<at::Tensor>& in_shift);
std::vector<at::Tensor> conv1x1_bwd_fused(const at::Tensor& g, const c10::optional<at::Tensor>& fold_x,
                                          const c10::optional<at::Tensor>& fold_coef, const at::Tensor& wt,
                                          const at::Tensor& z, const at::Tensor& scale, const at::Tensor& shift,
                                          const at::Tensor& mean, const at::Tensor& invstd, at::Tensor dw,
                                          bool accumulate);
// the conv_kernel_choice op's halves: each formats the route its entry point executes
std::string fwd_kernel_choice(int N, int H, int W, int C, int K, int R, int stride, int pad, int flags);
std::string dgrad_kernel_choice(int N, int H, int W, int C, int K, int R, int stride, int pad, int flags);
std::string wgrad_kernel_choice(int N, int H, int W, int C, int K, int R, int stride, int pad, int flags);

}  // namespace pcmp
