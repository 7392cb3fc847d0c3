// Implicit-GEMM convolution / Linear: forward (FWD) entry points.
// The kernels live in igemm_kernels.h, launchers and dispatch in igemm_launch.h, the GEMM planner in
// igemm_plan.h (all three through igemm.h); this translation unit holds the
// FWD entry points (split from igemm.hip in round 4 so the three modes compile in parallel).
#include "igemm.h"
#include "bnr_stream.h"

namespace pcmp {

static Knob kn_fwd_split_target("fwd_split_target", 256);
static Knob kn_fwd_split_mink("fwd_split_mink", 4);

// The path of one conv_fwd call: decided here from the geometry, the operands present and the knobs;
// conv_fwd_impl executes it and fwd_kernel_choice formats it.
enum FwdPath {
  FWD_STREAM,         // expanding 1x1 conv with statistics: the streaming kernel (bnr_stream.h)
  FWD_FOLD,           // BatchNorm-forward fold (act_sc / act_sh): the fold's own tiles
  FWD_PLAN,           // plain GEMM: the planner
  FWD_PLAN_SMALL_M,   // small-M conv: the planner, starting from the heuristic split
  FWD_SPLIT,          // small-M conv without the planner: split-K dispatch + splitk_epilogue_kernel
  FWD_PLAIN,
};
// heur_split: FWD_PLAN_SMALL_M's heuristic split count; k: what FWD_FOLD / FWD_SPLIT / FWD_PLAIN launch
struct FwdRoute { int path, heur_split; KernelChoice k; };
// (FWD_SPLIT sets p.nsplit / p.ksplit: the kernel choice depends on them)
static FwdRoute fwd_route(IgemmParams& p, bool want_stats) {
  if (want_stats && use_fwd_stream(p)) return {FWD_STREAM};
  if (p.act_sc) return {FWD_FOLD, 1, choose_kernel(MODE_FWD, p, want_stats)};
  if (!want_stats && plain_gemm_eligible<MODE_FWD>(p)) return {FWD_PLAN, 1};
  // Small-M shapes (batch-1 inference: 49..3136 pixels) leave most of the 256 CUs idle; split the
  // reduction so the grid reaches ~256 workgroups, then reduce + epilogue in one pass.
  const int tiles = ceil_div(p.gm, default_bm(p)) * ceil_div(p.gn, default_bn(p));
  const int ksteps = ceil_div(p.gk, BK);
  if (!want_stats && tiles < 128 && ksteps >= 8) {
    // knobs fwd_split_target / fwd_split_mink: grid target and minimum K-steps per split (A/B-only knobs
    // of the round-1 heuristic; numerics at high split counts are covered by the plan_force small-M tests)
    const int split_target = std::max(1, kn_fwd_split_target.get());
    const int split_mink = std::max(1, kn_fwd_split_mink.get());
    const int nsplit = std::max(1, std::min({ceil_div(split_target, tiles), ksteps / split_mink, 32}));
    if (kn_gemm_plan.get()) return {FWD_PLAN_SMALL_M, nsplit};
    if (nsplit > 1) {
      set_split(p, nsplit, BK);
      return {FWD_SPLIT, nsplit, choose_kernel(MODE_FWD, p, false)};
    }
  }
  return {FWD_PLAIN, 1, choose_kernel(MODE_FWD, p, want_stats)};
}

// x: [N,H,W,C] bf16, w: [K,R,S,C] bf16 -> y [N,P,Q,K] bf16.  Optional bias (f32 [K]), residual
// (bf16 [N,P,Q,K]) and activation (act: IgemmParams::relu) fused; optional stats output
// [tiles_m,2,K] f32 (returned).  act 2 (GELU) also returns the pre-activation u.
static std::vector<at::Tensor> conv_fwd_impl(const at::Tensor& x, const at::Tensor& w, int64_t stride, int64_t pad,
                                             const c10::optional<at::Tensor>& bias,
                                             const c10::optional<at::Tensor>& resid, int act, bool want_stats,
                                             const at::Tensor* in_scale = nullptr, const at::Tensor* in_shift = nullptr) {
  PCMP_CHECK_CUDA(x); PCMP_CHECK_BF16(x); PCMP_CHECK_BF16(w);
  PCMP_CHECK_CONTIG(x); PCMP_CHECK_CONTIG(w);
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4, "conv_fwd: NHWC x and KRSC w expected");
  const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int K = w.size(0), R = w.size(1), S = w.size(2);
  TORCH_CHECK(w.size(3) == C, "conv_fwd: channel mismatch");
  TORCH_CHECK(C % 8 == 0 && K % 8 == 0, "conv_fwd: C and K must be multiples of 8");
  IgemmParams p;
  fill_geometry(p, N, H, W, C, K, R, S, stride, pad);
  p.gm = N * p.P * p.Q; p.gn = K; p.gk = R * S * C;
  TORCH_CHECK((int64_t)N * H * W * C < (1ll << 31) && (int64_t)p.gm * K < (1ll << 31), "conv_fwd: tensor too large");
  auto y = at::empty({N, p.P, p.Q, K}, x.options());
  p.a = ptr<__bf16>(x); p.b = ptr<__bf16>(w); p.out = y.data_ptr();
  p.a_bytes = tensor_bytes(x); p.b_bytes = tensor_bytes(w);
  if (bias.has_value() && bias->defined()) { PCMP_CHECK_F32(*bias); p.bias = ptr<float>(*bias); }
  if (resid.has_value() && resid->defined()) {
    PCMP_CHECK_BF16(*resid); PCMP_CHECK_CONTIG(*resid);
    TORCH_CHECK(resid->numel() == y.numel(), "conv_fwd: residual shape");
    p.resid = ptr<__bf16>(*resid);
  }
  p.relu = act;
  at::Tensor u;
  if (act == 2) {
    TORCH_CHECK(!want_stats, "conv_fwd: GELU epilogue without statistics");
    u = at::empty_like(y);
    p.aux = ptr<__bf16>(u);
  }
  p.ksplit = p.gk; p.nsplit = 1;
  if (in_scale) {   // BatchNorm-forward fold: the operand is relu(in_scale * x + in_shift)
    TORCH_CHECK(in_shift && R == 1 && S == 1 && stride == 1 && C % BK == 0 && act != 2,
                "conv_fwd: the input activation fold needs a 1x1 stride-1 conv with C % 64 == 0");
    for (const at::Tensor* t : {in_scale, in_shift}) {
      PCMP_CHECK_F32(*t); PCMP_CHECK_CONTIG(*t);
      TORCH_CHECK(t->numel() == C, "conv_fwd: in_scale / in_shift must hold C values");
    }
    p.act_sc = ptr<float>(*in_scale); p.act_sh = ptr<float>(*in_shift);
  }
  const FwdRoute r = fwd_route(p, want_stats);
  const auto fopts = x.options().dtype(at::kFloat);
  auto st = cur_stream();
  at::Tensor stats;
  if (want_stats) {   // one partial row per workgroup group (stream) or per row tile of the chosen kernel
    p.stats_cap = r.path == FWD_STREAM ? fwd_stream_groups(p) : ceil_div(p.gm, r.k.bm);
    stats = at::empty({p.stats_cap, 2, K}, fopts);
    p.stats = ptr<float>(stats);
  }
  if (r.path == FWD_STREAM) {
    launch_fwd_stream(p, st);
  } else if (r.path == FWD_PLAN || r.path == FWD_PLAN_SMALL_M) {
    const GemmPlan pl = plan_gemm<MODE_FWD>(p, ptr<__bf16>(y), fopts, st, r.path == FWD_PLAN_SMALL_M, r.heur_split);
    run_plan<MODE_FWD>(p, pl, ptr<__bf16>(y), fopts, st);
  } else if (r.path == FWD_SPLIT) {
    const int64_t n = (int64_t)p.gm * p.gn;
    auto ws = at::empty({(int64_t)p.nsplit, n}, fopts);
    p.out = ws.data_ptr();
    dispatch<MODE_FWD>(p, r.k, st);
    const int blocks = (int)((n / 4 + 255) / 256);
    hipLaunchKernelGGL(splitk_epilogue_kernel, dim3(blocks), dim3(256), 0, st, ptr<float>(ws), ptr<__bf16>(y),
                       p.bias, p.resid, n, p.gn, p.nsplit, p.relu, p.aux);
    PCMP_LAUNCH_CHECK();
  } else {
    dispatch<MODE_FWD>(p, r.k, st);
  }
  if (want_stats) return {y, stats};
  return act == 2 ? std::vector<at::Tensor>{y, u} : std::vector<at::Tensor>{y};
}

// conv_kernel_choice, FWD: the route of conv_fwd_impl for a shape, as a tag.  flags: 1 statistics,
// 2 bias, 4 residual, 8 ReLU, 16 the input activation fold, 32 the GELU epilogue of linear_gelu_fwd
// (act 2 with the pre-activation output; not with statistics, ReLU or the fold).  Launches nothing.
std::string fwd_kernel_choice(int N, int H, int W, int C, int K, int R, int stride, int pad, int flags) {
  TORCH_CHECK(!(flags & 32) || !(flags & (1 | 8 | 16)),
              "conv_kernel_choice: FWD flag 32 (GELU) excludes flags 1, 8 and 16");
  IgemmParams p;
  fill_geometry(p, N, H, W, C, K, R, R, stride, pad);
  p.gm = N * p.P * p.Q; p.gn = K; p.gk = R * R * C;
  p.a = p.b = nullptr; p.a_bytes = p.b_bytes = 0; p.out = nullptr;
  const uintptr_t some = 16;   // operands the predicates only test for presence
  if (flags & 2) p.bias = reinterpret_cast<const float*>(some);
  if (flags & 4) p.resid = reinterpret_cast<const __bf16*>(some);
  p.relu = (flags & 8) ? 1 : 0;
  if (flags & 32) { p.relu = 2; p.aux = reinterpret_cast<__bf16*>(some); }
  p.ksplit = p.gk; p.nsplit = 1;
  if (flags & 16) { p.act_sc = reinterpret_cast<const float*>(some); p.act_sh = p.act_sc; }
  const FwdRoute r = fwd_route(p, flags & 1);
  switch (r.path) {
    case FWD_STREAM: return "fwd_stream/32x" + std::to_string(fwd_stream_bn(p));
    case FWD_PLAN: return plan_tag<MODE_FWD>(p);
    case FWD_PLAN_SMALL_M: return plan_tag<MODE_FWD>(p, true, r.heur_split);
    case FWD_SPLIT: return choice_tag(MODE_FWD, r.k) + "/ns" + std::to_string(p.nsplit);
    default: return choice_tag(MODE_FWD, r.k);
  }
}

std::vector<at::Tensor> conv_fwd(const at::Tensor& x, const at::Tensor& w, int64_t stride, int64_t pad,
                                 const c10::optional<at::Tensor>& bias,
                                 const c10::optional<at::Tensor>& resid, bool relu, bool want_stats,
                                 const c10::optional<at::Tensor>& in_scale, const c10::optional<at::Tensor>& in_shift) {
  const bool fold = in_scale.has_value() && in_scale->defined();
  TORCH_CHECK(!fold || (in_shift.has_value() && in_shift->defined()), "conv_fwd: in_shift required with in_scale");
  if (x.scalar_type() == at::kFloat)
    return f32::conv_fwd(x, w, stride, pad, bias, resid, relu, want_stats, fold ? &*in_scale : nullptr,
                         fold ? &*in_shift : nullptr);
  return conv_fwd_impl(x, w, stride, pad, bias, resid, relu ? 1 : 0, want_stats, fold ? &*in_scale : nullptr,
                       fold ? &*in_shift : nullptr);
}

// Linear y = gelu(x W^T + b) with the GELU fused into the GEMM epilogue: x [M, C], w [N, C] bf16
// -> [gelu(u), u] (u = x W^T + b, kept for the backward).  BERT's FFN up-projection
// (pytorch_on_language_distr.py:151-161 via BertIntermediate).
std::vector<at::Tensor> linear_gelu_fwd(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias) {
  if (x.scalar_type() == at::kFloat) return f32::linear_gelu_fwd(x, w, bias);
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(1) == w.size(1), "linear_gelu_fwd: x [M, C], w [N, C]");
  const int64_t M = x.size(0), C = x.size(1), N = w.size(0);
  auto r = conv_fwd_impl(x.view({M, 1, 1, C}), w.view({N, 1, 1, C}), 1, 0, bias, c10::nullopt, 2, false);
  return {r[0].view({M, N}), r[1].view({M, N})};
}

// Timings of every planner candidate for one conv_fwd call (reports / kernel tuning): runs the
// planner uncached with its log enabled.
std::vector<std::string> plan_candidates(const at::Tensor& x, const at::Tensor& w, int64_t stride, int64_t pad,
                                         const c10::optional<at::Tensor>& bias, const c10::optional<at::Tensor>& resid,
                                         bool relu) {
  std::vector<std::string> log;
  const int old = kn_plan_force.value.exchange(99);   // 99: no such kind -> every candidate, uncached
  g_plan_log = &log;
  try {
    conv_fwd(x, w, stride, pad, bias, resid, relu, false, c10::nullopt, c10::nullopt);
  } catch (...) {
    g_plan_log = nullptr;
    kn_plan_force.value.store(old);
    throw;
  }
  g_plan_log = nullptr;
  kn_plan_force.value.store(old);
  return log;
}

}  // namespace pcmp
