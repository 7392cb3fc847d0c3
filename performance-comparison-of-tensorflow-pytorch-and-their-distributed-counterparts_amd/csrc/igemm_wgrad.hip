// Implicit-GEMM convolution / Linear: weight-gradient (WGRAD) entry points.
// The kernels live in igemm_kernels.h, launchers and dispatch in igemm_launch.h, the GEMM planner in
// igemm_plan.h (all three through igemm.h); this translation unit holds the
// WGRAD entry points (split from igemm.hip in round 4 so the three modes compile in parallel).
#include "igemm.h"
#include "wgrad32.h"

namespace pcmp {

// split-K WGRAD on the chosen kernel: partial dW per split into a workspace, then one deterministic
// reduction pass
static void wgrad_run(IgemmParams p, const KernelChoice& c, int nsplit, float* out, bool accumulate,
                      const at::TensorOptions& fopts, hipStream_t st) {
  set_split(p, nsplit, BK);
  nsplit = p.nsplit;
  auto launch = [&] {
    if (c.family == KF_WGRAD_DMA32) launch_wgrad_dma32(p, c, st); else dispatch<MODE_WGRAD>(p, c, st);
  };
  if (nsplit == 1) {
    p.out = out;
    p.accumulate = accumulate;
    launch();
    return;
  }
  const int64_t n = (int64_t)p.gm * p.gn;
  TORCH_CHECK(n % 4 == 0, "conv_wgrad: numel % 4");
  auto ws = at::empty({(int64_t)nsplit, n}, fopts);
  p.out = ws.data_ptr();
  p.accumulate = 0;
  launch();
  if (n / 4 < (1ll << 31)) {
    launch_splitk_reduce2(ptr<float>(ws), out, (int)(n / 4), nsplit, accumulate, st);
    return;
  }
  const int blocks = (int)std::min<int64_t>(2048, (n / 4 + 255) / 256);
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, st, ptr<float>(ws), out, n, nsplit,
                     (int)accumulate);
  PCMP_LAUNCH_CHECK();
}

// The split count of a WGRAD for a workgroup target, on the tile of its chosen kernel.  Split cap:
// 256, or wgrad_cap_few for GEMMs of <= 4 output tiles (the stem WGRAD: one 64x256 tile over 3.2 M
// reduction rows, alone on the chip at the end of backward -- 256 splits are one 4-wave workgroup per CU).
static Knob kn_wgrad_cap_few("wgrad_cap_few", 1024);
struct WgradSplits {
  int tiles, ksteps, cap;
  WgradSplits(const IgemmParams& p, const KernelChoice& c)
      : tiles(ceil_div(p.gm, c.bm) * ceil_div(p.gn, c.bn)), ksteps(ceil_div(p.gk, BK)),
        cap(tiles <= 4 ? std::max(256, kn_wgrad_cap_few.get()) : 256) {}
  int for_target(int target) const { return std::max(1, std::min(std::min(ceil_div(target, tiles), ksteps / 8), cap)); }
};
// A fixed workgroup target, or 0 where the split count is timed.  PCMP_WGRAD_WGS (read once) goes first;
// then the knob wgrad_wgs: WGRADs launched on the side stream (ops/params.py run_on_side sets the knob
// around them) share the CUs with the DGRAD chain, and there a fixed 384-workgroup target beats the
// isolated autotune (ResNet-50 step +0.5-0.7 %, 3 of 3 interleaved rounds, profiles/r2_knob_sweep.txt sweep 6)
static int wgrad_fixed_target() {
  static const int env = [] {
    const char* e = std::getenv("PCMP_WGRAD_WGS");
    return e ? std::max(64, std::atoi(e)) : 0;
  }();
  if (env) return env;
  return kn_wgrad_wgs.get() > 0 ? std::max(64, kn_wgrad_wgs.get()) : 0;
}

// WGRAD split-K autotuning (cudnn.benchmark-style): the best split count of a shape depends on tile
// quantisation against 256 CUs and on the workspace traffic of the reduction, and measured
// non-monotonically (profiles/r1_wgrad_splitk_ab.txt), so the first call of each shape times a few
// grid targets on a scratch output and caches the fastest.  Never while a graph is being captured.
// PCMP_AUTOTUNE=0 (or an explicit PCMP_WGRAD_WGS) keeps the static 1024-workgroup target, which
// also keeps runs bitwise reproducible (a tuned split count changes the summation order).
static int wgrad_nsplit(const IgemmParams& p, const KernelChoice& c, const at::TensorOptions& fopts, hipStream_t st) {
  const WgradSplits sp(p, c);
  if (const int fixed_target = wgrad_fixed_target()) return sp.for_target(fixed_target);
  static const bool tune = [] {
    const char* e = std::getenv("PCMP_AUTOTUNE");
    return !(e && std::atoi(e) == 0);
  }();
  const int dflt = sp.for_target(1024);
  if (!tune) return dflt;
  auto& mu = g_plan_mu;
  auto& cache = g_wsplit_cache;
  char key[160];
  snprintf(key, sizeof(key), "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d%s", p.N, p.H, p.W, p.C, p.K, p.R, p.S, p.stride, p.pad,
           sp.cap, c.family == KF_WGRAD_DMA32 ? ",d32" : "");
  {
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;   // a graph captured after warm-up keeps the tuned split
  }
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return dflt;
  std::vector<int> cands;
  for (int t : {64, 128, 256, 512, 768, 1024, 1536, 2048, 3072, 4096}) {
    const int ns = sp.for_target(t);
    if (std::find(cands.begin(), cands.end(), ns) == cands.end()) cands.push_back(ns);
  }
  int best = dflt;
  if (cands.size() > 1) {
    auto scratch = at::empty({(int64_t)p.gm * p.gn}, fopts);
    hipEvent_t e0, e1;
    PCMP_HIP_CHECK(hipEventCreate(&e0));
    PCMP_HIP_CHECK(hipEventCreate(&e1));
    float best_ms = 1e30f;
    for (int ns : cands) {
      wgrad_run(p, c, ns, ptr<float>(scratch), false, fopts, st);   // warm (workspace allocation, caches)
      PCMP_HIP_CHECK(hipEventRecord(e0, st));
      for (int r = 0; r < 3; ++r) wgrad_run(p, c, ns, ptr<float>(scratch), false, fopts, st);
      PCMP_HIP_CHECK(hipEventRecord(e1, st));
      PCMP_HIP_CHECK(hipEventSynchronize(e1));
      float ms = 0.f;
      PCMP_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
      if (ms < best_ms) { best_ms = ms; best = ns; }
    }
    PCMP_HIP_CHECK(hipEventDestroy(e0));
    PCMP_HIP_CHECK(hipEventDestroy(e1));
  }
  std::lock_guard<std::mutex> g(mu);
  cache.emplace(key, best);
  return best;
}

// conv_kernel_choice, WGRAD: conv_wgrad's kernel, tile and split count for a shape, as a tag
// "<kernel>/<BM>x<BN>/ns<splits>"; "/nsauto" where the split count is timed (no wgrad_wgs knob, no
// PCMP_WGRAD_WGS).  flags: 1 the dz fold, 2 the activation fold.  Launches nothing.
std::string wgrad_kernel_choice(int N, int H, int W, int C, int K, int R, int stride, int pad, int flags) {
  IgemmParams p;
  fill_geometry(p, N, H, W, C, K, R, R, stride, pad);
  p.a = p.b = nullptr; p.a_bytes = p.b_bytes = 0; p.out = nullptr;
  p.gm = K; p.gn = R * R * C; p.gk = N * p.P * p.Q;
  const uintptr_t some = 16;   // operands the predicates only test for presence
  if (flags & 1) { p.fold_x = reinterpret_cast<const __bf16*>(some); p.fold_coef = reinterpret_cast<const float*>(some); }
  if (flags & 2) { p.act_sc = reinterpret_cast<const float*>(some); p.act_sh = p.act_sc; }
  const KernelChoice c = choose_kernel(MODE_WGRAD, p);
  const int target = wgrad_fixed_target();
  if (!target) return choice_tag(MODE_WGRAD, c) + "/nsauto";
  set_split(p, WgradSplits(p, c).for_target(target), BK);
  return choice_tag(MODE_WGRAD, c) + "/ns" + std::to_string(p.nsplit);
}

// dy: [N,P,Q,K], x: [N,H,W,C] -> writes dW (f32, [K,R,S,C]) into `out` (accumulate optional).
void conv_wgrad(const at::Tensor& dy, const at::Tensor& x, at::Tensor out, int64_t R, int64_t S,
                int64_t stride, int64_t pad, bool accumulate, const c10::optional<at::Tensor>& fold_x,
                const c10::optional<at::Tensor>& fold_coef, const c10::optional<at::Tensor>& in_scale,
                const c10::optional<at::Tensor>& in_shift) {
  const bool fold = fold_x.has_value() && fold_x->defined();
  const bool afold = in_scale.has_value() && in_scale->defined();
  TORCH_CHECK(!fold || dy.scalar_type() != at::kFloat, "conv_wgrad: the BatchNorm-backward fold is bf16 only");
  if (dy.scalar_type() == at::kFloat)
    return f32::conv_wgrad(dy, x, out, R, S, stride, pad, accumulate, afold ? &*in_scale : nullptr,
                           afold ? &*in_shift : nullptr);
  PCMP_CHECK_CUDA(dy); PCMP_CHECK_BF16(dy); PCMP_CHECK_BF16(x);
  PCMP_CHECK_CONTIG(dy); PCMP_CHECK_CONTIG(x); PCMP_CHECK_F32(out); PCMP_CHECK_CONTIG(out);
  const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3), K = dy.size(3);
  IgemmParams p;
  fill_geometry(p, N, H, W, C, K, R, S, stride, pad);
  TORCH_CHECK(dy.size(1) == p.P && dy.size(2) == p.Q, "conv_wgrad: dy shape");
  TORCH_CHECK(out.numel() == (int64_t)K * R * S * C, "conv_wgrad: out numel");
  p.gm = K; p.gn = R * S * C; p.gk = N * p.P * p.Q;
  p.a = ptr<__bf16>(dy); p.b = ptr<__bf16>(x);
  p.a_bytes = tensor_bytes(dy); p.b_bytes = tensor_bytes(x);
  if (fold) {   // dy operand = k1*g + k2*fold_x + k3 (dy passed as g)
    PCMP_CHECK_BF16(*fold_x); PCMP_CHECK_CONTIG(*fold_x);
    TORCH_CHECK(fold_x->numel() == dy.numel(), "conv_wgrad: fold_x must have dy's shape");
    TORCH_CHECK(fold_coef.has_value() && fold_coef->defined(), "conv_wgrad: fold_coef required with fold_x");
    PCMP_CHECK_F32(*fold_coef); PCMP_CHECK_CONTIG(*fold_coef);
    TORCH_CHECK(fold_coef->numel() == 3 * (int64_t)K, "conv_wgrad: fold_coef must be [3, K]");
    p.fold_x = ptr<__bf16>(*fold_x); p.fold_coef = ptr<float>(*fold_coef);
  }
  if (afold) {   // x operand = relu(in_scale * x + in_shift) (x passed as the pre-BN tensor)
    TORCH_CHECK(in_shift.has_value() && in_shift->defined(), "conv_wgrad: in_shift required with in_scale");
    for (const at::Tensor* t : {&*in_scale, &*in_shift}) {
      PCMP_CHECK_F32(*t); PCMP_CHECK_CONTIG(*t);
      TORCH_CHECK(t->numel() == C, "conv_wgrad: in_scale / in_shift must hold C values");
    }
    p.act_sc = ptr<float>(*in_scale); p.act_sh = ptr<float>(*in_shift);
  }
  const KernelChoice c = choose_kernel(MODE_WGRAD, p);   // (does not depend on the split count)
  auto st = cur_stream();
  const int nsplit = wgrad_nsplit(p, c, out.options(), st);
  wgrad_run(p, c, nsplit, ptr<float>(out), accumulate, out.options(), st);
}

}  // namespace pcmp
