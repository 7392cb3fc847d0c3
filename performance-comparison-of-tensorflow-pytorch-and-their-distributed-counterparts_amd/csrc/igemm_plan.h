// Plain-GEMM planner over the launchers of igemm_launch.h: the plan knobs, GemmPlan, run_plan,
// plan_gemm and the plan / split-count caches.
#pragma once
#include "igemm_launch.h"

#include <mutex>
#include <unordered_map>

namespace pcmp {

// ------------------------------------------------------------------------------------------------
// Plain-GEMM planner: a stride-1 1x1 convolution without a BatchNorm epilogue is a plain GEMM
// (every Linear layer: BERT-base's M = 4096-token projections, the VGG16 classifier, the transfer
// heads).  Those shapes have too few 128x128 / 256x256 tiles to fill 256 CUs (BERT's N = 768
// outputs: 48 tiles of 256x256), so the first call of each shape times a small candidate set --
// the 4-wave LDS-DMA kernel (128x128, 2 blocks/CU) and the 8-wave one (256x256, 1 block/CU), each
// with 1..6 K-splits whose fp32 partials are reduced by splitk_epilogue_kernel (bias / residual /
// ReLU fused there) -- and caches the fastest (cudnn.benchmark-style; never while a graph is being
// captured).  This replaces the round-1 hipBLASLt candidate for these GEMMs.
inline Knob kn_gemm_plan("gemm_plan", 1);   // 0 = default dispatch only, 1 = autotuned plan
inline Knob kn_plan_force("plan_force", -1); // tests: >= 0 restricts the candidates to that kind (uncached)
inline Knob kn_gemm32("gemm32", 1);          // 32x32x16-MFMA plain-GEMM candidates (plan kinds 9 / 10)
inline Knob kn_plan_nsplit("plan_nsplit", 0); // tests: >= 1 (with plan_force) also pins the split count
// a split candidate must beat the best by this many us per call to be chosen: its extra
// splitk_epilogue launch is host time the isolated timing does not see (BERT-base's eager step is
// host-bound: 56 split epilogues per step in round 4, verdict r4 weak #6)
inline Knob kn_plan_split_us("plan_split_us", 6);
// small-M (inference) plans are timed with the caches cold: a 64 MB memset before every timed call
// evicts the L2s.  Timed back to back, a conv's weights (0.1-4.7 MB at batch 1) stay L2-resident
// from the previous call and the tuner favoured kernels with one K-step in flight; inside the
// batch-1 graph every conv streams its weights from the MALL / HBM.  0 = the warm timing.
inline Knob kn_plan_cold("plan_cold", 1);

struct GemmPlan {
  int kind;     // 0 = default dispatch<>, 1 = DMA 128x128, 2 = DMA 256x256 (8 waves),
                // 3 = register-staged 64x64, 4 = register-staged 32x64, 5 = DMA 128x64 (small-M inference convs),
                // 6 = skinny FWD, 9 / 10 = 32x32x16 gemm32 128x128 / 256x256 (7 / 8: round 4 big kernel, removed)
  int nsplit;
};
static const char* plan_kind_name(int k) {
  switch (k) {
    case 1: return "dma128x128";
    case 2: return "dma256x256";
    case 3: return "reg64x64";
    case 4: return "reg32x64";
    case 5: return "dma128x64";
    case 6: return "skinny64x64";
    case 9: return "m32_128x128";
    case 10: return "m32_256x256";
    default: return "default";
  }
}

template <int MODE>
static void run_plan(IgemmParams p, const GemmPlan& pl, __bf16* out, const at::TensorOptions& fopts, hipStream_t st) {
  set_split(p, pl.nsplit, pl.kind == 6 ? 32 : BK);   // K granularity of the kernel
  const int nsplit = p.nsplit;
  const __bf16* resid = p.resid;
  at::Tensor ws;
  if (nsplit > 1) {
    ws = at::empty({(int64_t)nsplit, (int64_t)p.gm * p.gn}, fopts);
    p.out = ws.data_ptr();
  } else {
    p.out = out;
  }
  if (pl.kind == 1) launch_dma<MODE, 128, 128, 2, 2, NT, 2>(p, st);
  else if (pl.kind == 2) launch_dma<MODE, 256, 256, 2, 4, NT8, 1>(p, st);
  else if (pl.kind == 3) launch_cfg<MODE, 64, 64, 2, 2>(p, st);
  else if (pl.kind == 4) launch_cfg<MODE, 32, 64, 1, 4>(p, st);
  else if (pl.kind == 5) launch_dma<MODE, 128, 64, 2, 2, NT, 2>(p, st);
  else if (pl.kind == 9) launch_gemm32<128, 128, 2, 2, 2>(p, st);
  else if (pl.kind == 10) launch_gemm32<256, 256, 2, 2, 1>(p, st);
  else if (pl.kind == 6) {
    if constexpr (MODE == MODE_FWD) launch_skinny(p, st);
    else TORCH_CHECK(false, "skinny kernel is FWD only");
  } else dispatch<MODE>(p, st);
  if (nsplit > 1) {
    const int64_t n = (int64_t)p.gm * p.gn;
    const int blocks = (int)((n / 4 + 255) / 256);
    hipLaunchKernelGGL(splitk_epilogue_kernel, dim3(blocks), dim3(256), 0, st, ptr<float>(ws), out,
                       MODE == MODE_FWD ? p.bias : nullptr, resid, n, p.gn, nsplit, p.relu, p.aux);
    PCMP_LAUNCH_CHECK();
  }
}

template <int MODE>
static bool plain_gemm_eligible(const IgemmParams& p) {
  const int cin = MODE == MODE_FWD ? p.C : p.K;
  return kn_gemm_plan.get() && p.R == 1 && p.S == 1 && p.stride == 1 && p.pad == 0 && !p.stats && !p.bn_x &&
         p.gm >= 1024 && p.gk % BK == 0 && cin % BK == 0 && p.gn % 8 == 0 && p.gk / BK >= 4;
}

inline std::mutex g_plan_mu;
inline std::unordered_map<std::string, GemmPlan> g_plan_cache;
// wgrad_nsplit's tuned split counts (same mutex)
inline std::unordered_map<std::string, int> g_wsplit_cache;
inline std::vector<std::string>* g_plan_log = nullptr;   // candidate timings (plan_candidates op)

std::vector<std::string> gemm_plans();

// The candidates plan_gemm times for a shape: the default dispatch first, then the kinds and split
// counts the shape admits, restricted by the test knobs plan_force / plan_nsplit where a candidate
// matches them (plan_gemm and conv_kernel_choice's plan_tag share this list).
template <int MODE>
static std::vector<GemmPlan> plan_candidate_list(const IgemmParams& p, bool small_m, int heur_split) {
  const int force = kn_plan_force.get();
  GemmPlan dflt{0, small_m ? heur_split : 1};
  const int ksteps = ceil_div(p.gk, BK);
  std::vector<GemmPlan> cands{dflt};
  if (small_m) {
    // the LDS-DMA kernels keep 2-3 half-tiles of operands in flight (the register-staged ones one
    // K-step), which matters when a block's few K-steps are latency-bound; they need the
    // block-uniform tap walk
    const int cin = MODE == MODE_FWD ? p.C : p.K;
    const bool dma_ok = p.gk % BK == 0 && cin % BK == 0;
    for (int ns : {1, 2, 4, 8, 12, 16, 24, 32}) {
      if (ns > 1 && ksteps / ns < 2) continue;
      for (int kind : {0, 3, 4, 1, 5}) {
        if (kind == 0 && ns == heur_split) continue;
        if (kind == 4 && p.gm > 256) continue;
        if ((kind == 1 || kind == 5) && (!dma_ok || ceil_div(ksteps, ns) < 2)) continue;
        if (kind == 5 && p.gn > 1024) continue;
        cands.push_back({kind, ns});
      }
      if (MODE == MODE_FWD && p.relu < 2 && p.C % 32 == 0 && p.gk % 32 == 0 && p.gn % 4 == 0 && p.gm <= 1024 &&
          p.gk / 32 / ns >= 2)
        cands.push_back({6, ns});
    }
  } else {
    for (int ns : {1, 2, 3, 4, 6}) {
      if (ns > 1 && ksteps / ns < 4) continue;
      cands.push_back({1, ns});
      // 128x64 tiles: twice the 128x128 grid for N <= 1024 (BERT's N = 768 GEMMs: 384 tiles, not 192)
      if (p.gn <= 1024) cands.push_back({5, ns});
      if (kn_gemm32.get() && p.gn % 4 == 0) {   // 32x32x16 MFMA kernels
        cands.push_back({9, ns});
        if (p.gn >= 256) cands.push_back({10, ns});
      }
      if (p.gn >= 256) cands.push_back({2, ns});
    }
  }
  if (force >= 0) {
    std::vector<GemmPlan> f;
    for (const GemmPlan& c : cands)
      if (c.kind == force) f.push_back(c);
    if (!f.empty()) cands = f;
    if (kn_plan_nsplit.get() > 0) {   // a pinned split count makes repeated forced calls bitwise comparable
      f.clear();
      for (const GemmPlan& c : cands)
        if (c.nsplit == kn_plan_nsplit.get()) f.push_back(c);
      if (!f.empty()) cands = f;
    }
  }
  return cands;
}

// conv_kernel_choice's tag of a GEMM that goes through plan_gemm: "plan/auto" where the choice is
// timed; "plan/<kind>" or "plan/<kind>/ns<split>" where the test knobs leave candidates of one kind
// (and one split count) only.  A forced kind or split the shape has no candidate for leaves the
// unrestricted list, hence "plan/auto": a case pinned to a kernel then fails its tag.
template <int MODE>
static std::string plan_tag(const IgemmParams& p, bool small_m = false, int heur_split = 1) {
  if (kn_plan_force.get() < 0) return "plan/auto";
  const std::vector<GemmPlan> cands = plan_candidate_list<MODE>(p, small_m, heur_split);
  bool one_kind = true, one_split = true;
  for (const GemmPlan& c : cands) {
    one_kind = one_kind && c.kind == cands[0].kind;
    one_split = one_split && c.nsplit == cands[0].nsplit;
  }
  if (!one_kind) return "plan/auto";
  std::string t = std::string("plan/") + plan_kind_name(cands[0].kind);
  if (one_split) t += "/ns" + std::to_string(cands[0].nsplit);
  return t;
}

// small_m: an inference-sized convolution (few output tiles, long reduction): the candidates are
// the register-staged kernels at 128/64/32-row tiles with 1..32 K-splits (the split partials are
// reduced by splitk_epilogue_kernel together with bias / residual / ReLU), plus the round-1
// heuristic (default tile, heur_split splits) so the plan is never a regression by construction.
template <int MODE>
static GemmPlan plan_gemm(const IgemmParams& p, __bf16* out, const at::TensorOptions& fopts, hipStream_t st,
                          bool small_m = false, int heur_split = 1) {
  auto& mu = g_plan_mu;
  auto& cache = g_plan_cache;
  char key[192];
  snprintf(key, sizeof(key), "%d,%d,%d,%d,%d,%d,%d|%d,%d,%d,%d,%d,%d,%d,%d,%d", MODE, p.gm, p.gn, p.gk,
           p.bias != nullptr, p.resid != nullptr, p.relu, p.N, p.H, p.W, p.C, p.K, p.R, p.S, p.stride, p.pad);
  const int force = kn_plan_force.get();
  if (force < 0) {
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
  }
  GemmPlan dflt{0, small_m ? heur_split : 1};
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return dflt;
  std::vector<GemmPlan> cands = plan_candidate_list<MODE>(p, small_m, heur_split);
  hipEvent_t e0, e1;
  PCMP_HIP_CHECK(hipEventCreate(&e0));
  PCMP_HIP_CHECK(hipEventCreate(&e1));
  GemmPlan best = cands[0];
  float best_ms = 1e30f;
  const bool cold = small_m && kn_plan_cold.get();
  // the cache-evicting scratch of the cold timing: allocated once, never freed (no tensor destructor
  // runs at process exit, after the HIP runtime may be gone)
  static at::Tensor* flush = nullptr;
  if (cold && flush == nullptr) flush = new at::Tensor(at::empty({64 << 20}, fopts.dtype(at::kByte)));
  auto consider = [&](const GemmPlan& c, float ms) {
    if (c.nsplit > 1 && !small_m) ms += 3e-3f * kn_plan_split_us.get();   // 3 timed calls
    if (ms < best_ms) { best_ms = ms; best = c; }
    if (g_plan_log) g_plan_log->push_back(std::string(plan_kind_name(c.kind)) + "/split" + std::to_string(c.nsplit) +
                                          " " + std::to_string(ms / 3 * 1000.f) + "us");
  };
  if (cold) {
    // every candidate's three cold calls are enqueued with their own event pairs and the host waits
    // ONCE per shape (a wait per call cost ~0.2 s of a transfer-learning epoch's first steps)
    std::vector<hipEvent_t> ev(6 * cands.size());
    for (auto& e : ev) PCMP_HIP_CHECK(hipEventCreate(&e));
    for (size_t ci = 0; ci < cands.size(); ++ci) {
      run_plan<MODE>(p, cands[ci], out, fopts, st);   // warm (workspace allocation)
      for (int r = 0; r < 3; ++r) {
        PCMP_HIP_CHECK(hipMemsetAsync(flush->data_ptr(), r, flush->numel(), st));
        PCMP_HIP_CHECK(hipEventRecord(ev[6 * ci + 2 * r], st));
        run_plan<MODE>(p, cands[ci], out, fopts, st);
        PCMP_HIP_CHECK(hipEventRecord(ev[6 * ci + 2 * r + 1], st));
      }
    }
    PCMP_HIP_CHECK(hipEventSynchronize(ev.back()));
    for (size_t ci = 0; ci < cands.size(); ++ci) {
      float ms = 0.f;
      for (int r = 0; r < 3; ++r) {
        float one = 0.f;
        PCMP_HIP_CHECK(hipEventElapsedTime(&one, ev[6 * ci + 2 * r], ev[6 * ci + 2 * r + 1]));
        ms += one;
      }
      consider(cands[ci], ms);
    }
    for (auto& e : ev) PCMP_HIP_CHECK(hipEventDestroy(e));
  } else {
    for (const GemmPlan& c : cands) {
      run_plan<MODE>(p, c, out, fopts, st);   // warm (workspace allocation)
      float ms = 0.f;
      PCMP_HIP_CHECK(hipEventRecord(e0, st));
      for (int r = 0; r < 3; ++r) run_plan<MODE>(p, c, out, fopts, st);
      PCMP_HIP_CHECK(hipEventRecord(e1, st));
      PCMP_HIP_CHECK(hipEventSynchronize(e1));
      PCMP_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
      consider(c, ms);
    }
  }
  PCMP_HIP_CHECK(hipEventDestroy(e0));
  PCMP_HIP_CHECK(hipEventDestroy(e1));
  if (force >= 0) return best;
  std::lock_guard<std::mutex> g(mu);
  cache.emplace(key, best);
  return best;
}

}  // namespace pcmp
