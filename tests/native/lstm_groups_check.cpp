// Host check of csrc/lstm_groups.h: the launch plan and the per-group views of the persistent
// BiLSTM recurrences, over every B in 1..300, H in {32, 64, 192, 256, 512}, CU counts 256, 64 and 1
// and the lstm_groups values 0, 1, 2 and 1000; the kernels' LDS layouts and admission tests over
// every H in 32, 64, ..., 512.  Compiled by tests/test_lstm_groups_cpu.py with -fsanitize=undefined;
// exits non-zero at the first violated property.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lstm_groups.h"

namespace g = pcmp::lstmg;

#define CHECK(cond)                                                                                        \
  do {                                                                                                     \
    if (!(cond)) {                                                                                         \
      std::printf("lstm_groups_check: %s failed at B=%d H=%d cus=%d knob=%d (line %d)\n", #cond, B, H, cus, \
                  knob, __LINE__);                                                                         \
      std::exit(1);                                                                                        \
    }                                                                                                      \
  } while (0)

int main() {
  const int Hs[] = {32, 64, 192, 256, 512}, CUs[] = {256, 64, 1}, knobs[] = {0, 1, 2, 1000};
  long checked = 0;
  for (int H : Hs)
    for (int cus : CUs)
      for (int knob : knobs)
        for (int B = 1; B <= 300; ++B) {
          const int ng = g::n_groups(B), wgs = g::wgs_per_group(H);
          CHECK(ng == (B + 31) / 32 && wgs == 2 * (H / 16));
          // ---- plan: entries in [1, max(1, G_max)], sum = ceil(B / 32), consecutive group ranges
          const int gmax = cus / wgs, cap = gmax > 1 ? gmax : 1;
          CHECK(g::max_groups(H, cus) == cap);
          const int G = g::groups_per_launch(H, cus, knob);
          const int half = (cus / 2) / wgs;                      // automatic: half the CUs, all of them at H <= 64
          const int autog = H <= 64 ? cap : (half > 1 ? half : 1);
          CHECK(g::auto_groups(H, cus) == autog && autog <= cap);
          CHECK(G == (knob > 0 ? (knob < cap ? knob : cap) : autog));
          const int nl = g::n_launches(B, H, cus, knob);
          CHECK(nl >= 1);
          int sum = 0, largest = 0;
          for (int l = 0; l < nl; ++l) {
            const int n = g::launch_groups(B, H, cus, knob, l);
            CHECK(n >= 1 && n <= cap && n <= G);
            CHECK(g::launch_first(H, cus, knob, l) == sum);      // launches tile the groups in order
            CHECK(gmax < 1 || n * wgs <= cus);                     // one workgroup per CU
            if (knob == 1) CHECK(n == 1);
            if (l + 1 < nl) CHECK(n == G);                         // only the last launch is partial
            sum += n;
            largest = n > largest ? n : largest;
          }
          CHECK(sum == ng);
          const int slots = g::exchange_slots(B, H, cus, knob);
          CHECK(slots == largest);
          // ---- views: rows tile [0, B); local B in 1..32
          long long next = 0;
          for (int grp = 0; grp < ng; ++grp) {
            const long long r0 = g::row0(grp);
            const int lb = g::local_B(B, grp);
            CHECK(r0 == next && lb >= 1 && lb <= 32 && r0 + lb <= B);
            next = r0 + lb;
          }
          CHECK(next == B);
          CHECK(g::group_gates_bytes(B, 7, H) == (long long)(B < 32 ? B : 32) * 7 * 2 * 4 * H * 4);
          // ---- exchange slots of a launch: slot s covers [s * elems, (s + 1) * elems) of the
          //      allocation of `slots` slices: disjoint by construction, the last one inside
          const long long he = g::hbuf_elems(H), de = g::dgbuf_elems(H), pe = g::pbuf_elems(H);
          CHECK(he == 4LL * 32 * H && de == 4LL * 32 * 4 * H && pe == 4LL * (H / 16) * H * 32);
          for (int l = 0; l < nl; ++l)
            for (int s = 0; s < g::launch_groups(B, H, cus, knob, l); ++s) {
              CHECK(s >= 0 && (s + 1) * he <= slots * he && (s + 1) * de <= slots * de && (s + 1) * pe <= slots * pe);
              CHECK(g::launch_first(H, cus, knob, l) + s < ng);
            }
          // ---- counters: a pair of words per group, disjoint from each other, from the error word
          //      (2), the spare word (3) and the profile words, and inside the sync allocation
          for (int prof = 0; prof < 2; ++prof) {
            const int words = g::sync_words(B, prof != 0);
            CHECK(words == 4 + 16 * prof + 2 * (ng - 1));
            std::vector<int> used(words, 0);
            used[2] = used[3] = 1;
            for (int w = 4; w < 4 + 16 * prof; ++w) used[w] = 1;
            for (int grp = 0; grp < ng; ++grp) {
              const int c = g::counter_word(grp, prof != 0);
              CHECK(c >= 0 && c + 1 < words);
              CHECK(grp != 0 || c == 0);
              CHECK(!used[c] && !used[c + 1]);
              used[c] = used[c + 1] = 1;
            }
            for (int w = 0; w < words; ++w) CHECK(used[w]);      // no word left over
          }
          ++checked;
        }
  // ---- LDS layouts, every H the kernels take.  Totals against the sums the launcher used to write out
  //      by hand (LJ = 16 units, LB = 32 rows); regions in the kernels' order, none empty (so none
  //      overlaps the next), each 16-byte aligned (the flags, 4-byte words, come last); the budget
  //      admits every H but the round-1 backward's above 384.
  for (int H = 32; H <= 512; H += 32) {
    const int B = 32, cus = 0, knob = 0, LJ = 16, LB = 32;
    const g::Fwd1Lds f1 = g::fwd1_lds(H);
    const g::Bwd1Lds b1 = g::bwd1_lds(H);
    const g::Fwd2Lds f2 = g::fwd2_lds(H);
    const g::Bwd2Lds b2 = g::bwd2_lds(H);
    CHECK(f1.total == 4 * LJ * H * 2 + LB * H * 2 + LB * 4 * LJ * 4 + LB * LJ * 2);
    CHECK(b1.total == LJ * 4 * H * 2 + LB * 4 * H * 2 + LB * LJ * 4 + LB * 4 * LJ * 2);
    CHECK(f2.total == 4 * LJ * H * 2 + LB * H * 2 + 4 * LB * 4 * LJ * 4 + LB * LJ * 4 + LB * LJ * 2 + (2 * LB + 1) * 4);
    CHECK(b2.total == LJ * 4 * H * 2 + LB * LJ * 4 + LB * 4 * LJ * 2 + 2 * 7 * LB * LJ * 4 + (2 * LB + 1) * 4);
    const std::vector<std::vector<int>> layouts = {
        {f1.sW, f1.sH, f1.sG, f1.sHo, f1.total},
        {b1.sWt, b1.sD, b1.sR, b1.sDo, b1.total},
        {f2.sW, f2.sH, f2.sG, f2.sGx, f2.sA, f2.sC, f2.sHo, f2.sV, f2.total},
        {b2.sW, b2.sR, b2.sDo, b2.sF, b2.sV, b2.total}};
    for (const auto& l : layouts) {
      CHECK(l[0] == 0);
      for (size_t i = 0; i + 1 < l.size(); ++i) CHECK(l[i] < l[i + 1] && l[i] % 16 == 0);
    }
    // the sizes of the regions the kernels index by shape
    CHECK(f1.sH - f1.sW == 4 * LJ * H * 2 && f1.sG - f1.sH == LB * H * 2 && f1.sHo - f1.sG == LB * 4 * LJ * 4);
    CHECK(b1.sD - b1.sWt == LJ * 4 * H * 2 && b1.sR - b1.sD == LB * 4 * H * 2 && b1.sDo - b1.sR == LB * LJ * 4);
    CHECK(f2.sH - f2.sW == 4 * LJ * H * 2 && f2.sG - f2.sH == LB * H * 2 && f2.sGx - f2.sG == LB * 4 * LJ * 4 &&
          f2.sA - f2.sGx == 2 * LB * 4 * LJ * 4 && f2.sC - f2.sA == LB * 4 * LJ * 4 && f2.sHo - f2.sC == LB * LJ * 4 &&
          f2.sV - f2.sHo == LB * LJ * 2);
    CHECK(b2.sR - b2.sW == LJ * 4 * H * 2 && b2.sDo - b2.sR == LB * LJ * 4 && b2.sF - b2.sDo == LB * 4 * LJ * 2 &&
          b2.sV - b2.sF == 2 * 7 * LB * LJ * 4);
    CHECK(g::kLdsBudget == 160 * 1024);
    CHECK(g::lds_fits(f1.total) && g::lds_fits(f2.total) && g::lds_fits(b2.total));
    CHECK(g::lds_fits(b1.total) == (H <= 384));
    // the role-split kernels' admission: the forward gathers [32][H] in whole 256-thread passes of
    // 16 B (H a multiple of 64), the backwards take every H; all of them want 32-bit offsets
    CHECK(g::fwd2_admits(32, 128, H) == (H % 64 == 0) && g::bwd2_admits(32, 128, H) && g::bwd3_admits(32, 128, H));
    const long long per = 32ll * 2 * 4 * H * 4;                     // gates bytes of 32 rows per step
    const int Sbig = (int)(((1ll << 31) + per - 1) / per);          // the first S at which they reach 2^31
    CHECK(g::group_gates_bytes(32, Sbig, H) >= (1ll << 31) && !g::fwd2_admits(32, Sbig, H) &&
          !g::bwd2_admits(32, Sbig, H) && !g::bwd3_admits(32, Sbig, H));
    CHECK(g::offsets_fit_32(32, Sbig - 1, H) && g::bwd3_admits(32, Sbig - 1, H));
    ++checked;
  }
  static_assert(g::kErrWord == 2 && g::kSyncWords == 4 && g::kRoleThreads == 256, "sync words, role threads");
  // the plans the documentation quotes for a 256-CU device
  {
    const int B = 257, H = 256, cus = 256, knob = 1000;   // the residency limit: 8 groups
    CHECK(g::max_groups(H, cus) == 8 && g::max_groups(64, cus) == 32);
    CHECK(g::n_launches(B, H, cus, knob) == 2 && g::launch_groups(B, H, cus, knob, 0) == 8 &&
          g::launch_groups(B, H, cus, knob, 1) == 1);
  }
  {
    const int B = 257, H = 256, cus = 256, knob = 0;      // automatic: 4 groups
    CHECK(g::n_launches(B, H, cus, knob) == 3 && g::launch_groups(B, H, cus, knob, 0) == 4 &&
          g::launch_groups(B, H, cus, knob, 1) == 4 && g::launch_groups(B, H, cus, knob, 2) == 1);
  }
  {
    const int B = 40, H = 512, cus = 256, knob = 0;
    CHECK(g::max_groups(H, cus) == 4 && g::n_launches(B, H, cus, knob) == 1 && g::launch_groups(B, H, cus, knob, 0) == 2);
  }
  {
    const int B = 70, H = 64, cus = 256, knob = 2;
    CHECK(g::max_groups(H, cus) == 32 && g::n_launches(B, H, cus, knob) == 2 && g::launch_groups(B, H, cus, knob, 0) == 2 &&
          g::launch_groups(B, H, cus, knob, 1) == 1);
  }
  std::printf("lstm_groups_check: ok (%ld cases)\n", checked);
  return 0;
}
