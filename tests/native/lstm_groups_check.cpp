// Host check of csrc/lstm_groups.h: the launch plan and the per-group views of the persistent
// BiLSTM recurrences, over every B in 1..300, H in {32, 64, 192, 256, 512}, CU counts 256, 64 and 1
// and the lstm_groups values 0, 1, 2 and 1000.  Compiled by tests/test_lstm_groups_cpu.py with
// -fsanitize=undefined; exits non-zero at the first violated property.
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
