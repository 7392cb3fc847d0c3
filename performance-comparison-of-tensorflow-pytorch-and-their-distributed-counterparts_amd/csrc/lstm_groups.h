// Group arithmetic and LDS layouts of the persistent BiLSTM recurrences (csrc/rnn.hip).
//
// A *group* is one chunk of kGroupRows = 32 sequences: an independent recurrence that 2 * (H / 16)
// workgroups (one per direction and 16 hidden units) run to the end.  A launch carries several groups
// side by side: workgroups [g * wgs, (g + 1) * wgs) of the grid form the launch's g-th group.  Groups
// never talk to each other; each has its own rows of the batch tensors, its own slice of the
// exchange buffers and its own pair of arrival counters.
//
// The dynamic LDS of each kernel is described once, by a constexpr function of H that gives the byte
// offset of every region and the total: the kernel takes its pointers from it, the host the launch's
// LDS size and the admission test (lds_fits), so the two cannot drift apart.  (One pointer is not
// taken from here: sGx of lstm_fwd_persistent2, which that kernel reaches by typed steps over the two
// regions in front of it; rnn.hip says why.  Whoever moves a region of Fwd2Lds moves that line too.)
//
// Everything here is plain integer arithmetic with no HIP or torch dependency, shared by the kernels
// (per-group view, LDS pointers), the host launcher (launch plan, allocation sizes, LDS sizes, kernel
// admission) and a host test program (tests/native/lstm_groups_check.cpp).
#pragma once

#if defined(__HIPCC__)
#define LSTMG_HD __host__ __device__
#else
#define LSTMG_HD
#endif

namespace pcmp {
namespace lstmg {

constexpr int kGroupRows = 32;    // LB of rnn.hip: sequences of one group
constexpr int kUnits = 16;        // LJ of rnn.hip: hidden units per workgroup
constexpr int kRoleThreads = 256; // LC of rnn.hip: compute threads of a role-split workgroup (as many IO threads)
constexpr int kSyncWords = 4;     // sync words of group 0: counters [0], [1], error [2], spare [3]
constexpr int kErrWord = 2;       // the error word of the whole call (a bounded spin ran out)
constexpr int kProfWords = 16;    // knob lstm_prof: phase clocks behind the first four words

LSTMG_HD constexpr int n_groups(int B) { return (B + kGroupRows - 1) / kGroupRows; }
LSTMG_HD constexpr int wgs_per_group(int H) { return 2 * (H / kUnits); }

// ---------------------------------------------------------------------------- launch plan (host)
// A launch must be co-resident by its size alone: at most one workgroup per CU (the 512-thread
// kernels' occupancy; assumed at small H too, where LDS would admit more).  A device with fewer CUs
// than one group has workgroups still takes one group per launch, like the single-group kernels did.
LSTMG_HD constexpr int max_groups(int H, int cus) {
  const int w = wgs_per_group(H);
  const int g = w > 0 ? cus / w : 1;
  return g < 1 ? 1 : g;
}
// The automatic group count.  Residency admits max_groups, but the exchange traffic of the groups
// shares the fabric: on MI355X at H = 256 the forward step takes 3.3 / 4.5 / 6.9 / 11.5 / 17.6 us
// with 1 / 2 / 4 / 6 / 8 groups in the launch (docs/PERF_NOTES.md "BiLSTM batches above 32"), so two
// launches of 4 groups beat one of 8 (the backward is even); at H = 512 two launches of 2 groups beat
// one of 4.  The automatic launch therefore fills half the CUs: 4 groups at H = 256, 2 at H = 512.
// At H <= 64 a workgroup's exchange tile is 4 KB or less and the whole device is the fastest (32
// groups at H = 64: 8.5 us per step against 2 x 6.3 us for two launches of 16), so there it is max_groups.
constexpr int kAutoFullH = 64;
LSTMG_HD constexpr int auto_groups(int H, int cus) {
  if (H <= kAutoFullH) return max_groups(H, cus);
  const int w = wgs_per_group(H);
  const int g = w > 0 ? (cus / 2) / w : 1;
  return g < 1 ? 1 : g;
}
// groups of a full launch: knob lstm_groups = 0 -> auto_groups, n > 0 -> min(n, max_groups)
LSTMG_HD constexpr int groups_per_launch(int H, int cus, int knob) {
  const int gm = max_groups(H, cus);
  return knob > 0 ? (knob < gm ? knob : gm) : auto_groups(H, cus);
}
LSTMG_HD constexpr int n_launches(int B, int H, int cus, int knob) {
  const int g = groups_per_launch(H, cus, knob);
  return (n_groups(B) + g - 1) / g;
}
// first group and group count of launch l (0 <= l < n_launches)
LSTMG_HD constexpr int launch_first(int H, int cus, int knob, int l) { return l * groups_per_launch(H, cus, knob); }
LSTMG_HD constexpr int launch_groups(int B, int H, int cus, int knob, int l) {
  const int g = groups_per_launch(H, cus, knob), left = n_groups(B) - l * g;
  return left < g ? left : g;
}
// exchange-buffer slices to allocate: the group count of the largest (the first) launch
LSTMG_HD constexpr int exchange_slots(int B, int H, int cus, int knob) {
  const int g = groups_per_launch(H, cus, knob), n = n_groups(B);
  return n < g ? n : g;
}

// ---------------------------------------------------------------------------- per-group view
// rows [row0, row0 + local_B) of the batch tensors belong to group grp (0 <= grp < n_groups(B))
LSTMG_HD constexpr long long row0(int grp) { return (long long)grp * kGroupRows; }
LSTMG_HD constexpr int local_B(int B, int grp) {
  const int left = B - grp * kGroupRows;
  return left < kGroupRows ? left : kGroupRows;
}
// elements of one group's slice of each exchange buffer; slot s of a launch starts at s * elems
LSTMG_HD constexpr long long hbuf_elems(int H) { return 2LL * 2 * kGroupRows * H; }           // bf16 [2][2][LB][H]
LSTMG_HD constexpr long long dgbuf_elems(int H) { return 2LL * 2 * kGroupRows * 4 * H; }      // bf16 [2][2][LB][4H]
LSTMG_HD constexpr long long pbuf_elems(int H) { return 2LL * 2 * (H / kUnits) * H * kGroupRows; }   // f32 [2][2][nub][H][LB]
// bytes of the largest group's slice of the fp32 gates tensor (the largest tensor of a group): the
// 32-bit byte offsets of the role-split kernels' buffer resources are per group
LSTMG_HD constexpr long long group_gates_bytes(int B, int S, int H) {
  return (long long)local_B(B, 0) * S * 2 * 4 * H * 4;
}

// Sync words of one call: group 0 keeps words 0, 1 (its two arrival counters), 2 (the error word of
// the whole call) and 3; with lstm_prof the phase clocks of group 0 follow; the counter pairs of
// groups 1, 2, ... are appended behind.  Counters are per group of the BATCH, not of the launch: a
// later launch of the same call finds its counters still zero.
LSTMG_HD constexpr int counter_base(bool prof) { return kSyncWords + (prof ? kProfWords : 0); }
LSTMG_HD constexpr int counter_word(int grp, bool prof) { return grp == 0 ? 0 : counter_base(prof) + 2 * (grp - 1); }
LSTMG_HD constexpr int sync_words(int B, bool prof) { return counter_base(prof) + 2 * (n_groups(B) - 1); }

// ---------------------------------------------------------------------------- LDS layouts
// Byte offsets of the regions of each kernel's dynamic LDS, in their order, and the total; the fields
// carry the kernels' names for the regions.  Every region but the flags (sV) is read or written as
// 16-byte vectors and starts on a 16-byte boundary (H is a multiple of 32).  Next to each role-split
// layout stands the admission predicate of its kernel: what it asks of a call beyond the shape check
// of every LSTM call; a call it refuses runs the round-1 kernel.
constexpr int kLdsBudget = 160 * 1024;                 // LDS bytes one workgroup may ask for
LSTMG_HD constexpr bool lds_fits(int total) { return total <= kLdsBudget; }
constexpr int kWBytes = 4 * kUnits * 2;                // a workgroup's W_hh slice, bf16, per hidden unit of H
constexpr int kTileF32 = kGroupRows * kUnits * 4;      // f32 [kGroupRows][kUnits]: one value per (b, unit) pair
constexpr int kTileBf16 = kGroupRows * kUnits * 2;     // bf16 [kGroupRows][kUnits]
constexpr int kFlagBytes = (2 * kGroupRows + 1) * 4;   // int [2][kGroupRows] token-valid flags, [2 * kGroupRows] abort

// the IO waves' buffer resources take 32-bit byte offsets inside one group's slice
LSTMG_HD constexpr bool offsets_fit_32(int B, int S, int H) { return group_gates_bytes(B, S, H) < (1ll << 31); }
// an exchange tile bf16 [kGroupRows][cols] is gathered in whole passes of the compute threads, 16 B each
LSTMG_HD constexpr bool whole_gather_passes(int cols) { return (kGroupRows * cols / 8) % kRoleThreads == 0; }

// lstm_fwd_persistent (round 1)
struct Fwd1Lds { int sW, sH, sG, sHo, total; };
LSTMG_HD constexpr Fwd1Lds fwd1_lds(int H) {
  Fwd1Lds l{};
  l.sW = 0;                               // bf16 [4 * kUnits][H]  W_hh rows (row = gate * kUnits + jj)
  l.sH = l.sW + kWBytes * H;              // bf16 [kGroupRows][H]  h_{t-1}
  l.sG = l.sH + kGroupRows * H * 2;       // f32 [kGroupRows][4 * kUnits]  recurrent pre-activations
  l.sHo = l.sG + 4 * kTileF32;            // bf16 [kGroupRows][kUnits]  this workgroup's h_t slice
  l.total = l.sHo + kTileBf16;
  return l;
}

// lstm_bwd_persistent (round 1).  It keeps the whole direction's dgates tile: the one layout that
// outgrows the budget (H <= 384 fits).
struct Bwd1Lds { int sWt, sD, sR, sDo, total; };
LSTMG_HD constexpr Bwd1Lds bwd1_lds(int H) {
  Bwd1Lds l{};
  l.sWt = 0;                              // bf16 [kUnits][4H]  W_hh columns (row jj holds W_hh[:, j0 + jj])
  l.sD = l.sWt + kWBytes * H;             // bf16 [kGroupRows][4H]  dgates_t of the direction
  l.sR = l.sD + kGroupRows * 4 * H * 2;   // f32 [kGroupRows][kUnits]  dh_rec
  l.sDo = l.sR + kTileF32;                // bf16 [kGroupRows][4][kUnits]  this workgroup's dgates_t slice
  l.total = l.sDo + 4 * kTileBf16;
  return l;
}

// lstm_fwd_persistent2 (role-split)
struct Fwd2Lds { int sW, sH, sG, sGx, sA, sC, sHo, sV, total; };
LSTMG_HD constexpr Fwd2Lds fwd2_lds(int H) {
  Fwd2Lds l{};
  l.sW = 0;                               // bf16 [4 * kUnits][H]  W_hh rows (swizzled)
  l.sH = l.sW + kWBytes * H;              // bf16 [kGroupRows][H]  h_{t-1} (swizzled)
  l.sG = l.sH + kGroupRows * H * 2;       // f32 [kGroupRows][4 * kUnits]  recurrent pre-activations
  l.sGx = l.sG + 4 * kTileF32;            // f32 [2][kGroupRows][4 * kUnits]  input projections (ping-pong)
  l.sA = l.sGx + 2 * 4 * kTileF32;        // f32 [kGroupRows][4 * kUnits]  activations i,f,g,o (staging)
  l.sC = l.sA + 4 * kTileF32;             // f32 [kGroupRows][kUnits]  c_t (staging)
  l.sHo = l.sC + kTileF32;                // bf16 [kGroupRows][kUnits]  h_t (exchange + output)
  l.sV = l.sHo + kTileBf16;               // the flags
  l.total = l.sV + kFlagBytes;
  return l;
}
LSTMG_HD constexpr bool fwd2_admits(int B, int S, int H) {
  return lds_fits(fwd2_lds(H).total) && whole_gather_passes(H) && offsets_fit_32(B, S, H);
}

// lstm_bwd_persistent2 and lstm_bwd_persistent3 (role-split).  The W_hh slice is columns j0.. of all
// 4H rows in the one and the workgroup's 4 * kUnits rows, j-major, in the other: the same bytes.
struct Bwd2Lds { int sW, sR, sDo, sF, sV, total; };
LSTMG_HD constexpr Bwd2Lds bwd2_lds(int H) {
  Bwd2Lds l{};
  l.sW = 0;                               // bf16 [kUnits][4H] or [H][4 * kUnits]  W_hh slice (swizzled)
  l.sR = l.sW + kWBytes * H;              // f32 [kGroupRows][kUnits]  dh_rec
  l.sDo = l.sR + kTileF32;                // bf16 [kGroupRows][4][kUnits]  this slice's dgates_t
  l.sF = l.sDo + 4 * kTileBf16;           // f32 [2][7][kGroupRows][kUnits]  per-step inputs (ping-pong)
  l.sV = l.sF + 2 * 7 * kTileF32;         // the flags
  l.total = l.sV + kFlagBytes;
  return l;
}
LSTMG_HD constexpr bool bwd2_admits(int B, int S, int H) {   // the tile exchange: bf16 [kGroupRows][4H]
  return lds_fits(bwd2_lds(H).total) && whole_gather_passes(4 * H) && offsets_fit_32(B, S, H);
}
LSTMG_HD constexpr bool bwd3_admits(int B, int S, int H) {   // the partial exchange gathers 4-B words: any H
  return lds_fits(bwd2_lds(H).total) && offsets_fit_32(B, S, H);
}

}  // namespace lstmg
}  // namespace pcmp
