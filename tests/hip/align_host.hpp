// The serial reference of the alignment stages (abm_align.hpp), plain C++ with no device constructs: shared by
// tests/hip/pilot_score_check.hip and tests/hip/align_check.hip, and checked on its own against alignments written out
// by hand (tests/hip/align_host_main.cpp, built with the host compiler under ASan and UBSan).
//   host_align    the row loop of AbismalAlign::align (src/AbismalAlign.hpp:320-386) and get_traceback /
//                 build_cigar_len_and_pos (:166-193, :388-440): scores 2 / -3 / -4, cells clamped at 0, arrows with left
//                 before above before the diagonal, the first maximum in row-major order.  wrap: every candidate score is
//                 narrowed to int16_t before it competes (score_t, :35, :239-262).  keep: the table, each column's best
//                 value and its first row, and the tie counts come back as well.
//   host_publish  where a CIGAR goes (CigarSink, include/abismal_amd.h: slots of `stride` ops, longer ones whole in the
//                 arena, "what fitted" in the slot when the arena ran out)
//   host_choose   align_se_candidates (src/abismal.cpp:1435-1497)
#pragma once
#include "../../abismal_amd/csrc/abm_lds_layout.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#if defined(__HIP__)
#define AH_HD __host__ __device__
#else
#define AH_HD
#endif

namespace align_host {
using abm::u8;
using abm::u32;
using abm::u64;
using abm::i16;

constexpr u32 kHostFlagRC = 0x10, kHostFlagAmbig = 0x100, kHostFlagARich = 0x1000;

static unsigned long long rng_state = 88172645463325252ull;
static inline unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return static_cast<unsigned>(rng_state >> 16); }
static inline int rnd_in(int lo, int hi) { return lo + static_cast<int>(rnd() % static_cast<unsigned>(hi - lo + 1)); }

static std::vector<unsigned char> G;  // genome nibbles
static inline int host_band(int d, int md) { const int v = 2 * std::min(d, md) + 1; return v < 0 ? 61 : std::min(61, v); }
static inline u32 host_enc_of(u32 flags) {  // src/abismal.cpp:1463-1464
  const u32 rc = (flags & kHostFlagRC) ? 1u : 0u, ar = (flags & kHostFlagARich) ? 1u : 0u;
  return rc * 2u + (rc ^ ar);
}

struct Aligned {
  int score; std::vector<u32> cigar; u32 pos; u32 alen; int ins, del;
  // what the device's stages report on the way
  int br, bc;                  // the first maximum's row and column
  int clip_head, clip_tail;
  u32 n_body;                  // ops without the clips
  int end_row;                 // the row the walk ended in
  // keep:
  std::vector<u8> T;           // (L + bw) x bw: arrow (0 M, 1 I, 2 D, 3 none) | 4 if the cell's score is > 0; 3 outside the read
  std::vector<int> colbest, colrow;  // per column: best value, its first row (0, 0: none above 0)
  int left_ties, above_ties, three_ties, max_cells;  // cells where left tied with above or the diagonal (left won) / above tied with the diagonal / all three tied / cells that hold the maximum
};
// the reference's banded local alignment of read q[0, L) at position pos with band bw: scores 2 / -3 / -4, the first
// maximum in row-major order, arrows with left before above before the diagonal
static inline Aligned host_align(const unsigned char *q, int L, u32 pos, int bw, bool trace, bool wrap = false, bool keep = false) {
  const int rows = L + bw;
  const u32 t_beg = pos - static_cast<u32>((bw - 1) / 2);
  std::vector<int> C(static_cast<size_t>(rows) * bw, 0);
  std::vector<unsigned char> T(static_cast<size_t>(rows) * bw, 3);
  auto narrow = [wrap](int v) { return wrap ? static_cast<int>(static_cast<i16>(v)) : v; };
  int best = 0, br = 0, bc = 0, left_ties = 0, above_ties = 0, three_ties = 0, max_cells = 0;
  std::vector<int> colbest(keep ? bw : 0, 0), colrow(keep ? bw : 0, 0);
  for (int i = 1; i < rows; ++i)
    for (int j = 0; j < bw; ++j) {
      const int r = i + j - bw;
      if (r < 0 || r >= L) continue;
      const bool match = (q[r] & G[t_beg + i - 1]) != 0;
      const int sdiag = narrow(C[static_cast<size_t>(i - 1) * bw + j] + (match ? 2 : -3));
      int c = std::max(sdiag, 0), arrow = c == sdiag ? 0 : 3;
      bool two = false;
      if (j < bw - 1 && r < L - 1) {
        const int up = narrow(C[static_cast<size_t>(i - 1) * bw + j + 1] - 4);
        c = std::max(c, up);
        if (c == up) { two = arrow == 0 && up == sdiag; above_ties += two; arrow = 2; }
      }
      if (j > 0) {
        const int left = narrow(C[static_cast<size_t>(i) * bw + j - 1] - 4);
        const int before = c;
        c = std::max(c, left);
        if (c == left) { left_ties += arrow != 3 && left == before; three_ties += two && left == before; arrow = 1; }
      }
      C[static_cast<size_t>(i) * bw + j] = c;
      T[static_cast<size_t>(i) * bw + j] = static_cast<unsigned char>(arrow | (c > 0 ? 4 : 0));
      if (c > best) { best = c; br = i; bc = j; max_cells = 1; }
      else if (c == best) ++max_cells;
      if (keep && c > colbest[j]) { colbest[j] = c; colrow[j] = i; }
    }
  Aligned a{best, {}, pos, static_cast<u32>(L), 0, 0, br, bc, 0, 0, 0, 0, {}, {}, {}, left_ties, above_ties, three_ties, best > 0 ? max_cells : 0};
  if (keep) { a.T = T; a.colbest = colbest; a.colrow = colrow; }
  if (!trace || best == 0) { a.cigar.push_back(static_cast<u32>(L) << 4); return a; }
  int r = br, c = bc;
  const int clip_tail = (L + bw - 1) - (r + c);
  std::vector<u32> ops;
  auto emit = [&](u32 run, int op) {
    ops.push_back((run << 4) | static_cast<u32>(op));
    if (op == 1) a.ins = static_cast<short>(a.ins + static_cast<unsigned char>(run));
    if (op == 2) a.del = static_cast<short>(a.del + static_cast<unsigned char>(run));
  };
  auto step = [&](int ar) { if (ar != 1) --r; if (ar == 1) --c; if (ar == 2) ++c; };
  int op = T[static_cast<size_t>(r) * bw + c] & 3;
  step(op);
  u32 run = 1;
  for (;;) {
    const int cell = T[static_cast<size_t>(r) * bw + c];
    if (!(cell & 4)) break;
    const int ar = cell & 3;
    step(ar);
    if (ar != op) { emit(run, op); run = 0; }
    ++run;
    op = ar;
  }
  emit(run, op);
  const int clip_head = (r + c) - (bw - 1);
  if (clip_head > 0) a.cigar.push_back((static_cast<u32>(clip_head) << 4) | 4u);
  a.cigar.insert(a.cigar.end(), ops.rbegin(), ops.rend());
  if (clip_tail > 0) a.cigar.push_back((static_cast<u32>(clip_tail) << 4) | 4u);
  a.alen = static_cast<u32>(L - clip_tail - clip_head);
  a.pos = pos - static_cast<u32>((bw - 1) / 2) + static_cast<u32>(r);
  a.clip_head = clip_head; a.clip_tail = clip_tail; a.n_body = static_cast<u32>(ops.size()); a.end_row = r;
  return a;
}
AH_HD static inline int host_nm(int scr, u32 len, int ins, int del) {  // simple_aln::edit_distance, src/AbismalAlign.hpp:73-89
  if (scr == 0) return static_cast<short>(len);
  const int A = static_cast<short>(scr + 4 * (ins + del));
  const u32 num = 2u * (len - static_cast<u32>(ins)) - static_cast<u32>(A);
  return static_cast<short>(static_cast<short>(num / 5u) + ins + del);
}
AH_HD static inline bool host_long_enough(u32 alen, u32 readlen, u32 min_len) {  // valid_len, src/abismal.cpp:307-314
  const double min_frac = 1.0 - 0.4;
  const u32 need = static_cast<u32>(min_frac * readlen);
  return alen >= (min_len > need ? min_len : need);
}

// ---- where a CIGAR goes ---------------------------------------------------------------------------------------------
// A read's slot has `stride` words.  A CIGAR of at most `stride` ops lies in it.  A longer one lies whole in the arena,
// from the index that the slot's first word then holds: the arena hands out its words by a counter that every such CIGAR
// moves on by its op count, whether it then fits below arena_cap or not.  Without an arena, without room in it, or when
// the walk could not keep all its ops (more than ctmp_cap, of which the ones nearest the read's end stay), the launch is
// flagged and the slot holds what fits of what there is: the head clip, the kept ops in order, the tail clip -- from the
// front, `stride` words at most.  The op count reported is always the whole CIGAR's.  fin, where asked for, repeats the
// first kSeCap words of what was written.  Words not named here are not written.
struct HostSink { u32 stride, ctmp_cap; bool has_arena; u32 arena_cap, arena_count; bool want_fin; };
struct Published {
  u32 n_ops; bool overflow;
  std::vector<u32> slot;                 // [stride], kUnwritten where nothing is written
  bool in_arena; u32 arena_at;           // the whole CIGAR at arena[arena_at ..)
  u32 arena_count;                       // the counter afterwards
  std::vector<u32> fin;                  // the words fin gets (at most kSeCap)
};
constexpr u32 kUnwritten = 0xDEADBEEFu;
static inline Published host_publish(const Aligned &a, const HostSink &s) {
  Published p{static_cast<u32>(a.cigar.size()), false, std::vector<u32>(s.stride, kUnwritten), false, 0, s.arena_count, {}};
  std::vector<u32> written = a.cigar;
  if (p.n_ops <= s.stride) std::copy(a.cigar.begin(), a.cigar.end(), p.slot.begin());
  else {
    const bool kept_all = a.n_body <= s.ctmp_cap;
    if (s.has_arena && kept_all) {
      p.arena_at = s.arena_count;
      p.arena_count = s.arena_count + p.n_ops;
      p.in_arena = p.arena_at <= s.arena_cap && p.n_ops <= s.arena_cap - p.arena_at;
    }
    if (p.in_arena) p.slot[0] = p.arena_at;
    else {
      p.overflow = true;
      written.clear();
      if (a.clip_head > 0) written.push_back(a.cigar.front());
      const size_t body0 = a.clip_head > 0 ? 1 : 0, kept = std::min<size_t>(a.n_body, s.ctmp_cap);
      for (size_t k = a.n_body - kept; k < a.n_body; ++k) written.push_back(a.cigar[body0 + k]);
      if (a.clip_tail > 0) written.push_back(a.cigar.back());
      if (written.size() > s.stride) written.resize(s.stride);
      std::copy(written.begin(), written.end(), p.slot.begin());
    }
  }
  if (s.want_fin) p.fin.assign(written.begin(), written.begin() + std::min<size_t>(written.size(), abm::kSeCap));
  return p;
}

// ---- the choice of a single-end read's hit -----------------------------------------------------------------------------
struct HostJob { u32 pos, flags; int d; };
struct Expect {
  u32 pos, flags; int diffs; std::vector<u32> cigar;
  bool traced;          // a CIGAR was written (its hit may still have failed the length or NM test: pos 0 then)
  u32 n_aln, n_single;
};
// q[e]: the read in encoding e (host_enc_of); exact: the set's exact match (pos 0: none)
static inline Expect host_choose_jobs(const unsigned char *const q[4], int L, std::vector<HostJob> jobs, double frac, u32 min_len, bool wrap,
                                      const HostJob &exact) {
  const int md = static_cast<short>(frac * L), invalid_at = static_cast<short>(0.4 * L), perfect = static_cast<short>(2 * L);
  if (exact.pos != 0) return Expect{exact.pos, exact.flags, exact.d, {static_cast<u32>(L) << 4}, true, 0, 0};
  std::sort(jobs.begin(), jobs.end(), [](const HostJob &a, const HostJob &b) { return a.pos != b.pos ? a.pos < b.pos : a.flags < b.flags; });
  jobs.erase(std::unique(jobs.begin(), jobs.end(), [](const HostJob &a, const HostJob &b) { return a.pos == b.pos && a.flags == b.flags; }), jobs.end());
  int top = 0, b_d = 0;
  u32 top_pos = 0, b_pos = 0, b_flags = 0, n_aln = 0, n_jobs = 0;
  for (const auto &j : jobs) {
    if (j.pos == 0 || j.d >= invalid_at) continue;
    ++n_jobs;
    const int sc = host_align(q[host_enc_of(j.flags)], L, j.pos, host_band(j.d, md), false, wrap).score;
    ++n_aln;
    if (sc > top) { top = sc; top_pos = b_pos = j.pos; b_d = j.d; b_flags = j.flags; }
    else if (sc == top) {
      const u32 gap = j.pos > top_pos ? j.pos - top_pos : top_pos - j.pos;
      if (sc == perfect ? j.pos != top_pos : gap > 3u) b_flags |= kHostFlagAmbig;
    }
  }
  Expect e{0, b_flags, 0x7fff, {}, false, n_aln, n_jobs == 1 ? 1u : 0u};
  if (n_jobs == 1 && b_pos == 0) e.flags = kHostFlagAmbig;  // (a zero score ties with "nothing yet" at position 0)
  if (b_pos == 0) return e;
  const Aligned a = host_align(q[host_enc_of(b_flags)], L, b_pos, host_band(b_d, md), true, wrap);
  const int nm = host_nm(top, a.alen, a.ins, a.del);
  e.cigar = a.cigar;
  e.traced = true;
  if (host_long_enough(a.alen, static_cast<u32>(L), min_len) && nm <= md) { e.diffs = nm; e.pos = a.pos; }
  return e;
}
// a set of (position, d) on the read's first encoding, flags 0
static inline Expect host_choose(const unsigned char *q, int L, const std::vector<std::pair<u32, int>> &jobs, double frac) {
  std::vector<HostJob> js;
  for (const auto &j : jobs) js.push_back({j.first, 0u, j.second});
  const unsigned char *const qs[4] = {q, q, q, q};
  return host_choose_jobs(qs, L, js, frac, 32, false, HostJob{0, 0, 0});
}

// plants a copy of the read at pos: `subs` substitutions, and from read index `gap_at` on (if > 0) the copy lacks
// (gap < 0) or has in addition (gap > 0) |gap| bases, so that only a gapped alignment follows the read to its end
static inline void plant(const unsigned char *q, int L, u32 pos, int subs, int gap_at, int gap, const std::vector<int> *sub_at = nullptr) {
  std::vector<unsigned char> copy(q, q + L);
  for (int k = 0; k < subs; ++k) {
    const int at = sub_at ? (*sub_at)[k] : rnd_in(0, L - 1);
    copy[at] = static_cast<unsigned char>(1u << ((__builtin_ctz(copy[at]) + 1 + (sub_at ? 0 : static_cast<int>(rnd() % 3))) & 3));
  }
  if (gap_at > 0 && gap < 0) copy.erase(copy.begin() + gap_at, copy.begin() + gap_at - gap);
  if (gap_at > 0 && gap > 0) for (int k = 0; k < gap; ++k) copy.insert(copy.begin() + gap_at, static_cast<unsigned char>(1u << (rnd() & 3)));
  for (size_t k = 0; k < copy.size(); ++k) G[pos + k] = copy[k];
}
static inline int hamming(const unsigned char *q, int L, u32 pos) {
  int d = 0;
  for (int k = 0; k < L; ++k) d += (q[k] & G[pos + k]) == 0;
  return d;
}

}  // namespace align_host
