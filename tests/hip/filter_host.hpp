// The serial side of tests/hip/filter_check.hip: plain C++, no device, nothing taken from abm_seed.hpp.  Held to cases
// written out by hand in tests/hip/filter_host_main.cpp.
//
// THE DISTANCE.  full_compare (src/abismal.cpp:1105-1122) walks the read's packed words, 16 letters each, the read's
// letters at or past its length L holding 0xF: a word adds 16 - sum over its 16 letters of popcount(read nibble & genome
// nibble) to a running sum.  d is the total over the words, dmax the largest running sum seen on the way (the empty
// prefix, 0, included: a candidate is admitted iff every running sum stays within a cutoff that is never negative).
// serial_distance is that rule letter by letter.
//
// THE PLANE AND RECORD FORMS count the mismatches of the read's L letters alone.  The two coincide on a one-hot genome
// without a blank within the words' reach: a one-hot genome nibble shares at most one bit with any read nibble, so a
// letter below L adds popcount 1 where it matches and 0 where it does not, and a letter at or past L (0xF) always adds
// 1 -- the word's share is the number of the read's own letters in it that do not match, never negative, hence
// d = letter_count and dmax = d.  A blank nibble (0) matches nothing, not even the 0xF padding, and a nibble of two or
// more bits can add 2: there the forms part, and the filter steps redo such candidates on the nibble array.
//
// THE POSITION CACHE of the window steps: 256 slots, direct-mapped by (pos * 2654435761) >> 24 in 32-bit arithmetic,
// 0 = empty.  All lanes of a step look their slots up before any of them writes; the a half writes before the b half.
// Two DIFFERENT positions written to one slot by lanes of the same half leave either of them there: the model keeps
// the set of possible contents and says so (a lookup then has a range of outcomes, hit_lo .. hit_hi; `unsure` counts
// them, and filter_check.hip bounds that count and has cases in which it must be 0).
//
// THE SET is libstdc++'s heap calls in candidate order: contents, cutoff, sure_ambig, the exact hit and `updates` are
// derived here on their own.  `fifo` is not: it counts the updates that meet the condition under which the kernels apply
// a run of ties at a time (a full set whose first, 25th and last elements sit at the cutoff, and a newcomer that ties),
// and that condition is the product's own rule written out again.  Comparing wt.fifo_updates with it shows that the
// kernel counts what it says it counts, not that the rule is the right one; that the shortcut leaves the right set is
// what the comparison of the contents shows.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace filter_host {
using u8 = uint8_t;
using u16 = uint16_t;
using u32 = uint32_t;
using u64 = uint64_t;
using i16 = int16_t;

struct Rng {
  u64 s;
  explicit Rng(u64 seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) { if (!s) s = 1; }
  u32 next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return static_cast<u32>(s >> 20); }
  u32 below(u32 n) { return next() % n; }
};

// ---- letters ---------------------------------------------------------------------------------------------------------
// a read letter's nibble in the T-rich / A-rich alphabet (src/dna_four_bit_bisulfite.hpp:26-57); the complement as the
// mapper takes it (src/common.hpp:28-44)
inline u8 letter_nibble(char c, bool a_rich) {
  switch (c) {
    case 'A': return a_rich ? 5 : 1;
    case 'C': return 2;
    case 'G': return 4;
    case 'T': return a_rich ? 8 : 10;
    default: return 0;
  }
}
inline char complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }
// a read's four encodings, one nibble per base: enc = 2 * reverse-complement + A-rich
struct Read {
  u32 L = 0;
  std::vector<u8> nib[4];
};
inline Read encode(const std::string &s) {
  Read r;
  r.L = static_cast<u32>(s.size());
  for (int e = 0; e < 4; ++e) r.nib[e].resize(s.size());
  for (u32 k = 0; k < r.L; ++k) {
    const char f = s[k], c = complement(s[r.L - 1 - k]);
    r.nib[0][k] = letter_nibble(f, false); r.nib[1][k] = letter_nibble(f, true);
    r.nib[2][k] = letter_nibble(c, false); r.nib[3][k] = letter_nibble(c, true);
  }
  return r;
}
// packed as the mapper packs: 16 nibbles a word, 0xF past the read, W words per encoding
inline void pack(const Read &r, u32 W, u64 *dst) {
  for (u32 e = 0; e < 4; ++e)
    for (u32 w = 0; w < W; ++w) {
      u64 x = 0;
      for (u32 j = 0; j < 16; ++j) {
        const u32 k = 16 * w + j;
        x |= static_cast<u64>(k < r.L ? r.nib[e][k] : 15u) << (4 * j);
      }
      dst[e * W + w] = x;
    }
}
inline std::string random_letters(Rng &rng, u32 L, bool with_n) {
  std::string s(L, 'A');
  for (auto &c : s) { const u32 x = rng.below(with_n ? 17 : 16); c = x == 16 ? 'N' : "ACGT"[x & 3]; }
  return s;
}

// ---- the genome: one nibble per base; 0 beyond its end ---------------------------------------------------------------
inline u32 g_at(const std::vector<u8> &g, u64 pos) { return pos < g.size() ? g[pos] : 0u; }
inline std::vector<u64> pack_genome(const std::vector<u8> &g) {
  std::vector<u64> w((g.size() + 15) / 16, 0);
  for (size_t k = 0; k < g.size(); ++k) w[k / 16] |= static_cast<u64>(g[k] & 15u) << (4 * (k % 16));
  return w;
}

struct Dist { int d, dmax; };
inline Dist serial_distance(const std::vector<u8> &g, const std::vector<u8> &q, u64 pos, u32 nwords) {
  int d = 0, m = 0;
  for (u32 w = 0; w < nwords; ++w) {
    int shared = 0;
    for (u32 j = 0; j < 16; ++j) {
      const u32 k = 16 * w + j;
      const u32 rn = k < q.size() ? q[k] : 15u;
      shared += __builtin_popcount(rn & g_at(g, pos + k));
    }
    d += 16 - shared;
    m = std::max(m, d);
  }
  return {static_cast<i16>(d), static_cast<i16>(m)};
}
inline u32 words_of(u32 L) { return (L + 15) / 16; }
// the read's own letters that do not match
inline int letter_count(const std::vector<u8> &g, const std::vector<u8> &q, u64 pos) {
  int d = 0;
  for (size_t k = 0; k < q.size(); ++k) d += (q[k] & g_at(g, pos + k)) == 0;
  return d;
}
// the same as the bit planes see a genome with blanks: two bits per base cannot say "blank", the planes hold code 0 (the
// letter of nibble 1) there.  (A nibble of two or more bits has no defined code: not for such genomes.)
inline int plane_count(const std::vector<u8> &g, const std::vector<u8> &q, u64 pos) {
  int d = 0;
  for (size_t k = 0; k < q.size(); ++k) { const u32 n = g_at(g, pos + k); d += (q[k] & (n ? n : 1u)) == 0; }
  return d;
}

// ---- the position cache ----------------------------------------------------------------------------------------------
constexpr u32 kCacheSlots = 256;
inline u32 cache_slot(u32 pos) { return static_cast<u32>(pos * 2654435761u) >> 24; }
struct CacheModel {
  std::vector<u32> slot[kCacheSlots];  // the positions the slot may hold; none = empty
  long hits = 0, evictions = 0, unsure = 0;
  void clear() { for (auto &s : slot) s.clear(); }
  struct Look { int hit_lo, hit_hi; };
  // one step: positions of the a half and of the b half (lanes in order).  Returns one Look per candidate, a's first.
  std::vector<Look> step(const std::vector<u32> &a, const std::vector<u32> &b) {
    std::vector<Look> out;
    auto look = [&](u32 pos) {
      const std::vector<u32> &s = slot[cache_slot(pos)];
      size_t same = 0;
      for (u32 p : s) same += p == pos;
      Look l = {(!s.empty() && same == s.size()) ? 1 : 0, same > 0 ? 1 : 0};
      if (l.hit_lo) ++hits;
      else if (l.hit_hi) ++unsure;
      else if (!s.empty()) ++evictions;
      return l;
    };
    for (u32 p : a) out.push_back(look(p));
    for (u32 p : b) out.push_back(look(p));
    // writes, slot by slot and for each thing the slot may have held at the step's start (0: nothing): the candidates that
    // missed THAT content write their positions, the a half first; where several of one half write, any of them may stay
    std::vector<u32> of_a[kCacheSlots], of_b[kCacheSlots];
    std::vector<u32> touched;
    for (u32 p : a) { const u32 k = cache_slot(p); if (of_a[k].empty() && of_b[k].empty()) touched.push_back(k); of_a[k].push_back(p); }
    for (u32 p : b) { const u32 k = cache_slot(p); if (of_a[k].empty() && of_b[k].empty()) touched.push_back(k); of_b[k].push_back(p); }
    for (u32 k : touched) {
      std::vector<u32> held = slot[k], after;
      if (held.empty()) held.push_back(0);
      auto add = [&](u32 p) { if (std::find(after.begin(), after.end(), p) == after.end()) after.push_back(p); };
      for (u32 c : held) {
        std::vector<u32> now = {c};
        for (const std::vector<u32> *half : {&of_a[k], &of_b[k]}) {
          std::vector<u32> writers;
          for (u32 p : *half) if (p != c) writers.push_back(p);  // (the lookups all saw the step's start)
          if (!writers.empty()) now = writers;
        }
        for (u32 p : now) add(p);
      }
      after.erase(std::remove(after.begin(), after.end(), 0u), after.end());
      slot[k] = after;
    }
    return out;
  }
};

// ---- the single-end candidate set (se_candidates, src/abismal.cpp:334-449) on libstdc++'s heap calls -----------------
constexpr u32 kSetCap = 50;
constexpr u32 kAmbigFlag = 0x100;
struct SetModel {
  struct El { i16 d; u32 flags, pos; };
  std::vector<El> v;
  u32 sz = 1;
  int cutoff = 0, good_cutoff = 0;
  El best = {0, 0, 0};
  bool sure_ambig = false;
  long updates = 0, fifo = 0;
  static bool by_d(const El &a, const El &b) { return a.d < b.d; }
  void reset(u32 readlen) {
    v.assign(kSetCap, El{0, 0, 0});
    v[0].d = static_cast<i16>(0.4 * readlen);
    best = {v[0].d, 0, 0};
    cutoff = v[0].d;
    good_cutoff = static_cast<i16>(readlen / 10u);
    sure_ambig = false;
    sz = 1;
    updates = fifo = 0;
  }
  void update(bool specific, int d, u32 flags, u32 pos) {
    // the updates the kernels apply a run at a time: a full set whose first, 25th and last elements sit at the cutoff,
    // and a newcomer that ties with it
    if (sz == kSetCap && v[0].d == cutoff && v[24].d == cutoff && v[49].d == cutoff && d == cutoff) ++fifo;
    ++updates;
    if (d == 0) {
      if (best.pos == 0) best = {0, flags, pos};
      else if (best.pos != pos || best.flags != flags) best.flags |= kAmbigFlag;
    }
    else {
      if (sz == kSetCap) { std::pop_heap(v.begin(), v.begin() + sz, by_d); v[sz - 1] = El{static_cast<i16>(d), flags, pos}; }
      else v[sz++] = El{static_cast<i16>(d), flags, pos};
      std::push_heap(v.begin(), v.begin() + sz, by_d);
    }
    sure_ambig = (best.flags & kAmbigFlag) && best.d == 0;
    cutoff = specific ? std::min<int>(cutoff, v[0].d) : v[0].d;
  }
  // check_hits (src/abismal.cpp:1133-1149) over one chunk in candidate order: a candidate goes in iff every running sum
  // of its comparison stays within the cutoff of that moment; nothing more once the read is surely ambiguous
  struct Lane { bool valid; int h, hmax; u32 pos; };
  void replay(bool specific, u32 flags, const std::vector<Lane> &chunk) {
    for (const Lane &l : chunk) {
      if (sure_ambig) return;
      if (!l.valid || l.hmax > cutoff) continue;
      update(specific, l.h, flags, l.pos);
    }
  }
};

// ---- ghost letters ---------------------------------------------------------------------------------------------------
// The reference keeps one read buffer per encoding and only resizes it (prep_read; src/abismal.cpp:1377-1386): a read of
// at least map_len bases overwrites positions [0, len), a shorter one is not prepared at all, and what lies beyond a
// read's end is what earlier reads left there -- zero where nothing was ever written.  The 2-letter bit of a nibble is 1
// iff it has neither bit 0 nor bit 2 (get_bit, src/AbismalIndex.hpp:255-269): 1 for the zero fill.
struct GhostBuffers {
  std::vector<u8> buf[4];
  void take(const Read &r, u32 map_len) {
    if (r.L < map_len) return;
    for (int e = 0; e < 4; ++e) {
      if (buf[e].size() < r.L) buf[e].resize(r.L, 0);
      std::copy(r.nib[e].begin(), r.nib[e].end(), buf[e].begin());
    }
  }
  u32 bit(int e, u32 k) const { const u32 n = k < buf[e].size() ? buf[e][k] : 0u; return (n & 5u) == 0u; }
};
// the two words of an encoding's bit string after the ghost letters of a read of L < 64 bases: bits below L as they
// were, bits L .. L + 63 from the buffers, 1 from L + 64 on
inline void ghost_words(const GhostBuffers &gb, int e, u32 L, u64 word0_before, u64 out[2]) {
  out[0] = word0_before & ((1ull << L) - 1);
  out[1] = 0;
  for (u32 p = L; p < 128; ++p) {
    const u64 b = p < L + 64 ? gb.bit(e, p) : 1u;
    out[p >> 6] |= b << (p & 63u);
  }
}

}  // namespace filter_host
