// abismal_amd device code: the single-end candidate set, resident in one wavefront (gfx950).
#pragma once
#include "abm_kernels.hpp"

namespace abm {

// =============================================================================
// Wave-resident single-end candidate set (se_candidates, src/abismal.cpp:334-449).
// The heap array lives across lanes: lane k holds heap slot k as one packed key
// diffs*256 + payload_slot; (flags,pos) payloads never move -- lane p holds the
// payload whose slot number is p.  A sift step therefore moves one register.
// =============================================================================
struct SeSet {
  static constexpr bool kFifo = true;
  static constexpr bool kAppend = false;
  int hk;   // per lane k: heap[k] = diffs*256 + payload slot
  u32 pf;   // per lane p: flags of payload p
  u32 pp;   // per lane p: pos of payload p
  int sz, cutoff, good_cutoff;
  int best_d;
  u32 best_f, best_p;
  bool sure_ambig;

  __device__ __forceinline__ static int key_d(int k) { return k >> 8; }
  __device__ __forceinline__ void begin_read(u32 readlen) {
    const int worst = static_cast<i16>(0.4 * readlen);  // se_element::reset(readlen), :292-296
    hk = worst * 256; pf = 0; pp = 0;  // sentinel: heap[0] -> payload 0 = {pos 0}
    sz = 1;
    cutoff = worst;
    good_cutoff = static_cast<i16>(readlen / 10u);
    best_d = worst; best_f = 0; best_p = 0;
    sure_ambig = false;
  }
  __device__ __forceinline__ int top_d() const { return key_d(rdlane(hk, 0)); }
  // libstdc++ __push_heap with `key` entering at `hole`, comparator diffs<
  __device__ __forceinline__ void sift_up(int hole, int key) {
    int parent = (hole - 1) / 2;
    while (hole > 0) {
      const int pk = rdlane(hk, parent);
      if (!(key_d(pk) < key_d(key))) break;
      wrlane(hk, hole, pk);
      hole = parent;
      parent = (hole - 1) / 2;
    }
    wrlane(hk, hole, key);
  }
  // libstdc++ pop_heap on [0,n): returns the payload slot of the evicted maximum;
  // the caller overwrites heap[n-1] and pushes, so only __adjust_heap of the
  // displaced last element is performed here
  __device__ __forceinline__ int pop_max(int n) {
    const int len = n - 1;
    const int freed = rdlane(hk, 0) & 255;
    const int vk = rdlane(hk, len);
    int hole = 0, second = 0;
    while (second < (len - 1) / 2) {
      second = 2 * (second + 1);
      int sk = rdlane(hk, second);
      const int lk = rdlane(hk, second - 1);
      if (key_d(sk) < key_d(lk)) { --second; sk = lk; }
      wrlane(hk, hole, sk);
      hole = second;
    }
    if ((len & 1) == 0 && second == (len - 2) / 2) {
      second = 2 * (second + 1);
      wrlane(hk, hole, rdlane(hk, second - 1));
      hole = second - 1;
    }
    sift_up(hole, vk);
    return freed;
  }
  // pop_heap + overwrite + push_heap on the FULL set (50 elements) in straight-line code: the evicted maximum's
  // payload slot takes (f, p) and the key d enters.  Same result as pop_max + sift_up above, derived from
  // libstdc++'s __adjust_heap / __push_heap:
  //  * the hole left by the root walks down 0 -> p1 -> .. -> pm, always to the right child unless it compares
  //    less than the left one, while the node has two children in the 49-element heap (node < 24): every sibling
  //    comparison is made at once (one DPP move + one ballot) and the walk is bit tests on the result;
  //  * the displaced last element vk then rises from pm while the element above compares less -- and the element
  //    above hole p(i) at that point is the one that started in p(i) -- so the net effect on the path is: nodes
  //    above p(j) take their path child's key, p(j) takes vk, nodes below keep theirs, where j is the deepest
  //    path index >= 1 whose original key does not compare less than vk (0 if there is none);
  //  * the newcomer enters at 49 and rises along 24, 11, 5, 2, 0 while the parent compares less.
  // Returns the key left at the root.
  __device__ __forceinline__ int replace_top(int d, u32 f, u32 p) {
    static_assert(kSeCap == 50, "paths derived for a 50-element heap");
    const int left = __builtin_amdgcn_update_dpp(0, hk, 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
    const u64 right_wins = __ballot(!(key_d(hk) < key_d(left)));  // bit r, r even: the hole moves to r rather than r - 1
    auto down = [&](int node) { const int r = 2 * node + 2; return ((right_wins >> r) & 1ull) ? r : r - 1; };
    const int root = rdlane(hk, 0), vk = rdlane(hk, 49);
    const int p1 = down(0), p2 = down(p1), p3 = down(p2), p4 = down(p3);
    const bool five = p4 < 24;
    const int p5 = five ? down(p4) : 63;  // (lane 63 is not part of the set: a harmless stand-in)
    const int k1 = rdlane(hk, p1), k2 = rdlane(hk, p2), k3 = rdlane(hk, p3), k4 = rdlane(hk, p4), k5 = rdlane(hk, p5);
    const int dv = key_d(vk);
    int j = 0;
    if (key_d(k1) >= dv) j = 1;
    if (key_d(k2) >= dv) j = 2;
    if (key_d(k3) >= dv) j = 3;
    if (key_d(k4) >= dv) j = 4;
    if (five && key_d(k5) >= dv) j = 5;
    wrlane(hk, 0, j == 0 ? vk : k1);
    wrlane(hk, p1, j > 1 ? k2 : (j == 1 ? vk : k1));
    wrlane(hk, p2, j > 2 ? k3 : (j == 2 ? vk : k2));
    wrlane(hk, p3, j > 3 ? k4 : (j == 3 ? vk : k3));
    wrlane(hk, p4, j > 4 ? k5 : (j == 4 ? vk : k4));
    wrlane(hk, p5, j == 5 ? vk : k5);
    const int slot = root & 255;
    wrlane(pf, slot, f);
    wrlane(pp, slot, p);
    const int nk = d * 256 + slot;
    const int c24 = rdlane(hk, 24), c11 = rdlane(hk, 11), c5 = rdlane(hk, 5), c2 = rdlane(hk, 2), c0 = rdlane(hk, 0);
    const bool b24 = key_d(c24) < d, b11 = b24 && key_d(c11) < d, b5 = b11 && key_d(c5) < d, b2 = b5 && key_d(c2) < d,
               b0 = b2 && key_d(c0) < d;
    wrlane(hk, 49, b24 ? c24 : nk);
    wrlane(hk, 24, b24 ? (b11 ? c11 : nk) : c24);
    wrlane(hk, 11, b11 ? (b5 ? c5 : nk) : c11);
    wrlane(hk, 5, b5 ? (b2 ? c2 : nk) : c5);
    wrlane(hk, 2, b2 ? (b0 ? c0 : nk) : c2);
    const int top = b0 ? nk : c0;
    wrlane(hk, 0, top);
    return top;
  }

  // A RUN of survivors that tie with the cutoff while the set is full and heap[0], heap[24] and heap[49] all sit at
  // the cutoff c (tandem repeats, homopolymer reads: hundreds of thousands of such updates per read).  Each is
  // pop_heap + overwrite + push_heap as in replace_top, and under these conditions that is a shift register:
  //  * the displaced last element heap[49] has distance c, the maximum, so it comes to rest at the deepest node of
  //    the hole's path that holds a c (j in replace_top; the c's of a path are a prefix of it, the heap being a
  //    heap), and everything above moves up one node: the path's c-prefix p0..pj takes p1..pj, heap[49];
  //  * the newcomer (distance c) enters at 49 and stays there, its parent 24 not comparing less;
  //  * every node keeps its distance, so the sibling comparisons -- hence the path -- are the same for the next tie.
  // So a tie is: evict heap[0]'s payload, shift keys along the chain p0 <- p1 <- .. <- pj <- 49, put the newcomer
  // (with the evicted payload slot) at 49.  After n = chain length updates every old element is gone and the payload
  // slots are back in the same places, so of a run of m only the last n + m % n (at most 13) need to be played.
  // `ties` = lanes whose candidate has distance c; the leading ones of `todo` that are ties are consumed.
  // Returns how many updates were applied (0: conditions not met, nothing done).
  __device__ __forceinline__ int tie_run(u64 &todo, u64 ties, u32 cand_pos, u32 f) {
    static_assert(kSeCap == 50, "paths derived for a 50-element heap");
    const int lane = lane_id();
    const int c = cutoff;
    if (sz != static_cast<int>(kSeCap) || key_d(rdlane(hk, 0)) != c || key_d(rdlane(hk, 24)) != c || key_d(rdlane(hk, 49)) != c)
      return 0;
    const u64 brk = todo & ~ties;
    u64 run = brk ? (todo & ((brk & (0 - brk)) - 1)) : todo;
    if (run == 0) return 0;
    const int m = __popcll(run);
    todo &= ~run;
    // the hole's path and its c-prefix
    const int left = __builtin_amdgcn_update_dpp(0, hk, 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
    const u64 right_wins = __ballot(!(key_d(hk) < key_d(left)));
    auto down = [&](int node) { const int r = 2 * node + 2; return ((right_wins >> r) & 1ull) ? r : r - 1; };
    const int p1 = down(0), p2 = down(p1), p3 = down(p2), p4 = down(p3);
    const int p5 = p4 < 24 ? down(p4) : 63;
    const bool e1 = key_d(rdlane(hk, p1)) == c, e2 = e1 && key_d(rdlane(hk, p2)) == c, e3 = e2 && key_d(rdlane(hk, p3)) == c,
               e4 = e3 && key_d(rdlane(hk, p4)) == c, e5 = e4 && p4 < 24 && key_d(rdlane(hk, p5)) == c;
    const int n = 2 + (e1 ? 1 : 0) + (e2 ? 1 : 0) + (e3 ? 1 : 0) + (e4 ? 1 : 0) + (e5 ? 1 : 0);  // chain length incl. 49
    // where each lane's key comes from in one shift
    int src = lane;
    wrlane(src, 0, e1 ? p1 : 49);
    if (e1) wrlane(src, p1, e2 ? p2 : 49);
    if (e2) wrlane(src, p2, e3 ? p3 : 49);
    if (e3) wrlane(src, p3, e4 ? p4 : 49);
    if (e4) wrlane(src, p4, e5 ? p5 : 49);
    if (e5) wrlane(src, p5, 49);
    // the survivors that leave a trace: the last n + m % n of the run
    int play = m;
    while (play >= 2 * n) play -= n;
    u64 last = 0, rest = run;
    for (int k = 0; k < play; ++k) {
      const int top = 63 - __builtin_clzll(rest);
      last |= 1ull << top;
      rest &= ~(1ull << top);
    }
    const int c256 = c * 256;
    while (last) {
      const int l = __builtin_ctzll(last);
      last &= last - 1;
      const int slot = rdlane(hk, 0) & 255;
      const u32 p = rdlane(cand_pos, l);
      hk = __builtin_amdgcn_ds_bpermute(src << 2, hk);
      wrlane(hk, 49, c256 + slot);
      wrlane(pp, slot, p);
      wrlane(pf, slot, f);
    }
    return m;
  }

  // se_candidates::update, :394-404
  __device__ __forceinline__ void admit(bool specific, int d, u32 f, u32 p) {
    if (d == 0) {
      if (best_p == 0) { best_d = 0; best_f = f; best_p = p; }
      else if (p != best_p || f != best_f) best_f |= kFlagAmbig;
    }
    int top;
    if (d != 0 && sz == static_cast<int>(kSeCap)) top = key_d(replace_top(d, f, p));
    else {
      if (d != 0) {
        const int slot = sz++;
        wrlane(pf, slot, f);
        wrlane(pp, slot, p);
        sift_up(sz - 1, d * 256 + slot);
      }
      top = top_d();
    }
    sure_ambig = (best_f & kFlagAmbig) && best_d == 0;
    cutoff = specific ? min(cutoff, top) : top;
  }
};

}  // namespace abm
