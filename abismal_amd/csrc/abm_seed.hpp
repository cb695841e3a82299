// abismal_amd device code: seeding, shared by the single-end and paired-end mapping kernels (gfx950, one wavefront
// per read / pair) -- the per-wave LDS view, keys and bucket narrowing, the candidate filters, and the seed pass.
#pragma once
#include "abm_kernels.hpp"
#include "abm_seed_bounds.hpp"

namespace abm {

// Per-wave LDS carve-up
struct WaveLds {
  u64 *qpk;    // [4][W] packed encodings
  u64 *qbits;  // [4][WB] 2-letter bit strings, bit j = bit2(nibble j), 1 past the end
  u64 *qmask;  // [4][MB][4] per block of 64 read bases: which of them admit genome code 0, 1, 2, 3 (cooperative filter)
  u16 *mark;   // [64] (paired-end mating)
  u32 *smark;  // [128] seed pass: where the segments of a flattened block begin inside the current 128-candidate step (locate128)
  u32 *sdelta; // [128] seed pass: per segment, index-array position minus candidate number of its first entry
  u32 *ctmp;   // [ctmp_cap] reversed CIGAR scratch
  u8 *tb;      // traceback bytes
  u64 *gwin;   // [kMaxJobs][GW] genome windows of the alignments in flight
  u32 *jpos;   // [kSeCap] alignment job list: position
  u32 *jdf;    // [kSeCap] alignment job list: diffs<<16 | flags
  int *lbest;  // [64]
  u64 *pcache; // [1 << kPosCacheBits] candidate cache: pos | diffs<<32 | max-prefix-diffs<<48
  u16 *hres;   // [128] distances of the candidates of one step (cooperative window loads)
  u32 W, WB, GW, MB;
  u32 G;       // lanes that share one candidate's window (4 or 8), 0 = one lane per window
  u32 max_jobs;  // window slots in gwin: kMaxJobs, or 2 in the long-read kernel (its bands are 61 lanes wide: one slot of lanes)
};
// The single-end kernels' carve: se_lds_layout over this wave's allocation.  LONG: the CIGAR scratch and the traceback
// table are this wave's pieces of global memory.
template <bool LONG> __device__ __forceinline__ void se_carve(WaveLds &lds, unsigned char *smem, const SeArgs &a) {
  const SeLds<unsigned char *> at = se_lds_layout(smem, LONG, lds_shape(a));
  lds.W = a.W; lds.WB = a.WB; lds.GW = a.GW; lds.G = a.G;
  lds.MB = LONG ? 0u : lds_mask_blocks(a.max_len);
  lds.max_jobs = at.slots;
  lds.qpk = reinterpret_cast<u64 *>(at.qpk);
  lds.qbits = reinterpret_cast<u64 *>(at.qbits);
  lds.qmask = reinterpret_cast<u64 *>(at.qmask);
  lds.ctmp = LONG ? a.long_ctmp + static_cast<u64>(blockIdx.x) * ((a.ctmp_cap + 1) & ~1u) : reinterpret_cast<u32 *>(at.ctmp);
  lds.jpos = reinterpret_cast<u32 *>(at.jpos);
  lds.jdf = reinterpret_cast<u32 *>(at.jdf);
  lds.gwin = reinterpret_cast<u64 *>(at.gwin);
  lds.pcache = reinterpret_cast<u64 *>(at.pcache);
  lds.tb = LONG ? a.long_tb + static_cast<u64>(blockIdx.x) * a.long_tb_bytes : at.tb;
  lds.lbest = reinterpret_cast<int *>(at.lbest);
  lds.smark = reinterpret_cast<u32 *>(at.smark);
  lds.sdelta = reinterpret_cast<u32 *>(at.sdelta);
  lds.mark = reinterpret_cast<u16 *>(at.mark);
  lds.hres = reinterpret_cast<u16 *>(lds.lbest);  // idle during the seed passes
}

__device__ __forceinline__ u32 q_nibble(const u64 *qpk, u32 k) {
  return static_cast<u32>(qpk[k >> 4] >> ((k & 15u) << 2)) & 15u;
}

// 16 consecutive read nibbles starting at base i (nibbles at or past L read as 0)
__device__ __forceinline__ u64 q_window16(const u64 *qpk, u32 W, u32 i, u32 L) {
  const u32 w = i >> 4, s = (i & 15u) << 2;
  u64 x = qpk[w] >> s;
  if (s && w + 1 < W) x |= qpk[w + 1] << (64 - s);
  const u32 have = i < L ? min(16u, L - i) : 0u;
  if (have < 16) x &= (have == 0 ? 0ull : ((1ull << (have << 2)) - 1));
  return x;
}

// The genome letter at position q as the narrowing loops need it: its 2-letter bit / its 3-letter sort symbol
// (from the nibble array: a probe can land on an N, which the bit planes cannot express).
__device__ __forceinline__ u32 genome_bit2(const DevIndex &ix, u64 q) { return bit2(gnib(ix.genome, q)); }
__device__ __forceinline__ u32 genome_sortsym3(const DevIndex &ix, u64 q, bool g_to_a) { return sortsym3(gnib(ix.genome, q), g_to_a); }
// Is an N within reach of a window or a probe at pos?  1 or 0.  (The bit planes and the window records cannot express
// an N: whoever reads letters from them asks here first.)
template <class Pos> __device__ __forceinline__ u32 n_within_reach(const u32 *__restrict__ nmap, Pos pos) {
  return (nmap[pos >> (kPlaneChunkBits + 5)] >> ((pos >> kPlaneChunkBits) & 31u)) & 1u;
}

// find_candidates (src/abismal.cpp:1163-1194) and find_candidates_three (:1214-1259) of one seed offset, advanced
// TOGETHER.  Both narrow a bucket letter by letter with std::lower_bound bisections (one per letter on the 2-letter
// table; two per letter -- first symbol >= mid, first symbol >= top -- on a 3-letter table, which start at the same
// midpoint and share probes until their paths part).  Every round issues the next probe of the 2-letter bisection
// and of both 3-letter bisections before any of them is waited for (three dependent chains of index-entry ->
// genome-letter loads in flight per lane instead of one after the other); each bisection sees exactly
// std::lower_bound's probe sequence, so the boundaries are the reference's even where a bucket's tail is unsorted.
// A chain with nothing to probe in a round reads entry 0 of its table and ignores it.  The read's letters of the
// 2-letter chain come from its bit string qb (n_bits of it; 1 beyond): the loop ends at p == limit, and for reads
// of 44-46 bases limit = L - i is BELOW the starting length for the last offsets, so the reference keeps extending
// past the end of the read, through whatever its reused buffer holds there (the ghost bits put into qb: ghost_bits).
//
// REC: the letters come from the window records (DevIndex::wrec): entry k's record holds the genome from wrec_back bases
// before the entry's position, so the letter p bases after it is bit wrec_back + p of record k -- ONE load that does not
// wait for the index entry, where the nibble array takes two in a row (the entry, then the letter behind it).  Two bits
// cannot say N: the record's one spare base (its last; the filter never reaches it) says whether the record's stretch
// holds a blank nibble, and such a probe -- like one beyond the record's reach, which only a read of 44-46 bases
// extending past its end can ask for -- goes the old way.
__device__ __forceinline__ u32 record_nibble(const DevIndex &ix, const u32 *__restrict__ tbl, u32 rec0, bool live, u32 k, u32 p) {
  const u32 at = ix.wrec_back + p, last = ix.wrec_blocks * 64u - 1u;
  const bool in_reach = at < last;
  const u64 *r = ix.wrec + 2ull * (live ? static_cast<u64>(k + rec0) * ix.wrec_blocks : 0ull);
  const u32 blk = in_reach ? at >> 6 : 0u;
  const u64 lo = r[2 * blk], hi = r[2 * blk + 1], flag = r[2 * (ix.wrec_blocks - 1)];
  u32 nib = 1u << ((static_cast<u32>(lo >> (at & 63u)) & 1u) | ((static_cast<u32>(hi >> (at & 63u)) & 1u) << 1));
  if (live && (!in_reach || (flag >> 63))) nib = gnib(ix.genome, static_cast<u64>(tbl[k]) + p);
  return nib;
}
template <bool REC = false>
__device__ __forceinline__ void narrow_both(const DevIndex &ix, const u32 *__restrict__ tbl3, bool g_to_a, const u64 *qb,
                                            u32 n_bits, const u64 *qpk, u32 qbase, u32 limit, u32 maxc, bool run2, u32 &lo2,
                                            u32 &hi2, u32 &len2, bool run3, u32 &lo3, u32 &hi3, u32 &len3, u32 &probes, u32 rec3 = 0) {
  // (len2 / len3 on entry: the letters each range has been narrowed by already -- the key weights, or more where the
  // seed-extension tables have taken the first steps; run2 / run3 false: the table has finished that chain, nothing
  // is done to its range)
  const u32 *__restrict__ tbl2 = ix.index;
  const u32 mid_sym = g_to_a ? 2u : 1u, top_sym = g_to_a ? 8u : 4u;
  u32 pA = len2, ploA = lo2, phiA = hi2, blA = 0;
  int bnA = 0;
  auto goA = [&]() { return pA != limit && (hi2 - lo2) > maxc && qbase + pA < n_bits + 4096u; };
  bool actA = run2 && goA();
  if (actA) { blA = lo2; bnA = static_cast<int>(hi2 - lo2); }
  u32 pB = len3, ploB = lo3, phiB = hi3, l1 = 0, l2 = 0;
  int n1 = 0, n2 = 0;
  auto goB = [&]() { return pB != limit && (hi3 - lo3) > maxc; };
  bool actB = run3 && goB();
  if (actB) { l1 = l2 = lo3; n1 = n2 = static_cast<int>(hi3 - lo3); }
  while (actA || actB) {
    const int hA = bnA >> 1, h1 = n1 >> 1, h2 = n2 >> 1;
    const u32 kA = blA + static_cast<u32>(hA), m1 = l1 + static_cast<u32>(h1), m2 = l2 + static_cast<u32>(h2);
    const bool dA = actA, d1 = actB && n1 > 0, d2 = actB && n2 > 0 && !(d1 && m2 == m1);
    u32 sA, s1, s2;
    if constexpr (REC) {
      sA = bit2(record_nibble(ix, tbl2, 0u, dA, kA, pA));
      s1 = sortsym3(record_nibble(ix, tbl3, rec3, d1, m1, pB), g_to_a);
      s2 = sortsym3(record_nibble(ix, tbl3, rec3, d2, m2, pB), g_to_a);
    }
    else {
      const u32 eA = tbl2[dA ? kA : 0u], e1 = tbl3[d1 ? m1 : 0u], e2 = tbl3[d2 ? m2 : 0u];
      sA = genome_bit2(ix, static_cast<u64>(eA) + pA);
      s1 = genome_sortsym3(ix, static_cast<u64>(e1) + pB, g_to_a);
      s2 = genome_sortsym3(ix, static_cast<u64>(e2) + pB, g_to_a);
    }
    probes += (dA ? 1u : 0u) + (d1 ? 1u : 0u) + (d2 ? 1u : 0u);
    if (actA) {  // one step of first_not (std::lower_bound's probe sequence), then find_candidates' update
      if (sA < 1u) { blA = kA + 1; bnA -= hA + 1; } else bnA = hA;
      if (bnA <= 0) {
        const u32 at = qbase + pA;
        const bool one = at < n_bits ? ((qb[at >> 6] >> (at & 63u)) & 1ull) != 0 : true;
        lo2 = one ? blA : lo2;
        hi2 = one ? hi2 : blA;
        ++pA;
        actA = goA();
        if (actA) { ploA = lo2; phiA = hi2; blA = lo2; bnA = static_cast<int>(hi2 - lo2); }
      }
    }
    if (actB) {
      if (n2 > 0 && n1 > 0 && m2 == m1) s2 = s1;
      if (n1 > 0) { if (s1 < mid_sym) { l1 = m1 + 1; n1 -= h1 + 1; } else n1 = h1; }
      if (n2 > 0) { if (s2 < top_sym) { l2 = m2 + 1; n2 -= h2 + 1; } else n2 = h2; }
      if (n1 <= 0 && n2 <= 0) {
        const u32 sym = sortsym3(q_nibble(qpk, qbase + pB), g_to_a);
        const u32 nlo = sym == 0 ? lo3 : (sym == mid_sym ? l1 : l2), nhi = sym == 0 ? l1 : (sym == mid_sym ? l2 : hi3);
        lo3 = nlo;
        hi3 = nhi;
        ++pB;
        actB = goB();
        if (actB) { ploB = lo3; phiB = hi3; l1 = l2 = lo3; n1 = n2 = static_cast<int>(hi3 - lo3); }
      }
    }
  }
  if (run2 && lo2 == hi2) { --pA; lo2 = ploA; hi2 = phiA; }
  if (run3 && lo3 == hi3) { --pB; lo3 = ploB; hi3 = phiB; }
  len2 = pA;
  len3 = pB;
}

__device__ __forceinline__ u32 every_fourth_bit(u64 t) {  // bits 0, 4, 8, ... of t -> 16 contiguous bits
  t &= 0x1111111111111111ull;
  t = (t | (t >> 3)) & 0x0303030303030303ull;
  t = (t | (t >> 6)) & 0x000F000F000F000Full;
  t = (t | (t >> 12)) & 0x000000FF000000FFull;
  t = (t | (t >> 24)) & 0xFFFFull;
  return static_cast<u32>(t);
}

// ---- direct narrowing of big buckets ---------------------------------------------------------------------------
// find_candidates / find_candidates_three extend a seed letter by letter while its range holds more than
// max_candidates entries, each letter a bisection of the range: for a seed inside a high-copy repeat that is dozens of
// letters times log2(range) dependent probes, each a random line -- a quarter of the kernel's line requests at hg38
// scale.  The loop's outcome can be had with far fewer.  Let m(k) be the number of letters, from the current depth p0
// on and at most T = limit - p0, that entry k shares with the read.  The range after t more letters is {k: m(k) >= t};
// the loop stops at the first t whose range holds at most maxc entries (stepping back one letter if that range is
// empty) or at T.  With V the (maxc + 1)-th largest m and Mmax the largest, that is t_f = V + 1 if V < T and Mmax > V,
// else V.  A bucket is sorted by those very letters (src/AbismalIndex.cpp:857-978, 256 of them), so m rises towards the
// place `ins` where the read would be inserted and falls after it: ins costs one bisection with whole-string
// comparisons (64 letters per step from the bit planes), V is the best min(m(s), m(s + maxc)) over windows of
// maxc + 1 entries around ins (a bisection on a monotone difference), and the final range's ends are two more
// bisections -- log2(range) + ~30 probes in all, whatever the depth.  Exact wherever the bisections are: same sortedness
// they rely on; entries within reach of an N (which the planes cannot express: nmap) send their lane back to the
// letter-by-letter loop.  mode 0: 2-letter table; 1 / 2: 3-letter table, C->T / G->A alphabet (letter classes as
// find_candidates_three orders them: below mid, mid, top and above).
__device__ __forceinline__ void classes16(int mode, u64 x, u32 &c1, u32 &c2) {
  const u64 y = mode == 1 ? x : x >> 1;  // sym = nib & 5: 1 -> class 1, 4 or 5 -> class 2;  sym = nib & 10: 2 -> class 1, 8 or 10 -> class 2
  c2 = every_fourth_bit(y >> 2);
  c1 = every_fourth_bit(y & ~(y >> 2));
}
// the read's letter classes for positions [s, s + 64) as two bit strings (2-letter table: its bit string and 0)
__device__ __forceinline__ void read_classes64(int mode, const u64 *qb, u32 n_bits, const u64 *qpk, u32 W, u32 L, u32 s, u64 &r1, u64 &r2) {
  if (mode == 0) {
    const u32 w = s >> 6, sh = s & 63u;
    const u64 a = s < n_bits ? qb[w] : ~0ull, b = s + 64 < n_bits ? qb[w + 1] : ~0ull;
    r1 = sh ? (a >> sh) | (b << (64 - sh)) : a;
    r2 = 0;
    return;
  }
  r1 = r2 = 0;
#pragma unroll
  for (u32 j = 0; j < 4; ++j) {
    u32 c1, c2;
    classes16(mode, q_window16(qpk, W, s + 16 * j, L), c1, c2);
    r1 |= static_cast<u64>(c1) << (16 * j);
    r2 |= static_cast<u64>(c2) << (16 * j);
  }
}
// (Inlined into the single-end kernel this search cost more than it saved: that kernel runs at the register budget of
// its filter loop, and 200 bytes per lane of scratch instead of 100 made every read slower -- 729 -> 780 ms per 10 M
// reads although the probes fell from 585 to 241 per read; profiles/r03_exp_direct_narrowing_*.  The pair kernels, built
// for 128 / 170 registers and bound by line requests of which a quarter are narrowing probes, are where it runs.)
struct DirectArgs { const u64 *planes0; const u32 *nmap; const u64 *qb; const u64 *qpk; u32 n_bits, W, L, maxc; };
struct DirectRange { u32 lo, hi, len, probes; bool ok; };
__device__ __forceinline__ DirectRange narrow_direct(int mode, DirectArgs da, const u32 *__restrict__ tbl, u32 qbase, u32 limit, u32 lo, u32 hi, u32 len) {
  const u64 *qb = da.qb, *qpk = da.qpk;
  const u32 n_bits = da.n_bits, W = da.W, L = da.L, maxc = da.maxc;
  u32 probes = 0;
  const u32 p0 = len, T = limit - p0, s0 = qbase + p0;
  u64 R1, R2;
  read_classes64(mode, qb, n_bits, qpk, W, L, s0, R1, R2);
  bool bad = false;
  // m(k) and how entry k compares with the read (cmp < 0: before it)
  auto eval = [&](u32 k, int &cmp) -> u32 {
    ++probes;
    const u64 q = static_cast<u64>(tbl[k]) + p0;
    if (n_within_reach(da.nmap, q)) bad = true;
    for (u32 w = 0; 64 * w < T; ++w) {
      const u64 at = q + 64 * w;
      const u64 *b = da.planes0 + 2 * (at / kPlaneBlock);
      const u32 sh = static_cast<u32>(at % kPlaneBlock);
      u64 gl = b[0] >> sh, gh = b[1] >> sh;
      if (sh) { gl |= b[2] << (64 - sh); gh |= b[3] << (64 - sh); }
      u64 r1 = R1, r2 = R2;
      if (w) read_classes64(mode, qb, n_bits, qpk, W, L, s0 + 64 * w, r1, r2);
      const u64 g1 = mode == 0 ? gl : (mode == 1 ? ~gl & ~gh : gl & ~gh);
      const u64 g2 = mode == 0 ? 0ull : (mode == 1 ? ~gl & gh : gl & gh);
      u64 x = (g1 ^ r1) | (g2 ^ r2);
      const u32 have = T - 64 * w;
      if (have < 64) x &= (1ull << have) - 1;
      if (x) {
        const u32 j = static_cast<u32>(__builtin_ctzll(x));
        const u32 gv = static_cast<u32>((g1 >> j) & 1ull) + 2u * static_cast<u32>((g2 >> j) & 1ull);
        const u32 rv = static_cast<u32>((r1 >> j) & 1ull) + 2u * static_cast<u32>((r2 >> j) & 1ull);
        cmp = gv < rv ? -1 : 1;
        return 64 * w + j;
      }
    }
    cmp = 0;
    return T;
  };
  // One loop, one probe per turn, whatever step of the search a lane is at (lanes of a wave are at different ones):
  //  kIns   bisection for `ins`, where the read would be inserted
  //  kWinL / kWinR  bisection for the first window start s1 with m(s1) >= m(s1 + maxc): m(s) - m(s + maxc) is <= 0 for
  //         windows left of ins, >= 0 from ins on and monotone in between, so the best window is at the sign change
  //  kV1 / kV2  V = max(m(s1 + maxc), m(s1 - 1)), whichever exist
  //  kM1 / kM2  the largest m: next to ins
  //  kLeft / kRight  the ends of {k: m(k) >= tf} (m does not fall towards ins from either side)
  enum { kIns, kWinL, kWinR, kV1, kV2, kM1, kM2, kTf, kLeft, kRight, kDone };
  const u32 d_lo = lo, d_hi = hi - 1 - maxc;  // window starts: s in [d_lo, d_hi]  (hi - lo > maxc)
  int phase = kIns;
  u32 base = lo, cnt = hi - lo, ins = lo, s1 = 0, sx = 0, ml = 0, V = 0, mmax = 0, tf = 0, left = lo, right = hi, r_end = hi;
  while (phase != kDone) {
    // transitions that need no probe
    if (phase == kIns && cnt == 0) {
      ins = base;
      const u32 a = ins > maxc + 1 ? max(d_lo, ins - maxc - 1) : d_lo, b_end = min(d_hi, ins);
      base = min(a, b_end); cnt = b_end + 1 - base;
      phase = kWinL;
    }
    if (phase == kWinL && cnt == 0) { s1 = base; phase = kV1; }
    if (phase == kV1 && s1 > d_hi) phase = kV2;
    if (phase == kV2 && s1 <= d_lo) phase = kM1;
    if (phase == kM1 && ins <= lo) phase = kM2;
    if (phase == kM2 && ins >= hi) phase = kTf;
    if (phase == kTf) {
      tf = (V < T && mmax > V) ? V + 1 : V;
      u32 l0 = lo;
      r_end = hi;
      if (tf == V + 1) { l0 = ins > maxc ? max(lo, ins - maxc) : lo; r_end = min(hi, ins + maxc); }  // (at most maxc entries, all next to ins)
      if (tf == 0) { left = lo; right = hi; phase = kDone; }
      else { base = l0; cnt = ins - l0; phase = kLeft; }
    }
    if (phase == kLeft && cnt == 0) { left = base; base = ins; cnt = r_end - ins; phase = kRight; }
    if (phase == kRight && cnt == 0) { right = base; phase = kDone; }
    if (phase == kDone) break;
    // this turn's probe
    const u32 half = cnt >> 1;
    u32 k;
    if (phase == kIns || phase == kLeft || phase == kRight) k = base + half;
    else if (phase == kWinL) { sx = base + half; k = sx; }
    else if (phase == kWinR) k = sx + maxc;
    else if (phase == kV1) k = s1 + maxc;
    else if (phase == kV2) k = s1 - 1;
    else if (phase == kM1) k = ins - 1;
    else k = ins;
    int c;
    const u32 m = eval(k, c);
    if (phase == kIns) { if (c < 0) { base += half + 1; cnt -= half + 1; } else cnt = half; }
    else if (phase == kWinL) { ml = m; phase = kWinR; }
    else if (phase == kWinR) { if (ml < m) { base = sx + 1; cnt -= half + 1; } else cnt = half; phase = kWinL; }
    else if (phase == kV1) { V = max(V, m); phase = kV2; }
    else if (phase == kV2) { V = max(V, m); phase = kM1; }
    else if (phase == kM1) { mmax = max(mmax, m); phase = kM2; }
    else if (phase == kM2) { mmax = max(mmax, m); phase = kTf; }
    else if (phase == kLeft) { if (m < tf) { base += half + 1; cnt -= half + 1; } else cnt = half; }
    else { if (m >= tf) { base += half + 1; cnt -= half + 1; } else cnt = half; }
  }
  DirectRange out;
  out.lo = left; out.hi = right; out.len = p0 + tf; out.probes = probes; out.ok = !bad;
  return out;
}


// full_compare (src/abismal.cpp:1105-1122).  The reference adds one word's mismatches at a
// time and gives up as soon as the running sum exceeds the cutoff, so a candidate is admitted
// iff EVERY prefix sum stays within the cutoff, and then with the complete distance.  Both are
// returned: d (complete) and dmax (largest prefix sum; equals d unless an IUPAC genome letter
// makes a word's contribution negative).
__device__ __forceinline__ int hamming(const u64 *__restrict__ genome, const u64 *qpk, u32 nwords,
                                       u32 pos, int &dmax) {
  const u64 *g = genome + (pos >> 4);
  const u32 sh = (pos & 15u) << 2;
  int d = 0, m = 0;
  u64 g0 = g[0];
  for (u32 w = 0; w < nwords; ++w) {
    const u64 g1 = g[w + 1];
    const u64 win = (g0 >> sh) | ((g1 << (63 - sh)) << 1);
    d += 16 - __popcll(qpk[w] & win);
    m = max(m, d);
    g0 = g1;
  }
  dmax = static_cast<i16>(m);
  return static_cast<i16>(d);
}
__device__ __forceinline__ int hamming(const u64 *__restrict__ genome, const u64 *qpk, u32 nwords, u32 pos) {
  int unused;
  return hamming(genome, qpk, nwords, pos, unused);
}
// the same for two windows at once: the genome words are fetched two at a time (16-byte loads,
// half as many requests as word-by-word), eight words of each window in flight per step (a lane
// whose `want` flag is off issues no loads and its results are meaningless)
__device__ __forceinline__ void hamming2(const u64 *__restrict__ genome, const u64 *qpk, u32 nwords,
                                         u32 pos_a, bool want_a, u32 pos_b, bool want_b, int &d_a,
                                         int &dmax_a, int &d_b, int &dmax_b) {
  typedef u64 pair_t __attribute__((ext_vector_type(2), aligned(8)));
  const u64 *ga = genome + (pos_a >> 4), *gb = genome + (pos_b >> 4);
  const u32 sa = (pos_a & 15u) << 2, sb = (pos_b & 15u) << 2;
  int da = 0, ma = 0, db = 0, mb = 0;
  u64 last_a = 0, last_b = 0;  // word c-1 of each window, carried into the next step
  auto word = [&](u32 w, u64 a0, u64 a1, u64 b0, u64 b1) {
    const u64 q = qpk[w];
    da += 16 - __popcll(q & ((a0 >> sa) | ((a1 << (63 - sa)) << 1)));
    ma = max(ma, da);
    db += 16 - __popcll(q & ((b0 >> sb) | ((b1 << (63 - sb)) << 1)));
    mb = max(mb, db);
  };
  for (u32 c = 0; c <= nwords; c += 8) {
    u64 xa[8], xb[8];
#pragma unroll
    for (u32 p = 0; p < 4; ++p) {
      const bool in = c + 2 * p <= nwords;
      pair_t va = {0ull, 0ull}, vb = {0ull, 0ull};
      if (want_a && in) va = *reinterpret_cast<const pair_t *>(ga + c + 2 * p);
      if (want_b && in) vb = *reinterpret_cast<const pair_t *>(gb + c + 2 * p);
      xa[2 * p] = va.x; xa[2 * p + 1] = va.y;
      xb[2 * p] = vb.x; xb[2 * p + 1] = vb.y;
    }
    if (c > 0 && c - 1 < nwords) word(c - 1, last_a, xa[0], last_b, xb[0]);
#pragma unroll
    for (u32 j = 0; j < 7; ++j)
      if (c + j < nwords) word(c + j, xa[j], xa[j + 1], xb[j], xb[j + 1]);
    last_a = xa[7];
    last_b = xb[7];
  }
  d_a = static_cast<i16>(da); dmax_a = static_cast<i16>(ma);
  d_b = static_cast<i16>(db); dmax_b = static_cast<i16>(mb);
}

// ---- candidate filter, cooperative form ----------------------------------------------
// A lane that fetches its own candidate's window issues one load per word, and with ~20 waves
// sharing a CU's L1 the line has often been evicted again before the next word asks for it: a
// window then costs several L1 misses.  Here G lanes (4 for reads up to 192 bp, 8 up to 448 bp)
// share a candidate and fetch its window from the genome's bit planes (DevIndex::planes), one
// 16-byte block of 64 bases per lane: a whole window is covered by a single instruction whose
// lanes coalesce into one line request.  Each lane counts the mismatches of its 64 read bases (the
// bits past its block come from the next lane), the group adds up, and the sums travel through LDS
// to the lanes that own the candidates.  The 128 candidates of a step are slots 0..63 (lane's
// first) and 64..127 (lane's second); 64/G of them are fetched per round, kCoopRounds rounds in
// flight (few: registers are better spent on a fifth wave per SIMD).
__device__ __forceinline__ int dpp_row_shl1(int v) {  // lane i <- lane i+1 within a row of 16 (last lane: 0)
  return __builtin_amdgcn_update_dpp(0, v, 0x101, 0xf, 0xf, false);
}
// Neighbour-lane moves across the whole wave.  (Here beside the other lane moves although alignment uses them most: the
// pair set's scan, abm_pe_set.hpp, needs from_next_lane and includes this header, not abm_align.hpp.)
// (bound_ctrl: the lane without a source reads 0 and no lane keeps its old value, so the destination needs no initialising move)
__device__ __forceinline__ int from_prev_lane(int v) {  // lane j <- lane j-1 (lane 0 <- 0)
  return __builtin_amdgcn_update_dpp(0, v, 0x138 /*wave_shr:1*/, 0xf, 0xf, true);
}
__device__ __forceinline__ int from_next_lane(int v) {  // lane j <- lane j+1 (lane 63 <- 0)
  return __builtin_amdgcn_update_dpp(0, v, 0x130 /*wave_shl:1*/, 0xf, 0xf, true);
}
__device__ __forceinline__ int group_sum(int v, u32 G) {  // sum over aligned groups of 4 or 8 lanes, in every lane
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1 /*quad_perm 1,0,3,2*/, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E /*quad_perm 2,3,0,1*/, 0xf, 0xf, false);
  if (G == 8) v += __builtin_amdgcn_update_dpp(0, v, 0x141 /*row_half_mirror*/, 0xf, 0xf, false);
  return v;
}
#ifndef ABM_COOP_ROUNDS
#define ABM_COOP_ROUNDS 2  // measured best with 20 waves per CU (round 2, profiles/r02_experiments.md): 1, 2, 4, 8 -> 937, 923, 959, 1386 ms
#endif
constexpr u32 kCoopRounds = ABM_COOP_ROUNDS;  // rounds of window loads in flight per lane

// Per block of 64 read bases and per encoding: the four masks "read base j admits genome code c" (bit c of the
// read's nibble; everything past the read admits every code, like the 0xF padding of the packed words).
__device__ __forceinline__ void build_qmasks(const WaveLds &lds, u32 L) {
  const int lane = lane_id();
  const u32 nblk = (L + kPlaneBlock - 1) / kPlaneBlock;
  for (u32 e = 0; e < 4; ++e)
    for (u32 s = 0; s < nblk; ++s) {
      const u32 i = s * kPlaneBlock + static_cast<u32>(lane);
      const u32 nib = i < L ? q_nibble(lds.qpk + e * lds.W, i) : 15u;
      const u64 m0 = __ballot(nib & 1u), m1 = __ballot(nib & 2u), m2 = __ballot(nib & 4u), m3 = __ballot(nib & 8u);
      if (lane == 0) {
        u64 *q = lds.qmask + (e * lds.MB + s) * 4;
        q[0] = m0; q[1] = m1; q[2] = m2; q[3] = m3;
      }
    }
}

// Hamming distances of 128 candidates (two per lane: pos_a of lane c = candidate c, pos_b = candidate 64 + c)
// against the genome's bit planes (DevIndex::planes).  G lanes share a candidate: lane s of the group loads block
// (pos >> 6) + s of the window -- one 16-byte load, every window inside one 128-byte line of one of the two
// copies -- and counts the mismatches of read bases [64 s, 64 s + 64): the genome bits it needs beyond its own
// block arrive by DPP from the next lane.  mismatches = 64 - popcount(the mask of the code each genome base has).
// Identical to full_compare's sum over whole words for a one-hot genome (src/abismal.cpp:1093-1122; the early exit
// there changes a distance only when the hit is rejected anyway).
template <u32 kRounds = kCoopRounds>
__device__ __forceinline__ void hamming_planes(const DevIndex &ix, const WaveLds &lds, const u64 *qm, u32 L,
                                               u32 pos_a, bool want_a, u32 pos_b, bool want_b, int &d_a, int &d_b) {
  const int lane = lane_id();
  const u32 G = lds.G, sub = lane & (G - 1), grp = lane / G, per_round = 64 / G;
  const u64 wa = __ballot(want_a), wb = __ballot(want_b);
  const bool counts = sub * kPlaneBlock < L;  // this lane has read bases to compare
  u64 m0 = 0, m1 = 0, m2 = 0, m3 = 0;
  if (counts) { const u64 *q = qm + sub * 4; m0 = q[0]; m1 = q[1]; m2 = q[2]; m3 = q[3]; }
  for (u32 pass = 0; pass * kRounds * per_round < 128; ++pass) {
    {  // a pass none of whose slots is wanted (most steps of an ordinary read hold a few candidates) costs nothing
      const u32 slot0 = pass * kRounds * per_round;
      const u64 w = (slot0 >= 64 ? wb : wa) >> (slot0 & 63u);
      if (kRounds * per_round < 64 && (w & ((1ull << (kRounds * per_round)) - 1)) == 0) continue;
      if (kRounds * per_round >= 64 && w == 0) continue;
    }
    u64 xl[kRounds], xh[kRounds];
    u64 shifts = 0;  // (pos & 63) of the rounds' candidates, eight bits each (up to eight rounds)
#pragma unroll
    for (u32 r = 0; r < kRounds; ++r) {
      const u32 slot = (pass * kRounds + r) * per_round + grp;  // < 128; a round lies entirely in one half
      const bool second = (pass * kRounds + r) * per_round >= 64;
      const u32 c = slot & 63u;
      const u32 cp = static_cast<u32>(__shfl(static_cast<int>(second ? pos_b : pos_a), static_cast<int>(c)));
      shifts |= static_cast<u64>(cp & 63u) << (8 * r);
      // (a group of four always fetches four blocks, 64 contiguous bytes: the memory pipeline merges the loads of a
      // full quad of lanes into one request, and those of a partly active quad not at all -- measured, 2.5 requests per
      // window against 1.2; a group of eight fetches the blocks its window has)
      const u32 b0 = cp / kPlaneBlock, b1 = G == 4 ? b0 + 3 : (cp + L - 1) / kPlaneBlock;
      const bool act = (((second ? wb : wa) >> c) & 1ull) && b0 + sub <= b1;
      // Every lane loads, unconditionally, so that the rounds' loads are issued back to back (a load under a
      // divergent branch is waited for inside it): a lane with nothing to fetch reads the array's first line.
      // What it gets is never looked at -- its bits could only reach read positions past the end, whose masks
      // admit every code, or candidates whose result is discarded.
      const u64 *g = act ? ix.planes[(b0 / kPlaneLineBlocks) != (b1 / kPlaneLineBlocks) ? 1 : 0] + 2 * static_cast<u64>(b0 + sub)
                         : ix.planes[0];
      xl[r] = g[0];
      xh[r] = g[1];
    }
#pragma unroll
    for (u32 r = 0; r < kRounds; ++r) {
      const u32 slot = (pass * kRounds + r) * per_round + grp;
      const u32 sh = static_cast<u32>(shifts >> (8 * r)) & 63u;
      const u64 nl = (static_cast<u64>(static_cast<u32>(dpp_row_shl1(static_cast<int>(xl[r] >> 32)))) << 32) |
                     static_cast<u32>(dpp_row_shl1(static_cast<int>(xl[r])));
      const u64 nh = (static_cast<u64>(static_cast<u32>(dpp_row_shl1(static_cast<int>(xh[r] >> 32)))) << 32) |
                     static_cast<u32>(dpp_row_shl1(static_cast<int>(xh[r])));
      const u64 gl = (xl[r] >> sh) | ((nl << (63 - sh)) << 1), gh = (xh[r] >> sh) | ((nh << (63 - sh)) << 1);
      const u64 match = (~gh & ((~gl & m0) | (gl & m1))) | (gh & ((~gl & m2) | (gl & m3)));
      int d = counts ? 64 - __popcll(match) : 0;
      d = group_sum(d, G);
      if (sub == 0) lds.hres[slot] = static_cast<u16>(d);
    }
  }
  wave_sync();
  d_a = static_cast<i16>(lds.hres[lane]);
  d_b = static_cast<i16>(lds.hres[64 + lane]);
  wave_sync();
}

// Reads of up to 128 bases: TWO lanes per candidate, each fetching two consecutive blocks (32 bytes: lane s of the
// pair takes blocks s and s + 1 of the window, so the middle block is asked for twice and costs nothing more) and
// counting 64 read bases against them -- no exchange between the lanes, and 32 candidates per round instead of 16:
// the kernel is bound by vector-instruction issue once its windows are single lines (76 % of the SIMDs' cycles),
// and this halves the filter's instructions per candidate.  One round (32 windows, 8 registers) in flight per pass.
__device__ __forceinline__ void hamming_planes_pairs(const DevIndex &ix, const WaveLds &lds, const u64 *qm, u32 L,
                                                     u32 pos_a, bool want_a, u32 pos_b, bool want_b, int &d_a, int &d_b) {
  const int lane = lane_id();
  const u32 sub = lane & 1u, grp = lane >> 1;
  const u64 wa = __ballot(want_a), wb = __ballot(want_b);
  const bool counts = sub * kPlaneBlock < L;
  u64 m0 = 0, m1 = 0, m2 = 0, m3 = 0;
  if (counts) { const u64 *q = qm + sub * 4; m0 = q[0]; m1 = q[1]; m2 = q[2]; m3 = q[3]; }
#pragma unroll 1
  for (u32 pass = 0; pass < 4; ++pass) {
    const u32 slot = pass * 32 + grp;  // < 128; passes 0-1 are the lanes' first candidates, 2-3 their second
    const bool second = pass >= 2;
    // (a pass none of whose 32 slots is wanted costs nothing: most steps of an ordinary read hold a few candidates)
    if (static_cast<u32>((second ? wb : wa) >> ((pass & 1u) * 32u)) == 0u) continue;
    const u32 c = slot & 63u;
    const u32 cp = static_cast<u32>(__shfl(static_cast<int>(second ? pos_b : pos_a), static_cast<int>(c)));
    const u32 sh = cp & 63u;
    const u32 b0 = cp / kPlaneBlock, b1 = b0 + 2;  // a window of up to 128 bases has at most three blocks
    const bool act = ((second ? wb : wa) >> c) & 1ull;
    // (unconditional loads, as in hamming_planes: a lane with nothing to fetch reads the array's first line)
    const u64 *g = act ? ix.planes[(b0 / kPlaneLineBlocks) != (b1 / kPlaneLineBlocks) ? 1 : 0] + 2 * static_cast<u64>(b0 + sub)
                       : ix.planes[0];
    const u64 xl = g[0], xh = g[1], nl = g[2], nh = g[3];
    const u64 gl = (xl >> sh) | ((nl << (63 - sh)) << 1), gh = (xh >> sh) | ((nh << (63 - sh)) << 1);
    const u64 match = (~gh & ((~gl & m0) | (gl & m1))) | (gh & ((~gl & m2) | (gl & m3)));
    int d = counts ? 64 - __popcll(match) : 0;
    d += __builtin_amdgcn_update_dpp(0, d, 0xB1 /*quad_perm 1,0,3,2*/, 0xf, 0xf, false);
    if (sub == 0) lds.hres[slot] = static_cast<u16>(d);
  }
  wave_sync();
  d_a = static_cast<i16>(lds.hres[lane]);
  d_b = static_cast<i16>(lds.hres[64 + lane]);
  wave_sync();
}

// Window records: ONE lane per candidate.  A record is a few blocks laid end to end, so a lane takes its own candidate's
// window with three (reads up to 128 bases) or four (up to 192) 16-byte loads of consecutive addresses -- the lanes of a
// segment read consecutive records -- and compares the read's 64-base blocks itself: no shuffles to hand candidates to
// groups of lanes, no sums through LDS, 64 windows in flight per half step instead of 32 or 16 -- 0.7 vector instructions
// per candidate of a 100-base read against 1.4 for the two-lane groups, 1 against 2.8 for the four-lane groups of a
// 150-base read.  (The bit planes need the groups: a window there is a random gather, which only a group's single load
// fetches in one request.)  a / b: the lane's first and (if `two`) second candidate of the step.  The blocks a lane loads
// past its candidate's record (at most one) only reach read positions past the end of the read, whose masks admit every code.
template <bool WIDE>
__device__ __forceinline__ void hamming_records_lane(const DevIndex &ix, const u64 *qm, u32 L, u32 rec_a, u32 x_a, bool want_a,
                                                     u32 rec_b, u32 x_b, bool want_b, bool two, int &d_a, int &d_b) {
  auto funnel = [](u64 lo, u64 hi, u32 sh) { return (lo >> sh) | ((hi << (63 - sh)) << 1); };
  auto mismatches = [&](u64 gl, u64 gh, const u64 *q) {
    const u64 match = (~gh & ((~gl & q[0]) | (gl & q[1]))) | (gh & ((~gl & q[2]) | (gl & q[3])));
    return 64 - __popcll(match);
  };
  if constexpr (!WIDE) {
    // both candidates' loads first: six registers each
    const u64 *ra = ix.wrec + (want_a ? 2 * (static_cast<u64>(rec_a) + x_a / kPlaneBlock) : 0ull);
    const u64 a0l = ra[0], a0h = ra[1], a1l = ra[2], a1h = ra[3], a2l = ra[4], a2h = ra[5];
    u64 b0l = 0, b0h = 0, b1l = 0, b1h = 0, b2l = 0, b2h = 0;
    if (two) {
      const u64 *rb = ix.wrec + (want_b ? 2 * (static_cast<u64>(rec_b) + x_b / kPlaneBlock) : 0ull);
      b0l = rb[0]; b0h = rb[1]; b1l = rb[2]; b1h = rb[3]; b2l = rb[4]; b2h = rb[5];
    }
    const bool wide = L > kPlaneBlock;  // (uniform: the read has a second block of masks)
    {
      const u32 sh = x_a & 63u;
      int d = mismatches(funnel(a0l, a1l, sh), funnel(a0h, a1h, sh), qm);
      if (wide) d += mismatches(funnel(a1l, a2l, sh), funnel(a1h, a2h, sh), qm + 4);
      d_a = d;
    }
    d_b = 0x7fff;
    if (two) {
      const u32 sh = x_b & 63u;
      int d = mismatches(funnel(b0l, b1l, sh), funnel(b0h, b1h, sh), qm);
      if (wide) d += mismatches(funnel(b1l, b2l, sh), funnel(b1h, b2h, sh), qm + 4);
      d_b = d;
    }
  }
  else {
    // up to three blocks of read: four blocks of record, one candidate after the other (eight registers of window)
    auto one = [&](u32 rec, u32 x, bool want) {
      const u64 *r = ix.wrec + (want ? 2 * (static_cast<u64>(rec) + x / kPlaneBlock) : 0ull);
      const u64 l0 = r[0], h0 = r[1], l1 = r[2], h1 = r[3], l2 = r[4], h2 = r[5], l3 = r[6], h3 = r[7];
      const u32 sh = x & 63u;
      int d = mismatches(funnel(l0, l1, sh), funnel(h0, h1, sh), qm);
      if (L > kPlaneBlock) d += mismatches(funnel(l1, l2, sh), funnel(h1, h2, sh), qm + 4);
      if (L > 2 * kPlaneBlock) d += mismatches(funnel(l2, l3, sh), funnel(h2, h3, sh), qm + 8);
      return d;
    };
    d_a = one(rec_a, x_a, want_a);
    d_b = two ? one(rec_b, x_b, want_b) : 0x7fff;
  }
}

// ---- flattened candidates of one 64-offset block ---------------------------------------
// Per lane (= seed offset g0 + lane): its checked 2-letter bucket [lo2, lo2 + na) and 3-letter bucket
// [lo3, lo3 + nb), laid end to end in the reference's visiting order (offset ascending, 2-letter
// before 3-letter, index order): candidate c of the block is entry start_a + ... of whichever
// segment contains c.  Segment number = 2 * lane + (1 for the 3-letter table).
struct Segs {
  u32 start_a, na, lo2, nb, lo3;
  __device__ __forceinline__ u32 start_b() const { return start_a + na; }
};
constexpr u32 kSegEpochLimit = (1u << 24) - 4;
// once per block: where each segment's entries lie relative to their candidate numbers
__device__ __forceinline__ void publish_segs(const WaveLds &lds, const Segs &sg) {
  typedef u32 u32x2 __attribute__((ext_vector_type(2)));
  const u32x2 v = {sg.lo2 - sg.start_a, sg.lo3 - sg.start_b()};
  *reinterpret_cast<u32x2 *>(lds.sdelta + 2 * lane_id()) = v;
}
// Which segment each of the 128 candidates c0 + lane (a) and c0 + 64 + lane (b) belongs to, and where its index
// entry is.  Every segment that begins inside the step leaves a mark at its first candidate, a running maximum
// spreads it over the candidates that follow, and candidates before the first mark belong to `carry`, the segment
// open at c0 (0 at c0 == 0; updated for c0 + 128).  Marks are tagged with the call's epoch (seg_epoch: one counter
// per wave, owned by the kernel) and never cleared: a stale mark is smaller than any mark of this call and loses
// the maximum.
__device__ __forceinline__ void locate128(const WaveLds &lds, u32 &seg_epoch, const Segs &sg, u32 c0, u32 total, u32 &carry, bool &va,
                                          bool &vb, u32 &seg_a, u32 &seg_b, u32 &ea_at, u32 &eb_at) {
  const int lane = lane_id();
  const u32 epoch = ++seg_epoch, tag = epoch << 8;
  const u32 da = sg.start_a - c0, db = sg.start_b() - c0;
  if (sg.na && da < 128u) lds.smark[da] = tag | static_cast<u32>(2 * lane + 1);
  if (sg.nb && db < 128u) lds.smark[db] = tag | static_cast<u32>(2 * lane + 2);
  wave_sync();
  const bool two = c0 + 64 < total;  // (uniform)
  u32 ma = lds.smark[lane], mb = two ? lds.smark[64 + lane] : 0u;
  ma = wave_incl_max(ma);
  seg_a = (ma >> 8) == epoch ? (ma & 255u) - 1u : carry;
  carry = rdlane(seg_a, 63);
  va = c0 + lane < total;
  ea_at = c0 + lane + lds.sdelta[seg_a];
  vb = false; seg_b = 0; eb_at = 0;
  if (two) {
    mb = wave_incl_max(mb);
    seg_b = (mb >> 8) == epoch ? (mb & 255u) - 1u : carry;
    carry = rdlane(seg_b, 63);
    vb = c0 + 64 + lane < total;
    eb_at = c0 + 64 + lane + lds.sdelta[seg_b];
  }
}

// Ghost bits.  The reference hashes a read's first max(20, L/2) seed offsets and extends the last
// ones while their buckets are too big; for reads of up to 46 bases (DevIndex::map_len .. 46) that reaches PAST the end of the read,
// into whatever the reused per-thread buffer of that encoding still holds: position k carries the
// nibble the nearest earlier read longer than k left there (prep_read only resizes;
// src/abismal.cpp:1163-1194, :1302-1308, :1377-1386; zero where nothing was written).
// This rebuilds those 2-letter bits for positions L .. L+63 of the four encodings of read r from the
// reads handed over before it (lens / packed of the same batch, input order = the reference at -t 1)
// and writes them into the bit strings qbits (>= 2 words per encoding).  Lane j <-> position L + j.
__device__ __forceinline__ void ghost_bits(const u64 *__restrict__ packed, const u32 *__restrict__ lens, u64 r, u32 L,
                                           u32 max_len, u32 map_len, u32 W, u32 WB, u64 *qbits) {
  const int lane = lane_id();
  const u32 k = L + static_cast<u32>(lane);
  bool found = k >= max_len;  // no read of this batch ever wrote that far: still the zero fill
  u64 src = 0;
  for (u64 base = r; base > 0 && __ballot(!found) != 0; base = base > 64 ? base - 64 : 0) {
    const u32 len_q = base > static_cast<u64>(lane) ? lens[base - 1 - lane] : 0u;
    for (int t = 0; t < 64; ++t) {
      const u32 lt = rdlane(len_q, t);
      if (!found && lt >= map_len && lt > k) { found = true; src = base - 1 - t; }
    }
  }
  const bool have = found && k < max_len && src < r && lens[src] > k;
#pragma unroll
  for (u32 e = 0; e < 4; ++e) {
    u32 nib = 0;
    if (have) nib = static_cast<u32>(packed[(src * 4 + e) * W + (k >> 4)] >> ((k & 15u) << 2)) & 15u;
    const u64 m = __ballot(bit2(nib) != 0);  // bit j = 2-letter bit at position L + j (1 for the zero fill)
    if (lane == 0) {
      const u64 real = qbits[e * WB] & ((1ull << L) - 1);
      qbits[e * WB] = real | (m << L);
      qbits[e * WB + 1] = (m >> (64 - L)) | (~0ull << L);
    }
  }
  wave_sync();
}

// One (strand, alphabet) call of process_seeds (src/abismal.cpp:1269-1375) for
// the whole wave.  Lanes are seed offsets while probing/narrowing, then become
// candidates (all checked buckets of 64 offsets flattened in reference order)
// for the Hamming filter; survivors are replayed in order into the set.
#ifndef ABM_SE_DIRECT_NARROWING
// (the single-end kernel narrows big ranges directly as well -- since the window records: until then it was neutral to
// slower there at either register budget; with the records the probes had become the largest phase of a
// 150-base read.  10 M x 100 bp 461-464 -> 438-440 ms, 4 M x 150 bp random PBAT 7.4-7.5 -> 8.3-8.5 M reads/s;
// profiles/r05_exp_se_direct_narrowing.log)
#define ABM_SE_DIRECT_NARROWING true
#endif
#ifndef ABM_SE_RECORD_PROBES
#define ABM_SE_RECORD_PROBES false
#endif
#ifndef ABM_HEAVY_BLOCK
#define ABM_HEAVY_BLOCK 4096
#endif
constexpr u32 kHeavyBlock = ABM_HEAVY_BLOCK;  // candidates in one block of 64 seed offsets from which a read counts as heavy
struct WorkTally {
  u32 seed_iters, probes, cands, words, updates, cache_hits;
  u32 fifo_updates, steps, light_steps;  // diagnostic build only
  // diagnostic build only (TIMED): shader cycles per phase, from s_memtime
  long long t_probe, t_stream, t_replay, t_align, t_total;
};
// a stamp drains outstanding memory traffic first so that waits are charged to the
// phase that issued them (the scheduler may otherwise hoist s_memtime above the wait)
__device__ __forceinline__ long long phase_stamp() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
  __builtin_amdgcn_sched_barrier(0);
  return static_cast<long long>(t);
}
#define ABM_STAMP(var) do { if (TIMED) var = phase_stamp(); } while (0)

// REC: the launch filters on the window records (DevIndex::wrec; every read of the launch is short enough for them).  A
// candidate's window is then addressed by its entry NUMBER, so the step neither waits for the index entries nor reads them
// at all, except for the few candidates whose distance is within the cutoff: those alone need a position -- for the
// set, and to ask whether an N is within reach of the window (the planes' distance never exceeds the true one -- a blank
// nibble matches nothing, the planes' code 0 there may match -- so a candidate beyond the cutoff on the planes is beyond
// it on the nibble array too; not so for IUPAC letters, DevIndex::multibit, whose candidates the record's flag picks out
// before the cutoff test).  No position cache either: a repeated window costs a third of a line, not a line.
//
// The bounds memo (REC, single-end): the sensitive pass looks the first max(window, L/2) offsets up again, with the keys the
// specific pass of the same call has just used on the same lanes, and of a base bucket it needs only the exact range, or that
// it holds more than max_candidates (abm_seed_bounds.hpp).  The specific pass knows one or the other before it narrows
// anything -- from the table entry, or from the counters where it had to load them -- and leaves it in the idle cache
// region (16 bytes per offset; abm_lds_layout.hpp); the sensitive pass then loads no counter for those offsets.
// memo_n: offsets recorded by this call's specific pass (uniform; owned by the kernel like seg_epoch).
#ifndef ABM_SE_BOUNDS_MEMO
#define ABM_SE_BOUNDS_MEMO true  // (false: the sensitive pass loads every offset's counters, for same-box comparisons)
#endif
template <bool REC, class Set> constexpr bool kBoundsMemo = REC && !Set::kAppend && ABM_SE_BOUNDS_MEMO;

// What one (strand, alphabet) call knows before its first offset: the read's encodings, the alphabet's tables, and the
// pass's constants.  Built once by seed_call; the stages read it.
struct SeedCall {
  const u64 *qpk, *qb, *qmask;  // the encoding's packed nibbles, 2-letter bit string (n_bits of it), filter masks
  const u32 *cnt3, *idx3;       // the alphabet's 3-letter counters and index array
  u32 rec3;                     // (REC) record number of the 3-letter table's first entry
  u32 W, n_bits, L, nwords, maxc;
  u32 spec_len, n_off;
  bool g_to_a;
  bool use_ext;                 // the seed-extension tables answer for this pass's offsets
  bool memo_fits;               // (specific pass; uniform) the bounds memo has a slot for every offset
};
template <bool SPECIFIC, bool MEMO>
__device__ __forceinline__ SeedCall seed_call(const DevIndex &ix, const WaveLds &lds, u32 enc, bool g_to_a, u32 L) {
  SeedCall sc;
  sc.qpk = lds.qpk + enc * lds.W;
  sc.qb = lds.qbits + enc * lds.WB;
  sc.cnt3 = g_to_a ? ix.counter_a : ix.counter_t;
  sc.idx3 = g_to_a ? ix.index_a : ix.index_t;
  sc.maxc = ix.max_candidates;
  sc.nwords = (L + 15) >> 4;
  sc.spec_len = min(L - ix.window, L >> 1);
  sc.n_off = SPECIFIC ? max(ix.window, L >> 1) : L - kKeyWeight + 1;
  // the tables answer for offsets whose seed can be extended by all their letters inside the read (L - i >= depth for
  // every offset of the pass) and for the max_candidates they were built with; otherwise the loops start at the counters
  sc.use_ext = SPECIFIC && ix.ext2 != nullptr && ix.ext_maxc == sc.maxc &&
               L - sc.n_off + 1 >= max(kKeyWeight + ix.e2, kKeyWeight3 + ix.e3);
  sc.rec3 = g_to_a ? ix.wrec_a0 : ix.wrec_t0;
  sc.memo_fits = MEMO && sc.n_off <= kBoundsMemoSlots;
  sc.qmask = lds.qmask + enc * lds.MB * 4;
  sc.W = lds.W;
  sc.n_bits = 64u * lds.WB;
  sc.L = L;
  sc.g_to_a = g_to_a;
  return sc;
}

// ---- stage 1, per seed offset (one lane each): which buckets to check ------------------------------------------
// the keys of offset i: the read's next 64 2-letter bits, its 25-bit 2-letter key and its 16-digit base-3 key
__device__ __forceinline__ void seed_keys(const SeedCall &sc, u32 i, u64 &bits, u32 &k2, u32 &k3) {
  // 25-bit 2-letter key, MSB first (get_1bit_hash, src/AbismalIndex.hpp:285-294)
  const u32 wq = i >> 6, sq = i & 63u;
  bits = sc.qb[wq] >> sq;
  if (sq) bits |= sc.qb[wq + 1] << (64 - sq);
  k2 = __brev(static_cast<u32>(bits) & 0x1FFFFFFu) >> 7;
  // 16-digit base-3 key (get_base_3_hash, src/AbismalIndex.hpp:296-305)
  const u64 win = q_window16(sc.qpk, sc.W, i, sc.L);
  k3 = 0;
#pragma unroll
  for (u32 j = 0; j < 16; ++j)
    k3 = k3 * 3u + trit(static_cast<u32>(win >> (j << 2)) & 15u, sc.g_to_a);
}

// The two narrowing chains of one offset: the 2-letter and the 3-letter range, the letters each has been narrowed by,
// and whether it is still open (false: finished, nothing more is done to its range).
struct Chains {
  u32 lo2, hi2, len2, lo3, hi3, len3;
  bool run2, run3;
};
__device__ __forceinline__ u64 memo_entry(u32 lo, u32 d) { return lo | (static_cast<u64>(d) << 32); }

// Where the chains stand before any narrowing -- from the seed-extension tables or the counters -- and (MEMO) what the
// sensitive pass of this call will want to know of the offset's base buckets, left in the bounds memo.
template <bool MEMO>
__device__ __forceinline__ Chains specific_start(const DevIndex &ix, const WaveLds &lds, const SeedCall &sc, u32 i, u64 bits,
                                                 u32 k2, u32 k3) {
  Chains c;
  c.len2 = kKeyWeight; c.len3 = kKeyWeight3;
  c.run2 = true; c.run3 = true;
  if (sc.use_ext) {
    // seed-extension tables (abm_ext.hip): one independent 8-byte load per table says where the narrowing
    // loops stand after the next e2 / e3 letters -- for most offsets, finished
    const u32 D2 = kKeyWeight + ix.e2;
    const u32 K2 = __brev(static_cast<u32>(bits) & (D2 >= 32 ? 0xFFFFFFFFu : (1u << D2) - 1u)) >> (32 - D2);
    const u64 more = q_window16(sc.qpk, sc.W, i + 16, sc.L);
    u32 K3 = k3;
    for (u32 j = 0; j < ix.e3; ++j) K3 = K3 * 3u + trit(static_cast<u32>(more >> (j << 2)) & 15u, sc.g_to_a);
    const uint2 x2 = ix.ext2[K2], x3 = (sc.g_to_a ? ix.ext3a : ix.ext3t)[K3];
    const u32 st2 = x2.y >> 30, st3 = x3.y >> 30;
    c.lo2 = x2.x; c.hi2 = x2.x + (x2.y & 0x7FFFFFFu); c.len2 = kKeyWeight + ((x2.y >> 27) & 7u); c.run2 = st2 != 0;
    c.lo3 = x3.x; c.hi3 = x3.x + (x3.y & 0x7FFFFFFu); c.len3 = kKeyWeight3 + ((x3.y >> 27) & 7u); c.run3 = st3 != 0;
    if (st2 == 2) { c.lo2 = ix.counter[k2]; c.hi2 = ix.counter[k2 + 1]; c.len2 = kKeyWeight; }  // (not tabulated)
    if (st3 == 2) { c.lo3 = sc.cnt3[k3]; c.hi3 = sc.cnt3[k3 + 1]; c.len3 = kKeyWeight3; }
    if constexpr (MEMO) if (sc.memo_fits) {
      const BucketFact f2 = st2 == 2 ? BucketFact{c.lo2, c.hi2 - c.lo2} : bucket_fact_from_table(x2.x, x2.y);
      const BucketFact f3 = st3 == 2 ? BucketFact{c.lo3, c.hi3 - c.lo3} : bucket_fact_from_table(x3.x, x3.y);
      lds.pcache[2 * i] = memo_entry(f2.lo, f2.d);
      lds.pcache[2 * i + 1] = memo_entry(f3.lo, f3.d);
    }
  }
  else {
    c.lo2 = ix.counter[k2]; c.hi2 = ix.counter[k2 + 1];
    c.lo3 = sc.cnt3[k3];    c.hi3 = sc.cnt3[k3 + 1];
    if constexpr (MEMO) if (sc.memo_fits) {
      lds.pcache[2 * i] = memo_entry(c.lo2, c.hi2 - c.lo2);
      lds.pcache[2 * i + 1] = memo_entry(c.lo3, c.hi3 - c.lo3);
    }
  }
  return c;
}

// Big ranges -- seeds inside high-copy repeats -- are narrowed directly (narrow_direct): reads up to kSortDepth bases,
// ranges of at least direct_min entries and more than maxc, a chain not yet at its limit.  A result counts only if
// `ok`; small ranges, and lanes whose probes come within reach of an N, are left to the letter-by-letter loop.
__device__ __forceinline__ void narrow_direct_chains(const DevIndex &ix, const SeedCall &sc, u32 i, Chains &c, u32 &probes) {
  if (ix.direct_min == 0 || sc.L > kSortDepth || ix.planes[0] == nullptr) return;
  const u32 limit = sc.L - i;
  const DirectArgs da = {ix.planes[0], ix.nmap, sc.qb, sc.qpk, sc.n_bits, sc.W, sc.L, sc.maxc};
  // (the loop runs on locals: on the struct's members, picked by `three` inside the loop, nine of the single-end builds
  // came out with other scratch sizes and the long-read build with 129 registers for 127 -- a wave per SIMD less)
  u32 lo2 = c.lo2, hi2 = c.hi2, len2 = c.len2, lo3 = c.lo3, hi3 = c.hi3, len3 = c.len3;
  bool run2 = c.run2, run3 = c.run3;
#pragma unroll 1
  for (int chain = 0; chain < 2; ++chain) {  // (one copy of the search in the code: 2-letter table, then the 3-letter one)
    const bool three = chain != 0;
    const u32 clo = three ? lo3 : lo2, chi = three ? hi3 : hi2, clen = three ? len3 : len2;
    // (clen < limit: the last offsets of a 44-46-base read start BEYOND the end of the read -- limit = L - i is below the
    // key weight -- and the reference extends those through whatever its reused buffer holds: the letter loop's
    // business, with the ghost bits)
    if ((three ? run3 : run2) && chi - clo >= ix.direct_min && chi - clo > sc.maxc && clen < limit) {
      const DirectRange r = narrow_direct(three ? (sc.g_to_a ? 2 : 1) : 0, da, three ? sc.idx3 : ix.index, i, limit, clo, chi, clen);
      probes += r.probes;
      if (r.ok) {
        if (three) { lo3 = r.lo; hi3 = r.hi; len3 = r.len; run3 = false; }
        else { lo2 = r.lo; hi2 = r.hi; len2 = r.len; run2 = false; }
      }
    }
  }
  c = {lo2, hi2, len2, lo3, hi3, len3, run2, run3};
}

// The checked buckets of one live offset: entries [lo2, hi2) of the 2-letter table if chk2, [lo3, hi3) of the
// 3-letter one if chk3.
struct OffsetBuckets {
  u32 lo2, hi2, lo3, hi3;
  bool chk2, chk3;
};
template <bool SPECIFIC, bool TALLY, bool REC, class Set>
__device__ __forceinline__ OffsetBuckets offset_buckets(const DevIndex &ix, const WaveLds &lds, const SeedCall &sc, u32 i,
                                                        u32 memo_n, WorkTally &wt) {
  constexpr bool kMemo = kBoundsMemo<REC, Set>;
  constexpr bool kDirect = Set::kAppend ? ABM_PE_DIRECT_NARROWING : ABM_SE_DIRECT_NARROWING;
  OffsetBuckets b;
  // (sensitive pass: an offset the specific pass of this call recorded needs neither keys nor counters)
  const bool memo_hit = kMemo && !SPECIFIC && i < memo_n;
  u64 bits = 0;
  u32 k2 = 0, k3 = 0;
  if (!memo_hit) seed_keys(sc, i, bits, k2, k3);
  // (the bounds memo, measured on the record-fed kernel, 10 M x 100 bp: 1,710 -> 1,487 lines requested per read, -13 %,
  // and 432 -> 423 ms per launch, three alternating runs each of 440.7-443.9 and 433.2-435.6 ms per step --
  // profiles/se_bounds_memo_bench_ab.log.  The same idea with the counters in LDS of its own, when the repeated lines
  // were 4.4 % of a read's, had made the kernel of that time 1.6 % slower.)
  // (keeping the specific pass's distances too, one byte per candidate, so that the sensitive pass fetches no window for
  // a bucket entry it has seen: 290 of 2,850 candidates per read found there, -7 % lines, and 2.3 KB more LDS per wave
  // cost 15 % of the time -- profiles/r02_exp_distance_memo.log.  Not measured again on the idle cache region, where
  // it would cost no LDS.)
  if (SPECIFIC) {
    u32 probes = 0;
    Chains c = specific_start<kMemo>(ix, lds, sc, i, bits, k2, k3);
    if constexpr (kDirect) narrow_direct_chains(ix, sc, i, c, probes);
    // (letters from the window records in the pair kernels only: the single-end kernel, short of registers, is 6 %
    // slower with them -- 527 -> 558 ms per 10 M reads -- where the pair kernels' seed passes gain 1.5 %;
    // profiles/r05_exp_record_probes.log)
    narrow_both<REC && (Set::kAppend || ABM_SE_RECORD_PROBES)>(ix, sc.idx3, sc.g_to_a, sc.qb, sc.n_bits, sc.qpk, i, sc.L - i, sc.maxc,
                                                               c.run2, c.lo2, c.hi2, c.len2, c.run3, c.lo3, c.hi3, c.len3, probes, sc.rec3);
    b.lo2 = c.lo2; b.hi2 = c.hi2; b.chk2 = (c.hi2 - c.lo2) <= sc.maxc || c.len2 >= sc.spec_len;
    b.lo3 = c.lo3; b.hi3 = c.hi3; b.chk3 = (c.hi3 - c.lo3) <= sc.maxc || c.len3 >= sc.spec_len;
    if (TALLY) wt.probes += probes;
  }
  else if constexpr (kMemo) {
    BucketFact f2, f3;
    if (memo_hit) {
      const u64 m2 = lds.pcache[2 * i], m3 = lds.pcache[2 * i + 1];
      f2 = {static_cast<u32>(m2), static_cast<u32>(m2 >> 32)};
      f3 = {static_cast<u32>(m3), static_cast<u32>(m3 >> 32)};
    }
    else {
      f2.lo = ix.counter[k2]; f2.d = ix.counter[k2 + 1] - f2.lo;
      f3.lo = sc.cnt3[k3];    f3.d = sc.cnt3[k3 + 1] - f3.lo;
    }
    const SensBounds s = sensitive_bounds(f2, f3, sc.maxc);
    b.chk2 = s.chk2; b.lo2 = s.lo2; b.hi2 = s.lo2 + s.n2;
    b.chk3 = s.chk3; b.lo3 = s.lo3; b.hi3 = s.lo3 + s.n3;
  }
  else {
    b.lo2 = ix.counter[k2]; b.hi2 = ix.counter[k2 + 1];
    b.lo3 = sc.cnt3[k3];    b.hi3 = sc.cnt3[k3 + 1];
    const u32 d2 = b.hi2 - b.lo2, d3 = b.hi3 - b.lo3;
    b.chk2 = d2 != 0 && d2 <= sc.maxc && (d3 == 0 || d2 <= 10u * d3);
    b.chk3 = d3 != 0 && d3 <= sc.maxc;
  }
  if (TALLY) ++wt.seed_iters;
  return b;
}

// ---- stage 3, per step of 128 candidates: filter, then replay in order -----------------------------------------
// rare: the distances of the lanes whose window has an N within reach (na / nb) are redone on the nibble array, where
// an N is an N -- and an IUPAC letter (DevIndex::multibit) an IUPAC letter: such a letter can make a word's share
// negative, so a redone candidate carries its own largest prefix sum (hma / hmb), which admission follows
__device__ __forceinline__ void redo_on_nibbles(const DevIndex &ix, const SeedCall &sc, u32 na, u32 pa, int &ha, int &hma, u32 nb, u32 pb,
                                                int &hb, int &hmb) {
  if (__any(na | nb)) {
    if (na) ha = hamming(ix.genome, sc.qpk, sc.nwords, pa, hma);
    if (nb) hb = hamming(ix.genome, sc.qpk, sc.nwords, pb, hmb);
  }
}

// One entry of the position cache (WaveLds::pcache): pos | diffs << 32 | max-prefix-diffs << 48; 0 = empty.
struct PosCacheEntry {
  u64 v;
  __device__ __forceinline__ static u64 *slot(const WaveLds &lds, u32 pos) { return lds.pcache + ((pos * 2654435761u) >> (32 - kPosCacheBits)); }
  __device__ __forceinline__ static u64 pack(u32 pos, int h, int hmax) {
    return static_cast<u64>(pos) | (static_cast<u64>(static_cast<u16>(h)) << 32) | (static_cast<u64>(static_cast<u16>(hmax)) << 48);
  }
  __device__ __forceinline__ bool matches(u32 pos) const { return static_cast<u32>(v) == pos; }
  __device__ __forceinline__ void distances(int &h, int &hmax) const {
    h = static_cast<i16>(static_cast<u16>(v >> 32));
    hmax = static_cast<i16>(static_cast<u16>(v >> 48));
  }
};

// What a filter step hands to the replay, per lane and half (a: candidate c0 + lane, b: c0 + 64 + lane): whether the
// candidate is offered to the set, its position, its distance and largest prefix sum.  seen / cached: the lane's
// candidates of the step and how many of them the position cache answered (for the tallies).
struct FilterStep {
  bool va, vb;
  u32 pa, pb;
  int ha, hma, hb, hmb;
  u32 seen, cached;
};
// Where a block's candidate loop stands: the segment open at the step's first candidate (locate128) and, in the window
// loop, the NEXT step's candidates with their index entries, requested one step ahead.
struct StepCursor {
  u32 carry;
  bool nva, nvb;
  u32 nsa, nsb, nea, neb;
};
__device__ __forceinline__ void fetch_entries(const DevIndex &ix, const WaveLds &lds, const SeedCall &sc, u32 &seg_epoch, const Segs &sg,
                                              u32 c0, u32 total, StepCursor &cur) {
  u32 ea_at, eb_at;
  locate128(lds, seg_epoch, sg, c0, total, cur.carry, cur.nva, cur.nvb, cur.nsa, cur.nsb, ea_at, eb_at);
  cur.nea = 0; cur.neb = 0;
  if (cur.nva) cur.nea = (cur.nsa & 1u) ? sc.idx3[ea_at] : ix.index[ea_at];
  if (cur.nvb) cur.neb = (cur.nsb & 1u) ? sc.idx3[eb_at] : ix.index[eb_at];
}

// One step on the window records (REC, see above): distances by entry number, positions for the survivors alone.
template <class Set>
__device__ __forceinline__ FilterStep filter_step_records(const DevIndex &ix, const WaveLds &lds, const SeedCall &sc, const Set &S,
                                                          u32 &seg_epoch, const Segs &sg, u32 g0, u32 c0, u32 total, bool two,
                                                          StepCursor &cur) {
  bool va, vb;
  u32 sa, sb, ea, eb;
  locate128(lds, seg_epoch, sg, c0, total, cur.carry, va, vb, sa, sb, ea, eb);
  const u32 ia = g0 + (sa >> 1), ib = g0 + (sb >> 1);
  // record start (in 16-byte blocks) and the bit of the record the window begins at
  const u32 ra = (ea + ((sa & 1u) ? sc.rec3 : 0u)) * ix.wrec_blocks, rb = (eb + ((sb & 1u) ? sc.rec3 : 0u)) * ix.wrec_blocks;
  // A genome with IUPAC letters (uniform; no other genome takes this branch): such a letter can match where its arbitrary
  // plane code does not, so the planes' distance is no lower bound there and the cutoff test below may not drop a
  // candidate whose stretch holds one.  The record's own flag says so without the position: one 8-byte load per
  // candidate, from the last block of a record whose lines the window's loads ask for anyway.
  u32 fa = 0, fb = 0;
  if (ix.multibit) {
    if (va) fa = static_cast<u32>(ix.wrec[2 * (static_cast<u64>(ra) + ix.wrec_blocks - 1)] >> 63);
    if (two && vb) fb = static_cast<u32>(ix.wrec[2 * (static_cast<u64>(rb) + ix.wrec_blocks - 1)] >> 63);
  }
  int ha, hb = 0x7fff;
  if (lds.G == 2)
    hamming_records_lane<false>(ix, sc.qmask, sc.L, ra, ix.wrec_back - ia, va, rb, ix.wrec_back - ib, vb, two, ha, hb);
  else
    hamming_records_lane<true>(ix, sc.qmask, sc.L, ra, ix.wrec_back - ia, va, rb, ix.wrec_back - ib, vb, two, ha, hb);
  // the candidates that may still enter the set: these alone need their position
  const bool ca = va && (ha <= S.cutoff || fa), cb = two && vb && (hb <= S.cutoff || fb);
  u32 pa = 0, pb = 0;
  int hma = ha, hmb = hb;
  if (__any(ca || cb)) {
    if (ca) pa = ((sa & 1u) ? sc.idx3[ea] : ix.index[ea]) - ia;
    if (cb) pb = ((sb & 1u) ? sc.idx3[eb] : ix.index[eb]) - ib;
    const u32 na = ca ? (n_within_reach(ix.nmap, pa) | fa) : 0u, nb = cb ? (n_within_reach(ix.nmap, pb) | fb) : 0u;
    redo_on_nibbles(ix, sc, na, pa, ha, hma, nb, pb, hb, hmb);
  }
  return {ca, cb, pa, pb, ha, hma, hb, hmb, (va ? 1u : 0u) + (vb ? 1u : 0u), 0u};
}

// One step of the window loop: the step's candidates were located and their index entries requested a step ago
// (`cur`); the next step's are requested before this step's windows.
template <bool COOP>
__device__ __forceinline__ FilterStep filter_step_windows(const DevIndex &ix, const WaveLds &lds, const SeedCall &sc, u32 &seg_epoch,
                                                          const Segs &sg, u32 g0, u32 c0, u32 total, bool two, StepCursor &cur) {
  const bool va = cur.nva, vb = cur.nvb;
  const u32 pa = cur.nea - (g0 + (cur.nsa >> 1)), pb = cur.neb - (g0 + (cur.nsb >> 1));
  if (c0 + 128 < total) fetch_entries(ix, lds, sc, seg_epoch, sg, c0 + 128, total, cur);
  // the same genome position is proposed again and again (neighbouring seeds of one hit, the
  // sensitive pass repeating the specific one): a small per-call cache of (pos -> distances)
  // saves the 1-2 HBM lines of a window.  Distances are a pure function of (pos, encoding),
  // so a cache hit is exact by construction.  (Without it: 7 % more windows fetched, 18 instead of 25 spilled
  // VGPRs, 10 M reads 1.1 % faster and 1 M reads 2.4 % slower -- profiles/r02_exp_position_cache.log; kept.)
  u64 *slot_a = PosCacheEntry::slot(lds, pa), *slot_b = PosCacheEntry::slot(lds, pb);
  const PosCacheEntry ca = {va ? *slot_a : 0ull}, cb = {vb ? *slot_b : 0ull};
  const bool hit_a = va && ca.matches(pa), hit_b = vb && cb.matches(pb);
  int ha, hma, hb = 0x7fff, hmb = 0x7fff;
  if constexpr (COOP) {  // (distances are complete sums: no genome letter the planes answer for makes a word's share negative)
    // (is an N within reach of the window?  asked before the windows so that the answers arrive with them)
    const u32 na = va && !hit_a ? n_within_reach(ix.nmap, pa) : 0u, nb = vb && !hit_b ? n_within_reach(ix.nmap, pb) : 0u;
    if (lds.G == 2)
      hamming_planes_pairs(ix, lds, sc.qmask, sc.L, pa, va && !hit_a, pb, vb && !hit_b, ha, hb);
    else
      hamming_planes(ix, lds, sc.qmask, sc.L, pa, va && !hit_a, pb, vb && !hit_b, ha, hb);
    hma = ha; hmb = hb;
    redo_on_nibbles(ix, sc, na, pa, ha, hma, nb, pb, hb, hmb);
  }
  else
    hamming2(ix.genome, sc.qpk, sc.nwords, pa, va && !hit_a, pb, vb && !hit_b, ha, hma, hb, hmb);
  if (hit_a) ca.distances(ha, hma);
  if (va && !hit_a) *slot_a = PosCacheEntry::pack(pa, ha, hma);
  if (!va) { ha = hma = 0x7fff; }
  if (two) {
    if (hit_b) cb.distances(hb, hmb);
    if (vb && !hit_b) *slot_b = PosCacheEntry::pack(pb, hb, hmb);
    if (!vb) { hb = hmb = 0x7fff; }
  }
  return {va, vb, pa, pb, ha, hma, hb, hmb, (va ? 1u : 0u) + (vb ? 1u : 0u), (hit_a ? 1u : 0u) + (hit_b ? 1u : 0u)};
}
// 8-byte words fetched per window: on the records three or four 16-byte blocks; on the bit planes a group of four
// lanes fetches four 16-byte blocks, a group of eight the blocks its window has (at most L / 64 + 2); on the nibble
// array the read's words
template <bool COOP, bool REC> __device__ __forceinline__ u32 window_words(const WaveLds &lds, const SeedCall &sc) {
  if (REC) return lds.G == 2 ? 6u : 8u;
  return COOP ? (lds.G == 2 ? 6u : (lds.G == 4 ? 8u : 2u * ((sc.L + kPlaneBlock - 1) / kPlaneBlock + 1))) : sc.nwords;
}

// ordered replay of one 64-candidate sub-chunk (check_hits + update, :1133-1149, :394-404)
template <bool SPECIFIC, bool TALLY, class Set>
__device__ __forceinline__ void replay_chunk(Set &S, WorkTally &wt, u32 flags, bool valid, int h, int hmax, u32 pos) {
  u64 todo = __ballot(valid && hmax <= S.cutoff);
  if constexpr (Set::kAppend) if (SPECIFIC && !S.heaped && todo) {
    // growing paired-end set: every survivor goes in, the whole chunk at once (see PeSet)
    const int offered = __popcll(todo);
    todo = S.append(todo, h, pos);
    if (TALLY) wt.updates += static_cast<u32>(offered - __popcll(todo));
  }
  while (todo && !S.sure_ambig) {
    if constexpr (Set::kFifo) {
      // full set, survivors that tie with the cutoff: applied a run at a time (SeSet::tie_run)
      const int applied = S.tie_run(todo, __ballot(valid && h == S.cutoff), pos, flags);
      if (applied) {
        if (TALLY) wt.updates += static_cast<u32>(applied);
        if (TALLY) wt.fifo_updates += static_cast<u32>(applied);
        continue;
      }
    }
    const int l = __builtin_ctzll(todo);
    const int before = S.cutoff;
    S.admit(true, rdlane(h, l), flags, rdlane(pos, l));
    if (TALLY) ++wt.updates;
    todo &= ~(((1ull << l) << 1) - 1);
    if (S.cutoff < before) todo &= __ballot(valid && hmax <= S.cutoff);
  }
}

// ---- the driver --------------------------------------------------------------------------------------------------
// One (strand, alphabet) call for the whole wave: per block of 64 offsets, stage 1 (offset_buckets, a lane per
// offset), stage 2 (the checked buckets flattened: a lane per candidate from here on), stage 3 (a filter step and an
// ordered replay per 128 candidates).  The stamps and the per-step tallies are here and nowhere else.
template <bool SPECIFIC, bool TIMED, bool COOP, bool REC, class Set>
__device__ __forceinline__ void seed_pass(const DevIndex &ix, const WaveLds &lds, u32 enc, bool g_to_a,
                                          u32 flags, u32 L, Set &S, WorkTally &wt, u32 &seg_epoch, u32 &memo_n) {
  static_assert(!REC || COOP, "window records are filtered cooperatively");
  const int lane = lane_id();
  constexpr bool kMemo = kBoundsMemo<REC, Set>;
  const SeedCall sc = seed_call<SPECIFIC, kMemo>(ix, lds, enc, g_to_a, L);
  if constexpr (kMemo) {
    if (SPECIFIC) memo_n = 0;
    else wave_sync();  // (the specific pass's memo, written by other lanes' stores as far as the compiler knows)
  }
  // work tallies: the diagnostic builds keep them, the production kernels do not (they cost the single-end kernel
  // registers: 100 -> 64 bytes per lane of scratch without them; the pair kernels kept them until round 5, when five
  // lane-resident counters were what the seed kernel spilled in its offset loop)
  constexpr bool TALLY = TIMED;
  long long ta = 0, tb_ = 0, tc = 0, td = 0;
  if (SPECIFIC && !REC) {  // a new (strand, alphabet) call: the cache belongs to one encoding
    for (u32 k = lane; k < (1u << kPosCacheBits); k += 64) lds.pcache[k] = 0;
    wave_sync();
  }
  for (u32 g0 = 0; g0 < sc.n_off && !S.sure_ambig; g0 += 64) {
    ABM_STAMP(ta);
    // stage 1
    const u32 i = g0 + lane;
    OffsetBuckets b = {0, 0, 0, 0, false, false};
    if (i < sc.n_off) b = offset_buckets<SPECIFIC, TALLY, REC, Set>(ix, lds, sc, i, memo_n, wt);
    if constexpr (kMemo) if (SPECIFIC && sc.memo_fits) memo_n = min(g0 + 64u, sc.n_off);  // (this block's live lanes have written)
    // stage 2
    Segs sg;
    sg.na = b.chk2 ? b.hi2 - b.lo2 : 0u;
    sg.nb = b.chk3 ? b.hi3 - b.lo3 : 0u;
    sg.lo2 = b.lo2;
    sg.lo3 = b.lo3;
    if constexpr (TALLY && Set::kAppend) {
      // pair kernels: the 128-byte lines the checked buckets' index-entry runs span (32 entries a line) -- their share of a
      // pair's line requests (DESIGN 4.3's table); the words of the fetched windows follow from the candidate count
      if (sg.na) wt.words += ((sg.lo2 + sg.na - 1) >> 5) - (sg.lo2 >> 5) + 1;
      if (sg.nb) wt.words += ((sg.lo3 + sg.nb - 1) >> 5) - (sg.lo3 >> 5) + 1;
    }
    u32 total;
    sg.start_a = wave_excl_sum(sg.na + sg.nb, total);
    ABM_STAMP(tb_);
    if (TIMED) wt.t_probe += tb_ - ta;
    if (total == 0) continue;
    // A read with this many candidates in one block of offsets is one of the launch's costliest (a homopolymer, a
    // satellite): its wave is served first from here on (until the kernel's next read), so that it runs at the pace of
    // a wave alone on its SIMD instead of a fifth of it -- such reads are what a launch's last milliseconds wait for.
    if (total >= kHeavyBlock) __builtin_amdgcn_s_setprio(3);
    if (seg_epoch >= kSegEpochLimit) {  // (sixteen million steps on: start the mark tags over)
      lds.smark[lane] = 0; lds.smark[64 + lane] = 0;
      seg_epoch = 0;
    }
    publish_segs(lds, sg);
    // stage 3
    // Candidates are taken 128 at a time, two per lane (a: c0+lane, b: c0+64+lane): both index entries,
    // then both genome windows, are in flight together, which halves the dependent round trips of a
    // read with very many candidates.  The set still sees them strictly in the reference's order.
    // The index entries of the NEXT 128 candidates are requested before this step's windows, so a
    // step costs one dependent memory round trip instead of two (what a read with millions of
    // candidates -- one wave, no other latency hiding at the end of a launch -- is made of).
    // A step with at most 64 candidates (most steps of an ordinary read) does nothing for its b half.
    StepCursor cur = {0, false, false, 0, 0, 0, 0};
    if constexpr (!REC) fetch_entries(ix, lds, sc, seg_epoch, sg, 0, total, cur);
    for (u32 c0 = 0; c0 < total && !S.sure_ambig; c0 += 128) {
      ABM_STAMP(tc);
      if (TIMED) { ++wt.steps; if (total - c0 <= 64) ++wt.light_steps; }
      const bool two = c0 + 64 < total;  // (uniform: this step has a b half)
      FilterStep f;
      if constexpr (REC) f = filter_step_records(ix, lds, sc, S, seg_epoch, sg, g0, c0, total, two, cur);
      else f = filter_step_windows<COOP>(ix, lds, sc, seg_epoch, sg, g0, c0, total, two, cur);
      if (TALLY) {
        wt.cands += f.seen;
        if constexpr (!Set::kAppend) wt.words += f.seen * window_words<COOP, REC>(lds, sc);
        wt.cache_hits += f.cached;
      }
      ABM_STAMP(td);
      if (TIMED) wt.t_stream += td - tc;
      replay_chunk<SPECIFIC, TALLY>(S, wt, flags, f.va, f.ha, f.hma, f.pa);
      if (two && !S.sure_ambig) replay_chunk<SPECIFIC, TALLY>(S, wt, flags, f.vb, f.hb, f.hmb, f.pb);
      ABM_STAMP(tc);
      if (TIMED) wt.t_replay += tc - td;
    }
  }
}

// (the pair kernels, whose sets append: no memo)
template <bool SPECIFIC, bool TIMED, bool COOP, bool REC, class Set>
__device__ __forceinline__ void seed_pass(const DevIndex &ix, const WaveLds &lds, u32 enc, bool g_to_a,
                                          u32 flags, u32 L, Set &S, WorkTally &wt, u32 &seg_epoch) {
  u32 memo_n = 0;
  seed_pass<SPECIFIC, TIMED, COOP, REC>(ix, lds, enc, g_to_a, flags, L, S, wt, seg_epoch, memo_n);
}

}  // namespace abm
