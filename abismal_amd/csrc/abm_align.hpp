// abismal_amd device code: banded alignment of the candidates a seed pass leaves, CIGARs, and the choice of a
// single-end read's hit (gfx950, one wavefront per read / pair).
#pragma once
#include "abm_se_set.hpp"
#include "abm_seed.hpp"

namespace abm {

// =============================================================================
// Banded local alignment (AbismalAlign::align, src/AbismalAlign.hpp:320-386) as
// an anti-diagonal wavefront.  Cell (i,j) of the reference's band table (row i =
// target base t_beg+i-1, column j, read index q = i+j-bw) depends on (i-1,j)
// [substitution], (i-1,j+1) [from_above] and (i,j-1) [from_left]; on the
// anti-diagonal t = 2i+j all three are already known, from the same lane two
// steps ago and from the two neighbouring lanes one step ago.  So lane = band
// column, one DPP move per neighbour per step, and no in-row scan.  A band is
// at most 61 lanes wide and usually ~21 (2*min(diffs,max_diffs)+1), so several
// candidate alignments ("jobs") share one wave side by side.
// Cell validity (left/right of the reference's row loop) reduces to 0 <= q < L;
// invalid cells read as 0, exactly like the zero-filled table.
// =============================================================================
__device__ __forceinline__ int band_for(int diffs, int max_diffs) {
  const int v = 2 * min(diffs, max_diffs) + 1;
  return v < 0 ? static_cast<int>(kMaxBand) : min(static_cast<int>(kMaxBand), v);
}
// 16 nibbles starting at nibble index `start` of an LDS word array; nibbles
// outside [0, 16*nwords) read as 0 (they only ever feed invalid cells)
__device__ __forceinline__ u64 nibbles16(const u64 *words, int nwords, int start) {
  if (start <= -16 || start >= 16 * nwords)
    return 0ull;
  if (start < 0)
    return words[0] << ((-start) << 2);
  const int w = start >> 4, s = (start & 15) << 2;
  u64 x = words[w] >> s;
  if (s && w + 1 < nwords) x |= words[w + 1] << (64 - s);
  return x;
}

struct AlnJob {  // per lane: the job whose band column this lane is
  int bw;        // 0 = lane unassigned
  int jl;        // column within the band
  int qoff;      // word offset of the query encoding in lds.qpk
  int g;         // genome-window slot in lds.gwin
  int t0nib;     // t_beg & 15: nibble offset of row 1's target base inside the window
};

// Runs every job assigned in `job` to completion.  Returns, per lane, the best
// cell value of its own column (and its first row); with TB also stores one
// byte per cell: arrow (0 M, 1 I, 2 D, 3 none) | 4 if the cell's score is > 0.
// WRAP: every candidate score is narrowed to 16 bits before it competes, as the reference's score_t arithmetic does
// (src/AbismalAlign.hpp:35, :239-262: `const score_t score = ... + *cur_row`); it only ever matters for reads beyond
// 16383 bases, whose perfect score 2 L no longer fits -- the long-read kernel's instantiations.
template <bool WRAP> __device__ __forceinline__ int score16(int v) { return WRAP ? static_cast<int>(static_cast<i16>(v)) : v; }

template <bool TB, bool WRAP = false>
__device__ __forceinline__ void wavefront(const WaveLds &lds, const AlnJob &job, int L, int bw_min,
                                          int bw_max, int &bestv, int &bestrow) {
  const int jl = job.jl, bw = job.bw;
  const bool assigned = bw != 0;
  const u64 *qw = lds.qpk + job.qoff;
  const u64 *gw = lds.gwin + job.g * lds.GW;
  const int t_start = max(0, bw_min - 1), t_end = 2 * (L - 1 + bw_max);
  int cur = 0;
  u64 M = 0;
  bestv = 0; bestrow = 0;
  for (int t = t_start; t <= t_end; ++t) {
    if (((t - t_start) & 31) == 0) {
      // match bits for this lane's next 16 cells: nibble k set <=> q[i0+k+jl-bw] & T[i0+k-1] != 0
      const int ta = t + ((t - jl) & 1);
      const int i0 = (ta - jl) >> 1;
      u64 x = 0;
      if (assigned)
        x = nibbles16(qw, static_cast<int>(lds.W), i0 + jl - bw) &
            nibbles16(gw, static_cast<int>(lds.GW), job.t0nib + i0 - 1);
      x |= x >> 1;
      x |= x >> 2;
      M = x & 0x1111111111111111ull;
    }
    const int dlt = t - jl;
    const bool active = assigned && (dlt & 1) == 0;
    const int i = dlt >> 1;
    const int q = i + jl - bw;
    const bool valid = active && q >= 0 && q < L;
    const int lf = from_prev_lane(cur), up = from_next_lane(cur);
    const int sdiag = score16<WRAP>(cur + ((static_cast<u32>(M) & 1u) ? 2 : -3));
    int c = max(sdiag, 0);
    int arrow = (c == sdiag) ? 0 : 3;
    if (jl < bw - 1 && q < L - 1) {   // from_above: j in [left, right-1)
      const int s = score16<WRAP>(up - 4);
      c = max(c, s);
      if (TB && c == s) arrow = 2;
    }
    if (jl > 0 && q > 0) {            // from_left: j in [left+1, right)
      const int s = score16<WRAP>(lf - 4);
      c = max(c, s);
      if (TB && c == s) arrow = 1;
    }
    if (active) {
      M >>= 4;
      cur = valid ? c : 0;
      if (valid && c > bestv) { bestv = c; bestrow = i; }
      if (TB && i >= 0 && i < L + bw)
        lds.tb[i * bw + jl] = static_cast<u8>(valid ? (arrow | (c > 0 ? 4 : 0)) : 3);
    }
  }
}

// The traceback run row by row: ONE job on lanes [0, bw), every lane computes its cell of row i in the same step
// (the anti-diagonal schedule keeps a lone job's lanes idle every other step).  The one dependency inside a row --
// from_left, c(i,j) = max(base(i,j), c(i,j-1) - 4) -- unrolls to c(i,j) = max over k <= j of base(i,k) - 4 (j - k), an
// inclusive running maximum of base + 4 k over the band's lanes: ceil(log2 bw) DPP steps (two for the band of three
// a read with one mismatch gets).  Cells left of the read (q < 0) compute to 0 like the reference's zero-filled
// table, cells right of it (q >= L) cannot reach a valid cell through from_left and are masked when published.
// Arrows as the reference decides them: left wins ties, then above, then the diagonal.  Same table, scores, first
// maximum per column as wavefront<TB>; 32-bit scores (the long-read kernel keeps wavefront<TB, true>).  (Same table
// wherever wavefront<TB> writes one: cells outside the read that no step of its schedule falls on -- 2 i + j below
// bw - 1 or above 2 (L - 1 + bw) -- it leaves as they were, and no walk reads them; this run writes 3 there.)
#ifndef ABM_TB_ROWS
#define ABM_TB_ROWS true  // (false: the traceback run on the anti-diagonal schedule, for same-box comparisons)
#endif
constexpr bool kTracebackByRows = ABM_TB_ROWS;
template <bool TB>
__device__ __forceinline__ void wavefront_rows(const WaveLds &lds, const AlnJob &job, int L, int bw, int &bestv,
                                               int &bestrow) {
  const int jl = job.jl;
  const bool assigned = job.bw != 0;
  const u64 *qw = lds.qpk + job.qoff;
  const u64 *gw = lds.gwin + job.g * lds.GW;
  const int off4 = 4 * jl;
  const bool up_lane = assigned && jl < bw - 1;
  const int rows = L + bw;
  int cur = 0;
  u64 M = 0;
  bestv = 0; bestrow = 0;
  for (int i = 0; i < rows; ++i) {
    if ((i & 15) == 0) {  // match bits of this lane's next 16 rows
      u64 x = 0;
      if (assigned)
        x = nibbles16(qw, static_cast<int>(lds.W), i + jl - bw) & nibbles16(gw, static_cast<int>(lds.GW), job.t0nib + i - 1);
      x |= x >> 1;
      x |= x >> 2;
      M = x & 0x1111111111111111ull;
    }
    const int q = i + jl - bw;
    const bool valid = assigned && q >= 0 && q < L;
    const int up = from_next_lane(cur) - 4;
    const int sdiag = cur + ((static_cast<u32>(M) & 1u) ? 2 : -3);
    M >>= 4;
    int base = max(sdiag, 0);
    int arrow = (base == sdiag) ? 0 : 3;
    if (up_lane && q < L - 1) {  // from_above
      base = max(base, up);
      if (TB && base == up) arrow = 2;
    }
    u32 x = static_cast<u32>(base + off4);  // (>= 0: the scans' identity 0 never wins)
    if (bw > 1) x = max(x, dpp_from<0x111, 0xf>(0u, x));
    if (bw > 2) x = max(x, dpp_from<0x112, 0xf>(0u, x));
    if (bw > 4) x = max(x, dpp_from<0x114, 0xf>(0u, x));
    if (bw > 8) x = max(x, dpp_from<0x118, 0xf>(0u, x));
    if (bw > 16) x = max(x, dpp_from<0x142, 0xa>(0u, x));
    if (bw > 32) x = max(x, dpp_from<0x143, 0xc>(0u, x));
    const int c = static_cast<int>(x) - off4;
    if (TB && c == from_prev_lane(c) - 4) arrow = 1;  // from_left (an invalid or missing neighbour offers -4)
    cur = valid ? c : 0;
    if (valid && c > bestv) { bestv = c; bestrow = i; }
    if (TB && assigned) lds.tb[i * bw + jl] = static_cast<u8>(valid ? (arrow | (c > 0 ? 4 : 0)) : 3);
  }
}

// where CIGARs go: fixed slots of `stride` ops per read; one with more ops goes whole into the launch's
// overflow arena (bump-allocated), its slot's first word = where, and its count (> stride) says so.  Without room
// there the launch is flagged and the slot holds the CIGAR's first `stride` ops (of the ops the walk could keep).
struct CigarSink {
  u32 stride;
  u32 ctmp_cap;        // entries of the reversed-ops scratch in LDS (longest read + 2: no CIGAR has more ops)
  u32 *arena;          // [arena_cap] or null
  u32 *arena_count;    // ops handed out so far
  u32 arena_cap;
  u32 *fin;            // optional: the CIGAR's first kSeCap ops in LDS as well (the single-end kernel's SAM text is made from them)
};

// build_cigar_len_and_pos + get_traceback (src/AbismalAlign.hpp:166-193, :388-440) in two steps, both uniform on the
// wave: the walk through the traceback table, which leaves the ops reversed in LDS (ctmp) and touches nothing else,
// and the emission of what the walk found.  Between the two the table may be overwritten (choose_se_pilot does).
struct CigarWalk {
  u32 n;                 // ops found (those beyond the scratch's capacity are counted, not kept)
  int clip_head, clip_tail;
  int r;                 // the table row the walk ended in
};
__device__ __forceinline__ CigarWalk cigar_walk(const u8 *tb, u32 *ctmp, u32 ctmp_cap, int L, int bw, int best_r, int best_c,
                                                int &ins, int &del) {
  const int lane = lane_id();
  ins = del = 0;  // count_total_ops<I>/<D> with oplen() narrowed to uint8_t (abismal_cigar_utils.hpp:50-53)
  int r = best_r, c = best_c;
  const int clip_tail = (L + (bw - 1)) - (r + c);
  u32 n = 0;
  auto emit = [&](u32 run, int op) {
    if (n < ctmp_cap) { if (lane == 0) ctmp[n] = (run << 4) | static_cast<u32>(op); }
    const int r8 = static_cast<int>(static_cast<u8>(run));
    ins = op == 1 ? static_cast<i16>(ins + r8) : ins;  // (value selects: conditional stores through the two references go to scratch)
    del = op == 2 ? static_cast<i16>(del + r8) : del;
    ++n;
  };
  auto step = [&](int a) {
    if (a != 1) --r;
    if (a == 1) --c;
    if (a == 2) ++c;
  };
  int op = uni(tb[r * bw + c]) & 3;
  step(op);
  u32 run = 1;
  for (;;) {
    const int cell = uni(tb[r * bw + c]);
    if (!(cell & 4)) break;
    const int a = cell & 3;
    step(a);
    if (a != op) { emit(run, op); run = 0; }
    ++run;
    op = a;
  }
  emit(run, op);
  const int clip_head = (r + c) - (bw - 1);
  wave_sync();
  return {n, clip_head, clip_tail, r};
}
__device__ __forceinline__ void cigar_publish(const u32 *ctmp, const CigarWalk &w, int L, int bw, u32 *cig_out,
                                              const CigarSink &sink, u32 &n_ops, u32 &aln_len, u32 &t_pos, bool &overflow) {
  const int lane = lane_id();
  const u32 n = w.n;
  const int clip_head = w.clip_head, clip_tail = w.clip_tail;
  // final order: [head clip] reversed(ops) [tail clip]
  const u32 full = n + (clip_head > 0) + (clip_tail > 0);  // the CIGAR's op count
  u32 *dst = cig_out;
  u32 body = n, total = full, kept = n;  // kept: the ops the walk left in ctmp (ctmp[kept - 1] is the CIGAR's first)
  if (full > sink.stride) {  // too long for the slot: the whole CIGAR goes to the arena
    u32 at = 0xFFFFFFFFu;
    if (sink.arena != nullptr && n <= sink.ctmp_cap) {
      if (lane == 0) at = atomicAdd(sink.arena_count, full);
      at = static_cast<u32>(uni(static_cast<int>(at)));
      if (at > sink.arena_cap || full > sink.arena_cap - at) at = 0xFFFFFFFFu;
    }
    if (at != 0xFFFFFFFFu) {
      dst = sink.arena + at;
      if (lane == 0) store_out(cig_out, at);
    }
    else {  // no room: the slot gets what fits -- the CIGAR's leading ops -- and the launch is flagged
      overflow = true;
      kept = min(n, sink.ctmp_cap);
      body = min(kept, sink.stride);
      total = min(body + (clip_head > 0) + (clip_tail > 0), sink.stride);
    }
  }
  for (u32 k = lane; k < total; k += 64) {
    u32 v;
    const u32 kk = k - (clip_head > 0 ? 1u : 0u);
    if (clip_head > 0 && k == 0) v = (static_cast<u32>(clip_head) << 4) | 4u;
    else if (kk < body) v = ctmp[kept - 1 - kk];
    else v = (static_cast<u32>(clip_tail) << 4) | 4u;
    store_out(dst + k, v);
    if (sink.fin && k < kSeCap) sink.fin[k] = v;
  }
  n_ops = full;  // > stride: the ops are in the arena at slot[0] (or, with ABM_STATUS_CIGAR_OVERFLOW set, nowhere complete)
  aln_len = static_cast<u32>(L - clip_tail - clip_head);
  t_pos = t_pos - static_cast<u32>((bw - 1) / 2) + static_cast<u32>(w.r);
}
__device__ __forceinline__ void wave_cigar(const u8 *tb, u32 *ctmp, int L, int diffs, int max_diffs,
                                           int score, int best_r, int best_c, u32 *cig_out,
                                           const CigarSink &sink, u32 &n_ops, int &ins, int &del, u32 &aln_len,
                                           u32 &t_pos, bool &overflow) {
  if (score == 0 || diffs == 0) {
    ins = del = 0;
    if (lane_id() == 0) { store_out(cig_out, static_cast<u32>(L) << 4); if (sink.fin) sink.fin[0] = static_cast<u32>(L) << 4; }
    n_ops = 1;
    aln_len = static_cast<u32>(L);
    return;
  }
  const int bw = band_for(diffs, max_diffs);
  const CigarWalk w = cigar_walk(tb, ctmp, sink.ctmp_cap, L, bw, best_r, best_c, ins, del);
  cigar_publish(ctmp, w, L, bw, cig_out, sink, n_ops, aln_len, t_pos, overflow);
}

// simple_aln::edit_distance with the reference's integer types
// (src/AbismalAlign.hpp:73-89); ins/del are the op totals gathered in wave_cigar
__device__ __forceinline__ int edit_distance(int scr, u32 len, int ins, int del) {
  if (scr == 0)
    return static_cast<i16>(len);
  const int A = static_cast<i16>(scr + 4 * (ins + del));
  const u32 num = 2u * (len - static_cast<u32>(ins)) - static_cast<u32>(A);
  const int mism = static_cast<i16>(num / 5u);
  return static_cast<i16>(mism + ins + del);
}

__device__ __forceinline__ bool long_enough(u32 aln_len, u32 readlen, u32 kMinReadLen) {
  const double min_frac = 1.0 - 0.4;  // src/abismal.cpp:307-314
  return aln_len >= max(kMinReadLen, static_cast<u32>(min_frac * readlen));
}

// encoding index of the query a hit was found with (src/abismal.cpp:1463-1464)
__device__ __forceinline__ u32 enc_of(u32 flags) {
  const u32 rc = (flags & kFlagRC) ? 1u : 0u, ar = (flags & kFlagARich) ? 1u : 0u;
  return rc * 2u + (rc ^ ar);
}

// Stage the genome windows of jobs [first, first+n) of the LDS job list into
// lds.gwin (one coalesced sweep, loads issued before the stores)
__device__ __forceinline__ void stage_windows(const DevIndex &ix, const WaveLds &lds, int first, int n,
                                              int md) {
  const int lane = lane_id();
  const int GW = static_cast<int>(lds.GW), total = n * GW;
  for (int k0 = 0; k0 < total; k0 += 256) {
    u64 v[4];
    int at[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = k0 + lane + 64 * r;
      at[r] = -1;
      v[r] = 0;
      if (k < total) {
        const int g = k / GW, w = k - g * GW;
        const u32 pos = lds.jpos[first + g];
        const int bw = band_for(static_cast<int>(lds.jdf[first + g]) >> 16, md);
        const u64 t_beg = static_cast<u64>(pos) - static_cast<u64>((bw - 1) / 2);
        v[r] = ix.genome[(t_beg >> 4) + w];
        at[r] = k;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (at[r] >= 0) lds.gwin[at[r]] = v[r];
  }
}

// ---- scoring runs (align<false>): two job sets per wave ---------------------------
// On the anti-diagonal schedule a lane computes a cell only every other step.  A second
// set of jobs, laid out over the same lanes and started one step later, fills the idle
// steps: whatever a lane's neighbours published in the previous step then always belongs
// to the set the lane is working on now, so both sets share the two DPP moves and no
// select is needed -- each lane just alternates between its two jobs (`jp` on even steps
// counted from t_start, `jq` on odd ones; dp/dq = 1 if that job belongs to the delayed set).
template <bool WRAP = false>
__device__ __forceinline__ void wavefront_pair(const WaveLds &lds, const AlnJob &jp, const AlnJob &jq, int dp,
                                               int dq, int L, int bw_min, int bw_max, int &bestp, int &bestq) {
  const int t_start = max(0, bw_min - 1), t_end = 2 * (L - 1 + bw_max) + 1;
  const u64 *qp = lds.qpk + jp.qoff, *gp = lds.gwin + jp.g * lds.GW;
  const u64 *qq = lds.qpk + jq.qoff, *gq = lds.gwin + jq.g * lds.GW;
  int curp = 0, curq = 0, pub = 0;
  u64 Mp = 0, Mq = 0;
  bestp = bestq = 0;
  auto refill = [&](const AlnJob &j, const u64 *qw, const u64 *gw, int time) -> u64 {
    const int i0 = (time - j.jl) >> 1;
    u64 x = 0;
    if (j.bw)
      x = nibbles16(qw, static_cast<int>(lds.W), i0 + j.jl - j.bw) &
          nibbles16(gw, static_cast<int>(lds.GW), j.t0nib + i0 - 1);
    x |= x >> 1;
    x |= x >> 2;
    return x & 0x1111111111111111ull;
  };
  auto cell = [&](const AlnJob &j, int time, int &cur, u64 &M, int &best) {
    const int i = (time - j.jl) >> 1;
    const int q = i + j.jl - j.bw;
    const bool valid = j.bw != 0 && q >= 0 && q < L;
    const int lf = from_prev_lane(pub), up = from_next_lane(pub);
    int c = max(score16<WRAP>(cur + ((static_cast<u32>(M) & 1u) ? 2 : -3)), 0);
    if (j.jl < j.bw - 1 && q < L - 1) c = max(c, score16<WRAP>(up - 4));  // from_above
    if (j.jl > 0 && q > 0) c = max(c, score16<WRAP>(lf - 4));             // from_left
    M >>= 4;
    cur = valid ? c : 0;
    best = max(best, cur);
    pub = cur;
  };
  for (int t = t_start; t <= t_end; t += 2) {
    if (((t - t_start) & 31) == 0) {
      Mp = refill(jp, qp, gp, t - dp);
      Mq = refill(jq, qq, gq, t + 1 - dq);
    }
    cell(jp, t - dp, curp, Mp, bestp);
    cell(jq, t + 1 - dq, curq, Mq, bestq);
  }
}

__device__ __forceinline__ int wave_max_i32(int x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x = max(x, __shfl_xor(x, d));
  return x;
}

// Scores jobs [first, ...) of the LDS job list (jpos / jdf = diffs<<16 | flags), as many as fit
// one wave: consecutive jobs share a slot of lanes (one in each set), slots sit side by side.
// Returns one past the last job taken; the score of job first+k is left in lds.lbest[k].
template <bool WRAP = false>
__device__ __forceinline__ int score_round(const DevIndex &ix, const WaveLds &lds, int first, int n_jobs,
                                           int L, int md, int qbase) {
  const int lane = lane_id();
  AlnJob ja = {0, 0, 0, 0, 0}, jb = {0, 0, 0, 0, 0};
  int used = 0, s = first, bw_min = 64, bw_max = 0, my_o = 0;
  while (s < n_jobs && s - first + 2 <= static_cast<int>(lds.max_jobs)) {
    const bool two = s + 1 < n_jobs;
    const u32 dfa = lds.jdf[s], dfb = two ? lds.jdf[s + 1] : 0u;
    const int bwa = band_for(static_cast<int>(dfa) >> 16, md);
    const int bwb = two ? band_for(static_cast<int>(dfb) >> 16, md) : 0;
    const int width = max(bwa, bwb);
    if (used + width > 64) break;
    const int o = lane - used;
    if (o >= 0 && o < width) my_o = o;
    if (o >= 0 && o < bwa) {
      const u64 t_beg = static_cast<u64>(lds.jpos[s]) - static_cast<u64>((bwa - 1) / 2);
      ja.bw = bwa; ja.qoff = qbase + static_cast<int>(enc_of(dfa & 0xFFFFu) * lds.W);
      ja.g = s - first; ja.t0nib = static_cast<int>(t_beg & 15u);
    }
    if (o >= 0 && o < bwb) {
      const u64 t_beg = static_cast<u64>(lds.jpos[s + 1]) - static_cast<u64>((bwb - 1) / 2);
      jb.bw = bwb; jb.qoff = qbase + static_cast<int>(enc_of(dfb & 0xFFFFu) * lds.W);
      jb.g = s + 1 - first; jb.t0nib = static_cast<int>(t_beg & 15u);
    }
    used += width;
    bw_min = min(bw_min, two ? min(bwa, bwb) : bwa);
    bw_max = max(bw_max, width);
    s += two ? 2 : 1;
  }
  stage_windows(ix, lds, first, s - first, md);
  wave_sync();
  const int t_start = max(0, bw_min - 1);
  const bool even = ((t_start - my_o) & 1) == 0;  // which of the lane's jobs is due on even steps
  ja.jl = jb.jl = my_o;
  int bp, bq;
  wavefront_pair<WRAP>(lds, even ? ja : jb, even ? jb : ja, even ? 0 : 1, even ? 1 : 0, L, bw_min, bw_max, bp, bq);
  lds.lbest[lane] = (even ? bp : bq) | ((even ? bq : bp) << 16);
  wave_sync();
  int base = 0, mine = 0;
  for (int k = first; k < s;) {
    const bool two = k + 1 < s;
    const int bwa = band_for(static_cast<int>(lds.jdf[k]) >> 16, md);
    const int bwb = two ? band_for(static_cast<int>(lds.jdf[k + 1]) >> 16, md) : 0;
    const int v = lane < max(bwa, bwb) ? lds.lbest[base + lane] : 0;
    const int sa = wave_max_i32(lane < bwa ? (v & 0xFFFF) : 0);
    if (lane == k - first) mine = sa;
    if (two) {
      const int sb = wave_max_i32(lane < bwb ? (v >> 16) : 0);
      if (lane == k + 1 - first) mine = sb;
    }
    base += max(bwa, bwb);
    k += two ? 2 : 1;
  }
  wave_sync();
  lds.lbest[lane] = mine;
  wave_sync();
  return s;
}

// ---- scoring runs, four jobs per slot of lanes ----------------------------------------
// Scores fit 16 bits (2 L <= 2048 in these kernels), so a lane can carry TWO jobs of a set in the halves of one
// register and advance both with one packed instruction (v_pk_add_i16 / v_pk_max_i16): with the two sets of the
// anti-diagonal schedule that is four jobs per slot.  For the halves to share the lane's control flow the slot is laid
// out around the band's centre: lane offset o, c = o - K (K = the slot's half width, its widest job's), and a job of
// half width k <= K owns the lanes |c| <= k.  In these coordinates the read index q = i + o - width and the row's
// target base pos + i - K - 1 are the same for every job of the slot (the reference's column is j = c + k, its row
// i_ref = i - (K - k): q_ref = i_ref + j - bw = q, target = t_beg + i_ref - 1), so validity by q, the row clock and the DPP
// moves are shared, and what differs per job is loop-invariant: the band mask (halves 0xFFFF inside the job's band), the
// edge masks of from_above (c < k) and from_left (c > -k), and the offset of its staged window (row 1's target base
// sits K - k nibbles earlier).  A masked-off candidate is 0, which never beats a cell value (>= 0).
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32 pk_add(u32 a, u32 b) { return __builtin_bit_cast(u32, __builtin_bit_cast(s16x2, a) + __builtin_bit_cast(s16x2, b)); }
__device__ __forceinline__ u32 pk_max(u32 a, u32 b) {
  return __builtin_bit_cast(u32, __builtin_elementwise_max(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}
// maximum of both halves over the wave (values >= 0), uniform
__device__ __forceinline__ u32 wave_max_pk(u32 x) {
  x = pk_max(x, dpp_from<0x111, 0xf>(0u, x));
  x = pk_max(x, dpp_from<0x112, 0xf>(0u, x));
  x = pk_max(x, dpp_from<0x114, 0xf>(0u, x));
  x = pk_max(x, dpp_from<0x118, 0xf>(0u, x));
  x = pk_max(x, dpp_from<0x142, 0xa>(0u, x));
  x = pk_max(x, dpp_from<0x143, 0xc>(0u, x));
  return rdlane(x, 63);
}

struct QuadJob {         // per lane: the two jobs of one set that share this lane's slot (low half, high half)
  u32 mv, ma, ml;        // halves 0xFFFF: lane inside the job's band / may take from_above / may take from_left
  int qoff_lo, qoff_hi;  // word offsets of the query encodings in lds.qpk
  int g_lo, g_hi;        // genome-window slots in lds.gwin
  int gs_lo, gs_hi;      // nibble index of row 1's target base in the window, moved to the slot's band
};

// The loop (round 5).  At iteration n (anti-diagonal steps t_start + 2 n and + 2 n + 1) set P's cell has read index
// q = n + q0p and set Q's q = n + q0q, with per-lane constants q0: ((a + 2 n) >> 1 = (a >> 1) + n).  A cell needs its
// position only for three tests -- from_above exists if q < L - 1, from_left if q > 0, the cell itself if 0 <= q < L --
// and for all lanes at once they can only fail in the first and last few iterations (the lanes' q differ by at most a
// band's width).  So the iterations are cut in three: a head and a tail that make the tests, and a middle -- 1 <= q <=
// L - 2 in every lane, five sixths of the iterations of a 150-base read -- that does not: 15 vector instructions per
// packed cell against 28.  The match bits of a lane's next 16 cells sit one per cell in the halves of a 32-bit word
// (bit r: low job, bit 16 + r: high job), so "this cell's +2 / -3" is an AND and a packed multiply-add.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int wave_min_i32(int x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x = min(x, __shfl_xor(x, d));
  return x;
}
//
// FLOOR (choose_se_pilot): the caller already holds a score `floor` that some job of the read has reached, and a job
// that ends below it changes nothing.  Where the match bits are refilled -- every 16 iterations -- each lane bounds
// what its cells can still lead to: best so far, or the cell's value plus kScoreMatch for each read base the cell has
// not consumed (a step that consumes a read base gains at most kScoreMatch, a deletion consumes none and gains
// kScoreIndel <= 0, and a fresh start later in the lane is a start from 0 <= the cell with fewer bases left).  Every
// later cell of a job descends from the cells its lanes hold now, so once no lane of the wave can still reach `floor`
// the round ends: each job reports its best so far, which is below `floor`.  A job that would end at `floor` or
// above always objects, so it runs to its last row and reports its exact score; floor <= 0: no lane is ever below it.
// `iters`: iterations run (the full run's count is n_total: quad_iterations).
constexpr int kScoreMatch = 2, kScoreMismatch = -3, kScoreIndel = -4;  // simple_aln's scores (src/AbismalAlign.hpp:51-53)
static_assert(kScoreMatch > 0 && kScoreMismatch <= kScoreMatch && kScoreIndel <= 0,
              "the floor's bound: no step gains more than kScoreMatch per read base, and none that consumes no read base gains");
template <bool FLOOR = false>
__device__ __forceinline__ void wavefront_quad(const WaveLds &lds, const QuadJob &jp, const QuadJob &jq, int dp, int dq,
                                               int o, int width, int L, int w_min, int w_max, u32 &bestp, u32 &bestq,
                                               int floor = 0, int *iters = nullptr) {
  const int t_start = max(0, w_min - 1), t_end = 2 * (L - 1 + w_max) + 1;
  const int n_total = (t_end - t_start) / 2 + 1;
  const int W = static_cast<int>(lds.W), GW = static_cast<int>(lds.GW);
  const int q0p = ((t_start - dp - o) >> 1) + o - width, q0q = ((t_start + 1 - dq - o) >> 1) + o - width;
  // iterations [n_mid0, n_mid1): 1 <= q <= L - 2 for both cells of every lane that belongs to a slot (uniform)
  const bool in_slot = width != 0;
  const int q_lo = wave_min_i32(in_slot ? min(q0p, q0q) : 0x3fffffff), q_hi = wave_max_i32(in_slot ? max(q0p, q0q) : -0x3fffffff);
  const int n_mid0 = min(max(1 - q_lo, 0), n_total), n_mid1 = min(max(L - 1 - q_hi, n_mid0), n_total);
  u32 curp = 0, curq = 0, pub = 0, Mp = 0, Mq = 0;
  bestp = bestq = 0;
  auto refill = [&](const QuadJob &j, int q) -> u32 {  // match bits of the 16 cells from read index q on
    const int i0 = q - o + width;
    u64 lo = 0, hi = 0;
    if (j.mv & 0xFFFFu) lo = nibbles16(lds.qpk + j.qoff_lo, W, q) & nibbles16(lds.gwin + j.g_lo * GW, GW, j.gs_lo + i0 - 1);
    if (j.mv >> 16) hi = nibbles16(lds.qpk + j.qoff_hi, W, q) & nibbles16(lds.gwin + j.g_hi * GW, GW, j.gs_hi + i0 - 1);
    lo |= lo >> 1; lo |= lo >> 2;
    hi |= hi >> 1; hi |= hi >> 2;
    return every_fourth_bit(lo) | (every_fourth_bit(hi) << 16);
  };
  // +2 on a match, -3 otherwise, in both halves: 5 * bit - 3
  constexpr unsigned short kStep = kScoreMatch - kScoreMismatch, kMiss = static_cast<unsigned short>(kScoreMismatch);
  constexpr u32 kGap = static_cast<u32>(static_cast<unsigned short>(kScoreIndel)) * 0x00010001u;
  static_assert(kStep == 5 && kMiss == 0xFFFD && kGap == 0xFFFCFFFCu, "the packed cell's constants");
  auto step_delta = [&](u32 &M) -> u32 {
    const u16x2 bits = __builtin_bit_cast(u16x2, M & 0x00010001u);
    M >>= 1;
    const u16x2 five = {kStep, kStep}, minus3 = {kMiss, kMiss};
    return __builtin_bit_cast(u32, static_cast<u16x2>(bits * five + minus3));
  };
  // FLOOR: can a cell this lane holds (value cur, last read index q_done) or has held still lead to `floor`?
  auto alive = [&](const QuadJob &j, u32 cur, u32 best, int q_done) -> bool {
    const int left = min(max(L - 1 - q_done, 0), L);  // read bases the cell has not consumed
    const u32 ub = pk_max(best, pk_add(cur, static_cast<u32>(kScoreMatch * left) * 0x00010001u));
    return ((j.mv & 0xFFFFu) && static_cast<int>(ub & 0xFFFFu) >= floor) || ((j.mv >> 16) && static_cast<int>(ub >> 16) >= floor);
  };
  auto fast = [&](const QuadJob &j, u32 &cur, u32 &M, u32 &best) {
    const u32 lf = static_cast<u32>(from_prev_lane(static_cast<int>(pub))), up = static_cast<u32>(from_next_lane(static_cast<int>(pub)));
    u32 c = pk_max(pk_add(cur, step_delta(M)), 0u);
    c = pk_max(c, pk_add(up, kGap) & j.ma);  // from_above
    c = pk_max(c, pk_add(lf, kGap) & j.ml);  // from_left
    cur = c & j.mv;
    best = pk_max(best, cur);
    pub = cur;
  };
  auto slow = [&](const QuadJob &j, int q, u32 &cur, u32 &M, u32 &best) {
    const u32 lf = static_cast<u32>(from_prev_lane(static_cast<int>(pub))), up = static_cast<u32>(from_next_lane(static_cast<int>(pub)));
    u32 c = pk_max(pk_add(cur, step_delta(M)), 0u);
    c = pk_max(c, pk_add(up, kGap) & (q < L - 1 ? j.ma : 0u));  // from_above
    c = pk_max(c, pk_add(lf, kGap) & (q > 0 ? j.ml : 0u));      // from_left
    cur = static_cast<u32>(q) < static_cast<u32>(L) ? (c & j.mv) : 0u;
    best = pk_max(best, cur);
    pub = cur;
  };
  int n = 0;
#pragma clang loop unroll(disable)
  for (int seg = 0; seg < 3; ++seg) {
    const int end = seg == 0 ? n_mid0 : (seg == 1 ? n_mid1 : n_total);
    while (n < end) {
      if ((n & 15) == 0) {
        if constexpr (FLOOR) {
          if (n != 0 && !__any(alive(jp, curp, bestp, n - 1 + q0p) || alive(jq, curq, bestq, n - 1 + q0q))) { *iters = n; return; }
        }
        Mp = refill(jp, n + q0p); Mq = refill(jq, n + q0q);
      }
      const int stop = min(end, (n | 15) + 1);
      if (seg == 1) {
        for (; n < stop; ++n) { fast(jp, curp, Mp, bestp); fast(jq, curq, Mq, bestq); }
      }
      else {
        for (; n < stop; ++n) { slow(jp, n + q0p, curp, Mp, bestp); slow(jq, n + q0q, curq, Mq, bestq); }
      }
    }
  }
  if constexpr (FLOOR) *iters = n_total;
}
// iterations of a round that runs to its end (bands of w_min .. w_max lanes)
__device__ __forceinline__ int quad_iterations(int L, int w_min, int w_max) {
  return (2 * (L - 1 + w_max) + 1 - max(0, w_min - 1)) / 2 + 1;
}

// score_round with four jobs per slot: job first+4m+h of slot m is set (h & 1), half (h >> 1)
// FLOOR: see wavefront_quad; iters[0] += iterations run, iters[1] += iterations of the full run
template <bool FLOOR = false>
__device__ __forceinline__ int score_round_quad(const DevIndex &ix, const WaveLds &lds, int first, int n_jobs, int L, int md,
                                                int qbase, int floor = 0, u32 *iters = nullptr) {
  const int lane = lane_id();
  QuadJob ja = {0, 0, 0, 0, 0, 0, 0, 0, 0}, jb = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int used = 0, s = first, w_min = 64, w_max = 0, my_o = 0, my_w = 0;
  while (s < n_jobs) {
    const int cnt = min(4, n_jobs - s);
    if (s - first + cnt > static_cast<int>(lds.max_jobs)) break;
    int bwh[4], width = 0;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      bwh[h] = h < cnt ? band_for(static_cast<int>(lds.jdf[s + h]) >> 16, md) : 0;
      width = max(width, bwh[h]);
    }
    if (used + width > 64) break;
    const int o = lane - used, K = (width - 1) / 2, c = o - K;
    const bool in = o >= 0 && o < width;
    if (in) { my_o = o; my_w = width; }
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      if (h >= cnt) break;
      const int k = (bwh[h] - 1) / 2;
      if (in && c >= -k && c <= k) {
        const u32 df = lds.jdf[s + h];
        const u64 t_beg = static_cast<u64>(lds.jpos[s + h]) - static_cast<u64>(k);
        const u32 half = (h >> 1) ? 0xFFFF0000u : 0x0000FFFFu;
        QuadJob &j = (h & 1) ? jb : ja;
        j.mv |= half;
        if (c < k) j.ma |= half;
        if (c > -k) j.ml |= half;
        const int qoff = qbase + static_cast<int>(enc_of(df & 0xFFFFu) * lds.W);
        const int gs = static_cast<int>(t_beg & 15u) - (K - k);
        if (h >> 1) { j.qoff_hi = qoff; j.g_hi = s + h - first; j.gs_hi = gs; }
        else { j.qoff_lo = qoff; j.g_lo = s + h - first; j.gs_lo = gs; }
      }
    }
    used += width;
    w_min = min(w_min, width);
    w_max = max(w_max, width);
    s += cnt;
  }
  stage_windows(ix, lds, first, s - first, md);
  wave_sync();
  const int t_start = max(0, w_min - 1);
  const bool even = ((t_start - my_o) & 1) == 0;  // which of the lane's sets is due on even steps
  u32 bp, bq;
  if constexpr (FLOOR) {
    int ran = 0;
    wavefront_quad<true>(lds, even ? ja : jb, even ? jb : ja, even ? 0 : 1, even ? 1 : 0, my_o, my_w, L, w_min, w_max, bp, bq, floor, &ran);
    iters[0] += static_cast<u32>(ran);
    iters[1] += static_cast<u32>(quad_iterations(L, w_min, w_max));
  }
  else wavefront_quad(lds, even ? ja : jb, even ? jb : ja, even ? 0 : 1, even ? 1 : 0, my_o, my_w, L, w_min, w_max, bp, bq);
  const u32 best_a = even ? bp : bq, best_b = even ? bq : bp;
  int base = 0, mine = 0;
  for (int k = first; k < s;) {
    const int cnt = min(4, s - k);
    int width = 0;
#pragma unroll
    for (int h = 0; h < 4; ++h)
      if (h < cnt) width = max(width, band_for(static_cast<int>(lds.jdf[k + h]) >> 16, md));
    const bool in = lane >= base && lane < base + width;
    const u32 xa = wave_max_pk(in ? best_a : 0u), xb = cnt > 1 ? wave_max_pk(in ? best_b : 0u) : 0u;
    if (lane == k - first) mine = static_cast<int>(xa & 0xFFFFu);
    if (lane == k + 1 - first && cnt > 1) mine = static_cast<int>(xb & 0xFFFFu);
    if (lane == k + 2 - first && cnt > 2) mine = static_cast<int>(xa >> 16);
    if (lane == k + 3 - first && cnt > 3) mine = static_cast<int>(xb >> 16);
    base += width;
    k += cnt;
  }
  wave_sync();
  lds.lbest[lane] = mine;
  wave_sync();
  return s;
}

// a round of scoring runs: four jobs per slot (packed cells) when at least kQuadMinJobs are left, else two (plain cells);
// the long-read kernel's 16-bit wrapping arithmetic stays on the plain cells.  The packed cell costs a quarter more
// than the plain one, so by instruction count it pays from a slot's third job on -- but the kernel that holds only one
// of the two loops is the faster one (10 M reads, same box, profiles/r03_exp_quad_scoring.log: never 701-712 ms, from
// three jobs on 685-695 ms, always 678-681 ms).
#ifndef ABM_QUAD_MIN_JOBS
#define ABM_QUAD_MIN_JOBS 1
#endif
constexpr int kQuadMinJobs = ABM_QUAD_MIN_JOBS;
template <bool WRAP = false>
__device__ __forceinline__ int score_jobs(const DevIndex &ix, const WaveLds &lds, int first, int n_jobs, int L, int md, int qbase) {
  if constexpr (!WRAP) {
    if (n_jobs - first >= kQuadMinJobs) return score_round_quad(ix, lds, first, n_jobs, L, md, qbase);
  }
  return score_round<WRAP>(ix, lds, first, n_jobs, L, md, qbase);
}

// (list_se_jobs and first_maximum restate what choose_se does inline, for choose_se_pilot: called from choose_se they
// changed the register allocation of two pair kernels, and those are to stay what they were.  Two copies to keep in
// step: a change to either helper must be mirrored in choose_se's body, and the other way round.)
// prepare_for_alignments (src/abismal.cpp:1435-1497): the set's entries ordered by (pos, flags), duplicates dropped,
// as the job list in LDS (jpos / jdf).  Returns the number of jobs.  Lane k looks
// at heap entry k; its payload sits in lane (key & 255).
__device__ __forceinline__ int list_se_jobs(const WaveLds &lds, const SeSet &S, int Ls) {
  const int lane = lane_id();
  const bool mine = lane < S.sz;
  const int slot_of = S.hk & 255;
  const u32 e_pos = __shfl(S.pp, slot_of), e_flags = __shfl(S.pf, slot_of);
  const int e_d = SeSet::key_d(S.hk);
  const u64 key = (static_cast<u64>(e_pos) << 16) | e_flags;
  bool dup = false;
  for (int k = 0; k < S.sz; ++k) {
    const u64 kk = rdlane(key, k);
    dup |= (mine && k < lane && kk == key);
  }
  // jobs = unique entries that the reference would align: non-empty, diffs < 0.4L
  const int invalid_at = static_cast<i16>(0.4 * Ls);  // valid_hit, :323-326
  const bool is_job = mine && !dup && e_pos != 0 && e_d < invalid_at;
  const u64 jobs = __ballot(is_job);
  int rank = 0;
  for (int k = 0; k < S.sz; ++k) {
    const u64 kk = rdlane(key, k);
    rank += ((jobs >> k) & 1) && kk < key;
  }
  const int n_jobs = __popcll(jobs);
  if (is_job) {
    lds.jpos[rank] = e_pos;
    lds.jdf[rank] = (static_cast<u32>(e_d) << 16) | e_flags;
  }
  wave_sync();
  return n_jobs;
}

// the first maximum of a traceback run's table in row-major order (max value, then smallest row, then smallest
// column) from each lane's best cell of its own column: score, row, column
__device__ __forceinline__ void first_maximum(int bw, int bv, int brow, int &sc, int &br, int &bc) {
  const int lane = lane_id();
  const u64 k64 = (static_cast<u64>(static_cast<u32>(bv)) << 32) |
                  (static_cast<u64>(0xFFFFu - static_cast<u32>(brow)) << 8) |
                  static_cast<u64>(0xFFu - static_cast<u32>(lane));
  const u64 topk = wave_max_u64(lane < bw ? k64 : 0ull);
  br = static_cast<int>(0xFFFFu - static_cast<u32>((topk >> 8) & 0xFFFFu));
  bc = static_cast<int>(0xFFu - static_cast<u32>(topk & 0xFFu));
  sc = static_cast<i16>(static_cast<int>(topk >> 32));
}

template <bool TALLY>
__device__ __forceinline__ void choose_se_pilot(const DevIndex &ix, const WaveLds &lds, u32 L, double frac, SeSet &S, Hit &best,
                                                u32 *cig_out, const CigarSink &sink, u32 &n_ops, bool &overflow, u32 &n_aln,
                                                u32 &n_single, u32 *iters);

// align_se_candidates (src/abismal.cpp:1435-1497) on the wave-resident set
// PILOT (the single-end kernels for reads that fit LDS): choose_se_pilot's order of the same work; iters: its tallies
template <bool WRAP = false, bool PILOT = false, bool TALLY = false>
__device__ __forceinline__ void choose_se(const DevIndex &ix, const WaveLds &lds, u32 L, double frac,
                                          SeSet &S, Hit &best, u32 *cig_out, const CigarSink &sink,
                                          u32 &n_ops, bool &overflow, u32 &n_aln, u32 &n_single, u32 *iters = nullptr) {
  if constexpr (PILOT) {
    static_assert(!WRAP && kTracebackByRows && kQuadMinJobs <= 1, "the pilot order: 32-bit scores, every round on the packed cells");
    choose_se_pilot<TALLY>(ix, lds, L, frac, S, best, cig_out, sink, n_ops, overflow, n_aln, n_single, iters);
    return;
  }
  const int lane = lane_id();
  const int Ls = static_cast<i16>(L);
  const int md = static_cast<i16>(frac * static_cast<u32>(Ls));  // valid_diffs_cutoff
  const int perfect = static_cast<i16>(2 * L);
  n_ops = 0;
  if (S.best_p != 0) {  // exact match: no alignment needed
    best.diffs = static_cast<i16>(S.best_d); best.flags = static_cast<u16>(S.best_f); best.pos = S.best_p;
    if (lane == 0) { store_out(cig_out, L << 4); if (sink.fin) sink.fin[0] = L << 4; }
    n_ops = 1;
    return;
  }
  // prepare_for_alignments: order by (pos, flags), drop duplicates.  Lane k looks
  // at heap entry k; its payload sits in lane (key & 255).
  const bool mine = lane < S.sz;
  const int slot_of = S.hk & 255;
  const u32 e_pos = __shfl(S.pp, slot_of), e_flags = __shfl(S.pf, slot_of);
  const int e_d = SeSet::key_d(S.hk);
  const u64 key = (static_cast<u64>(e_pos) << 16) | e_flags;
  bool dup = false;
  for (int k = 0; k < S.sz; ++k) {
    const u64 kk = rdlane(key, k);
    dup |= (mine && k < lane && kk == key);
  }
  // jobs = unique entries that the reference would align: non-empty, diffs < 0.4L
  const int invalid_at = static_cast<i16>(0.4 * Ls);  // valid_hit, :323-326
  const bool is_job = mine && !dup && e_pos != 0 && e_d < invalid_at;
  const u64 jobs = __ballot(is_job);
  int rank = 0;
  for (int k = 0; k < S.sz; ++k) {
    const u64 kk = rdlane(key, k);
    rank += ((jobs >> k) & 1) && kk < key;
  }
  const int n_jobs = __popcll(jobs);
  if (is_job) {
    lds.jpos[rank] = e_pos;
    lds.jdf[rank] = (static_cast<u32>(e_d) << 16) | e_flags;
  }
  wave_sync();

  int top = 0;
  u32 top_pos = 0, b_pos = 0, b_flags = 0;
  int b_diffs = 0x7fff;
  // A set with ONE alignable entry (most reads that map uniquely with a mismatch or two): the reference scores it
  // (align<false>) and then aligns it again with traceback (align<true>) -- the same table twice, so the traceback
  // run's score is the scoring run's, and the scoring run is skipped.
  const bool single = n_jobs == 1;
  if (single) {
    const u32 df = lds.jdf[0];
    b_diffs = static_cast<int>(df) >> 16; b_flags = df & 0xFFFFu; b_pos = lds.jpos[0];
    ++n_aln;
    ++n_single;
  }
  for (int s = 0; s < n_jobs && !single;) {
    const int first = s;
    s = score_jobs<WRAP>(ix, lds, first, n_jobs, static_cast<int>(L), md, 0);
    // apply the reference's selection in job order
    for (int k = first; k < s; ++k) {
      const u32 df = lds.jdf[k];
      const int d = static_cast<int>(df) >> 16;
      const int sc = static_cast<i16>(lds.lbest[k - first]);
      const u32 pos = lds.jpos[k], flags = df & 0xFFFFu;
      ++n_aln;
      if (sc > top) { b_diffs = d; b_flags = flags; b_pos = pos; top = sc; top_pos = pos; }
      else if (sc == top) {
        const u32 gap = pos > top_pos ? pos - top_pos : top_pos - pos;
        if (sc == perfect ? pos != top_pos : gap > 3u) b_flags |= kFlagAmbig;
      }
    }
    wave_sync();
  }
  best.diffs = 0x7fff; best.flags = static_cast<u16>(b_flags); best.pos = 0;
  if (b_pos == 0)
    return;
  // traceback run of the winner: one job, band in lanes [0, bw)
  const int bw = band_for(b_diffs, md);
  AlnJob job = {0, 0, 0, 0, 0};
  const u64 t_beg = static_cast<u64>(b_pos) - static_cast<u64>((bw - 1) / 2);
  if (lane < bw) {
    job.bw = bw;
    job.jl = lane;
    job.qoff = static_cast<int>(enc_of(b_flags) * lds.W);
    job.t0nib = static_cast<int>(t_beg & 15u);
  }
  if (lane == 0) { lds.jpos[0] = b_pos; lds.jdf[0] = (static_cast<u32>(b_diffs) << 16) | (b_flags & 0xFFFFu); }
  wave_sync();
  stage_windows(ix, lds, 0, 1, md);
  wave_sync();
  int bv, brow;
  if constexpr (WRAP || !kTracebackByRows) wavefront<true, WRAP>(lds, job, static_cast<int>(L), bw, bw, bv, brow);
  else wavefront_rows<true>(lds, job, static_cast<int>(L), bw, bv, brow);
  // first maximum in row-major order: max value, then smallest row, then smallest column
  const u64 k64 = (static_cast<u64>(static_cast<u32>(bv)) << 32) |
                  (static_cast<u64>(0xFFFFu - static_cast<u32>(brow)) << 8) |
                  static_cast<u64>(0xFFu - static_cast<u32>(lane));
  const u64 topk = wave_max_u64(lane < bw ? k64 : 0ull);
  const int br = static_cast<int>(0xFFFFu - static_cast<u32>((topk >> 8) & 0xFFFFu));
  const int bc = static_cast<int>(0xFFu - static_cast<u32>(topk & 0xFFu));
  const int sc = static_cast<i16>(static_cast<int>(topk >> 32));
  wave_sync();
  if (single) {  // what the scoring run would have found
    top = sc;
    if (sc <= 0) { best.flags = static_cast<u16>(kFlagAmbig); return; }  // (a zero score ties with "nothing yet" at position 0)
  }
  u32 alen = 0, pos = b_pos;
  int n_ins = 0, n_del = 0;
  wave_cigar(lds.tb, lds.ctmp, static_cast<int>(L), b_diffs, md, sc, br, bc, cig_out, sink, n_ops,
             n_ins, n_del, alen, pos, overflow);
  wave_sync();
  // NM from the score found by the scoring pass (best_scr), as the reference does
  const int nm = edit_distance(top, alen, n_ins, n_del);
  if (long_enough(alen, static_cast<u32>(Ls), ix.min_len) && nm <= md) {
    best.diffs = static_cast<i16>(nm);
    best.pos = pos;
  }
  // (a hit that fails here leaves best.pos == 0; n_ops still counts the CIGAR the traceback wrote into the slot,
  // like the reference's r.cig, so that count and slot -- or arena reference -- always belong together)
}


// choose_se for the kernels whose reads fit LDS, with the work in another order and the same outcome.  The outcome is
// a function of the maximum score M over the jobs, the first job (in list order) that reaches M, and the later jobs
// that equal M; what a job below M scores exactly is never seen.  So, with two jobs or more:
//   1. the job with the fewest mismatches (the lowest index among equals) is the pilot: its traceback run comes first
//      -- the same table as its scoring run, so the table's maximum is the pilot's score Sp (as for a lone job);
//   2. the pilot's CIGAR is walked out of the table into ctmp and held back: the scoring rounds overwrite the table
//      (it overlays the window slots), and nothing is published before the pilot is confirmed;
//   3. the other jobs are scored in rounds against a floor (wavefront_quad<true>): Sp, then the best score seen.  A
//      round ends once none of its jobs can reach the floor; those jobs report less than the floor, hence less than M;
//   4. the reference's selection runs in list order over all scores, Sp in the pilot's place.  A job below M may take
//      the lead early or tie with a leader below M -- the first job at M overwrites both, as in the reference;
//   5. the pilot won: its held CIGAR is published.  Another job won (a tie from a lower position, or a gapped
//      alignment that beats the pilot): its traceback runs as in choose_se, over the held ops.
// The traceback code exists once: the loop below passes through it for the pilot and, if need be, again for the winner.
template <bool TALLY>
__device__ __forceinline__ void choose_se_pilot(const DevIndex &ix, const WaveLds &lds, u32 L, double frac, SeSet &S, Hit &best,
                                                u32 *cig_out, const CigarSink &sink, u32 &n_ops, bool &overflow, u32 &n_aln,
                                                u32 &n_single, u32 *iters) {
  const int lane = lane_id();
  const int Ls = static_cast<i16>(L);
  const int md = static_cast<i16>(frac * static_cast<u32>(Ls));  // valid_diffs_cutoff
  const int perfect = static_cast<i16>(2 * L);
  n_ops = 0;
  if (S.best_p != 0) {  // exact match: no alignment needed
    best.diffs = static_cast<i16>(S.best_d); best.flags = static_cast<u16>(S.best_f); best.pos = S.best_p;
    if (lane == 0) { store_out(cig_out, L << 4); if (sink.fin) sink.fin[0] = L << 4; }
    n_ops = 1;
    return;
  }
  const int n_jobs = list_se_jobs(lds, S, Ls);
  best.diffs = 0x7fff; best.flags = 0; best.pos = 0;
  if (n_jobs == 0) return;
  const bool single = n_jobs == 1;
  int pilot = 0;
  if (!single) pilot = wave_min_i32(lane < n_jobs ? static_cast<int>(((lds.jdf[lane] >> 16) << 8) | static_cast<u32>(lane)) : 0x7fffffff) & 255;
  const u32 p_pos = lds.jpos[pilot], p_df = lds.jdf[pilot];
  int trace = pilot;  // the list entry under traceback
  int top = 0, b_diffs = static_cast<int>(p_df) >> 16;
  u32 b_pos = p_pos, b_flags = p_df & 0xFFFFu;
  for (bool pilot_pass = !single;; pilot_pass = false) {
    // traceback run of list entry `trace`: one job, band in lanes [0, bw), its window in slot 0
    const int bw = band_for(b_diffs, md);
    AlnJob job = {0, 0, 0, 0, 0};
    const u64 t_beg = static_cast<u64>(b_pos) - static_cast<u64>((bw - 1) / 2);
    if (lane < bw) {
      job.bw = bw;
      job.jl = lane;
      job.qoff = static_cast<int>(enc_of(b_flags) * lds.W);
      job.t0nib = static_cast<int>(t_beg & 15u);
    }
    stage_windows(ix, lds, trace, 1, md);
    wave_sync();
    int bv, brow, sc, br, bc;
    wavefront_rows<true>(lds, job, static_cast<int>(L), bw, bv, brow);
    first_maximum(bw, bv, brow, sc, br, bc);
    wave_sync();
    // (wave_cigar's shortcut for a job without mismatches or without a score is not needed: a set entry has d >= 1 --
    // SeSet::admit keeps d == 0 apart as the exact match, which returned above -- and only a score > 0 is published)
    CigarWalk walk = {0, 0, 0, 0};
    int n_ins = 0, n_del = 0;
    if (sc > 0) walk = cigar_walk(lds.tb, lds.ctmp, sink.ctmp_cap, static_cast<int>(L), bw, br, bc, n_ins, n_del);
    if (single) {  // what the scoring run would have found
      ++n_aln;
      ++n_single;
      top = sc;
      if (sc <= 0) { best.flags = static_cast<u16>(kFlagAmbig); return; }  // (a zero score ties with "nothing yet" at position 0)
      best.flags = static_cast<u16>(b_flags);
    }
    if (pilot_pass) {
      // the pilot leaves the list (the entries behind it move up), the rest is scored against the floor
      u32 mv_pos = 0, mv_df = 0;
      const bool moves = lane > pilot && lane < n_jobs;
      if (moves) { mv_pos = lds.jpos[lane]; mv_df = lds.jdf[lane]; }
      wave_sync();
      if (moves) { lds.jpos[lane - 1] = mv_pos; lds.jdf[lane - 1] = mv_df; }
      wave_sync();
      const int n_rest = n_jobs - 1;
      int floor = sc, b_at = -1;  // b_at: the leader's list entry, -1 = the pilot
      u32 top_pos = 0;
      top = 0; b_pos = 0; b_flags = 0; b_diffs = 0x7fff;
      auto select = [&](int at, u32 pos, u32 df, int s) {  // the reference's selection, in job order
        const u32 flags = df & 0xFFFFu;
        ++n_aln;
        if (s > top) { b_diffs = static_cast<int>(df) >> 16; b_flags = flags; b_pos = pos; top = s; top_pos = pos; b_at = at; }
        else if (s == top) {
          const u32 gap = pos > top_pos ? pos - top_pos : top_pos - pos;
          if (s == perfect ? pos != top_pos : gap > 3u) b_flags |= kFlagAmbig;
        }
      };
      u32 it[2] = {0, 0};
      for (int s = 0; s < n_rest;) {
        const int first = s;
        s = score_round_quad<true>(ix, lds, first, n_rest, static_cast<int>(L), md, 0, floor, it);
        for (int k = first; k < s; ++k) {
          if (k == pilot) select(-1, p_pos, p_df, sc);
          const int sk = static_cast<i16>(lds.lbest[k - first]);
          select(k, lds.jpos[k], lds.jdf[k], sk);
          floor = max(floor, sk);
        }
        wave_sync();
      }
      if (pilot == n_rest) select(-1, p_pos, p_df, sc);
      if (TALLY) { iters[0] += it[0]; iters[1] += it[1]; }
      best.flags = static_cast<u16>(b_flags);
      if (b_pos == 0) return;
      if (b_at >= 0) { trace = b_at; continue; }  // not the pilot: the held ops are dropped
    }
    u32 alen = 0, pos = b_pos;
    cigar_publish(lds.ctmp, walk, static_cast<int>(L), bw, cig_out, sink, n_ops, alen, pos, overflow);
    wave_sync();
    // NM from the score found by the scoring pass (best_scr), as the reference does
    const int nm = edit_distance(top, alen, n_ins, n_del);
    if (long_enough(alen, static_cast<u32>(Ls), ix.min_len) && nm <= md) {
      best.diffs = static_cast<i16>(nm);
      best.pos = pos;
    }
    return;
  }
}

}  // namespace abm
