// abismal_amd HIP kernels for gfx950: paired-end mapping, one wavefront per pair.
// Restates map_paired_ended / map_paired_ended_rand's per-pair body
// (src/abismal.cpp:1950-1999, :2094-2155): two or four orientation calls
// (map_fragments :1849-1885), each seeding both ends into growable candidate
// sets (pe_candidates :775-863), mating them (best_pair :1722-1831), feeding the
// single-end sets (best_single :1715-1720), then valid_pair and the single-end
// fallback.  The per-pair body is split by phase where its register pressure
// is (round 5): a SEED kernel (both seed passes of every orientation call's two
// ends; shaped like the single-end kernel: no alignment state, small LDS) hands
// the finished candidate lists over in global memory, and MATE kernels take
// them from there (sort, scoring, mating, tracebacks, best_single, fallback) --
// lists of up to kPeTier1Cap entries in LDS, longer ones in global memory.
// Pairs whose sets outgrow the seed kernel (its staging area, or the heap of a
// sensitive pass) go through the WHOLE-pair kernel: the same code unsplit, one
// wave per pair with 32768-entry sets in global memory (tier 2).
#include <climits>
#include <utility>
#include "abm_align.hpp"
#include "abm_pe_set.hpp"
#include "abm_pe_wave.hpp"
#include "abm_sam.hpp"

// Waves per SIMD the pair kernels are compiled for: 4 (128 registers per lane), and for the production kernels on the
// bit planes also 3 (170 registers): with 2x150-base pairs the LDS of a wave allows 13 waves per CU anyway, and the
// build with more registers is the faster one there; with 2x100 the LDS allows 16 and four waves per SIMD win
// (profiles/r03_exp_pe_loop_and_registers.log, r03_exp_pe_2x100_variants.log).  pe_select() (abm_kernel_form.hpp) picks per launch.

namespace abm {

// ---- a pair's SAM records written by the wave that finished it (PeArgs::sam_tail) -----------------------------------
// select_output (src/abismal.cpp:1073-1088; the CLI's emit_pe / emit_se): the proper pair's two records (format_pe,
// :648-773), or else up to two single-end records (format_se, :481-545), each minus QNAME.  The line of end e of pair r
// goes to sam_tail + (2 r + e) * sam_stride, its length to sam_len[2 r + e] (0: no record), the pair's kind to
// sam_kind[r]: kPeTextPair, kPeTextSingles (also a proper pair whose ends cannot both be located on one chromosome), or
// kPeTextHost -- an end beyond kLdsReadLen bases, a CIGAR beyond `fin`, a line beyond its slot: the host formats the
// whole pair.  line: the traceback table's place, idle once both CIGARs are out (at least sam_stride bytes: the host
// checks, sam_line_room); fin: each end's last traceback's first kSeCap ops.
// BAM: each record as a BAM piece instead (BamWriter; PeArgs::sam_format == kRecordsBam picks these builds)
template <bool BAM>
__device__ __forceinline__ void format_pe_tails(const PeArgs &a, u8 *line, const u32 *fin, u64 r, const u32 L[2],
                                                const PairBest &best, const Hit &h1, const Hit &h2, const u32 n_ops[2]) {
  const int lane = lane_id();
  const bool allow = a.sam_allow_ambig != 0;
  u8 kind = kPeTextSingles;
  u32 len[2] = {0u, 0u};
  wave_sync();  // (fin was written by whichever lanes stored the CIGARs)
  if (a.lens1[r] > kLdsReadLen || a.lens2[r] > kLdsReadLen) kind = kPeTextHost;  // (the long-end launch's pair, or too long)
  else if (best.p1 != 0 && (allow || !(best.f1 & kFlagAmbig))) {  // format_pe
    if (n_ops[0] == 0 || n_ops[1] == 0 || n_ops[0] > kSeCap || n_ops[1] > kSeCap) kind = kPeTextHost;
    else {
      const u32 rl1 = sam_ref_len(fin, n_ops[0]), rl2 = sam_ref_len(fin + kSeCap, n_ops[1]);
      u32 ch1 = 0, ch2 = 0, b1 = 0, b2 = 0;
      if (sam_locate(a.ix, best.p1, rl1, ch1, b1) && sam_locate(a.ix, best.p2, rl2, ch2, b2) && ch1 == ch2) {
        kind = kPeTextPair;
        b1 = best.p1 - b1; b2 = best.p2 - b2;
        const u32 e2 = b2 + rl2;
        const bool rc1 = (best.f1 & kFlagRC) != 0, rc2 = (best.f2 & kFlagRC) != 0;
        const int isize = rc1 ? static_cast<int>(b1) - static_cast<int>(e2) : static_cast<int>(e2) - static_cast<int>(b1);
        const u32 amb = (allow && (best.f1 & kFlagAmbig)) ? 0x100u : 0u;
        const u32 f1 = 0x1u | 0x2u | 0x40u | (rc1 ? 0x10u : 0u) | (rc2 ? 0x20u : 0u) | amb;
        const u32 f2 = 0x1u | 0x2u | 0x80u | (rc2 ? 0x10u : 0u) | (rc1 ? 0x20u : 0u) | amb;
        for (int e = 0; e < 2; ++e) {
          if constexpr (BAM) {
            const BamFields f{static_cast<int>(ch1) - 1, e ? b2 : b1, e ? rl2 : rl1, e ? f2 : f1, static_cast<int>(ch1) - 1, e ? b1 : b2,
                              e ? -isize : isize, static_cast<i16>(e ? best.d2 : best.d1), ((e ? best.f2 : best.f1) & kFlagARich) != 0};
            len[e] = BamWriter{line, a.sam_stride}.write(f, fin + e * kSeCap, e ? n_ops[1] : n_ops[0], (e ? a.blob2 + a.off2[r] : a.blob1 + a.off1[r]),
                                                         e ? L[1] : L[0], e ? rc2 : rc1, a.sam_tail + (2 * r + e) * a.sam_stride);
            if (len[e] == 0xFFFFFFFFu) { kind = kPeTextHost; break; }
            wave_sync();  // (the next piece is built where this one was read from)
            continue;
          }
          SamWriter o{line, 0, a.sam_stride};
          o.put('\t');
          o.put_uint(e ? f2 : f1);
          o.put('\t');
          o.put_chrom(a.ix, ch1);
          o.put('\t');
          o.put_uint((e ? b2 : b1) + 1u);
          o.put_str("\t255\t", 5);
          o.put_cigar(fin + e * kSeCap, e ? n_ops[1] : n_ops[0]);
          o.put_str("\t=\t", 3);
          o.put_uint((e ? b1 : b2) + 1u);
          o.put('\t');
          o.put_int(e ? -isize : isize);
          o.put('\t');
          o.put_seq((e ? a.blob2 + a.off2[r] : a.blob1 + a.off1[r]), e ? L[1] : L[0], e ? rc2 : rc1);
          o.put_tags(static_cast<i16>(e ? best.d2 : best.d1), ((e ? best.f2 : best.f1) & kFlagARich) != 0);
          if (o.w > o.cap) { kind = kPeTextHost; break; }
          o.flush(reinterpret_cast<u32 *>(a.sam_tail + (2 * r + e) * a.sam_stride));
          wave_sync();  // (the next line is built where this one was read from)
          len[e] = o.w;
        }
      }
    }
  }
  if (kind == kPeTextSingles) {  // format_se of either end (the hits the fallback left; none if it did not run)
    for (int e = 0; e < 2; ++e) {
      const Hit &h = e ? h2 : h1;
      const u32 nops = e ? n_ops[1] : n_ops[0];
      const bool ambig = (h.flags & kFlagAmbig) != 0;
      if (h.pos == 0 || (ambig && !allow)) continue;
      if (nops == 0 || nops > kSeCap) { kind = kPeTextHost; break; }
      u32 chrom = 0, c0 = 0;
      const u32 reflen = sam_ref_len(fin + e * kSeCap, nops);
      if (!sam_locate(a.ix, h.pos, reflen, chrom, c0)) continue;
      const bool rc = (h.flags & kFlagRC) != 0;
      const u32 flag = (rc ? 0x10u : 0u) | ((allow && ambig) ? 0x100u : 0u);
      if constexpr (BAM) {
        const BamFields f{static_cast<int>(chrom) - 1, h.pos - c0, reflen, flag, -1, 0u, 0, h.diffs, (h.flags & kFlagARich) != 0};
        len[e] = BamWriter{line, a.sam_stride}.write(f, fin + e * kSeCap, nops, (e ? a.blob2 + a.off2[r] : a.blob1 + a.off1[r]), e ? L[1] : L[0], rc,
                                                     a.sam_tail + (2 * r + e) * a.sam_stride);
        if (len[e] == 0xFFFFFFFFu) { kind = kPeTextHost; break; }
        wave_sync();
        continue;
      }
      SamWriter o{line, 0, a.sam_stride};
      o.put('\t');
      o.put_uint(flag);
      o.put('\t');
      o.put_chrom(a.ix, chrom);
      o.put('\t');
      o.put_uint(h.pos - c0 + 1u);
      o.put_str("\t255\t", 5);
      o.put_cigar(fin + e * kSeCap, nops);
      o.put_str("\t*\t0\t0\t", 7);
      o.put_seq((e ? a.blob2 + a.off2[r] : a.blob1 + a.off1[r]), e ? L[1] : L[0], rc);
      o.put_tags(h.diffs, (h.flags & kFlagARich) != 0);
      if (o.w > o.cap) { kind = kPeTextHost; break; }
      o.flush(reinterpret_cast<u32 *>(a.sam_tail + (2 * r + e) * a.sam_stride));
      wave_sync();
      len[e] = o.w;
    }
  }
  if (kind == kPeTextHost) len[0] = len[1] = 0;
  if (lane == 0) {
    store_out(a.sam_len + 2 * r, len[0]);
    store_out(a.sam_len + 2 * r + 1, len[1]);
    a.sam_kind[r] = kind;
  }
}

// REC: the seed passes filter on the window records (DevIndex::wrec) -- a launch none of whose ends is longer than they serve
// TEXT: the pair's SAM records are written as well (PeArgs::sam_tail, format_pe_tails)
// BAM: ... as BAM pieces (TEXT builds of their own, so that the ones that existed keep their code)
// One kernel per row of kPeForms (abm_kernel_form.hpp): F is the row's id, PeForm::valid what the fields may be together
template <u32 F>
__global__ __launch_bounds__(64, pe_form_of(F).wps) void map_pe_kernel(PeArgs a) {
  constexpr PeForm form = pe_form_of(F);
  static_assert(form.valid(), "no such build of the pair kernels");
  constexpr bool BIG = form.big, TIMED = form.timed, COOP = form.coop, LONG = form.is_long, REC = form.rec, TEXT = form.text, BAM = form.bam;
  constexpr int PHASE = form.phase;
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  PeWave<BIG, COOP, LONG, PHASE, REC, TEXT> w{a};
  WaveLds &lds = w.lds;
  pe_carve<BIG, LONG, PHASE, TEXT>(lds, w.pl, w.fin, w.samp, smem, a);
  if constexpr (PHASE != kMate) { lds.smark[lane] = 0; lds.smark[64 + lane] = 0; }
  w.seg_epoch = 0;

  w.P.heap = w.pl.heap;
  w.samp_shift = 0; w.samp_n = 0;
  w.P.spill_pos = nullptr; w.P.spill_d = nullptr; w.P.spill_cap = 0; w.P.spilled = false;
  w.stage_pos = nullptr; w.stage_d = nullptr;
  if constexpr (PHASE == kSeed) {
    if (a.scap > a.cap) {
      w.stage_pos = a.stage_pos + static_cast<u64>(blockIdx.x) * a.scap;
      w.stage_d = a.stage_d + static_cast<u64>(blockIdx.x) * a.scap;
    }
  }
  w.log_base = BIG ? a.log_ws + static_cast<u64>(blockIdx.x) * (32ull + 12ull * a.cap) : nullptr;
  w.P.cap_avail = a.cap;
  w.wt = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  w.n_aln = 0;
  w.overflow = false;
  w.t_sort = w.t_score = w.t_mate = w.t_single = 0;
  bool too_long = false;
  long long t_begin = 0, t_fb = 0;
  u32 routed_small = 0, routed_whole = 0, routed_big = 0;  // seed kernel: pairs of this wave by route
  ABM_STAMP(t_begin);

  auto next_item = [&]() -> u64 {
    unsigned long long v = 0;
    if (lane == 0) v = atomicAdd(a.next_read, 1ull);
    return (static_cast<u64>(static_cast<u32>(uni(static_cast<int>(v >> 32)))) << 32) |
           static_cast<u32>(uni(static_cast<int>(v)));
  };
  const u64 n_items = BIG ? static_cast<u64>(*a.subset_count) : a.n_pairs;
  u64 it_next = next_item();
  while (it_next < n_items) {
    const u64 it = it_next;
    it_next = next_item();
    __builtin_amdgcn_s_setprio(0);  // (a heavy end raises its wave's priority: seed_pass)
    const u64 r = BIG ? static_cast<u64>(a.subset[it]) : (a.order ? static_cast<u64>(a.order[it]) : it);
    if constexpr (PHASE == kMate && !BIG) {  // (the small-list mate kernel walks the whole batch: the other routes' pairs are not its)
      if (static_cast<u8>(uni(static_cast<int>(a.need_big[r]))) != kRouteSmall) continue;
    }
    w.L[0] = a.lens1[r];
    w.L[1] = a.lens2[r];
    if (w.L[0] > kMaxReadLen || w.L[1] > kMaxReadLen) { too_long = true; w.L[0] = w.L[1] = 0; }
    // (a pair with an end beyond this launch's length is the long-end launch's: it overwrites what is stored for it here)
    if (!LONG && (w.L[0] > kLdsReadLen || w.L[1] > kLdsReadLen)) w.L[0] = w.L[1] = 0;
    // stage both ends' four encodings and their 2-letter bit strings (LONG: packed by list position)
    #pragma unroll
    for (int e = 0; e < 2; ++e) {
      const u64 *src = (e ? a.packed2 : a.packed1) + (LONG ? it : r) * 4 * a.W;
      for (u32 k = lane; k < 4 * a.W; k += 64) lds.qpk[e * 4 * a.W + k] = src[k];
    }
    wave_sync();
    if constexpr (PHASE != kMate) {
      for (u32 e8 = 0; e8 < 8; ++e8)
        for (u32 wb = 0; wb < a.WB; ++wb) {
          const u32 j = wb * 64 + lane, Le = e8 < 4 ? w.L[0] : w.L[1];
          const bool b = j < Le ? bit2(q_nibble(lds.qpk + e8 * a.W, j)) : true;
          const u64 word = __ballot(b);
          if (lane == 0) lds.qbits[e8 * a.WB + wb] = word;
        }
      if constexpr (COOP) { build_qmasks(w.lds_of(0), w.L[0]); build_qmasks(w.lds_of(1), w.L[1]); }
      wave_sync();
      #pragma unroll
      for (int e = 0; e < 2; ++e)  // 44-46 bases: seeds reach past the end of the read (see ghost_bits)
        if (w.L[e] >= a.ix.map_len() && w.L[e] < max(a.ix.window, w.L[e] >> 1) + kKeyWeight - 1)
          ghost_bits(e ? a.packed2 : a.packed1, e ? a.lens2 : a.lens1, r, w.L[e], a.max_len, a.ix.map_len(), a.W, a.WB, lds.qbits + e * 4 * a.WB);
    }

    if constexpr (PHASE == kSeed) {
      // both seed passes of every orientation call's two ends; the lists go to the hand-over area, the pair to its route
      w.need_big = false;
      w.max_set = 0;
      const int n_or = a.mode == 2 ? 4 : 2;
#pragma clang loop unroll(disable)
      for (int o = 0; o < n_or; ++o) {
        if (w.need_big) break;
        const bool ar_o = a.mode == 2 ? (o == 1 || o == 2) : ((a.mode == 1) != (o == 1));
        PairBest unused;
        (void)w.template orientation<TIMED>(o, o & 1, ar_o, r, unused);
      }
      const u8 route = w.need_big ? kRouteWhole : (w.max_set > static_cast<int>(kPeTier1Cap) ? kRouteBig : kRouteSmall);
      if (lane == 0) a.need_big[r] = route;
      routed_small += route == kRouteSmall; routed_whole += route == kRouteWhole; routed_big += route == kRouteBig;
      continue;
    }

    PairBest best;
    best.f1 = best.f2 = 0;
    best.clear(w.L[0] >= a.ix.map_len() ? w.L[0] : 0u, w.L[1] >= a.ix.map_len() ? w.L[1] : 0u);
    w.se[0].begin_read(w.L[0] >= a.ix.map_len() ? w.L[0] : 0u);
    w.se[1].begin_read(w.L[1] >= a.ix.map_len() ? w.L[1] : 0u);
    w.need_big = false;
    if (BIG && lane < 8) w.log_head(lane)[0] = 0;  // no list logged yet for this pair
    w.max_set = 0;
    long long t_pair = 0;
    ABM_STAMP(t_pair);
    const long long ph0[8] = {w.wt.t_probe, w.wt.t_stream, w.wt.t_replay, w.t_sort, w.t_score, w.t_mate, w.t_single, t_fb};
    w.n_ops[0] = w.n_ops[1] = 0;
    w.ref_len[0] = w.ref_len[1] = 0;

    bool any = false;
    // orientation(endA, alphabet): src/abismal.cpp:1963-1979, :2106-2133
    // ONE copy of the orientation code, looped over (six inlined copies made the tier-1 kernel 155 k lines of assembly)
    {
      const int n_or = a.mode == 2 ? 4 : 2;
#pragma clang loop unroll(disable)
      for (int o = 0; o < n_or; ++o) {
        if (o > 0 && w.need_big && !BIG) break;
        const bool ar_o = a.mode == 2 ? (o == 1 || o == 2) : ((a.mode == 1) != (o == 1));
        any |= w.template orientation<TIMED>(o, o & 1, ar_o, r, best);
      }
    }
    if (w.need_big && !BIG) {
      if (lane == 0) a.need_big[r] = kRouteWhole;
      continue;
    }
    if (!any) {  // :1981-1985
      best.clear();
      w.se[0].begin_read(0); w.se[0].hk = 32767 * 256; w.se[0].cutoff = 32767; w.se[0].best_d = 32767;
      w.se[1].begin_read(0); w.se[1].hk = 32767 * 256; w.se[1].cutoff = 32767; w.se[1].best_d = 32767;
    }
    {  // valid_pair, :624-631, on whatever CIGARs the mating left behind
      const u32 a1 = w.ref_len[0], a2 = w.ref_len[1];
      const bool ok = long_enough(a1, w.L[0], a.ix.min_len) && long_enough(a2, w.L[1], a.ix.min_len) &&
                      static_cast<i16>(best.d1 + best.d2) <= static_cast<i16>(a.valid_frac * (a1 + a2));
      if (!ok) best.clear();
    }
    Hit h1, h2;
    h1.diffs = static_cast<i16>(0.4 * w.L[0]); h1.flags = 0; h1.pos = 0;
    h2.diffs = static_cast<i16>(0.4 * w.L[1]); h2.flags = 0; h2.pos = 0;
    if (!best.should_report(a.allow_ambig != 0)) {  // single-end fallback at half the error budget
      if (BIG) { wave_sync(); w.replay_singles(); }
      long long tf0 = 0, tf1 = 0;
      ABM_STAMP(tf0);
      #pragma unroll
      for (int e = 0; e < 2; ++e) {
        const WaveLds we = w.lds_of(e);
        u32 nops = 0;
        Hit &h = e ? h2 : h1;
        u32 n_single = 0;
        choose_se<LONG>(a.ix, we, w.L[e], a.valid_frac / 2, w.se[e], h, w.cig_of(e, r), w.sink(e), nops,
                        w.overflow, w.n_aln, n_single);
        if (nops != 0) w.n_ops[e] = nops;  // whatever traceback ran last owns the slot (A.10)
      }
      ABM_STAMP(tf1);
      if (TIMED) t_fb += tf1 - tf0;
    }
    if constexpr (TEXT) format_pe_tails<BAM>(a, lds.tb, w.fin, r, w.L, best, h1, h2, w.n_ops);
    if (lane == 0) {
      u32 *po = reinterpret_cast<u32 *>(a.pairs) + r * 5;
      po[0] = static_cast<u32>(static_cast<u16>(static_cast<i16>(best.aln_score)));
      po[1] = static_cast<u32>(static_cast<u16>(static_cast<i16>(best.d1))) | ((best.f1 & 0xFFFFu) << 16);
      po[2] = best.p1;
      po[3] = static_cast<u32>(static_cast<u16>(static_cast<i16>(best.d2))) | ((best.f2 & 0xFFFFu) << 16);
      po[4] = best.p2;
      a.se1[r] = h1;
      a.se2[r] = h2;
      a.cig_n1[r] = w.n_ops[0];
      a.cig_n2[r] = w.n_ops[1];
      if (!BIG && PHASE == kWhole) a.need_big[r] = kRouteSmall;
      // (A wave that holds a 32768-entry pair stays resident for half a second.  On a GPU it shares with other processes its
      // s_memtime has been seen to step BACK between two stamps -- by 10^7 to 2 x 10^8 cycles, on several such waves in the
      // same launch, in whichever phase each was in -- which makes a phase's cycles negative: as an unsigned word that
      // would take the pair's earlier cycles away again, and set every bit of the word above.  Such a difference counts as 0.)
      if (TIMED && a.pair_diag)
        a.pair_diag[r] = (min(static_cast<u32>(w.max_set), 0xFFFFu) << 16) |
                         static_cast<u32>(max(min((phase_stamp() - t_pair) >> 20, 0xFFFFll), 0ll));
      if (TIMED && a.pair_phases) {
        const long long ph1[8] = {w.wt.t_probe, w.wt.t_stream, w.wt.t_replay, w.t_sort, w.t_score, w.t_mate, w.t_single, t_fb};
        for (int k = 0; k < 8; ++k) a.pair_phases[r * 8 + k] += static_cast<u32>(max(ph1[k] - ph0[k], 0ll) >> 10);
      }
    }
  }
  if (a.work) {
    auto wsum = [&](u32 v) { u32 t; (void)wave_excl_sum(v, t); return t; };
    const u32 s0 = wsum(w.wt.seed_iters), s1 = wsum(w.wt.probes), s2 = wsum(w.wt.cands), s3 = wsum(w.wt.words);
    const u32 wsum_hits = wsum(w.wt.cache_hits);
    if (lane == 0) {
      atomicAdd(&a.work[0], static_cast<unsigned long long>(s0));
      atomicAdd(&a.work[1], static_cast<unsigned long long>(s1));
      atomicAdd(&a.work[2], static_cast<unsigned long long>(s2));
      atomicAdd(&a.work[3], static_cast<unsigned long long>(s3));
      atomicAdd(&a.work[4], static_cast<unsigned long long>(w.wt.updates));
      atomicAdd(&a.work[5], static_cast<unsigned long long>(w.n_aln));
      atomicAdd(&a.work[11], static_cast<unsigned long long>(wsum_hits));
      if (TIMED) {
        atomicAdd(&a.work[6], static_cast<unsigned long long>(w.wt.t_probe));
        atomicAdd(&a.work[7], static_cast<unsigned long long>(w.wt.t_stream));
        atomicAdd(&a.work[8], static_cast<unsigned long long>(w.wt.t_replay));
        atomicAdd(&a.work[9], static_cast<unsigned long long>(t_fb));
        atomicAdd(&a.work[10], static_cast<unsigned long long>(phase_stamp() - t_begin));
        atomicAdd(&a.work[12], static_cast<unsigned long long>(w.t_sort));
        atomicAdd(&a.work[13], static_cast<unsigned long long>(w.t_score));
        atomicAdd(&a.work[14], static_cast<unsigned long long>(w.t_mate));
        atomicAdd(&a.work[15], static_cast<unsigned long long>(w.t_single));
      }
    }
  }
  if constexpr (PHASE == kSeed) {
    if (a.split_stats && lane == 0) {
      if (routed_small) atomicAdd(&a.split_stats[kRouteSmall], static_cast<unsigned long long>(routed_small));
      if (routed_whole) atomicAdd(&a.split_stats[kRouteWhole], static_cast<unsigned long long>(routed_whole));
      if (routed_big) atomicAdd(&a.split_stats[kRouteBig], static_cast<unsigned long long>(routed_big));
    }
  }
  if (lane == 0 && (w.overflow || too_long))
    atomicOr(a.status, (w.overflow ? 1u : 0u) | (too_long ? 2u : 0u));
  if (a.host_tail != nullptr && lane == 0) {  // the last wave to get here publishes the launch's two summary words
    __threadfence();
    const u32 before = atomicAdd(a.finished, 1u);
    if (before + 1u == gridDim.x) {
      __threadfence();
      a.host_tail[0] = __hip_atomic_load(a.cig_arena_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      a.host_tail[1] = __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// compact the pairs of one route (PeArgs::need_big) into a list for that route's launch, heaviest weight class first (a
// counting sort on the class the ordering kernels already computed): the few pairs with huge
// candidate sets run for a long time on their single wave and must not start last
__global__ __launch_bounds__(256) void big_hist_kernel(const u8 *__restrict__ need_big, const u8 *__restrict__ cls,
                                                       u64 n, u8 want, u32 *__restrict__ class_count) {
  __shared__ u32 hist[33];
  if (threadIdx.x < 33) hist[threadIdx.x] = 0;
  __syncthreads();
  const u64 r = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r < n && need_big[r] == want) atomicAdd(&hist[cls[r]], 1u);
  __syncthreads();
  if (threadIdx.x < 33 && hist[threadIdx.x]) atomicAdd(&class_count[threadIdx.x], hist[threadIdx.x]);
}
__global__ void big_bases_kernel(u32 *class_count /*[33] in: counts, out: start of each class*/, u32 *total) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    u32 at = 0;
    for (int c = 32; c >= 0; --c) { const u32 k = class_count[c]; class_count[c] = at; at += k; }
    *total = at;
  }
}
__global__ __launch_bounds__(256) void big_scatter_kernel(const u8 *__restrict__ need_big, const u8 *__restrict__ cls,
                                                          u64 n, u8 want, u32 *__restrict__ class_cursor,
                                                          u32 *__restrict__ subset) {
  __shared__ u32 hist[33], base[33];
  if (threadIdx.x < 33) hist[threadIdx.x] = 0;
  __syncthreads();
  const u64 r = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool take = r < n && need_big[r] == want;
  u32 c = 0, rank = 0;
  if (take) { c = cls[r]; rank = atomicAdd(&hist[c], 1u); }
  __syncthreads();
  if (threadIdx.x < 33 && hist[threadIdx.x]) base[threadIdx.x] = atomicAdd(&class_cursor[threadIdx.x], hist[threadIdx.x]);
  __syncthreads();
  if (take) subset[base[c] + rank] = static_cast<u32>(r);
}

template <size_t... I> static const void *pe_kernel_at(int i, std::index_sequence<I...>) {
  static const void *const fns[] = {reinterpret_cast<const void *>(&map_pe_kernel<kPeForms[I].id()>)...};
  return fns[i];
}
const void *pe_kernel(PeForm f) {
  const int i = pe_form_index(f);
  return i < 0 ? nullptr : pe_kernel_at(i, std::make_index_sequence<kPeFormCount>{});
}
hipError_t launch_pe(PeForm f, const PeArgs &a, size_t lds, u32 grid, hipStream_t st) {
  if (grid == 0) return hipSuccess;
  const void *fn = pe_kernel(f);
  if (fn == nullptr) return hipErrorInvalidValue;
  void *args[] = {const_cast<PeArgs *>(&a)};
  return hipLaunchKernel(fn, dim3(grid), dim3(64), args, lds, st);
}

// ---- the long-end launch --------------------------------------------------------------------------------------
// pairs of this batch with an end of kLdsReadLen + 1 .. kMaxReadLen bases
__global__ __launch_bounds__(256) void collect_long_pairs_kernel(const u32 *__restrict__ lens1, const u32 *__restrict__ lens2, u64 n,
                                                                 u32 *__restrict__ list, u32 *__restrict__ count) {
  const u64 r = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const u32 a = lens1[r], b = lens2[r];
  if ((a > kLdsReadLen || b > kLdsReadLen) && a <= kMaxReadLen && b <= kMaxReadLen) list[atomicAdd(count, 1u)] = static_cast<u32>(r);
}
hipError_t launch_collect_long_pairs(const u32 *d_lens1, const u32 *d_lens2, u64 n, u32 *d_list, u32 *d_count, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(collect_long_pairs_kernel, dim3(static_cast<u32>((n + 255) / 256)), dim3(256), 0, st, d_lens1, d_lens2, n, d_list, d_count);
  return hipGetLastError();
}
size_t pe_long_q_words(u32 W, u32 WB) { return 8ull * W + 8ull * WB; }

hipError_t launch_collect_big(const u8 *need_big, const u8 *cls, u64 n, u8 want, u32 *class33, u32 *subset, u32 *count,
                              hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(class33, 0, 33 * sizeof(u32), st);
  if (e != hipSuccess) return e;
  const u32 blocks = static_cast<u32>((n + 255) / 256);
  hipLaunchKernelGGL(big_hist_kernel, dim3(blocks), dim3(256), 0, st, need_big, cls, n, want, class33);
  hipLaunchKernelGGL(big_bases_kernel, dim3(1), dim3(64), 0, st, class33, count);
  hipLaunchKernelGGL(big_scatter_kernel, dim3(blocks), dim3(256), 0, st, need_big, cls, n, want, class33, subset);
  return hipGetLastError();
}

}  // namespace abm
