// abismal_amd: the one description of each mapping kernel's dynamic LDS (one allocation per wave), shared by the kernels
// that carve it (se_carve in abm_seed.hpp, pe_carve in abm_pe_set.hpp), the launchers that ask for its bytes
// and plain host C++ (tests/cpp/lds_layout_check.cpp).  No HIP runtime calls.
//
// A layout function walks the regions in their order once.  Its position type P is either u32 -- byte offsets from the
// start of the allocation, for the host -- or unsigned char * -- the kernel's pointers, formed by the same chain of
// increments.  A region the form does not have is absent (lds_absent).
//
// Overlays (regions that borrow another's bytes while it is idle), each with its room:
//   tb       the traceback table, later the SAM / BAM line: window slots 1.., the cache and tb_extra (tb_room)
//   scratch  tier 2's radix histogram (256 counters) and the bitonic sort's block: from gwin THROUGH the cache, which
//            follows it directly in every form that has both (scratch_room; the long forms' two slots alone can be
//            smaller than the histogram)
//   hres     128 x u16 on lbest;  samp, and tier 1's scratch table (PeLds::tmp), on the cache;  the single-end fin on jpos
//   memo     the record-fed single-end forms' base-bucket facts: one 16-byte slot (lo2, d2, lo3, d3) per seed offset of a
//            call's specific pass, from the cache's first byte, written by the specific pass and read by the sensitive
//            pass of the SAME (strand, alphabet) call (seed_pass, abm_seed_bounds.hpp).  Those forms keep no candidate
//            cache, so the region is idle during their seed passes; kBoundsMemoSlots slots fit, 86 are ever used (the
//            longest read of a record-fed launch).  tb -- the traceback table, then the SAM / BAM line -- takes the
//            cache only after a read's last seed pass, and the next read's first specific pass writes before anything
//            reads: the memo never outlives its call.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef ABM_HD
#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define ABM_HD __host__ __device__
#else
#define ABM_HD
#endif
#endif

namespace abm {

using u8 = uint8_t;
using u16 = uint16_t;
using u32 = uint32_t;
using u64 = uint64_t;
using i16 = int16_t;

constexpr u32 kMaxBand = 61;     // src/AbismalAlign.hpp:108,133
constexpr u32 kSeCap = 50;       // src/abismal.cpp:448
constexpr u32 kPlaneBlock = 64;  // bases per bit-plane block
constexpr u32 kPosCacheBits = 8;
constexpr u32 kMaxJobs = 21;     // 64 lanes / narrowest band (3)
constexpr u32 kCacheBytes = 8u << kPosCacheBits;
constexpr u32 kLaneSlots = 64;   // lbest (int) and mark (u16): one per lane
constexpr u32 kStepSlots = 128;  // smark, sdelta (u32) and hres (u16): one per candidate of a seed-pass step
constexpr u32 kSampSlots = 512;  // samp (u32)
// LDS a launch of the pair kernels with SAM text takes beyond its usual size: both ends' CigarSink::fin
constexpr u32 kPeFinBytes = 2 * kSeCap * 4;
static_assert(kStepSlots * sizeof(u16) <= kLaneSlots * sizeof(int), "hres lies on lbest");
static_assert(kSampSlots * sizeof(u32) <= kCacheBytes, "samp lies on the window cache");
// the bounds memo (see above): slots of two u64 (lo | d << 32 per table); the longest read the window records serve
// (window_record_max_len of the five blocks build_wrec stops at) has kRecordMaxLen / 2 specific offsets
constexpr u32 kBoundsMemoSlotBytes = 16;
constexpr u32 kBoundsMemoSlots = kCacheBytes / kBoundsMemoSlotBytes;
constexpr u32 kRecordMaxLen = 172;
static_assert((kRecordMaxLen / 2) * kBoundsMemoSlotBytes <= kCacheBytes, "the bounds memo lies on the window cache");

enum : int { kWhole = 0, kSeed = 1, kMate = 2 };  // the pair kernels' phases (abm_kernels_pe.hip)

// ---- shape arithmetic ---------------------------------------------------------------------------------------------
// lanes of the widest band a read of max_len bases can ask for (src/AbismalAlign.hpp: 2 * max_diffs + 1, at most 61)
ABM_HD inline u32 se_band_width(u32 max_len, double valid_frac) {
  const int md = static_cast<i16>(valid_frac * max_len);
  const int bw = 2 * md + 1;
  return (bw > static_cast<int>(kMaxBand) || bw < 1) ? kMaxBand : static_cast<u32>(bw);
}
ABM_HD inline u32 se_window_words(u32 max_len, double valid_frac) {
  return ((max_len + se_band_width(max_len, valid_frac) + 15 + 15) >> 4) + 1;
}
ABM_HD inline u32 lds_mask_blocks(u32 max_len) { return (max_len + kPlaneBlock - 1) / kPlaneBlock; }
// the two overlays' rooms: bytes from window slot 1 to the end of the cache and its extra bytes; u32 words from gwin
// through the cache
ABM_HD inline size_t lds_table_room(u32 GW, u32 tb_extra) { return static_cast<size_t>(kMaxJobs - 1) * GW * 8 + kCacheBytes + tb_extra; }
ABM_HD inline u32 lds_scratch_words(u32 slots, u32 GW) { return 2 * (slots * GW + (1u << kPosCacheBits)); }
// bytes the traceback table ((L + band) x band) needs beyond the LDS it overlays; the kernels carve exactly this much extra
ABM_HD inline u32 tb_extra_bytes(u32 GW, u32 max_len, double valid_frac) {
  const u32 bw = se_band_width(max_len, valid_frac);
  const size_t need = static_cast<size_t>(max_len + bw) * bw, have = lds_table_room(GW, 0);
  return need > have ? static_cast<u32>((need - have + 7) & ~static_cast<size_t>(7)) : 0u;
}

// what a layout is a function of: all of it in the kernels' argument blocks (lds_shape, abm_kernels.hpp)
struct LdsShape { u32 W, WB, GW, max_len, ctmp_cap, tb_extra; };

// ---- positions ----------------------------------------------------------------------------------------------------
constexpr u32 kLdsAbsent = 0xFFFFFFFFu;
ABM_HD inline void lds_absent(u32 &p) { p = kLdsAbsent; }
ABM_HD inline void lds_absent(unsigned char *&p) { p = nullptr; }
// n elements of T at the cursor, which moves past them
template <class T, class P> ABM_HD inline P lds_take(P &at, u32 n) {
  const P r = at;
  at += static_cast<size_t>(n) * sizeof(T);
  return r;
}
template <class P> ABM_HD inline u32 lds_total(P base, P end) { return (static_cast<u32>(end - base) + 15u) & ~15u; }

// ---- single-end: map_se_kernel / map_se_long_kernel ------------------------------------------------------------------
template <class P> struct SeLds {
  P qpk, qbits, qmask, ctmp, jpos, jdf, gwin, pcache, lbest, smark, sdelta, mark;  // in this order
  P tb;            // overlay: the traceback table / the SAM line (absent: in global memory)
  u32 slots;       // window slots in gwin
  u32 tb_room, scratch_room, bytes;
};
template <class P> ABM_HD inline SeLds<P> se_lds_layout(P base, bool lng, const LdsShape &s) {
  SeLds<P> o;
  P at = base;
  o.slots = lng ? 2u : kMaxJobs;
  o.qpk = lds_take<u64>(at, 4 * s.W);
  o.qbits = lds_take<u64>(at, 4 * s.WB);
  o.qmask = lds_take<u64>(at, lng ? 0u : 4 * lds_mask_blocks(s.max_len) * 4);
  if (lng) lds_absent(o.ctmp);
  else o.ctmp = lds_take<u32>(at, (s.ctmp_cap + 1) & ~1u);
  o.jpos = lds_take<u32>(at, kSeCap);
  o.jdf = lds_take<u32>(at, kSeCap);
  o.gwin = lds_take<u64>(at, o.slots * s.GW);
  o.pcache = lds_take<u8>(at, kCacheBytes + (lng ? 0u : s.tb_extra));
  if (lng) { lds_absent(o.tb); o.tb_room = 0; }
  else { o.tb = o.gwin + static_cast<size_t>(s.GW) * 8; o.tb_room = static_cast<u32>(lds_table_room(s.GW, s.tb_extra)); }
  o.scratch_room = 4 * lds_scratch_words(o.slots, s.GW);
  o.lbest = lds_take<int>(at, kLaneSlots);
  o.smark = lds_take<u32>(at, kStepSlots);
  o.sdelta = lds_take<u32>(at, kStepSlots);
  o.mark = lds_take<u16>(at, kLaneSlots);
  o.bytes = lds_total(base, at);
  return o;
}

// ---- pairs: map_pe_kernel's whole / seed / mate forms and the long-end form (lng: phase kWhole, big) -------------------
// big: heap and lists in global memory (absent here); cap: entries of each when they are not; text: fin
template <class P> struct PeLdsAt {
  P qpk, qbits, qmask, gwin, pcache, ctmp, jpos, jdf, jidx, lbest, heap, lpos[2], ld[2], lsc[2], smark, sdelta, mark, fin;  // in this order
  P tb;
  u32 slots;
  u32 tb_room, scratch_room, bytes;
};
template <class P> ABM_HD inline PeLdsAt<P> pe_lds_layout(P base, int phase, bool lng, bool big, bool text, const LdsShape &s, u32 cap) {
  PeLdsAt<P> o;
  P at = base;
  const bool reads = !lng, bits = !lng && phase != kMate, align = phase != kSeed;
  o.slots = !align ? 0u : (lng ? 2u : kMaxJobs);
  if (reads) o.qpk = lds_take<u64>(at, 8 * s.W); else lds_absent(o.qpk);
  if (bits) {
    o.qbits = lds_take<u64>(at, 8 * s.WB);
    o.qmask = lds_take<u64>(at, 8 * lds_mask_blocks(s.max_len) * 4);
  }
  else { lds_absent(o.qbits); lds_absent(o.qmask); }
  if (align) o.gwin = lds_take<u64>(at, o.slots * s.GW); else lds_absent(o.gwin);
  o.pcache = lds_take<u8>(at, kCacheBytes + ((align && !lng) ? s.tb_extra : 0u));
  if (align && !lng) {
    o.tb = o.gwin + static_cast<size_t>(s.GW) * 8; o.tb_room = static_cast<u32>(lds_table_room(s.GW, s.tb_extra));
    o.ctmp = lds_take<u32>(at, s.ctmp_cap);
  }
  else { lds_absent(o.tb); o.tb_room = 0; lds_absent(o.ctmp); }
  o.scratch_room = align ? 4 * lds_scratch_words(o.slots, s.GW) : 0u;
  if (align) {
    o.jpos = lds_take<u32>(at, kSeCap);
    o.jdf = lds_take<u32>(at, kSeCap);
    o.jidx = lds_take<u32>(at, kSeCap);
  }
  else { lds_absent(o.jpos); lds_absent(o.jdf); lds_absent(o.jidx); }
  o.lbest = lds_take<int>(at, kLaneSlots);
  if (big) { lds_absent(o.heap); lds_absent(o.lpos[0]); lds_absent(o.lpos[1]); lds_absent(o.ld[0]); lds_absent(o.ld[1]); lds_absent(o.lsc[0]); lds_absent(o.lsc[1]); }
  else if (phase == kSeed) {  // one list at a time (positions, diffs)
    o.heap = lds_take<u32>(at, cap);
    o.lpos[0] = o.lpos[1] = lds_take<u32>(at, cap);
    o.ld[0] = o.ld[1] = lds_take<i16>(at, cap + (cap & 1u));
    lds_absent(o.lsc[0]); lds_absent(o.lsc[1]);
  }
  else {
    o.heap = lds_take<u32>(at, cap);
    o.lpos[0] = lds_take<u32>(at, cap); o.lpos[1] = lds_take<u32>(at, cap);
    o.ld[0] = lds_take<i16>(at, cap); o.ld[1] = lds_take<i16>(at, cap);
    o.lsc[0] = lds_take<i16>(at, cap); o.lsc[1] = lds_take<i16>(at, cap);
  }
  if (phase != kMate) { o.smark = lds_take<u32>(at, kStepSlots); o.sdelta = lds_take<u32>(at, kStepSlots); }  // (no seed passes: no segment marks)
  else { lds_absent(o.smark); lds_absent(o.sdelta); }
  o.mark = lds_take<u16>(at, kLaneSlots);
  if (text) o.fin = lds_take<u8>(at, kPeFinBytes); else lds_absent(o.fin);
  o.bytes = lds_total(base, at);
  return o;
}

}  // namespace abm
