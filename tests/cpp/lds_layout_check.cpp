// The LDS layouts of abm_lds_layout.hpp on the CPU (built with sanitizers by tests/test_cabi_and_host.py): every form over
// a grid of shapes against the size formulas the launchers had before the layouts existed -- frozen here as the
// reference -- and against the properties the kernels rely on: regions in their order, none overlapping, each aligned to
// its element type, every overlay inside its room.
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../abismal_amd/csrc/abm_lds_layout.hpp"

using namespace abm;

// ---- the frozen formulas ---------------------------------------------------------------------------------------------
namespace frozen {
constexpr u32 kMaxBand = 61, kSeCap = 50, kPlaneBlock = 64, kPosCacheBits = 8, kMaxJobs = 21, kPeFinBytes = 400;
u32 se_window_words(u32 max_len, double valid_frac) {
  const int md = static_cast<i16>(valid_frac * max_len);
  int bw = 2 * md + 1;
  if (bw > static_cast<int>(kMaxBand) || bw < 1) bw = kMaxBand;
  return ((max_len + bw + 15 + 15) >> 4) + 1;
}
u32 band(u32 max_len, double valid_frac) {
  const int md = static_cast<i16>(valid_frac * max_len);
  int bw = 2 * md + 1;
  if (bw > static_cast<int>(kMaxBand) || bw < 0) bw = kMaxBand;
  if (bw < 1) bw = 1;
  return static_cast<u32>(bw);
}
u32 tb_extra_bytes(u32 GW, u32 max_len, double valid_frac) {
  const u32 bw = band(max_len, valid_frac);
  const size_t need = static_cast<size_t>(max_len + bw) * bw;
  const size_t have = static_cast<size_t>(kMaxJobs - 1) * GW * 8 + (static_cast<size_t>(8) << kPosCacheBits);
  return need > have ? static_cast<u32>((need - have + 7) & ~static_cast<size_t>(7)) : 0u;
}
size_t se_lds_bytes(u32 W, u32 WB, u32 cig_stride, u32 max_len, double valid_frac) {
  const u32 GW = se_window_words(max_len, valid_frac);
  const u32 MB = (max_len + kPlaneBlock - 1) / kPlaneBlock;
  size_t b = static_cast<size_t>(4) * W * 8 + static_cast<size_t>(4) * WB * 8 + static_cast<size_t>(4) * MB * 4 * 8 +
             (static_cast<size_t>(8) << kPosCacheBits) +
             static_cast<size_t>(kMaxJobs) * GW * 8 + static_cast<size_t>((cig_stride + 1) & ~1u) * 4 +
             2 * kSeCap * 4 + 64 * 4 + 2 * 128 * 4 + 64 * 2;
  b += tb_extra_bytes(GW, max_len, valid_frac);
  return (b + 15) & ~static_cast<size_t>(15);
}
size_t se_long_lds_bytes(u32 W, u32 WB, u32 GW) {
  const size_t b = static_cast<size_t>(4) * W * 8 + static_cast<size_t>(4) * WB * 8 + 2 * kSeCap * 4 + static_cast<size_t>(2) * GW * 8 +
                   (static_cast<size_t>(8) << kPosCacheBits) + 64 * 4 + 2 * 128 * 4 + 64 * 2;
  return (b + 15) & ~static_cast<size_t>(15);
}
size_t sam_line_room(u32 GW, u32 tb_extra) {
  return static_cast<size_t>(kMaxJobs - 1) * GW * 8 + (static_cast<size_t>(8) << kPosCacheBits) + tb_extra;
}
size_t pe_lds_bytes(u32 W, u32 WB, u32 GW, u32 cig_stride, u32 max_len, double valid_frac, u32 cap, bool big) {
  const u32 MB = (max_len + kPlaneBlock - 1) / kPlaneBlock;
  size_t b = static_cast<size_t>(8) * W * 8 + static_cast<size_t>(8) * WB * 8 + static_cast<size_t>(8) * MB * 4 * 8 +
             (static_cast<size_t>(8) << kPosCacheBits) + static_cast<size_t>(kMaxJobs) * GW * 8 +
             static_cast<size_t>(cig_stride) * 4 + 3 * kSeCap * 4 + 64 * 4 + 2 * 128 * 4 + 64 * 2;
  if (!big) b += static_cast<size_t>(cap) * (4 + 2 * 4 + 4 * 2);
  b += tb_extra_bytes(GW, max_len, valid_frac);
  return (b + 15) & ~static_cast<size_t>(15);
}
size_t pe_long_lds_bytes(u32 GW) {
  const size_t b = static_cast<size_t>(2) * GW * 8 + (static_cast<size_t>(8) << kPosCacheBits) + 3 * kSeCap * 4 + 64 * 4 + 2 * 128 * 4 + 64 * 2;
  return (b + 15) & ~static_cast<size_t>(15);
}
size_t pe_seed_lds_bytes(u32 W, u32 WB, u32 max_len, u32 cap) {
  const u32 MB = (max_len + kPlaneBlock - 1) / kPlaneBlock;
  const size_t b = static_cast<size_t>(8) * W * 8 + static_cast<size_t>(8) * WB * 8 + static_cast<size_t>(8) * MB * 4 * 8 +
                   (static_cast<size_t>(8) << kPosCacheBits) + 64 * 4 + static_cast<size_t>(cap) * 4 /* heap */ +
                   static_cast<size_t>(cap) * 4 + static_cast<size_t>(cap + (cap & 1u)) * 2 /* one list */ + 2 * 128 * 4 + 64 * 2;
  return (b + 15) & ~static_cast<size_t>(15);
}
size_t pe_mate_lds_bytes(u32 W, u32 GW, u32 cig_stride, u32 max_len, double valid_frac, u32 cap, bool big) {
  size_t b = static_cast<size_t>(8) * W * 8 + (static_cast<size_t>(8) << kPosCacheBits) + static_cast<size_t>(kMaxJobs) * GW * 8 +
             static_cast<size_t>(cig_stride) * 4 + 3 * kSeCap * 4 + 64 * 4 + 64 * 2;
  if (!big) b += static_cast<size_t>(cap) * (4 + 2 * 4 + 4 * 2);
  b += tb_extra_bytes(GW, max_len, valid_frac);
  return (b + 15) & ~static_cast<size_t>(15);
}
}  // namespace frozen

// ---- the checks --------------------------------------------------------------------------------------------------------
static int n_wrong = 0, n_points = 0;
static std::string where;
#define REQUIRE(cond)                                                              \
  do {                                                                             \
    if (!(cond)) { ++n_wrong; if (n_wrong <= 40) printf("WRONG %s: %s\n", where.c_str(), #cond); } \
  } while (0)

struct Region { const char *name; u32 at, bytes, align; };
// the regions a form has, in the documented order: each begins at or after its predecessor's end, aligned, inside `total`
static void check_regions(const std::vector<Region> &rs, u32 total) {
  u32 end = 0;
  for (const Region &r : rs) {
    if (r.at == kLdsAbsent) continue;
    if (r.at < end || r.at % r.align != 0 || r.at + r.bytes > total) {
      ++n_wrong;
      if (n_wrong <= 40) printf("WRONG %s: region %s at %u (+%u), after %u, inside %u\n", where.c_str(), r.name, r.at, r.bytes, end, total);
    }
    end = r.at + r.bytes;
  }
  REQUIRE(total % 16 == 0 && end <= total && total < end + 16);
}
// an overlay [at, at + bytes) inside the room [room_at, room_at + room)
static bool inside(u32 at, size_t bytes, u32 room_at, size_t room) { return at != kLdsAbsent && room_at != kLdsAbsent && at >= room_at && at + bytes <= room_at + room; }

static u32 words_for(u32 L) { return std::max(1u, (L + 15) / 16); }
static u32 bitwords_for(u32 L) { return (L + 63) / 64 + 1; }

static void check_se(u32 L, double frac) {
  const u32 W = words_for(L), WB = bitwords_for(L), GW = se_window_words(L, frac), cap2 = (L + 2 + 1) & ~1u;
  REQUIRE(GW == frozen::se_window_words(L, frac));
  const u32 extra = tb_extra_bytes(GW, L, frac), bw = se_band_width(L, frac);
  REQUIRE(extra == frozen::tb_extra_bytes(GW, L, frac) && bw == frozen::band(L, frac));
  const LdsShape s{W, WB, GW, L, L + 2, extra};
  const SeLds<u32> o = se_lds_layout<u32>(0, false, s);
  REQUIRE(o.bytes == frozen::se_lds_bytes(W, WB, s.ctmp_cap, L, frac));
  REQUIRE(o.tb_room == frozen::sam_line_room(GW, extra) && lds_table_room(GW, extra) == o.tb_room);
  const u32 MB = (L + 63) / 64;
  check_regions({{"qpk", o.qpk, 4 * W * 8, 8}, {"qbits", o.qbits, 4 * WB * 8, 8}, {"qmask", o.qmask, 4 * MB * 4 * 8, 8},
                 {"ctmp", o.ctmp, cap2 * 4, 4}, {"jpos", o.jpos, kSeCap * 4, 4}, {"jdf", o.jdf, kSeCap * 4, 4},
                 {"gwin", o.gwin, kMaxJobs * GW * 8, 8}, {"pcache", o.pcache, kCacheBytes + extra, 8}, {"lbest", o.lbest, 64 * 4, 4},
                 {"smark", o.smark, 128 * 4, 4}, {"sdelta", o.sdelta, 128 * 4, 4}, {"mark", o.mark, 64 * 2, 2}}, o.bytes);
  REQUIRE(o.qpk == 0 && o.slots == kMaxJobs);
  // overlays: the table, within window slots 1.. and the cache with its extra bytes; the scratch room, gwin through the cache
  REQUIRE(static_cast<size_t>(L + bw) * bw <= o.tb_room);
  REQUIRE(o.tb == o.gwin + GW * 8 && o.tb + o.tb_room == o.pcache + kCacheBytes + extra);
  REQUIRE(o.pcache == o.gwin + o.slots * GW * 8 && o.gwin + o.scratch_room == o.pcache + kCacheBytes);
}

static void check_se_long(u32 L, double frac) {
  const u32 W = words_for(L), WB = bitwords_for(L), GW = se_window_words(L, frac);
  REQUIRE(GW == frozen::se_window_words(L, frac));
  const LdsShape s{W, WB, GW, L, L + 2, 0};
  const SeLds<u32> o = se_lds_layout<u32>(0, true, s);
  REQUIRE(o.bytes == frozen::se_long_lds_bytes(W, WB, GW));
  check_regions({{"qpk", o.qpk, 4 * W * 8, 8}, {"qbits", o.qbits, 4 * WB * 8, 8}, {"qmask", o.qmask, 0, 8}, {"jpos", o.jpos, kSeCap * 4, 4},
                 {"jdf", o.jdf, kSeCap * 4, 4}, {"gwin", o.gwin, 2 * GW * 8, 8}, {"pcache", o.pcache, kCacheBytes, 8},
                 {"lbest", o.lbest, 64 * 4, 4}, {"smark", o.smark, 128 * 4, 4}, {"sdelta", o.sdelta, 128 * 4, 4}, {"mark", o.mark, 64 * 2, 2}}, o.bytes);
  REQUIRE(o.ctmp == kLdsAbsent && o.tb == kLdsAbsent && o.tb_room == 0 && o.slots == 2);
  REQUIRE(o.pcache == o.gwin + 2 * GW * 8 && o.gwin + o.scratch_room == o.pcache + kCacheBytes);
}

// phase kWhole / kSeed / kMate, or the long-end form (lng)
static void check_pe(u32 L, double frac, int phase, bool lng, bool big, bool text, u32 cap) {
  const u32 W = words_for(L), WB = bitwords_for(L), GW = se_window_words(L, frac);
  const u32 extra = lng ? 0u : tb_extra_bytes(GW, L, frac), bw = se_band_width(L, frac), MB = (L + 63) / 64;
  const LdsShape s{W, WB, GW, L, L + 2, extra};
  const PeLdsAt<u32> o = pe_lds_layout<u32>(0, phase, lng, big, text, s, cap);
  const size_t fin = text ? frozen::kPeFinBytes : 0;
  if (lng) REQUIRE(o.bytes == frozen::pe_long_lds_bytes(GW));
  else if (phase == kSeed) REQUIRE(o.bytes == frozen::pe_seed_lds_bytes(W, WB, L, cap));
  else if (phase == kMate) REQUIRE(o.bytes == frozen::pe_mate_lds_bytes(W, GW, s.ctmp_cap, L, frac, cap, big) + fin);
  else REQUIRE(o.bytes == frozen::pe_lds_bytes(W, WB, GW, s.ctmp_cap, L, frac, cap, big) + fin);
  const bool align = phase != kSeed, table = align && !lng;
  const u32 slots = !align ? 0u : (lng ? 2u : kMaxJobs), list2 = cap + (cap & 1u);
  std::vector<Region> rs = {{"qpk", o.qpk, 8 * W * 8, 8}, {"qbits", o.qbits, 8 * WB * 8, 8}, {"qmask", o.qmask, 8 * MB * 4 * 8, 8},
                            {"gwin", o.gwin, slots * GW * 8, 8}, {"pcache", o.pcache, kCacheBytes + (table ? extra : 0u), 8},
                            {"ctmp", o.ctmp, s.ctmp_cap * 4, 4}, {"jpos", o.jpos, kSeCap * 4, 4}, {"jdf", o.jdf, kSeCap * 4, 4},
                            {"jidx", o.jidx, kSeCap * 4, 4}, {"lbest", o.lbest, 64 * 4, 4}, {"heap", o.heap, cap * 4, 4}};
  if (phase == kSeed) { rs.push_back({"lpos", o.lpos[0], cap * 4, 4}); rs.push_back({"ld", o.ld[0], list2 * 2, 2}); }
  else {
    rs.push_back({"lpos0", o.lpos[0], cap * 4, 4}); rs.push_back({"lpos1", o.lpos[1], cap * 4, 4});
    rs.push_back({"ld0", o.ld[0], cap * 2, 2}); rs.push_back({"ld1", o.ld[1], cap * 2, 2});
    rs.push_back({"lsc0", o.lsc[0], cap * 2, 2}); rs.push_back({"lsc1", o.lsc[1], cap * 2, 2});
  }
  rs.push_back({"smark", o.smark, 128 * 4, 4}); rs.push_back({"sdelta", o.sdelta, 128 * 4, 4});
  rs.push_back({"mark", o.mark, 64 * 2, 2}); rs.push_back({"fin", o.fin, frozen::kPeFinBytes, 4});
  check_regions(rs, o.bytes);
  // which regions each form has
  REQUIRE((o.qpk != kLdsAbsent) == !lng && (o.qbits != kLdsAbsent) == (!lng && phase != kMate) && (o.qmask != kLdsAbsent) == (o.qbits != kLdsAbsent));
  REQUIRE((o.gwin != kLdsAbsent) == align && (o.jpos != kLdsAbsent) == align && (o.jdf != kLdsAbsent) == align && (o.jidx != kLdsAbsent) == align);
  REQUIRE((o.ctmp != kLdsAbsent) == table && (o.tb != kLdsAbsent) == table && o.pcache != kLdsAbsent && o.lbest != kLdsAbsent && o.mark != kLdsAbsent);
  REQUIRE((o.heap != kLdsAbsent) == !big && (o.lpos[0] != kLdsAbsent) == !big && (o.ld[1] != kLdsAbsent) == !big);
  REQUIRE((o.lsc[0] != kLdsAbsent) == (!big && phase != kSeed) && (o.lsc[1] != kLdsAbsent) == (!big && phase != kSeed));
  REQUIRE((o.smark != kLdsAbsent) == (phase != kMate) && (o.sdelta != kLdsAbsent) == (phase != kMate) && (o.fin != kLdsAbsent) == text);
  REQUIRE(o.slots == slots);
  if (phase == kSeed) REQUIRE(o.lpos[1] == o.lpos[0] && o.ld[1] == o.ld[0]);
  // overlays
  if (table) {
    REQUIRE(o.tb_room == frozen::sam_line_room(GW, extra));
    REQUIRE(static_cast<size_t>(L + bw) * bw <= o.tb_room);
    REQUIRE(o.tb == o.gwin + GW * 8 && o.tb + o.tb_room == o.pcache + kCacheBytes + extra);
  }
  else REQUIRE(o.tb_room == 0);
  if (align) {  // the scratch room: gwin through the cache, which follows it directly; tier 2's histogram is 256 counters
    REQUIRE(o.pcache == o.gwin + slots * GW * 8 && o.gwin + o.scratch_room == o.pcache + kCacheBytes);
    REQUIRE(o.scratch_room == 4 * lds_scratch_words(slots, GW));
    if (big) REQUIRE(o.scratch_room >= 256 * 4);
  }
  else REQUIRE(o.scratch_room == 0);
  REQUIRE(inside(o.pcache, kSampSlots * 4, o.pcache, kCacheBytes));          // samp
  if (!big) REQUIRE(inside(o.pcache, static_cast<size_t>(cap) * 4, o.pcache, kCacheBytes));  // tier 1's scratch table
}

int main() {
  const u32 lens[] = {44, 45, 46, 47, 64, 65, 100, 128, 129, 150, 172, 173, 250, 448, 449, 1024}, long_lens[] = {1025, 32766};
  const double fracs[] = {0.0, 0.1, 0.25, 1.0};
  const u32 caps[] = {32, 128, 256};
  char buf[160];
  for (const double frac : fracs) {
    for (const u32 L : lens) {
      snprintf(buf, sizeof buf, "single-end L=%u frac=%g", L, frac); where = buf; ++n_points;
      check_se(L, frac);
      for (const u32 cap : caps)
        for (int big = 0; big < 2; ++big)
          for (int text = 0; text < 2; ++text) {
            snprintf(buf, sizeof buf, "pairs L=%u frac=%g cap=%u big=%d text=%d", L, frac, cap, big, text); where = buf; n_points += 2;
            check_pe(L, frac, kWhole, false, big, text, cap);
            check_pe(L, frac, kMate, false, big, text, cap);
            if (!big && !text) { ++n_points; check_pe(L, frac, kSeed, false, false, false, cap); }  // (the seed form: lists in LDS, no text)
          }
    }
    for (const u32 L : long_lens) {
      snprintf(buf, sizeof buf, "long L=%u frac=%g", L, frac); where = buf; n_points += 2;
      check_se_long(L, frac);
      check_pe(L, frac, kWhole, true, true, false, 32u << 10);
    }
  }
  printf("%d points, %d wrong\n", n_points, n_wrong);
  return n_wrong ? 1 : 0;
}
