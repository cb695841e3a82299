// abismal_amd: the one description of each build of the mapping kernels -- which builds exist (the tables), which one a
// launch takes (the selectors), and whose occupancy sizes its grid (the donors).  Shared by the kernels (their one
// template argument is a form's id), the launchers and occupancy queries (abm_kernels.hip, abm_kernels_pe.hip), the
// launch layer (abm_api.hip) and plain host C++ (tests/cpp/kernel_form_check.cpp).  No HIP runtime calls.
#pragma once
#include "abm_lds_layout.hpp"

// waves per SIMD the builds are compiled for (launch bounds): single-end 5 (96 VGPRs per lane, 20 waves per CU), the
// pair kernels 4 -- and 3 for launches with much LDS (pe_select) -- the seed and mate kernels what each needs without
// scratch (profiles/r05_pe_split_resources.log)
#ifndef ABM_SE_WAVES_PER_SIMD
#define ABM_SE_WAVES_PER_SIMD 5
#endif
#ifndef ABM_PE_WAVES_PER_SIMD
#define ABM_PE_WAVES_PER_SIMD 4
#endif
#ifndef ABM_PE_SEED_WPS
#define ABM_PE_SEED_WPS 4
#endif
#ifndef ABM_PE_MATE_WPS
#define ABM_PE_MATE_WPS 4
#endif

namespace abm {

constexpr int kSeWps = ABM_SE_WAVES_PER_SIMD, kPeWps = ABM_PE_WAVES_PER_SIMD, kPeSeedWps = ABM_PE_SEED_WPS, kPeMateWps = ABM_PE_MATE_WPS;

// ---- forms ----------------------------------------------------------------------------------------------------------
// phase: kWhole / kSeed / kMate;  big: lists and heap in global memory (tier 2);  is_long: the long-end launch;
// timed: the diagnostic build (cycle stamps, seed tallies);  coop: lanes share a candidate's window on the bit planes;
// rec: ... or on the window records;  text: the pair's records are written as well;  bam: as BAM pieces;  wps: launch bound
struct PeForm {
  int phase;
  bool big, is_long, timed, coop, rec, text, bam;
  int wps;
  constexpr bool valid() const {
    return (!bam || text) &&                                               // BAM pieces: a build with the pair's records
           (!rec || (coop && phase != kMate)) &&                           // window records feed the cooperative filter of the seed passes
           (!is_long || (big && !coop && !timed && phase == kWhole)) &&    // the long-end launch: tier 2's lists, nibble filter, no stamps
           (phase != kSeed || !big) &&                                     // the seed kernel keeps its lists in LDS (and its staging area)
           (phase != kMate || !coop) &&                                    // the mate kernels fetch no candidate windows
           (!text || (!is_long && !timed && phase != kSeed));              // text: the launches that finish pairs in LDS
  }
  constexpr u32 id() const {
    return static_cast<u32>(phase) | (big ? 4u : 0u) | (is_long ? 8u : 0u) | (timed ? 16u : 0u) | (coop ? 32u : 0u) | (rec ? 64u : 0u) |
           (text ? 128u : 0u) | (bam ? 256u : 0u) | (static_cast<u32>(wps) << 9);
  }
};
constexpr PeForm pe_form_of(u32 id) {
  return PeForm{static_cast<int>(id & 3u), (id & 4u) != 0, (id & 8u) != 0, (id & 16u) != 0, (id & 32u) != 0, (id & 64u) != 0,
                (id & 128u) != 0, (id & 256u) != 0, static_cast<int>((id >> 9) & 15u)};
}
// single-end.  bam: the read's record as a BAM piece (SAM text needs no build of its own: SeArgs::sam_tail)
constexpr u32 kSeFormBit = 1u << 31;  // (in an id: tells the families apart where both are listed, abm_ctx_last_forms)
struct SeForm {
  bool timed, coop, rec, bam, is_long;
  int wps;
  constexpr bool valid() const {
    return (!rec || coop) &&                                   // window records feed the cooperative filter
           (!bam || !timed) &&                                 // the untimed builds once more, writing BAM pieces
           (!is_long || (!timed && !coop && !rec && !bam));    // the long-read launch: nibble filter, no stamps, no records written
  }
  constexpr u32 id() const {
    return kSeFormBit | (timed ? 1u : 0u) | (coop ? 2u : 0u) | (rec ? 4u : 0u) | (bam ? 8u : 0u) | (is_long ? 16u : 0u) | (static_cast<u32>(wps) << 9);
  }
};
constexpr SeForm se_form_of(u32 id) {
  return SeForm{(id & 1u) != 0, (id & 2u) != 0, (id & 4u) != 0, (id & 8u) != 0, (id & 16u) != 0, static_cast<int>((id >> 9) & 15u)};
}

// ---- the builds that exist --------------------------------------------------------------------------------------------
// These tables are the only cause of instantiation (pe_kernel / se_kernel walk them).
// (Built with ABM_PE_WAVES_PER_SIMD=3 the 3-wave rows repeat their neighbours: take them out for that experiment.)
inline constexpr PeForm kPeForms[] = {
    // phase  big    long   timed  coop   rec    text   bam    wps
    // the whole-pair kernel: tier 1 unsplit (LDS) and tier 2, on the bit planes (3 waves per SIMD, the usual ones, stamped) ...
    {kWhole, false, false, false, true, false, false, false, 3},
    {kWhole, false, false, false, true, false, false, false, kPeWps},
    {kWhole, false, false, true, true, false, false, false, kPeWps},
    {kWhole, true, false, false, true, false, false, false, 3},
    {kWhole, true, false, false, true, false, false, false, kPeWps},
    {kWhole, true, false, true, true, false, false, false, kPeWps},
    // ... on the nibble array ...
    {kWhole, false, false, false, false, false, false, false, kPeWps},
    {kWhole, false, false, true, false, false, false, false, kPeWps},
    {kWhole, true, false, false, false, false, false, false, kPeWps},
    {kWhole, true, false, true, false, false, false, false, kPeWps},
    // ... tier 2 on the window records ...
    {kWhole, true, false, false, true, true, false, false, 3},
    {kWhole, true, false, false, true, true, false, false, kPeWps},
    {kWhole, true, false, true, true, true, false, false, kPeWps},
    // ... and writing the pair's records: SAM text, BAM pieces
    {kWhole, false, false, false, true, false, true, false, kPeWps},
    {kWhole, true, false, false, true, false, true, false, kPeWps},
    {kWhole, false, false, false, true, false, true, true, kPeWps},
    {kWhole, true, false, false, true, false, true, true, kPeWps},
    // the long-end launch
    {kWhole, true, true, false, false, false, false, false, 1},
    // the seed kernel: records, planes, nibbles
    {kSeed, false, false, false, true, true, false, false, kPeSeedWps},
    {kSeed, false, false, true, true, true, false, false, kPeSeedWps},
    {kSeed, false, false, false, true, false, false, false, kPeSeedWps},
    {kSeed, false, false, true, true, false, false, false, kPeSeedWps},
    {kSeed, false, false, false, false, false, false, false, kPeSeedWps},
    {kSeed, false, false, true, false, false, false, false, kPeSeedWps},
    // the mate kernels: small lists (LDS) and lists in global memory; plain, stamped, SAM text, BAM pieces
    {kMate, false, false, false, false, false, false, false, kPeMateWps},
    {kMate, false, false, true, false, false, false, false, kPeMateWps},
    {kMate, false, false, false, false, false, true, false, kPeMateWps},
    {kMate, false, false, false, false, false, true, true, kPeMateWps},
    {kMate, true, false, false, false, false, false, false, kPeMateWps},
    {kMate, true, false, true, false, false, false, false, kPeMateWps},
    {kMate, true, false, false, false, false, true, false, kPeMateWps},
    {kMate, true, false, false, false, false, true, true, kPeMateWps},
};
inline constexpr SeForm kSeForms[] = {
    // timed coop   rec    bam    long   wps
    {false, true, true, false, false, kSeWps},    // window records: plain, stamped, BAM pieces
    {true, true, true, false, false, kSeWps},
    {false, true, true, true, false, kSeWps},
    {false, true, false, false, false, kSeWps},   // bit planes
    {true, true, false, false, false, kSeWps},
    {false, true, false, true, false, kSeWps},
    {false, false, false, false, false, kSeWps},  // nibble array
    {true, false, false, false, false, kSeWps},
    {false, false, false, true, false, kSeWps},
    {false, false, false, false, true, 1},        // the long-read launch
};
constexpr int kPeFormCount = sizeof(kPeForms) / sizeof(kPeForms[0]), kSeFormCount = sizeof(kSeForms) / sizeof(kSeForms[0]);

// where a form stands in its table, -1: no such build
constexpr int pe_form_index(PeForm f) {
  for (int i = 0; i < kPeFormCount; ++i)
    if (kPeForms[i].id() == f.id()) return i;
  return -1;
}
constexpr int se_form_index(SeForm f) {
  for (int i = 0; i < kSeFormCount; ++i)
    if (kSeForms[i].id() == f.id()) return i;
  return -1;
}
template <class F, int N> constexpr bool forms_valid_and_distinct(const F (&t)[N]) {
  for (int i = 0; i < N; ++i) {
    if (!t[i].valid() || t[i].wps < 1 || t[i].wps > 15) return false;
    for (int j = 0; j < i; ++j)
      if (t[i].id() == t[j].id()) return false;
  }
  return true;
}
static_assert(kPeFormCount == 32 && forms_valid_and_distinct(kPeForms), "the pair kernels' builds: valid, distinct");
static_assert(kSeFormCount == 10 && forms_valid_and_distinct(kSeForms), "the single-end builds: valid, distinct");

// ---- which build a launch takes -------------------------------------------------------------------------------------
// What the selectors are told.  G: lanes sharing one candidate window (0: one lane per window, the nibble array);
// rec_fit: the index has window records and they serve the launch's longest read (records_fit, abm_api.hip);
// timed: the stamps are on;  text: the launch has slots for records;  bam: ... as BAM pieces;  lds: bytes per wave;
// wps_override: 3 or 4 from the ABM_PE_WPS / ABM_PE_WPS2 experiment switches, else 0
enum class PeRole { kTier1, kTier2, kSeed, kMateSmall, kMateBig, kLong };  // tier 1 unsplit, tier 2, the split's three, long ends
struct PeFacts {
  PeRole role;
  u32 G;
  bool rec_fit, timed, text, bam;
  size_t lds;
  int wps_override;
};
struct PeChoice { bool ok; PeForm form; };
enum class SeRole { kMain, kLong };
struct SeFacts {
  SeRole role;
  u32 G;
  bool rec_fit, timed, text, bam;
};
struct SeChoice { bool ok; SeForm form; };

// The record-fed filter: single-end launches at two or four lanes per window, the pair kernels at four
constexpr bool records_serve(bool pairs, u32 G, bool rec_fit) { return rec_fit && (G == 4 || (!pairs && G == 2)); }
// Three waves per SIMD instead of the usual four: a launch on the planes whose LDS lets fewer than 14 waves onto a CU
// anyway (LDS of a CU: 160 KB on gfx950) takes the build with the larger register budget; the stamped builds and those
// with text come at four only
constexpr bool pe_three_waves(const PeFacts &k) {
  if (k.timed || k.G == 0 || k.text) return false;
  if (k.wps_override == 3 || k.wps_override == 4) return k.wps_override == 3;
  return k.lds != 0 && (160u * 1024u) / k.lds <= 13u;
}

// what of a role's form its LDS layout depends on (pe_lds_bytes); the rest is pe_select's
constexpr PeForm pe_role_form(PeRole role, bool text) {
  switch (role) {
    case PeRole::kTier1: return PeForm{kWhole, false, false, false, false, false, text, false, kPeWps};
    case PeRole::kTier2: return PeForm{kWhole, true, false, false, false, false, text, false, kPeWps};
    case PeRole::kSeed: return PeForm{kSeed, false, false, false, false, false, false, false, kPeSeedWps};
    case PeRole::kMateSmall: return PeForm{kMate, false, false, false, false, false, text, false, kPeMateWps};
    case PeRole::kMateBig: return PeForm{kMate, true, false, false, false, false, text, false, kPeMateWps};
    default: return PeForm{kWhole, true, true, false, false, false, false, false, 1};
  }
}
constexpr PeChoice pe_select(const PeFacts &k) {
  // records are written by the launches that finish pairs, on the bit planes only, never by a stamped build; the seed
  // kernel and the long-end launch (which has one build) write none and are not asked
  const bool finishes = k.role != PeRole::kSeed && k.role != PeRole::kLong;
  const bool text = finishes && k.text;
  PeForm f = pe_role_form(k.role, text);
  if (text && (k.timed || k.G == 0)) return PeChoice{false, f};
  if (k.role == PeRole::kLong) return PeChoice{true, f};
  f.timed = k.timed;
  f.bam = text && k.bam;
  if (f.phase != kMate) {  // (the filter)
    f.coop = k.G != 0;
    // (the planes serve an end the records would, with the same candidates: tier 1 unsplit and the builds with text stay on them)
    f.rec = !text && (f.big || f.phase == kSeed) && records_serve(true, k.G, k.rec_fit);
  }
  if (f.phase == kWhole && pe_three_waves(k)) f.wps = 3;
  return PeChoice{pe_form_index(f) >= 0, f};
}
constexpr SeChoice se_select(const SeFacts &k) {
  if (k.role == SeRole::kLong) return SeChoice{true, SeForm{false, false, false, false, true, 1}};
  SeForm f{k.timed, k.G != 0, records_serve(false, k.G, k.rec_fit), k.text && k.bam, false, kSeWps};
  return SeChoice{se_form_index(f) >= 0, f};  // (no stamped build writes BAM pieces)
}

// ---- grid donors ----------------------------------------------------------------------------------------------------
// A launch's persistent grid, and with it its per-wave workspaces, is sized by the occupancy of its form's DONOR, not
// its own: the plain build on the planes of its phase, list placement and waves per SIMD (the seed kernel's: of its
// own filter, without records), capped per CU.  This is a frozen fact of the code these tables replaced, kept so that no
// grid and no workspace changes size; letting each build size its own grid changes speed and memory and is another change.
constexpr PeForm pe_donor(PeForm f) {
  if (f.is_long) return f;
  f.timed = f.rec = f.text = f.bam = false;
  if (f.phase == kWhole) f.coop = true;
  return f;
}
constexpr SeForm se_donor(SeForm f) { return f.is_long ? f : SeForm{false, true, false, false, false, f.wps}; }
constexpr int kNoWaveCap = 1 << 20;
// waves per CU at most: the long-end launch one (each has megabytes of workspace in global memory), the long-read launch
// four, the single-end kernel what its launch bound stands for (more waves only spill: DESIGN.md)
constexpr int pe_waves_per_cu_cap(PeForm f) { return f.is_long ? 1 : kNoWaveCap; }
constexpr int se_waves_per_cu_cap(SeForm f) { return f.is_long ? 4 : 4 * kSeWps; }

// ---- LDS per wave -----------------------------------------------------------------------------------------------------
inline size_t pe_lds_bytes(PeForm f, const LdsShape &s, u32 cap) { return pe_lds_layout<u32>(0, f.phase, f.is_long, f.big, f.text, s, cap).bytes; }
inline size_t se_lds_bytes(SeForm f, const LdsShape &s) { return se_lds_layout<u32>(0, f.is_long, s).bytes; }

}  // namespace abm
