// abm_kernel_form.hpp as plain host C++ (g++, ASan + UBSan): the selectors, tables and donors held to a FROZEN restatement
// of the launchers and occupancy queries they replaced -- the if chains of launch_pe_variant, launch_map_pe,
// launch_pe_seed, launch_pe_mate, launch_map_pe_long, launch_map_se, launch_map_se_long, the stand-ins of
// pe_resident_waves, pe_seed_resident_waves, pe_mate_resident_waves, pe_long_resident_waves, se_resident_waves,
// se_long_resident_waves, and abm_api.hip's pe_whole_launch, pe_text_stride and se_text_stride -- over every combination
// of the selectors' inputs.  The restatement below is not to follow the header: it says what those functions did.
#include <cstdio>
#include <set>
#include "../../abismal_amd/csrc/abm_kernel_form.hpp"

using namespace abm;

static long points = 0, wrong = 0;
#define CHECK(cond, ...) \
  do { ++points; if (!(cond)) { ++wrong; if (wrong < 40) { std::printf("WRONG %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// an instantiation in the old spelling: map_pe_kernel<BIG, TIMED, COOP, WPS, LONG, PHASE, REC, TEXT, BAM>
struct OldPe { bool exists, big, timed, coop; int wps; bool lng; int phase; bool rec, text, bam; };
static bool same(const OldPe &o, const PeForm &f) {
  return o.big == f.big && o.timed == f.timed && o.coop == f.coop && o.wps == f.wps && o.lng == f.is_long && o.phase == f.phase &&
         o.rec == f.rec && o.text == f.text && o.bam == f.bam;
}
constexpr int W = 4, S = 4, M = 4;  // ABM_PE_WAVES_PER_SIMD, kPeSeedWps, kPeMateWps as they were

// pe_whole_launch: pe_waves_per_simd(lds, stamps, G != 0), the experiment override, the text builds at W
static int old_wps(size_t lds, bool stamps, u32 G, bool text, int override_wps) {
  int wps = (!stamps && G != 0 && lds != 0 && (160u * 1024u) / lds <= 13u) ? 3 : W;
  if ((override_wps == 3 || override_wps == 4) && !stamps && G != 0) wps = override_wps;
  if (text) wps = W;
  return wps;
}
// what ran (launch) and what sized the grid (donor) for one launch of the old code.  text: the launch was to write
// records -- which pe_text_stride only ever asked for with the stamps off and G != 0, for every launch of the batch alike;
// the launchers refused (hipErrorInvalidValue) stamps, and launch_map_pe G == 0 as well
static void old_pe(PeRole role, u32 G, bool wrec, bool fit, bool stamps, bool text, bool bam, size_t lds, int override_wps, OldPe &launch, OldPe &donor) {
  const bool records = G == 4 && wrec && fit;  // pe_records
  launch = donor = OldPe{true, false, false, false, W, false, kWhole, false, false, false};
  if (role == PeRole::kTier1 || role == PeRole::kTier2) {
    const bool big = role == PeRole::kTier2;
    const int wps = old_wps(lds, stamps, G, text, override_wps);
    donor = OldPe{true, big, false, true, wps == 3 ? 3 : W, false, kWhole, false, false, false};  // pe_resident_waves(lds, big, wps)
    if (text) {  // launch_map_pe
      if (stamps || G == 0) { launch.exists = false; return; }
      launch = OldPe{true, big, false, true, W, false, kWhole, false, true, bam};
      return;
    }
    // launch_pe_variant<BIG, TIMED>
    if (big && records) launch = (!stamps && wps == 3) ? OldPe{true, true, false, true, 3, false, kWhole, true, false, false} : OldPe{true, true, stamps, true, W, false, kWhole, true, false, false};
    else if (G != 0) launch = (!stamps && wps == 3) ? OldPe{true, big, false, true, 3, false, kWhole, false, false, false} : OldPe{true, big, stamps, true, W, false, kWhole, false, false, false};
    else launch = OldPe{true, big, stamps, false, W, false, kWhole, false, false, false};
  }
  else if (role == PeRole::kSeed) {  // launch_pe_seed (it never wrote records); pe_seed_resident_waves(lds, G != 0)
    donor = OldPe{true, false, false, G != 0, S, false, kSeed, false, false, false};
    if (records) launch = OldPe{true, false, stamps, true, S, false, kSeed, true, false, false};
    else launch = OldPe{true, false, stamps, G != 0, S, false, kSeed, false, false, false};
  }
  else if (role == PeRole::kMateSmall || role == PeRole::kMateBig) {  // launch_pe_mate; pe_mate_resident_waves(lds, big)
    const bool big = role == PeRole::kMateBig;
    donor = OldPe{true, big, false, false, M, false, kMate, false, false, false};
    if (text) {
      if (stamps || G == 0) { launch.exists = false; return; }  // (G == 0: pe_text_stride's rule, see above)
      launch = OldPe{true, big, false, false, M, false, kMate, false, true, bam};
    }
    else launch = OldPe{true, big, stamps, false, M, false, kMate, false, false, false};
  }
  else launch = donor = OldPe{true, true, false, false, 1, true, kWhole, false, false, false};  // launch_map_pe_long, pe_long_resident_waves
}

// single-end, old spelling: map_se_kernel<TIMED, COOP, REC>, map_se_bam_kernel<COOP, REC>, map_se_long_kernel
struct OldSe { bool exists; int kernel; bool timed, coop, rec; };  // kernel: 0 map_se_kernel, 1 map_se_bam_kernel, 2 map_se_long_kernel
static bool same(const OldSe &o, const SeForm &f) {
  return (o.kernel == 1) == f.bam && (o.kernel == 2) == f.is_long && o.timed == f.timed && o.coop == f.coop && o.rec == f.rec && f.wps == (o.kernel == 2 ? 1 : 5);
}
static void old_se(SeRole role, u32 G, bool wrec, bool fit, bool stamps, bool text, bool bam_format, OldSe &launch, OldSe &donor, int &cap) {
  if (role == SeRole::kLong) { launch = donor = OldSe{true, 2, false, false, false}; cap = 4; return; }  // launch_map_se_long, se_long_resident_waves
  donor = OldSe{true, 0, false, true, false};  // se_resident_waves: map_se_kernel<false, true>
  cap = 4 * 5;                                 // kSeWavesPerCu
  const bool bam = text && bam_format;         // a.sam_tail != nullptr && a.sam_format == kRecordsBam
  launch = OldSe{true, 0, false, false, false};
  if (bam && stamps) { launch.exists = false; return; }
  const int kernel = (!stamps && bam) ? 1 : 0;
  if (G != 0 && wrec && fit && (G == 2 || G == 4)) launch = OldSe{true, kernel, stamps, true, true};
  else if (G != 0) launch = OldSe{true, kernel, stamps, true, false};
  else launch = OldSe{true, kernel, stamps, false, false};
}

int main() {
  std::set<u32> pe_seen, se_seen;
  const PeRole pe_roles[] = {PeRole::kTier1, PeRole::kTier2, PeRole::kSeed, PeRole::kMateSmall, PeRole::kMateBig, PeRole::kLong};
  const u32 Gs[] = {0, 2, 4, 8};
  // 160 KB / lds <= 13 from 11703 bytes on: either side of it, and 0
  const size_t ldss[] = {0, 11702, 11703};
  static_assert((160u * 1024u) / 11702 == 14 && (160u * 1024u) / 11703 == 13, "the threshold's two sides");
  for (PeRole role : pe_roles)
    for (u32 G : Gs)
      for (int records = 0; records < 3; ++records)  // absent, serving, too short
        for (int stamps = 0; stamps < 2; ++stamps)
          for (int text = 0; text < 3; ++text)  // none, SAM, BAM
            for (size_t lds : ldss)
              for (int ov : {0, 3, 4}) {
                const bool wrec = records != 0, fit = records == 1;
                OldPe launch, donor;
                old_pe(role, G, wrec, fit, stamps != 0, text != 0, text == 2, lds, ov, launch, donor);
                const PeChoice c = pe_select(PeFacts{role, G, wrec && fit, stamps != 0, text != 0, text == 2, lds, ov});
                CHECK(c.ok == launch.exists, "role %d G %u records %d stamps %d text %d lds %zu override %d", static_cast<int>(role), G, records, stamps, text, lds, ov);
                if (!c.ok || !launch.exists) continue;
                CHECK(same(launch, c.form), "role %d G %u records %d stamps %d text %d lds %zu override %d: form id %u", static_cast<int>(role), G, records, stamps, text, lds, ov, c.form.id());
                CHECK(c.form.valid() && pe_form_index(c.form) >= 0, "selected form %u is not in the table", c.form.id());
                const PeForm d = pe_donor(c.form);
                CHECK(same(donor, d) && pe_form_index(d) >= 0, "donor of form %u: %u", c.form.id(), d.id());
                CHECK(pe_waves_per_cu_cap(c.form) == (role == PeRole::kLong ? 1 : kNoWaveCap), "cap of form %u", c.form.id());
                // the layout fields are the role's: the LDS the selector was told is the LDS of the form it returns
                const PeForm r = pe_role_form(role, c.form.text);
                CHECK(r.phase == c.form.phase && r.big == c.form.big && r.is_long == c.form.is_long && r.text == c.form.text, "layout fields of form %u", c.form.id());
                pe_seen.insert(c.form.id());
              }
  for (SeRole role : {SeRole::kMain, SeRole::kLong})
    for (u32 G : Gs)
      for (int records = 0; records < 3; ++records)
        for (int stamps = 0; stamps < 2; ++stamps)
          for (int text = 0; text < 3; ++text) {
            const bool wrec = records != 0, fit = records == 1;
            OldSe launch, donor;
            int cap = 0;
            old_se(role, G, wrec, fit, stamps != 0, text != 0, text == 2, launch, donor, cap);
            const SeChoice c = se_select(SeFacts{role, G, wrec && fit, stamps != 0, text != 0, text == 2});
            CHECK(c.ok == launch.exists, "se role %d G %u records %d stamps %d text %d", static_cast<int>(role), G, records, stamps, text);
            if (!c.ok || !launch.exists) continue;
            CHECK(same(launch, c.form), "se role %d G %u records %d stamps %d text %d: form id %u", static_cast<int>(role), G, records, stamps, text, c.form.id());
            CHECK(c.form.valid() && se_form_index(c.form) >= 0, "selected form %u is not in the table", c.form.id());
            const SeForm d = se_donor(c.form);
            CHECK(same(donor, d) && se_form_index(d) >= 0 && se_waves_per_cu_cap(c.form) == cap, "donor / cap of form %u", c.form.id());
            se_seen.insert(c.form.id());
          }
  // no dead build: every row of either table is some input's choice
  CHECK(kPeFormCount == 32 && kSeFormCount == 10, "%d + %d builds", kPeFormCount, kSeFormCount);
  for (const PeForm &f : kPeForms) CHECK(pe_seen.count(f.id()) == 1, "no input selects pair form %u", f.id());
  for (const SeForm &f : kSeForms) CHECK(se_seen.count(f.id()) == 1, "no input selects single-end form %u", f.id());
  CHECK(pe_seen.size() == 32 && se_seen.size() == 10, "%zu + %zu forms selected", pe_seen.size(), se_seen.size());
  // ids: they round-trip, the families' never meet, and their bits are where abismal_amd.h says they are
  for (const PeForm &f : kPeForms) CHECK(pe_form_of(f.id()).id() == f.id() && !(f.id() & kSeFormBit), "pair id %u", f.id());
  for (const SeForm &f : kSeForms) CHECK(se_form_of(f.id()).id() == f.id() && (f.id() & kSeFormBit), "single-end id %u", f.id());
  CHECK((PeForm{kMate, true, false, false, false, false, true, true, 4}.id()) == (2u | 4u | 128u | 256u | (4u << 9)), "pair id bits");
  CHECK((PeForm{kSeed, false, false, true, true, true, false, false, 4}.id()) == (1u | 16u | 32u | 64u | (4u << 9)), "pair id bits");
  CHECK((PeForm{kWhole, true, true, false, false, false, false, false, 1}.id()) == (4u | 8u | (1u << 9)), "pair id bits");
  CHECK((SeForm{true, true, true, false, false, 5}.id()) == (0x80000000u | 1u | 2u | 4u | (5u << 9)), "single-end id bits");
  CHECK((SeForm{false, false, false, true, false, 5}.id()) == (0x80000000u | 8u | (5u << 9)), "single-end id bits");
  CHECK((SeForm{false, false, false, false, true, 1}.id()) == (0x80000000u | 16u | (1u << 9)), "single-end id bits");
  std::printf("%ld points, %ld wrong\n", points, wrong);
  return wrong == 0 ? 0 : 1;
}
