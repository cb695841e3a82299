// abismal_amd: what the sensitive seed pass checks at one seed offset, as a function of what is known of the offset's two
// base buckets -- shared by seed_pass (abm_seed.hpp) and plain host C++ (tests/cpp/sensitive_bounds_check.cpp).
// No HIP runtime calls.
//
// The sensitive pass (process_seeds, src/abismal.cpp:1352-1371) looks at the base buckets only: the 2-letter bucket
// [counter[k2], counter[k2 + 1]) and the 3-letter one [cnt3[k3], cnt3[k3 + 1]).  It checks a bucket that is not empty
// and holds at most max_candidates entries; the 2-letter one also only while it is no more than ten times the
// 3-letter one.  So of a bucket beyond max_candidates nothing but that fact is needed, and the specific pass of the
// same call, which has just looked the offset up, knows either the exact bucket or that fact (see seed_pass).
#pragma once
#include "abm_lds_layout.hpp"

namespace abm {

// one base bucket: where it begins and how many entries it holds.  d is exact wherever it is at most max_candidates;
// a bucket beyond that may say so with kBucketLarge instead of its size (lo is then whatever the teller had)
constexpr u32 kBucketLarge = 0xFFFFFFFFu;
struct BucketFact { u32 lo, d; };
// the sensitive pass's decision: the entries [lo2, lo2 + n2) and [lo3, lo3 + n3) are checked (n = 0: none)
struct SensBounds { bool chk2, chk3; u32 lo2, n2, lo3, n3; };

ABM_HD inline SensBounds sensitive_bounds(BucketFact f2, BucketFact f3, u32 maxc) {
  const u32 d2 = f2.d, d3 = f3.d;
  SensBounds b;
  // (a 3-letter bucket beyond max_candidates is larger than any 2-letter bucket that is checked: d2 <= maxc < d3, and
  // the comparison d2 <= 10 d3 holds without its size)
  b.chk2 = d2 != 0 && d2 <= maxc && (d3 == 0 || d3 > maxc || d2 <= 10u * d3);
  b.chk3 = d3 != 0 && d3 <= maxc;
  b.lo2 = f2.lo; b.n2 = b.chk2 ? d2 : 0u;
  b.lo3 = f3.lo; b.n3 = b.chk3 ? d3 : 0u;
  return b;
}

// The specific pass's side: the fact about a base bucket from a seed-extension table entry (abm_ext.hip: lo, size |
// len << 27 | state << 30, built for the same max_candidates).  state 0 at len 0 is the base bucket itself -- small,
// empty, or emptied at the first letter and stepped back: exact either way; a range that was narrowed (len > 0) or is
// still open (state 1) began beyond max_candidates.  state 2 (not tabulated) is not for this function: the caller
// loads the counters.
ABM_HD inline BucketFact bucket_fact_from_table(u32 lo, u32 word) {
  const u32 state = word >> 30, len = (word >> 27) & 7u;
  return (state == 0 && len == 0) ? BucketFact{lo, word & 0x7FFFFFFu} : BucketFact{lo, kBucketLarge};
}

}  // namespace abm
