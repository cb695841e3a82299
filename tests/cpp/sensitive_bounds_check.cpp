// sensitive_bounds (abismal_amd/csrc/abm_seed_bounds.hpp) as plain host C++ against the sensitive pass's own conditionals
// (process_seeds, src/abismal.cpp:1352-1371: both base buckets from the counters), for every pair of bucket sizes
// 0 .. max_candidates + 2, with either side, or both, told only as "beyond max_candidates" as well, at max_candidates 100
// and 20; and bucket_fact_from_table for every state and length a seed-extension table entry can carry.  Exact.
#include "../../abismal_amd/csrc/abm_seed_bounds.hpp"

#include <cstdio>
#include <vector>

using namespace abm;

namespace {

struct Want { bool chk2, chk3; u32 lo2, hi2, lo3, hi3; };
// the sensitive pass as it reads the counters: two entries per table (counter[k], counter[k + 1])
Want from_counters(const std::vector<u32> &c2, u32 k2, const std::vector<u32> &c3, u32 k3, u32 maxc) {
  const u32 lo2 = c2[k2], hi2 = c2[k2 + 1], lo3 = c3[k3], hi3 = c3[k3 + 1];
  const u32 d2 = hi2 - lo2, d3 = hi3 - lo3;
  Want w;
  w.chk2 = d2 != 0 && d2 <= maxc && (d3 == 0 || d2 <= 10u * d3);
  w.chk3 = d3 != 0 && d3 <= maxc;
  w.lo2 = lo2; w.hi2 = hi2; w.lo3 = lo3; w.hi3 = hi3;
  return w;
}

unsigned long points = 0, wrong = 0;
void check(const Want &w, BucketFact f2, BucketFact f3, u32 maxc, const char *what, u32 d2, u32 d3) {
  const SensBounds b = sensitive_bounds(f2, f3, maxc);
  ++points;
  bool ok = b.chk2 == w.chk2 && b.chk3 == w.chk3;
  // the entries the pass goes on to check: the segment the kernel forms from a checked bucket (Segs: lo, n)
  if (w.chk2) ok = ok && b.lo2 == w.lo2 && b.n2 == w.hi2 - w.lo2;
  else ok = ok && b.n2 == 0;
  if (w.chk3) ok = ok && b.lo3 == w.lo3 && b.n3 == w.hi3 - w.lo3;
  else ok = ok && b.n3 == 0;
  if (!ok) {
    ++wrong;
    if (wrong <= 20) std::printf("WRONG %s maxc %u d2 %u d3 %u: chk %d %d (want %d %d) n %u %u\n", what, maxc, d2, d3, b.chk2, b.chk3, w.chk2, w.chk3, b.n2, b.n3);
  }
}

}  // namespace

int main() {
  for (u32 maxc : {100u, 20u}) {
    for (u32 d2 = 0; d2 <= maxc + 2; ++d2)
      for (u32 d3 = 0; d3 <= maxc + 2; ++d3) {
        // counter arrays with the two buckets somewhere in the middle
        const std::vector<u32> c2 = {0, 7, 7 + d2, 7 + d2 + 3}, c3 = {0, 1000, 1000 + d3, 1000 + d3 + 1};
        const Want w = from_counters(c2, 1, c3, 1, maxc);
        const BucketFact e2 = {c2[1], d2}, e3 = {c3[1], d3};
        check(w, e2, e3, maxc, "exact/exact", d2, d3);
        // a bucket beyond max_candidates may be told as "large", with any lo (a narrowed range's)
        const BucketFact l2 = {c2[1] + 5, kBucketLarge}, l3 = {c3[1] + 9, kBucketLarge};
        if (d2 > maxc) check(w, l2, e3, maxc, "large/exact", d2, d3);
        if (d3 > maxc) check(w, e2, l3, maxc, "exact/large", d2, d3);
        if (d2 > maxc && d3 > maxc) check(w, l2, l3, maxc, "large/large", d2, d3);
      }
    // "large" against buckets far beyond: the sizes a repeat-rich genome has
    for (u32 big : {maxc + 3, 10 * maxc, 10 * maxc + 1, 1u << 20, (1u << 27) - 1})
      for (u32 d = 0; d <= maxc + 2; ++d) {
        const std::vector<u32> cs = {0, 11, 11 + d, 11 + d + 2}, cb = {0, 5, 5 + big, 5 + big + 1};
        check(from_counters(cs, 1, cb, 1, maxc), {cs[1], d}, {cb[1], kBucketLarge}, maxc, "small/large", d, big);
        check(from_counters(cs, 1, cb, 1, maxc), {cs[1], d}, {cb[1], big}, maxc, "small/big", d, big);
        check(from_counters(cb, 1, cs, 1, maxc), {cb[1], kBucketLarge}, {cs[1], d}, maxc, "large/small", big, d);
        check(from_counters(cb, 1, cs, 1, maxc), {cb[1], big}, {cs[1], d}, maxc, "big/small", big, d);
      }
  }
  // table entries: state 0 at length 0 is the base bucket (exact, whatever its size); every other is beyond max_candidates
  for (u32 state = 0; state < 2; ++state)
    for (u32 len = 0; len < 8; ++len)
      for (u32 size : {0u, 1u, 100u, 101u, (1u << 27) - 1}) {
        const BucketFact f = bucket_fact_from_table(42u, size | (len << 27) | (state << 30));
        ++points;
        const bool exact = state == 0 && len == 0;
        if (f.lo != 42u || f.d != (exact ? size : kBucketLarge)) { ++wrong; std::printf("WRONG table entry state %u len %u size %u\n", state, len, size); }
      }
  std::printf("%lu points, %lu wrong\n", points, wrong);
  return wrong == 0 ? 0 : 1;
}
