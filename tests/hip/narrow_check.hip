// GPU test program (built and run by tests/test_gpu_narrowing_at_n_runs.py): the kernels' three ways of narrowing a
// bucket -- narrow_both<false> (letters from the nibble array), narrow_both<true> (letters from the window records, back
// to the nibble array where a record's N flag is set or the probe is beyond its reach: record_nibble) and narrow_direct
// followed by what seed_pass does with it (the result if `ok`, else the letter loop: the kernel's own narrow_direct_chains,
// abm_seed.hpp, run here as seed_pass runs it) -- against a plain restatement of
// find_candidates / find_candidates_three (src/abismal.cpp:1163-1259): std::lower_bound letter by letter on the nibble
// array, and the step back when the range empties.
//
// What the fixtures of the parity tests hardly hold is what this index is made of: entries whose letters are BLANK (N)
// from some depth on.  The reference orders and bisects a blank nibble as 2-letter bit 1 and 3-letter symbol 0; the bit
// planes and the window records hold code 0 (= A) there: bit 0, and symbol 1 in the C->T alphabet.
//
// The index is built by hand.  The genome (37 k bases) is background plus tandem arrays of one 11-base unit with point
// mutations, so that all entries -- every 11th base of an array -- share their letters until a mutation or a blank:
//   * 11 arrays of 245 ... 255 bases, each followed by a blank stretch (300 or 30 bases): their entries have their first
//     blank letter at every depth 25 ... 255, each depth once;
//   * 30 arrays of 200 bases and 32 of 120, each followed by a short blank stretch: clusters of 30 / 32 entries with the
//     same blank depth;
//   * one array that ends where the genome's end padding (blank) begins;
//   * a stretch of 12 k bases with no blank within reach (nmap clear): arrays whose entries are whole.
// Seven ranges of 64 ... 331 of those entries form the three index arrays, each range sorted as the builder sorts a bucket
// (256 letters, bit2 / sortsym3 of the nibbles; src/AbismalIndex.cpp:857-978).  Planes and nmap come from
// launch_make_planes, the records (three and five blocks) from build_window_records; the records' N flags are compared
// with the nibble array entry by entry.  A case = one range, one read (an entry's letters, the unit where they are blank,
// sometimes a changed letter at or next to the first blank), a limit (often the first blank depth, one below, one above),
// maxc in {5, 20, 100} and an alphabet.  All indices stay inside their range by construction.
// Prints "OK <cases> ..." with the liveness counts per table, or the first mismatch.
#include "../../abismal_amd/csrc/abm_kernels.hip"
#include "../../abismal_amd/csrc/abm_ext.hip"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace abm;

constexpr u32 kW = 20, kWB = 5;            // a case's read: 320 nibbles / bits (limit <= 256, a few bases in front)
constexpr u32 kStrideQ = 24, kStrideB = 8; // words per case, with room for the searches' reads past the end
constexpr u32 kDirectFrom = 16;            // DevIndex::direct_min of this index
constexpr int kUnit = 11;

struct Case { u32 lo, hi, qbase, limit, maxc, g_to_a; };
// v[0] narrow_both<false>, v[1] narrow_both<true>, v[2] narrow_direct where seed_pass tries it, then narrow_both<true>: lo2, hi2, len2, lo3, hi3, len3;
// open[chain]: the chain was still open after that (not tried, or ok == false)
struct Out { u32 v[3][6]; u32 open[2]; };

__global__ __launch_bounds__(64) void run(DevIndex ix, const Case *cases, u32 n, const u64 *qpk_all, const u64 *qb_all, Out *out) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Case c = cases[t];
  const u64 *qpk = qpk_all + static_cast<size_t>(t) * kStrideQ, *qb = qb_all + static_cast<size_t>(t) * kStrideB;
  const bool g_to_a = c.g_to_a != 0;
  const u32 *idx3 = g_to_a ? ix.index_a : ix.index_t;
  const u32 rec3 = g_to_a ? ix.wrec_a0 : ix.wrec_t0;
  // the call as the kernel's stage sees it: a read of qbase + limit bases (so that its limit at offset qbase is the case's)
  SeedCall sc = {};
  sc.qpk = qpk; sc.qb = qb; sc.idx3 = idx3; sc.rec3 = rec3;
  sc.W = kW; sc.n_bits = 64u * kWB; sc.L = c.qbase + c.limit; sc.maxc = c.maxc; sc.g_to_a = g_to_a;
  Out o = {};
  for (int v = 0; v < 3; ++v) {
    u32 lo2 = c.lo, hi2 = c.hi, len2 = kKeyWeight, lo3 = c.lo, hi3 = c.hi, len3 = kKeyWeight3, probes = 0;
    bool run2 = true, run3 = true;
    if (v == 2) {
      // the kernel's own rule for where narrow_direct is tried and what is taken from it (narrow_direct_chains, abm_seed.hpp)
      Chains ch = {lo2, hi2, len2, lo3, hi3, len3, run2, run3};
      narrow_direct_chains(ix, sc, c.qbase, ch, probes);
      lo2 = ch.lo2; hi2 = ch.hi2; len2 = ch.len2; run2 = ch.run2;
      lo3 = ch.lo3; hi3 = ch.hi3; len3 = ch.len3; run3 = ch.run3;
      o.open[0] = run2; o.open[1] = run3;
    }
    if (v == 0) narrow_both<false>(ix, idx3, g_to_a, qb, 64u * kWB, qpk, c.qbase, c.limit, c.maxc, run2, lo2, hi2, len2, run3, lo3, hi3, len3, probes, rec3);
    else narrow_both<true>(ix, idx3, g_to_a, qb, 64u * kWB, qpk, c.qbase, c.limit, c.maxc, run2, lo2, hi2, len2, run3, lo3, hi3, len3, probes, rec3);
    o.v[v][0] = lo2; o.v[v][1] = hi2; o.v[v][2] = len2; o.v[v][3] = lo3; o.v[v][4] = hi3; o.v[v][5] = len3;
  }
  out[t] = o;
}

// ---- the host's side -------------------------------------------------------------------------------------------
static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return static_cast<unsigned>(rng_state >> 16); }
static u32 rnd_in(u32 lo, u32 hi) { return lo + rnd() % (hi - lo + 1); }

static std::vector<u8> G;  // genome nibbles: 1, 2, 4, 8, or 0 = blank
static u8 unit[kUnit];
static u32 h_bit2(u32 nt) { return (nt & 5u) == 0u; }
static u32 h_sym3(u32 nt, bool g_to_a) { return g_to_a ? (nt & 10u) : (nt & 5u); }
static u32 h_sym(int table, u32 nt) { return table == 0 ? h_bit2(nt) : h_sym3(nt, table == 2); }  // table 0: 2-letter, 1: C->T, 2: G->A
static u8 other_base(u8 b) { return static_cast<u8>(1u << ((__builtin_ctz(b) + 1 + rnd() % 3) & 3)); }

static void plant_array(u32 at, u32 n, unsigned permille) {
  for (u32 j = 0; j < n; ++j) {
    u8 b = unit[j % kUnit];
    if (rnd() % 1000 < permille) b = other_base(b);
    G[at + j] = b;
  }
}
static void blank(u32 at, u32 n) { for (u32 j = 0; j < n; ++j) G[at + j] = 0; }
static u32 first_blank(u32 pos) { for (u32 d = 0; d < 256; ++d) if (G[pos + d] == 0) return d; return 256; }

struct Tally { long blank = 0, flagged = 0; };
// find_candidates (table 0) / find_candidates_three (1, 2) on tbl[lo, hi): q = the read's nibbles from the seed offset on
static void host_narrow(const std::vector<u32> &tbl, int table, u32 &lo, u32 &hi, u32 &len, u32 limit, u32 maxc, const u8 *q,
                        const std::vector<u8> &flag_at, Tally &t) {
  u32 p = len, plo = lo, phi = hi;
  const u32 mid = table == 2 ? 2u : 1u, top = table == 2 ? 8u : 4u;
  auto below = [&](u32 gp, u32 bound) {
    const u32 nib = G[gp + p];
    t.blank += nib == 0;
    t.flagged += flag_at[gp];
    return h_sym(table, nib) < bound;
  };
  for (; p != limit && hi - lo > maxc; ++p) {
    plo = lo; phi = hi;
    const auto first = tbl.begin() + lo, last = tbl.begin() + hi;
    if (table == 0) {
      const u32 ones = static_cast<u32>(std::lower_bound(first, last, 1u, below) - tbl.begin());
      if (h_bit2(q[p])) lo = ones; else hi = ones;
    }
    else {
      const u32 b1 = static_cast<u32>(std::lower_bound(first, last, mid, below) - tbl.begin());
      const u32 b2 = static_cast<u32>(std::lower_bound(first, last, top, below) - tbl.begin());
      const u32 sym = h_sym3(q[p], table == 2);
      if (sym == 0) hi = b1;
      else if (sym == mid) { lo = b1; hi = b2; }
      else lo = b2;
    }
  }
  if (lo == hi) { --p; lo = plo; hi = phi; }
  len = p;
}

#define HIP_OK(x) do { if ((x) != hipSuccess) { printf("FAIL hip call at line %d\n", __LINE__); return 1; } } while (0)

int main() {
  // ---- the genome ----
  const u32 kLead = 512, kTail = 1024, kCleanFrom = 8200, kCleanArrays = 19, kZoneB = 22200, kLastArray = 36000, kLastLen = 400;
  const u32 n_bases = kLastArray + kLastLen + kTail;
  G.assign(n_bases + 1024, 0);  // (nothing reads past n_bases; the slack is blank like the padding)
  for (u32 k = kLead; k < n_bases - kTail; ++k) G[k] = static_cast<u8>(1u << (rnd() & 3));
  for (auto &b : unit) b = static_cast<u8>(1u << (rnd() & 3));
  unit[0] = 1; unit[1] = 2; unit[2] = 4; unit[3] = 8;  // every letter class occurs in the unit
  std::vector<u32> singles, cluster_a, cluster_b, last, clean;
  u32 cur = 600;
  for (u32 r = 0; r < kUnit; ++r) {  // first blank at 245 + r - 11 k: every depth 25 ... 255 once
    const u32 t = 245 + r, bl = (r % 2) ? 30 : 300;
    plant_array(cur, t, 15);
    blank(cur + t, bl);
    for (u32 k = 0; t - kUnit * k >= 25 && kUnit * k < t; ++k) singles.push_back(cur + kUnit * k);
    cur += t + bl + 20;
  }
  if (cur > 8000) { printf("FAIL layout (zone A ends at %u)\n", cur); return 1; }
  for (u32 a = 0; a < kCleanArrays; ++a) {
    const u32 at = kCleanFrom + 640 * a;
    plant_array(at, 600, 15);
    for (u32 k = 0; k < 26; ++k) clean.push_back(at + kUnit * k);
  }
  cur = kZoneB;
  for (u32 a = 0; a < 30; ++a) {
    plant_array(cur, 200, 5);
    blank(cur + 200, a % 5 == 0 ? 300 : 20);
    for (u32 k = 0; k <= 14; k += 2) cluster_a.push_back(cur + kUnit * k);
    cur += 200 + (a % 5 == 0 ? 300 : 20) + 10;
  }
  for (u32 a = 0; a < 32; ++a) {
    plant_array(cur, 120, 5);
    blank(cur + 120, 12);
    for (u32 k = 0; k <= 6; k += 3) cluster_b.push_back(cur + kUnit * k);
    cur += 120 + 12 + 8;
  }
  if (cur > kLastArray - 300) { printf("FAIL layout (zone B ends at %u)\n", cur); return 1; }
  plant_array(kLastArray, kLastLen, 15);  // ends on the last base before the end padding
  for (u32 k = 0; kLastLen - kUnit * k >= 25; ++k) last.push_back(kLastArray + kUnit * k);
  for (size_t k = clean.size(); k > 1; --k) std::swap(clean[k - 1], clean[rnd() % k]);
  for (u32 pos : clean) if (first_blank(pos) < 256 || pos + 25 + 256 + 64 > 20480) { printf("FAIL layout (clean entry %u)\n", pos); return 1; }

  // ---- the ranges and the three index arrays ----
  auto some = [](const std::vector<u32> &v, size_t from, size_t n) { return std::vector<u32>(v.begin() + from, v.begin() + from + n); };
  auto every = [](const std::vector<u32> &v, size_t step) { std::vector<u32> o; for (size_t k = 0; k < v.size(); k += step) o.push_back(v[k]); return o; };
  auto join = [](std::vector<std::vector<u32>> parts) { std::vector<u32> o; for (auto &p : parts) o.insert(o.end(), p.begin(), p.end()); return o; };
  std::vector<std::vector<u32>> ranges = {
      join({singles, some(clean, 0, 100)}),                       // every blank depth once
      join({cluster_a, some(clean, 100, 60)}),                    // clusters of 30
      join({cluster_b, every(singles, 7), some(clean, 160, 40)}), // clusters of 32 among single ones
      join({last, some(clean, 200, 64)}),                         // ends in the genome's end padding
      some(clean, 264, 200),                                      // no blank within reach: narrow_direct's own result
      some(clean, 0, 64),
      join({every(singles, 23), some(clean, 300, 54)}),
  };
  std::vector<u32> range_lo, range_hi;
  std::vector<u32> index[3];
  long depth_count[257] = {0};
  for (auto &r : ranges) {
    if (r.size() < 64 || r.size() > 400) { printf("FAIL range of %zu entries\n", r.size()); return 1; }
    for (u32 pos : r) ++depth_count[first_blank(pos)];
    std::sort(r.begin(), r.end(), [](u32 a, u32 b) { return a > b; });  // (the builder fills a bucket in descending order)
    range_lo.push_back(static_cast<u32>(index[0].size()));
    for (int table = 0; table < 3; ++table) {
      std::vector<u32> s = r;
      const u32 skip = table == 0 ? kKeyWeight : kKeyWeight3;
      std::stable_sort(s.begin(), s.end(), [&](u32 a, u32 b) {
        for (u32 k = skip; k < kSortDepth; ++k) {
          const u32 x = h_sym(table, G[a + k]), y = h_sym(table, G[b + k]);
          if (x != y) return x < y;
        }
        return false;
      });
      index[table].insert(index[table].end(), s.begin(), s.end());
    }
    range_hi.push_back(static_cast<u32>(index[0].size()));
  }
  long biggest_cluster = 0;
  for (u32 d = 25; d <= 255; ++d) {
    if (!depth_count[d]) { printf("FAIL no entry whose first blank letter is at depth %u\n", d); return 1; }
    biggest_cluster = std::max(biggest_cluster, depth_count[d]);
  }
  if (biggest_cluster < 30) { printf("FAIL no cluster of 30 entries with one blank depth\n"); return 1; }
  const u32 n_entries = static_cast<u32>(index[0].size());

  // ---- the device's index ----
  std::vector<u64> gw((G.size() + 15) / 16, 0);
  for (size_t k = 0; k < G.size(); ++k) gw[k / 16] |= static_cast<u64>(G[k]) << (4 * (k % 16));
  const u64 n_blocks = (n_bases + kPlaneBlock - 1) / kPlaneBlock + 16, nmap_words = ((n_bases >> kPlaneChunkBits) + 64) / 32 + 1;
  u64 *d_genome, *d_p0, *d_p1;
  u32 *d_nmap, *d_bad, *d_index[3];
  HIP_OK(hipMalloc(&d_genome, gw.size() * 8));
  HIP_OK(hipMemcpy(d_genome, gw.data(), gw.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMalloc(&d_p0, n_blocks * 16 + 128)); HIP_OK(hipMemset(d_p0, 0, n_blocks * 16 + 128));
  HIP_OK(hipMalloc(&d_p1, n_blocks * 16 + 128)); HIP_OK(hipMemset(d_p1, 0, n_blocks * 16 + 128));
  HIP_OK(hipMalloc(&d_nmap, nmap_words * 4 + 64)); HIP_OK(hipMemset(d_nmap, 0, nmap_words * 4 + 64));
  HIP_OK(hipMalloc(&d_bad, 64)); HIP_OK(hipMemset(d_bad, 0, 64));
  HIP_OK(launch_make_planes(d_genome, gw.size(), n_bases, n_blocks, d_p0, d_p1, d_nmap, d_bad, nullptr));
  u32 bad = 1;
  HIP_OK(hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost));
  if (bad) { printf("FAIL the genome has no bit planes\n"); return 1; }
  for (int t = 0; t < 3; ++t) {
    HIP_OK(hipMalloc(&d_index[t], n_entries * 4));
    HIP_OK(hipMemcpy(d_index[t], index[t].data(), n_entries * 4, hipMemcpyHostToDevice));
  }
  DevIndex ix = {};
  ix.genome = d_genome;
  ix.index = d_index[0]; ix.index_t = d_index[1]; ix.index_a = d_index[2];
  ix.max_candidates = 100; ix.window = kWindow; ix.min_len = kKeyWeight + kWindow - 1;
  ix.planes[0] = d_p0; ix.planes[1] = d_p1; ix.nmap = d_nmap;
  ix.direct_min = kDirectFrom;

  // ---- the cases ----
  std::vector<Case> cases;
  std::vector<std::vector<u8>> reads;  // nibbles, limit + qbase of them
  for (size_t r = 0; r < ranges.size(); ++r)
    for (u32 g_to_a = 0; g_to_a < 2; ++g_to_a)
      for (u32 maxc : {5u, 20u, 100u})
        for (int k = 0; k < 150; ++k) {
          const std::vector<u32> &tbl = index[1 + g_to_a];
          // the entry the read follows: one with a blank tail more often than not (if the range has one)
          u32 e = tbl[rnd_in(range_lo[r], range_hi[r] - 1)];
          for (int tries = 0; tries < 3 && first_blank(e) == 256 && rnd() % 4 != 0; ++tries) e = tbl[rnd_in(range_lo[r], range_hi[r] - 1)];
          const u32 d = first_blank(e);
          Case c;
          c.lo = range_lo[r]; c.hi = range_hi[r]; c.maxc = maxc; c.g_to_a = g_to_a;
          c.qbase = rnd() % 4 == 0 ? rnd_in(1, 16) : 0;
          const u32 top = 256 - c.qbase;  // (qbase + limit = the read's length: up to kSortDepth, seed_pass's gate for narrow_direct)
          c.limit = rnd_in(26, top);
          if (d < 256 && rnd() % 2 == 0) c.limit = std::min(top, std::max(26u, d - 1 + rnd() % 3));  // the first blank depth, one below, one above
          if (c.qbase && rnd() % 4 == 0) c.limit = rnd_in(top + 1, 256);                               // a read beyond kSortDepth: no direct narrowing
          std::vector<u8> q(c.qbase + c.limit);
          for (u32 j = 0; j < c.qbase; ++j) q[j] = static_cast<u8>(rnd() & 3);
          for (u32 j = 0; j < c.limit; ++j) {
            const u8 nib = G[e + j] ? G[e + j] : unit[j % kUnit];  // (every entry lies at phase 0 of its array)
            q[c.qbase + j] = static_cast<u8>(__builtin_ctz(nib));
          }
          auto change = [&](u32 at) { if (at < c.limit) q[c.qbase + at] = (q[c.qbase + at] + 1 + rnd() % 3) & 3; };
          if (rnd() % 2 == 0) change(rnd_in(16, c.limit - 1));
          if (d < 256 && rnd() % 3 == 0) change(d - 1 + rnd() % 3);
          // read_nibble of A, C, G, T in the case's alphabet
          for (auto &b : q) b = b == 0 ? (g_to_a ? 5 : 1) : b == 1 ? 2 : b == 2 ? 4 : (g_to_a ? 8 : 10);
          cases.push_back(c);
          reads.push_back(q);
        }
  const u32 n_cases = static_cast<u32>(cases.size());
  std::vector<u64> qpk(static_cast<size_t>(n_cases) * kStrideQ, ~0ull), qbits(static_cast<size_t>(n_cases) * kStrideB, ~0ull);
  for (u32 t = 0; t < n_cases; ++t)
    for (size_t j = 0; j < reads[t].size(); ++j) {
      u64 &w = qpk[static_cast<size_t>(t) * kStrideQ + j / 16];
      w = (w & ~(15ull << (4 * (j % 16)))) | (static_cast<u64>(reads[t][j]) << (4 * (j % 16)));
      if (!h_bit2(reads[t][j])) qbits[static_cast<size_t>(t) * kStrideB + j / 64] &= ~(1ull << (j % 64));  // (1 past the end)
    }
  Case *d_cases; u64 *d_qpk, *d_qb; Out *d_out;
  HIP_OK(hipMalloc(&d_cases, n_cases * sizeof(Case)));
  HIP_OK(hipMemcpy(d_cases, cases.data(), n_cases * sizeof(Case), hipMemcpyHostToDevice));
  HIP_OK(hipMalloc(&d_qpk, qpk.size() * 8)); HIP_OK(hipMemcpy(d_qpk, qpk.data(), qpk.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMalloc(&d_qb, qbits.size() * 8)); HIP_OK(hipMemcpy(d_qb, qbits.data(), qbits.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMalloc(&d_out, n_cases * sizeof(Out)));

  long blank_probes[3] = {0, 0, 0}, flagged_probes[3] = {0, 0, 0}, not_ok[3] = {0, 0, 0}, ok_big[3] = {0, 0, 0}, beyond_reach = 0, flagged_records = 0;
  for (u32 blocks : {3u, 5u}) {
    // ---- window records of this size, their N flags against the nibble array ----
    u64 *d_wrec;
    const size_t wbytes = window_record_bytes(3ull * n_entries, blocks);
    HIP_OK(hipMalloc(&d_wrec, wbytes));
    HIP_OK(hipMemset(d_wrec, 0, wbytes));
    const u64 n_idx[3] = {n_entries, n_entries, n_entries};
    HIP_OK(build_window_records(ix, n_blocks, n_bases, n_idx, blocks, d_wrec, nullptr));
    HIP_OK(hipDeviceSynchronize());
    ix.wrec = d_wrec;
    ix.wrec_t0 = n_entries; ix.wrec_a0 = 2 * n_entries;
    ix.wrec_blocks = blocks;
    ix.wrec_max_len = window_record_max_len(blocks);
    ix.wrec_back = ix.wrec_max_len - kKeyWeight;
    std::vector<u64> wrec(3ull * n_entries * blocks * 2);
    HIP_OK(hipMemcpy(wrec.data(), d_wrec, wrec.size() * 8, hipMemcpyDeviceToHost));
    std::vector<u8> flag_at(G.size(), 0);
    for (int table = 0; table < 3; ++table)
      for (u32 k = 0; k < n_entries; ++k) {
        const u32 pos = index[table][k], first = pos - ix.wrec_back, end = first + 64 * blocks - 1;
        bool want = false;
        for (u32 x = first; x < end; ++x) want |= G[x] == 0;
        const bool got = (wrec[2ull * ((static_cast<u64>(table) * n_entries + k) * blocks + (blocks - 1))] >> 63) != 0;
        if (want != got) { printf("FAIL N flag of record %u of table %d (%u blocks, entry at %u): %d, the nibble array says %d\n", k, table, blocks, pos, got, want); return 1; }
        flag_at[pos] = want;
        flagged_records += want;
      }

    HIP_OK(hipMemset(d_out, 0xFF, n_cases * sizeof(Out)));
    hipLaunchKernelGGL(run, dim3((n_cases + 63) / 64), dim3(64), 0, 0, ix, d_cases, n_cases, d_qpk, d_qb, d_out);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<Out> out(n_cases);
    HIP_OK(hipMemcpy(out.data(), d_out, n_cases * sizeof(Out), hipMemcpyDeviceToHost));

    for (u32 t = 0; t < n_cases; ++t) {
      const Case &c = cases[t];
      const int table3 = 1 + static_cast<int>(c.g_to_a);
      const u8 *q = reads[t].data() + c.qbase;
      u32 want[6] = {c.lo, c.hi, kKeyWeight, c.lo, c.hi, kKeyWeight3};
      Tally t2, t3;
      host_narrow(index[0], 0, want[0], want[1], want[2], c.limit, c.maxc, q, flag_at, t2);
      host_narrow(index[table3], table3, want[3], want[4], want[5], c.limit, c.maxc, q, flag_at, t3);
      blank_probes[0] += t2.blank; blank_probes[table3] += t3.blank;
      flagged_probes[0] += t2.flagged; flagged_probes[table3] += t3.flagged;
      if (want[2] > ix.wrec_max_len || want[5] > ix.wrec_max_len) ++beyond_reach;  // (probes at depth >= max_len are at or past the record's last base)
      static const char *names[3] = {"narrow_both<false>", "narrow_both<true>", "narrow_direct + the letter loop"};
      for (int v = 0; v < 3; ++v)
        for (int f = 0; f < 6; ++f)
          if (out[t].v[v][f] != want[f]) {
            printf("FAIL case %u (%u-block records, range [%u, %u), %s, maxc %u, qbase %u, limit %u): %s gives 2-letter [%u, %u) len %u, 3-letter [%u, %u) len %u; "
                   "std::lower_bound gives [%u, %u) len %u, [%u, %u) len %u\n", t, blocks, c.lo, c.hi, c.g_to_a ? "G->A" : "C->T", c.maxc, c.qbase, c.limit, names[v],
                   out[t].v[v][0], out[t].v[v][1], out[t].v[v][2], out[t].v[v][3], out[t].v[v][4], out[t].v[v][5], want[0], want[1], want[2], want[3], want[4], want[5]);
            return 1;
          }
      // what narrow_direct said, chain by chain: tried under seed_pass's gate, and the chain still open means ok == false
      const bool tried = c.qbase + c.limit <= kSortDepth && c.hi - c.lo >= kDirectFrom && c.hi - c.lo > c.maxc;
      if (tried && blocks == 3) {
        if (kKeyWeight < c.limit) { if (out[t].open[0]) ++not_ok[0]; else if (c.hi - c.lo >= 64) ++ok_big[0]; }
        if (kKeyWeight3 < c.limit) { if (out[t].open[1]) ++not_ok[table3]; else if (c.hi - c.lo >= 64) ++ok_big[table3]; }
      }
    }
    HIP_OK(hipFree(d_wrec));
  }
  static const char *tables[3] = {"2-letter", "C->T", "G->A"};
  for (int t = 0; t < 3; ++t)
    if (!blank_probes[t] || !flagged_probes[t] || !not_ok[t] || !ok_big[t]) {
      printf("FAIL coverage, %s table: blank letters probed %ld, probes of flagged records %ld, narrow_direct not ok %ld, ok on 64 entries or more %ld\n",
             tables[t], blank_probes[t], flagged_probes[t], not_ok[t], ok_big[t]);
      return 1;
    }
  if (!beyond_reach) { printf("FAIL coverage: no case narrows beyond the records' reach\n"); return 1; }
  printf("OK %u cases x 2 record sizes x 3 functions, %u entries in %zu ranges, every first blank depth 25 ... 255, clusters of up to %ld, %ld flagged records;",
         n_cases, n_entries, ranges.size(), biggest_cluster, flagged_records);
  for (int t = 0; t < 3; ++t)
    printf(" %s: blank letters probed %ld, probes of flagged records %ld, narrow_direct not ok %ld / ok on >= 64 entries %ld;", tables[t], blank_probes[t],
           flagged_probes[t], not_ok[t], ok_big[t]);
  printf(" cases narrowed beyond a record's reach %ld\n", beyond_reach);
  return 0;
}
