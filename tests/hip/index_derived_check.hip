// GPU test program (built and run by tests/test_gpu_index_derived.py): the structures a context derives from the index on
// the device at upload -- the bit planes with nmap and the IUPAC flag (make_planes_kernel), the window records
// (window_records_kernel) and the seed-extension tables (ext_bounds_kernel, ext_gaps_kernel, ext_entries_kernel) -- each
// compared ENTRY BY ENTRY with plain serial host code written from the reference's rules: letters from the nibble array
// through bit2 / sortsym3 restated here, std::lower_bound letter by letter with the step back when the range empties
// (find_candidates / find_candidates_three, src/abismal.cpp:1163-1259).  Nothing is taken from the kernels under test.
//
//   index_derived_check - planes            hand-built genomes; plane contents, p0 == p1, the IUPAC flag, nmap complete and tight
//   index_derived_check FILE records        records of 3, 4 and 5 blocks over the file's arrays and over synthetic positions
//   index_derived_check FILE tables MAXC [sorted]   every table at 1 / 3 / 6 (2-letter) and 1 / 2 / 3 (3-letter) letters, each built
//                                           with the product's gap list and with one of 8 slots; `sorted` requires the liveness counts per table
//   index_derived_check FILE expect MAXC    the host's side of `tables` alone (no device): the liveness counts
//   index_derived_check - bigbucket         one base bucket of 2^27 + 1 entries: not tabulated, everything else empty
// Prints "OK <counts ...>" or the first mismatch.
#include "../../abismal_amd/csrc/abm_kernels.hip"
#include "../../abismal_amd/csrc/abm_ext.hip"
#include "../../abismal_amd/csrc/abm_index_file.cpp"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
using namespace abm;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("FAIL hip call at line %d: %s\n", __LINE__, hipGetErrorString(e_)); return 1; } } while (0)

// ---- the reference's letters, restated -------------------------------------------------------------------------
static u32 h_bit2(u32 nt) { return (nt & 5u) == 0u; }                                         // get_bit: 1 for C, T and blank
static u32 h_sym3(u32 nt, bool g_to_a) { return g_to_a ? (nt & 10u) : (nt & 5u); }            // the sort's 3-letter symbol
static u32 h_mid(int table) { return table == 2 ? 2u : 1u; }
static u32 h_top(int table) { return table == 2 ? 8u : 4u; }
// digit of a key (table 0: 2-letter bit; 1: C->T, 2: G->A: symbol class below mid / below top / the rest)
static u32 h_digit(int table, u32 nt) {
  if (table == 0) return h_bit2(nt);
  const u32 s = h_sym3(nt, table == 2);
  return s < h_mid(table) ? 0u : (s < h_top(table) ? 1u : 2u);
}
static u32 nib_of(const std::vector<u64> &g, u64 pos) { return (pos >> 4) < g.size() ? static_cast<u32>(g[pos >> 4] >> (4 * (pos & 15))) & 15u : 0u; }
static u32 code_of(u32 nib) { return nib ? static_cast<u32>(__builtin_ctz(nib)) : 0u; }
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// =================================================================================================================
// planes
// =================================================================================================================
struct PlaneGenome { const char *name; u64 n_bases; std::vector<u8> nib; bool want_bad; };

static int check_planes(const PlaneGenome &pg, long &flagged_out, long &unflagged_out, long &reach_only_out) {
  const u64 n_bases = pg.n_bases, n_words = (n_bases + 15) / 16;
  std::vector<u64> gw(n_words, 0);
  for (u64 k = 0; k < 16 * n_words && k < pg.nib.size(); ++k) gw[k / 16] |= static_cast<u64>(pg.nib[k]) << (4 * (k % 16));
  const u64 n_blocks = (n_bases + kPlaneBlock - 1) / kPlaneBlock + 16, nmap_words = ((n_bases >> kPlaneChunkBits) + 64) / 32 + 1;
  u64 *d_genome, *d_p0, *d_p1;
  u32 *d_nmap, *d_bad;
  HIP_OK(hipMalloc(&d_genome, n_words * 8));
  HIP_OK(hipMemcpy(d_genome, gw.data(), n_words * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMalloc(&d_p0, n_blocks * 16)); HIP_OK(hipMemset(d_p0, 0xA5, n_blocks * 16));  // (a block left unwritten shows)
  HIP_OK(hipMalloc(&d_p1, n_blocks * 16)); HIP_OK(hipMemset(d_p1, 0x5A, n_blocks * 16));
  HIP_OK(hipMalloc(&d_nmap, nmap_words * 4)); HIP_OK(hipMemset(d_nmap, 0, nmap_words * 4));
  HIP_OK(hipMalloc(&d_bad, 64)); HIP_OK(hipMemset(d_bad, 0, 64));
  HIP_OK(launch_make_planes(d_genome, n_words, n_bases, n_blocks, d_p0, d_p1, d_nmap, d_bad, nullptr));
  HIP_OK(hipDeviceSynchronize());
  std::vector<u64> p0(2 * n_blocks), p1(2 * n_blocks);
  std::vector<u32> nmap(nmap_words);
  u32 bad = 7;
  HIP_OK(hipMemcpy(p0.data(), d_p0, n_blocks * 16, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(p1.data(), d_p1, n_blocks * 16, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(nmap.data(), d_nmap, nmap_words * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost));
  HIP_OK(hipFree(d_genome)); HIP_OK(hipFree(d_p0)); HIP_OK(hipFree(d_p1)); HIP_OK(hipFree(d_nmap)); HIP_OK(hipFree(d_bad));

  // the IUPAC flag: a nibble of two or more bits INSIDE n_bases
  bool multi_inside = false;
  for (u64 q = 0; q < n_bases; ++q) multi_inside |= __builtin_popcount(nib_of(gw, q)) > 1;
  if (multi_inside != pg.want_bad) { printf("FAIL planes, genome %s: the fixture's own IUPAC expectation is off\n", pg.name); return 1; }
  if ((bad != 0) != multi_inside) { printf("FAIL planes, genome %s: bad flag %u, the nibble array says %d\n", pg.name, bad, multi_inside); return 1; }
  // contents
  for (u64 b = 0; b < n_blocks; ++b) {
    if (p0[2 * b] != p1[2 * b] || p0[2 * b + 1] != p1[2 * b + 1]) { printf("FAIL planes, genome %s: block %llu differs between the two copies\n", pg.name, (unsigned long long)b); return 1; }
    for (u32 j = 0; j < 64; ++j) {
      const u64 q = 64 * b + j;
      const u32 nb = nib_of(gw, q);  // (0 beyond n_words)
      if (__builtin_popcount(nb) > 1) continue;  // (an IUPAC letter has no code: the planes are not used then)
      const u32 got = static_cast<u32>((p0[2 * b] >> j) & 1u) | (static_cast<u32>((p0[2 * b + 1] >> j) & 1u) << 1);
      if (got != code_of(nb)) { printf("FAIL planes, genome %s: base %llu (nibble %u) has code %u, expected %u\n", pg.name, (unsigned long long)q, nb, got, code_of(nb)); return 1; }
    }
  }
  // nmap: blank = an empty nibble inside n_bases.  next_blank[p] = first blank at or after p
  const u64 n_chunks = nmap_words * 32, span = n_chunks << kPlaneChunkBits;
  std::vector<u64> next_blank(span + 1, ~0ull);
  for (u64 p = span; p-- > 0;) next_blank[p] = (p < n_bases && nib_of(gw, p) == 0) ? p : next_blank[p + 1];
  long flagged = 0, unflagged = 0, reach_only = 0;
  for (u64 c = 0; c < n_chunks; ++c) {
    const bool got = (nmap[c >> 5] >> (c & 31)) & 1u;
    bool must = false, may = false, own = false;
    for (u64 p = c << kPlaneChunkBits; p < (c + 1) << kPlaneChunkBits; ++p) {
      const u64 nb = next_blank[p];
      if (nb == ~0ull) continue;
      must |= nb - p <= kPlaneReach;
      may |= nb - p <= kPlaneReach + 63;
      own |= nb < (c + 1) << kPlaneChunkBits;
    }
    if (must && !got) { printf("FAIL planes, genome %s: chunk %llu holds a position with a blank within %u bases and is not flagged (nmap incomplete)\n", pg.name, (unsigned long long)c, kPlaneReach); return 1; }
    if (got && !may) { printf("FAIL planes, genome %s: chunk %llu is flagged and no position in it has a blank within %u + 63 bases (nmap not tight)\n", pg.name, (unsigned long long)c, kPlaneReach); return 1; }
    flagged += got; unflagged += !got; reach_only += got && !own;
  }
  flagged_out += flagged; unflagged_out += unflagged; reach_only_out += reach_only;
  return 0;
}

static int cmd_planes() {
  // 12 chunks of 4,096 bases and a ragged end; blank nibbles (chunk c = 4096 c ...):
  //   4096 * 1 + 448         first base of its block; at - kPlaneReach = 4096 * 1 - 64: just before the boundary -> chunk 0 by reach alone
  //   4096 * 3 + 512         first base of its block; at - kPlaneReach on the boundary -> chunk 3 alone, chunk 2 clear
  //   4096 * 5 + 511         LAST base of the block at 448: position 4096 * 5 - 1 is within reach -> chunk 4 by reach alone
  //   4096 * 7 + 576 ... +70 a run over a block boundary; at - kPlaneReach just after the boundary -> chunk 7 alone, chunk 6 clear
  //   4096 * 9 + 575         last base of the block at 512, and a run 4096 * 9 + 2000 ... 2300 -> chunk 9 alone, chunk 8 clear
  // chunks 10, 11, the ragged end and the guard blocks hold no blank: the empty nibbles beyond n_bases must not count.
  auto make = [](u64 n_bases, u64 seed) {
    std::vector<u8> g(n_bases + 64, 0);
    u64 s = seed;
    for (u64 k = 0; k < n_bases; ++k) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; g[k] = static_cast<u8>(1u << ((s >> 20) & 3)); }
    g[4096 * 1 + 448] = 0;
    g[4096 * 3 + 512] = 0;
    g[4096 * 5 + 511] = 0;
    for (u32 k = 576; k <= 646; ++k) g[4096 * 7 + k] = 0;
    g[4096 * 9 + 575] = 0;
    for (u32 k = 2000; k <= 2300; ++k) g[4096 * 9 + k] = 0;
    return g;
  };
  std::vector<PlaneGenome> gs;
  const u64 ragged = 4096 * 12 + 37, sixteen = 4096 * 12 + 48;  // 37: no multiple of 16; 48: a multiple of 16, none of 64
  gs.push_back({"of 12 chunks + 37 bases", ragged, make(ragged, 0x1234567ull), false});
  gs.push_back({"of 12 chunks + 48 bases", sixteen, make(sixteen, 0x7654321ull), false});
  { PlaneGenome g = {"with one IUPAC nibble inside", ragged, make(ragged, 0x1234567ull), true}; g.nib[4096 * 2 + 77] = 5; gs.push_back(g); }
  { PlaneGenome g = {"with an IUPAC nibble on its last base", ragged, make(ragged, 0x1234567ull), true}; g.nib[ragged - 1] = 12; gs.push_back(g); }
  { PlaneGenome g = {"with multi-bit nibbles only beyond its last base", ragged, make(ragged, 0x1234567ull), false}; g.nib[ragged] = 3; g.nib[ragged + 9] = 15; gs.push_back(g); }
  { PlaneGenome g = {"whose last base is blank", ragged, make(ragged, 0x1234567ull), false}; g.nib[ragged - 1] = 0; gs.push_back(g); }
  long flagged = 0, unflagged = 0, reach_only = 0;
  const double t0 = now_s();
  for (size_t k = 0; k < gs.size(); ++k) {
    long f = 0, u = 0, r = 0;
    if (check_planes(gs[k], f, u, r)) return 1;
    // the first five genomes: chunks 0, 1, 3, 4, 5, 7, 9 flagged, 0 and 4 by reach alone; the last one: its last two chunks (11, 12) as well
    const long want_f = k == 5 ? 9 : 7, want_r = k == 5 ? 3 : 2;
    if (f != want_f || r != want_r || u <= 0) { printf("FAIL planes, genome %s: %ld chunks flagged (%ld by reach alone), %ld not; the layout says %ld (%ld)\n", gs[k].name, f, r, u, want_f, want_r); return 1; }
    flagged += f; unflagged += u; reach_only += r;
  }
  printf("OK planes: %zu genomes, chunks flagged %ld, of them without a blank of their own %ld, not flagged %ld; %.2f s\n", gs.size(), flagged, reach_only, unflagged, now_s() - t0);
  return 0;
}

// =================================================================================================================
// the index file on the device
// =================================================================================================================
struct Dev {
  DevIndex ix = {};
  u64 n_bases = 0, n_blocks = 0;
  u64 n_idx[3] = {0, 0, 0};
};
template <class T> static int upload(const std::vector<T> &v, size_t slack, const T **out) {
  T *d;
  HIP_OK(hipMalloc(&d, v.size() * sizeof(T) + slack));
  HIP_OK(hipMemset(d, 0, v.size() * sizeof(T) + slack));
  if (!v.empty()) HIP_OK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = d;
  return 0;
}
static int upload_index(const HostIndex &h, Dev &d) {
  d.n_bases = h.chrom_starts.empty() ? 0 : h.chrom_starts.back();
  if (upload(h.genome, 64, &d.ix.genome) || upload(h.counter, 64, &d.ix.counter) || upload(h.counter_t, 64, &d.ix.counter_t) ||
      upload(h.counter_a, 64, &d.ix.counter_a) || upload(h.index, 64, &d.ix.index) || upload(h.index_t, 64, &d.ix.index_t) ||
      upload(h.index_a, 64, &d.ix.index_a)) return 1;
  d.n_idx[0] = h.index.size(); d.n_idx[1] = h.index_t.size(); d.n_idx[2] = h.index_a.size();
  d.ix.max_candidates = h.max_candidates; d.ix.window = h.window; d.ix.min_len = kKeyWeight + h.window - 1;
  return 0;
}

// =================================================================================================================
// records
// =================================================================================================================
struct RecLive { long before = 0, past = 0, aligned = 0, flagged = 0, unflagged = 0, records = 0; };

static int check_records(const HostIndex &h, const Dev &d, const u32 *d_arrays[3], const std::vector<u32> *arrays[3], u32 blocks, const char *what, RecLive &live) {
  const u32 back = window_record_max_len(blocks) - kKeyWeight;
  u64 n_idx[3], n_entries = 0;
  for (int m = 0; m < 3; ++m) { n_idx[m] = arrays[m]->size(); n_entries += n_idx[m]; }
  DevIndex ix = d.ix;
  ix.index = d_arrays[0]; ix.index_t = d_arrays[1]; ix.index_a = d_arrays[2];
  u64 *d_wrec;
  const size_t bytes = window_record_bytes(n_entries, blocks);
  HIP_OK(hipMalloc(&d_wrec, bytes));
  HIP_OK(hipMemset(d_wrec, 0xA5, bytes));  // (a record left unwritten, or written to another's place, shows)
  HIP_OK(build_window_records(ix, d.n_blocks, d.n_bases, n_idx, blocks, d_wrec, nullptr));
  HIP_OK(hipDeviceSynchronize());
  std::vector<u64> wrec(n_entries * blocks * 2);
  HIP_OK(hipMemcpy(wrec.data(), d_wrec, wrec.size() * 8, hipMemcpyDeviceToHost));
  HIP_OK(hipFree(d_wrec));
  const long long plane_end = static_cast<long long>(64 * d.n_blocks);
  u64 rec = 0;  // record numbers run through the three arrays
  for (int m = 0; m < 3; ++m)
    for (u64 e = 0; e < n_idx[m]; ++e, ++rec) {
      const long long first = static_cast<long long>((*arrays[m])[e]) - back;
      const u32 data_bits = 64 * blocks - 1;
      const u64 *r = wrec.data() + 2 * rec * blocks;
      bool blank = false;
      for (u32 j = 0; j < data_bits; ++j) {
        const long long q = first + j;
        const u32 want = q >= 0 && q < plane_end ? code_of(nib_of(h.genome, static_cast<u64>(q))) : 0u;
        const u32 got = static_cast<u32>((r[2 * (j / 64)] >> (j % 64)) & 1u) | (static_cast<u32>((r[2 * (j / 64) + 1] >> (j % 64)) & 1u) << 1);
        if (got != want) {
          printf("FAIL records (%s, %u blocks): record %llu (array %d, entry %llu at %u), bit %u = base %lld: code %u, expected %u\n", what, blocks,
                 (unsigned long long)rec, m, (unsigned long long)e, (*arrays[m])[e], j, q, got, want);
          return 1;
        }
        if (q >= 0 && (static_cast<u64>(q) >= d.n_bases || nib_of(h.genome, static_cast<u64>(q)) == 0)) blank = true;
      }
      const u32 spare_lo = static_cast<u32>(r[2 * (blocks - 1)] >> 63), spare_hi = static_cast<u32>(r[2 * (blocks - 1) + 1] >> 63);
      if (spare_lo != (blank ? 1u : 0u) || spare_hi != 0) {
        printf("FAIL records (%s, %u blocks): record %llu (array %d, entry %llu at %u): spare bits %u (low), %u (high); the stretch %s a blank or a base past the genome\n",
               what, blocks, (unsigned long long)rec, m, (unsigned long long)e, (*arrays[m])[e], spare_lo, spare_hi, blank ? "holds" : "holds no");
        return 1;
      }
      live.before += first < 0;
      live.past += first + 64ll * blocks > plane_end;
      live.aligned += (first & 63) == 0;
      live.flagged += blank; live.unflagged += !blank;
      ++live.records;
    }
  return 0;
}

static int cmd_records(const HostIndex &h) {
  Dev d;
  if (upload_index(h, d)) return 1;
  d.n_blocks = (d.n_bases + kPlaneBlock - 1) / kPlaneBlock + 16;
  const u64 nmap_words = ((d.n_bases >> kPlaneChunkBits) + 64) / 32 + 1;
  u64 *d_p0, *d_p1; u32 *d_nmap, *d_bad;
  HIP_OK(hipMalloc(&d_p0, d.n_blocks * 16)); HIP_OK(hipMalloc(&d_p1, d.n_blocks * 16));
  HIP_OK(hipMalloc(&d_nmap, nmap_words * 4)); HIP_OK(hipMemset(d_nmap, 0, nmap_words * 4));
  HIP_OK(hipMalloc(&d_bad, 64)); HIP_OK(hipMemset(d_bad, 0, 64));
  HIP_OK(launch_make_planes(d.ix.genome, h.genome.size(), d.n_bases, d.n_blocks, d_p0, d_p1, d_nmap, d_bad, nullptr));
  u32 bad = 1;
  HIP_OK(hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost));
  if (bad) { printf("FAIL records: the genome has no bit planes\n"); return 1; }
  d.ix.planes[0] = d_p0; d.ix.planes[1] = d_p1; d.ix.nmap = d_nmap;
  const double t0 = now_s();
  RecLive file_live, synth_live;
  for (u32 blocks : {3u, 4u, 5u}) {
    const u32 back = window_record_max_len(blocks) - kKeyWeight;
    const u32 *d_file[3] = {d.ix.index, d.ix.index_t, d.ix.index_a};
    const std::vector<u32> *file[3] = {&h.index, &h.index_t, &h.index_a};
    if (check_records(h, d, d_file, file, blocks, "the file's arrays", file_live)) return 1;
    // positions no index holds: within `back` bases of base 0, on the block grid, the genome's last base, and up to and
    // past the planes' last block (the kernel reads the nibble array below n_bases only, the planes below n_blocks only)
    const u32 plane_end = static_cast<u32>(64 * d.n_blocks), nb = static_cast<u32>(d.n_bases);
    std::vector<u32> s = {0, 1, back - 1, back, back + 1, back + 64, back + 640, back + 63, back + 65, nb - 1, nb, nb - 64 * blocks + back, nb - 64 * blocks + back + 1,
                          plane_end - 64 * blocks + back - 1, plane_end - 64 * blocks + back, plane_end - 64 * blocks + back + 1, plane_end - 64 * blocks + back + 64,
                          plane_end - 64, plane_end - 1, plane_end + back - 64, plane_end + back, plane_end + back + 1, plane_end + back + 6400};
    for (u32 k = 0; k < 200; ++k) s.push_back(back + 64 * ((k * 2654435761u) % static_cast<u32>(d.n_blocks - 20)));                 // on the grid
    for (u32 k = 0; k < 200; ++k) s.push_back(static_cast<u32>((k * 40503ull * 2654435761ull) % (plane_end + 700)));               // anywhere
    std::vector<u32> rev(s.rbegin(), s.rend()), part(s.begin() + 3, s.end());
    const u32 *d_s[3];
    if (upload(s, 64, &d_s[0]) || upload(rev, 64, &d_s[1]) || upload(part, 64, &d_s[2])) return 1;
    const std::vector<u32> *sy[3] = {&s, &rev, &part};
    if (check_records(h, d, d_s, sy, blocks, "synthetic positions", synth_live)) return 1;
    for (int m = 0; m < 3; ++m) HIP_OK(hipFree(const_cast<u32 *>(d_s[m])));
  }
  if (!synth_live.before || !synth_live.past || !synth_live.aligned || !synth_live.flagged || !synth_live.unflagged || !file_live.flagged || !file_live.unflagged) {
    printf("FAIL records coverage: synthetic: before base 0 %ld, past the planes %ld, on the block grid %ld, flagged %ld, unflagged %ld; file: flagged %ld, unflagged %ld\n",
           synth_live.before, synth_live.past, synth_live.aligned, synth_live.flagged, synth_live.unflagged, file_live.flagged, file_live.unflagged);
    return 1;
  }
  printf("OK records: 3, 4 and 5 blocks; file: %ld records, %ld flagged, %ld unflagged, %ld on the block grid; synthetic: %ld records, %ld from before base 0, "
         "%ld past the last plane block, %ld on the block grid, %ld flagged, %ld unflagged; %.2f s\n", file_live.records, file_live.flagged, file_live.unflagged,
         file_live.aligned, synth_live.records, synth_live.before, synth_live.past, synth_live.aligned, synth_live.flagged, synth_live.unflagged, now_s() - t0);
  return 0;
}

// =================================================================================================================
// tables
// =================================================================================================================
static const char *kTableName[3] = {"2-letter", "C->T", "G->A"};
static u32 key_weight(int table) { return table == 0 ? kKeyWeight : kKeyWeight3; }
static u64 h_span(int table, u32 letters) { u64 s = 1; for (u32 k = 0; k < letters; ++k) s *= table == 0 ? 2u : 3u; return s; }
static u64 h_key(const std::vector<u64> &g, u64 pos, u32 depth, int table) {
  u64 key = 0;
  for (u32 j = 0; j < depth; ++j) key = key * (table == 0 ? 2u : 3u) + h_digit(table, nib_of(g, pos + j));
  return key;
}

struct Live { long early = 0, stepped = 0, open = 0, blank = 0, gaps_inline = 0, gaps_list = 0, keys = 0, fallback_buckets = 0, buckets = 0, entries_inside = 0; };

// what one table must hold, for the keys under its non-empty base buckets (listed in `bases`, span keys each)
struct Expect {
  bool misplaced = false;
  std::vector<u32> bases;      // non-empty base buckets, ascending
  std::vector<u8> descent;     // per listed bucket
  std::vector<uint2> entry;    // [bases.size() * span]
  u64 nonzero = 0;             // listed entries whose second word is not 0
  u32 long_gaps = 0;           // gaps of more than kGapInline keys: what the gap list's counter must say
};

static void expect_table(const HostIndex &h, int table, u32 extra, u32 maxc, Expect &x, Live &live) {
  const std::vector<u32> &index = table == 0 ? h.index : (table == 1 ? h.index_t : h.index_a);
  const std::vector<u32> &counter = table == 0 ? h.counter : (table == 1 ? h.counter_t : h.counter_a);
  const u32 W = key_weight(table), limit = W + extra;
  const u64 span = h_span(table, extra), n_base = counter.size() - 1, n_keys = n_base * span;
  std::vector<u64> key(index.size());
  for (size_t k = 0; k < index.size(); ++k) {
    key[k] = h_key(h.genome, index[k], limit, table);
    const u64 b = key[k] / span;
    if (!(counter[b] <= k && k < counter[b + 1])) x.misplaced = true;
  }
  if (x.misplaced) return;
  // the gaps ext_bounds_kernel's threads fill: keys (previous entry's key, this entry's key], and those above the last
  for (size_t k = 0; k <= index.size(); ++k) {
    const u64 last = k < index.size() ? key[k] : n_keys, first = k == 0 ? 0 : key[k - 1] + 1;
    if (k > 0 && k < index.size() && key[k] < key[k - 1]) continue;
    if (first > last) continue;
    if (last - first + 1 <= kGapInline) ++live.gaps_inline; else { ++live.gaps_list; ++x.long_gaps; }
  }
  for (u64 b = 0; b < n_base; ++b) {
    const u32 lo0 = counter[b], hi0 = counter[b + 1];
    if (lo0 == hi0) continue;
    bool descent = false;
    for (u32 k = lo0 + 1; k < hi0; ++k) descent |= key[k] < key[k - 1];
    x.bases.push_back(static_cast<u32>(b));
    x.descent.push_back(descent);
    ++live.buckets; live.fallback_buckets += descent;
    if (!descent)
      for (u32 k = lo0; k < hi0; ++k) {
        bool blank = false;
        for (u32 p = W; p < limit; ++p) blank |= nib_of(h.genome, static_cast<u64>(index[k]) + p) == 0;
        live.blank += blank;
      }
    for (u64 K = b * span; K < (b + 1) * span; ++K) {
      ++live.keys;
      if (descent) { x.entry.push_back(make_uint2(0u, 2u << 30)); ++x.nonzero; continue; }
      // find_candidates / find_candidates_three from p = W to the limit W + extra; the read's letters are K's digits
      u32 lo = lo0, hi = hi0, plo = lo, phi = hi, p = W;
      bool stepped = false;
      for (; p != limit && hi - lo > maxc; ++p) {
        plo = lo; phi = hi;
        const u32 digit = static_cast<u32>((K / h_span(table, limit - 1 - p)) % (table == 0 ? 2u : 3u));
        const auto first = index.begin() + lo, last = index.begin() + hi;
        if (table == 0) {
          const u32 ones = static_cast<u32>(std::lower_bound(first, last, 1u, [&](u32 gp, u32 bound) { return h_bit2(nib_of(h.genome, static_cast<u64>(gp) + p)) < bound; }) - index.begin());
          if (digit) lo = ones; else hi = ones;
        }
        else {
          auto below = [&](u32 gp, u32 bound) { return h_sym3(nib_of(h.genome, static_cast<u64>(gp) + p), table == 2) < bound; };
          const u32 b1 = static_cast<u32>(std::lower_bound(first, last, h_mid(table), below) - index.begin());
          const u32 b2 = static_cast<u32>(std::lower_bound(first, last, h_top(table), below) - index.begin());
          if (digit == 0) hi = b1;
          else if (digit == 1) { lo = b1; hi = b2; }
          else lo = b2;
        }
      }
      if (lo == hi) { --p; lo = plo; hi = phi; stepped = true; }
      const u32 size = hi - lo, len = p - W, state = (p == limit && size > maxc) ? 1u : 0u;
      const uint2 e = size >= (1u << 27) ? make_uint2(0u, 2u << 30) : make_uint2(lo, size | (len << 27) | (state << 30));
      x.entry.push_back(e);
      x.nonzero += e.y != 0;
      live.stepped += stepped; live.open += state; live.early += !stepped && !state && len >= 1 && len < extra;
    }
  }
}

__global__ __launch_bounds__(256) void count_nonzero_kernel(const uint2 *__restrict__ t, u64 n, unsigned long long *__restrict__ count) {
  // plain: one thread per key (blocks of 256, two grid dimensions: 2^31 keys are 2^23 blocks)
  const u64 K = (static_cast<u64>(blockIdx.y) * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
  if (K < n && t[K].y != 0) atomicAdd(count, 1ull);
}
__global__ __launch_bounds__(256) void count_differing_kernel(const uint2 *__restrict__ a, const uint2 *__restrict__ b, u64 n, unsigned long long *__restrict__ count) {
  const u64 K = (static_cast<u64>(blockIdx.y) * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
  if (K < n && (a[K].x != b[K].x || a[K].y != b[K].y)) atomicAdd(count, 1ull);
}
__global__ __launch_bounds__(256) void gather_kernel(const uint2 *__restrict__ t, const u32 *__restrict__ bases, u64 n_listed, u32 span, uint2 *__restrict__ out) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n_listed * span) out[i] = t[static_cast<u64>(bases[i / span]) * span + i % span];
}
static dim3 grid_for(u64 n) {
  const u64 blocks = (n + 255) / 256;
  const u32 gx = static_cast<u32>(std::min<u64>(blocks, 65535u));
  return dim3(gx, static_cast<u32>((blocks + gx - 1) / gx));
}

// where build_ext_table keeps the gap list's counter in its scratch area (its own layout, restated)
static const u32 *gap_count_in(const void *scratch, int table, u32 extra) {
  const u64 n_keys = ext_keys(table, extra), n_base = ext_keys(table, 0);
  uintptr_t p = reinterpret_cast<uintptr_t>(scratch) + (n_keys + 1) * 4;
  p = (p + 63) & ~static_cast<uintptr_t>(63);
  p += ((n_base + 31) / 32 + 1) * 4;
  p = (p + 63) & ~static_cast<uintptr_t>(63);
  return reinterpret_cast<const u32 *>(p);
}

static const u32 kExtras[3][3] = {{1, 3, 6}, {1, 2, 3}, {1, 2, 3}};
constexpr u32 kSmallGapCap = 8;

static int require_liveness(const Live live[3], bool print_only) {
  for (int t = 0; t < 3; ++t) {
    const Live &l = live[t];
    printf(" %s: keys compared %ld in %ld buckets, finished before the last letter %ld, emptied and stepped back %ld, still open %ld, entries with a blank tabulated letter %ld, "
           "gaps filled inline %ld / through the list %ld, index entries inside their own key's range %ld;", kTableName[t], l.keys, l.buckets, l.early, l.stepped, l.open, l.blank,
           l.gaps_inline, l.gaps_list, l.entries_inside);
    // ("finished before the last letter" is printed, not required here: whether a bucket splits within its first letters depends
    // on maxc -- the caller requires it per table over the values of maxc it runs, tests/test_gpu_index_derived.py)
    if (!print_only && (!l.stepped || !l.open || !l.blank || !l.gaps_inline || !l.gaps_list)) { printf("\nFAIL tables coverage, %s table\n", kTableName[t]); return 1; }
  }
  return 0;
}

static int cmd_expect(const HostIndex &h, u32 maxc) {
  Live live[3];
  long fallback = 0; bool misplaced = false;
  for (int table = 0; table < 3; ++table)
    for (u32 extra : kExtras[table]) {
      Expect x;
      expect_table(h, table, extra, maxc, x, live[table]);
      misplaced |= x.misplaced;
    }
  for (int t = 0; t < 3; ++t) fallback += live[t].fallback_buckets;
  printf("OK expect maxc %u fallback_buckets=%ld misplaced=%d;", maxc, fallback, misplaced);
  require_liveness(live, true);
  printf("\n");
  return 0;
}

static int cmd_tables(const HostIndex &h, u32 maxc, bool need_live) {
  Dev d;
  if (upload_index(h, d)) return 1;
  for (int t = 0; t < 3; ++t) {
    const std::vector<u32> &counter = t == 0 ? h.counter : (t == 1 ? h.counter_t : h.counter_a);
    if (counter.size() - 1 != ext_keys(t, 0)) { printf("FAIL tables: the file's %s counter array has %zu buckets\n", kTableName[t], counter.size() - 1); return 1; }
  }
  size_t max_keys = 0, max_scratch = 0;
  for (int t = 0; t < 3; ++t) for (u32 e : kExtras[t]) { max_keys = std::max<size_t>(max_keys, ext_keys(t, e)); max_scratch = std::max(max_scratch, ext_scratch_bytes(t, e)); }
  uint2 *d_a, *d_b, *d_listed;
  void *d_scratch;
  u32 *d_fail, *d_bases;
  unsigned long long *d_count;
  HIP_OK(hipMalloc(&d_a, max_keys * 8)); HIP_OK(hipMalloc(&d_b, max_keys * 8));
  HIP_OK(hipMalloc(&d_scratch, max_scratch));
  HIP_OK(hipMalloc(&d_fail, 64)); HIP_OK(hipMalloc(&d_count, 64));
  Live live[3];
  long fails = 0, fallback = 0, overflowed = 0;
  double t_host = 0, t_dev = 0;
  for (int table = 0; table < 3; ++table)
    for (u32 extra : kExtras[table]) {
      const u64 n_keys = ext_keys(table, extra), span = h_span(table, extra);
      double t0 = now_s();
      Expect x;
      expect_table(h, table, extra, maxc, x, live[table]);
      t_host += now_s() - t0; t0 = now_s();
      // the table twice: with the product's gap list, and with one of 8 slots (the "list full" branch of ext_bounds_kernel)
      u32 fail[2] = {0, 0}, gap_count[2] = {0, 0};
      for (int run = 0; run < 2; ++run) {
        uint2 *out = run == 0 ? d_a : d_b;
        HIP_OK(hipMemset(out, 0xFF, n_keys * 8));  // (a key left unwritten shows as a non-zero second word)
        HIP_OK(hipMemset(d_fail, 0, 64));
        if (run == 0) HIP_OK(build_ext_table(d.ix, table, extra, maxc, d.n_idx[table], out, d_scratch, d_fail, nullptr));
        else HIP_OK(build_ext_table(d.ix, table, extra, maxc, d.n_idx[table], out, d_scratch, d_fail, nullptr, kSmallGapCap));
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(&fail[run], d_fail, 4, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(&gap_count[run], gap_count_in(d_scratch, table, extra), 4, hipMemcpyDeviceToHost));
      }
      if ((fail[0] != 0) != x.misplaced || (fail[1] != 0) != x.misplaced) {
        printf("FAIL tables (%s + %u letters): fail = %u / %u, and the host finds %s entry outside the bucket its letters name\n", kTableName[table], extra, fail[0], fail[1], x.misplaced ? "an" : "no");
        return 1;
      }
      if (x.misplaced) { ++fails; t_dev += now_s() - t0; continue; }  // (no table at all: nothing else is required)
      unsigned long long differing = 0, nonzero = 0;
      HIP_OK(hipMemset(d_count, 0, 64));
      hipLaunchKernelGGL(count_differing_kernel, grid_for(n_keys), dim3(256), 0, 0, d_a, d_b, n_keys, d_count);
      hipLaunchKernelGGL(count_nonzero_kernel, grid_for(n_keys), dim3(256), 0, 0, d_a, n_keys, d_count + 1);
      HIP_OK(hipGetLastError());
      HIP_OK(hipDeviceSynchronize());
      HIP_OK(hipMemcpy(&differing, d_count, 8, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(&nonzero, d_count + 1, 8, hipMemcpyDeviceToHost));
      if (differing) { printf("FAIL tables (%s + %u letters): %llu keys differ between the build with the product's gap list and the one with %u slots\n", kTableName[table], extra, differing, kSmallGapCap); return 1; }
      if (gap_count[0] > kExtGapCap) { printf("FAIL tables (%s + %u letters): the product's gap list overflowed (%u gaps)\n", kTableName[table], extra, gap_count[0]); return 1; }
      if (gap_count[0] != x.long_gaps || gap_count[1] != x.long_gaps) {
        printf("FAIL tables (%s + %u letters): %u gaps went to the product's list, %u to the small one; the keys have %u gaps of more than %u\n", kTableName[table], extra, gap_count[0], gap_count[1], x.long_gaps, kGapInline);
        return 1;
      }
      if (gap_count[1] > kSmallGapCap) ++overflowed;
      else if (need_live) { printf("FAIL tables (%s + %u letters): the list of %u slots did not overflow (%u long gaps)\n", kTableName[table], extra, kSmallGapCap, gap_count[1]); return 1; }
      // the keys under non-empty base buckets, entry by entry
      const u64 n_listed = x.bases.size();
      std::vector<uint2> got(n_listed * span);
      if (n_listed) {
        HIP_OK(hipMalloc(&d_bases, n_listed * 4)); HIP_OK(hipMalloc(&d_listed, n_listed * span * 8));
        HIP_OK(hipMemcpy(d_bases, x.bases.data(), n_listed * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(gather_kernel, dim3(static_cast<u32>((n_listed * span + 255) / 256)), dim3(256), 0, 0, d_a, d_bases, n_listed, static_cast<u32>(span), d_listed);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(got.data(), d_listed, n_listed * span * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d_bases)); HIP_OK(hipFree(d_listed));
      }
      for (u64 i = 0; i < n_listed * span; ++i)
        if (got[i].x != x.entry[i].x || got[i].y != x.entry[i].y) {
          const uint2 g = got[i], w = x.entry[i];
          printf("FAIL tables (%s + %u letters, maxc %u): key %llu (base bucket %u%s): entry lo %u size %u len %u state %u; the reference's loop gives lo %u size %u len %u state %u\n",
                 kTableName[table], extra, maxc, (unsigned long long)(static_cast<u64>(x.bases[i / span]) * span + i % span), x.bases[i / span], x.descent[i / span] ? ", with a descent" : "",
                 g.x, g.y & 0x7FFFFFFu, (g.y >> 27) & 7u, g.y >> 30, w.x, w.y & 0x7FFFFFFu, (w.y >> 27) & 7u, w.y >> 30);
          return 1;
        }
      // all other keys (empty base buckets): size 0, len 0, state 0 -- counted on the device, over the whole table
      if (nonzero != x.nonzero) {
        printf("FAIL tables (%s + %u letters): %llu of the table's %llu keys have a non-zero second word, %llu of them under non-empty base buckets: keys of empty buckets are not empty (or not written)\n",
               kTableName[table], extra, nonzero, (unsigned long long)n_keys, (unsigned long long)x.nonzero);
        return 1;
      }
      // every index entry of a bucket without a descent lies inside the range of the entry at its own letters' key
      const std::vector<u32> &index = table == 0 ? h.index : (table == 1 ? h.index_t : h.index_a);
      const std::vector<u32> &counter = table == 0 ? h.counter : (table == 1 ? h.counter_t : h.counter_a);
      for (u64 i = 0; i < n_listed; ++i) {
        if (x.descent[i]) continue;
        for (u32 k = counter[x.bases[i]]; k < counter[x.bases[i] + 1]; ++k) {
          const u64 K = h_key(h.genome, index[k], key_weight(table) + extra, table);
          const uint2 g = got[i * span + K % span];
          if (!(g.x <= k && k < g.x + (g.y & 0x7FFFFFFu))) { printf("FAIL tables (%s + %u letters): index entry %u lies outside [%u, %u + %u) of its own key %llu\n", kTableName[table], extra, k, g.x, g.x, g.y & 0x7FFFFFFu, (unsigned long long)K); return 1; }
          ++live[table].entries_inside;
        }
      }
      t_dev += now_s() - t0;
    }
  for (int t = 0; t < 3; ++t) fallback += live[t].fallback_buckets;
  printf("OK tables maxc %u: fail=%ld fallback_buckets=%ld overflowed=%ld of 9 configurations x 2 gap lists;", maxc, fails, fallback, overflowed);
  if (require_liveness(live, !need_live)) return 1;
  printf(" host %.2f s, device and comparison %.2f s\n", t_host, t_dev);
  return 0;
}

// one base bucket of 2^27 + 1 entries (no file): its keys are "not tabulated" (a size does not fit 27 bits), every other key is empty
static int cmd_bigbucket() {
  const u64 n_idx = (1ull << 27) + 1;
  const u32 extra = 1, pos = 100;
  const int table = 0;
  std::vector<u64> genome(64, 0x1248124812481248ull);
  const u64 key = h_key(genome, pos, kKeyWeight + extra, table), base = key >> extra, n_base = ext_keys(table, 0), n_keys = ext_keys(table, extra);
  std::vector<u32> counter(n_base + 1);
  for (u64 b = 0; b <= n_base; ++b) counter[b] = b <= base ? 0u : static_cast<u32>(n_idx);
  Dev d;
  if (upload(genome, 64, &d.ix.genome) || upload(counter, 64, &d.ix.counter)) return 1;
  u32 *d_index;
  HIP_OK(hipMalloc(&d_index, n_idx * 4));
  { std::vector<u32> index(n_idx, pos); HIP_OK(hipMemcpy(d_index, index.data(), n_idx * 4, hipMemcpyHostToDevice)); }
  d.ix.index = d_index;
  uint2 *d_out; void *d_scratch; u32 *d_fail; unsigned long long *d_count;
  HIP_OK(hipMalloc(&d_out, n_keys * 8)); HIP_OK(hipMemset(d_out, 0xFF, n_keys * 8));
  HIP_OK(hipMalloc(&d_scratch, ext_scratch_bytes(table, extra)));
  HIP_OK(hipMalloc(&d_fail, 64)); HIP_OK(hipMemset(d_fail, 0, 64));
  HIP_OK(hipMalloc(&d_count, 64)); HIP_OK(hipMemset(d_count, 0, 64));
  const double t0 = now_s();
  HIP_OK(build_ext_table(d.ix, table, extra, 100, n_idx, d_out, d_scratch, d_fail, nullptr));
  hipLaunchKernelGGL(count_nonzero_kernel, grid_for(n_keys), dim3(256), 0, 0, d_out, n_keys, d_count);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  u32 fail = 1; unsigned long long nonzero = 0; uint2 got[2];
  HIP_OK(hipMemcpy(&fail, d_fail, 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(&nonzero, d_count, 8, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(got, d_out + 2 * base, 16, hipMemcpyDeviceToHost));
  if (fail) { printf("FAIL bigbucket: fail = %u\n", fail); return 1; }
  for (int k = 0; k < 2; ++k)
    if (got[k].x != 0 || got[k].y != (2u << 30)) { printf("FAIL bigbucket: key %llu holds {%u, %u}, expected {0, 2 << 30}\n", (unsigned long long)(2 * base + k), got[k].x, got[k].y); return 1; }
  if (nonzero != 2) { printf("FAIL bigbucket: %llu keys have a non-zero second word, expected the bucket's 2\n", nonzero); return 1; }
  printf("OK bigbucket: %llu entries in base bucket %llu, its 2 keys not tabulated, the other %llu empty; %.2f s\n", (unsigned long long)n_idx, (unsigned long long)base, (unsigned long long)(n_keys - 2), now_s() - t0);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 3) { printf("FAIL usage: index_derived_check <index file | -> planes | records | tables <maxc> [sorted] | expect <maxc> | bigbucket\n"); return 2; }
  const std::string cmd = argv[2];
  if (cmd == "planes") return cmd_planes();
  if (cmd == "bigbucket") return cmd_bigbucket();
  HostIndex h;
  try { h.load(argv[1]); }
  catch (const std::exception &e) { printf("FAIL %s\n", e.what()); return 1; }
  if (h.multibit_genome) { printf("FAIL the index has IUPAC letters\n"); return 1; }
  if (cmd == "records") return cmd_records(h);
  if ((cmd == "tables" || cmd == "expect") && argc >= 4) {
    const u32 maxc = static_cast<u32>(std::atoi(argv[3]));
    if (cmd == "expect") return cmd_expect(h, maxc);
    return cmd_tables(h, maxc, argc >= 5 && std::string(argv[4]) == "sorted");
  }
  printf("FAIL unknown sub-command %s\n", cmd.c_str());
  return 2;
}
