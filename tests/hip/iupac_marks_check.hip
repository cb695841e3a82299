// GPU test program (built and run by tests/test_gpu_iupac_marks.py): the marks a genome with IUPAC letters gets at upload when
// abm_index_set_iupac_planes is on -- nmap from make_planes_kernel, the window records' spare bits from window_records_kernel
// -- each builder run alone on the hand-built genomes of iupac_marks_host.hpp and compared chunk by chunk / entry by entry with
// that header's serial host code.  With the marking off (today's arguments) the outputs must be today's: blanks only.
// Prints "OK <counts>" (the host half's own counts line) or the first mismatch.
#include "../../abismal_amd/csrc/abm_kernels.hip"
#include "../../abismal_amd/csrc/abm_ext.hip"
#include "iupac_marks_host.hpp"
#include <cstdlib>
using namespace abm;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("FAIL hip call at line %d: %s\n", __LINE__, hipGetErrorString(e_)); return 1; } } while (0)

static_assert(marks::kChunkBits == kPlaneChunkBits && marks::kReach == kPlaneReach && marks::kBlock == kPlaneBlock && marks::kKeyWeightHere == kKeyWeight,
              "the host half restates the device's constants");

static u32 code_of(u32 nib) { return nib ? static_cast<u32>(__builtin_ctz(nib)) : 0u; }

static int check_genome(const marks::Genome &g, bool mark_multi) {
  const u64 n_bases = g.n_bases, n_words = (n_bases + 15) / 16 + 4;
  std::vector<u64> gw(n_words, 0);
  for (u64 k = 0; k < g.nib.size(); ++k) gw[k / 16] |= static_cast<u64>(g.nib[k]) << (4 * (k % 16));
  const u64 n_blocks = (n_bases + kPlaneBlock - 1) / kPlaneBlock + 16, nmap_words = ((n_bases >> kPlaneChunkBits) + 64) / 32 + 1;
  u64 *d_genome, *d_p0, *d_p1;
  u32 *d_nmap, *d_bad;
  HIP_OK(hipMalloc(&d_genome, n_words * 8));
  HIP_OK(hipMemcpy(d_genome, gw.data(), n_words * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMalloc(&d_p0, n_blocks * 16)); HIP_OK(hipMemset(d_p0, 0xA5, n_blocks * 16));
  HIP_OK(hipMalloc(&d_p1, n_blocks * 16)); HIP_OK(hipMemset(d_p1, 0x5A, n_blocks * 16));
  HIP_OK(hipMalloc(&d_nmap, nmap_words * 4)); HIP_OK(hipMemset(d_nmap, 0, nmap_words * 4));
  HIP_OK(hipMalloc(&d_bad, 64)); HIP_OK(hipMemset(d_bad, 0, 64));
  if (mark_multi) HIP_OK(launch_make_planes(d_genome, n_words, n_bases, n_blocks, d_p0, d_p1, d_nmap, d_bad, nullptr, 1u));
  else HIP_OK(launch_make_planes(d_genome, n_words, n_bases, n_blocks, d_p0, d_p1, d_nmap, d_bad, nullptr));  // (today's arguments)
  HIP_OK(hipDeviceSynchronize());
  std::vector<u64> p0(2 * n_blocks), p1(2 * n_blocks);
  std::vector<u32> nmap(nmap_words);
  u32 bad = 7;
  HIP_OK(hipMemcpy(p0.data(), d_p0, n_blocks * 16, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(p1.data(), d_p1, n_blocks * 16, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(nmap.data(), d_nmap, nmap_words * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost));
  const char *mode = mark_multi ? "marking on" : "marking off";
  if ((bad != 0) != !g.letters.empty()) { printf("FAIL genome %s, %s: bad flag %u with %zu letters inside\n", g.name.c_str(), mode, bad, g.letters.size()); return 1; }
  // the planes: both copies, every one-hot or blank nibble's code (a multi-bit nibble's code is arbitrary)
  for (u64 b = 0; b < n_blocks; ++b) {
    if (p0[2 * b] != p1[2 * b] || p0[2 * b + 1] != p1[2 * b + 1]) { printf("FAIL genome %s, %s: block %llu differs between the two copies\n", g.name.c_str(), mode, (unsigned long long)b); return 1; }
    for (u32 j = 0; j < 64; ++j) {
      const u64 q = 64 * b + j;
      const u32 nb = q < g.nib.size() ? g.nib[q] : 0u;
      if (__builtin_popcount(nb) > 1) continue;
      const u32 got = static_cast<u32>((p0[2 * b] >> j) & 1u) | (static_cast<u32>((p0[2 * b + 1] >> j) & 1u) << 1);
      if (got != code_of(nb)) { printf("FAIL genome %s, %s: base %llu (nibble %u) has code %u\n", g.name.c_str(), mode, (unsigned long long)q, nb, got); return 1; }
    }
  }
  // nmap, complete and tight
  const u64 n_chunks = nmap_words * 32;
  const marks::ChunkRule rule = marks::chunk_rule(g, mark_multi, n_chunks);
  for (u64 c = 0; c < n_chunks; ++c) {
    const bool got = (nmap[c >> 5] >> (c & 31)) & 1u;
    if (rule.must[c] && !got) { printf("FAIL genome %s, %s: chunk %llu holds a position with a marked nibble within %u bases and is not flagged (nmap incomplete)\n", g.name.c_str(), mode, (unsigned long long)c, kPlaneReach); return 1; }
    if (got && !rule.may[c]) { printf("FAIL genome %s, %s: chunk %llu is flagged and no position in it has a marked nibble within %u + 63 bases (nmap not tight)\n", g.name.c_str(), mode, (unsigned long long)c, kPlaneReach); return 1; }
  }
  // the records' spare bits, entry by entry, for records of 3, 4 and 5 blocks
  for (u32 blocks : {3u, 4u, 5u}) {
    const std::vector<u32> entries = marks::record_entries(g, blocks);
    if (window_record_max_len(blocks) != marks::record_max_len(blocks)) { printf("FAIL the host half's record length for %u blocks\n", blocks); return 1; }
    u32 *d_e;
    u64 *d_wrec;
    HIP_OK(hipMalloc(&d_e, entries.size() * 4 + 64));
    HIP_OK(hipMemcpy(d_e, entries.data(), entries.size() * 4, hipMemcpyHostToDevice));
    const size_t bytes = window_record_bytes(entries.size(), blocks);
    HIP_OK(hipMalloc(&d_wrec, bytes));
    HIP_OK(hipMemset(d_wrec, 0xA5, bytes));
    DevIndex ix = {};
    ix.genome = d_genome; ix.planes[0] = d_p0; ix.planes[1] = d_p1; ix.nmap = d_nmap;
    ix.index = d_e; ix.index_t = d_e; ix.index_a = d_e;
    if (mark_multi) ix.multibit = 1;  // (left as DevIndex{} has it otherwise: today's arguments)
    const u64 n_idx[3] = {entries.size(), 0, 0};
    HIP_OK(build_window_records(ix, n_blocks, n_bases, n_idx, blocks, d_wrec, nullptr));
    HIP_OK(hipDeviceSynchronize());
    std::vector<u64> wrec(entries.size() * blocks * 2);
    HIP_OK(hipMemcpy(wrec.data(), d_wrec, wrec.size() * 8, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_e)); HIP_OK(hipFree(d_wrec));
    for (size_t k = 0; k < entries.size(); ++k) {
      const u64 *r = wrec.data() + 2 * k * blocks;
      const u32 lo = static_cast<u32>(r[2 * (blocks - 1)] >> 63), hi = static_cast<u32>(r[2 * (blocks - 1) + 1] >> 63);
      const bool want = marks::record_flag(g, entries[k], blocks, mark_multi);
      if (lo != (want ? 1u : 0u) || hi != 0) {
        printf("FAIL genome %s, %s, %u blocks: entry %zu at %u has spare bits %u (low) %u (high); its stretch %s a marked nibble or a base past the genome\n",
               g.name.c_str(), mode, blocks, k, entries[k], lo, hi, want ? "holds" : "holds no");
        return 1;
      }
    }
  }
  HIP_OK(hipFree(d_genome)); HIP_OK(hipFree(d_p0)); HIP_OK(hipFree(d_p1)); HIP_OK(hipFree(d_nmap)); HIP_OK(hipFree(d_bad));
  return 0;
}

int main() {
  const marks::Counts c = marks::expected_counts();
  for (const marks::Genome &g : marks::genomes())
    for (bool mark_multi : {false, true})
      if (check_genome(g, mark_multi)) return 1;
  printf("OK device ");
  marks::print_counts(c);
  return 0;
}
