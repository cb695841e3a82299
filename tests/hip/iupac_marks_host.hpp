// Host half of tests/hip/iupac_marks_check.hip, plain C++ (tests/hip/iupac_marks_host_main.cpp runs it without a device):
// hand-built genomes with blank and multi-bit nibbles at chunk, block and genome boundaries, and what the two builders must
// make of them, written from the rules alone:
//   nmap     chunk c is flagged if some position in it has a marked nibble within kPlaneReach bases at or after it
//            (complete), and only if one has such a nibble within kPlaneReach + 63 (tight: the builder works by 64-base blocks)
//   records  the spare bit of entry e's record of `blocks` blocks says whether [e - back, e - back + 64 blocks - 1) holds a
//            marked nibble or a base past the genome -- or, with mark_multi, whether one of the 15 bases after that stretch
//            (inside the genome) has two or more bits: full_compare sums whole 16-base words, the read's last one padded with
//            0xF, and only a multi-bit nibble under that padding can lower the sum
// marked = blank (no bit) inside the genome, and with mark_multi also two or more bits.  Nothing is taken from the kernels.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace marks {

constexpr uint32_t kChunkBits = 12, kReach = 512, kBlock = 64, kKeyWeightHere = 25;

struct Genome {
  std::string name;
  uint64_t n_bases;
  std::vector<uint8_t> nib;           // n_bases + 64 nibbles (those past n_bases do not belong to the genome)
  std::vector<uint64_t> letters;      // positions of the multi-bit nibbles inside the genome
};

inline bool is_marked(const Genome &g, uint64_t q, bool mark_multi) {
  if (q >= g.n_bases) return false;
  const uint32_t n = g.nib[q];
  return n == 0 || (mark_multi && __builtin_popcount(n) > 1);
}

inline Genome make(const std::string &name, uint64_t n_bases, uint64_t seed, const std::vector<uint64_t> &blanks,
                   const std::vector<uint64_t> &letters) {
  Genome g{name, n_bases, std::vector<uint8_t>(n_bases + 64, 0), {}};
  uint64_t s = seed;
  for (uint64_t k = 0; k < n_bases; ++k) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; g.nib[k] = static_cast<uint8_t>(1u << ((s >> 20) & 3)); }
  for (uint64_t p : blanks) g.nib[p] = 0;
  static const uint8_t codes[10] = {5, 10, 3, 12, 6, 9, 14, 13, 11, 7};  // R Y M K S W B D H V
  for (size_t k = 0; k < letters.size(); ++k) { g.nib[letters[k]] = codes[k % 10]; g.letters.push_back(letters[k]); }
  g.nib[n_bases] = 3; g.nib[n_bases + 9] = 15;  // (multi-bit nibbles past the last base must not count)
  return g;
}

// 16 chunks of 4,096 bases and a ragged end.  Letters (chunk c = 4096 c ...):
//   4096 * 2 - 1, 4096 * 2, 4096 * 2 + 1     just before, on and just after a chunk boundary
//   4096 * 5 + 511, + 512, + 513             around the reach: the first flags chunk 4 by reach alone, the others chunk 5 only
//   4096 * 8 + 447, + 448, + 449             around a block boundary; within reach of chunk 7's last positions
//   4096 * 11 + 63, + 64, + 65               around the first block boundary of a chunk; within reach of chunk 10
//   n_bases - 1                              the genome's last base (chunk 16, and 15 by reach)
// and one blank at 4096 * 13 + 700 (chunk 13 alone).  Chunks 0, 3, 6, 9, 12, 14 stay clear in every genome.
inline std::vector<Genome> genomes() {
  const uint64_t n = 4096 * 16 + 37;
  const std::vector<uint64_t> blanks = {4096 * 13 + 700};
  std::vector<Genome> gs;
  gs.push_back(make("with letters at chunk and block boundaries", n, 0x1234567ull, blanks,
                    {4096 * 2 - 1, 4096 * 2, 4096 * 2 + 1, 4096 * 5 + 511, 4096 * 5 + 512, 4096 * 5 + 513, 4096 * 8 + 447, 4096 * 8 + 448,
                     4096 * 8 + 449, 4096 * 11 + 63, 4096 * 11 + 64, 4096 * 11 + 65, n - 1}));
  gs.push_back(make("with one letter just before a chunk boundary", n, 0x7654321ull, blanks, {4096 * 2 - 1}));
  gs.push_back(make("with one letter on a chunk boundary", n, 0x7654321ull, blanks, {4096 * 2}));
  gs.push_back(make("with one letter on the last base", n, 0x7654321ull, blanks, {n - 1}));
  gs.push_back(make("with blanks only", n, 0x7654321ull, {4096 * 13 + 700, 4096 * 5 + 511}, {}));
  return gs;
}

struct ChunkRule { std::vector<uint8_t> must, may; long n_must = 0; };
inline ChunkRule chunk_rule(const Genome &g, bool mark_multi, uint64_t n_chunks) {
  const uint64_t span = n_chunks << kChunkBits;
  std::vector<uint64_t> next(span + 1, ~0ull);
  for (uint64_t p = span; p-- > 0;) next[p] = is_marked(g, p, mark_multi) ? p : next[p + 1];
  ChunkRule r{std::vector<uint8_t>(n_chunks, 0), std::vector<uint8_t>(n_chunks, 0), 0};
  for (uint64_t c = 0; c < n_chunks; ++c) {
    for (uint64_t p = c << kChunkBits; p < (c + 1) << kChunkBits; ++p) {
      if (next[p] == ~0ull) continue;
      if (next[p] - p <= kReach) r.must[c] = 1;
      if (next[p] - p <= kReach + 63) r.may[c] = 1;
    }
    r.n_must += r.must[c];
  }
  return r;
}

inline uint32_t record_max_len(uint32_t blocks) { return (64u * blocks + kKeyWeightHere) / 2u; }
inline uint32_t record_back(uint32_t blocks) { return record_max_len(blocks) - kKeyWeightHere; }
inline bool record_flag(const Genome &g, uint32_t entry, uint32_t blocks, bool mark_multi) {
  const long long first = static_cast<long long>(entry) - record_back(blocks), end = first + 64ll * blocks - 1;
  for (long long q = first < 0 ? 0 : first; q < end; ++q)
    if (static_cast<uint64_t>(q) >= g.n_bases || is_marked(g, static_cast<uint64_t>(q), mark_multi)) return true;
  if (mark_multi)
    for (long long q = end < 0 ? 0 : end; q < end + 15; ++q)
      if (static_cast<uint64_t>(q) < g.n_bases && __builtin_popcount(g.nib[q]) > 1) return true;
  return false;
}
// entries whose stretch has the marked nibble at p on its first base, one base before it, on its last covered base and on
// the first base past it, 2, 4, 15 and 16 bases past its last covered base (under the padding of a window's last word: the
// first three flag it when the nibble has several bits, a blank there or a letter 16 bases on does not), and a few clear of it
inline std::vector<uint32_t> record_entries(const Genome &g, uint32_t blocks) {
  std::vector<uint32_t> e;
  const long long back = record_back(blocks), len = 64ll * blocks - 1;
  std::vector<uint64_t> at = g.letters;
  at.push_back(4096 * 13 + 700);
  for (uint64_t p : at)
    for (long long first : {static_cast<long long>(p), static_cast<long long>(p) + 1, static_cast<long long>(p) - len + 1, static_cast<long long>(p) - len,
                            static_cast<long long>(p) - len / 2, static_cast<long long>(p) + 300, static_cast<long long>(p) - len - 300,
                            static_cast<long long>(p) - len - 1, static_cast<long long>(p) - len - 3, static_cast<long long>(p) - len - 14,
                            static_cast<long long>(p) - len - 15})
      if (first + back >= 0 && static_cast<uint64_t>(first + back) < g.n_bases + 600) e.push_back(static_cast<uint32_t>(first + back));
  for (uint32_t k = 0; k < 64; ++k) e.push_back(static_cast<uint32_t>((k * 2654435761u) % g.n_bases));
  return e;
}

// the counts both halves print: chunks that must be flagged with and without the letters, records flagged with and without
struct Counts { long must_on = 0, must_off = 0, rec = 0, rec_on = 0, rec_off = 0, last_covered = 0, first_past = 0, under_padding = 0, past_padding = 0; };
inline Counts expected_counts() {
  Counts c;
  for (const Genome &g : genomes()) {
    const uint64_t n_chunks = (g.n_bases >> kChunkBits) + 1;
    c.must_on += chunk_rule(g, true, n_chunks).n_must;
    c.must_off += chunk_rule(g, false, n_chunks).n_must;
    for (uint32_t blocks : {3u, 4u, 5u})
      for (uint32_t e : record_entries(g, blocks)) {
        ++c.rec;
        c.rec_on += record_flag(g, e, blocks, true);
        c.rec_off += record_flag(g, e, blocks, false);
        const long long first = static_cast<long long>(e) - record_back(blocks), last = first + 64ll * blocks - 2;
        for (uint64_t p : g.letters) { c.last_covered += static_cast<long long>(p) == last; c.first_past += static_cast<long long>(p) == last + 1;
                                       c.under_padding += static_cast<long long>(p) > last && static_cast<long long>(p) <= last + 15; c.past_padding += static_cast<long long>(p) == last + 16; }
      }
  }
  return c;
}
inline void print_counts(const Counts &c) {
  std::printf("chunks_must_on=%ld chunks_must_off=%ld records=%ld records_flagged_on=%ld records_flagged_off=%ld letter_on_last_covered=%ld letter_on_first_past=%ld letter_under_padding=%ld letter_just_past_padding=%ld\n",
              c.must_on, c.must_off, c.rec, c.rec_on, c.rec_off, c.last_covered, c.first_past, c.under_padding, c.past_padding);
}

}  // namespace marks
