// The serial alignment reference (align_host.hpp) on its own, no device: a dozen alignments small enough to write out --
// score, CIGAR, position, the first maximum, indel totals, tie counts and the whole traceback table (one string per row,
// one digit per cell: arrow 0 M, 1 I, 2 D, 3 none, + 4 if the cell's score is > 0) -- and the publication of a CIGAR into
// a slot or the arena on hand-made sinks.  Letters: A 1, C 2, G 4, T 8, R = A|G, Y = C|T, N 0; the target string lies at
// position 64 of a genome of N, one base before it where a case says so.  Built with the host compiler under
// -fsanitize=address,undefined and run by tests/test_gpu_align_stages.py::test_host_dp_on_written_out_alignments.
#include "align_host.hpp"
#include <cstring>
#include <string>
using namespace align_host;

struct Hand {
  const char *name, *read, *target;
  int bw, score;
  const char *cigar;
  u32 pos;
  int br, bc, ins, del, left_ties, above_ties, three_ties;
  std::vector<const char *> table;
  char before;  // the base in front of the target string (0: N)
};
static const Hand kHands[] = {
  {"perfect match", "ACGTAC", "ACGTAC", 1, 12, "6M", 64, 6, 0, 0, 0, 0, 0, 0,
   {"3", "4", "4", "4", "4", "4", "4"}},
  {"perfect match, band 3", "ACGTAC", "ACGTAC", 3, 12, "6M", 64, 7, 1, 0, 0, 0, 0, 0,
   {"333", "333", "343", "341", "245", "645", "645", "643", "433"}},
  {"one mismatch", "ACGTACGT", "ACGAACGT", 3, 11, "8M", 64, 9, 1, 0, 0, 1, 0, 0,
   {"333", "333", "343", "341", "245", "644", "345", "645", "645", "643", "433"}},
  {"1-base insertion", "ACGTACTGGATCCA", "ACGTACGGATCCA", 3, 22, "6M1I7M", 64, 14, 2, 1, 0, 0, 4, 0,
   {"333", "333", "343", "341", "245", "645", "645", "645", "644", "644", "664", "664", "664", "664", "664", "643", "433"}},
  {"3-base insertion", "ACGTACGTCAGGTTTGGATCCAGTCA", "ACGTACGTCAGGGGATCCAGTCA", 7, 34, "12M3I11M", 64, 26, 6, 3, 0, 12, 26, 5,
   {"3333333", "3333333", "3333333", "3333333", "3334333", "3334133", "3324533", "3364513", "3364553", "3264554", "3664555", "3664555", "4664555", "6664555", "6664555", "6664555", "6664554", "6664544", "6664564", "4445564", "6645664", "6645664", "6645664", "4646664", "6456664", "6456664", "6466664", "6666643", "6666433", "6664333", "6643333", "6433333", "4333333"}},
  {"1-base deletion", "ACGTACGGATCCA", "ACGTACTGGATCCA", 3, 22, "6M1D7M", 64, 15, 0, 0, 1, 4, 0, 0,
   {"333", "333", "343", "341", "245", "645", "645", "645", "645", "445", "455", "455", "455", "455", "453", "433"}},
  {"3-base deletion", "ACGTACGTCAGGGGATCCAGTCA", "ACGTACGTCAGGTTTGGATCCAGTCA", 7, 34, "12M3D11M", 64, 29, 0, 0, 3, 24, 14, 5,
   {"3333333", "3333333", "3333333", "3333333", "3334333", "3334133", "3324533", "3364513", "3364553", "3264554", "3664555", "3664555", "4664555", "6664555", "6664555", "6664555", "6664554", "6664545", "6664455", "4456455", "4556454", "4555455", "4555445", "4555545", "4555543", "4555533", "4555333", "4553333", "4533333", "4333333"}},
  {"soft-clipped head", "TTACGTAC", "GGACGTAC", 3, 12, "2S6M", 66, 9, 1, 0, 0, 0, 0, 0,
   {"333", "333", "333", "333", "343", "341", "245", "645", "645", "643", "433"}},
  {"soft-clipped tail", "ACGTACTT", "ACGTACGG", 3, 12, "6M2S", 64, 7, 1, 0, 0, 1, 1, 0,
   {"333", "333", "343", "341", "245", "645", "645", "645", "645", "643", "433"}},
  {"soft-clipped head and tail", "TTACGTACTT", "GGACGTACGG", 3, 12, "2S6M2S", 66, 9, 1, 0, 0, 1, 1, 0,
   {"333", "333", "333", "333", "343", "341", "245", "645", "645", "645", "645", "643", "433"}},
  {"all mismatches", "AAAAAA", "CCCCCC", 3, 0, "6M", 64, 0, 0, 0, 0, 0, 0, 0,
   {"333", "333", "333", "333", "333", "333", "333", "333", "333"}},
  {"IUPAC target letters", "ACGTAC", "RCGYAC", 1, 12, "6M", 64, 6, 0, 0, 0, 0, 0, 0,
   {"3", "4", "4", "4", "4", "4", "4"}},
  {"three-way tie", "CTCTAGT", "TCTATAC", 3, 8, "1S4M2S", 64, 5, 2, 0, 0, 2, 1, 1,
   {"333", "333", "334", "434", "414", "464", "464", "454", "433", "333"}, 'A'},
};

static unsigned char nib(char c) {
  switch (c) { case 'A': return 1; case 'C': return 2; case 'G': return 4; case 'T': return 8; case 'R': return 5; case 'Y': return 10; default: return 0; }
}
static std::string text(const std::vector<u32> &c) {
  std::string s;
  for (u32 o : c) { s += std::to_string(o >> 4); s += "MIDNS"[o & 15u]; }
  return s;
}
static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAIL "); std::printf(__VA_ARGS__); std::printf("\n"); ++fails; } } while (0)

int main() {
  int n_tables = 0, n_cells = 0;
  for (const Hand &h : kHands) {
    const u32 pos = 64;
    G.assign(512, 0);
    for (size_t k = 0; k < std::strlen(h.target); ++k) G[pos + k] = nib(h.target[k]);
    if (h.before) G[pos - 1] = nib(h.before);
    std::vector<unsigned char> q;
    for (const char *c = h.read; *c; ++c) q.push_back(nib(*c));
    const int L = static_cast<int>(q.size());
    for (int wrap = 0; wrap < 2; ++wrap) {  // (scores this small are the same in 16 bits)
      const Aligned a = host_align(q.data(), L, pos, h.bw, true, wrap != 0, true);
      CHECK(a.score == h.score, "%s: score %d, written %d", h.name, a.score, h.score);
      CHECK(text(a.cigar) == h.cigar, "%s: CIGAR %s, written %s", h.name, text(a.cigar).c_str(), h.cigar);
      CHECK(a.pos == h.pos && a.br == h.br && a.bc == h.bc, "%s: pos %u maximum (%d, %d), written %u (%d, %d)", h.name, a.pos, a.br, a.bc, h.pos, h.br, h.bc);
      CHECK(a.ins == h.ins && a.del == h.del, "%s: ins %d del %d, written %d %d", h.name, a.ins, a.del, h.ins, h.del);
      CHECK(a.left_ties == h.left_ties && a.above_ties == h.above_ties && a.three_ties == h.three_ties, "%s: ties %d %d %d, written %d %d %d", h.name,
            a.left_ties, a.above_ties, a.three_ties, h.left_ties, h.above_ties, h.three_ties);
      CHECK(static_cast<int>(h.table.size()) == L + h.bw, "%s: %zu rows written, the table has %d", h.name, h.table.size(), L + h.bw);
      for (int i = 0; i < L + h.bw && i < static_cast<int>(h.table.size()); ++i)
        for (int j = 0; j < h.bw; ++j) {
          CHECK(a.T[static_cast<size_t>(i) * h.bw + j] == h.table[i][j] - '0', "%s: cell (%d, %d) is %d, written %c", h.name, i, j, a.T[static_cast<size_t>(i) * h.bw + j], h.table[i][j]);
          ++n_cells;
        }
      // each column's best value is the score in the column that holds the maximum, and never above it
      for (int j = 0; j < h.bw; ++j) CHECK(a.colbest[j] <= a.score && (j != a.bc || (a.colbest[j] == a.score && a.colrow[j] == a.br)), "%s: column %d best %d row %d", h.name, j, a.colbest[j], a.colrow[j]);
      // the scoring run (no traceback) gives the same score and the default CIGAR
      const Aligned s = host_align(q.data(), L, pos, h.bw, false, wrap != 0);
      CHECK(s.score == h.score && s.cigar.size() == 1 && s.cigar[0] == static_cast<u32>(L) << 4, "%s: scoring run %d", h.name, s.score);
      ++n_tables;
    }
  }

  // publication: the CIGAR 2S 5M 1I 6M 1D 4M 3S (7 ops, 5 without the clips) on hand-made sinks
  Aligned a{};
  a.cigar = {(2u << 4) | 4u, 5u << 4, (1u << 4) | 1u, 6u << 4, (1u << 4) | 2u, 4u << 4, (3u << 4) | 4u};
  a.clip_head = 2; a.clip_tail = 3; a.n_body = 5;
  const u32 X = kUnwritten;
  struct Pub { const char *name; HostSink sink; u32 n_ops; bool overflow; std::vector<u32> slot; bool in_arena; u32 at, count; size_t fin; };
  const Pub pubs[] = {
    {"room in the slot", {8, 21, true, 100, 40, true}, 7, false, {a.cigar[0], a.cigar[1], a.cigar[2], a.cigar[3], a.cigar[4], a.cigar[5], a.cigar[6], X}, false, 0, 40, 7},
    {"fills the slot", {7, 21, false, 0, 0, false}, 7, false, a.cigar, false, 0, 0, 0},
    {"one op too many, arena with room", {6, 21, true, 100, 40, true}, 7, false, {40, X, X, X, X, X}, true, 40, 47, 7},
    {"arena fits exactly", {6, 21, true, 47, 40, false}, 7, false, {40, X, X, X, X, X}, true, 40, 47, 0},
    {"arena one op short", {6, 21, true, 46, 40, false}, 7, true, {a.cigar[0], a.cigar[1], a.cigar[2], a.cigar[3], a.cigar[4], a.cigar[5]}, false, 40, 47, 0},
    {"counter past the arena", {3, 21, true, 46, 50, true}, 7, true, {a.cigar[0], a.cigar[1], a.cigar[2]}, false, 50, 57, 3},
    {"no arena", {2, 21, false, 0, 0, false}, 7, true, {a.cigar[0], a.cigar[1]}, false, 0, 0, 0},
    {"the walk kept three ops of five", {6, 3, true, 100, 40, false}, 7, true, {a.cigar[0], a.cigar[3], a.cigar[4], a.cigar[5], a.cigar[6], X}, false, 0, 40, 0},
  };
  for (const Pub &p : pubs) {
    const Published g = host_publish(a, p.sink);
    CHECK(g.n_ops == p.n_ops && g.overflow == p.overflow && g.slot == p.slot && g.in_arena == p.in_arena && (!p.in_arena || g.arena_at == p.at) &&
          g.arena_count == p.count && g.fin.size() == p.fin, "publish, %s: ops %u overflow %d in arena %d at %u counter %u fin %zu", p.name, g.n_ops, g.overflow,
          g.in_arena, g.arena_at, g.arena_count, g.fin.size());
    for (size_t k = 0; k < g.fin.size(); ++k) CHECK(g.fin[k] == (g.overflow ? g.slot[k] : a.cigar[k]), "publish, %s: fin[%zu]", p.name, k);
  }

  // NM and the length test, by hand: 100 bases, score 200 - 5 per mismatch
  CHECK(host_nm(200, 100, 0, 0) == 0 && host_nm(190, 100, 0, 0) == 2 && host_nm(0, 100, 0, 0) == 100, "NM without indels");
  CHECK(host_nm(2 * 99 - 4, 100, 1, 0) == 1 && host_nm(2 * 100 - 8 - 5, 100, 0, 2) == 3, "NM with indels");  // 99 M + 1 I; 100 M, one a mismatch, + 2 D
  CHECK(host_long_enough(60, 100, 32) && !host_long_enough(59, 100, 32) && !host_long_enough(31, 40, 32) && host_long_enough(32, 40, 32), "the length test");
  CHECK(host_band(0, 10) == 1 && host_band(3, 10) == 7 && host_band(12, 10) == 21 && host_band(40, 100) == 61 && host_band(-5, 10) == 61, "bands");
  if (fails) return 1;
  std::printf("OK host %d tables, %d cells, %zu sinks\n", n_tables, n_cells, sizeof(pubs) / sizeof(pubs[0]));
  return 0;
}
