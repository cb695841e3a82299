// The serial side of the filter checks (filter_host.hpp) on its own, no device: encodings, distances, the position cache,
// the candidate set and the ghost letters on cases small enough to write out.  Genome letters: A 1, C 2, G 4, T 8, Y = C|T,
// N 0.  Built with the host compiler under -fsanitize=address,undefined and run by
// tests/test_gpu_filter_stages.py::test_host_side_on_written_out_cases.
#include "filter_host.hpp"
#include <cstring>
using namespace filter_host;

static int fails = 0, checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { std::printf("FAIL "); std::printf(__VA_ARGS__); std::printf("\n"); ++fails; } } while (0)

static std::vector<u8> genome(const char *s) {
  std::vector<u8> g;
  for (; *s; ++s) g.push_back(*s == 'A' ? 1 : *s == 'C' ? 2 : *s == 'G' ? 4 : *s == 'T' ? 8 : *s == 'Y' ? 10 : 0);
  return g;
}

int main() {
  // ---- encodings -----------------------------------------------------------------------------------------------------
  {
    const Read r = encode("ACGTN");  // reverse complement: NACGT
    const u8 want[4][5] = {{1, 2, 4, 10, 0}, {5, 2, 4, 8, 0}, {0, 1, 2, 4, 10}, {0, 5, 2, 4, 8}};
    for (int e = 0; e < 4; ++e) for (int k = 0; k < 5; ++k) CHECK(r.nib[e][k] == want[e][k], "encode: encoding %d letter %d is %u", e, k, r.nib[e][k]);
    u64 w[8];
    pack(r, 2, w);
    CHECK(w[0] == 0xFFFFFFFFFFF0A421ull && w[1] == ~0ull, "pack: T-rich words %016llx %016llx", (unsigned long long)w[0], (unsigned long long)w[1]);
    CHECK(w[6] == 0xFFFFFFFFFFF84250ull, "pack: A-rich reverse word %016llx", (unsigned long long)w[6]);
    const std::vector<u64> gw = pack_genome(genome("ACGTNY"));
    CHECK(gw.size() == 1 && gw[0] == 0xA08421ull, "pack_genome: %016llx", (unsigned long long)gw[0]);
  }
  // ---- distances: the read ACGT (T-rich: 1, 2, 4, 10) in one word ----------------------------------------------------------
  {
    const Read r = encode("ACGT");
    struct { const char *g; u64 pos; int d, dmax, letters, planes; const char *what; } c[] = {
      {"ACGTACGTACGTACGTACGT", 0, 0, 0, 0, 0, "an exact copy"},
      {"ACGCACGTACGTACGTACGT", 0, 0, 0, 0, 0, "C under the read's T: the bisulfite match"},
      {"ACGGACGTACGTACGTACGT", 0, 1, 1, 1, 1, "G under the read's T"},
      {"TACGTACGTACGTACGTACGT", 1, 0, 0, 0, 0, "the copy one base on"},
      {"TACGTACGTACGTACGTACGT", 0, 4, 4, 4, 4, "the window one base off its copy"},
      {"NCGTACGTACGTACGTACGT", 0, 1, 1, 1, 0, "a blank under the read's A: the planes' code 0 is an A"},
      {"ACNTACGTACGTACGTACGT", 0, 1, 1, 1, 1, "a blank under the read's G"},
      {"ACGTACGTACNTACGTACGT", 0, 1, 1, 0, 0, "a blank under the padding: the word counts it, the letters do not"},
      {"ACGYACGTACGTACGTACGT", 0, -1, 0, 0, 0, "Y under the read's T shares two bits: the word's share is -1"},
      {"ACGT", 0, 12, 12, 0, 0, "the genome ends with the read: twelve blank nibbles under the padding"},
    };
    for (const auto &k : c) {
      const std::vector<u8> g = genome(k.g);
      const Dist d = serial_distance(g, r.nib[0], k.pos, 1);
      CHECK(d.d == k.d && d.dmax == k.dmax, "serial_distance, %s: d %d dmax %d, expected %d %d", k.what, d.d, d.dmax, k.d, k.dmax);
      CHECK(letter_count(g, r.nib[0], k.pos) == k.letters, "letter_count, %s: %d, expected %d", k.what, letter_count(g, r.nib[0], k.pos), k.letters);
      CHECK(plane_count(g, r.nib[0], k.pos) == k.planes, "plane_count, %s: %d, expected %d", k.what, plane_count(g, r.nib[0], k.pos), k.planes);
    }
    // two words: three refused letters in the first, two Y under T in the second -- the running sum peaks at 3 and ends at 1
    const Read r2 = encode("ACGTACGTACGTACGTTTTT");
    const std::vector<u8> g2 = genome("CGTTACGTACGTACGTYYTTACGTACGTACGTACGT");
    const Dist d2 = serial_distance(g2, r2.nib[0], 0, words_of(20));
    CHECK(words_of(20) == 2 && words_of(16) == 1 && words_of(17) == 2, "words_of");
    CHECK(d2.d == 1 && d2.dmax == 3, "serial_distance, dmax above d: d %d dmax %d, expected 1 3", d2.d, d2.dmax);
    CHECK(letter_count(g2, r2.nib[0], 0) == 3, "letter_count beside it: %d", letter_count(g2, r2.nib[0], 0));
    // the A-rich alphabet: A (5) takes A and G, T (8) takes T alone
    CHECK(serial_distance(genome("GCGTACGTACGTACGTACGT"), r.nib[1], 0, 1).d == 0 && serial_distance(genome("ACGCACGTACGTACGTACGT"), r.nib[1], 0, 1).d == 1, "the A-rich alphabet");
  }
  // ---- the position cache ------------------------------------------------------------------------------------------------
  {
    CHECK(cache_slot(1) == 0x9E && cache_slot(2) == 0x3C && cache_slot(1u << 24) == 0xB1 && cache_slot(0) == 0, "cache_slot: %u %u %u", cache_slot(1), cache_slot(2), cache_slot(1u << 24));
    u32 p = 5000, q = 5001;
    while (cache_slot(q) != cache_slot(p)) ++q;
    CacheModel c;
    auto l = c.step({5, 5, 7}, {});
    CHECK(l.size() == 3 && l[0].hit_hi == 0 && l[1].hit_hi == 0 && l[2].hit_hi == 0, "a position twice in one step: both miss");
    l = c.step({7}, {5});
    CHECK(l[0].hit_lo == 1 && l[1].hit_lo == 1 && c.hits == 2, "... and both hit a step later");
    c.step({p}, {});
    l = c.step({q}, {});
    CHECK(l[0].hit_hi == 0 && c.evictions == 1, "another position of the same slot misses and takes it");
    l = c.step({p}, {});
    CHECK(l[0].hit_hi == 0 && c.evictions == 2, "the first one misses in its turn");
    l = c.step({q}, {p});  // within one step: the b half writes after the a half
    CHECK(l[0].hit_hi == 0 && l[1].hit_lo == 1, "q misses, p still hits: lookups come before the step's writes");
    l = c.step({q}, {});
    CHECK(l[0].hit_lo == 1, "q, written by the a half, and p not rewritten: q stays");
    c.clear();
    c.step({p, q}, {});
    l = c.step({p}, {});
    CHECK(l[0].hit_lo == 0 && l[0].hit_hi == 1 && c.unsure == 1, "two positions written to one slot by one half: either may be there");
    l = c.step({p}, {});
    CHECK(l[0].hit_lo == 1, "after which p is there for certain");
    c.clear();
    c.step({p, q}, {});
    l = c.step({p}, {q});  // if p was there, q misses and takes the slot; if q was there, p takes it and q, looked up before, hits
    CHECK(l[0].hit_lo == 0 && l[0].hit_hi == 1 && l[1].hit_lo == 0 && l[1].hit_hi == 1, "either of two: both lookups open");
    l = c.step({p}, {});
    CHECK(l[0].hit_lo == 0 && l[0].hit_hi == 1, "... and still either of the two afterwards");
    c.clear();
    l = c.step({p}, {});
    CHECK(l[0].hit_hi == 0, "cleared");
  }
  // ---- the candidate set ---------------------------------------------------------------------------------------------------
  {
    SetModel m;
    m.reset(100);
    CHECK(m.cutoff == 40 && m.good_cutoff == 10 && m.sz == 1 && m.v[0].d == 40, "reset(100): cutoff %d good %d", m.cutoff, m.good_cutoff);
    m.cutoff = m.good_cutoff;
    m.replay(true, 0, {{true, 5, 5, 100}, {false, 1, 1, 101}, {true, 11, 11, 102}, {true, 4, 12, 103}, {true, 10, 10, 104}});
    CHECK(m.sz == 3 && m.updates == 2 && m.cutoff == 10 && m.v[0].d == 40, "specific chunk: an invalid lane, one beyond the cutoff, one whose running sum peaked beyond it: size %u updates %ld", m.sz, m.updates);
    for (u32 k = 0; k < 47; ++k) m.update(true, 3, 0, 200 + k);
    CHECK(m.sz == 50 && m.v[0].d == 40 && m.fifo == 0, "full: size %u top %d", m.sz, m.v[0].d);
    m.cutoff = m.v[0].d;  // set_sensitive
    m.replay(false, 0, {{true, 30, 30, 300}, {true, 35, 35, 301}, {true, 20, 20, 302}, {true, 25, 25, 303}});
    CHECK(m.cutoff == 20 && m.updates == 51 && m.v[0].d == 20, "a cutoff that tightens in mid-chunk: 30 evicts the sentinel, 35 comes too late, 20 evicts 30, 25 comes too late: cutoff %d updates %ld", m.cutoff, m.updates);
    m.replay(false, 0, {{true, 5, 5, 400}});
    CHECK(m.cutoff == 10 && m.v[0].d == 10, "then 5 evicts 20 and the 10 is on top: cutoff %d", m.cutoff);
    m.replay(false, 0, {{true, 4, 4, 401}, {true, 3, 3, 402}});
    CHECK(m.cutoff == 5 && m.v[0].d == 5 && m.updates == 54, "4 evicts 10, 3 evicts one of the two 5s: cutoff %d", m.cutoff);
    SetModel t;
    t.reset(100);
    t.cutoff = t.good_cutoff;
    for (u32 k = 0; k < 49; ++k) t.update(true, 2, 0, 500 + k);
    t.cutoff = t.v[0].d;
    t.update(false, 2, 0, 600);  // evicts the sentinel: every element a 2
    CHECK(t.cutoff == 2 && t.fifo == 0, "a set of 2s: cutoff %d", t.cutoff);
    t.replay(false, 0, {{true, 2, 2, 601}, {true, 2, 2, 602}, {true, 1, 1, 603}, {true, 2, 2, 604}});
    CHECK(t.fifo == 2 && t.updates == 54, "two ties applied as a run, then a better hit, then a tie while the last element is the 1: fifo %ld updates %ld", t.fifo, t.updates);
    SetModel e;
    e.reset(60);
    e.cutoff = e.good_cutoff;
    e.replay(true, 0x10, {{true, 0, 0, 700}, {true, 0, 0, 700}, {true, 3, 3, 701}, {true, 0, 0, 702}, {true, 2, 2, 703}});
    CHECK(e.sure_ambig && e.sz == 2 && e.updates == 4 && e.best.pos == 700 && (e.best.flags & kAmbigFlag), "the same exact hit twice is one hit, a second one elsewhere ends the read: size %u updates %ld", e.sz, e.updates);
  }
  // ---- ghost letters -----------------------------------------------------------------------------------------------------
  {
    GhostBuffers gb;
    gb.take(encode("CCCCCC"), 3);
    gb.take(encode("AAAA"), 3);
    gb.take(encode("GG"), 3);  // too short to be prepared: writes nothing
    CHECK(gb.bit(0, 0) == 0 && gb.bit(0, 3) == 0 && gb.bit(0, 4) == 1 && gb.bit(0, 5) == 1 && gb.bit(0, 6) == 1, "buffer AAAACC: bits of positions 3 .. 6");
    CHECK(gb.bit(1, 3) == 0 && gb.bit(2, 3) == 1 && gb.bit(2, 1) == 1 && gb.bit(2, 4) == 0, "the A-rich alphabet, and the reverse strand (TTTTGG)");
    u64 w[2];
    ghost_words(gb, 0, 3, 0xFFFFFFFFFFFFFF05ull, w);
    CHECK(w[0] == (0x5ull | (~0ull << 4)) && w[1] == ~0ull, "a read of 3 bases after them: %016llx %016llx", (unsigned long long)w[0], (unsigned long long)w[1]);
    ghost_words(gb, 2, 1, 0, w);  // reverse strand buffer TTTTGG: the T-rich T (10) has bit 1, G bit 0
    CHECK(w[0] == ((~0ull << 6) | 0xEull) && w[1] == ~0ull, "reverse strand, a read of 1 base: %016llx", (unsigned long long)w[0]);
  }
  if (fails) return 1;
  std::printf("OK host %d checks\n", checks);
  return 0;
}
