// GPU test program (built and run by tests/test_gpu_pe_mating_steps.py): the steps the pair kernels take between a
// finished candidate set and a mated pair (PeWave, abm_pe_wave.hpp), each run alone on hand-made lists against plain
// serial host code written from the reference's rules:
//   freeze  heap_order_now / freeze_heap_order   vs  libstdc++'s push_heap / pop_heap array (pe_candidates::update, :824-842)
//   sort    sort_unique                          vs  std::sort + std::unique, diffs by full_compare (:1105-1122)
//   search  sample_list / search_list            vs  std::lower_bound / std::upper_bound; canary words behind samp
//   marks   mark_pairable                        vs  brute force over the other list
//   scan    scan_pairs                           vs  a transcription of best_pair's loops (:1728-1800), pe_element::update (:570-587)
// One wave per case, in the forms the kernels use: tier 1 (PeWave<false, false, false, kMate>, lists in LDS, 128
// entries), tier 2 (PeWave<true, false>, whole-pair, lists of 32768 entries in global memory) and for sort and search
// the long-end form (PeWave<true, false, true>: two window slots, the smallest scratch room).  Built a second time
// with -DABM_PE_RADIX_SORT_MIN=1000000, `sort` runs tier 2's bitonic network at every size.
// Usage: pe_mate_check freeze|sort|search|marks|scan.  Prints "OK ..." with the liveness counts of the cases, or the
// first mismatch.  With -DPE_MATE_HOST_ONLY (plain C++, no GPU) the cases are only built and walked on the host: what the
// liveness counts of `scan` are checked with before anything runs on a GPU.
#ifndef PE_MATE_HOST_ONLY
#include "../../abismal_amd/csrc/abm_pe_wave.hpp"
#define HD __host__ __device__
#else
#include "../../abismal_amd/csrc/abm_lds_layout.hpp"
#define HD
namespace abm {
constexpr u32 kPeCapSmall = 32, kPeCapLarge = 32u << 10, kPeTier1Cap = 128;
constexpr u32 kFlagRC = 0x10, kFlagAmbig = 0x100, kFlagARich = 0x1000;
}
#endif
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace abm;

constexpr u32 kPosLimit = 0xFFFFFFFFu - (1u << 17) + 1u;  // 2^32 - 2^17: the highest position a list holds here
constexpr u64 kGenomeWords = (1ull << 28) + 16;           // 16 bases a word: a read's length beyond ANY 32-bit position (a wrong sort must not read outside)
enum Op : int { kOpFreezeAppended, kOpFreezeHeaped, kOpSort, kOpSearch, kOpMarks, kOpScan };
enum Form : int { kTier1, kTier2, kLongEnd };
static const char *const kFormNames[] = {"tier 1", "tier 2", "long-end"};
constexpr int kMeta = 16;       // result words per case
constexpr u32 kCanaryWords = 16;
constexpr u32 kCanary = 0xC0FFEE00u;

struct Case {
  int op, endA;
  int n[2];      // entries of list 0 / list 1 (freeze: hits appended / hits admitted after set_sensitive)
  u32 off[2];    // where they start in the position / diffs / score arrays (results come back at the same places)
  u32 lflags[2];
  u32 L[2];
  u32 min_frag, max_frag;
  int best[8];   // scan: the standing best: aln_score, max_aln_score, d1, d2, f1, f2, p1, p2
  u32 q_off, q_n;  // search: this case's queries
};
struct Bufs {
  const Case *cases;
  const u32 *pos; const i16 *d; const i16 *sc;
  u32 *o_pos; i16 *o_d; i16 *o_sc;
  int *meta;
  const long long *q_add, *q_key; const int *q_from, *q_strict; int *q_out;
  const u64 *read;  // [2 ends][4 encodings][W]
};

struct Rng {
  u64 s;
  u64 next() { u64 z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  u32 below(u32 n) { return static_cast<u32>(next() % n); }
  u32 in(u32 lo, u32 hi) { return lo + below(hi - lo + 1); }
};

// the genome: word i holds 16 one-hot nibbles drawn from a hash of i
HD inline u64 genome_word(u64 i) {
  u64 z = i * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
  u64 w = 0;
  for (int k = 0; k < 16; ++k) w |= (1ull << ((z >> (2 * k)) & 3u)) << (4 * k);
  return w;
}
static u32 host_enc_of(u32 flags) {  // src/abismal.cpp:1463-1464
  const u32 rc = (flags & kFlagRC) ? 1u : 0u, ar = (flags & kFlagARich) ? 1u : 0u;
  return rc * 2u + (rc ^ ar);
}
// full_compare, src/abismal.cpp:1105-1122, without the cutoff: 16 bases a word, all words of the read
static int host_hamming(const u64 *q, u32 nwords, u32 pos) {
  const u64 i = pos >> 4;
  const u32 offset = (pos & 15u) << 2;
  int d = 0;
  for (u32 w = 0; w < nwords; ++w)
    d += 16 - __builtin_popcountll(q[w] & ((genome_word(i + w) >> offset) | ((genome_word(i + w + 1) << (63 - offset)) << 1)));
  return static_cast<i16>(d);
}

// ---- the cases of one launch and what came back -----------------------------------------------------------------------
struct Plan {
  std::vector<Case> cases;
  std::vector<u32> pos;
  std::vector<i16> d, sc;
  std::vector<long long> q_add, q_key;
  std::vector<int> q_from, q_strict;
  u32 add_list(const std::vector<u32> &p, const std::vector<i16> *dv, const std::vector<i16> *sv) {
    const u32 at = static_cast<u32>(pos.size());
    pos.insert(pos.end(), p.begin(), p.end());
    d.resize(pos.size(), 0); sc.resize(pos.size(), 0);
    if (dv) std::copy(dv->begin(), dv->end(), d.begin() + at);
    if (sv) std::copy(sv->begin(), sv->end(), sc.begin() + at);
    return at;
  }
};
struct Result {
  std::vector<u32> pos;
  std::vector<i16> d, sc;
  std::vector<int> meta, q_out;
};
static u64 g_reads[2][4][8];  // both ends' four packed encodings, random: 16 bases a word
static const u32 kLens[2] = {100, 90};
static void make_reads() {
  Rng r{77};
  for (int e = 0; e < 2; ++e)
    for (int enc = 0; enc < 4; ++enc)
      for (u32 w = 0; w < 8; ++w) {
        u64 x = 0;
        for (u32 k = 0; k < 16; ++k) {
          const u32 base = w * 16 + k;
          const u64 nib = base < kLens[e] ? 1u + r.below(15) : (base < ((kLens[e] + 15u) & ~15u) ? 15u : 0u);
          x |= nib << (4 * k);
        }
        g_reads[e][enc][w] = x;
      }
}

#ifndef PE_MATE_HOST_ONLY
#define CHECK(x)                                                                            \
  do {                                                                                      \
    hipError_t e_ = (x);                                                                    \
    if (e_ != hipSuccess) { printf("FAIL %s: %s\n", #x, hipGetErrorString(e_)); return 2; } \
  } while (0)

__global__ __launch_bounds__(256) void fill_genome(u64 *g, u64 n) {
  for (u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<u64>(gridDim.x) * blockDim.x) g[i] = genome_word(i);
}

template <bool BIG, bool LONG, int PHASE> __global__ __launch_bounds__(64) void step_kernel(PeArgs a0, Bufs b) {
  extern __shared__ __align__(16) unsigned char smem[];
  const Case &c = b.cases[blockIdx.x];
  PeArgs a = a0;
  a.min_frag = static_cast<u32>(uni(static_cast<int>(c.min_frag)));
  a.max_frag = static_cast<u32>(uni(static_cast<int>(c.max_frag)));
  const int lane = lane_id();
  PeWave<BIG, false, LONG, PHASE> w{a};
  pe_carve<BIG, LONG, PHASE, false>(w.lds, w.pl, w.fin, w.samp, smem, a);
  w.P.heap = w.pl.heap;
  w.samp_shift = 0; w.samp_n = 0;
  w.P.spill_pos = nullptr; w.P.spill_d = nullptr; w.P.spill_cap = 0; w.P.spilled = false;
  w.P.cap_avail = a.cap;
  const int op = uni(c.op), endA = uni(c.endA);
  const int n0 = uni(c.n[0]), n1 = uni(c.n[1]);
  const u32 off0 = static_cast<u32>(uni(static_cast<int>(c.off[0]))), off1 = static_cast<u32>(uni(static_cast<int>(c.off[1])));
  w.L[0] = static_cast<u32>(uni(static_cast<int>(c.L[0]))); w.L[1] = static_cast<u32>(uni(static_cast<int>(c.L[1])));
  w.lflags[0] = static_cast<u32>(uni(static_cast<int>(c.lflags[0]))); w.lflags[1] = static_cast<u32>(uni(static_cast<int>(c.lflags[1])));
  w.lsz[0] = w.lsz[1] = 0;
  w.heap_order[0] = w.heap_order[1] = false;
  for (u32 k = lane; k < 8 * a.W; k += 64) w.lds.qpk[k] = b.read[k];
  int *meta = b.meta + static_cast<size_t>(blockIdx.x) * kMeta;
  wave_sync();

  if (op == kOpFreezeAppended || op == kOpFreezeHeaped) {  // the set as seed_end builds and freezes it
    w.P.lpos = w.pl.lpos[0];
    w.P.ld = w.pl.ld[0];
    w.P.begin_read(w.L[0]);
    w.P.cutoff = w.P.good_cutoff;  // set_specific
    for (int i0 = 0; i0 < n0; i0 += 64) {
      const int i = i0 + lane;
      const bool have = i < n0;
      const int h = have ? static_cast<int>(b.d[off0 + i]) : 0;
      const u32 p = have ? b.pos[off0 + i] : 0u;
      (void)w.P.append(__ballot(have), h, p);
    }
    wave_sync();
    if (op == kOpFreezeHeaped) {
      w.P.set_sensitive();
      for (int k = 0; k < n1; ++k) {
        const int dk = uni(static_cast<int>(b.d[off1 + k]));
        const u32 pk = static_cast<u32>(uni(static_cast<int>(b.pos[off1 + k])));
        if (dk <= w.P.cutoff) w.P.admit(false, dk, 0u, pk);
      }
      wave_sync();
    }
    const int n = w.P.sz;
    w.lsz[0] = n;
    w.heap_order[0] = w.P.heaped || n <= 1;
    if (w.P.heaped) w.freeze_heap_order(0, n);
    else w.heap_order_now(0);
    if (lane == 0) { meta[0] = n; meta[1] = w.P.cutoff; meta[2] = w.P.capacity; meta[3] = w.heap_order[0]; }
  }
  else {
    for (int i = lane; i < n0; i += 64) { w.pl.lpos[0][i] = b.pos[off0 + i]; w.pl.ld[0][i] = b.d[off0 + i]; w.pl.lsc[0][i] = b.sc[off0 + i]; }
    for (int i = lane; i < n1; i += 64) { w.pl.lpos[1][i] = b.pos[off1 + i]; w.pl.ld[1][i] = b.d[off1 + i]; w.pl.lsc[1][i] = b.sc[off1 + i]; }
    w.lsz[0] = n0; w.lsz[1] = n1;
    wave_sync();
    if (op == kOpSort) {
      w.sort_unique(0, endA);
      if (lane == 0) meta[0] = w.lsz[0];
    }
    else if (op == kOpSearch) {
      if constexpr (BIG) {
        if (lane < static_cast<int>(kCanaryWords)) w.samp[kSampSlots + lane] = kCanary + lane;
        wave_sync();
        w.sample_list(0);
        const bool intact = lane >= static_cast<int>(kCanaryWords) || w.samp[kSampSlots + lane] == kCanary + lane;
        int wrong = 0;
        for (int j0 = 0; j0 < w.samp_n && j0 < static_cast<int>(kSampSlots + kCanaryWords); j0 += 64) {
          const int j = j0 + lane;
          const bool bad = j < w.samp_n && j < static_cast<int>(kSampSlots + kCanaryWords) &&
                           ((static_cast<long long>(j) << w.samp_shift) >= n0 || w.samp[j] != w.pl.lpos[0][static_cast<u32>(j) << w.samp_shift]);
          wrong += __popcll(__ballot(bad));
        }
        const int n_intact = __popcll(__ballot(intact));
        if (lane == 0) { meta[0] = w.samp_shift; meta[1] = w.samp_n; meta[2] = n_intact; meta[3] = wrong; }
        const u32 q_off = static_cast<u32>(uni(static_cast<int>(c.q_off))), q_n = static_cast<u32>(uni(static_cast<int>(c.q_n)));
        for (u32 q0 = 0; q0 < q_n; q0 += 64) {
          const u32 q = q0 + lane;
          if (q < q_n) {
            const long long add = b.q_add[q_off + q], key = b.q_key[q_off + q];
            const int from = b.q_from[q_off + q];
            b.q_out[q_off + q] = b.q_strict[q_off + q] ? w.template search_list<true>(0, add, key, from) : w.template search_list<false>(0, add, key, from);
          }
        }
      }
    }
    else if (op == kOpMarks) w.mark_pairable(endA);
    else if (op == kOpScan) {
      PairBest best;
      best.aln_score = uni(c.best[0]); best.max_aln_score = uni(c.best[1]);
      best.d1 = uni(c.best[2]); best.d2 = uni(c.best[3]);
      best.f1 = static_cast<u32>(uni(c.best[4])); best.f2 = static_cast<u32>(uni(c.best[5]));
      best.p1 = static_cast<u32>(uni(c.best[6])); best.p2 = static_cast<u32>(uni(c.best[7]));
      PairKept kept;
      w.scan_pairs(endA, best, kept);
      if (lane == 0) {
        meta[0] = best.aln_score; meta[1] = best.d1; meta[2] = best.d2; meta[3] = static_cast<int>(best.f1); meta[4] = static_cast<int>(best.f2);
        meta[5] = static_cast<int>(best.p1); meta[6] = static_cast<int>(best.p2);
        meta[7] = kept.sa; meta[8] = kept.sb; meta[9] = static_cast<int>(kept.pa); meta[10] = static_cast<int>(kept.pb);
      }
    }
  }
  wave_sync();
  const int m0 = w.lsz[0], m1 = w.lsz[1];
  for (int i = lane; i < m0; i += 64) { b.o_pos[off0 + i] = w.pl.lpos[0][i]; b.o_d[off0 + i] = w.pl.ld[0][i]; b.o_sc[off0 + i] = w.pl.lsc[0][i]; }
  if (op != kOpFreezeAppended && op != kOpFreezeHeaped)
    for (int i = lane; i < m1; i += 64) { b.o_pos[off1 + i] = w.pl.lpos[1][i]; b.o_d[off1 + i] = w.pl.ld[1][i]; b.o_sc[off1 + i] = w.pl.lsc[1][i]; }
}

static u64 *g_genome = nullptr;  // device; only `sort` reads it
static int make_genome() {
  CHECK(hipMalloc(&g_genome, kGenomeWords * sizeof(u64)));
  hipLaunchKernelGGL(fill_genome, dim3(1u << 16), dim3(256), 0, 0, g_genome, kGenomeWords);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  return 0;
}

template <class T> static hipError_t to_device(T *&dp, const std::vector<T> &v) {
  const hipError_t e = hipMalloc(&dp, std::max<size_t>(1, v.size()) * sizeof(T));
  if (e != hipSuccess || v.empty()) return e;
  return hipMemcpy(dp, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}
template <class T> static hipError_t zeroed(T *&dp, size_t n) {
  const hipError_t e = hipMalloc(&dp, std::max<size_t>(1, n) * sizeof(T));
  return e != hipSuccess ? e : hipMemset(dp, 0, std::max<size_t>(1, n) * sizeof(T));
}

// every case of `p` on a wave of its own, in form `f`
static int run(Form f, const Plan &p, Result &r) {
  const u32 grid = static_cast<u32>(p.cases.size());
  if (grid == 0) return 0;
  const bool lng = f == kLongEnd, big = f != kTier1;
  const u32 Ls = lng ? kLdsReadLen + 1 : 100;  // the launch's longest read: what its LDS is shaped by
  const double frac = 0.1;
  LdsShape s{(Ls + 15) / 16, (Ls + 63) / 64 + 1, se_window_words(Ls, frac), Ls, Ls + 2, 0};
  if (!lng) s.tb_extra = tb_extra_bytes(s.GW, Ls, frac);
  const u32 cap = big ? kPeCapLarge : kPeTier1Cap;
  const int phase = f == kTier1 ? kMate : kWhole;
  const u32 bytes = pe_lds_layout<u32>(0, phase, lng, big, false, s, cap).bytes;
  if (bytes > 64 * 1024) { printf("FAIL %u bytes of LDS\n", bytes); return 2; }
  PeArgs a{};
  a.ix.genome = g_genome;
  a.W = s.W; a.WB = s.WB; a.GW = s.GW; a.max_len = s.max_len; a.ctmp_cap = s.ctmp_cap; a.tb_extra = s.tb_extra; a.G = 4; a.cap = cap;
  a.valid_frac = frac;
  a.mode = 0;
  if (big) {
    CHECK(zeroed(a.heap_ws, static_cast<size_t>(grid) * cap));
    CHECK(zeroed(a.list_ws, static_cast<size_t>(grid) * 4 * cap));
    CHECK(zeroed(a.payload_ws, static_cast<size_t>(grid) * cap));
  }
  if (lng) {
    CHECK(zeroed(a.long_q, static_cast<size_t>(grid) * (8ull * s.W + 8ull * s.WB)));
    CHECK(zeroed(a.long_ctmp, static_cast<size_t>(grid) * ((s.ctmp_cap + 1) & ~1u)));
    CHECK(zeroed(a.long_tb, 16));
    a.long_tb_bytes = 0;
  }
  std::vector<u64> reads(8 * s.W, 0);
  for (int e = 0; e < 2; ++e)
    for (int enc = 0; enc < 4; ++enc)
      for (u32 k = 0; k < 8 && k < s.W; ++k) reads[(e * 4 + enc) * s.W + k] = g_reads[e][enc][k];
  Bufs b{};
  Case *d_cases; u32 *d_pos; i16 *d_d, *d_sc; long long *d_qa, *d_qk; int *d_qf, *d_qs; u64 *d_read;
  CHECK(to_device(d_cases, p.cases)); CHECK(to_device(d_pos, p.pos)); CHECK(to_device(d_d, p.d)); CHECK(to_device(d_sc, p.sc));
  CHECK(to_device(d_qa, p.q_add)); CHECK(to_device(d_qk, p.q_key)); CHECK(to_device(d_qf, p.q_from)); CHECK(to_device(d_qs, p.q_strict));
  CHECK(to_device(d_read, reads));
  b.cases = d_cases; b.pos = d_pos; b.d = d_d; b.sc = d_sc; b.q_add = d_qa; b.q_key = d_qk; b.q_from = d_qf; b.q_strict = d_qs; b.read = d_read;
  CHECK(zeroed(b.o_pos, p.pos.size())); CHECK(zeroed(b.o_d, p.pos.size())); CHECK(zeroed(b.o_sc, p.pos.size()));
  CHECK(zeroed(b.meta, static_cast<size_t>(grid) * kMeta)); CHECK(zeroed(b.q_out, p.q_add.size()));
  if (f == kTier1) hipLaunchKernelGGL((step_kernel<false, false, kMate>), dim3(grid), dim3(64), bytes, 0, a, b);
  else if (f == kTier2) hipLaunchKernelGGL((step_kernel<true, false, kWhole>), dim3(grid), dim3(64), bytes, 0, a, b);
  else hipLaunchKernelGGL((step_kernel<true, true, kWhole>), dim3(grid), dim3(64), bytes, 0, a, b);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  r.pos.resize(p.pos.size()); r.d.resize(p.pos.size()); r.sc.resize(p.pos.size());
  r.meta.resize(static_cast<size_t>(grid) * kMeta); r.q_out.resize(p.q_add.size());
  if (!r.pos.empty()) {
    CHECK(hipMemcpy(r.pos.data(), b.o_pos, r.pos.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(r.d.data(), b.o_d, r.d.size() * 2, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(r.sc.data(), b.o_sc, r.sc.size() * 2, hipMemcpyDeviceToHost));
  }
  CHECK(hipMemcpy(r.meta.data(), b.meta, r.meta.size() * 4, hipMemcpyDeviceToHost));
  if (!r.q_out.empty()) CHECK(hipMemcpy(r.q_out.data(), b.q_out, r.q_out.size() * 4, hipMemcpyDeviceToHost));
  for (void *ptr : {static_cast<void *>(a.heap_ws), static_cast<void *>(a.list_ws), static_cast<void *>(a.payload_ws), static_cast<void *>(a.long_q),
                    static_cast<void *>(a.long_ctmp), static_cast<void *>(a.long_tb), static_cast<void *>(d_cases), static_cast<void *>(d_pos),
                    static_cast<void *>(d_d), static_cast<void *>(d_sc), static_cast<void *>(d_qa), static_cast<void *>(d_qk), static_cast<void *>(d_qf),
                    static_cast<void *>(d_qs), static_cast<void *>(d_read), static_cast<void *>(b.o_pos), static_cast<void *>(b.o_d),
                    static_cast<void *>(b.o_sc), static_cast<void *>(b.meta), static_cast<void *>(b.q_out)})
    if (ptr) CHECK(hipFree(ptr));
  return 0;
}
#else
static int make_genome() { return 0; }
static int run(Form, const Plan &, Result &) { return -1; }  // (no device: the cases are built and walked on the host only)
#endif

// ---- freeze --------------------------------------------------------------------------------------------------------------
struct El { short d; unsigned pos; };
static bool by_d(const El &x, const El &y) { return x.d < y.d; }

static int cmd_freeze() {
  long long evictions = 0, cases = 0;
  for (const Form f : {kTier1, kTier2}) {
    Plan p;
    std::vector<std::vector<El>> want;
    Rng rng{f == kTier1 ? 11u : 12u};
    for (const int n : {1, 2, 33, 64, 65, 128, 1000, 32768}) {
      if (f == kTier1 && n > static_cast<int>(kPeTier1Cap)) continue;
      for (const Op op : {kOpFreezeAppended, kOpFreezeHeaped}) {
        // n - 1 hits within good_cutoff (10 of 100 bases) arrive in the specific pass: the set grows to n entries
        std::vector<u32> pa(n - 1), pb;
        std::vector<i16> da(n - 1), db;
        for (int i = 0; i < n - 1; ++i) { pa[i] = 1000u + rng.below(1u << 30); da[i] = static_cast<i16>(rng.below(11)); }
        // heaped: a sensitive pass follows, whose hits evict the top of the full set (a set below its capacity of 32 only grows)
        if (op == kOpFreezeHeaped && n >= static_cast<int>(kPeCapSmall))
          for (int i = 0; i < 150; ++i) { pb.push_back(1000u + rng.below(1u << 30)); db.push_back(static_cast<i16>(rng.below(13))); }
        std::vector<El> v(kPeCapLarge);
        v[0] = El{static_cast<short>(0.4 * kLens[0]), 0u};
        int sz = 1, capacity = kPeCapSmall;
        for (int i = 0; i < n - 1; ++i) {  // pe_candidates::update with specific = true and diffs <= good_cutoff: grow, never evict
          if (sz == capacity) ++capacity;
          v[sz++] = El{da[i], pa[i]};
          std::push_heap(v.begin(), v.begin() + sz, by_d);
        }
        if (op == kOpFreezeHeaped) {
          int cutoff = v[0].d;  // set_sensitive
          for (size_t i = 0; i < pb.size(); ++i) {
            if (db[i] > cutoff) continue;
            if (sz == capacity) { std::pop_heap(v.begin(), v.begin() + sz, by_d); --sz; ++evictions; }
            v[sz++] = El{db[i], pb[i]};
            std::push_heap(v.begin(), v.begin() + sz, by_d);
            cutoff = v[0].d;
          }
        }
        v.resize(sz);
        Case c{};
        c.op = op; c.n[0] = n - 1; c.n[1] = static_cast<int>(pb.size());
        c.L[0] = kLens[0]; c.L[1] = kLens[1];
        std::vector<u32> room(std::max(n, 1), 0u);  // (the frozen list comes back here: n entries, the sentinel included)
        std::copy(pa.begin(), pa.end(), room.begin());
        std::vector<i16> roomd(room.size(), 0);
        std::copy(da.begin(), da.end(), roomd.begin());
        c.off[0] = p.add_list(room, &roomd, nullptr);
        c.off[1] = p.add_list(pb, &db, nullptr);
        p.cases.push_back(c);
        want.push_back(v);
        ++cases;
      }
    }
    Result r;
    const int rc = run(f, p, r);
    if (rc > 0) return rc;
    if (rc < 0) continue;
    for (size_t k = 0; k < p.cases.size(); ++k) {
      const Case &c = p.cases[k];
      const std::vector<El> &v = want[k];
      const char *what = c.op == kOpFreezeHeaped ? "freeze_heap_order" : "heap_order_now";
      if (r.meta[k * kMeta] != static_cast<int>(v.size())) {
        printf("FAIL %s %s, %d hits: %d entries, libstdc++ %zu\n", kFormNames[f], what, c.n[0], r.meta[k * kMeta], v.size());
        return 1;
      }
      for (size_t i = 0; i < v.size(); ++i)
        if (r.pos[c.off[0] + i] != v[i].pos || r.d[c.off[0] + i] != v[i].d) {
          printf("FAIL %s %s, set of %zu: entry %zu is pos %u diffs %d, libstdc++'s array has pos %u diffs %d\n", kFormNames[f], what, v.size(), i,
                 r.pos[c.off[0] + i], r.d[c.off[0] + i], v[i].pos, v[i].d);
          return 1;
        }
    }
  }
  printf("OK freeze: %lld sets in heap order entry by entry (%lld evictions in the sensitive passes)\n", cases, evictions);
  return 0;
}

// ---- sort ----------------------------------------------------------------------------------------------------------------
static std::vector<u32> sort_input(int n, int dist, Rng &rng, bool shuffle) {
  std::vector<u32> v(n);
  auto full = [&]() { return 1u + static_cast<u32>(rng.next() % kPosLimit); };
  if (dist == 0 || dist == 4) for (auto &x : v) x = full();  // (i) every digit of all four passes varies
  else if (dist == 1) {  // (ii) one 64 K window: the upper digits constant
    const u32 base = (1u << 24) + static_cast<u32>(rng.next() % (kPosLimit - (1u << 25)));
    for (auto &x : v) x = base + rng.below(1u << 16);
  }
  else if (dist == 2) {  // (iii) runs of 64 inputs sharing one digit of one pass, and two digits alternating
    u32 byte = 0, d0 = 0, d1 = 0;
    bool alt = false;
    for (int i = 0; i < n; ++i) {
      if ((i & 63) == 0) { byte = rng.below(4); d0 = rng.below(byte == 3 ? 255u : 256u); d1 = rng.below(byte == 3 ? 255u : 256u); alt = rng.below(2) != 0; }
      u32 x = (full() & ~(255u << (8 * byte))) | ((alt && (i & 1) ? d1 : d0) << (8 * byte));
      if (x == 0 || x > kPosLimit) x = kPosLimit - rng.below(1000);
      v[i] = x;
    }
  }
  else {  // (iv) a quarter duplicates, in runs of 2 to 200 (adjacent in the input -- across its 64-entry chunks -- or shuffled)
    const int distinct = std::max(1, n - n / 4);
    for (int i = 0; i < distinct && i < n; ++i) v[i] = full();
    for (int i = distinct; i < n;) {
      const u32 x = v[rng.below(distinct)];
      for (int run = static_cast<int>(rng.in(2, 200)); run > 0 && i < n; --run) v[i++] = x;
    }
    if (shuffle) for (int i = n - 1; i > 0; --i) std::swap(v[i], v[rng.below(i + 1)]);
  }
  if (dist == 4 && n > 0) v[0] = 0;  // (v) the set's sentinel
  return v;
}

static int cmd_sort() {
  if (int rc = make_genome()) return rc;
  long long cases = 0, entries = 0, dropped = 0, top_digit_varies = 0;
  for (const Form f : {kTier1, kTier2, kLongEnd}) {
    Plan p;
    std::vector<std::vector<u32>> want;
    Rng rng{100u + f};
    const std::vector<int> sizes = f == kTier1 ? std::vector<int>{0, 1, 2, 63, 64, 65, 127, 128}
                                               : std::vector<int>{1, 65, 511, 512, 513, 577, 4096, 4097, 20001, 32767, 32768};
    for (const int n : sizes)
      for (int dist = 0; dist < 5; ++dist) {
        Case c{};
        c.op = kOpSort;
        c.endA = static_cast<int>((cases >> 1) & 1);
        const u32 combos[4] = {0u, kFlagARich, kFlagRC, kFlagRC | kFlagARich};
        c.lflags[0] = combos[cases & 3];
        c.L[0] = kLens[0]; c.L[1] = kLens[1];
        const std::vector<u32> in = sort_input(n, dist, rng, (cases & 1) != 0);
        c.n[0] = n;
        c.off[0] = p.add_list(in, nullptr, nullptr);
        std::vector<u32> s = in;
        std::sort(s.begin(), s.end());
        s.erase(std::unique(s.begin(), s.end()), s.end());
        int tops = 0;
        for (size_t i = 0; i < s.size(); ++i) tops += i == 0 || (s[i] >> 24) != (s[i - 1] >> 24);
        top_digit_varies += tops > 1;
        entries += n; dropped += n - static_cast<long long>(s.size());
        want.push_back(s);
        p.cases.push_back(c);
        ++cases;
      }
    Result r;
    const int rc = run(f, p, r);
    if (rc > 0) return rc;
    if (rc < 0) continue;
    for (size_t k = 0; k < p.cases.size(); ++k) {
      const Case &c = p.cases[k];
      const std::vector<u32> &s = want[k];
      const int dist = static_cast<int>(k % 5);
      if (r.meta[k * kMeta] != static_cast<int>(s.size())) {
        printf("FAIL %s sort_unique of %d positions (drawn as %d): %d left, std::unique leaves %zu\n", kFormNames[f], c.n[0], dist, r.meta[k * kMeta], s.size());
        return 1;
      }
      const u32 end = static_cast<u32>(c.endA), nwords = (kLens[end] + 15) >> 4;
      const u64 *q = g_reads[end][host_enc_of(c.lflags[0])];
      for (size_t i = 0; i < s.size(); ++i) {
        const int d = s[i] != 0 ? host_hamming(q, nwords, s[i]) : static_cast<int>(static_cast<i16>(0.4 * kLens[end]));
        if (r.pos[c.off[0] + i] != s[i] || r.d[c.off[0] + i] != d) {
          printf("FAIL %s sort_unique of %d positions (drawn as %d): entry %zu is pos %u diffs %d, the host has pos %u diffs %d\n", kFormNames[f], c.n[0], dist,
                 i, r.pos[c.off[0] + i], r.d[c.off[0] + i], s[i], d);
          return 1;
        }
      }
    }
  }
#ifndef PE_MATE_HOST_ONLY
  printf("OK sort (lists beyond %d entries by radix passes): ", kRadixSortMin);
#else
  printf("OK sort: ");
#endif
  printf("%lld lists, %lld positions, %lld duplicates dropped, %lld lists whose top digit varies\n", cases, entries, dropped, top_digit_varies);
  return 0;
}

// ---- sorted lists for search, marks and scan --------------------------------------------------------------------------------
// n sorted distinct positions from `from` on, in stretches of 20 to 400 entries with gaps of one scale each: 1-2 bases
// (windows of hundreds of entries), 10-40, 150-300 (about 180 entries in a 40,000-base window) and thousands (windows of 0 or 1)
static std::vector<u32> stretches(int n, u32 from, Rng &rng, bool dense) {
  std::vector<u32> v;
  u64 at = from;
  int left = 0;
  u32 lo = 1, hi = 2;
  while (static_cast<int>(v.size()) < n) {
    if (left == 0) {
      left = static_cast<int>(rng.in(20, 400));
      switch (dense ? 0u : rng.below(4)) {
        case 0: lo = 1; hi = 2; break;
        case 1: lo = 10; hi = 40; break;
        case 2: lo = 150; hi = 300; break;
        default: lo = 3000; hi = 60000; break;
      }
    }
    if (at > kPosLimit) break;
    v.push_back(static_cast<u32>(at));
    at += rng.in(lo, hi);
    --left;
  }
  return v;
}

static int cmd_search() {
  const u32 min_frag = 32, max_frag = 3000;
  long long cases = 0, queries = 0, with_samples = 0;
  for (const Form f : {kTier2, kLongEnd}) {
    Plan p;
    std::vector<int> want;
    Rng rng{200u + f};
    for (const int n : {0, 1, 2, 64, 511, 512, 513, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 2051, 2052, 4096, 4097, 4103, 4104, 16384, 16385, 32767, 32768}) {
      const std::vector<u32> v = stretches(n, 50000u + rng.below(100000), rng, false);
      if (static_cast<int>(v.size()) != n) { printf("FAIL the list of %d does not fit below 2^32\n", n); return 2; }
      Case c{};
      c.op = kOpSearch; c.n[0] = n;
      c.L[0] = kLens[0]; c.L[1] = kLens[1];
      c.off[0] = p.add_list(v, nullptr, nullptr);
      c.q_off = static_cast<u32>(p.q_add.size());
      int s = 0;  // the sampling step the kernel is to use: the first shift at which every 2^s-th entry fits kSampSlots
      while (((n + (1 << s) - 1) >> s) > static_cast<int>(kSampSlots)) ++s;
      with_samples += s > 0;
      u32 turn = 0;
      std::vector<char> answered(n + 1, 0);
      auto ask = [&](long long value) {  // both kinds of search for `value`, with this turn's add and from
        for (int strict = 0; strict < 2; ++strict, ++turn) {
          const long long add = (turn % 3) == 0 ? 0 : ((turn % 3) == 1 ? min_frag : max_frag);
          auto first = [&](int from) {
            const auto b = v.begin() + from;
            return static_cast<int>((strict ? std::upper_bound(b, v.end(), value, [](long long k, u32 x) { return k < static_cast<long long>(x); })
                                            : std::lower_bound(b, v.end(), value, [](u32 x, long long k) { return static_cast<long long>(x) < k; })) - v.begin());
          };
          const int ans = first(0);
          int from = 0;
          switch ((turn / 3) % 5) {
            case 0: from = 0; break;
            case 1: from = ans; break;
            case 2: from = std::max(ans - 1, 0); break;
            case 3: from = std::min(n, ((ans >> s) << s) + 1); break;
            default: from = n; break;
          }
          const int got = first(from);
          answered[got] = 1;
          p.q_add.push_back(add); p.q_key.push_back(value + add); p.q_from.push_back(from); p.q_strict.push_back(strict);
          want.push_back(got);
        }
      };
      for (int i = 0; i < n; ++i) {
        ask(static_cast<long long>(v[i]) - 1); ask(v[i]); ask(static_cast<long long>(v[i]) + 1);
        turn += 7;  // (every element meets another mix of add and from)
      }
      ask(n ? static_cast<long long>(v[0]) - 1000 : 5);
      ask(n ? static_cast<long long>(v[n - 1]) + 1000 : 1ll << 33);
      ask(-1); ask(1ll << 33);
      for (int i = 0; i <= n; ++i)  // every index is the answer of a search from the start
        if (!answered[i]) {
          p.q_add.push_back(0); p.q_key.push_back(i < n ? static_cast<long long>(v[i]) : (n ? static_cast<long long>(v[n - 1]) + 1 : 0)); p.q_from.push_back(0); p.q_strict.push_back(0);
          want.push_back(i);
        }
      c.q_n = static_cast<u32>(p.q_add.size()) - c.q_off;
      queries += c.q_n;
      p.cases.push_back(c);
      ++cases;
    }
    Result r;
    const int rc = run(f, p, r);
    if (rc > 0) return rc;
    if (rc < 0) continue;
    for (size_t k = 0; k < p.cases.size(); ++k) {
      const Case &c = p.cases[k];
      const int *m = &r.meta[k * kMeta];
      if (m[2] != 64 || m[1] > static_cast<int>(kSampSlots) || m[3] != 0) {
        printf("FAIL %s sample_list of %d entries: shift %d, %d samples (room for %u), %d of the %u words behind them overwritten, %d samples differ from the list\n",
               kFormNames[f], c.n[0], m[0], m[1], kSampSlots, 64 - m[2], kCanaryWords, m[3]);
        return 1;
      }
      for (u32 q = c.q_off; q < c.q_off + c.q_n; ++q)
        if (r.q_out[q] != want[q]) {
          printf("FAIL %s search_list<%s> in %d entries (shift %d): add %lld key %lld from %d gives %d, std::%s_bound %d\n", kFormNames[f], p.q_strict[q] ? "true" : "false",
                 c.n[0], m[0], p.q_add[q], p.q_key[q], p.q_from[q], r.q_out[q], p.q_strict[q] ? "upper" : "lower", want[q]);
          return 1;
        }
    }
  }
  printf("OK search: %lld lists (%lld of them sampled at a step above 1), %lld searches, the words behind the samples untouched\n", cases, with_samples, queries);
  return 0;
}

// ---- pairs of lists for marks and scan ---------------------------------------------------------------------------------------
struct Lists { std::vector<u32> a, b; };
// list 0 in stretches; half of list 1 derived from entries of list 0 (fragments at, one inside and one outside both limits,
// and anywhere between), half in stretches of its own; `sentinel`: list 1 starts with the set's pos == 0 entry
static Lists pair_lists(int na, int nb, u32 lenA, u32 lenB, u32 min_frag, u32 max_frag, bool dense, bool sentinel, Rng &rng) {
  Lists o;
  const u32 floor_pos = max_frag + lenA + lenB + 1;  // (nearer the origin the reference's rewind is undefined)
  o.a = stretches(na, floor_pos + rng.below(5000), rng, dense);
  std::vector<u32> b;
  if (sentinel && nb > 0) b.push_back(0);
  const u32 span_lo = o.a.empty() ? floor_pos : o.a.front(), span_hi = o.a.empty() ? floor_pos + 100000 : o.a.back();
  int guard = 0;
  while (static_cast<int>(b.size()) < nb && ++guard < 64) {
    const int need = nb - static_cast<int>(b.size());
    std::vector<u32> more;
    if (!o.a.empty())
      for (int i = 0; i < need / 2; ++i) {
        const u32 a = o.a[rng.below(static_cast<u32>(o.a.size()))];
        u32 frag;
        switch (rng.below(8)) {
          case 0: frag = min_frag - 1; break;
          case 1: frag = min_frag; break;
          case 2: frag = min_frag + 1; break;
          case 3: frag = max_frag - 1; break;
          case 4: frag = max_frag; break;
          case 5: frag = max_frag + 1; break;
          default: frag = rng.in(min_frag, max_frag); break;
        }
        const long long x = static_cast<long long>(a) + frag - lenB;
        if (x >= floor_pos && x <= kPosLimit) more.push_back(static_cast<u32>(x));
      }
    const std::vector<u32> own = stretches(need - static_cast<int>(more.size()), span_lo + rng.below(span_hi - span_lo + max_frag + 4 * static_cast<u32>(nb) + 1), rng, dense && nb < 1000);
    more.insert(more.end(), own.begin(), own.end());
    b.insert(b.end(), more.begin(), more.end());
    std::sort(b.begin(), b.end());
    b.erase(std::unique(b.begin(), b.end()), b.end());
  }
  o.b = b;
  return o;
}
struct Shape { int na, nb; };
static std::vector<Shape> shapes_of(Form f) {
  if (f == kTier1) return {{0, 5}, {1, 1}, {5, 70}, {64, 64}, {65, 128}, {128, 128}};
  return {{600, 700}, {5000, 3000}, {32768, 2000}, {2000, 32768}};
}
static const u32 kLimits[3][2] = {{150, 300}, {32, 3000}, {32, 40000}};

static int cmd_marks() {
  long long cases = 0, marked[3] = {0, 0, 0};
  for (const Form f : {kTier1, kTier2}) {
    Plan p;
    std::vector<std::vector<i16>> want;  // per case: list 0's marks, then list 1's
    Rng rng{300u + f};
    for (const Shape sh : shapes_of(f))
      for (int lim = 0; lim < 3; ++lim)
        for (int endA = 0; endA < 2; ++endA) {
          const u32 lenA = kLens[endA], lenB = kLens[1 - endA], mn = kLimits[lim][0], mx = kLimits[lim][1];
          const Lists l = pair_lists(sh.na, sh.nb, lenA, lenB, mn, mx, (cases % 3) == 2, (cases & 1) != 0, rng);
          if (static_cast<int>(l.a.size()) != sh.na || static_cast<int>(l.b.size()) != sh.nb) { printf("FAIL lists of %d and %d could not be made (%zu, %zu)\n", sh.na, sh.nb, l.a.size(), l.b.size()); return 2; }
          std::vector<i16> da(sh.na), db(sh.nb);
          for (auto &x : da) x = static_cast<i16>(rng.below(8) ? 1 + rng.below(10) : 0);
          for (auto &x : db) x = static_cast<i16>(rng.below(8) ? 1 + rng.below(10) : 0);
          Case c{};
          c.op = kOpMarks; c.endA = endA; c.n[0] = sh.na; c.n[1] = sh.nb;
          c.L[0] = kLens[0]; c.L[1] = kLens[1];
          c.min_frag = mn; c.max_frag = mx;
          c.off[0] = p.add_list(l.a, &da, nullptr);
          c.off[1] = p.add_list(l.b, &db, nullptr);
          std::vector<i16> w(sh.na + sh.nb, 0);
          for (int i = 0; i < sh.na; ++i) {
            bool any = false;
            for (int j = 0; j < sh.nb && !any; ++j) {
              const long long e = static_cast<long long>(l.b[j]) + lenB;
              any = static_cast<long long>(l.a[i]) + mn <= e && e <= static_cast<long long>(l.a[i]) + mx;
            }
            w[i] = !any ? 0 : (da[i] == 0 ? static_cast<i16>(2 * lenA) : -1);
          }
          for (int j = 0; j < sh.nb; ++j) {
            bool any = false;
            const long long e = static_cast<long long>(l.b[j]) + lenB;
            for (int i = 0; i < sh.na && !any; ++i) any = static_cast<long long>(l.a[i]) + mn <= e && e <= static_cast<long long>(l.a[i]) + mx;
            w[sh.na + j] = !any ? 0 : (db[j] == 0 ? static_cast<i16>(2 * lenB) : -1);
          }
          for (const i16 x : w) ++marked[x == 0 ? 0 : (x < 0 ? 1 : 2)];
          want.push_back(w);
          p.cases.push_back(c);
          ++cases;
        }
    Result r;
    const int rc = run(f, p, r);
    if (rc > 0) return rc;
    if (rc < 0) continue;
    for (size_t k = 0; k < p.cases.size(); ++k) {
      const Case &c = p.cases[k];
      for (int which = 0; which < 2; ++which)
        for (int i = 0; i < c.n[which]; ++i) {
          const i16 got = r.sc[c.off[which] + i], exp = want[k][(which ? c.n[0] : 0) + i];
          if (got != exp) {
            printf("FAIL %s mark_pairable, lists of %d and %d, limits %u..%u, endA %d: list %d entry %d (pos %u, diffs %d) is marked %d, brute force says %d\n",
                   kFormNames[f], c.n[0], c.n[1], c.min_frag, c.max_frag, c.endA, which, i, p.pos[c.off[which] + i], p.d[c.off[which] + i], got, exp);
            return 1;
          }
        }
    }
  }
  printf("OK marks: %lld pairs of lists; %lld entries without a partner, %lld to align, %lld exact\n", cases, marked[0], marked[1], marked[2]);
  return 0;
}

// ---- scan ----------------------------------------------------------------------------------------------------------------
struct HostEl {  // se_element
  i16 diffs; u16 flags; u32 pos;
};
struct HostBest {  // pe_element, :547-619
  i16 aln_score, max_aln_score;
  HostEl r1, r2;
  bool ambig() const { return (r1.flags & kFlagAmbig) != 0; }
  bool sure_ambig() const { return ambig() && aln_score == max_aln_score; }
  int tie_flags = 0;
  bool update(i16 scr, const HostEl &s1, const HostEl &s2) {  // :570-587
    const auto rd = r1.diffs + r2.diffs;
    const auto sd = s1.diffs + s2.diffs;
    if (scr > aln_score || (scr == aln_score && sd < rd)) {
      r1 = s1; r2 = s2; aln_score = scr;
      return true;
    }
    else if (scr == aln_score && sd == rd) {
      if (!ambig()) ++tie_flags;
      r1.flags |= kFlagAmbig;
      return false;
    }
    return false;
  }
};
struct Live { long long better, stale, stale_first, tie_flag, stop_at_max, realigned, carry_chunks, over64, over128, windows[4]; };
struct Kept { i16 scr1, scr2; u32 pos1, pos2; };

// best_pair's loops, :1728-1800; aln.align is a look-up of the entry's given score
static Kept host_scan(bool swap_ends, const std::vector<HostEl> &res1, const std::vector<HostEl> &res2, const std::vector<i16> &score1,
                      const std::vector<i16> &score2, u32 readlen2, u32 min_dist, u32 max_dist, HostBest &best, Live &live) {
  Kept k{0, 0, 0, 0};
  if (res1.empty()) return k;  // (the reference's sets hold their sentinel at least; its rewind would step before an empty list)
  size_t j1 = 0, j2 = 0;
  const size_t j1_end = res1.size(), j2_end = res2.size(), j1_beg = 0;
  std::vector<i16> mem_scr1(res1.size(), 0);
  std::vector<char> visited(res1.size(), 0);
  i16 scr1 = 0;
  HostEl s1, s2;
  for (; j1 != j1_end && res1[j1].pos == 0; ++j1)
    ;
  for (; j2 != j2_end && res2[j2].pos == 0; ++j2)
    ;
  const size_t j2_first = j2;
  bool last_stale = false, last_stale_first = false;  // of the pair this call records last: the one whose scores it hands on
  for (; j2 != j2_end && !best.sure_ambig(); ++j2) {
    s2 = res2[j2];
    i16 scr2 = 0;
    const u32 lim = s2.pos + readlen2;
    for (; (j1 == j1_end) || (j1 != j1_beg && res1[j1].pos + max_dist >= lim); --j1)
      ;
    for (; j1 != j1_end && res1[j1].pos + max_dist < lim; ++j1)
      ;
    long long steps = 0;
    for (; j1 != j1_end && res1[j1].pos + min_dist <= lim && !best.sure_ambig(); ++j1) {
      s1 = res1[j1];
      ++steps;
      if (scr2 == 0) scr2 = score2[j2];
      if (mem_scr1[j1] == 0) {
        if (visited[j1]) ++live.realigned;
        visited[j1] = 1;
        scr1 = score1[j1];
        mem_scr1[j1] = scr1;
      }
      const i16 pair_scr = static_cast<i16>(scr2 + mem_scr1[j1]);
      const bool was_sure = best.sure_ambig();
      if (swap_ends ? best.update(pair_scr, s2, s1) : best.update(pair_scr, s1, s2)) {
        k.scr1 = scr1; k.scr2 = scr2; k.pos1 = res1[j1].pos; k.pos2 = res2[j2].pos;
        ++live.better;
        // (recorded with the score of ANOTHER entry's alignment: this one was aligned before and is not aligned again; and
        // the same at the first of 64 list-1 entries the kernel takes together, which carries "visited so far" across)
        last_stale = scr1 != mem_scr1[j1];
        last_stale_first = last_stale && j2 >= j2_first + 64 && (j2 - j2_first) % 64 == 0;
      }
      if (!was_sure && best.sure_ambig()) ++live.stop_at_max;
    }
    live.over64 += steps > 64; live.over128 += steps > 128;
    ++live.windows[steps == 0 ? 0 : (steps == 1 ? 1 : (steps <= 5 ? 2 : 3))];
  }
  live.stale += last_stale; live.stale_first += last_stale_first;
  live.tie_flag += best.tie_flags;
  best.tie_flags = 0;
  return k;
}
// 64 entries of list 1 lay their windows' steps out one after the other, 64 steps a chunk: chunks in which no window begins
static long long carry_chunks(const std::vector<u32> &a, const std::vector<u32> &b, u32 lenB, u32 mn, u32 mx) {
  long long n = 0;
  size_t ib0 = (!b.empty() && b[0] == 0) ? 1 : 0;
  for (; ib0 < b.size(); ib0 += 64) {
    std::vector<long long> starts;
    long long total = 0;
    for (size_t ib = ib0; ib < std::min(b.size(), ib0 + 64); ++ib) {
      const long long lim = static_cast<long long>(b[ib]) + lenB;
      const auto lo = std::lower_bound(a.begin(), a.end(), lim - mx, [](u32 x, long long k) { return static_cast<long long>(x) < k; });
      const auto hi = std::upper_bound(a.begin(), a.end(), lim - mn, [](long long k, u32 x) { return k < static_cast<long long>(x); });
      if (hi > lo) { starts.push_back(total); total += hi - lo; }
    }
    for (long long c0 = 0; c0 < total; c0 += 64) {
      bool any = false;
      for (const long long s : starts) any |= s >= c0 && s < c0 + 64;
      n += !any;
    }
  }
  return n;
}

static int cmd_scan() {
  long long cases[2] = {0, 0};
  Live live[2];
  std::memset(live, 0, sizeof(live));
  for (const Form f : {kTier1, kTier2}) {
    Plan p;
    struct Want { HostBest best; Kept kept; };
    std::vector<Want> want;
    Rng rng{400u + f};
    Live &lv = live[f == kTier1 ? 0 : 1];
    struct Combo { Shape sh; int lim, dense, table, swapped; };
    std::vector<Combo> combos;
    if (f == kTier1) {
      for (const Shape sh : shapes_of(f))
        for (int lim = 0; lim < 3; ++lim)
          for (int dense = 0; dense < 2; ++dense)
            for (int table = 0; table < 5; ++table)
              for (int swapped = 0; swapped < 2; ++swapped) combos.push_back(Combo{sh, lim, dense, table, swapped});
    }
    else {  // every shape at every pair of limits, twice; the score table and the order of the ends take turns; dense lists at the smallest shape
      int turn = 0;
      for (int pass = 0; pass < 2; ++pass)
        for (const Shape sh : shapes_of(f))
          for (int lim = 0; lim < 3; ++lim, ++turn) combos.push_back(Combo{sh, lim, sh.na == 600 && pass == 1, (turn + 2 * pass) % 5, ((turn >> 1) + pass) & 1});
    }
    int variety = 0;
    for (const Combo &cb : combos) {
            {
              const Shape sh = cb.sh;
              const int lim = cb.lim, dense = cb.dense, table = cb.table, swapped = cb.swapped;
              ++variety;
              const int endA = swapped;
              const u32 lenA = kLens[endA], lenB = kLens[1 - endA], mn = kLimits[lim][0], mx = kLimits[lim][1];
              const Lists l = pair_lists(sh.na, sh.nb, lenA, lenB, mn, mx, dense != 0, rng.below(3) == 0, rng);
              if (static_cast<int>(l.a.size()) != sh.na || static_cast<int>(l.b.size()) != sh.nb) { printf("FAIL lists of %d and %d could not be made (%zu, %zu)\n", sh.na, sh.nb, l.a.size(), l.b.size()); return 2; }
              // table 0: scores of 150..400; 1: one score throughout (every pair ties), diffs differ; 2: ... and so do the diffs'
              // sums; 3: scores below the best possible one, which exact hits early in both lists have; 4: list 1's scores rise
              // along the list (better pairs keep coming, also at list-0 entries aligned long before); every table: a few scores of 0
              std::vector<i16> da(sh.na), db(sh.nb), sa(sh.na), sb(sh.nb);
              for (int which = 0; which < 2; ++which) {
                std::vector<i16> &dv = which ? db : da, &sv = which ? sb : sa;
                const int n = which ? sh.nb : sh.na;
                const i16 top = static_cast<i16>(2 * (which ? lenB : lenA));
                for (int i = 0; i < n; ++i) {
                  dv[i] = static_cast<i16>(table == 2 ? 3 : rng.below(13));
                  sv[i] = static_cast<i16>((table == 1 || table == 2) ? 300 : (table == 3 ? rng.in(100, top - 1) : rng.in(150, 400)));
                  if (table == 4 && which == 1) sv[i] = static_cast<i16>(150 + (200ll * i) / n);
                  if (table == 3 && i < n / 4 + 2 && rng.below(which ? 12 : 3) == 0) { sv[i] = top; dv[i] = 0; }
                  if (rng.below(32) == 0) sv[i] = 0;
                }
              }
              // (table 4: the kernel takes 64 list-1 entries at a time; the first of each such group scores above the rest, the last
              // group's highest, so that the pair recorded last is found there, where "visited so far" comes from the group before)
              if (table == 4)
                for (int i = (sh.nb > 0 && l.b[0] == 0 ? 1 : 0) + 64; i < sh.nb; i += 64) sb[i] = static_cast<i16>(400 - (sh.nb - 1 - i) / 64);
              const u32 flag_sets[4] = {0u, kFlagARich, kFlagRC, kFlagRC | kFlagARich};
              const u32 fa = flag_sets[variety & 3], fb = flag_sets[(variety + 2) & 3];
              std::vector<HostEl> res1(sh.na), res2(sh.nb);
              for (int i = 0; i < sh.na; ++i) res1[i] = HostEl{da[i], static_cast<u16>(fa), l.a[i]};
              for (int i = 0; i < sh.nb; ++i) res2[i] = HostEl{db[i], static_cast<u16>(fb), l.b[i]};
              const u32 off_a = p.add_list(l.a, &da, &sa), off_b = p.add_list(l.b, &db, &sb);
              lv.carry_chunks += carry_chunks(l.a, l.b, lenB, mn, mx);
              // the standing best: cleared; a middling score; this call's own result, which its first equal step then ties with
              HostBest cleared{};
              cleared.aln_score = 0;
              cleared.max_aln_score = static_cast<i16>(static_cast<i16>(2 * kLens[0]) + static_cast<i16>(2 * kLens[1]));
              cleared.r1 = HostEl{static_cast<i16>(0.4 * kLens[0]), 0, 0};
              cleared.r2 = HostEl{static_cast<i16>(0.4 * kLens[1]), 0, 0};
              HostBest own = cleared;
              for (int standing = 0; standing < 3; ++standing) {
                HostBest start = cleared;
                if (standing == 1) { start.aln_score = 550; start.r1 = HostEl{4, static_cast<u16>(kFlagRC), 123456}; start.r2 = HostEl{4, static_cast<u16>(kFlagARich), 123556}; }
                if (standing == 2) { start = own; start.r1.flags &= ~kFlagAmbig; if (start.r1.pos) { start.r1.pos = 777777; start.r2.pos = 888888; } }
                Case c{};
                c.op = kOpScan; c.endA = endA; c.n[0] = sh.na; c.n[1] = sh.nb;
                c.off[0] = off_a; c.off[1] = off_b;
                c.lflags[0] = fa; c.lflags[1] = fb;
                c.L[0] = kLens[0]; c.L[1] = kLens[1];
                c.min_frag = mn; c.max_frag = mx;
                const int b8[8] = {start.aln_score, start.max_aln_score, start.r1.diffs, start.r2.diffs, start.r1.flags, start.r2.flags,
                                   static_cast<int>(start.r1.pos), static_cast<int>(start.r2.pos)};
                std::copy(b8, b8 + 8, c.best);
                Want w;
                w.best = start;
                w.kept = host_scan(swapped != 0, res1, res2, sa, sb, lenB, mn, mx, w.best, lv);
                if (standing == 0) own = w.best;
                want.push_back(w);
                p.cases.push_back(c);
                ++cases[f == kTier1 ? 0 : 1];
              }
            }
    }
    Result r;
    const int rc = run(f, p, r);
    if (rc > 0) return rc;
    if (rc < 0) continue;
    for (size_t k = 0; k < p.cases.size(); ++k) {
      const Case &c = p.cases[k];
      const int *m = &r.meta[k * kMeta];
      const Want &w = want[k];
      const int exp[11] = {w.best.aln_score, w.best.r1.diffs, w.best.r2.diffs, w.best.r1.flags, w.best.r2.flags, static_cast<int>(w.best.r1.pos),
                           static_cast<int>(w.best.r2.pos), w.kept.scr1, w.kept.scr2, static_cast<int>(w.kept.pos1), static_cast<int>(w.kept.pos2)};
      if (!std::equal(exp, exp + 11, m)) {
        printf("FAIL %s scan_pairs, case %zu: lists of %d and %d, limits %u..%u, swapped %d, standing score %d\n", kFormNames[f], k, c.n[0], c.n[1], c.min_frag, c.max_frag,
               c.endA, c.best[0]);
        printf("  gpu:  score %d d1 %d d2 %d f1 %#x f2 %#x p1 %u p2 %u; kept scores %d %d positions %u %u\n", m[0], m[1], m[2], m[3], m[4], static_cast<u32>(m[5]),
               static_cast<u32>(m[6]), m[7], m[8], static_cast<u32>(m[9]), static_cast<u32>(m[10]));
        printf("  host: score %d d1 %d d2 %d f1 %#x f2 %#x p1 %u p2 %u; kept scores %d %d positions %u %u\n", exp[0], exp[1], exp[2], exp[3], exp[4], static_cast<u32>(exp[5]),
               static_cast<u32>(exp[6]), exp[7], exp[8], static_cast<u32>(exp[9]), static_cast<u32>(exp[10]));
        return 1;
      }
    }
  }
  // liveness: what the host walk met, per tier (tier 1's 128 entries cannot hold a window of more than 128 steps)
  for (int t = 0; t < 2; ++t) {
    const Live &v = live[t];
    const bool ok = v.better && v.stale && v.stale_first && v.tie_flag && v.stop_at_max && v.realigned && v.carry_chunks && v.over64 && (t == 0 || v.over128) && v.windows[0] && v.windows[1] &&
                    v.windows[2] && v.windows[3];
    if (!ok) {
      printf("FAIL scan: tier %d's cases do not exercise everything: better %lld (calls whose last one keeps another entry's score: %lld, %lld at the first of 64), ties flagged %lld, stops at the maximum %lld, re-aligned %lld, chunks without a window "
             "start %lld, windows over 64 / 128 steps %lld / %lld, windows of 0 / 1 / 2-5 / more steps %lld / %lld / %lld / %lld\n",
             t + 1, v.better, v.stale, v.stale_first, v.tie_flag, v.stop_at_max, v.realigned, v.carry_chunks, v.over64, v.over128, v.windows[0], v.windows[1], v.windows[2], v.windows[3]);
      return 1;
    }
  }
  printf("OK scan:");
  for (int t = 0; t < 2; ++t) {
    const Live &v = live[t];
    printf(" tier %d: %lld calls, %lld better pairs (calls whose last one keeps another entry's score: %lld, %lld of them at the first of 64 list-1 entries), %lld ties flagged, %lld stops at the maximum, %lld zero-score entries re-aligned, %lld chunks without a window start, "
           "%lld / %lld windows over 64 / 128 steps, %lld / %lld / %lld / %lld windows of 0 / 1 / 2-5 / more steps;",
           t + 1, cases[t], v.better, v.stale, v.stale_first, v.tie_flag, v.stop_at_max, v.realigned, v.carry_chunks, v.over64, v.over128, v.windows[0], v.windows[1], v.windows[2], v.windows[3]);
  }
  printf("\n");
  return 0;
}

int main(int argc, char **argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  make_reads();
  if (cmd == "freeze") return cmd_freeze();
  if (cmd == "sort") return cmd_sort();
  if (cmd == "search") return cmd_search();
  if (cmd == "marks") return cmd_marks();
  if (cmd == "scan") return cmd_scan();
  printf("usage: pe_mate_check freeze|sort|search|marks|scan\n");
  return 2;
}
