// GPU test program (built and run by tests/test_gpu_align_stages.py): the alignment stages of abm_align.hpp, each run
// alone on hand-made input -- one 64-lane block per case -- against the serial banded DP of tests/hip/align_host.hpp.
// Every comparison is exact.
//   table   wavefront<true, false>, wavefront<true, true>, wavefront_rows<true>: every byte of the traceback table, each
//           lane's best value and first row, first_maximum
//   wrap    reads beyond 16383 bases: wavefront<true, true> (table in global memory) and score_round<true> against the
//           16-bit host DP, which must differ from the 32-bit one
//   rounds  score_round<false>, score_round<true>, score_round_quad<false> driven over `first` until the list is consumed
//   floor   score_round_quad<true> on the same lists against floors taken from the host scores
//   cigar   cigar_walk + cigar_publish and wave_cigar on every kind of sink; edit_distance and long_enough over a grid
//   choose  choose_se<false, false> and choose_se<true, false> against host_choose
// Reads and targets: random nibbles with planted copies (substitutions, indels at head, middle or tail, all-match and
// all-mismatch pairs, multi-bit and zero target nibbles, the 0xF padding of a read's last word).  GW and W are what the
// launcher computes for the case's length and widest band; the genome buffer is padded past its last window.
// The anti-diagonal wavefront<true> never writes some cells outside the read (the first rows of the left columns' upper
// triangle and the last rows of the right columns: no step of its schedule falls on them, and no walk reads them);
// wavefront_rows<true> writes 3 there, as the host table has it.  `table` prefills with 0xEE, accepts 0xEE from the
// anti-diagonal runs only where the host has 3, and counts those cells.
// Usage: align_check table|wrap|rounds|floor|cigar|choose.  Prints "OK <step> ..." with the liveness counts, or the first
// mismatch.  With -DALIGN_HOST_ONLY (plain C++, no GPU) the cases are only built and the counts printed ("HOST <step> ...").
#ifndef ALIGN_HOST_ONLY
#include "../../abismal_amd/csrc/abm_align.hpp"
#endif
#include "align_host.hpp"
#include <cstring>
#include <string>
using namespace abm;
using namespace align_host;

#ifdef ALIGN_HOST_ONLY
constexpr bool kDevice = false;
#else
constexpr bool kDevice = true;
#endif
constexpr int kLens[11] = {32, 33, 47, 48, 49, 63, 64, 65, 100, 150, 151};
constexpr int kMd = 30;             // max_diffs of every case but choose's: band_for(d, kMd) = 2 d + 1 up to 61
constexpr u8 kFill = 0xEE;          // a table byte nothing wrote
constexpr u32 kCanary = 0xC0FFEE00u;
static u32 words_for(int L) { return static_cast<u32>(L + 15) / 16; }
// the valid fraction at which a launch's widest band is bw: md = (bw - 1) / 2
static double frac_for(int L, int bw) { return ((bw - 1) / 2 + 0.5) / L; }

// ---- cases -------------------------------------------------------------------------------------------------------------
static std::vector<unsigned char> random_read(int L) {
  std::vector<unsigned char> q(L);
  for (auto &b : q) b = static_cast<unsigned char>(1u << (rnd() & 3));
  return q;
}
static void pack(const std::vector<unsigned char> &q, u64 *dst, u32 W) {  // 0xF in the last word's padding
  for (u32 w = 0; w < W; ++w) dst[w] = ~0ull;
  for (size_t k = 0; k < q.size(); ++k) dst[k / 16] = (dst[k / 16] & ~(15ull << (4 * (k % 16)))) | (static_cast<u64>(q[k]) << (4 * (k % 16)));
}
// a fresh stretch of the genome (random one-hot nibbles) and in it a position whose band of bw starts at nibble t0nib of its word
static u32 g_next = 4096;
static u32 place(int bw, int t0nib, u32 span = 768) {
  const u32 base = (g_next + 15u) & ~15u;
  g_next = base + span;
  const size_t old = G.size();
  if (G.size() < g_next + 4096) { G.resize(g_next + 4096); for (size_t k = old; k < G.size(); ++k) G[k] = static_cast<unsigned char>(1u << (rnd() & 3)); }
  return base + 96u + static_cast<u32>(t0nib) + static_cast<u32>((bw - 1) / 2);
}
struct Plan {
  int subs = 0;
  std::vector<std::pair<int, int>> gaps;  // (read index, gap): gap < 0 the copy lacks bases (the read has an insertion), > 0 it has extra ones
  int iupac = 0, zeros = 0;
  bool all_mismatch = false;
};
static unsigned char other(unsigned char b) { return static_cast<unsigned char>(1u << ((__builtin_ctz(b) + 1 + static_cast<int>(rnd() % 3)) & 3)); }
static void plant_plan(const std::vector<unsigned char> &q, u32 pos, const Plan &p) {
  std::vector<unsigned char> copy(q);
  const int L = static_cast<int>(q.size());
  if (p.all_mismatch) for (auto &b : copy) b = other(b);
  for (int k = 0; k < p.subs; ++k) { const int at = rnd_in(0, L - 1); copy[at] = other(q[at]); }
  std::vector<std::pair<int, int>> gaps(p.gaps);
  std::sort(gaps.begin(), gaps.end());
  for (size_t g = gaps.size(); g-- > 0;) {
    const int at = gaps[g].first, gap = gaps[g].second;
    if (gap < 0) copy.erase(copy.begin() + at, copy.begin() + std::min<int>(at - gap, static_cast<int>(copy.size())));
    else for (int k = 0; k < gap; ++k) copy.insert(copy.begin() + at, static_cast<unsigned char>(1u << (rnd() & 3)));
  }
  for (int k = 0; k < p.iupac; ++k) { auto &b = copy[rnd() % copy.size()]; b = static_cast<unsigned char>(b | other(b) | (rnd() & 1 ? other(b) : 0)); }
  for (int k = 0; k < p.zeros; ++k) copy[rnd() % copy.size()] = 0;
  for (size_t k = 0; k < copy.size(); ++k) G[pos + k] = copy[k];
}
// the plans the stages are run on: 0 substitutions, 1 an indel at head / middle / tail, 2 all-match, 3 all-mismatch, 4 multi-bit
// and zero target nibbles, 5 an insertion and a deletion, 6 one extra target base two from the read's end (the maximum twice)
static Plan plan_of(int kind, int L, int n) {
  Plan p;
  if (kind == 0) p.subs = rnd_in(0, 6);
  else if (kind == 1) {
    int g = rnd_in(1, 30);
    const bool lacks = rnd() & 1;
    const int where = n % 3;
    int at = where == 0 ? 2 : (where == 1 ? L / 2 : L - 2);
    if (lacks) { if (where == 2) at = std::max(2, L - 2 - g); g = std::min(g, L - at - 2); }
    p.gaps.push_back({at, lacks ? -g : g});
    p.subs = rnd_in(0, 2);
  }
  else if (kind == 3) p.all_mismatch = true;
  else if (kind == 4) { p.iupac = rnd_in(1, 8); p.zeros = rnd_in(1, 3); p.subs = rnd_in(0, 3); }
  else if (kind == 5) { const int a = rnd_in(1, 3), b = rnd_in(1, 3), sg = rnd() & 1 ? 1 : -1; p.gaps.push_back({L / 3, sg * a}); p.gaps.push_back({2 * L / 3, -sg * b}); }
  else if (kind == 6) p.gaps.push_back({L - 2, 1});
  return p;
}

struct Carve { u32 qwords, ctmp_words, slots, GW, tb_bytes; };  // a launch's LDS: the largest of its cases
static size_t carve_bytes(const Carve &c) {
  const size_t win = static_cast<size_t>(c.slots) * c.GW * 8, tbl = c.tb_bytes ? static_cast<size_t>(c.GW) * 8 + c.tb_bytes + 16 : 0;
  return static_cast<size_t>(c.qwords) * 8 + ((c.ctmp_words + 1u) & ~1u) * 4 + 2 * kSeCap * 4 + 64 * 4 + (kSeCap + 2) * 4 + std::max(win, tbl) + 16;
}
struct TabCase { u32 L, bw, pos, W, GW, read_off, out_off; };
struct ListCase { u32 L, n, W, GW, max_jobs, qbase, n_enc, read_off, job_off; int floor; };
struct ListOut { int score[kSeCap]; int visits[kSeCap]; int round_end[kSeCap + 2]; u32 round_it[kSeCap + 2][2]; int n_rounds, bad; u32 iters[2]; };
constexpr u32 kSlotWords = 192, kArenaWords = 256;
struct CigCase {
  u32 L, bw, pos, W, GW, read_off;
  u32 stride, ctmp_cap, arena_cap, arena_count;
  int has_arena, want_fin;
  int mode;           // 0: cigar_walk + cigar_publish, 1: wave_cigar
  int diffs, score0;  // wave_cigar: the diffs it is told, and whether it is told score 0
};
struct CigOut { u32 n_ops, aln_len, t_pos, arena_count, ctmp_guard, walk_n; int ins, del, clip_head, clip_tail, overflow, walk_r, sc, br, bc, skipped; u32 fin[kSeCap + 1]; };
constexpr u32 kChooseStride = 152;
struct SetIn { u32 L, n; u32 pos[kSeCap], flags[kSeCap]; int d[kSeCap]; u32 exact_p, exact_f; u32 tb_off; };
struct SetOut { u32 pos, flags; int diffs; u32 n_ops, n_aln, n_single; int overflow; u32 cig[kChooseStride]; };

#ifndef ALIGN_HOST_ONLY
#define HIPCHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("FAIL hip: %s (%s)\n", hipGetErrorString(e_), #x); std::exit(1); } } while (0)
template <class T> static T *up(const std::vector<T> &v) {
  T *d = nullptr;
  HIPCHK(hipMalloc(&d, std::max<size_t>(v.size(), 1) * sizeof(T)));
  if (!v.empty()) HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}
template <class T> static std::vector<T> down(const T *d, size_t n) {
  std::vector<T> v(n);
  HIPCHK(hipDeviceSynchronize());
  if (n) HIPCHK(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
  return v;
}
static void allow_lds(const void *kernel, size_t bytes) {
  if (bytes > 160 * 1024) { std::printf("FAIL lds %zu\n", bytes); std::exit(1); }
  if (bytes > 48 * 1024) HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)));
}

// the wave's LDS, carved by hand in the kernels' order of use: the table overlays window slots 1.. as in the kernels
__device__ __forceinline__ WaveLds carve(unsigned char *p, const Carve &c, u32 W, u32 GW, u32 max_jobs, u8 *tb_global, u32 *&fin) {
  WaveLds lds = {};
  lds.W = W; lds.GW = GW; lds.max_jobs = max_jobs;
  lds.qpk = reinterpret_cast<u64 *>(p); p += c.qwords * 8;
  lds.ctmp = reinterpret_cast<u32 *>(p); p += ((c.ctmp_words + 1u) & ~1u) * 4;
  lds.jpos = reinterpret_cast<u32 *>(p); p += kSeCap * 4;
  lds.jdf = reinterpret_cast<u32 *>(p); p += kSeCap * 4;
  lds.lbest = reinterpret_cast<int *>(p); p += 64 * 4;
  fin = reinterpret_cast<u32 *>(p); p += (kSeCap + 2) * 4;
  lds.gwin = reinterpret_cast<u64 *>(p);
  lds.tb = tb_global ? tb_global : p + GW * 8;
  return lds;
}
static_assert((2 * kSeCap * 4 + 64 * 4 + (kSeCap + 2) * 4) % 8 == 0, "gwin stays 8-byte aligned");

// one traceback run of one job on lanes [0, bw): the window staged as the kernels stage it, the table left in lds.tb
template <int VARIANT>
__device__ __forceinline__ void trace_one(const u64 *genome, const WaveLds &lds, u32 L, u32 bw, u32 pos, int &bv, int &brow) {
  const int lane = lane_id();
  if (lane == 0) { lds.jpos[0] = pos; lds.jdf[0] = ((bw - 1) / 2) << 16; }
  wave_sync();
  DevIndex ix = {};
  ix.genome = genome;
  ix.min_len = 32;
  stage_windows(ix, lds, 0, 1, kMd);
  wave_sync();
  AlnJob job = {0, 0, 0, 0, 0};
  const u64 t_beg = static_cast<u64>(pos) - static_cast<u64>((bw - 1) / 2);
  if (lane < static_cast<int>(bw)) { job.bw = static_cast<int>(bw); job.jl = lane; job.qoff = 0; job.t0nib = static_cast<int>(t_beg & 15u); }
  if constexpr (VARIANT == 0) wavefront<true, false>(lds, job, static_cast<int>(L), static_cast<int>(bw), static_cast<int>(bw), bv, brow);
  else if constexpr (VARIANT == 1) wavefront<true, true>(lds, job, static_cast<int>(L), static_cast<int>(bw), static_cast<int>(bw), bv, brow);
  else wavefront_rows<true>(lds, job, static_cast<int>(L), static_cast<int>(bw), bv, brow);
  wave_sync();
}

template <int VARIANT>
__global__ __launch_bounds__(64) void k_table(const u64 *genome, const u64 *reads, const TabCase *cs, Carve cv, u8 *tb_out, int tb_is_global,
                                              int *lane_out, int *fm_out) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x;
  const TabCase c = cs[blockIdx.x];
  u32 *fin;
  WaveLds lds = carve(smem, cv, c.W, c.GW, kMaxJobs, tb_is_global ? tb_out + c.out_off : nullptr, fin);
  for (u32 k = lane; k < c.W; k += 64) lds.qpk[k] = reads[c.read_off + k];
  const u32 cells = (c.L + c.bw) * c.bw;
  if (!tb_is_global) for (u32 k = lane; k < cells + 16; k += 64) lds.tb[k] = kFill;
  wave_sync();
  int bv, brow, sc, br, bc;
  trace_one<VARIANT>(genome, lds, c.L, c.bw, c.pos, bv, brow);
  first_maximum(static_cast<int>(c.bw), bv, brow, sc, br, bc);
  lane_out[(blockIdx.x * 64 + lane) * 2] = bv;
  lane_out[(blockIdx.x * 64 + lane) * 2 + 1] = brow;
  if (lane == 0) { fm_out[blockIdx.x * 3] = sc; fm_out[blockIdx.x * 3 + 1] = br; fm_out[blockIdx.x * 3 + 2] = bc; }
  if (!tb_is_global) for (u32 k = lane; k < cells + 16; k += 64) tb_out[c.out_off + k] = lds.tb[k];
}

// VARIANT 0 score_round<false>, 1 score_round<true>, 2 score_round_quad<false>, 3 score_round_quad<true> against c.floor
template <int VARIANT>
__global__ __launch_bounds__(64) void k_rounds(const u64 *genome, const u64 *reads, const ListCase *cs, const u32 *jpos, const u32 *jdf, Carve cv, ListOut *out) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x;
  const ListCase c = cs[blockIdx.x];
  ListOut &o = out[blockIdx.x];
  u32 *fin;
  WaveLds lds = carve(smem, cv, c.W, c.GW, c.max_jobs, nullptr, fin);
  for (u32 k = lane; k < c.n_enc * c.W; k += 64) lds.qpk[k] = reads[c.read_off + k];
  for (u32 k = lane; k < c.n; k += 64) { lds.jpos[k] = jpos[c.job_off + k]; lds.jdf[k] = jdf[c.job_off + k]; }
  wave_sync();
  DevIndex ix = {};
  ix.genome = genome;
  ix.min_len = 32;
  const int n = static_cast<int>(c.n), L = static_cast<int>(c.L), qbase = static_cast<int>(c.qbase);
  int first = 0, rounds = 0, bad = 0;
  u32 it[2] = {0, 0};
  while (first < n && rounds < static_cast<int>(kSeCap)) {
    const u32 it0 = it[0], it1 = it[1];
    int s;
    if constexpr (VARIANT == 0) s = score_round<false>(ix, lds, first, n, L, kMd, qbase);
    else if constexpr (VARIANT == 1) s = score_round<true>(ix, lds, first, n, L, kMd, qbase);
    else if constexpr (VARIANT == 2) s = score_round_quad<false>(ix, lds, first, n, L, kMd, qbase);
    else s = score_round_quad<true>(ix, lds, first, n, L, kMd, qbase, c.floor, it);
    s = uni(s);
    if (lane == 0) { o.round_end[rounds] = s; o.round_it[rounds][0] = it[0] - it0; o.round_it[rounds][1] = it[1] - it1; }
    ++rounds;
    if (!(s > first && s <= n)) { bad = 1; break; }  // (a round that takes nothing would never end)
    if (lane < s - first) { o.score[first + lane] = static_cast<i16>(lds.lbest[lane]); o.visits[first + lane] += 1; }
    wave_sync();
    first = s;
  }
  if (lane == 0) { o.n_rounds = rounds; o.bad = bad | (first < n ? 2 : 0); o.iters[0] = it[0]; o.iters[1] = it[1]; }
}

__global__ __launch_bounds__(64) void k_cigar(const u64 *genome, const u64 *reads, const CigCase *cs, Carve cv, u32 *slots, u32 *arenas, CigOut *out) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x;
  const CigCase c = cs[blockIdx.x];
  CigOut &o = out[blockIdx.x];
  u32 *fin;
  WaveLds lds = carve(smem, cv, c.W, c.GW, kMaxJobs, nullptr, fin);
  for (u32 k = lane; k < c.W; k += 64) lds.qpk[k] = reads[c.read_off + k];
  if (lane <= static_cast<int>(kSeCap)) fin[lane] = kCanary;
  if (lane == 0) lds.ctmp[c.ctmp_cap] = kCanary;
  wave_sync();
  int bv, brow, sc, br, bc;
  trace_one<2>(genome, lds, c.L, c.bw, c.pos, bv, brow);
  first_maximum(static_cast<int>(c.bw), bv, brow, sc, br, bc);
  wave_sync();
  u32 *slot = slots + static_cast<size_t>(blockIdx.x) * kSlotWords, *arena = arenas + static_cast<size_t>(blockIdx.x) * kArenaWords;
  u32 *counter = &o.arena_count;
  if (lane == 0) *counter = c.arena_count;
  wave_sync();
  const CigarSink sink = {c.stride, c.ctmp_cap, c.has_arena ? arena : nullptr, counter, c.arena_cap, c.want_fin ? fin : nullptr};
  u32 n_ops = 0, aln_len = 0, t_pos = c.pos, walk_n = 0;
  int ins = -1, del = -1, clip_head = 0, clip_tail = 0, walk_r = 0, skipped = 0;
  bool overflow = false;
  if (c.mode == 0) {
    if (sc > 0) {  // (as in the kernels: a table without a score is not walked)
      const CigarWalk w = cigar_walk(lds.tb, lds.ctmp, c.ctmp_cap, static_cast<int>(c.L), static_cast<int>(c.bw), br, bc, ins, del);
      cigar_publish(lds.ctmp, w, static_cast<int>(c.L), static_cast<int>(c.bw), slot, sink, n_ops, aln_len, t_pos, overflow);
      clip_head = w.clip_head; clip_tail = w.clip_tail; walk_n = w.n; walk_r = w.r;
    }
    else skipped = 1;
  }
  else wave_cigar(lds.tb, lds.ctmp, static_cast<int>(c.L), c.diffs, kMd, c.score0 ? 0 : sc, br, bc, slot, sink, n_ops, ins, del, aln_len, t_pos, overflow);
  wave_sync();
  if (lane == 0) {
    o.n_ops = n_ops; o.aln_len = aln_len; o.t_pos = t_pos; o.ins = ins; o.del = del; o.clip_head = clip_head; o.clip_tail = clip_tail;
    o.overflow = overflow; o.walk_n = walk_n; o.walk_r = walk_r; o.sc = sc; o.br = br; o.bc = bc; o.skipped = skipped;
    o.ctmp_guard = lds.ctmp[c.ctmp_cap];
  }
  if (lane <= static_cast<int>(kSeCap)) o.fin[lane] = fin[lane];
}

// edit_distance and long_enough against the host's int16_t arithmetic, compiled for the device: scores -1..300 (blockIdx.x),
// lengths 0..200 (blockIdx.y), ins and del 0..30; long_enough: alignment lengths 0..200 x read lengths 0..200 x two minima
__global__ __launch_bounds__(64) void k_grid(unsigned long long *mismatches, unsigned long long *sum, unsigned long long *first_bad) {
  const int scr = static_cast<int>(blockIdx.x) - 1;
  const u32 len = blockIdx.y;
  unsigned long long bad = 0, total = 0;
  for (int k = threadIdx.x; k < 31 * 31; k += 64) {
    const int ins = k / 31, del = k % 31;
    const int got = edit_distance(scr, len, ins, del), want = host_nm(scr, len, ins, del);
    total += static_cast<unsigned long long>(static_cast<u32>(got) & 0xFFFFu);
    if (got != want) { ++bad; atomicMin(first_bad, (static_cast<unsigned long long>(blockIdx.x) << 32) | (len << 16) | static_cast<u32>(k)); }
  }
  if (blockIdx.x <= 200) {
    for (u32 m = 0; m < 2; ++m) {
      const u32 min_len = m ? 32u : 0u;
      for (u32 rl = threadIdx.x; rl <= 200; rl += 64) {
        const bool got = long_enough(blockIdx.x, rl, min_len), want = host_long_enough(blockIdx.x, rl, min_len);
        if (blockIdx.y == 0) { total += got ? 1000003ull : 0ull; if (got != want) { ++bad; atomicMin(first_bad, 0xFFFF000000000000ull | (static_cast<unsigned long long>(blockIdx.x) << 16) | rl); } }
      }
    }
  }
  if (bad) atomicAdd(mismatches, bad);
  atomicAdd(sum, total);
}

template <bool WRAP>
__global__ __launch_bounds__(64) void k_choose(const u64 *genome, const u64 *reads, const SetIn *in, SetOut *out, Carve cv, u32 W, u32 GW, double frac, u8 *tb_global) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x;
  const SetIn &s = in[blockIdx.x];
  u32 *fin;
  WaveLds lds = carve(smem, cv, W, GW, WRAP ? 2u : kMaxJobs, WRAP ? tb_global + s.tb_off : nullptr, fin);
  for (u32 k = lane; k < 4 * W; k += 64) lds.qpk[k] = reads[static_cast<size_t>(blockIdx.x) * 4 * W + k];
  // (what choose_se does not set is harmless to read: a list entry it left out points into the genome, and the words in
  // front of the table end any walk that strays there)
  if (lane < static_cast<int>(kSeCap)) { lds.jpos[lane] = 4096u; lds.jdf[lane] = 1u << 16; }
  if (lane <= static_cast<int>(kSeCap) + 1) fin[lane] = 0u;
  wave_sync();
  DevIndex ix = {};
  ix.genome = genome;
  ix.min_len = 32;
  SeSet S;
  S.begin_read(s.L);
  S.sz = static_cast<int>(s.n);
  S.hk = lane < static_cast<int>(s.n) ? s.d[lane] * 256 + lane : 0;
  S.pp = lane < static_cast<int>(s.n) ? s.pos[lane] : 0u;
  S.pf = lane < static_cast<int>(s.n) ? s.flags[lane] : 0u;
  if (s.exact_p != 0) { S.best_p = s.exact_p; S.best_f = s.exact_f; S.best_d = 0; }
  Hit best;
  best.diffs = 0x7fff; best.flags = 0; best.pos = 0;
  u32 n_ops = 0, n_aln = 0, n_single = 0;
  bool overflow = false;
  const CigarSink sink = {kChooseStride, kChooseStride, nullptr, nullptr, 0, nullptr};
  choose_se<WRAP, false, false>(ix, lds, s.L, frac, S, best, out[blockIdx.x].cig, sink, n_ops, overflow, n_aln, n_single);
  if (lane == 0) {
    SetOut &o = out[blockIdx.x];
    o.pos = best.pos; o.flags = best.flags; o.diffs = best.diffs; o.n_ops = n_ops; o.n_aln = n_aln; o.n_single = n_single; o.overflow = overflow;
  }
}
#endif  // ALIGN_HOST_ONLY

static std::vector<u64> packed_genome(u32 pad_words) {
  std::vector<u64> gw(G.size() / 16 + pad_words, 0);
  for (size_t k = 0; k < G.size(); ++k) gw[k / 16] |= static_cast<u64>(G[k]) << (4 * (k % 16));
  return gw;
}
static std::string cigar_text(const std::vector<u32> &c) {
  std::string s;
  for (u32 o : c) { s += std::to_string(o >> 4); s += "MIDNS"[o & 15u]; }
  return s;
}

// ==== table, wrap ====================================================================================================
struct TabHost { TabCase c; int kind; std::vector<unsigned char> q; };
// is cell (i, j) one the anti-diagonal schedule of a lone job passes over?  steps t = bw - 1 .. 2 (L - 1 + bw), cell at t = 2 i + j
static bool antidiagonal_writes(int L, int bw, int i, int j) { const int t = 2 * i + j; return t >= bw - 1 && t <= 2 * (L - 1 + bw); }

static int compare_tables(const char *step, const std::vector<TabHost> &cases, const std::vector<Aligned> &want, int variant, const std::vector<u8> &tb,
                          const std::vector<int> &lanes, const std::vector<int> &fm, long long &unwritten) {
  static const char *const names[3] = {"wavefront<true, false>", "wavefront<true, true>", "wavefront_rows<true>"};
  for (size_t n = 0; n < cases.size(); ++n) {
    const TabCase &c = cases[n].c;
    const Aligned &a = want[n];
    const int L = static_cast<int>(c.L), bw = static_cast<int>(c.bw);
    for (int i = 0; i < L + bw; ++i)
      for (int j = 0; j < bw; ++j) {
        const u8 got = tb[c.out_off + static_cast<size_t>(i) * bw + j], exp = a.T[static_cast<size_t>(i) * bw + j];
        if (got == exp) continue;
        if (variant != 2 && got == kFill && exp == 3 && !antidiagonal_writes(L, bw, i, j)) { ++unwritten; continue; }
        std::printf("FAIL %s %s: case %zu (kind %d, L %d, band %d, t0nib %u): table row %d lane %d expected %u got %u\n", step, names[variant], n,
                    cases[n].kind, L, bw, (c.pos - (c.bw - 1) / 2) & 15u, i, j, exp, got);
        return 1;
      }
    for (int k = 0; k < 16; ++k)
      if (tb[c.out_off + static_cast<size_t>(L + bw) * bw + k] != kFill) {
        std::printf("FAIL %s %s: case %zu (L %d, band %d): byte %d behind the table written\n", step, names[variant], n, L, bw, k);
        return 1;
      }
    for (int j = 0; j < bw; ++j)
      if (lanes[(n * 64 + j) * 2] != a.colbest[j] || lanes[(n * 64 + j) * 2 + 1] != a.colrow[j]) {
        std::printf("FAIL %s %s: case %zu (kind %d, L %d, band %d): lane %d best %d in row %d, expected %d in row %d\n", step, names[variant], n, cases[n].kind, L,
                    bw, j, lanes[(n * 64 + j) * 2], lanes[(n * 64 + j) * 2 + 1], a.colbest[j], a.colrow[j]);
        return 1;
      }
    if (fm[n * 3] != a.score || fm[n * 3 + 1] != a.br || fm[n * 3 + 2] != a.bc) {
      std::printf("FAIL %s %s: case %zu (kind %d, L %d, band %d): first maximum %d at (%d, %d), expected %d at (%d, %d)\n", step, names[variant], n, cases[n].kind,
                  L, bw, fm[n * 3], fm[n * 3 + 1], fm[n * 3 + 2], a.score, a.br, a.bc);
      return 1;
    }
  }
  return 0;
}

static TabHost table_case(int L, int bw, int t0nib, int kind, int n, std::vector<u64> &reads, u32 &tb_off) {
  TabHost h;
  h.kind = kind;
  h.q = random_read(L);
  const u32 pos = place(bw, t0nib);
  plant_plan(h.q, pos, plan_of(kind, L, n));
  const u32 W = words_for(L);
  h.c = TabCase{static_cast<u32>(L), static_cast<u32>(bw), pos, W, se_window_words(static_cast<u32>(L), frac_for(L, bw)), static_cast<u32>(reads.size()), tb_off};
  reads.resize(reads.size() + W);
  pack(h.q, reads.data() + h.c.read_off, W);
  tb_off += ((h.c.L + h.c.bw) * h.c.bw + 16 + 15) & ~15u;
  return h;
}

static int do_table() {
  std::vector<TabHost> cases;
  std::vector<u64> reads;
  u32 tb_bytes = 0;
  int n = 0;
  for (int L : {33, 150})
    for (int bw = 1; bw <= 61; bw += 2)
      for (int t0 = 0; t0 < 16; ++t0, ++n) cases.push_back(table_case(L, bw, t0, n % 7, n / 7, reads, tb_bytes));
  for (int L : kLens) {
    if (L == 33 || L == 150) continue;
    for (int k = 0; k < 42; ++k, ++n) {
      const int bw = k == 0 ? 1 : (k == 1 ? 61 : 2 * rnd_in(0, 30) + 1), t0 = k == 2 ? 15 : rnd_in(0, 15);
      cases.push_back(table_case(L, bw, t0, n % 7, n / 7, reads, tb_bytes));
    }
  }
  std::vector<Aligned> want;
  int with_i = 0, with_d = 0, with_both = 0, left_ties = 0, above_ties = 0, twice = 0, zero = 0, pairs33 = 0, pairs150 = 0;
  Carve cv = {0, 2, kMaxJobs, 0, 0};
  for (const auto &h : cases) {
    want.push_back(host_align(h.q.data(), static_cast<int>(h.c.L), h.c.pos, static_cast<int>(h.c.bw), true, false, true));
    const Aligned &a = want.back();
    with_i += a.ins > 0 && a.del == 0; with_d += a.del > 0 && a.ins == 0; with_both += a.ins > 0 && a.del > 0;
    left_ties += a.left_ties; above_ties += a.above_ties; twice += a.max_cells > 1; zero += a.score == 0;
    pairs33 += h.c.L == 33; pairs150 += h.c.L == 150;
    cv.qwords = std::max(cv.qwords, h.c.W); cv.GW = std::max(cv.GW, h.c.GW); cv.tb_bytes = std::max(cv.tb_bytes, (h.c.L + h.c.bw) * h.c.bw);
  }
  long long unwritten = 0;
#ifndef ALIGN_HOST_ONLY
  const std::vector<u64> gw = packed_genome(cv.GW + 64);
  std::vector<TabCase> tc;
  for (const auto &h : cases) tc.push_back(h.c);
  const u64 *dg = up(gw), *dr = up(reads);
  const TabCase *dc = up(tc);
  u8 *dtb; int *dl, *dfm;
  HIPCHK(hipMalloc(&dtb, tb_bytes)); HIPCHK(hipMalloc(&dl, cases.size() * 128 * sizeof(int))); HIPCHK(hipMalloc(&dfm, cases.size() * 3 * sizeof(int)));
  const size_t lds = carve_bytes(cv);
  allow_lds(reinterpret_cast<const void *>(k_table<0>), lds); allow_lds(reinterpret_cast<const void *>(k_table<1>), lds); allow_lds(reinterpret_cast<const void *>(k_table<2>), lds);
  for (int variant = 0; variant < 3; ++variant) {
    HIPCHK(hipMemset(dtb, 0, tb_bytes));
    if (variant == 0) hipLaunchKernelGGL(k_table<0>, dim3(cases.size()), dim3(64), lds, 0, dg, dr, dc, cv, dtb, 0, dl, dfm);
    else if (variant == 1) hipLaunchKernelGGL(k_table<1>, dim3(cases.size()), dim3(64), lds, 0, dg, dr, dc, cv, dtb, 0, dl, dfm);
    else hipLaunchKernelGGL(k_table<2>, dim3(cases.size()), dim3(64), lds, 0, dg, dr, dc, cv, dtb, 0, dl, dfm);
    HIPCHK(hipGetLastError());
    const std::vector<u8> tb = down(dtb, tb_bytes);
    const std::vector<int> lanes = down(dl, cases.size() * 128), fm = down(dfm, cases.size() * 3);
    if (compare_tables("table", cases, want, variant, tb, lanes, fm, unwritten)) return 1;
  }
#endif
  const bool live = with_i && with_d && with_both && left_ties && above_ties && twice && zero && pairs33 == 496 && pairs150 == 496;
  std::printf("%s table %zu cases x 3 runs; tables with an I run %d, with a D run %d, with both %d, cells where left tied and won %d, where above tied with the "
              "diagonal %d, tables with the maximum twice %d, without a score %d, (band, t0nib) pairs at L 33 %d, at L 150 %d, cells the anti-diagonal runs leave "
              "unwritten (all outside the read) %lld\n", !live ? "FAIL coverage:" : (kDevice ? "OK" : "HOST"), cases.size(), with_i, with_d, with_both, left_ties,
              above_ties, twice, zero, pairs33, pairs150, unwritten);
  return live ? 0 : 1;
}

// a near-perfect copy of a long read: an indel every few thousand bases
static void plant_long(const std::vector<unsigned char> &q, u32 pos, int every, int phase) {
  Plan p;
  for (int at = every / 2 + phase, k = 0; at < static_cast<int>(q.size()) - 100; at += every, ++k) p.gaps.push_back({at, (k & 1) ? 1 : -1});
  p.subs = 1;
  plant_plan(q, pos, p);
}

static int do_wrap() {
  std::vector<TabHost> cases;
  std::vector<u64> reads;
  std::vector<ListCase> lists;
  std::vector<u32> jpos, jdf;
  std::vector<Aligned> want;
  u32 tb_bytes = 0;
  int score_differs = 0, cells_differ_tables = 0, clamped_cells = 0;
  Carve cv = {0, 2, 2, 0, 0};
  for (int L : {16400, 20000}) {
    const std::vector<unsigned char> q = random_read(L);
    const u32 W = words_for(L), GW = se_window_words(static_cast<u32>(L), 0.1), read_off = static_cast<u32>(reads.size());
    reads.resize(reads.size() + W);
    pack(q, reads.data() + read_off, W);
    lists.push_back(ListCase{static_cast<u32>(L), 2, W, GW, 2, 0, 1, read_off, static_cast<u32>(jpos.size()), 0});
    for (int k = 0; k < 2; ++k) {
      const u32 pos = place(61, k ? 15 : 3, static_cast<u32>(L) + 2048);
      plant_long(q, pos, k ? 7000 : 6000, 100 * k);
      TabHost h;
      h.kind = 7; h.q = q;
      h.c = TabCase{static_cast<u32>(L), 61, pos, W, GW, read_off, tb_bytes};
      tb_bytes += ((h.c.L + 61) * 61 + 16 + 15) & ~15u;
      cases.push_back(h);
      jpos.push_back(pos); jdf.push_back(30u << 16);
      want.push_back(host_align(q.data(), L, pos, 61, true, true, true));
      const Aligned wide = host_align(q.data(), L, pos, 61, true, false, true);
      size_t differ = 0;
      for (size_t c = 0; c < wide.T.size(); ++c) differ += wide.T[c] != want.back().T[c];
      if (wide.score == want.back().score || differ == 0) {
        std::printf("FAIL wrap: L %d job %d: the 16-bit host DP scores %d, the 32-bit one %d, %zu table cells differ: the narrowing is not live\n", L, k,
                    want.back().score, wide.score, differ);
        return 1;
      }
      ++score_differs; cells_differ_tables += differ > 0; clamped_cells += static_cast<int>(differ);
    }
    cv.qwords = std::max(cv.qwords, W); cv.GW = std::max(cv.GW, GW);
  }
#ifndef ALIGN_HOST_ONLY
  const std::vector<u64> gw = packed_genome(cv.GW + 64);
  std::vector<TabCase> tc;
  for (const auto &h : cases) tc.push_back(h.c);
  const u64 *dg = up(gw), *dr = up(reads);
  const TabCase *dc = up(tc);
  u8 *dtb; int *dl, *dfm;
  HIPCHK(hipMalloc(&dtb, tb_bytes)); HIPCHK(hipMalloc(&dl, cases.size() * 128 * sizeof(int))); HIPCHK(hipMalloc(&dfm, cases.size() * 3 * sizeof(int)));
  HIPCHK(hipMemset(dtb, kFill, tb_bytes));
  const size_t lds = carve_bytes(cv);
  allow_lds(reinterpret_cast<const void *>(k_table<1>), lds); allow_lds(reinterpret_cast<const void *>(k_rounds<1>), lds);
  hipLaunchKernelGGL(k_table<1>, dim3(cases.size()), dim3(64), lds, 0, dg, dr, dc, cv, dtb, 1, dl, dfm);
  HIPCHK(hipGetLastError());
  const std::vector<u8> tb = down(dtb, tb_bytes);
  const std::vector<int> lanes = down(dl, cases.size() * 128), fm = down(dfm, cases.size() * 3);
  long long unwritten = 0;
  if (compare_tables("wrap", cases, want, 1, tb, lanes, fm, unwritten)) return 1;
  ListOut *dout;
  HIPCHK(hipMalloc(&dout, lists.size() * sizeof(ListOut)));
  HIPCHK(hipMemset(dout, 0, lists.size() * sizeof(ListOut)));
  hipLaunchKernelGGL(k_rounds<1>, dim3(lists.size()), dim3(64), lds, 0, dg, dr, up(lists), up(jpos), up(jdf), cv, dout);
  HIPCHK(hipGetLastError());
  const std::vector<ListOut> out = down(dout, lists.size());
  for (size_t l = 0; l < lists.size(); ++l)
    for (int k = 0; k < 2; ++k)
      if (out[l].bad || out[l].n_rounds != 1 || out[l].visits[k] != 1 || out[l].score[k] != want[2 * l + k].score) {
        std::printf("FAIL wrap score_round<true>: L %u job %d: score %d (%d visits, %d rounds, flag %d), the 16-bit host DP %d\n", lists[l].L, k, out[l].score[k],
                    out[l].visits[k], out[l].n_rounds, out[l].bad, want[2 * l + k].score);
        return 1;
      }
#endif
  std::printf("%s wrap %zu jobs of 16400 and 20000 bases, band 61; 16-bit and 32-bit host scores differ in %d, tables in %d (%d cells)\n", kDevice ? "OK" : "HOST",
              cases.size(), score_differs, cells_differ_tables, clamped_cells);
  return 0;
}

// ==== rounds, floor ==================================================================================================
struct ListHost { ListCase c; std::vector<int> band, score; std::vector<u32> flags; };
static const u32 kEncFlags[4] = {0u, kHostFlagARich, kHostFlagRC | kHostFlagARich, kHostFlagRC};  // encodings 0, 1, 2, 3
static void add_list(std::vector<ListHost> &lists, std::vector<u64> &reads, std::vector<u32> &jpos, std::vector<u32> &jdf, int L, const std::vector<int> &bands,
                     bool end1, u32 max_jobs) {
  ListHost h;
  const u32 W = words_for(L);
  std::vector<unsigned char> enc[8];
  const u32 read_off = static_cast<u32>(reads.size());
  reads.resize(reads.size() + 8 * W);
  for (int e = 0; e < 8; ++e) { enc[e] = random_read(L); pack(enc[e], reads.data() + read_off + e * W, W); }  // (eight different reads; an end's other four are garbage to it)
  h.c = ListCase{static_cast<u32>(L), static_cast<u32>(bands.size()), W, se_window_words(static_cast<u32>(L), frac_for(L, 61)), max_jobs, end1 ? 4 * W : 0u, 8, read_off,
                 static_cast<u32>(jpos.size()), 0};
  h.band = bands;
  for (size_t k = 0; k < bands.size(); ++k) {
    const int bw = bands[k], half = (bw - 1) / 2;
    const u32 flags = kEncFlags[(k + lists.size()) % 4];
    const std::vector<unsigned char> &q = enc[(end1 ? 4 : 0) + host_enc_of(flags)];
    const u32 pos = place(bw, k % 5 == 0 ? 15 : rnd_in(0, 15));
    Plan p;
    const int kind = rnd_in(0, 9);
    if (kind < 5) p.subs = rnd_in(0, 6);
    else if (kind < 8) { if (half > 0) { const int g = rnd_in(1, std::min(half, L / 2 - 4)); p.gaps.push_back({rnd_in(2, L - g - 3), rnd() & 1 ? g : -g}); } p.subs = rnd_in(0, 3); }
    else if (kind == 8) p.all_mismatch = true;
    else { p.iupac = rnd_in(1, 6); p.zeros = rnd_in(0, 2); p.subs = rnd_in(0, 8); }
    plant_plan(q, pos, p);
    h.flags.push_back(flags);
    h.score.push_back(host_align(q.data(), L, pos, bw, false).score);
    jpos.push_back(pos);
    jdf.push_back((static_cast<u32>(half) << 16) | flags);
  }
  lists.push_back(h);
}
static void build_lists(std::vector<ListHost> &lists, std::vector<u64> &reads, std::vector<u32> &jpos, std::vector<u32> &jdf, int n_random) {
  for (int L : {33, 64, 100, 150}) {
    auto add = [&](const std::vector<int> &b, bool end1 = false, u32 mj = kMaxJobs) { add_list(lists, reads, jpos, jdf, L, b, end1, mj); };
    add(std::vector<int>(5, 61));                      // all bands 61, an odd count (4m + 1)
    add(std::vector<int>(kSeCap, 1));                  // all bands 1 (4m + 2)
    add(std::vector<int>(49, 3));                      // all bands 3
    add({61, 61, 3, 3, 5, 7, 9});                      // two-set: 61 + 3 = 64 lanes (4m + 3)
    add({61, 5, 7, 9, 3, 1, 3, 1, 11, 13});            // packed: 61 + 3 = 64 lanes
    add({21, 19, 21, 21, 17, 21, 1, 1, 5});            // two-set: 21 + 21 + 21 + 1 = 64
    add({21, 21, 21, 21, 21, 21, 1});                  // the same with a lone last job
    add({21, 21, 21, 21, 23, 23, 3});                  // two-set: 21 + 21 + 23 = 65
    add({21, 1, 3, 5, 21, 7, 9, 11, 23, 1, 1, 1, 3});  // packed: 21 + 21 + 23 = 65
    add({1, 61, 7, 21, 3, 3});                         // a slot of four different half-widths, 1 and 61 among them
    add({7, 21, 1, 61, 61, 1, 21, 7}, true);           // the same from end 1's encodings
    add({1});
    add({61});
    add({5, 9}, true);
    add({61, 61, 61, 3, 21, 1, 1}, false, 2);          // the long-read layout: one slot a round
    add({3, 61}, true, 2);
    for (int k = 0; k < n_random; ++k) {
      std::vector<int> b(rnd_in(1, kSeCap));
      const int top = k % 3 == 0 ? 30 : (k % 3 == 1 ? 6 : 2);
      for (auto &x : b) x = 2 * rnd_in(0, top) + 1;
      add(b, (k & 3) == 3, k % 7 == 6 ? 2u : kMaxJobs);
    }
  }
}
// the rounds a list is scored in when every round takes what the header says it may: consecutive jobs share a slot (two, or four
// packed), slots side by side while they fit 64 lanes and the jobs fit max_jobs window slots (the two-set round counts a slot as two)
static std::vector<int> host_rounds(const ListHost &h, bool quad) {
  std::vector<int> ends;
  const int n = static_cast<int>(h.band.size()), g = quad ? 4 : 2;
  for (int first = 0; first < n;) {
    int s = first, used = 0;
    while (s < n) {
      const int cnt = std::min(g, n - s);
      if (s - first + (quad ? cnt : 2) > static_cast<int>(h.c.max_jobs)) break;
      int width = 0;
      for (int k = 0; k < cnt; ++k) width = std::max(width, h.band[s + k]);
      if (used + width > 64) break;
      used += width; s += cnt;
    }
    if (s == first) break;
    ends.push_back(s);
    first = s;
  }
  return ends;
}
struct Live {
  int lists = 0, jobs = 0, rounds = 0, side_by_side = 0, widths_differ = 0, lone_last = 0, later_rounds = 0, exact64 = 0, stop65 = 0, stop_lanes = 0, stop_jobs = 0,
      four_widths = 0, all61 = 0, all1 = 0, all3 = 0, slots3 = 0, end1 = 0, two_slots = 0, odd = 0, mod4[4] = {0, 0, 0, 0}, enc[4] = {0, 0, 0, 0};
};
static void tally(Live &v, const ListHost &h, const std::vector<int> &ends, bool quad) {
  const int n = static_cast<int>(h.band.size()), g = quad ? 4 : 2;
  ++v.lists; v.jobs += n; v.end1 += h.c.qbase != 0; v.two_slots += h.c.max_jobs == 2; v.odd += n & 1; ++v.mod4[n & 3];
  for (u32 f : h.flags) ++v.enc[host_enc_of(f)];
  int first = 0;
  for (int s : ends) {
    int used = 0, slots = 0, lo = 64, hi = 0;
    for (int a = first; a < s; a += g, ++slots) {
      const int cnt = std::min(g, s - a);
      int width = 0;
      for (int k = 0; k < cnt; ++k) { width = std::max(width, h.band[a + k]); lo = std::min(lo, h.band[a + k]); hi = std::max(hi, h.band[a + k]); }
      used += width;
      if (quad && cnt == 4) {
        std::vector<int> b(h.band.begin() + a, h.band.begin() + a + 4);
        std::sort(b.begin(), b.end());
        v.four_widths += b[0] == 1 && b[3] == 61 && b[0] != b[1] && b[1] != b[2] && b[2] != b[3];
      }
    }
    ++v.rounds; v.side_by_side += slots > 1; v.widths_differ += lo != hi; v.lone_last += !quad && ((s - first) & 1); v.later_rounds += first != 0;
    v.exact64 += used == 64 && slots > 1;
    v.all61 += lo == 61; v.all1 += hi == 1; if (lo == 3 && hi == 3) { ++v.all3; v.slots3 = std::max(v.slots3, slots); }
    if (s < n) {
      const int cnt = std::min(g, n - s);
      int width = 0;
      for (int k = 0; k < cnt; ++k) width = std::max(width, h.band[s + k]);
      if (s - first + (quad ? cnt : 2) > static_cast<int>(h.c.max_jobs)) ++v.stop_jobs;
      else if (used + width == 65) ++v.stop65;
      else ++v.stop_lanes;
    }
    first = s;
  }
}
static bool live_enough(const Live &v, bool quad, bool two_slot_lists) {
  return v.side_by_side && v.widths_differ && (quad || v.lone_last) && v.later_rounds && v.exact64 && v.stop65 && v.stop_jobs && (!quad || v.four_widths) && v.all61 &&
         v.all1 && v.all3 && v.end1 && (!two_slot_lists || v.two_slots) && v.odd && v.mod4[1] && v.mod4[2] && v.mod4[3] && v.enc[0] && v.enc[1] && v.enc[2] && v.enc[3];
}
static void print_live(const Live &v) {
  std::printf("%d lists, %d jobs, %d rounds; rounds with slots side by side %d, with bands of different widths %d, with a lone last job %d, with first != 0 %d, filling "
              "exactly 64 lanes %d, cut at 65 lanes %d, cut at more %d, cut by max_jobs %d, slots of four different widths with 1 and 61 %d, rounds all of band 61 %d, "
              "of band 1 %d, of band 3 %d (up to %d slots), lists from end 1's encodings %d, with max_jobs 2 %d, of odd length %d, of length 4m+1 %d 4m+2 %d 4m+3 %d, "
              "jobs per encoding %d %d %d %d", v.lists, v.jobs, v.rounds, v.side_by_side, v.widths_differ, v.lone_last, v.later_rounds, v.exact64, v.stop65, v.stop_lanes,
              v.stop_jobs, v.four_widths, v.all61, v.all1, v.all3, v.slots3, v.end1, v.two_slots, v.odd, v.mod4[1], v.mod4[2], v.mod4[3], v.enc[0], v.enc[1], v.enc[2], v.enc[3]);
}
// what every run of a list must satisfy, whatever the scores: first < s <= n_jobs, at most max_jobs jobs a round, every job once
static int check_rounds(const char *name, size_t l, const ListHost &h, const ListOut &o, std::vector<int> &ends) {
  const int n = static_cast<int>(h.band.size());
  ends.clear();
  int first = 0;
  for (int r = 0; r < o.n_rounds; ++r) {
    const int s = o.round_end[r];
    if (!(s > first && s <= n) || s - first > static_cast<int>(h.c.max_jobs)) {
      std::printf("FAIL %s: list %zu (L %u, %d jobs, max_jobs %u): round %d from job %d returned %d\n", name, l, h.c.L, n, h.c.max_jobs, r, first, s);
      return 1;
    }
    ends.push_back(s);
    first = s;
  }
  if (o.bad || first != n) { std::printf("FAIL %s: list %zu (L %u, %d jobs): the rounds ended at job %d (flag %d)\n", name, l, h.c.L, n, first, o.bad); return 1; }
  for (int k = 0; k < n; ++k)
    if (o.visits[k] != 1) { std::printf("FAIL %s: list %zu (L %u, %d jobs): job %d scored %d times\n", name, l, h.c.L, n, k, o.visits[k]); return 1; }
  return 0;
}

static int do_rounds() {
  std::vector<ListHost> lists;
  std::vector<u64> reads;
  std::vector<u32> jpos, jdf;
  build_lists(lists, reads, jpos, jdf, 14);
  static const char *const names[3] = {"score_round<false>", "score_round<true>", "score_round_quad<false>"};
  Live live[3];
#ifndef ALIGN_HOST_ONLY
  Carve cv = {8 * words_for(150), 2, kMaxJobs, se_window_words(150, frac_for(150, 61)), 0};
  const std::vector<u64> gw = packed_genome(cv.GW + 64);
  const u64 *dg = up(gw), *dr = up(reads);
  const u32 *dp = up(jpos), *df = up(jdf);
  const size_t lds = carve_bytes(cv);
#endif
  for (int variant = 0; variant < 3; ++variant) {
    std::vector<size_t> which;
    for (size_t l = 0; l < lists.size(); ++l) if (variant != 2 || lists[l].c.max_jobs == kMaxJobs) which.push_back(l);
#ifndef ALIGN_HOST_ONLY
    std::vector<ListCase> lc;
    for (size_t l : which) lc.push_back(lists[l].c);
    ListOut *dout;
    HIPCHK(hipMalloc(&dout, lc.size() * sizeof(ListOut)));
    HIPCHK(hipMemset(dout, 0, lc.size() * sizeof(ListOut)));
    if (variant == 0) hipLaunchKernelGGL(k_rounds<0>, dim3(lc.size()), dim3(64), lds, 0, dg, dr, up(lc), dp, df, cv, dout);
    else if (variant == 1) hipLaunchKernelGGL(k_rounds<1>, dim3(lc.size()), dim3(64), lds, 0, dg, dr, up(lc), dp, df, cv, dout);
    else hipLaunchKernelGGL(k_rounds<2>, dim3(lc.size()), dim3(64), lds, 0, dg, dr, up(lc), dp, df, cv, dout);
    HIPCHK(hipGetLastError());
    const std::vector<ListOut> out = down(dout, lc.size());
#endif
    for (size_t w = 0; w < which.size(); ++w) {
      const ListHost &h = lists[which[w]];
      std::vector<int> ends = host_rounds(h, variant == 2);
#ifndef ALIGN_HOST_ONLY
      if (check_rounds(names[variant], which[w], h, out[w], ends)) return 1;
      for (size_t k = 0; k < h.band.size(); ++k)
        if (out[w].score[k] != h.score[k]) {
          std::printf("FAIL rounds %s: list %zu (L %u, %zu jobs, max_jobs %u, qbase %u): job %zu (band %d, t0nib %u, flags %x) scored %d, the host DP %d\n", names[variant],
                      which[w], h.c.L, h.band.size(), h.c.max_jobs, h.c.qbase, k, h.band[k], (jpos[h.c.job_off + k] - (h.band[k] - 1) / 2) & 15u, h.flags[k],
                      out[w].score[k], h.score[k]);
          return 1;
        }
#endif
      tally(live[variant], h, ends, variant == 2);
    }
  }
  bool ok = true;
  for (int variant = 0; variant < 3; ++variant) ok = ok && live_enough(live[variant], variant == 2, variant != 2);
  std::printf("%s rounds", !ok ? "FAIL coverage:" : (kDevice ? "OK" : "HOST"));
  for (int variant = 0; variant < 3; ++variant) { std::printf("%s %s: ", variant ? ";" : "", names[variant]); print_live(live[variant]); }
  std::printf("\n");
  return ok ? 0 : 1;
}

static int host_quad_iterations(int L, int w_min, int w_max) {  // anti-diagonal steps max(0, w_min - 1) .. 2 (L - 1 + w_max) + 1, two an iteration
  return (2 * (L - 1 + w_max) + 1 - std::max(0, w_min - 1)) / 2 + 1;
}
static int do_floor() {
  std::vector<ListHost> lists;
  std::vector<u64> reads;
  std::vector<u32> jpos, jdf;
  build_lists(lists, reads, jpos, jdf, 8);
  std::vector<size_t> which;
  std::vector<ListCase> lc;
  for (size_t l = 0; l < lists.size(); ++l) {
    if (lists[l].c.max_jobs != kMaxJobs) continue;
    std::vector<int> sorted(lists[l].score);
    std::sort(sorted.begin(), sorted.end());
    const int floors[5] = {sorted.back(), sorted[sorted.size() / 2], 1, 0, -1};
    for (int f : floors) { which.push_back(l); lc.push_back(lists[l].c); lc.back().floor = f; }
  }
  Live live;
  int early = 0, full_positive = 0, below = 0, exact = 0, nonpositive = 0;
#ifndef ALIGN_HOST_ONLY
  Carve cv = {8 * words_for(150), 2, kMaxJobs, se_window_words(150, frac_for(150, 61)), 0};
  const std::vector<u64> gw = packed_genome(cv.GW + 64);
  const size_t lds = carve_bytes(cv);
  ListOut *dout;
  HIPCHK(hipMalloc(&dout, lc.size() * sizeof(ListOut)));
  HIPCHK(hipMemset(dout, 0, lc.size() * sizeof(ListOut)));
  hipLaunchKernelGGL(k_rounds<3>, dim3(lc.size()), dim3(64), lds, 0, up(gw), up(reads), up(lc), up(jpos), up(jdf), cv, dout);
  HIPCHK(hipGetLastError());
  const std::vector<ListOut> out = down(dout, lc.size());
#endif
  for (size_t w = 0; w < which.size(); ++w) {
    const ListHost &h = lists[which[w]];
    const int floor = lc[w].floor, L = static_cast<int>(h.c.L);
    (void)L;
    std::vector<int> ends = host_rounds(h, true);
#ifndef ALIGN_HOST_ONLY
    const ListOut &o = out[w];
    if (check_rounds("floor", which[w], h, o, ends)) return 1;
    for (size_t k = 0; k < h.band.size(); ++k) {
      const bool holds = h.score[k] >= floor ? o.score[k] == h.score[k] : (o.score[k] < floor && o.score[k] <= h.score[k] && o.score[k] >= 0);
      if (!holds) {
        std::printf("FAIL floor: list %zu (L %d, %zu jobs) floor %d: job %zu (band %d) reports %d, the host DP %d\n", which[w], L, h.band.size(), floor, k, h.band[k],
                    o.score[k], h.score[k]);
        return 1;
      }
      below += h.score[k] < floor; exact += h.score[k] >= floor;
    }
    u32 full = 0;
    int first = 0;
    for (size_t r = 0; r < ends.size(); ++r) {
      int w_min = 64, w_max = 0;
      for (int a = first; a < ends[r]; a += 4) {
        int width = 0;
        for (int k = a; k < std::min(a + 4, ends[r]); ++k) width = std::max(width, h.band[k]);
        w_min = std::min(w_min, width); w_max = std::max(w_max, width);
      }
      const u32 all = static_cast<u32>(host_quad_iterations(L, w_min, w_max));
      if (o.round_it[r][1] != all || o.round_it[r][0] > all || o.round_it[r][0] == 0 || (floor <= 0 && o.round_it[r][0] != all)) {
        std::printf("FAIL floor: list %zu (L %d) floor %d: round %zu (jobs %d..%d, slots of %d..%d lanes) ran %u iterations of %u, a full run has %u\n", which[w], L, floor,
                    r, first, ends[r], w_min, w_max, o.round_it[r][0], o.round_it[r][1], all);
        return 1;
      }
      early += o.round_it[r][0] < all; full_positive += floor > 0 && o.round_it[r][0] == all;
      full += all;
      first = ends[r];
    }
    if (o.iters[1] != full || o.iters[0] > o.iters[1] || (floor <= 0 && o.iters[0] != o.iters[1])) {
      std::printf("FAIL floor: list %zu (L %d) floor %d: iters %u of %u, the rounds' full runs sum to %u\n", which[w], L, floor, o.iters[0], o.iters[1], full);
      return 1;
    }
#endif
    nonpositive += floor <= 0;
    tally(live, h, ends, true);
  }
  const bool ok = live_enough(live, true, false) && (!kDevice || (early && full_positive && below && exact)) && nonpositive;
  std::printf("%s floor score_round_quad<true>: runs with floor <= 0 %d, rounds that ended early %d, that ran to the end with a positive floor %d, jobs below the floor %d, "
              "at or above it %d; ", !ok ? "FAIL coverage:" : (kDevice ? "OK" : "HOST"), nonpositive, early, full_positive, below, exact);
  print_live(live);
  std::printf("\n");
  return ok ? 0 : 1;
}

// ==== cigar ==========================================================================================================
struct CigHost { CigCase c; size_t base; int sink_kind; };
enum SinkKind : int { kRoom, kFills, kArenaRoom, kArenaExact, kArenaShort, kArenaPast, kNoArena, kFewKept, kTinySlot, kShortScore0, kShortDiffs0, kWaveCigar, kSinkKinds };
static const char *const kSinkNames[kSinkKinds] = {"full < stride", "full == stride", "full == stride + 1, arena with room", "arena fits exactly", "arena one op short",
                                                   "arena counter past arena_cap", "null arena", "ctmp_cap below the walk's ops", "slot of two ops, no arena",
                                                   "wave_cigar told score 0", "wave_cigar told diffs 0", "wave_cigar"};
static int do_cigar() {
  struct Base { TabHost t; Aligned a; };
  std::vector<Base> bases;
  std::vector<u64> reads;
  u32 unused = 0;
  int n = 0;
  for (int L : kLens)
    for (int k = 0; k < 14; ++k, ++n) {
      Base b;
      if (k < 11) {
        static const int kinds[11] = {0, 1, 1, 1, 4, 5, 5, 6, 3, 2, 0};
        const int kind = kinds[k], bw = kind == 2 || k == 10 ? 1 : 2 * rnd_in(kind == 0 ? 1 : 3, 30) + 1;
        const int t0 = rnd_in(0, 15);
        b.t = table_case(L, bw, t0, kind, n, reads, unused);
      }
      else {  // a CIGAR of many ops: every few bases an indel, insertions and deletions in turn
        const int bw = 2 * rnd_in(1, 4) + 1, t0 = rnd_in(0, 15);
        b.t = table_case(L, bw, t0, 2, n, reads, unused);
        Plan p;
        const int period = k == 11 ? 4 : (k == 12 ? 5 : 7);
        for (int at = period, g = 0; at < L - period; at += period, ++g) p.gaps.push_back({at, (g & 1) ? 1 : -1});
        plant_plan(b.t.q, b.t.c.pos, p);
      }
      b.a = host_align(b.t.q.data(), L, b.t.c.pos, static_cast<int>(b.t.c.bw), true, false, true);
      bases.push_back(b);
    }
  std::vector<CigHost> cases;
  int live[kSinkKinds] = {0}, fin_long = 0, with_head = 0, with_tail = 0, gapped = 0, truncated_body = 0;
  for (size_t b = 0; b < bases.size(); ++b) {
    const TabCase &t = bases[b].t.c;
    const Aligned &a = bases[b].a;
    const u32 F = static_cast<u32>(a.cigar.size()), cap = t.L + 2;
    auto add = [&](int kind, u32 stride, u32 ctmp_cap, int has_arena, u32 arena_cap, u32 arena_count, int want_fin, int mode, int diffs, int score0) {
      cases.push_back(CigHost{CigCase{t.L, t.bw, t.pos, t.W, t.GW, t.read_off, stride, ctmp_cap, arena_cap, arena_count, has_arena, want_fin, mode, diffs, score0}, b, kind});
      ++live[kind];
    };
    const int d = static_cast<int>(t.bw - 1) / 2;
    add(kShortScore0, F + 1, cap, 1, 200, 17, b & 1, 1, d, 1);
    if (t.bw == 1) add(kShortDiffs0, F + 1, cap, 1, 200, 17, b & 1, 1, 0, 0);
    if (t.bw > 1) add(kWaveCigar, b % 3 ? F : F - (F > 1), cap, 1, 200, 17, 1, 1, d, 0);  // (told diffs > 0: score 0 takes the shortcut, any other the walk)
    if (a.score == 0) continue;
    add(kRoom, F + 3, cap, 1, 200, 17, 1, 0, 0, 0);
    add(kFills, F, cap, 0, 0, 0, b & 1, 0, 0, 0);
    if (F < 2) continue;
    add(kArenaRoom, F - 1, cap, 1, 200, 17, 1, 0, 0, 0);
    add(kArenaExact, F - 1, cap, 1, 17 + F, 17, 0, 0, 0, 0);
    add(kArenaShort, F - 1, cap, 1, 17 + F - 1, 17, b & 1, 0, 0, 0);
    add(kArenaPast, F > 2 ? F - 2 : 1, cap, 1, 40, 45, 1, 0, 0, 0);
    add(kNoArena, F - 1, cap, 0, 0, 0, 0, 0, 0, 0);
    add(kTinySlot, F > 2 ? 2 : 1, cap, 0, 0, 0, 1, 0, 0, 0);
    if (a.n_body >= 2) add(kFewKept, F - 1, a.n_body - 1, 1, 200, 17, b & 1, 0, 0, 0);
    fin_long += F > kSeCap; with_head += a.clip_head > 0; with_tail += a.clip_tail > 0; gapped += a.ins > 0 || a.del > 0;
    truncated_body += a.n_body > 2;
  }
#ifndef ALIGN_HOST_ONLY
  Carve cv = {words_for(151), 151 + 4, kMaxJobs, 0, 0};
  for (const auto &b : bases) { cv.GW = std::max(cv.GW, b.t.c.GW); cv.tb_bytes = std::max(cv.tb_bytes, (b.t.c.L + b.t.c.bw) * b.t.c.bw); }
  const std::vector<u64> gw = packed_genome(cv.GW + 64);
  std::vector<CigCase> cc;
  for (const auto &c : cases) cc.push_back(c.c);
  std::vector<u32> slots_in(cases.size() * kSlotWords, kUnwritten), arenas_in(cases.size() * kArenaWords, kUnwritten);
  u32 *dslots = up(slots_in), *darenas = up(arenas_in);
  CigOut *dout;
  HIPCHK(hipMalloc(&dout, cases.size() * sizeof(CigOut)));
  HIPCHK(hipMemset(dout, 0, cases.size() * sizeof(CigOut)));
  const size_t lds = carve_bytes(cv);
  allow_lds(reinterpret_cast<const void *>(k_cigar), lds);
  hipLaunchKernelGGL(k_cigar, dim3(cases.size()), dim3(64), lds, 0, up(gw), up(reads), up(cc), cv, dslots, darenas, dout);
  HIPCHK(hipGetLastError());
  const std::vector<CigOut> out = down(dout, cases.size());
  const std::vector<u32> slots = down(dslots, slots_in.size()), arenas = down(darenas, arenas_in.size());
  for (size_t n = 0; n < cases.size(); ++n) {
    const CigCase &c = cases[n].c;
    const Aligned &a = bases[cases[n].base].a;
    const CigOut &o = out[n];
    const bool shortcut = c.mode == 1 && (c.score0 || c.diffs == 0 || a.score == 0);
    Aligned e = a;
    if (shortcut) { e = Aligned{}; e.cigar = {c.L << 4}; e.alen = c.L; e.pos = c.pos; }
    const Published p = host_publish(e, HostSink{c.stride, c.ctmp_cap, c.has_arena != 0, c.arena_cap, c.arena_count, c.want_fin != 0});
    auto fail = [&](const char *what, long long exp, long long got) {
      std::printf("FAIL cigar: case %zu (%s; L %u, band %u, CIGAR %s, stride %u, ctmp_cap %u, arena %d cap %u counter %u, fin %d): %s expected %lld got %lld\n", n,
                  kSinkNames[cases[n].sink_kind], c.L, c.bw, cigar_text(a.cigar).c_str(), c.stride, c.ctmp_cap, c.has_arena, c.arena_cap, c.arena_count, c.want_fin, what, exp, got);
      return 1;
    };
    if (o.skipped) return fail("a table with a score: walked", 0, 1);
    if (o.sc != a.score || o.br != a.br || o.bc != a.bc) return fail("first maximum's score", a.score, o.sc);
    if (o.n_ops != p.n_ops) return fail("n_ops", p.n_ops, o.n_ops);
    if (o.aln_len != e.alen) return fail("aln_len", e.alen, o.aln_len);
    if (o.t_pos != e.pos) return fail("t_pos", e.pos, o.t_pos);
    if (o.ins != e.ins) return fail("ins", e.ins, o.ins);
    if (o.del != e.del) return fail("del", e.del, o.del);
    if (c.mode == 0 && o.clip_head != a.clip_head) return fail("clip_head", a.clip_head, o.clip_head);
    if (c.mode == 0 && o.clip_tail != a.clip_tail) return fail("clip_tail", a.clip_tail, o.clip_tail);
    if (c.mode == 0 && o.walk_n != a.n_body) return fail("the walk's op count", a.n_body, o.walk_n);
    if (c.mode == 0 && o.walk_r != a.end_row) return fail("the walk's last row", a.end_row, o.walk_r);
    if ((o.overflow != 0) != p.overflow) return fail("overflow", p.overflow, o.overflow);
    if (o.arena_count != p.arena_count) return fail("the arena counter", p.arena_count, o.arena_count);
    if (o.ctmp_guard != kCanary) return fail("the word behind ctmp", kCanary, o.ctmp_guard);
    for (u32 k = 0; k < kSlotWords; ++k) {
      const u32 exp = k < c.stride ? p.slot[k] : kUnwritten;
      if (slots[n * kSlotWords + k] != exp) { std::printf("(slot word %u%s) ", k, k >= c.stride ? ", past stride" : ""); return fail("slot word", exp, slots[n * kSlotWords + k]); }
    }
    for (u32 k = 0; k < kArenaWords; ++k) {
      const u32 exp = p.in_arena && k >= p.arena_at && k < p.arena_at + p.n_ops ? e.cigar[k - p.arena_at] : kUnwritten;
      if (arenas[n * kArenaWords + k] != exp) { std::printf("(arena word %u%s) ", k, k >= c.arena_cap ? ", past arena_cap" : ""); return fail("arena word", exp, arenas[n * kArenaWords + k]); }
    }
    for (u32 k = 0; k <= kSeCap; ++k) {
      const u32 exp = k < p.fin.size() ? p.fin[k] : kCanary;
      if (o.fin[k] != exp) { std::printf("(fin word %u) ", k); return fail("fin word", exp, o.fin[k]); }
    }
  }
  // edit_distance and long_enough
  unsigned long long *dcount;
  HIPCHK(hipMalloc(&dcount, 3 * sizeof(unsigned long long)));
  const unsigned long long init[3] = {0, 0, ~0ull};
  HIPCHK(hipMemcpy(dcount, init, sizeof(init), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_grid, dim3(302, 201), dim3(64), 0, 0, dcount, dcount + 1, dcount + 2);
  HIPCHK(hipGetLastError());
  const std::vector<unsigned long long> grid = down(dcount, 3);
  unsigned long long sum = 0;
  for (int scr = -1; scr <= 300; ++scr)
    for (u32 len = 0; len <= 200; ++len)
      for (int ins = 0; ins <= 30; ++ins)
        for (int del = 0; del <= 30; ++del) sum += static_cast<u32>(host_nm(scr, len, ins, del)) & 0xFFFFu;
  for (u32 al = 0; al <= 200; ++al)
    for (u32 rl = 0; rl <= 200; ++rl) sum += (host_long_enough(al, rl, 0) ? 1000003ull : 0ull) + (host_long_enough(al, rl, 32) ? 1000003ull : 0ull);
  if (grid[0] != 0 || grid[1] != sum) {
    std::printf("FAIL cigar: edit_distance / long_enough differ from the host's int16_t arithmetic in %llu grid points (first %llx: score + 1 << 32 | length << 16 | 31 ins + "
                "del; top 16 bits set: long_enough, alignment length << 16 | read length), sums %llu device %llu host\n", grid[0], grid[2], grid[1], sum);
    return 1;
  }
#endif
  bool ok = fin_long && with_head && with_tail && gapped && truncated_body;
  for (int k = 0; k < kSinkKinds; ++k) ok = ok && live[k];
  std::printf("%s cigar %zu alignments, %zu sink cases:", !ok ? "FAIL coverage:" : (kDevice ? "OK" : "HOST"), bases.size(), cases.size());
  for (int k = 0; k < kSinkKinds; ++k) std::printf(" %s %d;", kSinkNames[k], live[k]);
  std::printf(" alignments of more than %u ops %d, with a head clip %d, a tail clip %d, an indel %d, of more than two ops without the clips %d; edit_distance on 302 x 201 x 31 x 31 "
              "and long_enough on 201 x 201 x 2 grid points\n", kSeCap, fin_long, with_head, with_tail, gapped, truncated_body);
  return ok ? 0 : 1;
}

// ==== choose =========================================================================================================
static int do_choose() {
  constexpr int kSetsPerLen = 300, kExtraPerLen = 60, kPerLen = kSetsPerLen + kExtraPerLen, kMaxL = 150, kSlot = 256, kRegion = 32 * kSlot;
  constexpr double kFrac = 0.1;
  const int lens[3] = {50, 100, 150};
  const int n_sets = 3 * kPerLen;
  const u32 W = words_for(kMaxL), GW = se_window_words(kMaxL, kFrac);
  (void)GW;
  G.assign(static_cast<size_t>(n_sets + 1) * kRegion, 0);
  for (auto &g : G) g = static_cast<unsigned char>(1u << (rnd() & 3));
  std::vector<SetIn> in(n_sets);
  std::vector<u64> reads(static_cast<size_t>(n_sets) * 4 * W, ~0ull);
  std::vector<std::vector<unsigned char>> q(static_cast<size_t>(n_sets) * 4);
  for (int s = 0; s < n_sets; ++s) {
    const int L = lens[s / kPerLen], idx = s % kPerLen, kind = idx < kSetsPerLen ? idx % 8 : 8 + (idx - kSetsPerLen) % 5;
    for (int e = 0; e < 4; ++e) { q[4 * s + e] = random_read(L); pack(q[4 * s + e], reads.data() + (static_cast<size_t>(s) * 4 + e) * W, W); }
    const std::vector<unsigned char> &q0 = q[4 * s];
    SetIn &si = in[s];
    std::memset(&si, 0, sizeof(si));
    si.L = static_cast<u32>(L);
    si.tb_off = static_cast<u32>(s) * 16384u;
    si.n = static_cast<u32>(kind == 3 ? rnd_in(13, 30) : (kind == 9 ? 1 : rnd_in(2, 30)));
    const int cap = static_cast<short>(0.4 * L) - 1;  // the most mismatches a job may state
    for (u32 k = 0; k < si.n; ++k) {
      const u32 pos = static_cast<u32>(s) * kRegion + kSlot / 2 + k * kSlot + static_cast<u32>(rnd_in(0, 20));
      si.pos[k] = pos;
      int extra = 0;
      if (kind == 4 || (kind == 9 && (idx & 8))) {  // nothing matches anywhere near: every score is 0
        for (int x = -70; x < L + 70; ++x) G[pos + x] = 0;
        si.d[k] = rnd_in(1, cap);
        continue;
      }
      if (kind == 1 && k == si.n / 2) plant(q0.data(), L, pos, 0, 2 * L / 3, rnd_in(0, 1) ? -1 : 1);  // wins through its gap
      else if (kind == 1) plant(q0.data(), L, pos, rnd_in(3, L / 6), 0, 0);
      else if (kind == 2 && k < 2) {  // the same copy twice; the one at the lower position states two mismatches more
        const std::vector<int> at = {L / 5, L / 2, L - 7};
        plant(q0.data(), L, pos, 3, 0, 0, &at);
        extra = k == 0 ? 2 : 0;
      }
      else if (kind == 5 && k < 3) plant(q0.data(), L, pos, 2, 0, 0);
      else if (kind == 6) plant(q0.data(), L, pos, rnd_in(1, L / 3), (rnd() % 4 == 0) ? rnd_in(L / 2, 3 * L / 4) : 0, rnd_in(0, 1) ? -rnd_in(1, 3) : rnd_in(1, 3));
      else if ((kind == 7 || kind >= 8) && k % 3 == 0) plant(q0.data(), L, pos, rnd_in(1, 2), 0, 0);
      else plant(q0.data(), L, pos, rnd_in(1, std::max(5, L / 3)), 0, 0);
      si.d[k] = std::min(std::max(1, hamming(q0.data(), L, pos)) + extra, kind == 0 ? 1000 : cap);
    }
    if (kind == 8) { si.exact_p = si.pos[si.n / 2] + 3; si.exact_f = kHostFlagARich; }                              // an exact match: nothing is aligned
    if (kind == 10) {                                                                                              // duplicate (pos, flags); the same position in another encoding
      const u32 n0 = si.n;
      for (u32 k = 0; k < 3 && si.n < kSeCap; ++k) { si.pos[si.n] = si.pos[k % n0]; si.d[si.n] = si.d[k % n0]; si.flags[si.n] = 0; ++si.n; }
      si.pos[si.n] = si.pos[0]; si.d[si.n] = 3; si.flags[si.n] = kHostFlagARich; ++si.n;
    }
    if (kind == 11) for (u32 k = 0; k < si.n; k += 3) si.d[k] = static_cast<short>(0.4 * L) + static_cast<int>(k % 2);  // the best copies state too many mismatches
    if (kind == 12) for (u32 k = 1; k < si.n; k += 2) si.pos[k] = 0;                                                // empty slots
  }
  static const char *const names[2] = {"choose_se<false, false>", "choose_se<true, false>"};
#ifndef ALIGN_HOST_ONLY
  Carve cv = {4 * W, kChooseStride + 2, kMaxJobs, GW, (kMaxL + 31u) * 31u};
  const std::vector<u64> gw = packed_genome(GW + 64);
  const u64 *dg = up(gw), *dr = up(reads);
  const SetIn *di = up(in);
  SetOut *dout;
  u8 *dtb;
  HIPCHK(hipMalloc(&dout, n_sets * sizeof(SetOut)));
  HIPCHK(hipMalloc(&dtb, static_cast<size_t>(n_sets) * 16384));
  const size_t lds = carve_bytes(cv);
  allow_lds(reinterpret_cast<const void *>(k_choose<false>), lds); allow_lds(reinterpret_cast<const void *>(k_choose<true>), lds);
#endif
  int exact = 0, lone_zero = 0, lone_hit = 0, dups = 0, invalid = 0, empty = 0, mapped = 0, ambiguous = 0, two_rounds = 0, gapped = 0, failed_hit = 0, other_enc = 0;
  for (int variant = 0; variant < 2; ++variant) {
#ifndef ALIGN_HOST_ONLY
    HIPCHK(hipMemset(dout, 0, n_sets * sizeof(SetOut)));
    if (variant == 0) hipLaunchKernelGGL(k_choose<false>, dim3(n_sets), dim3(64), lds, 0, dg, dr, di, dout, cv, W, GW, kFrac, dtb);
    else hipLaunchKernelGGL(k_choose<true>, dim3(n_sets), dim3(64), lds, 0, dg, dr, di, dout, cv, W, GW, kFrac, dtb);
    HIPCHK(hipGetLastError());
    const std::vector<SetOut> out = down(dout, n_sets);
#endif
    for (int s = 0; s < n_sets; ++s) {
      const SetIn &si = in[s];
      const int L = static_cast<int>(si.L), invalid_at = static_cast<short>(0.4 * L);
      std::vector<HostJob> jobs;
      for (u32 k = 0; k < si.n; ++k) jobs.push_back({si.pos[k], si.flags[k], si.d[k]});
      const unsigned char *const qs[4] = {q[4 * s].data(), q[4 * s + 1].data(), q[4 * s + 2].data(), q[4 * s + 3].data()};
      const Expect e = host_choose_jobs(qs, L, jobs, kFrac, 32, variant == 1, HostJob{si.exact_p, si.exact_f, 0});
#ifndef ALIGN_HOST_ONLY
      const SetOut &o = out[s];
      const u32 e_ops = e.traced ? static_cast<u32>(e.cigar.size()) : 0u;
      bool ok = o.pos == e.pos && o.flags == e.flags && o.diffs == static_cast<short>(e.diffs) && o.n_ops == e_ops && o.n_aln == e.n_aln && o.n_single == e.n_single && !o.overflow;
      size_t bad_op = 0;
      for (size_t k = 0; ok && k < e_ops; ++k) if (o.cig[k] != e.cigar[k]) { ok = false; bad_op = k; }
      if (!ok) {
        std::printf("FAIL choose %s: set %d (kind %d, L %d, %u entries): gpu pos %u flags %x NM %d ops %u alignments %u single %u, host pos %u flags %x NM %d ops %u (%s) "
                    "alignments %u single %u; first differing op %zu\n", names[variant], s, (s % kPerLen) < kSetsPerLen ? (s % kPerLen) % 8 : 8 + ((s % kPerLen) - kSetsPerLen) % 5,
                    L, si.n, o.pos, o.flags, o.diffs, o.n_ops, o.n_aln, o.n_single, e.pos, e.flags, e.diffs, e_ops, cigar_text(e.cigar).c_str(), e.n_aln, e.n_single, bad_op);
        return 1;
      }
#endif
      if (variant) continue;
      bool has_dup = false, has_other = false;
      int n_invalid = 0, n_empty = 0;
      for (u32 k = 0; k < si.n; ++k) {
        n_invalid += si.pos[k] != 0 && si.d[k] >= invalid_at; n_empty += si.pos[k] == 0; has_other |= si.flags[k] != 0;
        for (u32 m = 0; m < k; ++m) has_dup |= si.pos[k] != 0 && si.pos[m] == si.pos[k] && si.flags[m] == si.flags[k];
      }
      exact += si.exact_p != 0; lone_zero += e.n_single == 1 && e.pos == 0 && e.flags == kHostFlagAmbig && !e.traced; lone_hit += e.n_single == 1 && e.pos != 0;
      dups += has_dup; invalid += n_invalid > 0; empty += n_empty > 0; mapped += e.pos != 0; ambiguous += (e.flags & kHostFlagAmbig) != 0; two_rounds += e.n_aln > kMaxJobs;
      other_enc += has_other; failed_hit += e.traced && e.pos == 0;
      bool g = false;
      for (u32 op : e.cigar) g |= (op & 15u) == 1 || (op & 15u) == 2;
      gapped += g;
    }
  }
  const bool ok = exact && lone_zero && lone_hit && dups && invalid && empty && mapped && ambiguous && two_rounds && gapped && other_enc;
  std::printf("%s choose %d sets x 2 (%s, %s); with a hit %d, ambiguous %d, gapped %d, traced and then dropped %d, more than %u alignments %d, exact matches %d, lone jobs "
              "without a score %d, lone jobs with a hit %d, sets with duplicate entries %d, with a second encoding %d, with d >= 0.4 L %d, with empty slots %d\n",
              !ok ? "FAIL coverage:" : (kDevice ? "OK" : "HOST"), n_sets, names[0], names[1], mapped, ambiguous, gapped, failed_hit, kMaxJobs, two_rounds, exact, lone_zero,
              lone_hit, dups, other_enc, invalid, empty);
  return ok ? 0 : 1;
}

int main(int argc, char **argv) {
  const std::string step = argc > 1 ? argv[1] : "";
  if (step == "table") return do_table();
  if (step == "wrap") return do_wrap();
  if (step == "rounds") return do_rounds();
  if (step == "floor") return do_floor();
  if (step == "cigar") return do_cigar();
  if (step == "choose") return do_choose();
  std::printf("usage: align_check table|wrap|rounds|floor|cigar|choose\n");
  return 2;
}
