// GPU test program (built and run by tests/test_gpu_se_pilot.py): choose_se in the pilot order (choose_se_pilot: the
// fewest-mismatch job traced first, the others scored against a floor and dropped once beaten) against a plain host
// DP that scores EVERY job of the set to its last row, selects as align_se_candidates does (src/abismal.cpp:1435-1497)
// and traces the winner back.  Random job sets of 2-30 jobs, reads of 50, 100 and 150 bases; what must be equal:
// the hit's position (the winner, moved by its traceback), its flags (ambiguity), NM -- computed from the winning
// score, which is how the score shows in the result -- and the CIGAR.  By construction the sets contain: a winner that
// is not the fewest-mismatch job because it wins through a gap; a tie whose lower-position job is not the pilot; more
// than 12 jobs (two scoring rounds); a set whose scores are all <= 0 (0, cells being clamped there); pilots with equal mismatch counts.
// A job is (position, d): d only sets the band and picks the pilot, as in the kernel, so a set may state it freely.
// Prints "OK <n sets> ..." or the first mismatch.
#include "../../abismal_amd/csrc/abm_kernels.hip"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace abm;

constexpr int kMaxL = 150, kSlot = 256, kRegion = 32 * kSlot;  // a set's piece of the genome: 30 jobs, one per slot
constexpr int kSetsPerLen = 1000, kStride = kMaxL + 2;
constexpr double kFrac = 0.1;

struct SetIn { u32 L, n; u32 pos[30]; int d[30]; };
struct SetOut { Hit best; u32 n_ops; u32 cig[kStride]; };

__global__ __launch_bounds__(64) void run(const u64 *genome, const u64 *reads, const SetIn *in, SetOut *out, u32 W, u32 GW,
                                          u32 tb_bytes) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x;
  const SetIn &s = in[blockIdx.x];
  WaveLds lds = {};
  lds.W = W; lds.GW = GW; lds.max_jobs = kMaxJobs;
  unsigned char *p = smem;
  lds.qpk = reinterpret_cast<u64 *>(p); p += 4 * W * 8;
  lds.ctmp = reinterpret_cast<u32 *>(p); p += kStride * 4;
  lds.jpos = reinterpret_cast<u32 *>(p); p += kSeCap * 4;
  lds.jdf = reinterpret_cast<u32 *>(p); p += kSeCap * 4;
  lds.gwin = reinterpret_cast<u64 *>(p); p += GW * 8;
  lds.tb = p; p += max(tb_bytes, (kMaxJobs - 1) * GW * 8);  // (the table overlays window slots 1.. as in the kernels)
  lds.lbest = reinterpret_cast<int *>(p);
  for (u32 k = lane; k < 4 * W; k += 64) lds.qpk[k] = k < W ? reads[blockIdx.x * W + k] : ~0ull;
  wave_sync();
  DevIndex ix = {};
  ix.genome = genome;
  ix.min_len = 32;
  SeSet S;
  S.begin_read(s.L);
  S.sz = static_cast<int>(s.n);
  S.hk = lane < static_cast<int>(s.n) ? s.d[lane] * 256 + lane : 0;
  S.pp = lane < static_cast<int>(s.n) ? s.pos[lane] : 0u;
  S.pf = 0;
  Hit best;
  best.diffs = 0x7fff; best.flags = 0; best.pos = 0;
  u32 n_ops = 0, n_aln = 0, n_single = 0;
  bool overflow = false;
  const CigarSink sink = {kStride, kStride, nullptr, nullptr, 0, nullptr};
  choose_se<false, true, false>(ix, lds, s.L, kFrac, S, best, out[blockIdx.x].cig, sink, n_ops, overflow, n_aln, n_single);
  if (lane == 0) { out[blockIdx.x].best = best; out[blockIdx.x].n_ops = overflow ? 0xFFFFFFFFu : n_ops; }
}

// ---- the host's side -------------------------------------------------------------------------------------------
static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return static_cast<unsigned>(rng_state >> 16); }
static int rnd_in(int lo, int hi) { return lo + static_cast<int>(rnd() % static_cast<unsigned>(hi - lo + 1)); }

static std::vector<unsigned char> G;  // genome nibbles
static int host_band(int d, int md) { const int v = 2 * std::min(d, md) + 1; return v < 0 ? 61 : std::min(61, v); }

struct Aligned { int score; std::vector<u32> cigar; u32 pos; u32 alen; int ins, del; };
// the reference's banded local alignment of read q[0, L) at position pos with band bw: scores 2 / -3 / -4, the first
// maximum in row-major order, arrows with left before above before the diagonal
static Aligned host_align(const unsigned char *q, int L, u32 pos, int bw, bool trace) {
  const int rows = L + bw;
  const u32 t_beg = pos - static_cast<u32>((bw - 1) / 2);
  std::vector<int> C(static_cast<size_t>(rows) * bw, 0);
  std::vector<unsigned char> T(static_cast<size_t>(rows) * bw, 3);
  int best = 0, br = 0, bc = 0;
  for (int i = 1; i < rows; ++i)
    for (int j = 0; j < bw; ++j) {
      const int r = i + j - bw;
      if (r < 0 || r >= L) continue;
      const bool match = (q[r] & G[t_beg + i - 1]) != 0;
      const int sdiag = C[(i - 1) * bw + j] + (match ? 2 : -3);
      int c = std::max(sdiag, 0), arrow = c == sdiag ? 0 : 3;
      if (j < bw - 1 && r < L - 1) { const int up = C[(i - 1) * bw + j + 1] - 4; c = std::max(c, up); if (c == up) arrow = 2; }
      if (j > 0) { const int left = C[i * bw + j - 1] - 4; c = std::max(c, left); if (c == left) arrow = 1; }
      C[i * bw + j] = c;
      T[i * bw + j] = static_cast<unsigned char>(arrow | (c > 0 ? 4 : 0));
      if (c > best) { best = c; br = i; bc = j; }
    }
  Aligned a{best, {}, pos, static_cast<u32>(L), 0, 0};
  if (!trace || best == 0) { a.cigar.push_back(static_cast<u32>(L) << 4); return a; }
  int r = br, c = bc;
  const int clip_tail = (L + bw - 1) - (r + c);
  std::vector<u32> ops;
  auto emit = [&](u32 run, int op) {
    ops.push_back((run << 4) | static_cast<u32>(op));
    if (op == 1) a.ins = static_cast<short>(a.ins + static_cast<unsigned char>(run));
    if (op == 2) a.del = static_cast<short>(a.del + static_cast<unsigned char>(run));
  };
  auto step = [&](int ar) { if (ar != 1) --r; if (ar == 1) --c; if (ar == 2) ++c; };
  int op = T[r * bw + c] & 3;
  step(op);
  u32 run = 1;
  for (;;) {
    const int cell = T[r * bw + c];
    if (!(cell & 4)) break;
    const int ar = cell & 3;
    step(ar);
    if (ar != op) { emit(run, op); run = 0; }
    ++run;
    op = ar;
  }
  emit(run, op);
  const int clip_head = (r + c) - (bw - 1);
  if (clip_head > 0) a.cigar.push_back((static_cast<u32>(clip_head) << 4) | 4u);
  a.cigar.insert(a.cigar.end(), ops.rbegin(), ops.rend());
  if (clip_tail > 0) a.cigar.push_back((static_cast<u32>(clip_tail) << 4) | 4u);
  a.alen = static_cast<u32>(L - clip_tail - clip_head);
  a.pos = pos - static_cast<u32>((bw - 1) / 2) + static_cast<u32>(r);
  return a;
}
static int host_nm(int scr, u32 len, int ins, int del) {  // simple_aln::edit_distance, src/AbismalAlign.hpp:73-89
  if (scr == 0) return static_cast<short>(len);
  const int A = static_cast<short>(scr + 4 * (ins + del));
  const u32 num = 2u * (len - static_cast<u32>(ins)) - static_cast<u32>(A);
  return static_cast<short>(static_cast<short>(num / 5u) + ins + del);
}

struct Expect { u32 pos, flags; int diffs; std::vector<u32> cigar; };
static Expect host_choose(const unsigned char *q, int L, std::vector<std::pair<u32, int>> jobs /* (pos, d) */) {
  const int md = static_cast<short>(kFrac * L), invalid_at = static_cast<short>(0.4 * L), perfect = 2 * L;
  std::sort(jobs.begin(), jobs.end());
  int top = 0, b_d = 0;
  u32 top_pos = 0, b_pos = 0, b_flags = 0;
  for (const auto &j : jobs) {
    if (j.second >= invalid_at) continue;
    const int sc = host_align(q, L, j.first, host_band(j.second, md), false).score;
    if (sc > top) { top = sc; top_pos = b_pos = j.first; b_d = j.second; b_flags = 0; }
    else if (sc == top) {
      const u32 gap = j.first > top_pos ? j.first - top_pos : top_pos - j.first;
      if (sc == perfect ? j.first != top_pos : gap > 3u) b_flags |= kFlagAmbig;
    }
  }
  Expect e{0, b_flags, 0x7fff, {}};
  if (b_pos == 0) return e;
  const Aligned a = host_align(q, L, b_pos, host_band(b_d, md), true);
  const int nm = host_nm(top, a.alen, a.ins, a.del);
  e.cigar = a.cigar;
  if (a.alen >= std::max(32u, static_cast<u32>(0.6 * L)) && nm <= md) { e.diffs = nm; e.pos = a.pos; }
  return e;
}

// plants a copy of the read at pos: `subs` substitutions, and from read index `gap_at` on (if > 0) the copy lacks
// (gap < 0) or has in addition (gap > 0) |gap| bases, so that only a gapped alignment follows the read to its end
static void plant(const unsigned char *q, int L, u32 pos, int subs, int gap_at, int gap, const std::vector<int> *sub_at = nullptr) {
  std::vector<unsigned char> copy(q, q + L);
  for (int k = 0; k < subs; ++k) {
    const int at = sub_at ? (*sub_at)[k] : rnd_in(0, L - 1);
    copy[at] = static_cast<unsigned char>(1u << ((__builtin_ctz(copy[at]) + 1 + (sub_at ? 0 : static_cast<int>(rnd() % 3))) & 3));
  }
  if (gap_at > 0 && gap < 0) copy.erase(copy.begin() + gap_at, copy.begin() + gap_at - gap);
  if (gap_at > 0 && gap > 0) for (int k = 0; k < gap; ++k) copy.insert(copy.begin() + gap_at, static_cast<unsigned char>(1u << (rnd() & 3)));
  for (size_t k = 0; k < copy.size(); ++k) G[pos + k] = copy[k];
}
static int hamming(const unsigned char *q, int L, u32 pos) {
  int d = 0;
  for (int k = 0; k < L; ++k) d += (q[k] & G[pos + k]) == 0;
  return d;
}

int main() {
  const int lens[3] = {50, 100, 150};
  const int n_sets = 3 * kSetsPerLen;
  const u32 W = (kMaxL + 15) / 16, GW = se_window_words(kMaxL, kFrac);
  G.resize(static_cast<size_t>(n_sets + 1) * kRegion);
  for (auto &g : G) g = static_cast<unsigned char>(1u << (rnd() & 3));
  std::vector<SetIn> in(n_sets);
  std::vector<u64> reads(static_cast<size_t>(n_sets) * W, ~0ull);
  std::vector<std::vector<unsigned char>> q(n_sets);
  int kinds[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int s = 0; s < n_sets; ++s) {
    const int L = lens[s / kSetsPerLen], kind = s % 8;
    q[s].resize(L);
    for (auto &b : q[s]) b = static_cast<unsigned char>(1u << (rnd() & 3));
    for (int k = 0; k < L; ++k) {
      u64 &w = reads[static_cast<size_t>(s) * W + k / 16];
      w = (w & ~(15ull << (4 * (k % 16)))) | (static_cast<u64>(q[s][k]) << (4 * (k % 16)));
    }
    SetIn &si = in[s];
    si.L = static_cast<u32>(L);
    si.n = static_cast<u32>(kind == 3 ? rnd_in(13, 30) : rnd_in(2, 30));
    const int cap = static_cast<short>(0.4 * L) - 1;  // the most mismatches a job may state
    for (u32 k = 0; k < si.n; ++k) {
      const u32 pos = static_cast<u32>(s) * kRegion + kSlot / 2 + k * kSlot + static_cast<u32>(rnd_in(0, 20));
      si.pos[k] = pos;
      int extra = 0;
      if (kind == 4) {  // nothing matches anywhere near: every score is 0
        for (int x = -70; x < L + 70; ++x) G[pos + x] = 0;
        si.d[k] = rnd_in(1, cap);
        continue;
      }
      if (kind == 1 && k == si.n / 2) plant(q[s].data(), L, pos, 0, 2 * L / 3, rnd_in(0, 1) ? -1 : 1);  // wins through its gap
      else if (kind == 1) plant(q[s].data(), L, pos, rnd_in(3, L / 6), 0, 0);
      else if (kind == 2 && k < 2) {  // the same copy twice; the one at the lower position states two mismatches more
        const std::vector<int> at = {L / 5, L / 2, L - 7};
        plant(q[s].data(), L, pos, 3, 0, 0, &at);
        extra = k == 0 ? 2 : 0;
      }
      else if (kind == 5 && k < 3) plant(q[s].data(), L, pos, 2, 0, 0);  // pilots with equal mismatch counts
      else if (kind == 6) plant(q[s].data(), L, pos, rnd_in(1, L / 3), (rnd() % 4 == 0) ? rnd_in(L / 2, 3 * L / 4) : 0, rnd_in(0, 1) ? -rnd_in(1, 3) : rnd_in(1, 3));
      else if (kind == 7 && k % 3 == 0) plant(q[s].data(), L, pos, 1, 0, 0);
      else plant(q[s].data(), L, pos, rnd_in(1, std::max(5, L / 3)), 0, 0);
      si.d[k] = std::min(std::max(1, hamming(q[s].data(), L, pos)) + extra, kind == 0 ? 1000 : cap);
    }
    ++kinds[kind];
  }
  std::vector<u64> gw(G.size() / 16);
  for (size_t k = 0; k < G.size(); ++k) gw[k / 16] |= static_cast<u64>(G[k]) << (4 * (k % 16));

  const u32 bw_max = 2 * static_cast<u32>(kFrac * kMaxL) + 1, tb_bytes = ((kMaxL + bw_max) * bw_max + 15u) & ~15u;
  const size_t lds = 4 * W * 8 + kStride * 4 + 2 * kSeCap * 4 + GW * 8 + std::max<size_t>(tb_bytes, (kMaxJobs - 1) * GW * 8) + 64 * 4 + 64;
  if (lds > 64 * 1024) { printf("FAIL lds %zu\n", lds); return 1; }
  u64 *dg, *dr; SetIn *di; SetOut *dout;
  if (hipMalloc(&dg, gw.size() * 8) != hipSuccess || hipMalloc(&dr, reads.size() * 8) != hipSuccess ||
      hipMalloc(&di, in.size() * sizeof(SetIn)) != hipSuccess || hipMalloc(&dout, n_sets * sizeof(SetOut)) != hipSuccess) { printf("FAIL alloc\n"); return 1; }
  if (hipMemcpy(dg, gw.data(), gw.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dr, reads.data(), reads.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(di, in.data(), in.size() * sizeof(SetIn), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(dout, 0, n_sets * sizeof(SetOut)) != hipSuccess) { printf("FAIL copy in\n"); return 1; }
  hipLaunchKernelGGL(run, dim3(n_sets), dim3(64), lds, 0, dg, dr, di, dout, W, GW, tb_bytes);
  if (hipDeviceSynchronize() != hipSuccess) { printf("FAIL launch\n"); return 1; }
  std::vector<SetOut> out(n_sets);
  if (hipMemcpy(out.data(), dout, n_sets * sizeof(SetOut), hipMemcpyDeviceToHost) != hipSuccess) { printf("FAIL copy out\n"); return 1; }

  int gap_wins = 0, low_not_pilot = 0, two_rounds = 0, all_zero = 0, equal_pilots = 0, mapped = 0;
  for (int s = 0; s < n_sets; ++s) {
    const SetIn &si = in[s];
    const int L = static_cast<int>(si.L), invalid_at = static_cast<short>(0.4 * L);
    std::vector<std::pair<u32, int>> jobs;
    for (u32 k = 0; k < si.n; ++k) jobs.push_back({si.pos[k], si.d[k]});
    const Expect e = host_choose(q[s].data(), L, jobs);
    const SetOut &o = out[s];
    bool ok = o.best.pos == e.pos && o.best.flags == e.flags && o.best.diffs == e.diffs;
    if (ok && e.pos != 0) {
      ok = o.n_ops == e.cigar.size();
      for (size_t k = 0; ok && k < e.cigar.size(); ++k) ok = o.cig[k] == e.cigar[k];
    }
    if (!ok) {
      printf("FAIL set %d (kind %d, L %d, %u jobs): gpu pos %u flags %x diffs %d ops %u, host pos %u flags %x diffs %d ops %zu\n", s, s % 8, L,
             si.n, o.best.pos, o.best.flags, o.best.diffs, o.n_ops, e.pos, e.flags, e.diffs, e.cigar.size());
      return 1;
    }
    // what the sets were built to contain, counted from the host's side
    int n_valid = 0, dmin = 1 << 30, n_min = 0;
    u32 pilot_pos = 0;
    std::sort(jobs.begin(), jobs.end());
    for (const auto &j : jobs) if (j.second < invalid_at) { ++n_valid; if (j.second < dmin) { dmin = j.second; n_min = 1; pilot_pos = j.first; } else if (j.second == dmin) ++n_min; }
    mapped += e.pos != 0;
    two_rounds += n_valid > 13;  // (the pilot leaves the packing: more than 12 OTHER jobs)
    equal_pilots += n_min > 1;
    all_zero += n_valid >= 2 && e.pos == 0 && e.flags == kFlagAmbig && s % 8 == 4;
    bool gapped = false;
    for (u32 op : e.cigar) gapped |= (op & 15u) == 1 || (op & 15u) == 2;
    const u32 near = e.pos > pilot_pos ? e.pos - pilot_pos : pilot_pos - e.pos;
    gap_wins += e.pos != 0 && gapped && near > 64;
    low_not_pilot += e.pos != 0 && (e.flags & kFlagAmbig) && near > 64 && e.pos < pilot_pos;
  }
  if (!gap_wins || !low_not_pilot || !two_rounds || !all_zero || !equal_pilots) {
    printf("FAIL coverage: gap winners %d, ties won from below the pilot %d, sets of two rounds %d, all-zero sets %d, equal pilots %d\n",
           gap_wins, low_not_pilot, two_rounds, all_zero, equal_pilots);
    return 1;
  }
  printf("OK %d sets (%d with a hit); winners through a gap that are not the pilot %d, ties won from below the pilot %d, sets of two rounds %d, "
         "all-zero sets %d, sets with equal pilots %d\n", n_sets, mapped, gap_wins, low_not_pilot, two_rounds, all_zero, equal_pilots);
  return 0;
}
