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
#include "align_host.hpp"
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

// ---- the host's side: tests/hip/align_host.hpp (host_band, host_align, host_nm, host_choose, the genome nibbles G, plant, hamming)
using namespace align_host;

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
    const Expect e = host_choose(q[s].data(), L, jobs, kFrac);
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
