// GPU test program (built and run by tests/test_gpu_filter_stages.py): stage 3 of seed_pass (abm_seed.hpp) -- the Hamming
// filter -- routine by routine, one wave per workgroup and one case per workgroup, against the plain serial side of
// tests/hip/filter_host.hpp (a letter-by-letter count restating full_compare's rule; why the plane and record forms must
// give that count over the read's L letters on a one-hot genome without a blank in reach: that header).  Every comparison
// is exact.  The bit planes and the window records are built by the product's own kernels (launch_make_planes,
// build_window_records) with the product's sizes (16 slack blocks, copy 1 half a line on, window_record_bytes), and every
// wave's LDS is carved by se_carve over se_lds_layout.
//
//   masks     build_qmasks (all four encodings, every L 35..448: each mask bit against the nibble it came from, 1 past L,
//             blocks past the read untouched) and q_window16 (every L 35..512, every i in [0, L + 16))
//   distance  hamming_planes_pairs, hamming_planes<1 / 2 / 4> with groups of four and eight lanes, hamming_records_lane
//             <false / true>, both overloads of hamming, hamming2 -- each alone, on planted copies and on random windows
//   step      filter_step_windows<true> (groups of 2, 4, 8), filter_step_windows<false>, filter_step_records<SeSet>, driven
//             as seed_pass drives them; every field of every FilterStep, with a model of the position cache
//   replay    replay_chunk<true / false, true, SeSet> against libstdc++'s heap calls in candidate order
//   ghost     ghost_bits against a simulation of the reference's reused read buffers
//
// PLANTED COPIES.  For a read of L letters and one of its encodings the genome gets copies of the read -- each letter the
// read's nibble admits, drawn among them where it admits two -- every copy in a slot of its own with pos & 63 == s: copy
// (j, s) has a letter the read refuses at j, and one exact copy per s.  Every copy's two flanks (pos - 1 and pos + L) hold
// a letter the read's first / last letter refuses: each copy is thereby also the copy "whose change lies outside the
// window", and a window displaced by one base shows.  (In a four-letter genome without blanks no letter is refused by
// every read letter; the neighbour's refusal is what can be had.)  Expected distances come from the serial count, which on
// these copies is 1 and 0 -- the program checks that of its own fixture.  Edge lengths get every j and all 64 shifts (the
// 1024 letters that only hamming / hamming2 take, 64 words: 16 shifts, their shift being pos & 15); every other length
// 35..448 gets shifts 0, 1, 31, 32, 62, 63 and j in {0, 15, 16, 63, 64, 65, L - 1}.  Nothing is thinned: every routine
// that takes an edge length -- hamming_planes<1> and <4> and hamming / hamming2 included -- is given every one of its copies.
//
// THE CACHE MODEL'S LATITUDE.  Where two different positions are written to one slot by lanes of one half, either may stay
// (filter_host.hpp), and a later lookup of one of them is compared with a range.  `step` bounds that: lookups held to a
// hit must outnumber the open ones four to one, and the cases marked `sure` take their positions from a pool in which no
// two share a slot -- the model must then be sure of every lookup, and `cached` is one number for every lane of them.
//
// Usage: filter_check masks|distance|step|replay|ghost.  Prints "OK <step> <liveness counts ...>" or the first mismatch.
#include "../../abismal_amd/csrc/abm_kernels.hip"
#include "../../abismal_amd/csrc/abm_ext.hip"
#include "../../abismal_amd/csrc/abm_pe_set.hpp"
#include "filter_host.hpp"
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
using namespace abm;
using namespace filter_host;

#define HIPCHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("FAIL hip: %s (%s), line %d\n", hipGetErrorString(e_), #x, __LINE__); std::exit(1); } } while (0)
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
template <class T> static T *up(const std::vector<T> &v, size_t slack_bytes = 0) {
  T *d = nullptr;
  const size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T) + slack_bytes;
  HIPCHK(hipMalloc(&d, bytes));
  HIPCHK(hipMemset(d, 0, bytes));
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

// ---- a launch's argument block, shaped as the launcher shapes it ---------------------------------------------------------
constexpr double kFrac = 0.1;
static SeArgs make_args(const DevIndex &ix, u32 max_len, u32 G) {
  SeArgs a = {};
  a.ix = ix;
  a.max_len = max_len;
  a.W = std::max(1u, (max_len + 15) / 16);
  a.WB = (max_len + 63) / 64 + 1;
  a.valid_frac = a.size_frac = kFrac;
  a.GW = se_window_words(max_len, kFrac);
  a.tb_extra = tb_extra_bytes(a.GW, max_len, kFrac);
  a.ctmp_cap = max_len + 2;
  a.G = G;
  return a;
}
static size_t lds_bytes(const SeArgs &a) { return se_lds_layout<u32>(0u, false, lds_shape(a)).bytes; }
static void upload_reads(SeArgs &a, const std::vector<Read> &reads) {
  std::vector<u64> packed(reads.size() * 4 * a.W);
  std::vector<u32> lens(reads.size());
  for (size_t r = 0; r < reads.size(); ++r) { pack(reads[r], a.W, packed.data() + r * 4 * a.W); lens[r] = reads[r].L; }
  a.packed = up(packed, 64);
  a.lens = up(lens, 64);
  a.n_reads = reads.size();
}
static void free_reads(SeArgs &a) { HIPCHK(hipFree(const_cast<u64 *>(a.packed))); HIPCHK(hipFree(const_cast<u32 *>(a.lens))); }

// the wave's LDS by the product's carve, the read's four encodings staged as the mapping kernel stages them
__device__ __forceinline__ WaveLds wave_lds(unsigned char *smem, const SeArgs &a, u64 read) {
  WaveLds lds;
  se_carve<false>(lds, smem, a);
  const u64 *src = a.packed + read * 4 * a.W;
  for (u32 k = lane_id(); k < 4 * a.W; k += 64) lds.qpk[k] = src[k];
  wave_sync();
  return lds;
}

// ---- a genome on the device: nibble words, and the bit planes with nmap by the product's kernel and sizes ---------------
struct Dev {
  DevIndex ix = {};
  u64 n_bases = 0, n_blocks = 0;
  void *plane_mem[2] = {nullptr, nullptr};
};
static Dev make_dev(const std::vector<u8> &g, bool planes, bool mark_multi) {
  Dev d;
  const std::vector<u64> words = pack_genome(g);
  d.ix.genome = up(words, 64);
  d.n_bases = g.size();
  d.ix.max_candidates = 100; d.ix.window = 20; d.ix.min_len = kKeyWeight + 20 - 1;
  if (!planes) return d;
  d.n_blocks = (d.n_bases + kPlaneBlock - 1) / kPlaneBlock + 16;
  const u64 nmap_words = ((d.n_bases >> kPlaneChunkBits) + 64) / 32 + 1;
  for (int k = 0; k < 2; ++k) { HIPCHK(hipMalloc(&d.plane_mem[k], d.n_blocks * 16 + 256)); HIPCHK(hipMemset(d.plane_mem[k], 0, d.n_blocks * 16 + 256)); }
  u64 *p0 = static_cast<u64 *>(d.plane_mem[0]), *p1 = reinterpret_cast<u64 *>(static_cast<char *>(d.plane_mem[1]) + 64);
  u32 *nmap = up(std::vector<u32>(nmap_words, 0u), 64), *bad = up(std::vector<u32>(16, 0u));
  HIPCHK(launch_make_planes(d.ix.genome, words.size(), d.n_bases, d.n_blocks, p0, p1, nmap, bad, nullptr, mark_multi ? 1u : 0u));
  const u32 is_bad = down(bad, 1)[0];
  if (is_bad && !mark_multi) { std::printf("FAIL fixture: the genome has IUPAC letters and was to have none\n"); std::exit(1); }
  d.ix.planes[0] = p0; d.ix.planes[1] = p1; d.ix.nmap = nmap;
  d.ix.multibit = is_bad ? 1u : 0u;
  HIPCHK(hipFree(bad));
  return d;
}
static void free_dev(Dev &d) {
  HIPCHK(hipFree(const_cast<u64 *>(d.ix.genome)));
  for (void *m : d.plane_mem) if (m) HIPCHK(hipFree(m));
  if (d.ix.nmap) HIPCHK(hipFree(const_cast<u32 *>(d.ix.nmap)));
  d = Dev{};
}
// the window records of `blocks` blocks over the three index arrays, by the product's kernel
static void add_records(Dev &d, const std::vector<u32> idx[3], u32 blocks) {
  d.ix.index = up(idx[0], 64); d.ix.index_t = up(idx[1], 64); d.ix.index_a = up(idx[2], 64);
  const u64 n_idx[3] = {idx[0].size(), idx[1].size(), idx[2].size()}, n_entries = n_idx[0] + n_idx[1] + n_idx[2];
  u64 *wrec = nullptr;
  const size_t bytes = window_record_bytes(n_entries, blocks);
  HIPCHK(hipMalloc(&wrec, bytes));
  HIPCHK(hipMemset(wrec, 0, bytes));
  HIPCHK(build_window_records(d.ix, d.n_blocks, d.n_bases, n_idx, blocks, wrec, nullptr));
  HIPCHK(hipDeviceSynchronize());
  d.ix.wrec = wrec;
  d.ix.wrec_t0 = static_cast<u32>(n_idx[0]); d.ix.wrec_a0 = static_cast<u32>(n_idx[0] + n_idx[1]);
  d.ix.wrec_blocks = blocks;
  d.ix.wrec_max_len = window_record_max_len(blocks);
  d.ix.wrec_back = d.ix.wrec_max_len - kKeyWeight;
}
static void free_records(Dev &d) {
  HIPCHK(hipFree(const_cast<u64 *>(d.ix.wrec))); HIPCHK(hipFree(const_cast<u32 *>(d.ix.index)));
  HIPCHK(hipFree(const_cast<u32 *>(d.ix.index_t))); HIPCHK(hipFree(const_cast<u32 *>(d.ix.index_a)));
  d.ix.wrec = nullptr;
}

static void grow_random(std::vector<u8> &g, size_t n, Rng &rng) {
  size_t at = g.size();
  g.resize(at + n);
  while (at < g.size()) {
    rng.next();
    u64 x = rng.s;
    for (int k = 0; k < 24 && at < g.size(); ++k, x >>= 2) g[at++] = static_cast<u8>(1u << (x & 3));
  }
}
static u8 admitted_letter(Rng &rng, u8 q) {  // a one-hot nibble that shares a bit with q (q != 0)
  for (;;) { const u8 n = static_cast<u8>(1u << rng.below(4)); if (n & q) return n; }
}
static u8 refused_letter(Rng &rng, u8 q) {  // a one-hot nibble that shares none (q has at most two bits)
  for (;;) { const u8 n = static_cast<u8>(1u << rng.below(4)); if (!(n & q)) return n; }
}

// =================================================================================================================
// masks
// =================================================================================================================
constexpr u32 kWinSlots = 528;
constexpr u64 kMaskCanary = 0xC0FFEE11C0FFEE11ull;
__global__ __launch_bounds__(64) void k_masks(SeArgs a, int do_masks, u64 *masks_out, u64 *win_out) {
  extern __shared__ __align__(16) unsigned char smem[];
  const u64 r = blockIdx.x;
  const u32 L = a.lens[r], lane = lane_id();
  WaveLds lds = wave_lds(smem, a, r);
  if (do_masks) {
    for (u32 k = lane; k < 16 * lds.MB; k += 64) lds.qmask[k] = kMaskCanary;
    wave_sync();
    build_qmasks(lds, L);
    wave_sync();
    for (u32 k = lane; k < 16 * lds.MB; k += 64) masks_out[r * 16 * lds.MB + k] = lds.qmask[k];
  }
  for (u32 e = 0; e < 4; ++e)
    for (u32 i = lane; i < L + 16; i += 64) win_out[(r * 4 + e) * kWinSlots + i] = q_window16(lds.qpk + e * a.W, a.W, i, L);
}

static int cmd_masks() {
  const double t0 = now_s();
  Rng rng(11);
  long nibble_seen[16] = {0}, past_end = 0, mask_bits = 0, windows = 0, untouched = 0;
  for (int part = 0; part < 2; ++part) {
    const u32 lo = part == 0 ? 35u : 449u, hi = part == 0 ? 448u : 512u, max_len = hi;
    std::vector<Read> reads;
    for (u32 L = lo; L <= hi; ++L) for (int k = 0; k < 2; ++k) reads.push_back(encode(random_letters(rng, L, true)));
    SeArgs a = make_args(DevIndex{}, max_len, 0);
    upload_reads(a, reads);
    const u32 MB = lds_mask_blocks(max_len);
    u64 *d_masks = up(std::vector<u64>(reads.size() * 16 * MB, 0)), *d_win = up(std::vector<u64>(reads.size() * 4 * kWinSlots, 0));
    allow_lds(reinterpret_cast<const void *>(k_masks), lds_bytes(a));
    hipLaunchKernelGGL(k_masks, dim3(static_cast<u32>(reads.size())), dim3(64), lds_bytes(a), 0, a, part == 0 ? 1 : 0, d_masks, d_win);
    HIPCHK(hipGetLastError());
    const std::vector<u64> masks = down(d_masks, reads.size() * 16 * MB), win = down(d_win, reads.size() * 4 * kWinSlots);
    for (size_t r = 0; r < reads.size(); ++r) {
      const Read &rd = reads[r];
      const u32 L = rd.L, nblk = (L + 63) / 64;
      for (u32 e = 0; e < 4; ++e) {
        if (part == 0)
          for (u32 s = 0; s < MB; ++s)
            for (u32 c = 0; c < 4; ++c) {
              const u64 got = masks[r * 16 * MB + (e * MB + s) * 4 + c];
              if (s >= nblk) {
                if (got != kMaskCanary) { std::printf("FAIL masks: L %u, encoding %u: block %u, beyond the read's %u, was written (code %u: %016llx)\n", L, e, s, nblk, c, (unsigned long long)got); return 1; }
                ++untouched;
                continue;
              }
              for (u32 j = 0; j < 64; ++j) {
                const u32 i = 64 * s + j, nib = i < L ? rd.nib[e][i] : 15u, want = (nib >> c) & 1u, bit = static_cast<u32>(got >> j) & 1u;
                if (bit != want) { std::printf("FAIL masks: L %u, encoding %u, block %u, code %u, base %u (nibble %u): mask bit %u, expected %u\n", L, e, s, c, i, nib, bit, want); return 1; }
                ++mask_bits; past_end += i >= L;
                if (i < L && c == 0) ++nibble_seen[nib];
              }
            }
        for (u32 i = 0; i < L + 16; ++i) {
          u64 want = 0;
          for (u32 k = 0; k < 16; ++k) want |= static_cast<u64>(i + k < L ? rd.nib[e][i + k] : 0u) << (4 * k);
          const u64 got = win[(r * 4 + e) * kWinSlots + i];
          if (got != want) { std::printf("FAIL masks: q_window16, L %u, encoding %u, i %u: %016llx, expected %016llx\n", L, e, i, (unsigned long long)got, (unsigned long long)want); return 1; }
          ++windows;
        }
      }
    }
    free_reads(a); HIPCHK(hipFree(d_masks)); HIPCHK(hipFree(d_win));
  }
  for (u32 n : {0u, 1u, 2u, 4u, 5u, 8u, 10u}) if (!nibble_seen[n]) { std::printf("FAIL masks coverage: no read nibble %u\n", n); return 1; }
  if (!past_end || !untouched) { std::printf("FAIL masks coverage: bits past the end %ld, blocks past the read %ld\n", past_end, untouched); return 1; }
  std::printf("OK masks mask_bits=%ld past_end_bits=%ld untouched_words=%ld windows=%ld nibbles 0/1/2/4/5/8/10=%ld/%ld/%ld/%ld/%ld/%ld/%ld; %.2f s\n", mask_bits, past_end, untouched, windows,
              nibble_seen[0], nibble_seen[1], nibble_seen[2], nibble_seen[4], nibble_seen[5], nibble_seen[8], nibble_seen[10], now_s() - t0);
  return 0;
}

// =================================================================================================================
// distance
// =================================================================================================================
enum { kPairs, kPlanes1, kPlanes2, kPlanes4, kRecNarrow, kRecWide, kHam, kHam2, kRoutines };
static const char *kRoutineName[kRoutines] = {"hamming_planes_pairs", "hamming_planes<1>", "hamming_planes<2>", "hamming_planes<4>", "hamming_records_lane<false>",
                                              "hamming_records_lane<true>", "hamming", "hamming2"};
struct DCase { u32 routine, L, read, enc, G, two; };

__global__ __launch_bounds__(64) void k_distance(SeArgs a, const DCase *cs, const u32 *pos, const u32 *rec, const u32 *xs, const u8 *want, int *out) {
  extern __shared__ __align__(16) unsigned char smem[];
  const DCase c = cs[blockIdx.x];
  const u32 lane = lane_id(), routine = static_cast<u32>(uni(static_cast<int>(c.routine))), L = static_cast<u32>(uni(static_cast<int>(c.L)));
  WaveLds lds = wave_lds(smem, a, c.read);
  lds.G = static_cast<u32>(uni(static_cast<int>(c.G)));
  if (routine < kHam) { build_qmasks(lds, L); wave_sync(); }
  const u64 *qm = lds.qmask + c.enc * lds.MB * 4, *qpk = lds.qpk + c.enc * a.W;
  const size_t base = static_cast<size_t>(blockIdx.x) * 128;
  const u32 pa = pos[base + lane], pb = pos[base + 64 + lane];
  const bool wa = want[base + lane] != 0, wb = want[base + 64 + lane] != 0;
  const u32 nwords = (L + 15) >> 4;
  int da = -1, db = -1, ma = -1, mb = -1, ea = -1, eb = -1;
  if (routine == kPairs) hamming_planes_pairs(a.ix, lds, qm, L, pa, wa, pb, wb, da, db);
  else if (routine == kPlanes1) hamming_planes<1>(a.ix, lds, qm, L, pa, wa, pb, wb, da, db);
  else if (routine == kPlanes2) hamming_planes<2>(a.ix, lds, qm, L, pa, wa, pb, wb, da, db);
  else if (routine == kPlanes4) hamming_planes<4>(a.ix, lds, qm, L, pa, wa, pb, wb, da, db);
  else if (routine == kRecNarrow) hamming_records_lane<false>(a.ix, qm, L, rec[base + lane], xs[base + lane], wa, rec[base + 64 + lane], xs[base + 64 + lane], wb, c.two != 0, da, db);
  else if (routine == kRecWide) hamming_records_lane<true>(a.ix, qm, L, rec[base + lane], xs[base + lane], wa, rec[base + 64 + lane], xs[base + 64 + lane], wb, c.two != 0, da, db);
  else if (routine == kHam) {
    if (wa) { da = hamming(a.ix.genome, qpk, nwords, pa, ma); ea = hamming(a.ix.genome, qpk, nwords, pa); }
    if (wb) { db = hamming(a.ix.genome, qpk, nwords, pb, mb); eb = hamming(a.ix.genome, qpk, nwords, pb); }
  }
  else hamming2(a.ix.genome, qpk, nwords, pa, wa, pb, wb, da, ma, db, mb);
  int *o = out + base * 3;
  o[lane * 3] = da; o[lane * 3 + 1] = ma; o[lane * 3 + 2] = ea;
  o[(64 + lane) * 3] = db; o[(64 + lane) * 3 + 1] = mb; o[(64 + lane) * 3 + 2] = eb;
}

struct Copy { u32 pos; int j; };
struct PlantSet { Read read; u32 enc = 0; std::vector<Copy> copies; };
struct Cand { u32 pos, i; int j; };  // i: the seed offset (records), j: the planted change (-1 exact, -2 a random window)
struct DLaunch {
  u32 max_len = 0, blocks = 0;  // blocks: records of that many blocks (0: none)
  bool iupac = false;           // the nibble genome with blanks and IUPAC letters (hamming, hamming2)
  std::vector<Read> reads;
  std::vector<DCase> cases;
  std::vector<u32> pos, rec, xs, entries;
  std::vector<u8> want;
  std::vector<int> planted;     // per slot: Cand::j
};
struct DLive { long compared = 0, copy1 = 0, skipped = 0, last_block = 0, dmax_gt = 0, last_record = 0, one_half = 0, not_wanted = 0, cases = 0, exact = 0, one_off = 0; };

static std::vector<u8> Gn, Gi;  // the one-hot genome; the small one with blanks and IUPAC letters
static Rng g_rng(2024);
static std::map<u32, PlantSet> g_plants;

static PlantSet &plant_for(u32 L, bool edge, u32 n_shifts = 64) {
  auto it = g_plants.find(L);
  if (it != g_plants.end()) return it->second;
  PlantSet &ps = g_plants[L];
  ps.read = encode(random_letters(g_rng, L, false));
  ps.enc = static_cast<u32>(g_plants.size() - 1) % 4;
  const std::vector<u8> &q = ps.read.nib[ps.enc];
  std::vector<int> js;
  std::vector<u32> shifts;
  if (edge) { for (u32 j = 0; j < L; ++j) js.push_back(static_cast<int>(j)); for (u32 s = 0; s < n_shifts; ++s) shifts.push_back(s); }
  else {
    for (u32 j : {0u, 15u, 16u, 63u, 64u, 65u, L - 1}) if (j < L && std::find(js.begin(), js.end(), static_cast<int>(j)) == js.end()) js.push_back(static_cast<int>(j));
    shifts = {0, 1, 31, 32, 62, 63};
  }
  js.push_back(-1);
  const u32 slot = (L + 66 + 63) & ~63u;
  for (int j : js)
    for (u32 s : shifts) {
      const size_t base = Gn.size();  // (a multiple of 64)
      grow_random(Gn, slot, g_rng);
      const u32 pos = static_cast<u32>(base) + s;
      for (u32 k = 0; k < L; ++k) Gn[pos + k] = admitted_letter(g_rng, q[k]);
      if (j >= 0) Gn[pos + j] = refused_letter(g_rng, q[j]);
      Gn[pos - 1] = refused_letter(g_rng, q[0]);
      Gn[pos + L] = refused_letter(g_rng, q[L - 1]);
      ps.copies.push_back({pos, j});
    }
  return ps;
}

static const u32 kWantSingles[10] = {0, 15, 16, 31, 32, 63, 64, 95, 96, 127};
// the 14 patterns besides "all wanted": none, ten single slots, a half only, b half only, sparse
static void want_pattern(int p, Rng &rng, u8 w[128]) {
  for (int k = 0; k < 128; ++k) w[k] = 0;
  if (p == 0) return;
  if (p <= 10) { w[kWantSingles[p - 1]] = 1; return; }
  if (p == 11) { for (int k = 0; k < 64; ++k) w[k] = 1; return; }
  if (p == 12) { for (int k = 64; k < 128; ++k) w[k] = 1; return; }
  for (int k = 0; k < 128; ++k) w[k] = rng.below(9) == 0;
}

// One routine over a list of candidates: the 14 patterns on the list's first 128 (slots not wanted hold OTHER candidates of
// the list, so that whatever they fetch is real and differs), then the whole list all wanted, 128 a case, the last case
// filled up with candidates seen before (positions repeated within one step).
static void add_cases(DLaunch &ln, u32 routine, u32 G, u32 L, u32 read, u32 enc, const std::vector<Cand> &cands, bool patterns) {
  const u32 back = ln.blocks ? window_record_max_len(ln.blocks) - kKeyWeight : 0u;
  std::map<std::pair<u32, u32>, u32> entry_of;
  auto put = [&](const Cand &c, bool wanted) {
    ln.pos.push_back(c.pos); ln.want.push_back(wanted); ln.planted.push_back(c.j);
    if (ln.blocks) {
      auto key = std::make_pair(c.pos, c.i);
      auto it = entry_of.find(key);
      if (it == entry_of.end()) { it = entry_of.emplace(key, static_cast<u32>(ln.entries.size())).first; ln.entries.push_back(c.pos + c.i); }
      ln.rec.push_back(it->second * ln.blocks); ln.xs.push_back(back - c.i);
    }
    else { ln.rec.push_back(0); ln.xs.push_back(0); }
  };
  const size_t n = cands.size();
  if (patterns)
    for (int p = 0; p < 14; ++p) {
      u8 w[128];
      want_pattern(p, g_rng, w);
      bool any_b = false;
      for (int k = 64; k < 128; ++k) any_b |= w[k] != 0;
      // (the record routines' `two`: false where no b slot is wanted -- d_b must then read 0x7fff)
      ln.cases.push_back({routine, L, read, enc, G, (routine == kRecNarrow || routine == kRecWide) ? (any_b ? 1u : 0u) : 1u});
      for (u32 k = 0; k < 128; ++k) put(w[k] ? cands[k % n] : cands[(k * 7 + 13 + g_rng.below(static_cast<u32>(n))) % n], w[k] != 0);
    }
  for (size_t at = 0; at < n; at += 128) {
    ln.cases.push_back({routine, L, read, enc, G, 1u});
    for (u32 k = 0; k < 128; ++k) put(at + k < n ? cands[at + k] : cands[at + k % (n - at)], true);
  }
}

static std::vector<Cand> cands_of(const PlantSet &ps, bool records) {
  std::vector<Cand> v;
  const u32 L = ps.read.L, n_off = L - kKeyWeight + 1;
  if (!records) { for (const Copy &c : ps.copies) v.push_back({c.pos, 0, c.j}); return v; }
  // records: the shift a lane sees is that of x = wrec_back - i, so every changed letter j meets every seed offset i the
  // read has; the copy it is taken from is the one at shift i (of the shifts the set has)
  std::map<int, std::vector<u32>> by_j;
  for (const Copy &c : ps.copies) by_j[c.j].push_back(c.pos);
  for (auto &kv : by_j)
    for (u32 i = 0; i < n_off; ++i) v.push_back({kv.second[i % kv.second.size()], i, kv.first});
  return v;
}
// random windows of the one-hot genome: anywhere, in its first block, in its last blocks, on every block number mod 8
static std::vector<Cand> random_cands(const std::vector<u8> &g, u32 L, u32 reach, u32 n, bool records) {
  std::vector<Cand> v;
  const u32 n_off = L - kKeyWeight + 1, last = static_cast<u32>(g.size()) - reach;
  for (u32 k = 0; k < n; ++k) {
    u32 pos;
    if (k % 8 == 0) pos = g_rng.below(64);
    else if (k % 8 == 1) pos = last - g_rng.below(130);
    else if (k % 8 == 2) pos = last;
    else if (k % 8 == 3) pos = 64 * (8 * g_rng.below(last / 512 - 1) + k % 64 / 8) + g_rng.below(64);
    else pos = g_rng.below(last);
    if (pos == 0) pos = 1;
    v.push_back({pos, records ? g_rng.below(n_off) : 0u, -2});
  }
  return v;
}

static int check_launch(const Dev &dev, DLaunch &ln, const std::vector<u8> &g, DLive &live) {
  Dev d = dev;
  if (ln.blocks) {
    const std::vector<u32> idx[3] = {ln.entries, {}, {}};
    add_records(d, idx, ln.blocks);
  }
  SeArgs a = make_args(d.ix, ln.max_len, 0);
  upload_reads(a, ln.reads);
  const size_t n = ln.cases.size();
  DCase *d_cases = up(ln.cases);
  u32 *d_pos = up(ln.pos), *d_rec = up(ln.rec), *d_xs = up(ln.xs);
  u8 *d_want = up(ln.want);
  int *d_out = up(std::vector<int>(n * 128 * 3, -7));
  allow_lds(reinterpret_cast<const void *>(k_distance), lds_bytes(a));
  hipLaunchKernelGGL(k_distance, dim3(static_cast<u32>(n)), dim3(64), lds_bytes(a), 0, a, d_cases, d_pos, d_rec, d_xs, d_want, d_out);
  HIPCHK(hipGetLastError());
  const std::vector<int> out = down(d_out, n * 128 * 3);
  const u32 last_entry = ln.entries.empty() ? 0u : static_cast<u32>(ln.entries.size() - 1);
  for (size_t c = 0; c < n; ++c) {
    const DCase &cs = ln.cases[c];
    const std::vector<u8> &q = ln.reads[cs.read].nib[cs.enc];
    const bool plane = cs.routine <= kPlanes4, record = cs.routine == kRecNarrow || cs.routine == kRecWide;
    ++live.cases;
    u64 w[2] = {0, 0};
    for (u32 k = 0; k < 128; ++k) if (ln.want[c * 128 + k]) w[k >> 6] |= 1ull << (k & 63);
    if ((w[0] == 0) != (w[1] == 0)) ++live.one_half;
    if (plane) {  // passes none of whose slots is wanted: 32 slots a pass for the pairs, rounds * 64 / G otherwise
      const u32 per = cs.routine == kPairs ? 32u : (cs.routine == kPlanes1 ? 1u : (cs.routine == kPlanes2 ? 2u : 4u)) * 64u / cs.G;
      for (u32 s0 = 0; s0 < 128; s0 += per) {
        const u64 m = per >= 64 ? ~0ull : ((1ull << per) - 1) << (s0 & 63);
        if ((w[s0 >> 6] & m) == 0) ++live.skipped;
      }
    }
    for (u32 k = 0; k < 128; ++k) {
      const size_t at = c * 128 + k;
      const int d0 = out[at * 3], d1 = out[at * 3 + 1], d2 = out[at * 3 + 2];
      if (!ln.want[at]) {
        ++live.not_wanted;
        if (record && k >= 64 && !cs.two && d0 != 0x7fff) { std::printf("FAIL distance: %s, case %zu, L %u: two == false and d_b of lane %u is %d, not 0x7fff\n", kRoutineName[cs.routine], c, cs.L, k - 64, d0); return 1; }
        continue;
      }
      const u32 pos = ln.pos[at];
      int want_d, want_m = -1;
      if (cs.routine >= kHam) { const Dist sd = serial_distance(g, q, pos, words_of(cs.L)); want_d = sd.d; want_m = sd.dmax; live.dmax_gt += sd.dmax > sd.d; }
      else want_d = letter_count(g, q, pos);
      if (!ln.iupac && ln.planted[at] >= -1) {  // the fixture's own promise: 1 for copy (j, s), 0 for an exact one
        const int promised = ln.planted[at] >= 0 ? 1 : 0;
        if (want_d != promised && !(cs.routine >= kHam && pos + 16 * words_of(cs.L) > g.size())) { std::printf("FAIL fixture: the copy at %u (change at %d) of the read of %u letters counts %d\n", pos, ln.planted[at], cs.L, want_d); return 1; }
        live.exact += promised == 0; live.one_off += promised == 1;
      }
      bool bad = d0 != want_d;
      if (cs.routine == kHam) bad |= d1 != want_m || d2 != want_d;
      if (cs.routine == kHam2) bad |= d1 != want_m;
      if (bad) {
        std::printf("FAIL distance: %s, case %zu, L %u, G %u, encoding %u, slot %u (lane %u, %c half), pos %u (shift %u, block %u), planted change at %d", kRoutineName[cs.routine], c, cs.L, cs.G, cs.enc,
                    k, k & 63, k < 64 ? 'a' : 'b', pos, pos & 63, pos / 64, ln.planted[at]);
        if (record) std::printf(", record %u, x %u", ln.rec[at] / ln.blocks, ln.xs[at]);
        std::printf(": expected d %d", want_d);
        if (cs.routine >= kHam) std::printf(" dmax %d", want_m);
        std::printf(", got d %d", d0);
        if (cs.routine >= kHam) std::printf(" dmax %d", d1);
        if (cs.routine == kHam) std::printf(" (four-argument overload: %d)", d2);
        std::printf("; want a %016llx b %016llx\n", (unsigned long long)w[0], (unsigned long long)w[1]);
        return 1;
      }
      ++live.compared;
      if (plane) {
        const u32 b0 = pos / 64, b1 = cs.routine == kPairs ? b0 + 2 : (cs.G == 4 ? b0 + 3 : (pos + cs.L - 1) / 64);
        live.copy1 += b0 / 8 != b1 / 8;
      }
      live.last_block += pos + cs.L > g.size() - 64;
      if (record && ln.rec[at] / ln.blocks == last_entry) ++live.last_record;
    }
  }
  HIPCHK(hipFree(d_cases)); HIPCHK(hipFree(d_pos)); HIPCHK(hipFree(d_rec)); HIPCHK(hipFree(d_xs)); HIPCHK(hipFree(d_want)); HIPCHK(hipFree(d_out));
  free_reads(a);
  if (ln.blocks) free_records(d);
  return 0;
}

static int cmd_distance() {
  const double t0 = now_s();
  grow_random(Gn, 128, g_rng);
  const std::set<u32> pair_edges = {35, 63, 64, 65, 100, 127, 128}, g4_edges = {35, 64, 65, 128, 129, 150, 191, 192},
                      g8_edges = {193, 256, 257, 320, 384, 385, 447, 448}, rec_edges = {35, 64, 65, 100, 108, 109, 128, 129, 140, 141, 172}, ham_only = {233};
  const std::map<u32, u32> ham_len = {{3, 35}, {7, 100}, {8, 128}, {9, 129}, {15, 233}, {16, 256}, {17, 257}, {28, 448}, {64, 1024}};
  std::set<u32> edges;
  for (const auto *s : {&pair_edges, &g4_edges, &g8_edges, &rec_edges, &ham_only}) edges.insert(s->begin(), s->end());
  // launches: one per LDS shape
  DLaunch pairs, g4, g8, rec3, rec4, rec5, ham, ham_iupac;
  pairs.max_len = 128; g4.max_len = 192; g8.max_len = 448; ham.max_len = 1024; ham_iupac.max_len = 1024; ham_iupac.iupac = true;
  rec3.blocks = 3; rec4.blocks = 4; rec5.blocks = 5;
  for (DLaunch *r : {&rec3, &rec4, &rec5}) r->max_len = window_record_max_len(r->blocks);
  if (rec3.max_len != 108 || rec4.max_len != 140 || rec5.max_len != 172) { std::printf("FAIL fixture: records of 3 / 4 / 5 blocks serve %u / %u / %u bases\n", rec3.max_len, rec4.max_len, rec5.max_len); return 1; }
  auto read_in = [](DLaunch &ln, const Read &r) { ln.reads.push_back(r); return static_cast<u32>(ln.reads.size() - 1); };
  // planted copies
  for (u32 L = 35; L <= 448; ++L) {
    const bool edge = edges.count(L) != 0;
    PlantSet &ps = plant_for(L, edge);
    const std::vector<Cand> cp = cands_of(ps, false);
    if (L <= 128) add_cases(pairs, kPairs, 2, L, read_in(pairs, ps.read), ps.enc, cp, pair_edges.count(L) != 0);
    if (L <= 192) {
      const u32 r = read_in(g4, ps.read);
      const bool e = g4_edges.count(L) != 0;
      add_cases(g4, kPlanes2, 4, L, r, ps.enc, cp, e);
      if (e || L % 16 == 5) { add_cases(g4, kPlanes1, 4, L, r, ps.enc, cp, e); add_cases(g4, kPlanes4, 4, L, r, ps.enc, cp, e); }
    }
    else {
      const u32 r = read_in(g8, ps.read);
      const bool e = g8_edges.count(L) != 0;
      add_cases(g8, kPlanes2, 8, L, r, ps.enc, cp, e);
      if (e || L % 16 == 5) { add_cases(g8, kPlanes1, 8, L, r, ps.enc, cp, e); add_cases(g8, kPlanes4, 8, L, r, ps.enc, cp, e); }
    }
    if (L <= 172) {
      DLaunch &rl = L <= 108 ? rec3 : (L <= 140 ? rec4 : rec5);
      add_cases(rl, L <= 108 ? kRecNarrow : kRecWide, L <= 108 ? 2 : 4, L, read_in(rl, ps.read), ps.enc, cands_of(ps, true), rec_edges.count(L) != 0);
    }
  }
  for (const auto &kv : ham_len) {
    const u32 L = kv.second;
    if ((L + 15) / 16 != kv.first) { std::printf("FAIL fixture: %u letters are not %u words\n", L, kv.first); return 1; }
    PlantSet &ps = plant_for(L, true, 16);
    const std::vector<Cand> cp = cands_of(ps, false);
    const u32 r = read_in(ham, ps.read);
    add_cases(ham, kHam, 0, L, r, ps.enc, cp, false);
    add_cases(ham, kHam2, 0, L, r, ps.enc, cp, true);
  }
  grow_random(Gn, 1024, g_rng);  // (the genome's last blocks: random letters, whole windows of every length)
  // random windows against random reads (N among their letters), every encoding
  for (u32 L : {35u, 36u, 63u, 64u, 65u, 100u, 127u, 128u, 129u, 150u, 172u, 191u, 192u, 193u, 256u, 257u, 320u, 384u, 385u, 447u, 448u})
    for (u32 enc = 0; enc < 4; ++enc) {
      const Read rd = encode(random_letters(g_rng, L, true));
      const std::vector<Cand> rc = random_cands(Gn, L, L, 256, false);
      if (L <= 128) add_cases(pairs, kPairs, 2, L, read_in(pairs, rd), enc, rc, false);
      if (L <= 192) { const u32 r = read_in(g4, rd); for (u32 rt : {kPlanes1, kPlanes2, kPlanes4}) add_cases(g4, rt, 4, L, r, enc, rc, false); }
      else { const u32 r = read_in(g8, rd); for (u32 rt : {kPlanes1, kPlanes2, kPlanes4}) add_cases(g8, rt, 8, L, r, enc, rc, false); }
      if (L <= 172) {
        DLaunch &rl = L <= 108 ? rec3 : (L <= 140 ? rec4 : rec5);
        add_cases(rl, L <= 108 ? kRecNarrow : kRecWide, L <= 108 ? 2 : 4, L, read_in(rl, rd), enc, random_cands(Gn, L, L, 256, true), false);
      }
    }
  for (const auto &kv : ham_len)
    for (u32 enc = 0; enc < 4; ++enc) {
      const u32 L = 16 * kv.first - (kv.first == 3 ? enc * 4 : enc * 5);  // (48, 44, 40, 36 letters in three words; 16 n - 0, 5, 10, 15 otherwise)
      const Read rd = encode(random_letters(g_rng, L, true));
      const u32 r = read_in(ham, rd);
      const std::vector<Cand> rc = random_cands(Gn, L, L, 256, false);  // (a window's last word may reach past the genome's end: zero nibbles there, for both sides)
      add_cases(ham, kHam, 0, L, r, enc, rc, false);
      add_cases(ham, kHam2, 0, L, r, enc, rc, false);
    }
  // the nibble genome with blanks and IUPAC letters: random nibbles of every kind, and copies of the reads in which every
  // letter matches and most carry extra bits -- a T (or an A-rich A) read letter then shares two bits, a word's share
  // goes negative, and with a few refused letters in the copy's first word the running sum peaks above its end: dmax > d
  {
    Rng rng(77);
    Gi.resize(1 << 19);
    for (auto &n : Gi) { const u32 x = rng.below(16); n = static_cast<u8>(x < 10 ? 1u << (x & 3) : (x < 12 ? 0u : 1u + rng.below(15))); }
    u32 at = 2048;
    for (const auto &kv : ham_len)
      for (u32 enc = 0; enc < 4; ++enc) {
        const u32 L = 16 * kv.first - (enc * 3 + 1);
        const Read rd = encode(random_letters(rng, L, true));
        const std::vector<u8> &q = rd.nib[enc];
        std::vector<Cand> cs;
        for (u32 copy = 0; copy < 16; ++copy) {
          const u32 pos = at + copy;  // (every pos & 15 over the 16 copies)
          for (u32 k = 0; k < L + 16; ++k) Gi[pos + k] = static_cast<u8>((k < L ? q[k] : 0u) | (rng.below(3) ? 1u + rng.below(15) : 0u));
          for (u32 k = 0; k < copy % 5; ++k) { const u32 j = rng.below(16); if (q[j] && q[j] != 15) Gi[pos + j] = refused_letter(rng, q[j]); }
          cs.push_back({pos, 0, -2});
          at += ((L + 47) & ~15u);
        }
        for (const Cand &c : random_cands(Gi, L, L + 16, 112, false)) cs.push_back(c);
        if (at + 2048 > Gi.size()) { std::printf("FAIL fixture: the IUPAC genome is full\n"); return 1; }
        const u32 r = read_in(ham_iupac, rd);
        add_cases(ham_iupac, kHam, 0, L, r, enc, cs, false);
        add_cases(ham_iupac, kHam2, 0, L, r, enc, cs, enc == 0);
      }
  }
  const double t1 = now_s();
  Dev dev = make_dev(Gn, true, false), dev_i = make_dev(Gi, false, false);
  DLive live[kRoutines];
  DLive total;
  for (DLaunch *ln : {&pairs, &g4, &g8, &rec3, &rec4, &rec5, &ham, &ham_iupac}) {
    DLive l;
    if (check_launch(ln->iupac ? dev_i : dev, *ln, ln->iupac ? Gi : Gn, l)) return 1;
    total.compared += l.compared; total.copy1 += l.copy1; total.skipped += l.skipped; total.last_block += l.last_block; total.dmax_gt += l.dmax_gt;
    total.last_record += l.last_record; total.one_half += l.one_half; total.not_wanted += l.not_wanted; total.cases += l.cases; total.exact += l.exact; total.one_off += l.one_off;
    // per launch: what that launch is there for
    const bool plane = ln == &pairs || ln == &g4 || ln == &g8, rec = ln->blocks != 0;
    if (!l.compared || !l.not_wanted || !l.one_half || !l.last_block || (plane && (!l.copy1 || !l.skipped)) || (rec && !l.last_record) || (ln->iupac && !l.dmax_gt) || (!ln->iupac && (!l.exact || !l.one_off))) {
      std::printf("FAIL distance coverage (launch for reads up to %u, records of %u blocks): compared %ld, not wanted %ld, one half only %ld, last block %ld, copy 1 %ld, passes skipped %ld, last record %ld, dmax > d %ld, exact copies %ld, one-off copies %ld\n",
                  ln->max_len, ln->blocks, l.compared, l.not_wanted, l.one_half, l.last_block, l.copy1, l.skipped, l.last_record, l.dmax_gt, l.exact, l.one_off);
      return 1;
    }
  }
  free_dev(dev); free_dev(dev_i);
  std::printf("OK distance cases=%ld compared=%ld copy1_windows=%ld passes_skipped=%ld last_block_windows=%ld dmax_gt_d=%ld last_record=%ld one_half_cases=%ld slots_not_wanted=%ld exact_copies=%ld one_off_copies=%ld; genome %zu bases; host build %.2f s, device and comparison %.2f s\n",
              total.cases, total.compared, total.copy1, total.skipped, total.last_block, total.dmax_gt, total.last_record, total.one_half, total.not_wanted, total.exact, total.one_off, Gn.size(), t1 - t0, now_s() - t1);
  return 0;
}

// =================================================================================================================
// step
// =================================================================================================================
struct SCase { u32 L, read, enc, mode, G, cutoff, n_blocks, block_off; };  // mode 0: planes, 1: nibble array, 2: records
struct SBlock { u32 g0, clear, seg_off, step_off; };
struct SegIn { u32 na, lo2, nb, lo3; };
struct StepOut { u32 va, vb, pa, pb; int ha, hma, hb, hmb; u32 seen, cached, total, two; };

template <int MODE>
__global__ __launch_bounds__(64) void k_step(SeArgs a, const SCase *cs, const SBlock *blocks, const SegIn *segs, StepOut *out) {
  extern __shared__ __align__(16) unsigned char smem[];
  const SCase c = cs[blockIdx.x];
  const u32 lane = lane_id(), L = static_cast<u32>(uni(static_cast<int>(c.L)));
  WaveLds lds = wave_lds(smem, a, c.read);
  lds.G = static_cast<u32>(uni(static_cast<int>(c.G)));
  lds.smark[lane] = 0; lds.smark[64 + lane] = 0;
  if (MODE != 1) build_qmasks(lds, L);
  wave_sync();
  const bool g_to_a = (c.enc & 1u) != 0;
  const SeedCall sc = seed_call<true, false>(a.ix, lds, c.enc, g_to_a, L);
  SeSet S;
  S.begin_read(L);
  S.cutoff = static_cast<int>(c.cutoff);
  u32 seg_epoch = 0;
  for (u32 b = 0; b < c.n_blocks; ++b) {
    const SBlock bl = blocks[c.block_off + b];
    if (bl.clear) {  // (as seed_pass begins a specific call on the windows)
      for (u32 k = lane; k < (1u << kPosCacheBits); k += 64) lds.pcache[k] = 0;
      wave_sync();
    }
    const SegIn in = segs[bl.seg_off + lane];
    Segs sg;
    sg.na = in.na; sg.nb = in.nb; sg.lo2 = in.lo2; sg.lo3 = in.lo3;
    u32 total;
    sg.start_a = wave_excl_sum(sg.na + sg.nb, total);
    if (total == 0) continue;
    publish_segs(lds, sg);
    StepCursor cur = {0, false, false, 0, 0, 0, 0};
    if constexpr (MODE != 2) fetch_entries(a.ix, lds, sc, seg_epoch, sg, 0, total, cur);
    u32 step = 0;
    for (u32 c0 = 0; c0 < total; c0 += 128, ++step) {
      const bool two = c0 + 64 < total;
      FilterStep f;
      if constexpr (MODE == 2) f = filter_step_records(a.ix, lds, sc, S, seg_epoch, sg, bl.g0, c0, total, two, cur);
      else f = filter_step_windows<MODE == 0>(a.ix, lds, sc, seg_epoch, sg, bl.g0, c0, total, two, cur);
      StepOut o = {f.va ? 1u : 0u, f.vb ? 1u : 0u, f.pa, f.pb, f.ha, f.hma, f.hb, f.hmb, f.seen, f.cached, total, two ? 1u : 0u};
      out[static_cast<size_t>(bl.step_off + step) * 64 + lane] = o;
    }
  }
}

struct SLive { long cands = 0, hits = 0, collisions = 0, unsure = 0, sure_cases = 0, sure_hits = 0, sure_collisions = 0, redone = 0, flagged_kept = 0, dropped = 0, offered = 0, steps_two = 0, steps_one = 0, twice_in_step = 0, alias = 0, unflagged_dropped = 0; };
struct StepFixture {
  std::vector<u8> g;
  bool multibit = false;
  std::vector<u32> idx[3];
  std::vector<Read> reads;
  std::vector<SCase> cases;
  std::vector<u8> sure;         // per case: built so that the cache model never has two possible contents to choose from
  std::vector<SBlock> blocks;
  std::vector<SegIn> segs;
  std::vector<std::vector<u32>> block_pos;  // per block: its candidates' positions in order
  u32 n_steps = 0;
};

// a block of offsets: `positions` in candidate order, dealt to the lanes' 2-letter and 3-letter buckets -- empty buckets,
// buckets of one, and (where there are enough candidates) buckets of several hundred
static void add_block(StepFixture &fx, Rng &rng, u32 L, u32 g0, bool clear, bool g_to_a, const std::vector<u32> &positions) {
  const u32 total = static_cast<u32>(positions.size());
  std::vector<u32> size(128, 0);  // bucket sizes in order: lane 0's 2-letter, lane 0's 3-letter, lane 1's ...
  u32 left = total;
  const u32 n_lanes = std::min(64u, L - kKeyWeight + 1 - g0);  // (the offsets the read has: L - key weight + 1)
  for (u32 k = 0; k < 2 * n_lanes && left; ++k) {
    const u32 kind = rng.below(8);
    u32 n = kind < 2 ? 0u : (kind < 4 ? 1u : (kind < 7 ? 1u + rng.below(9) : 200u + rng.below(300)));
    if (k == 2 * n_lanes - 1) n = left;
    n = std::min(n, left);
    size[k] = n; left -= n;
  }
  SBlock b = {g0, clear ? 1u : 0u, static_cast<u32>(fx.segs.size()), fx.n_steps};
  u32 at = 0;
  std::vector<u32> &i3 = fx.idx[g_to_a ? 2 : 1];
  for (u32 lane = 0; lane < 64; ++lane) {
    SegIn s = {size[2 * lane], static_cast<u32>(fx.idx[0].size()), size[2 * lane + 1], 0};
    for (u32 k = 0; k < s.na; ++k) fx.idx[0].push_back(positions[at++] + g0 + lane);
    s.lo3 = static_cast<u32>(i3.size());
    for (u32 k = 0; k < s.nb; ++k) i3.push_back(positions[at++] + g0 + lane);
    fx.segs.push_back(s);
  }
  fx.blocks.push_back(b);
  fx.block_pos.push_back(positions);
  fx.n_steps += (total + 127) / 128;
}

// does the record of the entry at `e` carry the flag?  Its stretch of 64 * blocks - 1 bases from e - back holds a blank,
// a base past the genome or (IUPAC genome) a nibble of two or more bits -- or such a nibble lies in the 15 bases after it
static bool record_flagged(const StepFixture &fx, u32 e, u32 blocks, u32 back) {
  const long long first = static_cast<long long>(e) - back, end = first + 64ll * blocks - 1;
  for (long long q = std::max(first, 0ll); q < end; ++q) {
    if (q >= static_cast<long long>(fx.g.size())) return true;
    const u32 n = fx.g[q];
    if (n == 0 || (fx.multibit && (n & (n - 1)))) return true;
  }
  if (fx.multibit)
    for (long long q = std::max(end, 0ll); q < end + 15 && q < static_cast<long long>(fx.g.size()); ++q) { const u32 n = fx.g[q]; if (n & (n - 1)) return true; }
  return false;
}

template <int MODE> static int run_step(StepFixture &fx, Dev &dev, u32 max_len, u32 rec_blocks, SLive &live) {
  if (MODE == 2) add_records(dev, fx.idx, rec_blocks);
  else { dev.ix.index = up(fx.idx[0], 64); dev.ix.index_t = up(fx.idx[1], 64); dev.ix.index_a = up(fx.idx[2], 64); }
  SeArgs a = make_args(dev.ix, max_len, 0);
  upload_reads(a, fx.reads);
  SCase *d_cases = up(fx.cases); SBlock *d_blocks = up(fx.blocks); SegIn *d_segs = up(fx.segs);
  StepOut *d_out = up(std::vector<StepOut>(static_cast<size_t>(fx.n_steps) * 64, StepOut{9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9}));
  allow_lds(reinterpret_cast<const void *>(k_step<MODE>), lds_bytes(a));
  hipLaunchKernelGGL(k_step<MODE>, dim3(static_cast<u32>(fx.cases.size())), dim3(64), lds_bytes(a), 0, a, d_cases, d_blocks, d_segs, d_out);
  HIPCHK(hipGetLastError());
  const std::vector<StepOut> out = down(d_out, static_cast<size_t>(fx.n_steps) * 64);
  static const char *kMode[3] = {"filter_step_windows<true>", "filter_step_windows<false>", "filter_step_records"};
  const u32 back = MODE == 2 ? dev.ix.wrec_back : 0u;
  for (size_t ci = 0; ci < fx.cases.size(); ++ci) {
    const SCase &c = fx.cases[ci];
    const std::vector<u8> &q = fx.reads[c.read].nib[c.enc];
    CacheModel cache;
    for (u32 b = 0; b < c.n_blocks; ++b) {
      const SBlock &bl = fx.blocks[c.block_off + b];
      const std::vector<u32> &pos = fx.block_pos[c.block_off + b];
      const u32 total = static_cast<u32>(pos.size());
      if (bl.clear) cache.clear();
      // the offset each candidate comes from (records: its window's place in the record), from the buckets in order
      std::vector<u32> off_of(total), entry_of(total);
      {
        u32 at = 0;
        for (u32 lane = 0; lane < 64; ++lane) {
          const SegIn &s = fx.segs[bl.seg_off + lane];
          for (u32 k = 0; k < s.na; ++k, ++at) { off_of[at] = bl.g0 + lane; entry_of[at] = fx.idx[0][s.lo2 + k]; }
          for (u32 k = 0; k < s.nb; ++k, ++at) { off_of[at] = bl.g0 + lane; entry_of[at] = fx.idx[(c.enc & 1) ? 2 : 1][s.lo3 + k]; }
        }
        if (at != total) { std::printf("FAIL fixture: a block's buckets hold %u candidates of %u\n", at, total); return 1; }
      }
      for (u32 c0 = 0, step = 0; c0 < total; c0 += 128, ++step) {
        const bool two = c0 + 64 < total;
        (two ? live.steps_two : live.steps_one) += 1;
        std::vector<u32> pa, pb;
        for (u32 k = c0; k < std::min(total, c0 + 64); ++k) pa.push_back(pos[k]);
        for (u32 k = c0 + 64; k < std::min(total, c0 + 128); ++k) pb.push_back(pos[k]);
        std::vector<CacheModel::Look> looks;
        if (MODE != 2) {
          looks = cache.step(pa, pb);
          std::set<u32> seen_here;
          for (u32 k = c0; k < std::min(total, c0 + 128); ++k) if (!seen_here.insert(pos[k]).second) ++live.twice_in_step;
        }
        for (u32 k = c0; k < c0 + 128; ++k) {
          const u32 lane = (k - c0) & 63u;
          const bool second = k - c0 >= 64;
          const StepOut &o = out[static_cast<size_t>(bl.step_off + step) * 64 + lane];
          const bool valid = k < total;
          const u32 got_v = second ? o.vb : o.va, got_p = second ? o.pb : o.pa;
          const int got_h = second ? o.hb : o.ha, got_m = second ? o.hmb : o.hma;
          auto fail = [&](const char *what, long long want, long long got) {
            std::printf("FAIL step: %s, case %zu (L %u, G %u, encoding %u, cutoff %u), block %u (g0 %u, %u candidates), step %u, lane %u %c half, candidate %u at pos %u from offset %u: %s expected %lld got %lld\n",
                        kMode[MODE], ci, c.L, c.G, c.enc, c.cutoff, b, bl.g0, total, step, lane, second ? 'b' : 'a', k, valid ? pos[k] : 0u, valid ? off_of[k] : 0u, what, want, got);
            return 1;
          };
          if (!second && (o.total != total || o.two != (two ? 1u : 0u))) return fail("the block's total / two", total, o.total);
          if (!second) {
            const u32 seen = (k < total ? 1u : 0u) + (k + 64 < total ? 1u : 0u);
            if (o.seen != seen) return fail("seen", seen, o.seen);
          }
          if (!valid) { if (got_v) return fail("valid", 0, got_v); continue; }
          ++live.cands;
          const Dist sd = serial_distance(fx.g, q, pos[k], words_of(c.L));
          if (MODE == 2) {
            const bool flagged = fx.multibit && record_flagged(fx, entry_of[k], rec_blocks, back);
            // (the planes' count over the read's letters, code 0 where the genome is blank; an unflagged record of the IUPAC
            // genome is one-hot throughout)
            const int on_record = plane_count(fx.g, q, pos[k]);
            const bool offered = flagged || on_record <= static_cast<int>(c.cutoff);
            if (got_v != (offered ? 1u : 0u)) return fail(flagged ? "offered (a flagged record)" : "offered", offered, got_v);
            if (!offered) {
              if (sd.dmax <= static_cast<int>(c.cutoff)) return fail("a dropped candidate's serial dmax against the cutoff: above", c.cutoff + 1, sd.dmax);
              ++live.dropped; live.unflagged_dropped += fx.multibit;
              continue;
            }
            if (flagged) {  // beyond the cutoff on the planes whatever codes the IUPAC letters got?
              int lb = 0;
              for (u32 j = 0; j < c.L; ++j) { const u32 n = g_at(fx.g, pos[k] + j); if ((n & (n - 1)) == 0) lb += (q[j] & (n ? n : 1u)) == 0; }
              live.flagged_kept += lb > static_cast<int>(c.cutoff);
            }
          }
          else if (!got_v) return fail("valid", 1, 0);
          ++live.offered;
          if (got_p != pos[k]) return fail("pos", pos[k], got_p);
          if (got_h != sd.d) return fail("h", sd.d, got_h);
          if (got_m != sd.dmax) return fail("hmax", sd.dmax, got_m);
          if (MODE != 1 && plane_count(fx.g, q, pos[k]) != sd.d) ++live.redone;  // (what the planes alone would have said differs)
          if (MODE != 2 && (pos[k] & 0xFFFFFFu) == 0) ++live.alias;
        }
        // cached, per lane: the a and the b candidate's lookups together
        for (u32 lane = 0; lane < 64; ++lane) {
          const StepOut &o = out[static_cast<size_t>(bl.step_off + step) * 64 + lane];
          int lo = 0, hi = 0;
          if (MODE != 2) {
            if (lane < pa.size()) { lo += looks[lane].hit_lo; hi += looks[lane].hit_hi; }
            if (lane < pb.size()) { lo += looks[pa.size() + lane].hit_lo; hi += looks[pa.size() + lane].hit_hi; }
          }
          if (static_cast<int>(o.cached) < lo || static_cast<int>(o.cached) > hi) {
            std::printf("FAIL step: %s, case %zu (L %u, G %u), block %u, step %u, lane %u: cached %u, the cache model says %d .. %d (a at %u, b at %u)\n", kMode[MODE], ci, c.L, c.G, b, step, lane,
                        o.cached, lo, hi, lane < pa.size() ? pa[lane] : 0u, lane < pb.size() ? pb[lane] : 0u);
            return 1;
          }
        }
      }
    }
    live.hits += cache.hits; live.collisions += cache.evictions; live.unsure += cache.unsure;
    if (fx.sure[ci]) {  // every `cached` of this case was held to one value
      if (cache.unsure) { std::printf("FAIL fixture: case %zu was to leave the cache model sure of every lookup and left %ld open\n", ci, cache.unsure); return 1; }
      ++live.sure_cases; live.sure_hits += cache.hits; live.sure_collisions += cache.evictions;
    }
  }
  HIPCHK(hipFree(d_cases)); HIPCHK(hipFree(d_blocks)); HIPCHK(hipFree(d_segs)); HIPCHK(hipFree(d_out));
  free_reads(a);
  if (MODE == 2) free_records(dev);
  else { HIPCHK(hipFree(const_cast<u32 *>(dev.ix.index))); HIPCHK(hipFree(const_cast<u32 *>(dev.ix.index_t))); HIPCHK(hipFree(const_cast<u32 *>(dev.ix.index_a))); }
  return 0;
}

// The cases of one mode on one genome: per length, encoding and block size, a specific call (the cache cleared, windows
// alone) and a sensitive call of the same encoding that proposes many of its positions again.
static void step_cases(StepFixture &fx, Rng &rng, u32 mode, const std::vector<std::pair<u32, u32>> &len_g, const std::vector<u32> &blanks, const std::vector<u32> &iupacs) {
  static const u32 kTotals[9] = {1, 63, 64, 65, 127, 128, 129, 300, 1000};
  const u32 n_bases = static_cast<u32>(fx.g.size());
  u32 plant_at = 4096 + 8192 * mode;
  u32 n = 0;
  for (const auto &lg : len_g)
    for (u32 total : kTotals) {
      const u32 L = lg.first, enc = n++ % 4;
      const Read rd = encode(random_letters(rng, L, n % 3 == 0));
      const std::vector<u8> &q = rd.nib[enc];
      fx.reads.push_back(rd);
      // near copies of the read (0 .. 7 letters changed), some of them running into a blank stretch or an IUPAC letter
      std::vector<u32> near;
      for (u32 k = 0; k < 12; ++k) {
        const u32 pos = plant_at + rng.below(64);
        plant_at += (L + 200) & ~63u;
        for (u32 j = 0; j < L; ++j) if (q[j]) fx.g[pos + j] = admitted_letter(rng, q[j]);
        for (u32 j = 0; j < k % 8; ++j) { const u32 at = rng.below(L); if (q[at]) fx.g[pos + at] = refused_letter(rng, q[at]); }
        if (k % 4 == 1) fx.g[pos + rng.below(L)] = 0;                      // a blank inside the window
        if (k % 4 == 2) fx.g[pos + L + rng.below(16)] = 0;                 // ... under the last word's padding, or just past it
        if (fx.multibit && k % 4 == 3) { const u32 at = pos + rng.below(L + 15); fx.g[at] = static_cast<u8>(fx.g[at] | (1u << rng.below(4)) | (1u << rng.below(4))); }
        near.push_back(pos);
      }
      // a pair of positions that share a cache slot
      u32 p1 = 70000 + rng.below(n_bases - 200000), p2 = p1 + 1;
      while (cache_slot(p2) != cache_slot(p1)) ++p2;
      auto draw = [&](u32 k) -> u32 {
        const u32 kind = rng.below(16);
        if (kind < 5) return near[rng.below(static_cast<u32>(near.size()))];
        if (kind < 7 && !blanks.empty()) return blanks[rng.below(static_cast<u32>(blanks.size()))] - rng.below(L + 20);
        if (kind < 8 && !iupacs.empty()) return iupacs[rng.below(static_cast<u32>(iupacs.size()))] - rng.below(L + 14);
        if (kind < 9 && n_bases > (1u << 24) + 4096 && mode != 2) return 1u << 24;
        (void)k;
        return 1000 + rng.below(n_bases - 3000);
      };
      // every third case of the window steps with 65 candidates or more leaves the model nothing to choose: its positions
      // come from a pool in which no two share a slot (none p1's and p2's either), so that two different positions never
      // write one slot in one step; p1 and p2 meet in different steps.  `cached` is then one number for every lane.
      const bool sure = mode != 2 && total >= 65 && n % 3 == 1;
      std::vector<u32> pool;
      if (sure) {
        std::set<u32> slots = {cache_slot(p1)};
        for (u32 tries = 0; pool.size() < 150 && tries < 100000; ++tries) { const u32 p = draw(0); if (slots.insert(cache_slot(p)).second) pool.push_back(p); }
      }
      auto pick = [&](u32 k) -> u32 { return sure ? pool[rng.below(static_cast<u32>(pool.size()))] : draw(k); };
      std::vector<u32> first, second;
      for (u32 k = 0; k < total; ++k) first.push_back(pick(k));
      if (total >= 3) { first[1] = first[0]; }                                    // proposed twice in one step ...
      if (total >= 129) { first[2] = p1; first[70] = first[3]; first[128] = first[5]; }
      for (u32 k = 0; k < total; ++k) second.push_back(k % 3 == 0 ? first[rng.below(total)] : pick(k));  // ... and again in a later call
      if (sure) for (u32 k = 0; k < std::min(total, 128u); ++k) if (second[k] == p1) second[k] = pool[k % pool.size()];  // (p1 not in p2's step)
      if (total >= 129) { second[0] = p2; second[128] = p1; }                     // p2 evicts p1, which then misses
      const u32 cutoff = mode == 2 ? (n % 2 ? L / 10 : static_cast<u32>(0.4 * L)) : 0u;
      SCase c = {L, static_cast<u32>(fx.reads.size() - 1), enc, mode, lg.second, cutoff, 0, static_cast<u32>(fx.blocks.size())};
      add_block(fx, rng, L, 0, mode != 2, (enc & 1) != 0, first);
      add_block(fx, rng, L, 0, false, (enc & 1) != 0, second);
      c.n_blocks = 2;
      if (L >= 100 && total <= 300) {  // the sensitive call's second block of offsets (g0 = 64)
        std::vector<u32> third;
        for (u32 k = 0; k < std::min(total, 130u); ++k) third.push_back(k % 2 ? first[rng.below(total)] : pick(k));
        add_block(fx, rng, L, 64, false, (enc & 1) != 0, third);
        c.n_blocks = 3;
      }
      fx.cases.push_back(c);
      fx.sure.push_back(sure ? 1 : 0);
    }
}

static int cmd_step() {
  const double t0 = now_s();
  Rng rng(4242);
  // the large genome (a position at 2^24: its low 24 bits are those of an empty cache slot) with blank stretches, and a small
  // one with IUPAC letters as well
  std::vector<u8> big, small;
  grow_random(big, (1u << 24) + 16384, rng);
  grow_random(small, 1u << 19, rng);
  std::vector<u32> blanks_big, blanks_small, iupacs;
  for (u32 k = 0; k < 40; ++k) {
    const u32 at = 300000 + k * 39119, run = k % 3 == 0 ? 1u : 1u + rng.below(90);
    for (u32 j = 0; j < run; ++j) { big[at + j] = 0; if (k < 10) small[at / 4 + j] = 0; }
    blanks_big.push_back(at); if (k < 10) blanks_small.push_back(at / 4);
  }
  for (u32 k = 0; k < 40; ++k) {
    const u32 at = 150000 + k * 8111;
    small[at] = static_cast<u8>(3u + rng.below(13)); if ((small[at] & (small[at] - 1)) == 0) small[at] = 10;
    iupacs.push_back(at);
  }
  SLive lw, ln, lr, lm;
  {  // planes: pairs, groups of four and of eight
    StepFixture fx; fx.g = big;
    step_cases(fx, rng, 0, {{50, 2}, {100, 2}, {128, 2}, {150, 4}, {192, 4}, {300, 8}, {448, 8}}, blanks_big, {});
    // (the genome is the fixture's: the planted copies went into fx.g)
    Dev d = make_dev(fx.g, true, false);
    if (run_step<0>(fx, d, 448, 0, lw)) return 1;
    free_dev(d);
  }
  {  // planes of the genome with IUPAC letters
    StepFixture fx; fx.g = small; fx.multibit = true;
    step_cases(fx, rng, 0, {{100, 2}, {150, 4}}, blanks_small, iupacs);
    Dev d = make_dev(fx.g, true, true);
    if (!d.ix.multibit) { std::printf("FAIL fixture: the small genome's IUPAC letters were not seen\n"); return 1; }
    SLive l;
    if (run_step<0>(fx, d, 448, 0, l)) return 1;
    free_dev(d);
    lw.redone += l.redone; lw.cands += l.cands; lw.hits += l.hits; lw.collisions += l.collisions; lw.unsure += l.unsure; lw.sure_cases += l.sure_cases; lw.sure_hits += l.sure_hits; lw.sure_collisions += l.sure_collisions; lw.steps_one += l.steps_one; lw.steps_two += l.steps_two;
  }
  {  // the nibble array
    StepFixture fx; fx.g = small; fx.multibit = true;
    step_cases(fx, rng, 1, {{50, 0}, {129, 0}, {448, 0}, {1000, 0}}, blanks_small, iupacs);
    Dev d = make_dev(fx.g, false, false);
    if (run_step<1>(fx, d, 1024, 0, ln)) return 1;
    free_dev(d);
  }
  for (int multi = 0; multi < 2; ++multi) {  // records of three blocks (one lane a window, two mask blocks) and of four
    for (u32 blocks : {3u, 4u}) {
      StepFixture fx; fx.g = small; fx.multibit = multi != 0;
      if (!multi) for (u32 at : iupacs) fx.g[at] = 4;
      if (blocks == 3) step_cases(fx, rng, 2, {{50, 2}, {100, 2}, {108, 2}}, blanks_small, multi ? iupacs : std::vector<u32>());
      else step_cases(fx, rng, 2, {{109, 4}, {140, 4}}, blanks_small, multi ? iupacs : std::vector<u32>());
      Dev d = make_dev(fx.g, true, multi != 0);
      if (run_step<2>(fx, d, window_record_max_len(blocks), blocks, multi ? lm : lr)) return 1;
      free_dev(d);
    }
  }
  // the cache model may leave a lookup open (unsure_lookups) only where two positions really raced for a slot: the cases
  // built to have no such race must be many and hold hits and collisions of their own (every `cached` there is compared
  // with one number), and over all cases the lookups held to a hit must outnumber the open ones four to one
  const bool model_held = lw.sure_cases && lw.sure_hits && lw.sure_collisions && ln.sure_cases && ln.sure_hits && ln.sure_collisions && lw.hits >= 4 * lw.unsure && ln.hits >= 4 * ln.unsure;
  const bool ok = model_held && lw.hits && lw.collisions && lw.redone && lw.steps_one && lw.steps_two && lw.twice_in_step && lw.alias && ln.hits && ln.collisions && ln.steps_one && ln.steps_two &&
                  lr.redone && lr.dropped && lr.offered && lr.steps_one && lr.steps_two && lm.flagged_kept && lm.unflagged_dropped && lm.redone && lm.dropped;
  std::printf("%s step windows<true>: candidates=%ld cache_hits=%ld slot_collisions=%ld unsure_lookups=%ld exact_cases=%ld exact_cache_hits=%ld exact_slot_collisions=%ld redone=%ld twice_in_step=%ld at_2^24=%ld steps_with_b=%ld steps_without_b=%ld; "
              "windows<false>: candidates=%ld cache_hits=%ld slot_collisions=%ld unsure_lookups=%ld exact_cases=%ld exact_cache_hits=%ld exact_slot_collisions=%ld steps_with_b=%ld steps_without_b=%ld; records: candidates=%ld offered=%ld dropped_by_cutoff=%ld redone=%ld steps_with_b=%ld steps_without_b=%ld; "
              "records, IUPAC genome: candidates=%ld flagged_kept=%ld unflagged_dropped=%ld redone=%ld; %.2f s\n", ok ? "OK" : "FAIL coverage:",
              lw.cands, lw.hits, lw.collisions, lw.unsure, lw.sure_cases, lw.sure_hits, lw.sure_collisions, lw.redone, lw.twice_in_step, lw.alias, lw.steps_two, lw.steps_one, ln.cands, ln.hits, ln.collisions, ln.unsure, ln.sure_cases, ln.sure_hits, ln.sure_collisions, ln.steps_two, ln.steps_one,
              lr.cands, lr.offered, lr.dropped, lr.redone, lr.steps_two, lr.steps_one, lm.cands, lm.flagged_kept, lm.unflagged_dropped, lm.redone, now_s() - t0);
  return ok ? 0 : 1;
}

// =================================================================================================================
// replay
// =================================================================================================================
struct RCase { u32 L, flags, n_spec, n_sens, chunk_off; };
struct RLane { int valid, h, hmax; u32 pos; };
struct ROut { int hk; u32 pf, pp; int sz, cutoff, sure_ambig, best_d; u32 best_f, best_p, updates, fifo, ran_sensitive; };

__global__ __launch_bounds__(64) void k_replay(const RCase *cs, const RLane *lanes, ROut *out) {
  const RCase c = cs[blockIdx.x];
  const u32 lane = lane_id();
  SeSet S;
  S.begin_read(c.L);
  WorkTally wt = {};
  S.cutoff = S.good_cutoff;  // set_specific
  for (u32 k = 0; k < c.n_spec && !S.sure_ambig; ++k) {
    const RLane l = lanes[static_cast<size_t>(c.chunk_off + k) * 64 + lane];
    replay_chunk<true, true>(S, wt, c.flags, l.valid != 0, l.h, l.hmax, l.pos);
  }
  u32 ran = 0;
  if (S.sz != static_cast<int>(kSeCap) || S.cutoff > S.good_cutoff) {  // should_do_sensitive
    ran = 1;
    S.cutoff = S.top_d();  // set_sensitive
    for (u32 k = 0; k < c.n_sens && !S.sure_ambig; ++k) {
      const RLane l = lanes[static_cast<size_t>(c.chunk_off + c.n_spec + k) * 64 + lane];
      replay_chunk<false, true>(S, wt, c.flags, l.valid != 0, l.h, l.hmax, l.pos);
    }
  }
  ROut o = {S.hk, S.pf, S.pp, S.sz, S.cutoff, S.sure_ambig ? 1 : 0, S.best_d, S.best_f, S.best_p, wt.updates, wt.fifo_updates, ran};
  out[static_cast<size_t>(blockIdx.x) * 64 + lane] = o;
}

// the appending path of the pair set: a specific call on a set that has not turned into a heap -- every survivor of the
// chunk's first ballot goes into the list, in lane order
__global__ __launch_bounds__(64) void k_replay_append(const RCase *cs, const RLane *lanes, u32 *pos_out, i16 *d_out, int *meta, u32 cap) {
  __shared__ u32 heap[1024], lpos[1024];
  __shared__ i16 ld[1024];
  const RCase c = cs[blockIdx.x];
  const u32 lane = lane_id();
  PeSet S = {};
  S.heap = heap; S.lpos = lpos; S.ld = ld; S.cap_avail = cap;
  S.begin_read(c.L);
  S.cutoff = S.good_cutoff;
  WorkTally wt = {};
  for (u32 k = 0; k < c.n_spec && !S.sure_ambig; ++k) {
    const RLane l = lanes[static_cast<size_t>(c.chunk_off + k) * 64 + lane];
    replay_chunk<true, true>(S, wt, c.flags, l.valid != 0, l.h, l.hmax, l.pos);
  }
  wave_sync();
  for (u32 k = lane; k < cap; k += 64) { pos_out[static_cast<size_t>(blockIdx.x) * cap + k] = lpos[k]; d_out[static_cast<size_t>(blockIdx.x) * cap + k] = ld[k]; }
  if (lane == 0) { int *m = meta + 6 * blockIdx.x; m[0] = S.sz; m[1] = S.cutoff; m[2] = S.sure_ambig; m[3] = S.overflow; m[4] = S.heaped; m[5] = static_cast<int>(wt.updates); }
}

static int cmd_replay() {
  const double t0 = now_s();
  Rng rng(99);
  std::vector<RCase> cases;
  std::vector<RLane> lanes;
  const u32 kShapes = 8, kCases = 320;
  for (u32 n = 0; n < kCases; ++n) {
    const u32 shape = n % kShapes, L = 60 + 10 * (n % 15);  // good_cutoff 6 .. 20, the sentinel at 24 .. 80
    const int good = static_cast<int>(L / 10), worst = static_cast<int>(0.4 * L);
    RCase c = {L, (n & 1) ? kFlagRC : 0u, 4 + n % 5, 6 + n % 7, static_cast<u32>(lanes.size() / 64)};
    u32 next_pos = 1000;
    for (u32 k = 0; k < c.n_spec + c.n_sens; ++k) {
      const bool sens = k >= c.n_spec;
      for (u32 lane = 0; lane < 64; ++lane) {
        RLane l = {1, 0, 0, next_pos++};
        const u32 r = rng.next();
        switch (shape) {
          case 0: l.h = 1 + r % (sens ? worst + 4 : good + 4); break;                                   // uniform around the cutoff
          case 1: l.h = (r % 16) ? good : 1 + r % good; break;                                          // mostly ties at the specific cutoff
          case 2: l.h = sens ? std::max(1, worst - static_cast<int>((k - c.n_spec) * 64 + lane) / 6 + static_cast<int>(r % 2)) : good + 1 + r % 3; break;  // a sensitive call whose cutoff keeps tightening
          case 3: l.h = (r % 200) ? 2 : 1; break;                                                      // long runs of ties with a full set
          case 4: l.h = (r % 90 == 0) ? 0 : 1 + r % (good + 2); if (l.h == 0 && (r >> 8) % 2) l.pos = 777; break;  // exact hits, some of them the same one again
          case 5: l.h = sens ? 1 + r % worst : 1 + r % good; break;
          case 6: l.h = (lane % 21 == 20 && k == c.n_spec + 1) ? 0 : (sens ? worst - 1 - static_cast<int>(r % 3) : good + 1); break;  // two exact hits in mid-chunk, valid lanes after them
          default: l.h = 3 + r % 3; break;                                                             // a narrow band: ties of several values
        }
        l.hmax = l.h;
        if ((r >> 12) % 7 == 0) l.hmax = l.h + 1 + static_cast<int>((r >> 16) % (shape == 3 ? 2 : 12));  // an IUPAC candidate's running sum peaked higher
        if ((r >> 20) % 5 == 0 && shape != 3) l.valid = 0;                                               // invalid lanes in between
        if (shape == 3 && (r >> 20) % 40 == 0) l.valid = 0;
        if (!l.valid) { l.h = static_cast<int>(r % 3); l.hmax = l.h; }                                   // (what an invalid lane holds must not matter: small distances)
        lanes.push_back(l);
      }
    }
    cases.push_back(c);
  }
  RCase *d_cases = up(cases); RLane *d_lanes = up(lanes);
  ROut *d_out = up(std::vector<ROut>(cases.size() * 64));
  hipLaunchKernelGGL(k_replay, dim3(static_cast<u32>(cases.size())), dim3(64), 0, 0, d_cases, d_lanes, d_out);
  HIPCHK(hipGetLastError());
  const std::vector<ROut> out = down(d_out, cases.size() * 64);
  long updates = 0, fifo = 0, invalid_between = 0, peak_refused = 0, tightened = 0, ambig_cut = 0, sensitive = 0, full_sets = 0, exact = 0;
  for (size_t n = 0; n < cases.size(); ++n) {
    const RCase &c = cases[n];
    SetModel m;
    m.reset(c.L);
    m.cutoff = m.good_cutoff;
    auto run = [&](bool specific, u32 first, u32 count) {
      for (u32 k = 0; k < count && !m.sure_ambig; ++k) {
        std::vector<SetModel::Lane> chunk;
        const RLane *l = lanes.data() + static_cast<size_t>(c.chunk_off + first + k) * 64;
        const int at_start = m.cutoff;
        for (u32 j = 0; j < 64; ++j) chunk.push_back({l[j].valid != 0, l[j].h, l[j].hmax, l[j].pos});
        // liveness, from a walk of its own over the same rule
        {
          SetModel w = m;
          bool seen_valid = false, gap = false;
          for (u32 j = 0; j < 64; ++j) {
            if (w.sure_ambig) { for (u32 i = j; i < 64; ++i) if (l[i].valid && l[i].hmax <= w.cutoff) { ++ambig_cut; break; } break; }
            if (!l[j].valid) { gap |= seen_valid; continue; }
            if (gap) { ++invalid_between; gap = false; }
            seen_valid = true;
            if (l[j].hmax > w.cutoff) { peak_refused += l[j].h <= w.cutoff; tightened += l[j].hmax <= at_start; continue; }
            exact += l[j].h == 0;
            w.update(specific, l[j].h, c.flags, l[j].pos);
          }
        }
        m.replay(specific, c.flags, chunk);
      }
    };
    run(true, 0, c.n_spec);
    const bool want_sens = m.sz != kSetCap || m.cutoff > m.good_cutoff;
    if (want_sens) { m.cutoff = m.v[0].d; run(false, c.n_spec, c.n_sens); ++sensitive; }
    const ROut *o = out.data() + n * 64;
    auto fail = [&](const char *what, long long want, long long got) {
      std::printf("FAIL replay: case %zu (shape %zu, L %u, %u specific and %u sensitive chunks): %s expected %lld got %lld\n", n, n % kShapes, c.L, c.n_spec, c.n_sens, what, want, got);
      return 1;
    };
    if (o[0].ran_sensitive != (want_sens ? 1u : 0u)) return fail("sensitive call", want_sens, o[0].ran_sensitive);
    if (o[0].sz != static_cast<int>(m.sz)) return fail("size", m.sz, o[0].sz);
    if (o[0].cutoff != m.cutoff) return fail("cutoff", m.cutoff, o[0].cutoff);
    if (o[0].sure_ambig != (m.sure_ambig ? 1 : 0)) return fail("sure_ambig", m.sure_ambig, o[0].sure_ambig);
    if (o[0].best_d != m.best.d || o[0].best_f != m.best.flags || o[0].best_p != m.best.pos) return fail("the exact hit's position", m.best.pos, o[0].best_p);
    if (o[0].updates != m.updates) return fail("wt.updates", m.updates, o[0].updates);
    if (o[0].fifo != m.fifo) return fail("wt.fifo_updates", m.fifo, o[0].fifo);
    for (u32 k = 0; k < m.sz; ++k) {
      const int key = o[k].hk, slot = key & 255;
      if ((key >> 8) != m.v[k].d || slot >= 64 || o[slot].pp != m.v[k].pos || o[slot].pf != m.v[k].flags) {
        std::printf("FAIL replay: case %zu (shape %zu, L %u): heap[%u] holds d %d pos %u flags %u, libstdc++'s d %d pos %u flags %u\n", n, n % kShapes, c.L, k, key >> 8, slot < 64 ? o[slot].pp : 0u,
                    slot < 64 ? o[slot].pf : 0u, m.v[k].d, m.v[k].pos, m.v[k].flags);
        return 1;
      }
    }
    updates += m.updates; fifo += m.fifo; full_sets += m.sz == kSetCap;
  }
  HIPCHK(hipFree(d_out));
  // the pair set, appending: the same chunks' specific parts
  const u32 cap = 1024;
  u32 *d_pos = up(std::vector<u32>(cases.size() * cap, 0));
  i16 *d_d = up(std::vector<i16>(cases.size() * cap, 0));
  int *d_meta = up(std::vector<int>(cases.size() * 6, 0));
  hipLaunchKernelGGL(k_replay_append, dim3(static_cast<u32>(cases.size())), dim3(64), 0, 0, d_cases, d_lanes, d_pos, d_d, d_meta, cap);
  HIPCHK(hipGetLastError());
  const std::vector<u32> apos = down(d_pos, cases.size() * cap);
  const std::vector<i16> ad = down(d_d, cases.size() * cap);
  const std::vector<int> meta = down(d_meta, cases.size() * 6);
  long appended = 0, append_refused = 0;
  for (size_t n = 0; n < cases.size(); ++n) {
    const RCase &c = cases[n];
    // pe_candidates in its specific pass (src/abismal.cpp:824-842): the cutoff stays at good_cutoff, every hit within it is kept in order
    const int cutoff = static_cast<int>(c.L / 10);
    std::vector<u32> wp = {0};
    std::vector<int> wd = {static_cast<i16>(0.4 * c.L)};
    // (sure_ambig needs a full set at cutoff 0; the cutoff here is a tenth of 60 letters or more, so it stays false)
    for (u32 k = 0; k < c.n_spec; ++k)
      for (u32 j = 0; j < 64; ++j) {
        const RLane &l = lanes[static_cast<size_t>(c.chunk_off + k) * 64 + j];
        if (!l.valid) continue;
        if (l.hmax > cutoff) { append_refused += l.h <= cutoff; continue; }
        wp.push_back(l.pos); wd.push_back(l.h);
      }
    const int *m = meta.data() + 6 * n;
    if (wp.size() > cap) { std::printf("FAIL fixture: case %zu appends %zu entries\n", n, wp.size()); return 1; }
    if (m[0] != static_cast<int>(wp.size()) || m[1] != cutoff || m[2] || m[3] || m[4] || m[5] != static_cast<int>(wp.size()) - 1) {
      std::printf("FAIL replay: pair set, case %zu (L %u): size %d cutoff %d sure_ambig %d overflow %d heaped %d updates %d; expected size %zu cutoff %d, none of the three, %zu updates\n", n, c.L, m[0], m[1], m[2], m[3], m[4], m[5], wp.size(), cutoff, wp.size() - 1);
      return 1;
    }
    for (size_t k = 0; k < wp.size(); ++k)
      if (apos[n * cap + k] != wp[k] || ad[n * cap + k] != wd[k]) {
        std::printf("FAIL replay: pair set, case %zu (L %u): list entry %zu holds pos %u d %d, expected pos %u d %d\n", n, c.L, k, apos[n * cap + k], ad[n * cap + k], wp[k], wd[k]);
        return 1;
      }
    appended += static_cast<long>(wp.size()) - 1;
  }
  const bool ok = updates && fifo && invalid_between && peak_refused && tightened && ambig_cut && sensitive && full_sets && exact && appended && append_refused;
  std::printf("%s replay cases=%zu updates=%ld fifo_updates=%ld invalid_lanes_between_valid=%ld hmax_above_h_below_cutoff=%ld refused_after_mid_chunk_tightening=%ld chunks_cut_by_sure_ambig=%ld exact_hits=%ld sensitive_calls=%ld "
              "full_sets=%ld pair_set_appended=%ld pair_set_hmax_refused=%ld; %.2f s\n", ok ? "OK" : "FAIL coverage:", cases.size(), updates, fifo, invalid_between, peak_refused, tightened, ambig_cut, exact, sensitive, full_sets,
              appended, append_refused, now_s() - t0);
  return ok ? 0 : 1;
}

// =================================================================================================================
// ghost
// =================================================================================================================
constexpr u64 kGhostCanary = 0x5EED5EED5EED5EEDull;
__global__ __launch_bounds__(64) void k_ghost(SeArgs a, const u32 *which, u32 map_len, const u64 *word0, u64 *out) {
  extern __shared__ __align__(16) unsigned char smem[];
  const u64 r = which[blockIdx.x];
  const u32 L = a.lens[r], lane = lane_id();
  WaveLds lds = wave_lds(smem, a, r);
  for (u32 k = lane; k < 4 * a.WB; k += 64) lds.qbits[k] = (k % a.WB == 0) ? word0[blockIdx.x * 4 + k / a.WB] : kGhostCanary;
  wave_sync();
  ghost_bits(a.packed, a.lens, r, L, a.max_len, map_len, a.W, a.WB, lds.qbits);
  for (u32 k = lane; k < 4 * a.WB; k += 64) out[static_cast<size_t>(blockIdx.x) * 4 * a.WB + k] = lds.qbits[k];
}

static int cmd_ghost() {
  const double t0 = now_s();
  Rng rng(5);
  long compared = 0, zero_fill = 0, past_max = 0, from_donor = 0, donor_back[4] = {0, 0, 0, 0}, no_donor = 0, layered = 0, short_between = 0, reads_checked = 0;
  // a batch: its reads' lengths, the longest read its launch is shaped for, the shortest it maps
  struct Batch { std::vector<u32> lens; u32 max_len, map_len; };
  std::vector<Batch> batches;
  const u32 kTest[6] = {0, 1, 63, 64, 65, 200}, kLens[4] = {35, 44, 45, 46};
  for (u32 variant = 0; variant < 12; ++variant) {
    Batch b;
    b.map_len = variant % 4 == 3 ? 29u : 35u;                   // (29: an index with window 12)
    b.max_len = variant % 3 == 0 ? 150u : (variant % 3 == 1 ? 100u : 60u);   // (100, 60: k = L + lane reaches and passes it)
    const u32 n = 260;
    b.lens.assign(n, 0);
    for (u32 r = 0; r < n; ++r) b.lens[r] = rng.below(3) == 0 ? b.map_len - 1 - rng.below(10) : (rng.below(4) == 0 ? 47 + rng.below(b.max_len - 46) : 20 + rng.below(20));
    if (variant == 11) for (u32 r = 0; r < n; ++r) b.lens[r] = 10 + rng.below(b.map_len - 10);  // no earlier read is long enough
    for (u32 k = 0; k < 6; ++k) {
      const u32 r = kTest[k];
      b.lens[r] = b.map_len == 29 ? 36 + (k + variant) % 3 : kLens[(k + variant) % 4];
      if (variant == 11) continue;
      // the donor 1, 64, 65 or 150 reads back, nothing of its length in between; a shorter donor in front of it on some
      const u32 backs[4] = {1, 64, 65, 150}, back = backs[(k + variant / 4) % 4];
      if (r >= back) {
        for (u32 q = r - back + 1; q < r; ++q) b.lens[q] = (q % 3 == 0 && variant % 2) ? b.map_len + rng.below(b.lens[r] - b.map_len + 1) : 10 + rng.below(b.map_len - 10);
        b.lens[r - back] = b.max_len - rng.below(8);
        if (back > 1 && variant % 2 == 0) b.lens[r - 1] = b.lens[r] + 1 + rng.below(12);  // covers the first ghost letters only: the rest come from further back
      }
    }
    batches.push_back(b);
  }
  for (size_t bi = 0; bi < batches.size(); ++bi) {
    const Batch &b = batches[bi];
    std::vector<Read> reads;
    for (u32 len : b.lens) reads.push_back(encode(random_letters(rng, len, true)));
    SeArgs a = make_args(DevIndex{}, b.max_len, 0);
    upload_reads(a, reads);
    std::vector<u32> which;
    for (u32 r = 0; r < b.lens.size(); ++r) if (b.lens[r] >= b.map_len && b.lens[r] <= 46) which.push_back(r);
    std::vector<u64> word0(which.size() * 4);
    for (auto &w : word0) { rng.next(); w = rng.s; }
    u32 *d_which = up(which); u64 *d_word0 = up(word0);
    u64 *d_out = up(std::vector<u64>(which.size() * 4 * a.WB, 0));
    allow_lds(reinterpret_cast<const void *>(k_ghost), lds_bytes(a));
    hipLaunchKernelGGL(k_ghost, dim3(static_cast<u32>(which.size())), dim3(64), lds_bytes(a), 0, a, d_which, b.map_len, d_word0, d_out);
    HIPCHK(hipGetLastError());
    const std::vector<u64> out = down(d_out, which.size() * 4 * a.WB);
    GhostBuffers gb;
    std::vector<int> writer(1200, -1);  // who wrote position k last
    size_t wi = 0;
    for (u32 r = 0; r < b.lens.size(); ++r) {
      if (wi < which.size() && which[wi] == r) {
        const u32 L = b.lens[r];
        ++reads_checked;
        std::set<int> donors;
        for (u32 k = L; k < L + 64; ++k) {
          const int w = writer[k];
          if (w < 0) { ++zero_fill; past_max += k >= b.max_len; continue; }
          ++from_donor; donors.insert(w);
          const u32 back = r - static_cast<u32>(w);
          for (int t = 0; t < 4; ++t) donor_back[t] += back == (t == 0 ? 1u : (t == 1 ? 64u : (t == 2 ? 65u : 150u)));
        }
        if (donors.empty()) ++no_donor;
        if (donors.size() > 1) ++layered;
        for (int w : donors) for (u32 q = static_cast<u32>(w) + 1; q < r; ++q) if (b.lens[q] < b.map_len) { ++short_between; break; }
        for (int e = 0; e < 4; ++e) {
          u64 want[2];
          ghost_words(gb, e, L, word0[wi * 4 + e], want);
          for (u32 k = 0; k < a.WB; ++k) {
            const u64 got = out[(wi * 4 + e) * a.WB + k], w = k < 2 ? want[k] : kGhostCanary;
            if (got != w) {
              std::printf("FAIL ghost: batch %zu (max_len %u, map_len %u), read %u of %u bases, encoding %d, word %u of the bit string: %016llx, expected %016llx (first differing position %d)\n", bi, b.max_len, b.map_len,
                          r, L, e, k, (unsigned long long)got, (unsigned long long)w, static_cast<int>(64 * k) + __builtin_ctzll(got ^ w));
              return 1;
            }
            ++compared;
          }
        }
        ++wi;
      }
      gb.take(reads[r], b.map_len);
      if (b.lens[r] >= b.map_len) for (u32 k = 0; k < b.lens[r]; ++k) writer[k] = static_cast<int>(r);
    }
    free_reads(a); HIPCHK(hipFree(d_which)); HIPCHK(hipFree(d_word0)); HIPCHK(hipFree(d_out));
  }
  const bool ok = compared && zero_fill && past_max && from_donor && donor_back[0] && donor_back[1] && donor_back[2] && donor_back[3] && no_donor && layered && short_between;
  std::printf("%s ghost reads=%ld words_compared=%ld letters_from_donors=%ld donor_1_back=%ld donor_64_back=%ld donor_65_back=%ld donor_150_back=%ld zero_fill_letters=%ld of_them_at_or_past_max_len=%ld reads_without_donor=%ld "
              "reads_with_several_donors=%ld short_reads_between=%ld; %.2f s\n", ok ? "OK" : "FAIL coverage:", reads_checked, compared, from_donor, donor_back[0], donor_back[1], donor_back[2], donor_back[3], zero_fill, past_max,
              no_donor, layered, short_between, now_s() - t0);
  return ok ? 0 : 1;
}

int main(int argc, char **argv) {
  if (argc < 2) { std::printf("FAIL usage: filter_check masks|distance|step|replay|ghost\n"); return 2; }
  const std::string cmd = argv[1];
  if (cmd == "masks") return cmd_masks();
  if (cmd == "distance") return cmd_distance();
  if (cmd == "step") return cmd_step();
  if (cmd == "replay") return cmd_replay();
  if (cmd == "ghost") return cmd_ghost();
  std::printf("FAIL unknown sub-command %s\n", cmd.c_str());
  return 2;
}
