// GPU test program (built and run by tests/test_gpu_lds_layout.py): the carve functions the mapping kernels call
// (se_carve, pe_carve) against the host-side layouts of abm_lds_layout.hpp.  One wave per form, launched with the layout's
// bytes of dynamic LDS: the kernel carves, reports where every pointer lies inside the allocation (or that it does not),
// fills every region over its full extent with the region's own tag, and after a barrier copies the allocation out.  The
// host wants the offsets of its own layout and every byte under its own region's tag: a wrong extent, an overlap or a region
// past the allocation (whose writes are dropped) all leave a wrong tag.  Prints "OK ..." or the first mismatches.
#include "../../abismal_amd/csrc/abm_pe_set.hpp"
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>
using namespace abm;

constexpr int kMaxRegions = 28;
struct Job { u32 bytes; u32 size[kMaxRegions]; };  // size 0: an overlay, an alias or an absent region -- reported, not filled

__device__ void fill_and_copy(unsigned char *smem, unsigned char *const *ptr, int n, const Job &job, u32 *off_out, u8 *image) {
  const u32 lane = threadIdx.x;
  for (u32 i = lane; i < job.bytes; i += 64) smem[i] = 0;
  __syncthreads();
  for (int r = 0; r < n; ++r) {
    const u64 d = reinterpret_cast<u64>(ptr[r]) - reinterpret_cast<u64>(smem);
    const u32 off = d < job.bytes ? static_cast<u32>(d) : kLdsAbsent;  // (a pointer into global memory, or null, is far from LDS)
    if (lane == 0) off_out[r] = off;
    if (off != kLdsAbsent)
      for (u32 i = lane; i < job.size[r]; i += 64) ptr[r][i] = static_cast<u8>(r + 1);
  }
  __syncthreads();
  for (u32 i = lane; i < job.bytes; i += 64) image[i] = smem[i];
}
#define P(x) reinterpret_cast<unsigned char *>(x)

constexpr int kSeRegions = 14;
static const char *const kSeNames[kSeRegions] = {"qpk", "qbits", "qmask", "ctmp", "jpos", "jdf", "gwin", "pcache", "lbest", "smark", "sdelta", "mark", "tb", "hres"};
template <bool LONG> __global__ __launch_bounds__(64) void se_form(SeArgs a, Job job, u32 *off_out, u8 *image) {
  extern __shared__ __align__(16) unsigned char smem[];
  WaveLds lds;
  se_carve<LONG>(lds, smem, a);
  unsigned char *const ptr[kSeRegions] = {P(lds.qpk), P(lds.qbits), P(lds.qmask), P(lds.ctmp), P(lds.jpos), P(lds.jdf), P(lds.gwin),
                                          P(lds.pcache), P(lds.lbest), P(lds.smark), P(lds.sdelta), P(lds.mark), P(lds.tb), P(lds.hres)};
  fill_and_copy(smem, ptr, kSeRegions, job, off_out, image);
}

constexpr int kPeRegions = 25;
static const char *const kPeNames[kPeRegions] = {"qpk", "qbits", "qmask", "gwin", "pcache", "ctmp", "jpos", "jdf", "jidx", "lbest", "heap", "lpos0", "lpos1",
                                                 "ld0", "ld1", "lsc0", "lsc1", "smark", "sdelta", "mark", "fin", "tb", "hres", "tmp", "samp"};
template <bool BIG, bool LONG, int PHASE, bool TEXT> __global__ __launch_bounds__(64) void pe_form(PeArgs a, Job job, u32 *off_out, u8 *image) {
  extern __shared__ __align__(16) unsigned char smem[];
  WaveLds lds;
  PeLds pl;
  u32 *fin, *samp;
  pe_carve<BIG, LONG, PHASE, TEXT>(lds, pl, fin, samp, smem, a);
  unsigned char *const ptr[kPeRegions] = {P(lds.qpk), P(lds.qbits), P(lds.qmask), P(lds.gwin), P(lds.pcache), P(lds.ctmp), P(lds.jpos), P(lds.jdf), P(pl.jidx),
                                          P(lds.lbest), P(pl.heap), P(pl.lpos[0]), P(pl.lpos[1]), P(pl.ld[0]), P(pl.ld[1]), P(pl.lsc[0]), P(pl.lsc[1]),
                                          P(lds.smark), P(lds.sdelta), P(lds.mark), P(fin), P(lds.tb), P(lds.hres), P(pl.tmp), P(samp)};
  fill_and_copy(smem, ptr, kPeRegions, job, off_out, image);
}

#define CHECK(x)                                                                        \
  do {                                                                                  \
    hipError_t e_ = (x);                                                                \
    if (e_ != hipSuccess) { printf("FAIL %s: %s\n", #x, hipGetErrorString(e_)); return 2; } \
  } while (0)

static int n_wrong = 0;
static u32 *d_off;
static u8 *d_image;

// what the kernel left against the host's layout: offsets (in the kernels' order) and the image
static int compare(const std::string &form, const char *const *names, const std::vector<u32> &want_off, const Job &job) {
  const int n = static_cast<int>(want_off.size());
  std::vector<u32> off(n);
  std::vector<u8> image(job.bytes), want(job.bytes, 0);
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(off.data(), d_off, n * sizeof(u32), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(image.data(), d_image, job.bytes, hipMemcpyDeviceToHost));
  for (int r = 0; r < n; ++r) {
    if (off[r] != want_off[r] && ++n_wrong <= 20) printf("WRONG %s: %s at %u, the layout says %u\n", form.c_str(), names[r], off[r], want_off[r]);
    if (want_off[r] != kLdsAbsent)
      for (u32 i = 0; i < job.size[r] && want_off[r] + i < job.bytes; ++i) want[want_off[r] + i] = static_cast<u8>(r + 1);
  }
  for (u32 i = 0; i < job.bytes; ++i)
    if (image[i] != want[i]) {
      if (++n_wrong <= 20) printf("WRONG %s: byte %u carries tag %u (%s), not %u\n", form.c_str(), i, image[i], image[i] ? names[image[i] - 1] : "none", want[i]);
      break;
    }
  return 0;
}

static LdsShape shape_for(u32 L, bool lng) {
  const double frac = 0.1;
  LdsShape s{std::max(1u, (L + 15) / 16), (L + 63) / 64 + 1, se_window_words(L, frac), L, L + 2, 0};
  if (!lng) s.tb_extra = tb_extra_bytes(s.GW, L, frac);
  return s;
}

template <class K, class Args> static int launch(K kernel, const Args &a, const Job &job) {
  if (job.bytes > 160 * 1024) { printf("FAIL a form of %u bytes: more than a CU's LDS\n", job.bytes); return 2; }
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(job.bytes)));
  hipLaunchKernelGGL(kernel, dim3(1), dim3(64), job.bytes, 0, a, job, d_off, d_image);
  CHECK(hipGetLastError());
  return 0;
}

static int run_se(u32 L, bool lng) {
  const LdsShape s = shape_for(L, lng);
  const SeLds<u32> o = se_lds_layout<u32>(0, lng, s);
  SeArgs a{};
  a.W = s.W; a.WB = s.WB; a.GW = s.GW; a.max_len = s.max_len; a.ctmp_cap = s.ctmp_cap; a.tb_extra = s.tb_extra; a.G = 2;
  const u32 MB = lng ? 0u : (L + 63) / 64;
  Job job{o.bytes, {4 * s.W * 8, 4 * s.WB * 8, 4 * MB * 4 * 8, lng ? 0u : ((s.ctmp_cap + 1) & ~1u) * 4, kSeCap * 4, kSeCap * 4, o.slots * s.GW * 8,
                    kCacheBytes + s.tb_extra, 64 * 4, 128 * 4, 128 * 4, 64 * 2, 0, 0}};
  const std::vector<u32> want = {o.qpk, o.qbits, o.qmask, o.ctmp, o.jpos, o.jdf, o.gwin, o.pcache, o.lbest, o.smark, o.sdelta, o.mark, o.tb, o.lbest};
  if (int rc = lng ? launch(se_form<true>, a, job) : launch(se_form<false>, a, job)) return rc;
  return compare("single-end" + std::string(lng ? " long " : " ") + std::to_string(L), kSeNames, want, job);
}

static int run_pe(u32 L, int phase, bool lng, bool big, bool text) {
  const LdsShape s = shape_for(L, lng);
  const u32 cap = big ? kPeCapLarge : kPeTier1Cap;
  const PeLdsAt<u32> o = pe_lds_layout<u32>(0, phase, lng, big, text, s, cap);
  PeArgs a{};
  a.W = s.W; a.WB = s.WB; a.GW = s.GW; a.max_len = s.max_len; a.ctmp_cap = s.ctmp_cap; a.tb_extra = s.tb_extra; a.G = 4; a.cap = cap;
  const bool seed = phase == kSeed, table = !seed && !lng;
  const u32 MB = (L + 63) / 64, list = big ? 0u : cap;
  Job job{o.bytes, {8 * s.W * 8, 8 * s.WB * 8, 8 * MB * 4 * 8, o.slots * s.GW * 8, kCacheBytes + (table ? s.tb_extra : 0u), s.ctmp_cap * 4, kSeCap * 4, kSeCap * 4,
                    kSeCap * 4, 64 * 4, list * 4, list * 4, seed ? 0u : list * 4, seed ? (list + (list & 1u)) * 2 : list * 2, seed ? 0u : list * 2,
                    list * 2, list * 2, 128 * 4, 128 * 4, 64 * 2, kPeFinBytes, 0, 0, 0, 0}};
  const std::vector<u32> want = {o.qpk, o.qbits, o.qmask, o.gwin, o.pcache, o.ctmp, o.jpos, o.jdf, o.jidx, o.lbest, o.heap, o.lpos[0], o.lpos[1],
                                 o.ld[0], o.ld[1], o.lsc[0], o.lsc[1], o.smark, o.sdelta, o.mark, o.fin, o.tb, o.lbest, big ? kLdsAbsent : o.pcache, o.pcache};
  int rc;
  if (lng) rc = launch(pe_form<true, true, kWhole, false>, a, job);
  else if (seed) rc = launch(pe_form<false, false, kSeed, false>, a, job);
  else if (phase == kMate) rc = big ? (text ? launch(pe_form<true, false, kMate, true>, a, job) : launch(pe_form<true, false, kMate, false>, a, job))
                                    : (text ? launch(pe_form<false, false, kMate, true>, a, job) : launch(pe_form<false, false, kMate, false>, a, job));
  else rc = big ? (text ? launch(pe_form<true, false, kWhole, true>, a, job) : launch(pe_form<true, false, kWhole, false>, a, job))
                : (text ? launch(pe_form<false, false, kWhole, true>, a, job) : launch(pe_form<false, false, kWhole, false>, a, job));
  if (rc) return rc;
  const char *const phases[] = {"whole", "seed", "mate"};
  return compare(std::string("pairs ") + (lng ? "long" : phases[phase]) + (big ? " big" : "") + (text ? " text" : "") + " " + std::to_string(L), kPeNames, want, job);
}

int main() {
  CHECK(hipMalloc(&d_off, kMaxRegions * sizeof(u32)));
  CHECK(hipMalloc(&d_image, 160 * 1024));
  int forms = 0;
  for (const u32 L : {44u, 100u, 172u, 1024u}) { if (int rc = run_se(L, false)) return rc; ++forms; }
  if (int rc = run_se(1025, true)) return rc;
  ++forms;
  for (const u32 L : {44u, 150u, 1024u}) {
    for (int text = 0; text < 2; ++text)
      for (int big = 0; big < 2; ++big) {
        if (int rc = run_pe(L, kWhole, false, big, text)) return rc;
        if (int rc = run_pe(L, kMate, false, big, text)) return rc;
        forms += 2;
      }
    if (int rc = run_pe(L, kSeed, false, false, false)) return rc;
    ++forms;
  }
  if (int rc = run_pe(1025, kWhole, true, true, false)) return rc;
  ++forms;
  if (n_wrong) { printf("%d mismatches in %d forms\n", n_wrong, forms); return 1; }
  printf("OK %d forms\n", forms);
  return 0;
}
