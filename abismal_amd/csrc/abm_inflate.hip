// abismal_amd: BGZF blocks inflated on the device -- inflate_bgzf_kernel and its launch layer (abm_inflater, the C ABI's
// abm_bgzf_scan / abm_inflate_bgzf / abm_inflate_bgzf_device).  The decoder itself is abm_inflate_core.hpp.
#include "../../include/abismal_amd.h"
#include "abm_device.hpp"
#include "abm_inflate_core.hpp"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>

namespace abm { void set_last_error(const std::string &what); }  // abm_api.hip
namespace abm { int resident_waves(const void *kernel, size_t lds, int per_cu_cap); }  // abm_kernels.hip: the one occupancy query

namespace {

using namespace abm_inflate;
using abm::lane_id;
using abm::rdlane;
using abm::wave_sync;

// One wavefront per block, blocks taken in a grid-stride loop.  A block's bit stream is serial and its bytes are not:
// lane 0 runs the core's round() -- up to 64 tokens from a 2 KB window of the stream that the wave stages in LDS -- and
// the wave executes them: a prefix sum of the token lengths places every token, the literals go out in one pass (one lane
// per byte), the matches are copied one after the other by all lanes (a match may read what an earlier token of the same
// round wrote; a copy with dist < len replicates its period: byte k comes from k mod dist), then a stored run, if the round
// ended in one, straight from the block.  The output window is the block's own text in device memory.  Every bounds check
// was made by round() when it emitted the token; the wave only executes.  4.9 KB of LDS per wave.
struct WaveLds {
  Tables t;
  State s;
  u32 tok[kMaxTok];
  u32 n_tok, copy_src, copy_len;
  u8 win[kWindow];
};

__device__ u32 inflate_one(const u8 *__restrict__ in, u32 len, u8 *out, u32 text_len, WaveLds &w) {
  const u32 lane = static_cast<u32>(lane_id());
  if (len > kMaxBlock) return ABM_INFLATE_HEADER;
  if (text_len > kMaxBlock) return ABM_INFLATE_SIZE;
  u32 total = 0, data_off = 0;
  const u32 hs = parse_header(in, len, total, data_off);  // (every lane the same)
  if (hs != ABM_INFLATE_OK) return hs;
  if (total != len) return ABM_INFLATE_HEADER;
  if (lane == 0) start(w.s, data_off, len, text_len);
  wave_sync();
  const u32 end = len - 8;
  u32 at = 0;  // text written so far
  for (;;) {
    // a new window where the reader stands, once the one it has is spent (whole bytes in its buffer go back to the stream
    // first): 2 KB serve about a dozen rounds
    const u32 pos0 = w.s.b.pos, bits0 = w.s.b.n, phase0 = w.s.phase;
    const bool stage = window_spent(w.s.b);
    const u32 base = pos0 - (bits0 >> 3), n_win = min(end - base, kWindow);
    if (stage)
      for (u32 k = lane; k < n_win; k += 64) w.win[k] = in[base + k];
    wave_sync();
    if (lane == 0) {
      State s = w.s;
      if (stage) {
        unread_bytes(s.b);
        place_window(s, w.win, base, n_win);
      }
      u32 n_tok, copy_src, copy_len;
      round(s, w.t, w.tok, n_tok, copy_src, copy_len);
      w.s = s;
      w.n_tok = n_tok;
      w.copy_src = copy_src;
      w.copy_len = copy_len;
    }
    wave_sync();
    const u32 n_tok = w.n_tok, copy_src = w.copy_src, copy_len = w.copy_len, phase = w.s.phase;
    // a round that changed nothing would repeat for ever (the core's window sizes rule it out)
    if (n_tok == 0 && copy_len == 0 && phase == phase0 && w.s.b.pos * 8 - w.s.b.n == pos0 * 8 - bits0) return ABM_INFLATE_DATA;
    const u32 tk = lane < n_tok ? w.tok[lane] : 0u;
    const u32 dist = tk >> 9, l = lane < n_tok ? (dist ? (tk & 511u) : 1u) : 0u;
    u32 sum;
    const u32 p = at + abm::wave_excl_sum(l, sum);
    if (lane < n_tok && !dist) out[p] = static_cast<u8>(tk);
    unsigned long long matches = __ballot(dist != 0);
    // stores of this wave that a later load of it may meet are ordered by a fence; a match needs one only if it reads
    // bytes written since the last one (FASTQ's matches mostly reach far behind the round's own output)
    u32 dirty_from = matches ? at : 0xFFFFFFFFu;  // (the literals of this round)
    while (matches) {
      const int i = __builtin_ctzll(matches);
      matches &= matches - 1;
      const u32 L = rdlane(l, i), D = rdlane(dist, i), P = rdlane(p, i);
      if (P - D + min(L, D) > dirty_from) { wave_sync(); dirty_from = 0xFFFFFFFFu; }
      if (D >= L) { for (u32 k = lane; k < L; k += 64) out[P + k] = out[P - D + k]; }
      else { for (u32 k = lane; k < L; k += 64) out[P + k] = out[P - D + (k % D)]; }
      dirty_from = min(dirty_from, P);
    }
    at += sum;
    for (u32 k = lane; k < copy_len; k += 64) out[at + k] = in[copy_src + k];
    at += copy_len;
    wave_sync();
    if (phase == kPhaseFailed) return w.s.status;
    if (phase == kPhaseDone) break;
  }
  // CRC-32 of the text in 64 pieces, one per lane, combined by the shift operator (abm_inflate_core.hpp)
  const u32 piece = (text_len + 63) / 64;
  const u32 lo = min(lane * piece, text_len), hi = min(lo + piece, text_len);
  u32 r = lane == 0 ? 0xFFFFFFFFu : 0u;
  for (u32 k = lo; k < hi; ++k) r = crc_byte(r, out[k]);
  u32 crc = crc_shift(r, text_len - hi);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) crc ^= __shfl_xor(crc, d);
  return check_trailer(in, len, w.s.out, text_len, ~crc);
}

__global__ __launch_bounds__(64, 4) void inflate_bgzf_kernel(const u8 *__restrict__ comp, u64 comp_bytes, const abm_bgzf_block *__restrict__ blocks,
                                                          u32 n_blocks, u8 *text, u64 text_bytes, u8 *status) {
  __shared__ WaveLds w;
  for (u32 b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const abm_bgzf_block d = blocks[b];
    // (the host entry point refused such a descriptor before the launch; the device one cannot look)
    const bool inside = d.at <= comp_bytes && d.len <= comp_bytes - d.at && d.text_at <= text_bytes && d.text_len <= text_bytes - d.text_at;
    const u32 st = inside ? inflate_one(comp + d.at, d.len, text + d.text_at, d.text_len, w) : static_cast<u32>(ABM_INFLATE_HEADER);
    if (lane_id() == 0) status[b] = static_cast<u8>(st);
    wave_sync();
  }
}

void hip_check(hipError_t e, const char *what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
#define HIPCHK(x) hip_check((x), #x)

template <class F> int guarded(F &&f) {
  try { return f(); }
  catch (const std::exception &e) { abm::set_last_error(e.what()); return -1; }
  catch (...) { abm::set_last_error("unknown error"); return -1; }
}

// grow-only allocations, freed with their owner (as abm_api.hip's)
struct DevBytes {
  u8 *p = nullptr;
  size_t cap = 0;
  DevBytes() = default;
  DevBytes(const DevBytes &) = delete;
  DevBytes &operator=(const DevBytes &) = delete;
  ~DevBytes() { if (p) (void)hipFree(p); }
  void reserve(size_t n) {
    if (n <= cap) return;
    if (p) HIPCHK(hipFree(p));
    p = nullptr; cap = 0;
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&p), n));
    cap = n;
  }
};
struct PinnedBytes {
  u8 *p = nullptr;
  size_t cap = 0;
  PinnedBytes() = default;
  PinnedBytes(const PinnedBytes &) = delete;
  PinnedBytes &operator=(const PinnedBytes &) = delete;
  ~PinnedBytes() { if (p) (void)hipHostFree(p); }
  void reserve(size_t n) {
    if (n <= cap) return;
    if (p) HIPCHK(hipHostFree(p));
    p = nullptr; cap = 0;
    HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&p), n, hipHostMallocPortable));
    cap = n;
  }
};
size_t grown(size_t n) { return std::max<size_t>(n + n / 4, 1u << 16); }

}  // namespace

// One owner per buffer: the inflater owns its stream, its device buffers (compressed bytes, descriptors, text, statuses)
// and its pinned staging; nothing of it is shared with an abm_ctx or with another inflater.
struct abm_inflater {
  int device = 0;
  u32 max_waves = 0;  // grid: the waves the device holds at once (registers allow 16 per CU); further blocks by the grid-stride loop
  hipStream_t stream = nullptr;
  DevBytes d_comp, d_blocks, d_text, d_status;
  PinnedBytes h_comp, h_blocks, h_text, h_status;
  std::mutex mu;
  ~abm_inflater() { if (stream) (void)hipStreamDestroy(stream); }
  void launch(const void *d_c, u64 comp_bytes, const abm_bgzf_block *d_b, u32 n_blocks, void *d_t, u64 text_bytes, u8 *d_s, hipStream_t on) {
    if (!n_blocks) return;
    const u32 grid = std::min(n_blocks, max_waves);
    hipLaunchKernelGGL(inflate_bgzf_kernel, dim3(grid), dim3(64), 0, on, static_cast<const u8 *>(d_c), comp_bytes, d_b, n_blocks,
                       static_cast<u8 *>(d_t), text_bytes, d_s);
    HIPCHK(hipGetLastError());
  }
};

extern "C" {

int abm_bgzf_scan(const void *comp, uint64_t bytes, abm_bgzf_block *out, uint64_t capacity, uint64_t *n_blocks, uint64_t *text_bytes) {
  return guarded([&]() -> int {
    if ((!comp && bytes) || !n_blocks || !text_bytes || (!out && capacity)) throw std::runtime_error("abm_bgzf_scan: null argument");
    const u8 *p = static_cast<const u8 *>(comp);
    u64 at = 0, text = 0, n = 0;
    while (at < bytes) {
      u32 total = 0, data_off = 0;
      if (parse_header(p + at, bytes - at, total, data_off) != ABM_INFLATE_OK)
        throw std::runtime_error("abm_bgzf_scan: not a BGZF block header, or the data ends inside it, at byte " + std::to_string(at));
      if (total > bytes - at) throw std::runtime_error("abm_bgzf_scan: the data ends inside the block at byte " + std::to_string(at));
      const u32 isize = le32(p + at + total - 4);
      if (isize > kMaxBlock) throw std::runtime_error("abm_bgzf_scan: a text of more than 65536 bytes in the block at byte " + std::to_string(at));
      if (n < capacity) out[n] = abm_bgzf_block{at, text, total, isize};
      ++n;
      text += isize;
      at += total;
    }
    *n_blocks = n;
    *text_bytes = text;
    if (n > capacity && out) { abm::set_last_error("abm_bgzf_scan: more blocks than the capacity given"); return ABM_ERR_CAPACITY; }
    return 0;
  });
}

int abm_inflater_create(int device, abm_inflater **out) {
  return guarded([&]() -> int {
    if (!out) throw std::runtime_error("abm_inflater_create: null argument");
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) throw std::runtime_error("abm_inflater_create: no HIP device (the library has no CPU fallback)");
    if (device < 0 || device >= n_dev) throw std::runtime_error("abm_inflater_create: no such device: " + std::to_string(device));
    HIPCHK(hipSetDevice(device));
    abm_inflater *inf = new abm_inflater;
    try {
      inf->device = device;
      hipDeviceProp_t prop;
      HIPCHK(hipGetDeviceProperties(&prop, device));
      // (at least one wave per CU, whatever the query answers)
      const int waves = abm::resident_waves(reinterpret_cast<const void *>(inflate_bgzf_kernel), 0, 1 << 20);
      inf->max_waves = static_cast<u32>(std::max({1, prop.multiProcessorCount, waves}));
      HIPCHK(hipStreamCreateWithFlags(&inf->stream, hipStreamNonBlocking));
    }
    catch (...) { delete inf; throw; }
    *out = inf;
    return 0;
  });
}

void abm_inflater_destroy(abm_inflater *inf) {
  if (!inf) return;
  (void)hipSetDevice(inf->device);
  if (inf->stream) (void)hipStreamSynchronize(inf->stream);
  delete inf;
}

int abm_inflate_bgzf(abm_inflater *inf, const void *comp, uint64_t comp_bytes, const abm_bgzf_block *blocks, uint32_t n_blocks, void *text,
                     uint64_t text_bytes, uint8_t *status) {
  return guarded([&]() -> int {
    if ((!comp && comp_bytes) || (!blocks && n_blocks) || (!text && text_bytes) || (!status && n_blocks))
      throw std::runtime_error("abm_inflate_bgzf: null argument");
    // every descriptor, before anything is launched; and the span of the buffers the blocks use
    u64 c_lo = comp_bytes, c_hi = 0, t_lo = text_bytes, t_hi = 0;
    for (u32 b = 0; b < n_blocks; ++b) {
      const abm_bgzf_block &d = blocks[b];
      if (d.at > comp_bytes || d.len > comp_bytes - d.at)
        throw std::runtime_error("abm_inflate_bgzf: block " + std::to_string(b) + " lies outside the compressed bytes given");
      if (d.text_at > text_bytes || d.text_len > text_bytes - d.text_at)
        throw std::runtime_error("abm_inflate_bgzf: the text of block " + std::to_string(b) + " lies outside the text buffer given");
      c_lo = std::min(c_lo, d.at); c_hi = std::max(c_hi, d.at + d.len);
      t_lo = std::min(t_lo, d.text_at); t_hi = std::max(t_hi, d.text_at + d.text_len);
    }
    if (!inf) throw std::runtime_error("abm_inflate_bgzf: null inflater");
    if (!n_blocks) return 0;
    if (c_hi < c_lo) c_hi = c_lo;
    if (t_hi < t_lo) t_hi = t_lo;
    std::lock_guard<std::mutex> lk(inf->mu);
    HIPCHK(hipSetDevice(inf->device));
    const u64 c_n = c_hi - c_lo, t_n = t_hi - t_lo;
    const size_t b_n = static_cast<size_t>(n_blocks) * sizeof(abm_bgzf_block);
    inf->d_comp.reserve(grown(c_n)); inf->h_comp.reserve(grown(c_n));
    inf->d_blocks.reserve(grown(b_n)); inf->h_blocks.reserve(grown(b_n));
    inf->d_text.reserve(grown(t_n)); inf->h_text.reserve(grown(t_n));
    inf->d_status.reserve(grown(n_blocks)); inf->h_status.reserve(grown(n_blocks));
    // (the device sees the spans, so the descriptors move with them)
    std::memcpy(inf->h_comp.p, static_cast<const u8 *>(comp) + c_lo, c_n);
    abm_bgzf_block *hb = reinterpret_cast<abm_bgzf_block *>(inf->h_blocks.p);
    for (u32 b = 0; b < n_blocks; ++b) hb[b] = abm_bgzf_block{blocks[b].at - c_lo, blocks[b].text_at - t_lo, blocks[b].len, blocks[b].text_len};
    hipStream_t st = inf->stream;
    if (c_n) HIPCHK(hipMemcpyAsync(inf->d_comp.p, inf->h_comp.p, c_n, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(inf->d_blocks.p, inf->h_blocks.p, b_n, hipMemcpyHostToDevice, st));
    inf->launch(inf->d_comp.p, c_n, reinterpret_cast<const abm_bgzf_block *>(inf->d_blocks.p), n_blocks, inf->d_text.p, t_n, inf->d_status.p, st);
    if (t_n) HIPCHK(hipMemcpyAsync(inf->h_text.p, inf->d_text.p, t_n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(inf->h_status.p, inf->d_status.p, n_blocks, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // only the blocks' own ranges of `text` are written
    bool all_ok = true;
    for (u32 b = 0; b < n_blocks; ++b) {
      status[b] = inf->h_status.p[b];
      all_ok &= status[b] == ABM_INFLATE_OK;
      if (blocks[b].text_len) std::memcpy(static_cast<u8 *>(text) + blocks[b].text_at, inf->h_text.p + hb[b].text_at, blocks[b].text_len);
    }
    if (!all_ok) { abm::set_last_error("abm_inflate_bgzf: a block did not inflate (see its status)"); return ABM_ERR_INFLATE; }
    return 0;
  });
}

int abm_inflate_bgzf_device(abm_inflater *inf, const void *d_comp, uint64_t comp_bytes, const abm_bgzf_block *d_blocks, uint32_t n_blocks,
                            void *d_text, uint64_t text_bytes, uint8_t *d_status, void *stream) {
  return guarded([&]() -> int {
    if (!inf || (!d_comp && comp_bytes) || (!d_blocks && n_blocks) || (!d_text && text_bytes) || (!d_status && n_blocks))
      throw std::runtime_error("abm_inflate_bgzf_device: null argument");
    HIPCHK(hipSetDevice(inf->device));
    inf->launch(d_comp, comp_bytes, d_blocks, n_blocks, d_text, text_bytes, d_status, static_cast<hipStream_t>(stream));
    return 0;
  });
}

}  // extern "C"
