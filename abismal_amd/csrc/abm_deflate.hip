// abismal_amd: text deflated into BGZF blocks on the device -- deflate_bgzf_kernel, pack_bgzf_kernel and their launch
// layer (abm_deflater, the C ABI's abm_deflate_bgzf / abm_deflate_bgzf_device), and the same encoder run serially on the
// host (abm_deflate_bgzf_host).  The encoder itself is abm_deflate_core.hpp.
#include "../../include/abismal_amd.h"
#include "abm_deflate_core.hpp"
#include "abm_device.hpp"

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>

namespace abm { void set_last_error(const std::string &what); }  // abm_api.hip
namespace abm { int resident_waves(const void *kernel, size_t lds, int per_cu_cap); }  // abm_kernels.hip: the one occupancy query

namespace {

using namespace abm_deflate;
using abm::lane_id;
using abm::wave_sync;

// The scratch bytes a member of a call cut every block_bytes is encoded into: what the longest member takes (the stored
// form), a multiple of 4 so that every member's stream starts where the one before it did, modulo 4.
__host__ __device__ inline u32 slot_bytes(u32 block_bytes) { return (block_bytes + kHeader + kStoredExtra + kTrailer + 3u) & ~3u; }

// One wavefront per block of text, blocks taken in a grid-stride loop: the core's phases on all 64 lanes, a wave_sync()
// between them.  The wave's LDS is the core's Shared (16.6 KB, static: the launcher's occupancy query sees it), the text
// is read from and the stream written to device memory.  Returns the member's length (every lane the same).
__device__ u32 deflate_one(const u8 *__restrict__ text, u32 n, u8 *__restrict__ member, Shared &sh) {
  const u32 lane = static_cast<u32>(lane_id());
  u8 *stream = member + kHeader;
  u32 crc = crc_piece(lane, text, n);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) crc ^= __shfl_xor(crc, d);
  crc = ~crc;
  bool stored = n == 0;
  u32 bits = 3, words = 0;
  if (!stored) {
    u32 *table_words = reinterpret_cast<u32 *>(sh.table);
    for (u32 k = lane; k < (1u << kHashBits) / 2; k += kLanes) table_words[k] = 0;
    for (u32 k = lane; k < kStageWords; k += kLanes) sh.stage[k] = k == 0 ? 3u : 0u;
    wave_sync();
    u32 next = 0;
    for (u32 r0 = 0; r0 < n; r0 += kLanes) {
      if (next >= r0 + kLanes) continue;
      const u32 i = r0 + lane;
      Lane l;
      probe(l, sh, text, n, i);
      wave_sync();  // (every lane has the entry from before the round)
      for (;;) {
        const bool wrote = enter_once(l, sh, i);
        wave_sync();
        if (!__ballot(wrote)) break;
      }
      measure(l, sh, lane, text, n, i);
      const u64 matches = __ballot(l.len != 0);
      wave_sync();
      u32 rel = 0;
      u64 on = walk(sh, matches, next - r0, rel);
      if (n - r0 < kLanes) on &= ~(~0ull << (n - r0));
      next = r0 + rel;
      u32 tok = 0, tok_bits = 0;
      if (on >> lane & 1u) tok = token(l, text[i], tok_bits);
      u32 sum;
      const u32 before = abm::wave_excl_sum(tok_bits, sum);
      if (would_overflow(bits + sum, n)) { stored = true; break; }
      place(sh, bits - 32 * words + before, tok, tok_bits);
      wave_sync();
      bits += sum;
      const u32 whole = bits / 32 - words;  // <= 62
      const u32 mine = sh.stage[lane], carry = sh.stage[whole];
      if (lane < whole) __builtin_memcpy(stream + 4 * (words + lane), &mine, 4);
      wave_sync();
      sh.stage[lane] = lane == 0 ? carry : 0u;
      if (lane < kStageWords - kLanes) sh.stage[kLanes + lane] = 0;
      wave_sync();
      words += whole;
    }
  }
  if (stored) {
    if (lane == 0) stored_header(stream, n);
    for (u32 k = lane; k < n; k += kLanes) stream[kStoredExtra + k] = text[k];
    if (lane == 0) frame(member, kStoredExtra + n, crc, n);
    return kHeader + kStoredExtra + n + kTrailer;
  }
  bits += 7;
  const u32 stream_bytes = (bits + 7) / 8;
  for (u32 k = 4 * words + lane; k < stream_bytes; k += kLanes) stream[k] = static_cast<u8>(sh.stage[(k - 4 * words) >> 2] >> (8 * (k & 3u)));
  if (lane == 0) frame(member, stream_bytes, crc, n);
  return kHeader + stream_bytes + kTrailer;
}

__global__ __launch_bounds__(64) void deflate_bgzf_kernel(const u8 *__restrict__ text, u64 text_bytes, u32 block_bytes, u32 n_blocks,
                                                          u8 *__restrict__ scratch, u32 *__restrict__ lens) {
  __shared__ Shared sh;
  const u32 slot = slot_bytes(block_bytes);
  for (u32 b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const u64 at = static_cast<u64>(b) * block_bytes;
    const u32 n = static_cast<u32>(min(static_cast<u64>(block_bytes), text_bytes - at));
    const u32 len = deflate_one(text + at, n, scratch + static_cast<u64>(b) * slot, sh);
    if (lane_id() == 0) lens[b] = len;
    wave_sync();
  }
}

// The members end to end: workgroup b sums the lengths before its member (from where its previous member stood, in the
// grid-stride loop), moves the member from its slot to out + that, bytes at or beyond `capacity` left out, and fills in
// its descriptor; the last member's workgroup writes the total, clipped or not.
constexpr u32 kPackThreads = 256;
__global__ __launch_bounds__(kPackThreads) void pack_bgzf_kernel(const u8 *__restrict__ scratch, const u32 *__restrict__ lens, u32 n_blocks,
                                                                 u64 text_bytes, u32 block_bytes, u8 *__restrict__ out, u64 capacity,
                                                                 abm_bgzf_block *__restrict__ blocks, u64 *__restrict__ total) {
  __shared__ u64 part[kPackThreads];
  const u32 tid = threadIdx.x, slot = slot_bytes(block_bytes);
  u64 off = 0;
  u32 prev = 0;
  for (u32 b = blockIdx.x; b < n_blocks; prev = b, b += gridDim.x) {
    u64 s = 0;
    for (u32 k = prev + tid; k < b; k += kPackThreads) s += lens[k];
    part[tid] = s;
    __syncthreads();
    for (u32 d = kPackThreads / 2; d >= 1; d >>= 1) {
      if (tid < d) part[tid] += part[tid + d];
      __syncthreads();
    }
    off += part[0];
    __syncthreads();
    const u32 len = lens[b];
    const u8 *src = scratch + static_cast<u64>(b) * slot;
    const u32 m = off < capacity ? static_cast<u32>(min(static_cast<u64>(len), capacity - off)) : 0u;
    u8 *dst = out + off;
    // bytes up to dst's first whole word, whole words (the source is read unaligned), the bytes after them
    const u32 head = min(m, static_cast<u32>((4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u)), n_words = (m - head) / 4;
    if (tid < head) dst[tid] = src[tid];
    for (u32 k = tid; k < n_words; k += kPackThreads) *reinterpret_cast<u32 *>(dst + head + 4 * k) = load32(src + head + 4 * k);
    const u32 done = head + 4 * n_words;
    if (tid < m - done) dst[done + tid] = src[done + tid];
    if (tid == 0) {
      const u64 text_at = static_cast<u64>(b) * block_bytes;
      if (blocks) blocks[b] = abm_bgzf_block{off, text_at, len, static_cast<u32>(min(static_cast<u64>(block_bytes), text_bytes - text_at))};
      if (b == n_blocks - 1) *total = off + len;
    }
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

// grow-only allocations, freed with their owner (as abm_inflate.hip's)
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

// block_bytes as the entry points take it: 0 = kMaxText; above kMaxText is refused
u32 checked_block_bytes(const char *who, u32 block_bytes) {
  if (block_bytes > kMaxText) throw std::runtime_error(std::string(who) + ": block_bytes above 0xff00");
  return block_bytes ? block_bytes : kMaxText;
}
u32 checked_n_blocks(const char *who, u64 text_bytes, u32 bb) {
  const u64 n = n_blocks_of(text_bytes, bb);
  if (n > 0x7FFFFFFFull) throw std::runtime_error(std::string(who) + ": more than 2^31 - 1 blocks in one call");
  return static_cast<u32>(n);
}

}  // namespace

// One owner per buffer: the deflater owns its stream, its device buffers (text, the members' slots and lengths, the packed
// output, descriptors, the total) and its pinned staging; nothing of it is shared with an abm_ctx, an inflater or another
// deflater.
struct abm_deflater {
  int device = 0;
  u32 max_waves = 0;  // grid: the waves the device holds at once (LDS allows nine per CU); further blocks by the grid-stride loop
  hipStream_t stream = nullptr;
  DevBytes d_text, d_scratch, d_lens, d_out, d_blocks, d_total;
  PinnedBytes h_text, h_out, h_blocks, h_total;
  std::mutex mu;
  ~abm_deflater() { if (stream) (void)hipStreamDestroy(stream); }
  // (under mu) both kernels on `on`; the scratch is this deflater's
  void launch(const void *d_t, u64 text_bytes, u32 bb, u32 n_blocks, void *d_o, u64 capacity, u64 *d_n, abm_bgzf_block *d_b, hipStream_t on) {
    if (!n_blocks) { HIPCHK(hipMemsetAsync(d_n, 0, sizeof(u64), on)); return; }
    d_scratch.reserve(grown(static_cast<size_t>(n_blocks) * slot_bytes(bb)));
    d_lens.reserve(grown(static_cast<size_t>(n_blocks) * sizeof(u32)));
    const u32 grid = std::min(n_blocks, max_waves);
    hipLaunchKernelGGL(deflate_bgzf_kernel, dim3(grid), dim3(64), 0, on, static_cast<const u8 *>(d_t), text_bytes, bb, n_blocks, d_scratch.p,
                       reinterpret_cast<u32 *>(d_lens.p));
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(pack_bgzf_kernel, dim3(grid), dim3(kPackThreads), 0, on, d_scratch.p, reinterpret_cast<const u32 *>(d_lens.p), n_blocks,
                       text_bytes, bb, static_cast<u8 *>(d_o), capacity, d_b, d_n);
    HIPCHK(hipGetLastError());
  }
};

extern "C" {

uint64_t abm_deflate_bgzf_bound(uint64_t text_bytes, uint32_t block_bytes) {
  if (block_bytes > kMaxText) { abm::set_last_error("abm_deflate_bgzf_bound: block_bytes above 0xff00"); return 0; }
  return bound_of(text_bytes, block_bytes ? block_bytes : kMaxText);
}

int abm_deflater_create(int device, abm_deflater **out) {
  return guarded([&]() -> int {
    if (!out) throw std::runtime_error("abm_deflater_create: null argument");
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) throw std::runtime_error("abm_deflater_create: no HIP device (abm_deflate_bgzf_host runs the same encoder on the CPU)");
    if (device < 0 || device >= n_dev) throw std::runtime_error("abm_deflater_create: no such device: " + std::to_string(device));
    HIPCHK(hipSetDevice(device));
    abm_deflater *def = new abm_deflater;
    try {
      def->device = device;
      hipDeviceProp_t prop;
      HIPCHK(hipGetDeviceProperties(&prop, device));
      // (at least one wave per CU, whatever the query answers)
      const int waves = abm::resident_waves(reinterpret_cast<const void *>(deflate_bgzf_kernel), 0, 1 << 20);
      def->max_waves = static_cast<u32>(std::max({1, prop.multiProcessorCount, waves}));
      HIPCHK(hipStreamCreateWithFlags(&def->stream, hipStreamNonBlocking));
      def->d_total.reserve(sizeof(u64));
      def->h_total.reserve(sizeof(u64));
    }
    catch (...) { delete def; throw; }
    *out = def;
    return 0;
  });
}

void abm_deflater_destroy(abm_deflater *def) {
  if (!def) return;
  (void)hipSetDevice(def->device);
  if (def->stream) (void)hipStreamSynchronize(def->stream);
  delete def;
}

int abm_deflate_bgzf(abm_deflater *def, const void *text, uint64_t text_bytes, uint32_t block_bytes, void *out, uint64_t out_capacity,
                     uint64_t *out_bytes, abm_bgzf_block *blocks, uint64_t blocks_capacity, uint64_t *n_blocks) {
  return guarded([&]() -> int {
    if ((!text && text_bytes) || (!out && out_capacity) || !out_bytes || !n_blocks || (!blocks && blocks_capacity))
      throw std::runtime_error("abm_deflate_bgzf: null argument");
    const u32 bb = checked_block_bytes("abm_deflate_bgzf", block_bytes);
    const u32 nb = checked_n_blocks("abm_deflate_bgzf", text_bytes, bb);
    if (!def) throw std::runtime_error("abm_deflate_bgzf: null deflater");
    *n_blocks = nb;
    *out_bytes = 0;
    if (!nb) return 0;
    std::lock_guard<std::mutex> lk(def->mu);
    HIPCHK(hipSetDevice(def->device));
    const u64 bound = bound_of(text_bytes, bb);
    const size_t b_n = static_cast<size_t>(nb) * sizeof(abm_bgzf_block);
    def->d_text.reserve(grown(text_bytes)); def->h_text.reserve(grown(text_bytes));
    def->d_out.reserve(grown(bound)); def->h_out.reserve(grown(bound));
    def->d_blocks.reserve(grown(b_n)); def->h_blocks.reserve(grown(b_n));
    std::memcpy(def->h_text.p, text, text_bytes);
    hipStream_t st = def->stream;
    HIPCHK(hipMemcpyAsync(def->d_text.p, def->h_text.p, text_bytes, hipMemcpyHostToDevice, st));
    def->launch(def->d_text.p, text_bytes, bb, nb, def->d_out.p, bound, reinterpret_cast<u64 *>(def->d_total.p),
                reinterpret_cast<abm_bgzf_block *>(def->d_blocks.p), st);
    HIPCHK(hipMemcpyAsync(def->h_total.p, def->d_total.p, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(def->h_blocks.p, def->d_blocks.p, b_n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    u64 total = 0;
    std::memcpy(&total, def->h_total.p, sizeof(u64));
    if (total > bound) throw std::runtime_error("abm_deflate_bgzf: the members are longer than their bound");
    *out_bytes = total;
    if (total > out_capacity || (blocks && nb > blocks_capacity)) {
      abm::set_last_error(total > out_capacity ? "abm_deflate_bgzf: the members need more bytes than out_capacity"
                                               : "abm_deflate_bgzf: more members than blocks_capacity");
      return ABM_ERR_CAPACITY;
    }
    HIPCHK(hipMemcpyAsync(def->h_out.p, def->d_out.p, total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::memcpy(out, def->h_out.p, total);
    if (blocks) std::memcpy(blocks, def->h_blocks.p, b_n);
    return 0;
  });
}

int abm_deflate_bgzf_device(abm_deflater *def, const void *d_text, uint64_t text_bytes, uint32_t block_bytes, void *d_out, uint64_t out_capacity,
                            uint64_t *d_out_bytes, abm_bgzf_block *d_blocks, void *stream) {
  return guarded([&]() -> int {
    if (!def || (!d_text && text_bytes) || (!d_out && out_capacity) || !d_out_bytes || (!d_blocks && text_bytes))
      throw std::runtime_error("abm_deflate_bgzf_device: null argument");
    const u32 bb = checked_block_bytes("abm_deflate_bgzf_device", block_bytes);
    const u32 nb = checked_n_blocks("abm_deflate_bgzf_device", text_bytes, bb);
    std::lock_guard<std::mutex> lk(def->mu);
    HIPCHK(hipSetDevice(def->device));
    def->launch(d_text, text_bytes, bb, nb, d_out, out_capacity, d_out_bytes, d_blocks, static_cast<hipStream_t>(stream));
    return 0;
  });
}

int abm_deflate_bgzf_host(const void *text, uint64_t text_bytes, uint32_t block_bytes, void *out, uint64_t out_capacity, uint64_t *out_bytes,
                          abm_bgzf_block *blocks, uint64_t blocks_capacity, uint64_t *n_blocks) {
  return guarded([&]() -> int {
    if ((!text && text_bytes) || (!out && out_capacity) || !out_bytes || !n_blocks || (!blocks && blocks_capacity))
      throw std::runtime_error("abm_deflate_bgzf_host: null argument");
    const u32 bb = checked_block_bytes("abm_deflate_bgzf_host", block_bytes);
    const u32 nb = checked_n_blocks("abm_deflate_bgzf_host", text_bytes, bb);
    // (everything is encoded before anything is written: a call that does not fit writes nothing)
    std::unique_ptr<Shared> sh(new Shared);
    std::unique_ptr<u8[]> all(new u8[bound_of(text_bytes, bb) + 1]);
    std::unique_ptr<abm_bgzf_block[]> desc(new abm_bgzf_block[nb + 1]);
    u64 total = 0;
    for (u32 b = 0; b < nb; ++b) {
      const u64 at = static_cast<u64>(b) * bb;
      const u32 n = static_cast<u32>(std::min<u64>(bb, text_bytes - at));
      const u32 len = deflate_member(static_cast<const u8 *>(text) + at, n, all.get() + total, *sh);
      desc[b] = abm_bgzf_block{total, at, len, n};
      total += len;
    }
    *n_blocks = nb;
    *out_bytes = total;
    if (total > out_capacity || (blocks && nb > blocks_capacity)) {
      abm::set_last_error(total > out_capacity ? "abm_deflate_bgzf_host: the members need more bytes than out_capacity"
                                               : "abm_deflate_bgzf_host: more members than blocks_capacity");
      return ABM_ERR_CAPACITY;
    }
    if (total) std::memcpy(out, all.get(), total);
    if (blocks && nb) std::memcpy(blocks, desc.get(), static_cast<size_t>(nb) * sizeof(abm_bgzf_block));
    return 0;
  });
}

}  // extern "C"
