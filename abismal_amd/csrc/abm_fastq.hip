// abismal_amd: FASTQ text parsed on the device -- the kernels and their launch layer (abm_fastq_parser, the C ABI's
// abm_fastq_parse / abm_fastq_parse_device / abm_fastq_parse_host).  The rules themselves are abm_fastq_core.hpp.
#include "../../include/abismal_amd.h"
#include "abm_device.hpp"
#include "abm_fastq_core.hpp"

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>

namespace abm { void set_last_error(const std::string &what); }  // abm_api.hip

namespace {

using namespace abm_fastq;

// Six kernels, each bounded by text_bytes, by the record capacity `cap` its launcher sized the scratch arrays with, and by
// blob_capacity:
//   count_newlines   one workgroup per tile of kTileBytes: the tile's newlines
//   scan_tiles       ONE workgroup, kScanTiles counts per step with a running carry: newlines before each tile; the text's
//                    lines and records; whether the records fit `cap` (if not, *info says how many there are and every
//                    later kernel returns at once)
//   mark_lines       one workgroup per tile: every newline's rank is its line's number k; k % 4 says what it ends -- a name
//                    line (name_end, and an empty one is an error), a sequence line (seq_end), a quality line (the next
//                    record's name_at)
//   apply_rules      one workgroup per chunk of kChunkRecords, a group of 16 lanes per record, looping over lines of any
//                    length: the name's length, the read's range, the errors; the chunk's sum and maximum of read lengths
//   scan_chunks      ONE workgroup: the chunks' sums scanned, kScanTiles per step; *info; off[n]
//   copy_reads       one workgroup per chunk: the chunk's read lengths scanned into off[], the reads copied
// Text offsets are u32 (a text of 2^32 bytes or more is refused before any launch); blob offsets are u64.
struct Head {
  u64 n_records;
  u64 err;       // the minimum of error_key(line, code): kNoError = none
  u32 newlines;
  u32 fits;      // n_records <= cap
};
struct Scratch {  // (device pointers: the parser's own arrays)
  Head *head;
  u32 *tile;      // per tile: its newlines, then the newlines before it
  u32 *name_at, *name_end, *seq_end;  // per record: where its name line begins, where that line and the sequence line end
  u32 *read_at, *read_len;            // per record: its read within the text
  u64 *chunk_sum;                     // per chunk: its reads' bytes, then the bytes before it
  u32 *chunk_max;
};

constexpr u32 kTileThreads = kTileBytes / 16;  // 16 bytes of text per thread
constexpr u32 kChunkThreads = 256, kGroup = 16, kGroups = kChunkThreads / kGroup;
static_assert(kTileThreads == 256 && kChunkRecords == 4 * kChunkThreads && kChunkRecords % kGroups == 0, "the kernels' shapes");

__device__ __forceinline__ u32 load32(const u8 *p) { u32 v; __builtin_memcpy(&v, p, 4); return v; }

// bit b set: byte at + b of the text is a newline (bytes at or beyond text_bytes are none)
__device__ __forceinline__ u32 newline_mask16(const u8 *__restrict__ text, u64 at, u64 text_bytes) {
  u32 m = 0;
  if (at + 16 <= text_bytes) {
#pragma unroll
    for (u32 w = 0; w < 4; ++w) {
      const u32 x = load32(text + at + 4 * w) ^ 0x0a0a0a0au;
      const u32 z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);  // 0x80 in every byte of x that is 0
      m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * w);
    }
  }
  else {
    for (u32 b = 0; b < 16 && at + b < text_bytes; ++b) m |= static_cast<u32>(text[at + b] == '\n') << b;
  }
  return m;
}

// exclusive prefix sum over the workgroup's threads (NT a multiple of 64, at most 1024); part: NT / 64 + 1 values of LDS
template <class T, u32 NT> __device__ __forceinline__ T block_excl_sum(T v, T &total, T *part) {
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(incl, d);
    if (lane >= static_cast<u32>(d)) incl += o;
  }
  __syncthreads();  // (part may still be read from the previous call)
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    T s = 0;
    for (u32 w = 0; w < NT / 64; ++w) { const T t = part[w]; part[w] = s; s += t; }
    part[NT / 64] = s;
  }
  __syncthreads();
  total = part[NT / 64];
  return part[wave] + incl - v;
}

__global__ __launch_bounds__(kTileThreads) void count_newlines_kernel(const u8 *__restrict__ text, u64 text_bytes, u32 n_tiles, u32 *__restrict__ tile) {
  __shared__ u32 part[kTileThreads / 64 + 1];
  const u32 t = blockIdx.x;
  if (t >= n_tiles) return;
  const u64 at = static_cast<u64>(t) * kTileBytes + 16u * threadIdx.x;
  u32 total;
  (void)block_excl_sum<u32, kTileThreads>(__popc(newline_mask16(text, at, text_bytes)), total, part);
  if (threadIdx.x == 0) tile[t] = total;
}

__global__ __launch_bounds__(kScanTiles) void scan_tiles_kernel(const u8 *__restrict__ text, u64 text_bytes, u32 n_tiles, u64 cap, Scratch s,
                                                                abm_fastq_info *__restrict__ info) {
  __shared__ u32 part[kScanTiles / 64 + 1];
  u32 carry = 0;
  for (u32 base = 0; base < n_tiles; base += kScanTiles) {
    const u32 i = base + threadIdx.x;
    u32 total;
    const u32 before = block_excl_sum<u32, kScanTiles>(i < n_tiles ? s.tile[i] : 0u, total, part);
    if (i < n_tiles) s.tile[i] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) {
    const u64 lines = static_cast<u64>(carry) + (text_bytes && text[text_bytes - 1] != '\n' ? 1u : 0u);
    const u64 n = records_of(lines);
    s.head->n_records = n;
    s.head->err = kNoError;
    s.head->newlines = carry;
    s.head->fits = n <= cap;
    if (n > cap) *info = abm_fastq_info{n, 0, 0, ABM_FASTQ_OK, 0, 0};
  }
}

__global__ __launch_bounds__(kTileThreads) void mark_lines_kernel(const u8 *__restrict__ text, u64 text_bytes, u32 n_tiles, Scratch s) {
  __shared__ u32 part[kTileThreads / 64 + 1];
  const u32 t = blockIdx.x;
  if (t >= n_tiles || !s.head->fits) return;
  const u64 n = s.head->n_records;
  const u64 at = static_cast<u64>(t) * kTileBytes + 16u * threadIdx.x;
  u32 mask = newline_mask16(text, at, text_bytes), total;
  u64 k = static_cast<u64>(s.tile[t]) + block_excl_sum<u32, kTileThreads>(__popc(mask), total, part);
  for (; mask; mask &= mask - 1, ++k) {
    const u64 i = at + static_cast<u32>(__builtin_ctz(mask)), j = k >> 2;  // line k ends at byte i
    switch (k & 3u) {
    case 0:
      if (j < n) s.name_end[j] = static_cast<u32>(i);
      if (i == 0 || text[i - 1] == '\n') atomicMin(reinterpret_cast<unsigned long long *>(&s.head->err), error_key(k, ABM_FASTQ_EMPTY_NAME));
      break;
    case 1:
      if (j < n) s.seq_end[j] = static_cast<u32>(i);
      break;
    case 3:
      if (i + 1 < text_bytes && j + 1 < n) s.name_at[j + 1] = static_cast<u32>(i + 1);
      break;
    }
  }
  if (threadIdx.x == 0) {
    if (t == 0 && n) s.name_at[0] = 0;
    // a last line without a newline ends where the text does: it matters if it is a sequence line
    if (t == n_tiles - 1 && text[text_bytes - 1] != '\n') {
      const u64 last = static_cast<u64>(s.tile[t]) + total;
      if ((last & 3u) == 1 && (last >> 2) < n) s.seq_end[last >> 2] = static_cast<u32>(text_bytes);
    }
  }
}

// the 16 bits of a ballot that belong to this lane's group
__device__ __forceinline__ u32 group_ballot(bool p) {
  return static_cast<u32>(__ballot(p) >> ((threadIdx.x & 63u) & ~(kGroup - 1))) & 0xFFFFu;
}
__device__ __forceinline__ void group_merge(SeqScan &sc) {
#pragma unroll
  for (int d = 1; d < static_cast<int>(kGroup); d <<= 1) {
    SeqScan o;
    o.letters = __shfl_xor(sc.letters, d);
    o.end = __shfl_xor(sc.end, d);
    o.first = __shfl_xor(sc.first, d);
    seq_merge(sc, o);
  }
}

__global__ __launch_bounds__(kChunkThreads) void apply_rules_kernel(const u8 *__restrict__ text, u64 text_bytes, u32 min_letters, Scratch s,
                                                                    u64 *__restrict__ out_name_at, u32 *__restrict__ out_name_len) {
  __shared__ u64 g_sum[kGroups];
  __shared__ u32 g_max[kGroups];
  if (!s.head->fits) return;
  const u64 n = s.head->n_records, first = static_cast<u64>(blockIdx.x) * kChunkRecords;
  if (first >= n) return;
  const u32 l = threadIdx.x & (kGroup - 1), g = threadIdx.x / kGroup;
  unsigned long long *err = reinterpret_cast<unsigned long long *>(&s.head->err);
  u64 sum = 0;
  u32 longest = 0;
  for (u32 r = g; r < kChunkRecords; r += kGroups) {
    const u64 j = first + r;
    if (j >= n) break;
    const u32 ns = s.name_at[j], ne = s.name_end[j], ss = ne + 1, se = s.seq_end[j];
    // (holds by construction: ns <= ne < se <= text_bytes; a record that broke it would be skipped, not read)
    if (!(ns <= ne && ne < se && se <= text_bytes)) { if (l == 0) { s.read_at[j] = 0; s.read_len[j] = 0; } continue; }
    // the name: from ns + 1 to the first space or tab, or to the line's end
    u32 stop = ne;
    for (u32 q = ns + 1; q < ne; q += kGroup) {
      const u32 hit = group_ballot(q + l < ne && ends_name(text[q + l]));
      if (hit) { stop = q + static_cast<u32>(__builtin_ctz(hit)); break; }
    }
    const u32 name_n = ne > ns ? stop - (ns + 1) : 0u;
    // the read
    const u32 len = se - ss;
    u32 at = 0, m = 0, code = ABM_FASTQ_OK;
    if (too_long(len)) code = ABM_FASTQ_TOO_LONG;
    else {
      SeqScan sc;
      for (u32 q = 4 * l; q < len; q += 4 * kGroup) {
        if (q + 4 <= len) {
          const u32 w = load32(text + ss + q);
#pragma unroll
          for (u32 b = 0; b < 4; ++b) seq_byte(sc, q + b, static_cast<u8>(w >> (8 * b)));
        }
        else {
          for (u32 b = 0; q + b < len; ++b) seq_byte(sc, q + b, text[ss + q + b]);
        }
      }
      group_merge(sc);
      code = seq_finish(sc, min_letters, at, m);
    }
    if (l == 0) {
      if (code != ABM_FASTQ_OK) atomicMin(err, error_key(4 * j + 1, code));
      s.read_at[j] = ss + at;
      s.read_len[j] = m;
      if (out_name_at) out_name_at[j] = static_cast<u64>(ns) + 1;
      if (out_name_len) out_name_len[j] = name_n;
    }
    sum += m;
    longest = max(longest, m);
  }
  if (l == 0) { g_sum[g] = sum; g_max[g] = longest; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (u32 k = 1; k < kGroups; ++k) { sum += g_sum[k]; longest = max(longest, g_max[k]); }
    s.chunk_sum[blockIdx.x] = sum;
    s.chunk_max[blockIdx.x] = longest;
  }
}

__global__ __launch_bounds__(kScanTiles) void scan_chunks_kernel(Scratch s, u64 *__restrict__ off, abm_fastq_info *__restrict__ info) {
  __shared__ u64 part[kScanTiles / 64 + 1];
  __shared__ u32 w_max[kScanTiles / 64];
  if (!s.head->fits) return;
  const u64 n = s.head->n_records;
  const u32 n_chunks = static_cast<u32>((n + kChunkRecords - 1) / kChunkRecords);
  u64 carry = 0;
  u32 longest = 0;
  for (u32 base = 0; base < n_chunks; base += kScanTiles) {
    const u32 i = base + threadIdx.x;
    u64 total;
    const u64 before = block_excl_sum<u64, kScanTiles>(i < n_chunks ? s.chunk_sum[i] : 0ull, total, part);
    if (i < n_chunks) { s.chunk_sum[i] = carry + before; longest = max(longest, s.chunk_max[i]); }
    carry += total;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) longest = max(longest, static_cast<u32>(__shfl_xor(longest, d)));
  if ((threadIdx.x & 63u) == 0) w_max[threadIdx.x >> 6] = longest;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (u32 w = 1; w < kScanTiles / 64; ++w) longest = max(longest, w_max[w]);
    const u64 key = s.head->err;
    abm_fastq_info r{n, carry, longest, ABM_FASTQ_OK, 0, 0};
    if (key != kNoError) {
      r.code = key_code(key);
      r.line = key_line(key);
      const u64 j = r.line >> 2;
      if (r.code == ABM_FASTQ_TOO_LONG && j < n) r.value = s.seq_end[j] - (s.name_end[j] + 1);
    }
    *info = r;
    off[n] = carry;
  }
}

__global__ __launch_bounds__(kChunkThreads) void copy_reads_kernel(const u8 *__restrict__ text, Scratch s, u8 *__restrict__ blob, u64 blob_capacity,
                                                                   u64 *__restrict__ off) {
  __shared__ u32 part[kChunkThreads / 64 + 1];
  __shared__ u32 rel[kChunkRecords];
  if (!s.head->fits) return;
  const u64 n = s.head->n_records, first = static_cast<u64>(blockIdx.x) * kChunkRecords;
  if (first >= n) return;
  const u64 base = s.chunk_sum[blockIdx.x];
  u32 mine[4], own = 0;
#pragma unroll
  for (u32 q = 0; q < 4; ++q) {
    const u64 j = first + 4u * threadIdx.x + q;
    mine[q] = j < n ? s.read_len[j] : 0u;
    own += mine[q];
  }
  u32 total;
  u32 at = block_excl_sum<u32, kChunkThreads>(own, total, part);
#pragma unroll
  for (u32 q = 0; q < 4; ++q) {
    const u64 j = first + 4u * threadIdx.x + q;
    rel[4u * threadIdx.x + q] = at;
    if (j < n) off[j] = base + at;
    at += mine[q];
  }
  __syncthreads();
  const u32 l = threadIdx.x & (kGroup - 1), g = threadIdx.x / kGroup;
  for (u32 r = g; r < kChunkRecords; r += kGroups) {
    const u64 j = first + r;
    if (j >= n) break;
    const u64 to = base + rel[r];
    const u32 len = s.read_len[j];
    const u32 m = to < blob_capacity ? static_cast<u32>(min(static_cast<u64>(len), blob_capacity - to)) : 0u;
    const u8 *src = text + s.read_at[j];
    u8 *dst = blob + to;
    // bytes up to dst's first whole word, whole words (the source is read unaligned), the bytes after them
    const u32 head = min(m, static_cast<u32>((4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u)), n_words = (m - head) / 4;
    if (l < head) dst[l] = src[l];
    for (u32 k = l; k < n_words; k += kGroup) *reinterpret_cast<u32 *>(dst + head + 4 * k) = load32(src + head + 4 * k);
    const u32 done = head + 4 * n_words;
    if (l < m - done) dst[done + l] = src[done + l];
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

void check_text_bytes(const char *who, u64 text_bytes) {
  if (text_bytes >> 32) throw std::runtime_error(std::string(who) + ": a text of 2^32 bytes or more (cut it at a record's first line)");
}
// records a text of this many bytes can hold at most: every record but the last has four newlines
u64 most_records(u64 text_bytes) { return records_of(text_bytes); }

}  // namespace

// One owner per buffer: the parser owns its stream, its scratch arrays, the device copies of a host call's text and outputs
// and its pinned staging; nothing of it is shared with an abm_ctx, an inflater, a deflater or another parser.
struct abm_fastq_parser {
  int device = 0;
  hipStream_t stream = nullptr;
  DevBytes d_head, d_tile, d_rec, d_chunk;                           // the scratch
  DevBytes d_text, d_blob, d_off, d_name_at, d_name_len, d_info;     // abm_fastq_parse's device side
  PinnedBytes h_text, h_blob, h_off, h_name_at, h_name_len, h_info;  // ... and its staging
  std::mutex mu;
  ~abm_fastq_parser() { if (stream) (void)hipStreamDestroy(stream); }

  static u32 tiles_of(u64 text_bytes) { return static_cast<u32>((text_bytes + kTileBytes - 1) / kTileBytes); }
  // (under mu) the scratch for a text of text_bytes with room for `cap` records
  Scratch scratch(u64 text_bytes, u64 cap) {
    const size_t n_chunks = static_cast<size_t>((cap + kChunkRecords - 1) / kChunkRecords);
    d_head.reserve(sizeof(Head));
    d_tile.reserve(grown(static_cast<size_t>(tiles_of(text_bytes)) * sizeof(u32)));
    d_rec.reserve(grown(static_cast<size_t>(cap) * 5 * sizeof(u32)));
    d_chunk.reserve(grown(n_chunks * (sizeof(u64) + sizeof(u32))));
    Scratch s;
    s.head = reinterpret_cast<Head *>(d_head.p);
    s.tile = reinterpret_cast<u32 *>(d_tile.p);
    u32 *r = reinterpret_cast<u32 *>(d_rec.p);
    s.name_at = r; s.name_end = r + cap; s.seq_end = r + 2 * cap; s.read_at = r + 3 * cap; s.read_len = r + 4 * cap;
    s.chunk_sum = reinterpret_cast<u64 *>(d_chunk.p);
    s.chunk_max = reinterpret_cast<u32 *>(d_chunk.p + n_chunks * sizeof(u64));
    return s;
  }
  // (under mu) the first two kernels: the text's records, and whether they fit `fit` (what the caller's arrays hold)
  void launch_count(const u8 *d_t, u64 text_bytes, u64 fit, const Scratch &s, abm_fastq_info *d_i, hipStream_t on) {
    const u32 n_tiles = tiles_of(text_bytes);
    if (n_tiles) {
      hipLaunchKernelGGL(count_newlines_kernel, dim3(n_tiles), dim3(kTileThreads), 0, on, d_t, text_bytes, n_tiles, s.tile);
      HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(kScanTiles), 0, on, d_t, text_bytes, n_tiles, fit, s, d_i);
    HIPCHK(hipGetLastError());
  }
  // ... and the other four; cap: the records the scratch arrays were sized for (>= every count that fits)
  void launch_parse(const u8 *d_t, u64 text_bytes, u32 min_letters, u64 cap, const Scratch &s, u8 *d_b, u64 blob_capacity, u64 *d_o, u64 *d_na,
                    u32 *d_nl, abm_fastq_info *d_i, hipStream_t on) {
    const u32 n_tiles = tiles_of(text_bytes), n_chunks = static_cast<u32>((cap + kChunkRecords - 1) / kChunkRecords);
    if (n_tiles) {
      hipLaunchKernelGGL(mark_lines_kernel, dim3(n_tiles), dim3(kTileThreads), 0, on, d_t, text_bytes, n_tiles, s);
      HIPCHK(hipGetLastError());
    }
    if (n_chunks) {
      hipLaunchKernelGGL(apply_rules_kernel, dim3(n_chunks), dim3(kChunkThreads), 0, on, d_t, text_bytes, min_letters, s, d_na, d_nl);
      HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(scan_chunks_kernel, dim3(1), dim3(kScanTiles), 0, on, s, d_o, d_i);
    HIPCHK(hipGetLastError());
    if (n_chunks) {
      hipLaunchKernelGGL(copy_reads_kernel, dim3(n_chunks), dim3(kChunkThreads), 0, on, d_t, s, d_b, blob_capacity, d_o);
      HIPCHK(hipGetLastError());
    }
  }
};

namespace {

// what the host entry points do once *info is known: the return code, with its message
int outcome(const char *who, const abm_fastq_info &info, u64 blob_capacity, u64 rec_capacity, bool &write) {
  write = false;
  if (info.n_records > rec_capacity || info.blob_bytes > blob_capacity) {
    abm::set_last_error(std::string(who) + (info.n_records > rec_capacity ? ": more records than rec_capacity" : ": the reads need more bytes than blob_capacity"));
    return ABM_ERR_CAPACITY;
  }
  write = true;
  if (info.code != ABM_FASTQ_OK) {
    static const char *const what[] = {"", "an empty read name", "a read that is too long", "a read without A/C/G/T"};
    abm::set_last_error(std::string(who) + ": " + what[info.code & 3u] + " at line " + std::to_string(info.line) + " of the text");
    return ABM_ERR_FASTQ;
  }
  return 0;
}

}  // namespace

extern "C" {

void abm_fastq_sizes(uint32_t *tile_bytes, uint32_t *scan_tiles, uint32_t *chunk_records) {
  if (tile_bytes) *tile_bytes = kTileBytes;
  if (scan_tiles) *scan_tiles = kScanTiles;
  if (chunk_records) *chunk_records = kChunkRecords;
}

int abm_fastq_parser_create(int device, abm_fastq_parser **out) {
  return guarded([&]() -> int {
    if (!out) throw std::runtime_error("abm_fastq_parser_create: null argument");
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) throw std::runtime_error("abm_fastq_parser_create: no HIP device (abm_fastq_parse_host runs the same rules on the CPU)");
    if (device < 0 || device >= n_dev) throw std::runtime_error("abm_fastq_parser_create: no such device: " + std::to_string(device));
    HIPCHK(hipSetDevice(device));
    abm_fastq_parser *p = new abm_fastq_parser;
    try {
      p->device = device;
      HIPCHK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
      p->d_info.reserve(sizeof(abm_fastq_info));
      p->h_info.reserve(sizeof(abm_fastq_info));
    }
    catch (...) { delete p; throw; }
    *out = p;
    return 0;
  });
}

void abm_fastq_parser_destroy(abm_fastq_parser *p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  delete p;
}

int abm_fastq_parse(abm_fastq_parser *p, const void *text, uint64_t text_bytes, uint32_t min_letters, char *blob, uint64_t blob_capacity,
                    uint64_t *off, uint64_t *name_at, uint32_t *name_len, uint64_t rec_capacity, abm_fastq_info *info) {
  return guarded([&]() -> int {
    if ((!text && text_bytes) || (!blob && blob_capacity) || !off || !info) throw std::runtime_error("abm_fastq_parse: null argument");
    check_text_bytes("abm_fastq_parse", text_bytes);
    if (!p) throw std::runtime_error("abm_fastq_parse: null parser");
    std::lock_guard<std::mutex> lk(p->mu);
    HIPCHK(hipSetDevice(p->device));
    hipStream_t st = p->stream;
    abm_fastq_info *d_i = reinterpret_cast<abm_fastq_info *>(p->d_info.p), *h_i = reinterpret_cast<abm_fastq_info *>(p->h_info.p);
    p->d_text.reserve(grown(text_bytes)); p->h_text.reserve(grown(text_bytes));
    if (text_bytes) {
      std::memcpy(p->h_text.p, text, text_bytes);
      HIPCHK(hipMemcpyAsync(p->d_text.p, p->h_text.p, text_bytes, hipMemcpyHostToDevice, st));
    }
    // the records first: everything after is sized by their number (the count is 8 bytes back and one wait)
    Scratch s = p->scratch(text_bytes, 0);
    p->launch_count(p->d_text.p, text_bytes, ~0ull, s, d_i, st);
    HIPCHK(hipMemcpyAsync(h_i, s.head, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    u64 n = 0;
    std::memcpy(&n, h_i, sizeof(u64));
    if (n > most_records(text_bytes)) throw std::runtime_error("abm_fastq_parse: more records than the text can hold");
    s = p->scratch(text_bytes, n);
    const size_t off_n = static_cast<size_t>(n + 1) * sizeof(u64), at_n = static_cast<size_t>(n) * sizeof(u64), len_n = static_cast<size_t>(n) * sizeof(u32);
    p->d_blob.reserve(grown(text_bytes));
    p->d_off.reserve(grown(off_n));
    p->d_name_at.reserve(grown(at_n));
    p->d_name_len.reserve(grown(len_n));
    p->launch_parse(p->d_text.p, text_bytes, min_letters, n, s, p->d_blob.p, text_bytes, reinterpret_cast<u64 *>(p->d_off.p),
                    reinterpret_cast<u64 *>(p->d_name_at.p), reinterpret_cast<u32 *>(p->d_name_len.p), d_i, st);
    HIPCHK(hipMemcpyAsync(h_i, d_i, sizeof(abm_fastq_info), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    abm_fastq_info r;
    std::memcpy(&r, h_i, sizeof r);
    if (r.n_records != n || r.blob_bytes > text_bytes) throw std::runtime_error("abm_fastq_parse: the device's counts disagree");
    *info = r;
    bool write = false;
    const int rc = outcome("abm_fastq_parse", r, blob_capacity, rec_capacity, write);
    if (!write) return rc;
    p->h_blob.reserve(grown(r.blob_bytes)); p->h_off.reserve(grown(off_n));
    if (r.blob_bytes) HIPCHK(hipMemcpyAsync(p->h_blob.p, p->d_blob.p, r.blob_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(p->h_off.p, p->d_off.p, off_n, hipMemcpyDeviceToHost, st));
    if (name_at && n) { p->h_name_at.reserve(grown(at_n)); HIPCHK(hipMemcpyAsync(p->h_name_at.p, p->d_name_at.p, at_n, hipMemcpyDeviceToHost, st)); }
    if (name_len && n) { p->h_name_len.reserve(grown(len_n)); HIPCHK(hipMemcpyAsync(p->h_name_len.p, p->d_name_len.p, len_n, hipMemcpyDeviceToHost, st)); }
    HIPCHK(hipStreamSynchronize(st));
    if (r.blob_bytes) std::memcpy(blob, p->h_blob.p, r.blob_bytes);
    std::memcpy(off, p->h_off.p, off_n);
    if (name_at && n) std::memcpy(name_at, p->h_name_at.p, at_n);
    if (name_len && n) std::memcpy(name_len, p->h_name_len.p, len_n);
    return rc;
  });
}

int abm_fastq_parse_device(abm_fastq_parser *p, const void *d_text, uint64_t text_bytes, uint32_t min_letters, char *d_blob, uint64_t blob_capacity,
                           uint64_t *d_off, uint64_t *d_name_at, uint32_t *d_name_len, uint64_t rec_capacity, abm_fastq_info *d_info, void *stream) {
  return guarded([&]() -> int {
    if (!p || (!d_text && text_bytes) || (!d_blob && blob_capacity) || !d_off || !d_info) throw std::runtime_error("abm_fastq_parse_device: null argument");
    check_text_bytes("abm_fastq_parse_device", text_bytes);
    std::lock_guard<std::mutex> lk(p->mu);
    HIPCHK(hipSetDevice(p->device));
    hipStream_t on = static_cast<hipStream_t>(stream);
    // (a text holds at most most_records(): a larger capacity asks for no larger scratch)
    const u64 cap = std::min<u64>(rec_capacity, most_records(text_bytes));
    const Scratch s = p->scratch(text_bytes, cap);
    p->launch_count(static_cast<const u8 *>(d_text), text_bytes, cap, s, d_info, on);
    p->launch_parse(static_cast<const u8 *>(d_text), text_bytes, min_letters, cap, s, reinterpret_cast<u8 *>(d_blob), blob_capacity, d_off, d_name_at,
                    d_name_len, d_info, on);
    return 0;
  });
}

int abm_fastq_parse_host(const void *text, uint64_t text_bytes, uint32_t min_letters, char *blob, uint64_t blob_capacity, uint64_t *off,
                         uint64_t *name_at, uint32_t *name_len, uint64_t rec_capacity, abm_fastq_info *info) {
  return guarded([&]() -> int {
    if ((!text && text_bytes) || (!blob && blob_capacity) || !off || !info) throw std::runtime_error("abm_fastq_parse_host: null argument");
    check_text_bytes("abm_fastq_parse_host", text_bytes);
    const u8 *t = static_cast<const u8 *>(text);
    abm_fastq_info r;
    parse_serial(t, text_bytes, min_letters, false, nullptr, nullptr, nullptr, nullptr, r);
    *info = r;
    bool write = false;
    const int rc = outcome("abm_fastq_parse_host", r, blob_capacity, rec_capacity, write);
    if (write) parse_serial(t, text_bytes, min_letters, true, reinterpret_cast<u8 *>(blob), off, name_at, name_len, r);
    return rc;
  });
}

}  // extern "C"
