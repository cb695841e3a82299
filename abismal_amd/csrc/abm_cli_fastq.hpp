// abismal-amd, FASTQ front end: buffers and their pools, slices and batches, the splitter of compressed input, the
// parser with ReadLoader's rules, the lead-in ("ghost") helpers.  Part of abm_cli.cpp's one translation unit (and of
// tests/cpp/cli_parse_harness.cpp, which includes that): everything here has internal linkage.
#pragma once
#include "abm_cli_records.hpp"
#include "abm_fastq_core.hpp"

#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

#include <atomic>
#include <memory>
#include <mutex>

namespace {

constexpr uint32_t kPadding = abm_fastq::kMaxRead;  // 32767
uint32_t g_min_read_len = 44;  // key weight + the index's window - 1 (src/abismal.cpp:212-213): 36 with a short-read index
uint32_t g_map_read_len = 35;  // shortest trimmed read the library maps (DevIndex::map_len, abm_device.hpp): 29 with a short-read index

// ---- FASTQ, with ReadLoader's rules (src/abismal.cpp:164-201) -----------------
// Stage 1 (one thread per input file) only cuts the file into batches of whole records;
// stage 2 (a pool) applies the reference's per-record rules and lays the reads out for the C ABI.
// A batch's FASTQ text: grown with realloc (large blocks are remapped, not copied, and never
// zero-filled) and recycled through a small pool so that its pages stay faulted in.
std::atomic<uint64_t> g_pinned_bytes{0};  // page-locked memory the run has asked the library for (batches' read buffers)
struct RawBuf {
  char *p = nullptr;
  size_t n = 0, cap = 0;
  bool pinned = false;  // page-locked memory from the library (abm_host_alloc): what a batch's reads are uploaded from
  RawBuf() = default;
  RawBuf(const RawBuf &) = delete;
  RawBuf &operator=(const RawBuf &) = delete;
  RawBuf(RawBuf &&o) noexcept : p(o.p), n(o.n), cap(o.cap), pinned(o.pinned) { o.p = nullptr; o.n = o.cap = 0; }
  RawBuf &operator=(RawBuf &&o) noexcept { std::swap(p, o.p); std::swap(n, o.n); std::swap(cap, o.cap); std::swap(pinned, o.pinned); return *this; }
  ~RawBuf() { if (pinned) abm_host_free(p); else std::free(p); }
  // Big blocks are 2 MB-aligned and advised to use huge pages: a run touches gigabytes of fresh memory
  // from a hundred threads at once, and with 4 KB pages that is a million page faults on one address space.
  void reserve(size_t want) {
    if (want <= cap) return;
    want = std::max(want, cap + cap / 2);
    char *q;
    if (pinned) {
      void *v = nullptr;
      if (abm_host_alloc(want, &v) != 0) throw std::bad_alloc();
      g_pinned_bytes += want - cap;
      q = static_cast<char *>(v);
      if (n) std::memcpy(q, p, n);
      abm_host_free(p);
    }
    else if (want >= (4u << 20)) {
      want = (want + (2u << 20) - 1) & ~static_cast<size_t>((2u << 20) - 1);
      q = static_cast<char *>(std::aligned_alloc(2u << 20, want));
      if (!q) throw std::bad_alloc();
      ::madvise(q, want, MADV_HUGEPAGE);
      if (n) std::memcpy(q, p, n);
      std::free(p);
    }
    else {
      q = static_cast<char *>(std::realloc(p, want));
      if (!q) throw std::bad_alloc();
    }
    p = q; cap = want;
  }
  void append(const char *src, size_t len) { reserve(n + len); std::memcpy(p + n, src, len); n += len; }
  // the part of std::string's interface the formatting code uses (contents are never zero-filled)
  void append(size_t count, char c) { reserve(n + count); std::memset(p + n, c, count); n += count; }
  void append(const std::string &t) { append(t.data(), t.size()); }
  RawBuf &operator+=(char c) { if (n == cap) reserve(n + 1); p[n++] = c; return *this; }
  RawBuf &operator+=(const std::string &t) { append(t.data(), t.size()); return *this; }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
  void resize(size_t m) { reserve(m); n = m; }
  void clear() { n = 0; }
  char &operator[](size_t i) { return p[i]; }
  const char &operator[](size_t i) const { return p[i]; }
  char *data() { return p; }
  const char *data() const { return p; }
  void swap(RawBuf &o) { std::swap(p, o.p); std::swap(n, o.n); std::swap(cap, o.cap); }
};
// std::vector<T>'s resize/data/[] for plain-data T without the zero fill (a batch's result arrays are a few
// hundred megabytes that the C ABI overwrites entirely; filling them first, single-threaded, cost a 8 M-read
// batch 0.3 s before its upload could start)
template <class T> struct PodVec {
  RawBuf b;
  void resize(size_t n) { b.resize(n * sizeof(T)); }
  void assign(size_t n, T v) { resize(n); for (size_t i = 0; i < n; ++i) data()[i] = v; }
  size_t size() const { return b.size() / sizeof(T); }
  T *data() { return reinterpret_cast<T *>(b.p); }
  const T *data() const { return reinterpret_cast<const T *>(b.p); }
  T &operator[](size_t i) { return data()[i]; }
  const T &operator[](size_t i) const { return data()[i]; }
};
struct RawPool {
  std::mutex mu;
  std::vector<RawBuf> free_list;
  RawBuf get() {
    std::lock_guard<std::mutex> lk(mu);
    if (free_list.empty()) return RawBuf();
    RawBuf b = std::move(free_list.back());
    free_list.pop_back();
    b.n = 0;
    return b;
  }
  void put(RawBuf &&b) {
    std::lock_guard<std::mutex> lk(mu);
    if (free_list.size() < 1024) free_list.push_back(std::move(b));
  }
};

struct Batch;

// The unit of host work: up to `slice_reads` records of the input, in file order.  Slices are cut,
// parsed, formatted and written independently; a batch handed to a GPU is a run of consecutive slices.
struct Slice {
  uint64_t g = 0;                    // slice number within its region = output order
  int region = 0;                    // which contiguous share of the input (= which output file) it belongs to
  int node = 0;                      // NUMA node its buffers were first touched on: where it is parsed and formatted
  uint64_t place = 0;                // its text's offset in the region's file, once every earlier slice's size is known
  std::vector<uint32_t> tail;        // records that can still be a ghost-bit source for later reads (ghost_tail)
  uint64_t first_line[2] = {0, 0};
  uint64_t byte_lo[2] = {0, 0}, byte_hi[2] = {0, 0};  // plain files: the slice's text in each file
  RawBuf raw[2];                     // the FASTQ text (names point into it)
  std::vector<NameRef> names[2];
  RawBuf blob[2];                    // reads as ReadLoader hands them over, concatenated
  std::vector<uint64_t> off[2];
  size_t n() const { return names[0].size(); }
  Batch *batch = nullptr;            // once mapped: the batch whose arrays hold this slice's results ...
  size_t base = 0;                   // ... from this index on
  RawBuf text;                       // formatted output
  Stats3 stats;
  // single-end batches hand their results over slice by slice while the kernel runs (abm_map_se_batch_sliced): the
  // slice then holds its own copy -- hits and a compact CIGAR blob with n() + 1 offsets
  bool own = false;
  bool virt = false;                 // virtual GPUs: own_* are filled in by the formatter (made-up hits)
  PodVec<abm_hit> own_se;
  PodVec<uint32_t> own_cig;
  PodVec<uint64_t> own_cig_off;
  // ... and, when the kernel wrote the reads' SAM text itself (abm_ctx_set_sam_tails), every read's line after QNAME:
  // lengths (0 = no record, 0xFFFFFFFF = format it here) and the text, one after the other
  bool has_tails = false;
  PodVec<uint32_t> tail_len;
  RawBuf tail_text;
  // (pairs: two lengths per pair, end 1's then end 2's, and the pair's kind -- abm_ctx_pe_sam_tails; 0xFF = format it here)
  PodVec<uint8_t> tail_kind;
};

// written slices are recycled with their buffers (names, reads, output text keep their capacity): a
// process with a hundred threads that keeps allocating and freeing multi-megabyte blocks spends its
// time on the address-space lock
struct SlicePool {
  std::mutex mu;
  std::vector<std::unique_ptr<Slice>> free_list;
  std::unique_ptr<Slice> get() {
    std::unique_ptr<Slice> s;
    {
      std::lock_guard<std::mutex> lk(mu);
      if (!free_list.empty()) { s = std::move(free_list.back()); free_list.pop_back(); }
    }
    if (!s) s.reset(new Slice);
    return s;
  }
  void put(std::unique_ptr<Slice> s) {
    for (int e = 0; e < 2; ++e) { s->names[e].clear(); s->blob[e].clear(); s->off[e].clear(); s->raw[e].n = 0; }
    s->text.clear();
    s->stats = Stats3();
    s->batch = nullptr;
    s->base = 0;
    s->own = false;
    s->virt = false;
    s->tail.clear();
    std::lock_guard<std::mutex> lk(mu);
    if (free_list.size() < 1024) free_list.push_back(std::move(s));
  }
};

bool g_pin_batches = true;  // batch blobs in page-locked memory (not with virtual GPUs: it comes from the HIP runtime)
struct Batch {
  Batch() { for (int e = 0; e < 2; ++e) blob[e].pinned = off_bytes[e].pinned = g_pin_batches; }
  uint64_t seq = 0;
  int gpu = 0;
  int node = 0;                      // NUMA node of its GPU: the pool it returns to
  std::vector<std::unique_ptr<Slice>> slices;
  size_t n = 0;
  std::vector<std::string> carry[2]; // reads of the input just before this batch, mapped along for their side effects only
  RawBuf blob[2];                    // carry + the slices' reads concatenated, as the C ABI takes them
  RawBuf off_bytes[2];               // ... and their n + 1 offsets (uint64_t)
  uint64_t *off_of(int e) { return reinterpret_cast<uint64_t *>(off_bytes[e].p); }
  PodVec<abm_hit> se[2];
  PodVec<abm_pair> pairs;
  PodVec<uint32_t> cig[2];
  PodVec<uint64_t> cig_off[2];
  int slices_left = 0;               // not yet written
};

// What a read of 44-46 bases finds past its end comes, position by position, from the nearest EARLIER
// read that is longer than that position -- up to 64 positions out, so a read of kGhostReach = 46 + 64 bases hides
// everything before it, and reads that are not mapped (empty, or shorter than g_map_read_len) leave nothing.
// ghost_tail: of n records (off[e][k], off[e][k + 1]: read k of end e), scanning backwards, those that are longer in
// some end than every record after them, until all ends have reached kGhostReach -- the only records of this input
// that can still be such a source for reads that come later.  Indices in descending order; at most 67 per end.
constexpr uint32_t kGhostReach = 110;
inline uint32_t ghost_len(uint64_t len) { return len < g_map_read_len ? 0u : static_cast<uint32_t>(std::min<uint64_t>(len, kGhostReach)); }
// (reach: how far each end is covered by the records after these n -- a scan that continues further back in the input
// passes the same array on; a fresh scan starts from ghost_reach_start)
inline void ghost_reach_start(uint32_t reach[2], int ends) { reach[0] = 0; reach[1] = ends == 2 ? 0u : kGhostReach; }
inline bool ghost_closed(const uint32_t reach[2]) { return reach[0] >= kGhostReach && reach[1] >= kGhostReach; }
std::vector<uint32_t> ghost_tail(const std::vector<uint64_t> *off, size_t n, int ends, uint32_t reach[2]) {
  std::vector<uint32_t> out;
  for (size_t k = n; k-- > 0 && (reach[0] < kGhostReach || reach[1] < kGhostReach);) {
    bool raises = false;
    for (int e = 0; e < ends; ++e) {
      const uint32_t len = ghost_len(off[e][k + 1] - off[e][k]);
      if (len > reach[e]) { raises = true; reach[e] = len; }
    }
    if (raises) out.push_back(static_cast<uint32_t>(k));
  }
  return out;
}
std::vector<uint32_t> ghost_tail(const std::vector<uint64_t> *off, size_t n, int ends) {
  uint32_t reach[2];
  ghost_reach_start(reach, ends);
  return ghost_tail(off, n, ends, reach);
}

// batches are recycled with their buffers as well (a full batch's arrays are a gigabyte)
struct BatchPool {
  std::mutex mu;
  std::vector<std::unique_ptr<Batch>> free_list;
  std::unique_ptr<Batch> get() {
    std::unique_ptr<Batch> b;
    {
      std::lock_guard<std::mutex> lk(mu);
      if (!free_list.empty()) { b = std::move(free_list.back()); free_list.pop_back(); }
    }
    if (!b) b.reset(new Batch);
    return b;
  }
  void put(std::unique_ptr<Batch> b) {
    b->slices.clear();
    b->n = 0; b->seq = 0; b->gpu = 0; b->slices_left = 0;
    for (int e = 0; e < 2; ++e) { b->carry[e].clear(); b->blob[e].clear(); b->off_bytes[e].clear(); }
    std::lock_guard<std::mutex> lk(mu);
    if (free_list.size() < 64) free_list.push_back(std::move(b));
  }
};

// advances over [p + from, p + len) counting newlines until `need` lines are complete; returns the
// offset just past the last newline consumed (block counts vectorise; only the block in which the
// target falls is walked line by line)
size_t scan_lines(const char *p, size_t from, size_t len, uint64_t need, uint64_t &lines) {
  size_t i = from, last = from;
  while (i < len && lines < need) {
    const size_t blk = std::min<size_t>(len - i, 8192);
    uint32_t c = 0;
    for (size_t k = 0; k < blk; ++k) c += (p[i + k] == '\n');
    if (lines + c < need) {
      if (c) last = static_cast<size_t>(static_cast<const char *>(memrchr(p + i, '\n', blk)) - p) + 1;
      lines += c;
      i += blk;
      continue;
    }
    while (lines < need) {
      const char *nl = static_cast<const char *>(std::memchr(p + i, '\n', len - i));
      i = static_cast<size_t>(nl - p) + 1;
      ++lines;
    }
    return i;
  }
  return last;
}

struct RawSplitter {
  gzFile f = nullptr;  // gzip/bgzip-compressed FASTQ goes through zlib (bamxx::bgzf_file in the reference)
  int fd = -1;         // plain text is read directly
  std::string path, carry;  // carry: text read past the end of the previous batch
  uint64_t line_no = 0;
  bool eof = false;
  explicit RawSplitter(const std::string &p) : path(p) {
    fd = ::open(p.c_str(), O_RDONLY);
    if (fd < 0) throw std::runtime_error("cannot open reads file: " + p);
    unsigned char magic[2] = {0, 0};
    const ssize_t got = ::pread(fd, magic, 2, 0);
    if (got == 2 && magic[0] == 0x1f && magic[1] == 0x8b) {
      ::close(fd);
      fd = -1;
      f = gzopen(p.c_str(), "rb");
      if (!f) throw std::runtime_error("cannot open reads file: " + p);
      gzbuffer(f, 1u << 20);
    }
  }
  ~RawSplitter() { if (f) gzclose(f); if (fd >= 0) ::close(fd); }
  size_t fill(char *dst, size_t want) {
    size_t have = 0;
    while (have < want) {
      long got;
      if (f) got = gzread(f, dst + have, static_cast<unsigned>(std::min<size_t>(want - have, 1u << 30)));
      else got = static_cast<long>(::read(fd, dst + have, want - have));
      if (got < 0) throw std::runtime_error("error reading " + path);
      if (got == 0) break;
      have += static_cast<size_t>(got);
    }
    return have;
  }
  // up to `want` records (4 lines each) of text; returns the number of complete lines delivered
  uint64_t next(size_t want, RawBuf &out, uint64_t &first_line) {
    first_line = line_no;
    out.n = 0;
    out.append(carry.data(), carry.size());
    carry.clear();
    const uint64_t need = 4 * static_cast<uint64_t>(want);
    uint64_t lines = 0;
    size_t scanned = scan_lines(out.p, 0, out.n, need, lines);  // meaningful once lines == need
    while (lines < need && !eof) {
      const size_t old = out.n, chunk = 32u << 20;
      out.reserve(std::max(old + chunk, last_size + chunk));
      const size_t got = fill(out.p + old, chunk);
      out.n = old + got;
      if (got < chunk) eof = true;
      scanned = scan_lines(out.p, old, out.n, need, lines);
    }
    if (lines == need) { carry.assign(out.p + scanned, out.n - scanned); out.n = scanned; }
    else if (out.n && out.p[out.n - 1] != '\n') ++lines;  // a last line without a newline still counts (getline semantics)
    last_size = out.n;
    line_no += lines;
    return lines;
  }
  size_t last_size = 0;
  bool exhausted() const { return eof && carry.empty(); }
};

// (the per-record rules are abm_fastq_core.hpp's: the device parser and abm_fastq_parse_host apply the same)
void parse_raw(const char *text, size_t text_n, uint64_t first_line, const std::string &path, std::vector<NameRef> &names,
               RawBuf &blob, std::vector<uint64_t> &off) {
  names.clear(); blob.clear(); off.assign(1, 0);
  blob.reserve(text_n / 2);
  names.reserve(text_n / 200 + 16);
  off.reserve(text_n / 200 + 16);
  const char *p = text, *end = p + text_n;
  for (uint64_t k = 0; p < end; ++k) {
    const char *nl = static_cast<const char *>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
    const char *le = nl ? nl : end;
    const size_t len = static_cast<size_t>(le - p);
    if (k % 4 == 0) {
      if (len == 0)
        throw std::runtime_error("file " + path + " contains an empty read name at line " + std::to_string(first_line + k));
      names.push_back(NameRef{p + 1, abm_fastq::name_length(reinterpret_cast<const uint8_t *>(p), len)});
    }
    else if (k % 4 == 1) {
      if (abm_fastq::too_long(len))
        throw std::runtime_error("found a read of size " + std::to_string(len) +
                                 ", which is too long. Maximum allowed read size = " + std::to_string(kPadding));
      uint32_t at = 0, n = 0;
      if (abm_fastq::seq_rules(reinterpret_cast<const uint8_t *>(p), static_cast<uint32_t>(len), g_min_read_len, at, n) == ABM_FASTQ_NO_BASE)
        throw std::runtime_error("read without A/C/G/T at line " + std::to_string(first_line + k));
      blob.append(p + at, n);
      off.push_back(blob.size());
    }
    if (!nl) break;
    p = nl + 1;
  }
  names.resize(off.size() - 1);  // a trailing name line without its sequence is not a record
}
void parse_raw(const RawBuf &raw, uint64_t first_line, const std::string &path, std::vector<NameRef> &names,
               RawBuf &blob, std::vector<uint64_t> &off) {
  parse_raw(raw.p, raw.n, first_line, path, names, blob, off);
}

// The input's first 256 records, read once per file (through zlib, which passes plain text on as it is): the first
// read's length, the longest read's, and the bytes a record takes on average -- what set-up sizes its buffers by.
struct Sniff {
  bool any = false;       // the file has a first record (its name and sequence lines)
  uint32_t first_len = 0;
  int longest = 0;
  uint64_t rec_bytes = 0;  // 0: not one whole record
};
Sniff sniff_reads(const std::string &path) {
  Sniff s;
  gzFile zf = gzopen(path.c_str(), "rb");
  if (!zf) return s;
  std::vector<char> line(1 << 20);
  uint64_t bytes = 0, recs = 0, got = 0;
  auto next_line = [&] { const bool ok = gzgets(zf, line.data(), static_cast<int>(line.size())) != nullptr; if (ok) got += std::strlen(line.data()); return ok; };
  for (int rec = 0; rec < 256; ++rec) {
    got = 0;
    if (!next_line() || !next_line()) break;
    const uint32_t len = static_cast<uint32_t>(std::strcspn(line.data(), "\r\n"));
    if (!s.any) { s.any = true; s.first_len = len; }
    s.longest = std::max(s.longest, static_cast<int>(len));
    if (!next_line() || !next_line()) break;
    bytes += got; ++recs;
  }
  gzclose(zf);
  if (recs) s.rec_bytes = bytes / recs;
  return s;
}

}  // namespace
