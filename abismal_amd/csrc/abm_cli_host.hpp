// abismal-amd, host placement: the NUMA nodes and cores threads are pinned to, the container's CPU quota, what kind of
// file an input is, the BGZF inflater and deflater on a GPU, the SIGBUS handler of mapped input.  Part of abm_cli.cpp's one translation unit:
// everything here has internal linkage.
#pragma once
#include <fcntl.h>
#include <sched.h>
#include <signal.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

namespace {

// ---- where threads run and where their memory lives --------------------------------------------------------------
// The NUMA nodes of the box and the CPUs this process may use on each (its affinity mask at start-up), the first SMT
// sibling of every core listed apart: a group of threads that fits on a node's cores is kept off their second siblings.
// ABM_CLI_PIN=0 leaves every thread where the scheduler puts it (round 3's behaviour).
struct Topology {
  std::vector<std::vector<int>> primary, all;  // [node] -> CPUs
  std::vector<int> node_id;                    // [node] -> the system's id of that node (nodes without an allowed CPU are left out)
  bool pinning = true;
  static std::vector<int> parse_list(const std::string &s) {
    std::vector<int> out;
    size_t i = 0;
    while (i < s.size() && std::isdigit(static_cast<unsigned char>(s[i]))) {
      const int a = std::atoi(s.c_str() + i);
      while (i < s.size() && std::isdigit(static_cast<unsigned char>(s[i]))) ++i;
      int b = a;
      if (i < s.size() && s[i] == '-') { ++i; b = std::atoi(s.c_str() + i); while (i < s.size() && std::isdigit(static_cast<unsigned char>(s[i]))) ++i; }
      for (int c = a; c <= b; ++c) out.push_back(c);
      if (i < s.size() && s[i] == ',') ++i;
    }
    return out;
  }
  static std::string first_line(const std::string &path) {
    std::ifstream f(path);
    std::string s;
    std::getline(f, s);
    return s;
  }
  Topology() {
    if (const char *e = std::getenv("ABM_CLI_PIN")) pinning = e[0] != '0';
    cpu_set_t mine;
    CPU_ZERO(&mine);
    const bool have_mask = sched_getaffinity(0, sizeof(mine), &mine) == 0;
    for (int n = 0; n < 64; ++n) {
      const std::vector<int> cpus = parse_list(first_line("/sys/devices/system/node/node" + std::to_string(n) + "/cpulist"));
      if (cpus.empty()) { if (n == 0) continue; else break; }
      std::vector<int> p, a;
      for (int c : cpus) {
        if (have_mask && !CPU_ISSET(c, &mine)) continue;
        a.push_back(c);
        const std::vector<int> sib = parse_list(first_line("/sys/devices/system/cpu/cpu" + std::to_string(c) + "/topology/thread_siblings_list"));
        if (sib.empty() || sib.front() == c) p.push_back(c);
      }
      if (a.empty()) continue;
      if (p.empty()) p = a;
      primary.push_back(p);
      all.push_back(a);
      node_id.push_back(n);
    }
    if (all.empty()) {  // no sysfs: one node holding whatever the mask allows
      std::vector<int> a;
      for (int c = 0; c < CPU_SETSIZE; ++c) if (!have_mask || CPU_ISSET(c, &mine)) { if (have_mask || c < static_cast<int>(std::thread::hardware_concurrency())) a.push_back(c); }
      primary.push_back(a);
      all.push_back(a);
      node_id.push_back(0);
      pinning = false;
    }
  }
  int n_nodes() const { return static_cast<int>(all.size()); }
  // the index here of the system's node `id` (sysfs numbering), or -1 if this process may not run there
  int index_of(int id) const {
    for (size_t k = 0; k < node_id.size(); ++k) if (node_id[k] == id) return static_cast<int>(k);
    return -1;
  }
  size_t n_cores() const { size_t k = 0; for (const auto &p : primary) k += p.size(); return k; }
  // the calling thread onto `node`: onto its cores' first siblings while the `group` threads that share the node fit there
  void pin(int node, size_t group) const {
    if (!pinning) return;
    const std::vector<int> &cpus = group <= primary[node].size() ? primary[node] : all[node];
    cpu_set_t set;
    CPU_ZERO(&set);
    for (int c : cpus) CPU_SET(c, &set);
    (void)sched_setaffinity(0, sizeof(set), &set);
  }
};

// ---- BGZF input (bgzip-compressed FASTQ): blocks are independent gzip members that say how long they are ----------
// header: 1f 8b 08 04 | mtime(4) xfl os | xlen(2) | subfields ... 'B' 'C' 02 00 BSIZE(2) ... | deflate data | crc32 isize
// (SAM spec 4.1).  bsize_at returns the block's whole length (BSIZE + 1) or 0 if `p` does not start a BGZF block.
inline uint32_t le16(const unsigned char *p) { return static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8); }
inline uint32_t le32(const unsigned char *p) { return le16(p) | (le16(p + 2) << 16); }
uint32_t bgzf_block_length(const unsigned char *p, uint64_t avail, uint32_t &data_off) {
  if (avail < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return 0;
  const uint32_t xlen = le16(p + 10);
  if (12ull + xlen > avail) return 0;
  for (uint32_t at = 0; at + 4 <= xlen;) {
    const unsigned char *sf = p + 12 + at;
    const uint32_t slen = le16(sf + 2);
    if (sf[0] == 'B' && sf[1] == 'C' && slen == 2 && at + 6 <= xlen) {
      const uint32_t total = le16(sf + 4) + 1;
      data_off = 12 + xlen;
      return total >= data_off + 8 && total <= avail ? total : 0;
    }
    at += 4 + slen;
  }
  return 0;
}
// What a reads file is, told from its first bytes, once: plain text; BGZF (a gzip member whose extra field holds the BC
// subfield -- only the first block's header is checked here, the scan of the blocks checks every one); or a stream: any
// other gzip file, and whatever is not a regular file (a pipe), which one thread reads from front to back.
enum class FileKind { Stream, Bgzf, Plain };
struct InputFile {
  FileKind kind = FileKind::Stream;
  bool regular = false, gzip = false;  // gzip: the two magic bytes (BGZF included)
  uint64_t size = 0;                   // of a regular file
};
InputFile probe_input(const std::string &path) {
  const int fd = ::open(path.c_str(), O_RDONLY);
  if (fd < 0) throw std::runtime_error("cannot open reads file: " + path);
  unsigned char head[512];
  const ssize_t got = ::pread(fd, head, sizeof(head), 0);
  struct stat sb;
  InputFile f;
  f.regular = ::fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode);
  ::close(fd);
  if (!f.regular) return f;
  f.size = static_cast<uint64_t>(sb.st_size);
  f.gzip = got >= 2 && head[0] == 0x1f && head[1] == 0x8b;
  if (!f.gzip) { f.kind = FileKind::Plain; return f; }
  if (got < 18 || head[2] != 8 || !(head[3] & 4)) return f;
  const uint32_t xlen = le16(head + 10);
  for (uint32_t at = 0; at + 6 <= xlen && 12 + at + 6 <= static_cast<uint32_t>(got);) {
    const unsigned char *sf = head + 12 + at;
    if (sf[0] == 'B' && sf[1] == 'C' && le16(sf + 2) == 2) { f.kind = FileKind::Bgzf; break; }
    at += 4 + le16(sf + 2);
  }
  return f;
}
// one thread's inflate state, reset per block
struct BgzfInflater {
  z_stream zs;
  bool live = false;
  ~BgzfInflater() { if (live) inflateEnd(&zs); }
  // block at `p` (whole length `len`, deflate data from `data_off`) -> dst (room for isize bytes); checks size and CRC
  void block(const unsigned char *p, uint32_t len, uint32_t data_off, char *dst, uint32_t isize) {
    if (!live) {
      std::memset(&zs, 0, sizeof(zs));
      if (inflateInit2(&zs, -15) != Z_OK) throw std::runtime_error("inflateInit2 failed");
      live = true;
    }
    else inflateReset(&zs);
    zs.next_in = const_cast<Bytef *>(p + data_off);
    zs.avail_in = len - data_off - 8;
    zs.next_out = reinterpret_cast<Bytef *>(dst);
    zs.avail_out = isize;
    const int rc = inflate(&zs, Z_FINISH);
    if (rc != Z_STREAM_END || zs.total_out != isize) throw std::runtime_error("corrupt BGZF block in the reads file");
    if (static_cast<uint32_t>(crc32(crc32(0L, Z_NULL, 0), reinterpret_cast<const Bytef *>(dst), isize)) != le32(p + len - 8))
      throw std::runtime_error("BGZF block with a wrong checksum in the reads file");
  }
};

// one thread's inflater on a GPU (the C ABI's abm_inflater: its own stream, device buffers and pinned staging), with the
// descriptors and statuses of its current call
struct DeviceBgzf {
  abm_inflater *inf = nullptr;
  std::vector<abm_bgzf_block> blocks;
  std::vector<uint8_t> status;
  DeviceBgzf() = default;
  DeviceBgzf(const DeviceBgzf &) = delete;
  ~DeviceBgzf() { if (inf) abm_inflater_destroy(inf); }
  void open(int device) {
    if (!inf && abm_inflater_create(device, &inf) != 0) throw std::runtime_error(abm_last_error());
  }
  // `blocks` (offsets relative to comp and text) -> text; true: every block inflated, false: see `status`
  bool run(const unsigned char *comp, uint64_t comp_bytes, char *text, uint64_t text_bytes) {
    status.assign(blocks.size(), 0);
    const int rc = abm_inflate_bgzf(inf, comp, comp_bytes, blocks.data(), static_cast<uint32_t>(blocks.size()), text, text_bytes, status.data());
    if (rc != 0 && rc != ABM_ERR_INFLATE) throw std::runtime_error(abm_last_error());
    return rc == 0;
  }
};

// one thread's deflater on a GPU (the C ABI's abm_deflater: its own stream, device buffers and pinned staging)
struct DeviceDeflate {
  abm_deflater *def = nullptr;
  DeviceDeflate() = default;
  DeviceDeflate(const DeviceDeflate &) = delete;
  ~DeviceDeflate() { if (def) abm_deflater_destroy(def); }
  void open(int device) {
    if (!def && abm_deflater_create(device, &def) != 0) throw std::runtime_error(abm_last_error());
  }
  // raw -> BGZF members appended to out (no end-of-file block); their number in n_blocks.  false: the call failed and out
  // is as it was (the caller compresses on the host)
  template <class A, class B> bool run(const A &raw, B &out, uint64_t &n_blocks) {
    const size_t at0 = out.size();
    const uint64_t cap = abm_deflate_bgzf_bound(raw.size(), 0);
    uint64_t n_out = 0;
    out.resize(at0 + cap);
    const int rc = abm_deflate_bgzf(def, raw.data(), raw.size(), 0, &out[at0], cap, &n_out, nullptr, 0, &n_blocks);
    out.resize(at0 + (rc == 0 ? n_out : 0));
    return rc == 0;
  }
};

// one thread's FASTQ parser on a GPU (the C ABI's abm_fastq_parser: its own stream, device buffers and pinned staging), with
// the name table of its current call
struct DeviceParse {
  abm_fastq_parser *par = nullptr;
  std::vector<uint64_t> name_at;
  std::vector<uint32_t> name_len;
  DeviceParse() = default;
  DeviceParse(const DeviceParse &) = delete;
  ~DeviceParse() { if (par) abm_fastq_parser_destroy(par); }
  void open(int device) {
    if (!par && abm_fastq_parser_create(device, &par) != 0) throw std::runtime_error(abm_last_error());
  }
  // text -> names (views into it), blob, off, as parse_raw leaves them.  false: the text has an error or the call failed
  // (the caller parses it on the host, which throws the reference's message or gives its result).  The capacities start
  // from what records look like and follow the call's own figures when it says they were too small.
  bool run(const char *text, size_t text_n, std::vector<NameRef> &names, RawBuf &blob, std::vector<uint64_t> &off) {
    uint64_t recs = text_n / 64 + 16, bytes = text_n / 2 + 64;
    abm_fastq_info info;
    for (int attempt = 0; attempt < 2; ++attempt) {
      blob.clear();
      blob.reserve(bytes);
      off.resize(recs + 1);
      name_at.resize(recs);
      name_len.resize(recs);
      const int rc = abm_fastq_parse(par, text, text_n, g_min_read_len, blob.p, bytes, off.data(), name_at.data(), name_len.data(), recs, &info);
      if (rc == ABM_ERR_CAPACITY && attempt == 0) { recs = info.n_records; bytes = info.blob_bytes; continue; }
      if (rc != 0) return false;
      blob.n = info.blob_bytes;
      off.resize(info.n_records + 1);
      names.resize(info.n_records);
      for (uint64_t j = 0; j < info.n_records; ++j) names[j] = NameRef{text + name_at[j], name_len[j]};
      return true;
    }
    return false;
  }
};

// a mapped input file that shrinks under the run (truncated, a network file system losing it) faults with SIGBUS
void install_sigbus_handler() {
  struct sigaction sa;
  std::memset(&sa, 0, sizeof(sa));
  sa.sa_handler = [](int) {
    static const char msg[] = "abismal-amd: an input file changed or became unreadable while it was being read (SIGBUS on its mapping)\n";
    (void)!::write(2, msg, sizeof(msg) - 1);
    ::_exit(EXIT_FAILURE);
  };
  ::sigaction(SIGBUS, &sa, nullptr);
}

// The CPU time the container gives this process (CFS bandwidth control: cgroup v2 cpu.max, v1 cpu.cfs_quota_us): a pod
// of an 8-GPU node typically gets its share of the cores (16 of 128 on the box this was measured on) although it sees
// all 256 hardware threads.  More runnable threads than that do not run more: they burn the period's quota in its first
// milliseconds and the whole process is frozen for the rest of it (profiles/r04_trace_parts8_t64.log: every thread
// stalled 77 of every 100 ms) -- which is what made round 3's host pipeline "anti-scale" with its thread count.
struct CpuQuota {
  double cpus = 0;          // 0 = unlimited / unknown
  std::string stat_path;    // cpu.stat of the same cgroup
  bool v2 = false;
  static bool read_file(const std::string &path, std::string &out) {
    std::ifstream f(path);
    if (!f) return false;
    std::stringstream ss;
    ss << f.rdbuf();
    out = ss.str();
    return true;
  }
  CpuQuota() {
    std::string own, v1_path, v2_path;
    if (read_file("/proc/self/cgroup", own)) {
      std::istringstream is(own);
      std::string line;
      while (std::getline(is, line)) {
        const size_t a = line.find(':'), b = line.find(':', a + 1);
        if (a == std::string::npos || b == std::string::npos) continue;
        const std::string ctl = line.substr(a + 1, b - a - 1), path = line.substr(b + 1);
        if (ctl.empty()) v2_path = path;
        else if (("," + ctl + ",").find(",cpu,") != std::string::npos) v1_path = path;
      }
    }
    std::string s;
    for (const std::string &dir : {std::string("/sys/fs/cgroup") + v2_path, std::string("/sys/fs/cgroup")})
      if (cpus == 0 && read_file(dir + "/cpu.max", s)) {
        long long q = 0, per = 0;
        if (std::sscanf(s.c_str(), "%lld %lld", &q, &per) == 2 && q > 0 && per > 0) { cpus = static_cast<double>(q) / per; stat_path = dir + "/cpu.stat"; v2 = true; }
        else if (s.compare(0, 3, "max") == 0) { stat_path = dir + "/cpu.stat"; v2 = true; break; }
      }
    if (stat_path.empty())
      for (const std::string &dir : {std::string("/sys/fs/cgroup/cpu") + v1_path, std::string("/sys/fs/cgroup/cpu")}) {
        std::string qs, ps;
        if (read_file(dir + "/cpu.cfs_quota_us", qs) && read_file(dir + "/cpu.cfs_period_us", ps)) {
          const long long q = std::atoll(qs.c_str()), per = std::atoll(ps.c_str());
          if (q > 0 && per > 0) cpus = static_cast<double>(q) / per;
          stat_path = dir + "/cpu.stat";
          break;
        }
      }
  }
  // periods in which the cgroup was throttled so far, and for how long (seconds)
  void throttled(uint64_t &periods, double &seconds) const {
    periods = 0; seconds = 0;
    std::string s;
    if (stat_path.empty() || !read_file(stat_path, s)) return;
    std::istringstream is(s);
    std::string key;
    unsigned long long v = 0;
    while (is >> key >> v) {
      if (key == "nr_throttled") periods = v;
      else if (key == "throttled_usec") seconds = static_cast<double>(v) * 1e-6;
      else if (key == "throttled_time") seconds = static_cast<double>(v) * 1e-9;
    }
  }
};

unsigned default_build_threads() {
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const CpuQuota q;
  return q.cpus > 0 ? std::min(hw, std::max(1u, static_cast<unsigned>(q.cpus + 0.5))) : hw;
}

}  // namespace
