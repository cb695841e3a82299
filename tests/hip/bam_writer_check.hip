// GPU test program (built and run by tests/test_gpu_bam_records.py): the device's BAM piece writer (BamWriter,
// abm_sam.hpp) alone, on synthetic fields that mapping on a small genome cannot reach -- every NM type, positions and
// reference lengths either side of each bin level, every length's packing on both strands, every byte value as a base,
// 1 to 50 CIGAR ops, a piece beyond its slot -- against a host restatement of put_bam_record (abm_cli_records.hpp) without
// the name.  One launch, one wave per case.  Prints "OK <n cases>" or the first mismatch.
#include "../../abismal_amd/csrc/abm_sam.hpp"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace abm;

constexpr u32 kSlot = 1792;  // >= the longest piece here: 36 + 4 * 50 + 512 + 1024 + 9
struct Case {
  BamFields f;
  u32 n_ops, L, rc, seq_at, cap;
};

__global__ __launch_bounds__(64) void run(const Case *cases, const u32 *ops, const char *blob, u8 *out, u32 *len) {
  __shared__ __align__(16) u8 line[kSlot];
  const Case c = cases[blockIdx.x];
  const BamWriter o{line, c.cap};
  const u32 n = o.put(c.f, ops + blockIdx.x * kSeCap, c.n_ops, blob + c.seq_at, c.L, c.rc != 0);
  if (n != 0xFFFFFFFFu) o.flush(reinterpret_cast<u32 *>(out + static_cast<size_t>(blockIdx.x) * kSlot), n);
  if (threadIdx.x == 0) len[blockIdx.x] = n;
}

// ---- the host's record, field by field (put_bam_record without the name, block_size without it) ----
static int reg2bin(long long beg, long long end) {
  --end;
  if (beg >> 14 == end >> 14) return static_cast<int>(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return static_cast<int>(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return static_cast<int>(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return static_cast<int>(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return static_cast<int>(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}
static unsigned code4(unsigned char c, bool rc) {
  static const char nt16[] = "=ACMGRSVTWYHKDBN";
  char shown;
  if (rc) shown = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
  else {
    const char u = (c >= 'a' && c <= 'z') ? static_cast<char>(c - 32) : static_cast<char>(c);
    shown = (u && std::strchr(nt16, u)) ? u : 'N';
  }
  return static_cast<unsigned>(std::strchr(nt16, shown) - nt16);
}
static std::vector<u8> host_piece(const Case &c, const u32 *ops, const char *seq) {
  std::vector<u8> o;
  auto le32 = [&](u32 v) { for (int k = 0; k < 4; ++k) o.push_back(static_cast<u8>(v >> (8 * k))); };
  auto le16 = [&](u32 v) { o.push_back(static_cast<u8>(v)); o.push_back(static_cast<u8>(v >> 8)); };
  le32(0);
  le32(static_cast<u32>(c.f.refid));
  le32(c.f.pos);
  o.push_back(0);
  o.push_back(255);
  le16(static_cast<u32>(reg2bin(c.f.pos, static_cast<long long>(c.f.pos) + (c.f.reflen ? c.f.reflen : 1))));
  le16(c.n_ops);
  le16(c.f.flag);
  le32(c.L);
  le32(static_cast<u32>(c.f.next_refid));
  le32(c.f.next_refid < 0 ? 0xFFFFFFFFu : c.f.next_pos);
  le32(static_cast<u32>(c.f.tlen));
  for (u32 k = 0; k < c.n_ops; ++k) le32(ops[k]);
  const unsigned char *s = reinterpret_cast<const unsigned char *>(seq);
  for (u32 i = 0; i < c.L; i += 2) {
    const unsigned hi = code4(c.rc ? s[c.L - 1 - i] : s[i], c.rc != 0);
    const unsigned lo = i + 1 < c.L ? code4(c.rc ? s[c.L - 2 - i] : s[i + 1], c.rc != 0) : 0;
    o.push_back(static_cast<u8>(hi << 4 | lo));
  }
  for (u32 i = 0; i < c.L; ++i) o.push_back(0xFF);
  const int nm = c.f.nm;
  o.push_back('N'); o.push_back('M');
  if (nm >= 0 && nm <= 255) { o.push_back('C'); o.push_back(static_cast<u8>(nm)); }
  else if (nm >= 0) { o.push_back('S'); le16(static_cast<u32>(nm)); }
  else if (nm >= -128) { o.push_back('c'); o.push_back(static_cast<u8>(nm)); }
  else { o.push_back('s'); le16(static_cast<u32>(static_cast<uint16_t>(static_cast<int16_t>(nm)))); }
  o.push_back('C'); o.push_back('V'); o.push_back('A'); o.push_back(c.f.a_rich ? 'A' : 'T');
  const u32 bs = static_cast<u32>(o.size() - 4);
  for (int k = 0; k < 4; ++k) o[k] = static_cast<u8>(bs >> (8 * k));
  return o;
}

int main() {
  std::vector<Case> cases;
  std::vector<u32> ops;
  std::string blob;
  u32 rng = 12345u;
  auto draw = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
  auto add = [&](BamFields f, u32 n_ops, const std::string &seq, bool rc, u32 cap = kSlot) {
    Case c{f, n_ops, static_cast<u32>(seq.size()), rc ? 1u : 0u, static_cast<u32>(blob.size()), cap};
    blob += seq;
    for (u32 k = 0; k < kSeCap; ++k) ops.push_back(k < n_ops ? ((1 + draw() % 300) << 4 | (draw() % 9)) : 0xDEADBEEFu);
    cases.push_back(c);
  };
  auto random_seq = [&](u32 L) {
    std::string s(L, 'A');
    for (u32 i = 0; i < L; ++i) { const u32 d = draw() % 64; s[i] = d < 60 ? "ACGT"[d & 3] : "NRyn"[d & 3]; }
    return s;
  };
  const BamFields base{3, 1000u, 100u, 0x10u, -1, 0u, 0, 2, false};
  // NM: every type and its limits
  for (int nm : {-129, -128, -1, 0, 255, 256, 32767, -32768, 1, 127, 128}) { BamFields f = base; f.nm = nm; f.a_rich = (nm & 1) != 0; add(f, 1, random_seq(10), false); }
  // bin: positions and reference lengths either side of every level's boundary, a reference length of 0
  for (int k : {14, 17, 20, 23, 26})
    for (int dp : {-101, -2, -1, 0, 1})
      for (u32 rl : {0u, 1u, 2u, 3u, 100u, 101u, 102u}) { BamFields f = base; f.pos = (1u << k) + dp; f.reflen = rl; add(f, 2, random_seq(7), true); }
  for (u32 pos : {0u, 1u, 0x7FFFFFFFu, 0xFFFFFF00u}) { BamFields f = base; f.pos = pos; f.reflen = 150; add(f, 1, random_seq(5), false); }
  // a proper pair's fields (mate, negative TLEN), flags
  { BamFields f = base; f.flag = 0x1 | 0x2 | 0x80 | 0x10 | 0x100; f.next_refid = 3; f.next_pos = 77777u; f.tlen = -412; add(f, 3, random_seq(150), true); f.tlen = 412; f.refid = 0; f.next_refid = 0; add(f, 3, random_seq(151), false); }
  // lengths: odd and even, the lane rounds at 64 and 128 bases / packed bytes, the longest
  for (u32 L = 1; L <= 132; ++L) for (int rc = 0; rc < 2; ++rc) add(base, 1 + L % 4, random_seq(L), rc != 0);
  for (u32 L : {255u, 256u, 257u, 1023u, 1024u}) for (int rc = 0; rc < 2; ++rc) add(base, 4, random_seq(L), rc != 0);
  // every byte value as a base, at even and odd places
  { std::string all(256, 'A'); for (int c = 0; c < 256; ++c) all[c] = static_cast<char>(c);
    for (int rc = 0; rc < 2; ++rc) { add(base, 1, all, rc != 0); add(base, 1, "C" + all, rc != 0); } }
  // 1 .. 50 CIGAR ops
  for (u32 n = 1; n <= kSeCap; ++n) add(base, n, random_seq(20 + n % 3), (n & 1) != 0);
  // a piece one byte beyond its slot, and one that fills it exactly (36 + 4 + 50 + 100 + 8 = 198)
  add(base, 1, random_seq(100), false, 197);
  add(base, 1, random_seq(100), false, 198);

  const size_t n = cases.size();
  Case *dc; u32 *dops, *dlen; char *dblob; u8 *dout;
  if (hipMalloc(&dc, n * sizeof(Case)) != hipSuccess || hipMalloc(&dops, ops.size() * 4) != hipSuccess || hipMalloc(&dblob, blob.size()) != hipSuccess ||
      hipMalloc(&dout, n * kSlot) != hipSuccess || hipMalloc(&dlen, n * 4) != hipSuccess) { printf("FAIL alloc\n"); return 1; }
  hipMemcpy(dc, cases.data(), n * sizeof(Case), hipMemcpyHostToDevice);
  hipMemcpy(dops, ops.data(), ops.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(dblob, blob.data(), blob.size(), hipMemcpyHostToDevice);
  hipMemset(dout, 0xAB, n * kSlot);
  hipLaunchKernelGGL(run, dim3(static_cast<unsigned>(n)), dim3(64), 0, 0, dc, dops, dblob, dout, dlen);
  if (hipDeviceSynchronize() != hipSuccess) { printf("FAIL launch\n"); return 1; }
  std::vector<u8> out(n * kSlot);
  std::vector<u32> len(n);
  hipMemcpy(out.data(), dout, out.size(), hipMemcpyDeviceToHost);
  hipMemcpy(len.data(), dlen, n * 4, hipMemcpyDeviceToHost);
  for (size_t i = 0; i < n; ++i) {
    const Case &c = cases[i];
    const std::vector<u8> want = host_piece(c, ops.data() + i * kSeCap, blob.data() + c.seq_at);
    const u8 *got = out.data() + i * kSlot;
    if (want.size() > c.cap) {
      if (len[i] != 0xFFFFFFFFu || got[0] != 0xAB) { printf("FAIL case %zu: a piece of %zu bytes in a slot of %u was written (length %u)\n", i, want.size(), c.cap, len[i]); return 1; }
      continue;
    }
    if (len[i] != want.size()) { printf("FAIL case %zu (L %u, %u ops, nm %d): length %u, the host's %zu\n", i, c.L, c.n_ops, c.f.nm, len[i], want.size()); return 1; }
    for (size_t k = 0; k < want.size(); ++k)
      if (got[k] != want[k]) { printf("FAIL case %zu (L %u, rc %u, %u ops, nm %d, pos %u, reflen %u): byte %zu is %02x, the host's %02x\n", i, c.L, c.rc, c.n_ops, c.f.nm, c.f.pos, c.f.reflen, k, got[k], want[k]); return 1; }
    for (size_t k = (want.size() + 3) / 4 * 4; k < kSlot; ++k)
      if (got[k] != 0xAB) { printf("FAIL case %zu: byte %zu beyond the piece's last word was written\n", i, k); return 1; }
  }
  printf("OK %zu cases\n", n);
  return 0;
}
