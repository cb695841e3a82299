// abismal-amd, record writing: SAM lines and BAM records (from a hit's fields, or from what the kernels wrote), the BGZF
// deflater, the statistics.  Part of abm_cli.cpp's one translation unit: everything here has internal linkage.
#pragma once
#include "../../include/abismal_amd.h"

#include <zlib.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

struct NameRef {  // a read name inside its slice's FASTQ text
  const char *p;
  uint32_t n;
};
struct Stats { 
  uint64_t v[6] = {0, 0, 0, 0, 0, 0};  // total, unique, ambiguous, skipped, edits, bases
  void tally(bool empty_read, const abm_hit &h, bool count_ambig_error, uint32_t bases);
  std::string yaml(const std::string &label) const;
  std::string json() const;
};
struct Stats3 { Stats s[3]; };  // SE: s[0]; PE: pairs, read1, read2

// ---- SAM text (format_se / format_pe, src/abismal.cpp:481-545, :648-773) -------
struct Chroms {
  std::vector<std::string> names;
  std::vector<uint32_t> starts;
  bool locate(uint32_t pos, uint32_t reflen, int32_t &chrom, uint32_t &off) const {
    auto it = std::upper_bound(starts.begin(), starts.end(), pos);
    if (it == starts.begin()) return false;
    --it;
    chrom = static_cast<int32_t>(it - starts.begin());
    off = pos - starts[chrom];
    return pos + reflen <= starts[chrom + 1];
  }
};

uint32_t ref_len(const uint32_t *c, size_t n) {
  uint32_t r = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t op = c[i] & 15u;
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) r += c[i] >> 4;
  }
  return r;
}

// SEQ as htslib prints it after its 4-bit round trip: IUPAC upper-cased, everything else N;
// the reverse-strand variant complements first (src/common.hpp:28-44: non-ACGT -> N)
struct SeqTables {
  char fwd[256], rc[256];
  SeqTables() {
    static const char ok[] = "=ACMGRSVTWYHKDBN";
    for (int c = 0; c < 256; ++c) {
      const char u = static_cast<char>(std::toupper(c));
      fwd[c] = (u && std::strchr(ok, u)) ? u : 'N';
      rc[c] = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
    }
  }
};
const SeqTables kSeq;
// SEQ of a record: the tables above applied to a whole read.  A read is almost always upper-case A, C, G, T, N, so the
// forward form is a copy wherever 32 bytes at a time are nothing else, and the reverse-complement form -- A <-> T,
// C <-> G, everything else N, back to front -- is four compares and blends per 32 bytes; both fall back to the tables
// for a read's last bytes and for anything unusual, and are the tables themselves on a CPU without AVX2.  (SEQ was the
// costliest field of a line: a table look-up per base.)
#if defined(__x86_64__)
__attribute__((target("avx2"))) static void seq_forward_avx2(char *w, const char *s, size_t n) {
  size_t i = 0;
  const __m256i a = _mm256_set1_epi8('A'), c = _mm256_set1_epi8('C'), g = _mm256_set1_epi8('G'), t = _mm256_set1_epi8('T'), nn = _mm256_set1_epi8('N');
  for (; i + 32 <= n; i += 32) {
    const __m256i v = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(s + i));
    const __m256i ok = _mm256_or_si256(_mm256_or_si256(_mm256_or_si256(_mm256_cmpeq_epi8(v, a), _mm256_cmpeq_epi8(v, c)),
                                                       _mm256_or_si256(_mm256_cmpeq_epi8(v, g), _mm256_cmpeq_epi8(v, t))), _mm256_cmpeq_epi8(v, nn));
    if (static_cast<uint32_t>(_mm256_movemask_epi8(ok)) == 0xFFFFFFFFu) _mm256_storeu_si256(reinterpret_cast<__m256i *>(w + i), v);
    else for (size_t k = i; k < i + 32; ++k) w[k] = kSeq.fwd[static_cast<unsigned char>(s[k])];
  }
  for (; i < n; ++i) w[i] = kSeq.fwd[static_cast<unsigned char>(s[i])];
}
__attribute__((target("avx2"))) static void seq_revcomp_avx2(char *w, const char *s, size_t n) {
  // w[i] = rc[s[n - 1 - i]]: 32 bytes from the back of s at a time, reversed, then mapped
  const __m256i rev = _mm256_setr_epi8(15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0);
  const __m256i a = _mm256_set1_epi8('A'), c = _mm256_set1_epi8('C'), g = _mm256_set1_epi8('G'), t = _mm256_set1_epi8('T'), nn = _mm256_set1_epi8('N');
  size_t i = 0;
  for (; i + 32 <= n; i += 32) {
    __m256i v = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(s + n - 32 - i));
    v = _mm256_permute2x128_si256(_mm256_shuffle_epi8(v, rev), _mm256_shuffle_epi8(v, rev), 0x01);  // bytes reversed across the whole register
    __m256i o = nn;
    o = _mm256_blendv_epi8(o, t, _mm256_cmpeq_epi8(v, a));
    o = _mm256_blendv_epi8(o, g, _mm256_cmpeq_epi8(v, c));
    o = _mm256_blendv_epi8(o, c, _mm256_cmpeq_epi8(v, g));
    o = _mm256_blendv_epi8(o, a, _mm256_cmpeq_epi8(v, t));
    _mm256_storeu_si256(reinterpret_cast<__m256i *>(w + i), o);
  }
  for (; i < n; ++i) w[i] = kSeq.rc[static_cast<unsigned char>(s[n - 1 - i])];
}
static const bool kHaveAvx2 = __builtin_cpu_supports("avx2");
static const bool g_scalar_seq = std::getenv("ABM_CLI_SCALAR_SEQ") != nullptr;  // (tests: the table form on a CPU that has AVX2)
#else
static const bool kHaveAvx2 = false;
#endif
inline void put_seq(char *w, const char *s, size_t n, bool rc) {
#if defined(__x86_64__)
  if (kHaveAvx2 && !g_scalar_seq) { if (rc) seq_revcomp_avx2(w, s, n); else seq_forward_avx2(w, s, n); return; }
#endif
  if (rc) for (size_t i = 0; i < n; ++i) w[i] = kSeq.rc[static_cast<unsigned char>(s[n - 1 - i])];
  else for (size_t i = 0; i < n; ++i) w[i] = kSeq.fwd[static_cast<unsigned char>(s[i])];
}

template <class S> inline void put_uint(S &o, uint64_t v) {
  char buf[24];
  int k = 24;
  do { buf[--k] = static_cast<char>('0' + v % 10); v /= 10; } while (v);
  o.append(buf + k, static_cast<size_t>(24 - k));
}
template <class S> inline void put_int(S &o, int64_t v) {
  if (v < 0) { o += '-'; put_uint(o, static_cast<uint64_t>(-v)); }
  else put_uint(o, static_cast<uint64_t>(v));
}

struct Record {
  const NameRef *name;
  uint16_t flag;
  int32_t tid, mtid;
  uint32_t pos, mpos;
  int tlen;
  const uint32_t *cig;
  size_t n_cig;
  const char *seq;
  size_t n_seq;
  bool rc;
  int nm;
  char cv;
};

template <class S> void put_bam_record(S &o, const Record &r);
thread_local bool t_bam = false;  // formatter threads switch put_record to BAM encoding
// digits of v at w, returns one past them
inline char *write_uint(char *w, uint64_t v) {
  char buf[24];
  int k = 24;
  do { buf[--k] = static_cast<char>('0' + v % 10); v /= 10; } while (v);
  std::memcpy(w, buf + k, static_cast<size_t>(24 - k));
  return w + (24 - k);
}
template <class S> void put_record(S &o, const Chroms &ch, const Record &r) {
  if (t_bam) { put_bam_record(o, r); return; }
  // one reservation for the whole line (its longest possible form), then plain pointer writes: a line is a dozen short
  // fields, and appending them one by one through the buffer's capacity checks was a third of the formatting time
  const std::string &chrom = ch.names[r.tid + 1];
  const std::string *mate = r.mtid < 0 || r.mtid == r.tid ? nullptr : &ch.names[r.mtid + 1];
  const size_t at0 = o.size();
  o.resize(at0 + r.name->n + chrom.size() + (mate ? mate->size() : 1) + r.n_cig * 12 + r.n_seq + 128);
  char *w = &o[at0];
  std::memcpy(w, r.name->p, r.name->n); w += r.name->n; *w++ = '\t';
  w = write_uint(w, r.flag); *w++ = '\t';
  std::memcpy(w, chrom.data(), chrom.size()); w += chrom.size(); *w++ = '\t';
  w = write_uint(w, static_cast<uint64_t>(r.pos) + 1);
  std::memcpy(w, "\t255\t", 5); w += 5;
  for (size_t i = 0; i < r.n_cig; ++i) { w = write_uint(w, r.cig[i] >> 4); *w++ = "MIDNSHP=XB"[std::min<uint32_t>(r.cig[i] & 15u, 9)]; }
  *w++ = '\t';
  if (r.mtid < 0) { std::memcpy(w, "*\t0\t", 4); w += 4; }
  else {
    if (!mate) *w++ = '=';
    else { std::memcpy(w, mate->data(), mate->size()); w += mate->size(); }
    *w++ = '\t'; w = write_uint(w, static_cast<uint64_t>(r.mpos) + 1); *w++ = '\t';
  }
  if (r.tlen < 0) { *w++ = '-'; w = write_uint(w, static_cast<uint64_t>(-static_cast<int64_t>(r.tlen))); }
  else w = write_uint(w, static_cast<uint64_t>(r.tlen));
  *w++ = '\t';
  put_seq(w, r.seq, r.n_seq, r.rc);
  w += r.n_seq;
  std::memcpy(w, "\t*\tNM:i:", 8); w += 8;
  if (r.nm < 0) { *w++ = '-'; w = write_uint(w, static_cast<uint64_t>(-static_cast<int64_t>(r.nm))); }
  else w = write_uint(w, static_cast<uint64_t>(r.nm));
  std::memcpy(w, "\tCV:A:", 6); w += 6;
  *w++ = r.cv; *w++ = '\n';
  o.resize(static_cast<size_t>(w - &o[0]));
}

// ---- BAM (-B): the same records as binary BAM in BGZF blocks (SAM spec 4.2 / 4.1) ------------------
// htslib's bam_set1 + bam_aux_update_int("NM") + bam_aux_append("CV",'A') in the reference
// (src/abismal.cpp:513-543); quality is absent (0xFF), MAPQ 255.
template <class S> inline void put_le32(S &o, uint32_t v) { char b[4] = {static_cast<char>(v), static_cast<char>(v >> 8), static_cast<char>(v >> 16), static_cast<char>(v >> 24)}; o.append(b, 4); }
template <class S> inline void put_le16(S &o, uint16_t v) { char b[2] = {static_cast<char>(v), static_cast<char>(v >> 8)}; o.append(b, 2); }
inline int reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return static_cast<int>(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return static_cast<int>(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return static_cast<int>(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return static_cast<int>(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return static_cast<int>(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}
// 4-bit BAM base codes of what SEQ shows (kSeq.fwd / kSeq.rc, then htslib's seq_nt16_table)
struct Seq4Tables {
  unsigned char fwd[256], rc[256];
  Seq4Tables() {
    static const char nt16[] = "=ACMGRSVTWYHKDBN";
    for (int c = 0; c < 256; ++c) {
      const char *qf = std::strchr(nt16, kSeq.fwd[c]), *qr = std::strchr(nt16, kSeq.rc[c]);
      fwd[c] = static_cast<unsigned char>(qf && kSeq.fwd[c] ? qf - nt16 : 15);
      rc[c] = static_cast<unsigned char>(qr && kSeq.rc[c] ? qr - nt16 : 15);
    }
  }
};
const Seq4Tables kSeq4;
template <class S> void put_bam_record(S &o, const Record &r) {
  // (one reservation for the record, then pointer writes, as for the SAM line)
  const size_t start = o.size();
  const size_t l_seq = r.n_seq, packed = (l_seq + 1) / 2;
  o.resize(start + 36 + r.name->n + 1 + 4 * r.n_cig + packed + l_seq + 16);
  unsigned char *w = reinterpret_cast<unsigned char *>(&o[start]);
  auto le32w = [&](uint32_t v) { w[0] = static_cast<unsigned char>(v); w[1] = static_cast<unsigned char>(v >> 8); w[2] = static_cast<unsigned char>(v >> 16); w[3] = static_cast<unsigned char>(v >> 24); w += 4; };
  auto le16w = [&](uint32_t v) { w[0] = static_cast<unsigned char>(v); w[1] = static_cast<unsigned char>(v >> 8); w += 2; };
  unsigned char *const size_at = w;
  le32w(0);  // block_size, patched below
  le32w(static_cast<uint32_t>(r.tid));
  le32w(r.pos);
  const uint32_t rl = ref_len(r.cig, r.n_cig);
  *w++ = static_cast<unsigned char>(r.name->n + 1);
  *w++ = 255;
  le16w(static_cast<uint32_t>(reg2bin(r.pos, static_cast<int64_t>(r.pos) + (rl ? rl : 1))));
  le16w(static_cast<uint32_t>(r.n_cig));
  le16w(r.flag);
  le32w(static_cast<uint32_t>(l_seq));
  le32w(static_cast<uint32_t>(r.mtid));
  le32w(r.mtid < 0 ? 0xFFFFFFFFu : r.mpos);
  le32w(static_cast<uint32_t>(r.tlen));
  std::memcpy(w, r.name->p, r.name->n); w += r.name->n; *w++ = 0;
  for (size_t i = 0; i < r.n_cig; ++i) le32w(r.cig[i]);
  const unsigned char *s = reinterpret_cast<const unsigned char *>(r.seq);
  if (r.rc)
    for (size_t i = 0; i < l_seq; i += 2)
      *w++ = static_cast<unsigned char>((kSeq4.rc[s[l_seq - 1 - i]] << 4) | (i + 1 < l_seq ? kSeq4.rc[s[l_seq - 2 - i]] : 0));
  else
    for (size_t i = 0; i < l_seq; i += 2)
      *w++ = static_cast<unsigned char>((kSeq4.fwd[s[i]] << 4) | (i + 1 < l_seq ? kSeq4.fwd[s[i + 1]] : 0));
  std::memset(w, 0xFF, l_seq); w += l_seq;
  *w++ = 'N'; *w++ = 'M';  // bam_aux_update_int: smallest type that holds the value
  if (r.nm >= 0 && r.nm <= 255) { *w++ = 'C'; *w++ = static_cast<unsigned char>(r.nm); }
  else if (r.nm >= 0) { *w++ = 'S'; le16w(static_cast<uint32_t>(r.nm)); }
  else if (r.nm >= -128) { *w++ = 'c'; *w++ = static_cast<unsigned char>(r.nm); }
  else { *w++ = 's'; le16w(static_cast<uint32_t>(static_cast<uint16_t>(static_cast<int16_t>(r.nm)))); }
  *w++ = 'C'; *w++ = 'V'; *w++ = 'A'; *w++ = static_cast<unsigned char>(r.cv);
  const size_t end = static_cast<size_t>(reinterpret_cast<char *>(w) - &o[0]);
  const uint32_t bs = static_cast<uint32_t>(end - start - 4);
  size_at[0] = static_cast<unsigned char>(bs); size_at[1] = static_cast<unsigned char>(bs >> 8); size_at[2] = static_cast<unsigned char>(bs >> 16); size_at[3] = static_cast<unsigned char>(bs >> 24);
  o.resize(end);
}
// A record the kernels wrote (abismal_amd.h): SAM text after QNAME -- the name goes in front -- or, with -B, a BAM piece:
// its 36 fixed bytes, block_size and l_read_name taking the name in, then the name and a NUL, then the rest of the piece.
// Byte for byte what put_record / put_bam_record make of the same read.
template <class S> inline void put_device_record(S &o, bool bam, const NameRef &name, const char *tail, uint32_t len) {
  const size_t at0 = o.size();
  if (!bam) {
    o.resize(at0 + name.n + len);
    std::memcpy(&o[at0], name.p, name.n);
    std::memcpy(&o[at0 + name.n], tail, len);
    return;
  }
  o.resize(at0 + len + name.n + 1);
  unsigned char *w = reinterpret_cast<unsigned char *>(&o[at0]);
  std::memcpy(w, tail, 36);
  const uint32_t bs = (static_cast<uint32_t>(w[0]) | static_cast<uint32_t>(w[1]) << 8 | static_cast<uint32_t>(w[2]) << 16 | static_cast<uint32_t>(w[3]) << 24) + static_cast<uint32_t>(name.n + 1);
  w[0] = static_cast<unsigned char>(bs); w[1] = static_cast<unsigned char>(bs >> 8); w[2] = static_cast<unsigned char>(bs >> 16); w[3] = static_cast<unsigned char>(bs >> 24);
  w[12] = static_cast<unsigned char>(name.n + 1);
  std::memcpy(w + 36, name.p, name.n);
  w[36 + name.n] = 0;
  std::memcpy(w + 37 + name.n, tail + 36, len - 36);
}
// raw bytes -> BGZF blocks (each an independent gzip member with the BC extra field)
int g_bgzf_level = 1;  // deflate level of BAM output (-z): 1 = the fast encoder below, 0 = stored, 2..9 = zlib; decoded content is the same at every level
// ---- a fast deflate for BGZF blocks (-z 1, the default) ---------------------------------------------------------------
// zlib at level 1 costs 1.15 us of CPU per 100-base record (BAM through 16 CPUs: 13.6 M reads/s, profiles/r04_host_ceiling.log)
// -- more than everything else the host does per read, six times over.  A BAM record stream is an easy input: runs (the
// 0xFF of absent qualities), fields repeated from the record before, 4-bit sequence that does not compress.  This encoder
// takes one greedy match per position from a single-probe hash of the last occurrence of each 4-byte string and writes
// ONE block with the fixed Huffman code (RFC 1951 3.2.6: no trees to build or ship); whatever inflates it gets the same
// bytes back.  Returns the compressed size, or 0 if `cap` does not suffice (the caller then stores the block).
struct FastDeflate {
  // fixed code, bit-reversed for the LSB-first stream: literal / length symbol -> (code, bits); length -> (symbol, extra)
  uint16_t lit_code[288];
  uint8_t lit_bits[288];
  uint16_t len_sym[259];
  uint8_t len_extra_bits[259];
  uint16_t len_extra_val[259];
  uint8_t dist_sym_small[513];  // distances 1..512 -> symbol; beyond: by the distance's top bits
  static uint32_t rev(uint32_t v, int n) { uint32_t r = 0; for (int i = 0; i < n; ++i) { r = (r << 1) | (v & 1u); v >>= 1; } return r; }
  FastDeflate() {
    for (int s = 0; s < 288; ++s) {
      uint32_t code; int bits;
      if (s < 144) { code = 0x30 + s; bits = 8; }
      else if (s < 256) { code = 0x190 + (s - 144); bits = 9; }
      else if (s < 280) { code = s - 256; bits = 7; }
      else { code = 0xC0 + (s - 280); bits = 8; }
      lit_code[s] = static_cast<uint16_t>(rev(code, bits));
      lit_bits[s] = static_cast<uint8_t>(bits);
    }
    static const uint16_t base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    for (int len = 3; len <= 258; ++len) {
      int k = 28;
      while (base[k] > len) --k;
      if (len == 258) k = 28;
      len_sym[len] = static_cast<uint16_t>(257 + k);
      len_extra_bits[len] = extra[k];
      len_extra_val[len] = static_cast<uint16_t>(len - base[k]);
    }
    for (int d = 1; d <= 512; ++d) dist_sym_small[d] = static_cast<uint8_t>(dist_symbol_slow(static_cast<uint32_t>(d)));
  }
  static int dist_symbol_slow(uint32_t d) {
    static const uint16_t base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    int k = 29;
    while (base[k] > d) --k;
    return k;
  }
  size_t operator()(const unsigned char *src, size_t n, unsigned char *dst, size_t cap, uint16_t *table /*[1 << 13], zeroed by this call*/) const {
    static const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static const uint8_t dextra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    if (n > 0xFFFF || cap < 16) return 0;
    std::memset(table, 0, sizeof(uint16_t) << 13);
    uint64_t acc = 0;
    int nbits = 0;
    unsigned char *out = dst, *const out_end = dst + cap - 16;
    auto put = [&](uint32_t v, int b) {
      acc |= static_cast<uint64_t>(v) << nbits;
      nbits += b;
      if (nbits >= 32) { std::memcpy(out, &acc, 4); out += 4; acc >>= 32; nbits -= 32; }
    };
    put(1, 1);  // BFINAL
    put(1, 2);  // BTYPE = 01, fixed Huffman
    size_t i = 0;
    const size_t last_hashable = n >= 4 ? n - 4 : 0;
    while (i < n) {
      if (out > out_end) return 0;
      size_t mlen = 0, mdist = 0;
      if (n >= 4 && i <= last_hashable) {
        uint32_t w;
        std::memcpy(&w, src + i, 4);
        const uint32_t h = (w * 2654435761u) >> 19;
        const size_t cand = table[h];  // position + 1 of the last string with this hash; 0 = none
        table[h] = static_cast<uint16_t>(i + 1);
        if (cand != 0) {
          const size_t p = cand - 1;
          uint32_t v;
          std::memcpy(&v, src + p, 4);
          if (v == w && i - p <= 32768) {
            const size_t lim = std::min<size_t>(258, n - i);
            size_t l = 4;
            while (l + 8 <= lim) {
              uint64_t a, b;
              std::memcpy(&a, src + p + l, 8);
              std::memcpy(&b, src + i + l, 8);
              if (a != b) { l += static_cast<size_t>(__builtin_ctzll(a ^ b) >> 3); break; }
              l += 8;
            }
            if (l + 8 > lim) while (l < lim && src[p + l] == src[i + l]) ++l;
            mlen = std::min(l, lim);
            mdist = i - p;
          }
        }
      }
      if (mlen >= 4) {
        const uint32_t ls = len_sym[mlen];
        put(lit_code[ls], lit_bits[ls]);
        if (len_extra_bits[mlen]) put(len_extra_val[mlen], len_extra_bits[mlen]);
        const int ds = mdist <= 512 ? dist_sym_small[mdist] : dist_symbol_slow(static_cast<uint32_t>(mdist));
        put(rev(static_cast<uint32_t>(ds), 5), 5);
        if (dextra[ds]) put(static_cast<uint32_t>(mdist - dbase[ds]), dextra[ds]);
        // (the strings inside the match are not entered into the table: the next record repeats this one's fields at
        // the positions where matches begin)
        i += mlen;
      }
      else {
        put(lit_code[src[i]], lit_bits[src[i]]);
        ++i;
      }
    }
    put(lit_code[256], lit_bits[256]);  // end of block
    while (nbits > 0) { if (out >= dst + cap) return 0; *out++ = static_cast<unsigned char>(acc); acc >>= 8; nbits -= 8; }
    return static_cast<size_t>(out - dst);
  }
};
const FastDeflate kFastDeflate;

// One deflate state and one block buffer per thread, reset per block: deflateInit2 allocates a quarter of a megabyte,
// and a hundred formatter threads doing that once per 64 KB block spent six times their compression time waiting on
// the allocator (profiles/r04_host_ceiling.log: -B busy 384 s for 60 s of CPU).
struct BgzfDeflater {
  z_stream zs;
  bool live = false;
  int level = -2;
  std::vector<unsigned char> buf;
  ~BgzfDeflater() { if (live) deflateEnd(&zs); }
  void prepare(int want_level) {
    if (live && level == want_level) { deflateReset(&zs); return; }
    if (live) deflateEnd(&zs);
    std::memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, want_level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) throw std::runtime_error("deflateInit2 failed");
    live = true;
    level = want_level;
  }
};
template <class A, class B> void bgzf_compress(const A &raw, B &out) {
  constexpr size_t kBlock = 0xff00;
  thread_local BgzfDeflater d;
  if (d.buf.empty()) d.buf.resize(compressBound(kBlock) + 64);
  thread_local std::vector<uint16_t> hash_table(size_t(1) << 13);
  for (size_t at = 0; at < raw.size(); at += kBlock) {
    const size_t len = std::min(kBlock, raw.size() - at);
    size_t clen = 0;
    if (g_bgzf_level == 1)  // the fast encoder (a block it cannot fit -- incompressible input -- goes through zlib, stored)
      clen = kFastDeflate(reinterpret_cast<const unsigned char *>(raw.data() + at), len, d.buf.data(), std::min<size_t>(d.buf.size(), 0xFFFF - 26), hash_table.data());
    if (clen == 0) {
      d.prepare(g_bgzf_level == 1 ? 0 : g_bgzf_level);
      z_stream &zs = d.zs;
      zs.next_in = reinterpret_cast<Bytef *>(const_cast<char *>(raw.data() + at));
      zs.avail_in = static_cast<uInt>(len);
      zs.next_out = d.buf.data();
      zs.avail_out = static_cast<uInt>(d.buf.size());
      if (deflate(&zs, Z_FINISH) != Z_STREAM_END) throw std::runtime_error("deflate failed");
      clen = zs.total_out;
    }
    const uint32_t crc = static_cast<uint32_t>(crc32(crc32(0L, Z_NULL, 0), reinterpret_cast<const Bytef *>(raw.data() + at), static_cast<uInt>(len)));
    static const unsigned char head[12] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0};
    out.append(reinterpret_cast<const char *>(head), 12);
    out.append("BC", 2); put_le16(out, 2); put_le16(out, static_cast<uint16_t>(clen + 25));
    out.append(reinterpret_cast<const char *>(d.buf.data()), clen);
    put_le32(out, crc); put_le32(out, static_cast<uint32_t>(len));
  }
}
std::string bam_header_bytes(const std::string &text, const Chroms &ch) {
  std::string o("BAM\1", 4);
  put_le32(o, static_cast<uint32_t>(text.size()));
  o += text;
  put_le32(o, static_cast<uint32_t>(ch.names.size() - 2));
  for (size_t i = 1; i + 1 < ch.names.size(); ++i) {
    put_le32(o, static_cast<uint32_t>(ch.names[i].size() + 1));
    o += ch.names[i]; o += '\0';
    put_le32(o, ch.starts[i + 1] - ch.starts[i]);
  }
  return o;
}
// (t_bam is defined above put_record's first use)

enum Outcome { UNMAPPED, UNIQUE, AMBIG };

template <class S> Outcome emit_se(S &o, bool allow_ambig, const abm_hit &h, const Chroms &ch, const NameRef &name,
                const char *seq, size_t n_seq, const uint32_t *cig, size_t n_cig) {
  const bool ambig = h.flags & 0x100;
  if (!allow_ambig && ambig) return AMBIG;
  uint32_t off = 0; int32_t chrom = 0;
  if (h.pos == 0 || !ch.locate(h.pos, ref_len(cig, n_cig), chrom, off)) return UNMAPPED;
  Record r{&name, 0, chrom - 1, -1, off, 0, 0, cig, n_cig, seq, n_seq, (h.flags & 0x10) != 0, h.diffs,
           (h.flags & 0x1000) ? 'A' : 'T'};
  if (h.flags & 0x10) r.flag |= 0x10;
  if (allow_ambig && ambig) r.flag |= 0x100;
  put_record(o, ch, r);
  return ambig ? AMBIG : UNIQUE;
}

template <class S> Outcome emit_pe(S &o, bool allow_ambig, const abm_pair &p, const Chroms &ch, const NameRef &n1,
                const NameRef &n2, const char *s1, size_t l1, const char *s2, size_t l2, const uint32_t *c1,
                size_t nc1, const uint32_t *c2, size_t nc2) {
  if (p.r1.pos == 0) return UNMAPPED;
  const bool ambig = p.r1.flags & 0x100;
  if (!allow_ambig && ambig) return AMBIG;
  int32_t ch1 = 0, ch2 = 0; uint32_t b1 = 0, b2 = 0;
  const uint32_t rl1 = ref_len(c1, nc1), rl2 = ref_len(c2, nc2);
  if (!ch.locate(p.r1.pos, rl1, ch1, b1) || !ch.locate(p.r2.pos, rl2, ch2, b2) || ch1 != ch2) return UNMAPPED;
  const uint32_t e2 = b2 + rl2;
  const bool rc1 = p.r1.flags & 0x10, rc2 = p.r2.flags & 0x10;
  const int isize = rc1 ? static_cast<int>(b1) - static_cast<int>(e2) : static_cast<int>(e2) - static_cast<int>(b1);
  uint16_t f1 = 0x1 | 0x2 | 0x40, f2 = 0x1 | 0x2 | 0x80;
  if (rc1) { f1 |= 0x10; f2 |= 0x20; }
  if (rc2) { f2 |= 0x10; f1 |= 0x20; }
  if (allow_ambig && ambig) { f1 |= 0x100; f2 |= 0x100; }
  put_record(o, ch, Record{&n1, f1, ch1 - 1, ch2 - 1, b1, b2, isize, c1, nc1, s1, l1, rc1, p.r1.diffs, (p.r1.flags & 0x1000) ? 'A' : 'T'});
  put_record(o, ch, Record{&n2, f2, ch2 - 1, ch1 - 1, b2, b1, -isize, c2, nc2, s2, l2, rc2, p.r2.diffs, (p.r2.flags & 0x1000) ? 'A' : 'T'});
  return ambig ? AMBIG : UNIQUE;
}

// ---- statistics (src/abismal.cpp:865-1071); 6 counters x {pairs|se, read1, read2} ----
void Stats::tally(bool empty_read, const abm_hit &h, bool count_ambig_error, uint32_t bases) {
  ++v[0];
  const bool valid = h.pos != 0, amb = h.flags & 0x100;
  v[1] += valid && !amb; v[2] += valid && amb; v[3] += empty_read;
  if (valid && (!amb || count_ambig_error)) { v[4] += static_cast<uint64_t>(static_cast<int64_t>(h.diffs)); v[5] += bases; }
}
std::string Stats::yaml(const std::string &label) const {
  // the reference keeps the first four in 32-bit counters (they wrap there)
  const uint32_t total = static_cast<uint32_t>(v[0]), unique = static_cast<uint32_t>(v[1]),
                 ambiguous = static_cast<uint32_t>(v[2]), skipped = static_cast<uint32_t>(v[3]);
  auto frac = [&](double x) { return total > 0 ? x / total : 0.0; };
  const uint32_t mapped = unique + ambiguous, unmapped = total - mapped;
  std::ostringstream s; const char *t = "    ";
  s << label << ":\n" << t << "total_reads: " << total << '\n' << t << "mapped:\n"
    << t << "    num_mapped: " << mapped << '\n' << t << "    num_unique: " << unique << '\n'
    << t << "    num_ambiguous: " << ambiguous << '\n' << t << "    percent_mapped: " << frac(mapped) * 100.0 << '\n'
    << t << "    percent_unique: " << frac(unique) * 100.0 << '\n' << t << "    percent_ambiguous: " << frac(ambiguous) * 100.0 << '\n'
    << t << "    unique_error:\n" << t << "        edits: " << v[4] << '\n' << t << "        total_bases: " << v[5] << '\n'
    << t << "        error_rate: " << (v[5] > 0 ? static_cast<double>(v[4]) / v[5] : 0.0) << '\n'
    << t << "num_unmapped: " << unmapped << '\n' << t << "num_skipped: " << skipped << '\n'
    << t << "percent_unmapped: " << frac(unmapped) * 100.0 << '\n' << t << "percent_skipped: " << frac(skipped) * 100.0 << '\n';
  return s.str();
}
std::string Stats::json() const {
  std::ostringstream s;
  s << "{\"edit_distance\":" << v[4] << ",\"reads_mapped_ambiguous\":" << static_cast<uint32_t>(v[2])
    << ",\"reads_mapped_unique\":" << static_cast<uint32_t>(v[1]) << ",\"reads_skipped\":" << static_cast<uint32_t>(v[3])
    << ",\"total_bases\":" << v[5] << ",\"total_reads\":" << static_cast<uint32_t>(v[0]) << "}";
  return s.str();
}

}  // namespace
