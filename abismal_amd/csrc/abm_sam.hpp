// abismal_amd: SAM text written by the mapping kernels themselves (device side, shared by the single-end kernel's
// format_sam_tail and the pair kernels' format_pe_tails).  A record's line after QNAME -- put_record of the CLI, byte
// for byte -- is written by lane 0 into an LDS line buffer, SEQ by all lanes, and leaves as 4-byte words.  BamWriter
// writes the same record as a BAM piece (put_bam_record of the CLI minus the name) through the same buffer and stores.
#pragma once
#include "abm_device.hpp"

namespace abm {

// Scalar fields are written byte by byte by lane 0 into an LDS line buffer (a few hundred scalar instructions: 1 % of a
// read's work); past `cap` only the length is counted (the caller then leaves the record to the host)
struct SamWriter {
  u8 *buf;
  u32 w, cap;
  __device__ __forceinline__ void put(u32 c) { if (w < cap && lane_id() == 0) buf[w] = static_cast<u8>(c); ++w; }
  __device__ __forceinline__ void put_uint(u32 v) {
    u32 digits = 1;
    for (u32 t = v; t >= 10u; t /= 10u) ++digits;
    u32 at = w + digits;
    w = at;
    do { --at; if (at < cap && lane_id() == 0) buf[at] = static_cast<u8>('0' + v % 10u); v /= 10u; } while (v);
  }
  __device__ __forceinline__ void put_int(int v) { if (v < 0) { put('-'); put_uint(static_cast<u32>(-v)); } else put_uint(static_cast<u32>(v)); }
  __device__ __forceinline__ void put_str(const char *s, u32 n) { for (u32 i = 0; i < n; ++i) put(static_cast<u8>(s[i])); }
  // CIGAR ops as the kernels store them (length << 4 | op), from LDS (CigarSink::fin)
  __device__ __forceinline__ void put_cigar(const u32 *fin, u32 n_ops) {
    for (u32 k = 0; k < n_ops; ++k) {
      const u32 v = static_cast<u32>(uni(static_cast<int>(fin[k])));
      put_uint(v >> 4);
      put(static_cast<u8>("MIDNSHP=XB"[min(v & 15u, 9u)]));
    }
  }
  // RNAME of chromosome `chrom` (DevIndex::chrom_names)
  __device__ __forceinline__ void put_chrom(const DevIndex &ix, u32 chrom) {
    const u32 n0 = static_cast<u32>(uni(static_cast<int>(ix.chrom_name_off[chrom]))), n1 = static_cast<u32>(uni(static_cast<int>(ix.chrom_name_off[chrom + 1])));
    for (u32 i = n0; i < n1; ++i) put(static_cast<u8>(uni(static_cast<int>(ix.chrom_names[i]))));
  }
  // SEQ as htslib prints it after its 4-bit round trip: IUPAC letters upper-cased, everything else N; a reverse-strand
  // hit shows the reverse complement as the mapper makes it (src/common.hpp:28-44: A<->T, C<->G, everything else N).
  // All lanes.
  __device__ __forceinline__ void put_seq(const char *seq, u32 L, bool rc) {
    for (u32 i = lane_id(); i < L; i += 64) {
      u32 c = static_cast<u8>(seq[rc ? L - 1 - i : i]);
      if (rc) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
      else {
        const u32 u = (c >= 'a' && c <= 'z') ? c - 32u : c;
        // "=ACMGRSVTWYHKDBN": the letters A B C D G H K M N R S T V W Y
        const bool ok = u == '=' || (u >= 'A' && u <= 'Z' && ((0x016E34CFu >> (u - 'A')) & 1u));
        c = ok ? u : 'N';
      }
      if (w + i < cap) buf[w + i] = static_cast<u8>(c);
    }
    w += L;
  }
  // "\t*\tNM:i:<nm>\tCV:A:<cv>\n"
  __device__ __forceinline__ void put_tags(int nm, bool a_rich) {
    put_str("\t*\tNM:i:", 8);
    put_int(nm);
    put_str("\tCV:A:", 6);
    put(a_rich ? 'A' : 'T');
    put('\n');
  }
  // the line to dst (4-byte aligned) as 4-byte words, written through; all lanes, after the line is complete
  __device__ __forceinline__ void flush(u32 *dst) const {
    wave_sync();
    const u32 *src = reinterpret_cast<const u32 *>(buf);
    for (u32 k = lane_id(); k < (w + 3) / 4; k += 64) store_out(dst + k, src[k]);
  }
};

// reference length of a CIGAR held in LDS (ops M, D, N, =, X)
__device__ __forceinline__ u32 sam_ref_len(const u32 *fin, u32 n_ops) {
  u32 reflen = 0;
  for (u32 k = 0; k < n_ops; ++k) {
    const u32 v = static_cast<u32>(uni(static_cast<int>(fin[k]))), op = v & 15u;
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) reflen += v >> 4;
  }
  return reflen;
}

// Chroms::locate: the last start <= pos; true if the alignment ends inside that chromosome (chrom: its index into the
// table, c0: its start)
__device__ __forceinline__ bool sam_locate(const DevIndex &ix, u32 pos, u32 reflen, u32 &chrom, u32 &c0) {
  u32 lo = 0, n = ix.n_chroms + 1;  // upper_bound over starts[0 .. n_chroms]
  while (n > 0) {
    const u32 half = n >> 1;
    const u32 sv = static_cast<u32>(uni(static_cast<int>(ix.chrom_starts[lo + half])));
    if (!(pos < sv)) { lo += half + 1; n -= half + 1; } else n = half;
  }
  if (lo == 0 || lo > ix.n_chroms) return false;
  chrom = lo - 1;
  c0 = static_cast<u32>(uni(static_cast<int>(ix.chrom_starts[chrom])));
  const u32 c1 = static_cast<u32>(uni(static_cast<int>(ix.chrom_starts[chrom + 1])));
  return static_cast<u64>(pos) + reflen <= c1;
}

// ---- the same record as a BAM piece (SeArgs / PeArgs::sam_format == kRecordsBam) ---------------------------------------
// put_bam_record of the CLI without the read's name, which only the host has.  Bytes [0, 36): block_size (of the record
// WITHOUT its name) and the 32 fixed bytes, l_read_name 0; bytes [36, len): the CIGAR ops as stored, SEQ two bases a
// byte (high nibble first), l_seq bytes 0xFF (no qualities), NM with the smallest type that holds it, CV:A.  The host
// copies the 36 bytes, adds strlen(name) + 1 to block_size and stores it as l_read_name, appends the name and a NUL, then
// bytes [36, len).
constexpr int kRecordsSam = 0, kRecordsBam = 1;  // == ABM_RECORDS_*

// reg2bin of the SAM specification (5.3) over [beg, end)
__device__ __forceinline__ u32 bam_reg2bin(u64 beg, u64 end) {
  --end;
  if (beg >> 14 == end >> 14) return static_cast<u32>(((1u << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return static_cast<u32>(((1u << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return static_cast<u32>(((1u << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return static_cast<u32>(((1u << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return static_cast<u32>(((1u << 3) - 1) / 7 + (beg >> 26));
  return 0;
}
// 4-bit code of what SEQ shows for read byte c (put_seq's letter, then its index in "=ACMGRSVTWYHKDBN")
__device__ __forceinline__ u32 bam_seq4(u32 c, bool rc) {
  if (rc) return c == 'A' ? 8u : c == 'C' ? 4u : c == 'G' ? 2u : c == 'T' ? 1u : 15u;
  if (c == '=') return 0u;
  const u32 k = ((c >= 'a' && c <= 'z') ? c - 32u : c) - 'A';
  // one nibble per letter A .. P and Q .. Z: A 1, B 14, C 2, D 13, G 4, H 11, K 12, M 3, N 15, R 5, S 6, T 8, V 7, W 9, Y 10
  const u64 tab = k < 16u ? 0xFFF3FCFFB4FFD2E1ull : 0xFFFFFFFAF97F865Full;
  return k < 26u ? static_cast<u32>(tab >> ((k & 15u) * 4u)) & 15u : 15u;
}
struct BamFields {  // what put_bam_record takes from its Record, the name aside
  int refid;        // the chromosome's number in the BAM header (its place in the index's table less the padding entry)
  u32 pos, reflen, flag;
  int next_refid;   // < 0: no mate (next pos is then written as -1 whatever next_pos says)
  u32 next_pos;
  int tlen, nm;
  bool a_rich;
};
struct BamWriter {
  u8 *buf;   // LDS, 4-byte aligned, cap bytes
  u32 cap;
  __device__ __forceinline__ static u32 nm_bytes(int nm) { return (nm >= -128 && nm <= 255) ? 4u : 5u; }
  __device__ __forceinline__ static u32 piece_len(u32 n_ops, u32 L, int nm) { return 36u + 4u * n_ops + (L + 1u) / 2u + L + nm_bytes(nm) + 4u; }
  // the piece into buf: lane 0 the scalar fields, all lanes the CIGAR, SEQ and the absent qualities (one packed byte
  // per lane per round).  Returns its length, or 0xFFFFFFFF -- nothing written -- if it is longer than cap.
  __device__ __forceinline__ u32 put(const BamFields &f, const u32 *fin, u32 n_ops, const char *seq, u32 L, bool rc) const {
    const u32 len = piece_len(n_ops, L, f.nm);
    if (len > cap) return 0xFFFFFFFFu;
    const u32 lane = static_cast<u32>(lane_id());
    u32 *wd = reinterpret_cast<u32 *>(buf);
    const u32 packed = (L + 1u) / 2u;
    u8 *s = buf + 36u + 4u * n_ops;
    if (lane == 0) {
      wd[0] = len - 4u;
      wd[1] = static_cast<u32>(f.refid);
      wd[2] = f.pos;
      wd[3] = (255u << 8) | ((bam_reg2bin(f.pos, static_cast<u64>(f.pos) + (f.reflen ? f.reflen : 1u)) & 0xFFFFu) << 16);
      wd[4] = (n_ops & 0xFFFFu) | ((f.flag & 0xFFFFu) << 16);
      wd[5] = L;
      wd[6] = static_cast<u32>(f.next_refid);
      wd[7] = f.next_refid < 0 ? 0xFFFFFFFFu : f.next_pos;
      wd[8] = static_cast<u32>(f.tlen);
      u8 *t = s + packed + L;
      *t++ = 'N'; *t++ = 'M';
      if (f.nm >= 0 && f.nm <= 255) { *t++ = 'C'; *t++ = static_cast<u8>(f.nm); }
      else if (f.nm >= 0) { *t++ = 'S'; *t++ = static_cast<u8>(f.nm); *t++ = static_cast<u8>(f.nm >> 8); }
      else if (f.nm >= -128) { *t++ = 'c'; *t++ = static_cast<u8>(f.nm); }
      else { *t++ = 's'; *t++ = static_cast<u8>(f.nm); *t++ = static_cast<u8>(static_cast<u32>(f.nm) >> 8); }
      *t++ = 'C'; *t++ = 'V'; *t++ = 'A'; *t++ = f.a_rich ? 'A' : 'T';
    }
    for (u32 k = lane; k < n_ops; k += 64) wd[9 + k] = fin[k];
    for (u32 i = lane; i < packed; i += 64) {
      const u32 j = 2u * i;
      const u32 hi = bam_seq4(static_cast<u8>(seq[rc ? L - 1u - j : j]), rc);
      const u32 lo = j + 1u < L ? bam_seq4(static_cast<u8>(seq[rc ? L - 2u - j : j + 1u]), rc) : 0u;
      s[i] = static_cast<u8>((hi << 4) | lo);
    }
    for (u32 i = lane; i < L; i += 64) s[packed + i] = 0xFFu;
    return len;
  }
  // the piece to dst (4-byte aligned) as 4-byte words, written through; all lanes (as SamWriter::flush)
  __device__ __forceinline__ void flush(u32 *dst, u32 len) const {
    wave_sync();
    const u32 *src = reinterpret_cast<const u32 *>(buf);
    for (u32 k = lane_id(); k < (len + 3) / 4; k += 64) store_out(dst + k, src[k]);
  }
  // put, then flush to the record's slot: the piece's length, or 0xFFFFFFFF (the host formats this one)
  __device__ __forceinline__ u32 write(const BamFields &f, const u32 *fin, u32 n_ops, const char *seq, u32 L, bool rc, char *slot) const {
    const u32 len = put(f, fin, n_ops, seq, L, rc);
    if (len != 0xFFFFFFFFu) flush(reinterpret_cast<u32 *>(slot), len);
    return len;
  }
};

}  // namespace abm
