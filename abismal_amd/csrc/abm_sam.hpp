// abismal_amd: SAM text written by the mapping kernels themselves (device side, shared by the single-end kernel's
// format_sam_tail and the pair kernels' format_pe_tails).  A record's line after QNAME -- put_record of the CLI, byte
// for byte -- is written by lane 0 into an LDS line buffer, SEQ by all lanes, and leaves as 4-byte words.
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

}  // namespace abm
