// abismal_amd: RFC 1951 deflate of ONE block of text into ONE BGZF member (SAM specification 4.1), shared by the device
// kernel (abm_deflate.hip) and by plain host C++ (abm_deflate_bgzf_host; tests/cpp/deflate_core_check.cpp runs it under
// sanitizers).  The member: the 18-byte header with the BC subfield, one deflate stream, CRC-32 and ISIZE.  The stream is
// ONE fixed-Huffman block (3.2.6: no trees to build or ship), or -- if that would be longer than text_len + 5 bytes, as
// for 4-bit sequence and anything else without repeats (bytes >= 144 cost 9 bits) -- one STORED block; an empty text is a
// stored block of length 0.  A member is therefore at most text_len + 31 bytes.
//
// The encoder is written for a wavefront.  The text is taken in ROUNDS of 64 consecutive positions, one per lane, and a
// round is a sequence of PHASES, each a function of (lane, that lane's registers, the wave's shared state):
//   probe    hash the 4 bytes at the position, read the table's entry from before the round
//   enter    table[hash] = max(table[hash], position + 1): the round's highest position wins
//   measure  the longer of two candidate matches: the table's, and position - 1 (runs, which a round cannot see in its
//            own table: the 0xFF of absent qualities, poly-N), by 8-byte compares, <= 258 bytes, <= 32768 back
//   walk     the greedy parse, left to right from where the previous round's last token ended: a position covered by an
//            earlier match emits nothing, a match may run past the round's end.  Literals need no step: the walk jumps
//            from match to match over the ballot of "this lane has a match".
//   token    a surviving position's bits: a literal, or length symbol + extra + distance symbol + extra (<= 31 bits)
//   place    OR the bits into the staging words at the offset a prefix sum of the bit counts gives
//   flush    whole staging words go out to the stream; the last, partial one is carried into the next round
// The device runs a phase on all lanes at once with wave_sync() between phases; the host runs it in a loop over lanes
// 0..63 (deflate_member below), with a loop for the ballot and a running sum for the prefix sum.  No phase depends on
// the order of the lanes within it, so both give the same bytes.
//
// Bounds: the text is read only at [0, n) (probe: i + 4 <= n; measure: every compare below lim = min(258, n - i));
// the stream is written only below text_len + 5 bytes (would_overflow is asked before every flush), so the member fits
// text_len + 31 bytes whatever the text.
#pragma once
#include <stdint.h>

#include "abm_inflate_core.hpp"  // ABM_HD, crc_byte / crc_shift, kCrcPoly: one CRC-32 for both directions

namespace abm_deflate {

using abm_inflate::u8;
using abm_inflate::u16;
using abm_inflate::u32;
using abm_inflate::u64;

constexpr u32 kMaxText = 0xff00;      // the text of one member, as the host's bgzf_compress cuts it
constexpr u32 kHeader = 18, kTrailer = 8;
constexpr u32 kStoredExtra = 5;       // 1 byte of block header, LEN, NLEN
constexpr u32 kMaxMember = kMaxText + kHeader + kStoredExtra + kTrailer;  // 65311: BSIZE fits
constexpr u32 kHashBits = 13;
constexpr u32 kMinMatch = 4, kMaxMatch = 258, kMaxDist = 32768;
constexpr u32 kLanes = 64;
constexpr u32 kStageWords = 66;       // 31 carried bits + 64 tokens of <= 31 bits = 2015 bits, and a spare word
static_assert(kMaxMember <= 65536, "BSIZE holds a member's length");

// the wave's shared state: LDS on the device (16.6 KB: nine waves to a CU's 160 KB)
struct Shared {
  u16 table[1u << kHashBits];  // position + 1 of the last string with this hash; 0 = none
  u32 stage[kStageWords];      // the stream's bits from word `words` on
  u16 mlen[kLanes];            // the round's match lengths (0 = none), for the walk
};
// one lane's values between the phases of a round (registers on the device)
struct Lane {
  u32 hash;  // kNoHash: fewer than 4 bytes left at this position
  u32 cand;  // table entry before the round
  u32 len, dist;
};
constexpr u32 kNoHash = 0xFFFFFFFFu;

ABM_HD inline u32 load32(const u8 *p) { u32 v; __builtin_memcpy(&v, p, 4); return v; }
ABM_HD inline u64 load64(const u8 *p) { u64 v; __builtin_memcpy(&v, p, 8); return v; }
ABM_HD inline u32 min_u32(u32 a, u32 b) { return a < b ? a : b; }
ABM_HD inline u32 log2_u32(u32 v) { return 31u - static_cast<u32>(__builtin_clz(v)); }  // v != 0
ABM_HD inline u32 rev_bits(u32 v, u32 n) {  // the low n <= 16 bits, reversed (Huffman codes go most significant bit first)
  v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
  v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
  v = ((v & 0x0F0Fu) << 4) | ((v >> 4) & 0x0F0Fu);
  v = ((v & 0x00FFu) << 8) | ((v >> 8) & 0x00FFu);
  return v >> (16u - n);
}
// OR into a staging word: lanes of one phase share words
ABM_HD inline void or_word(u32 *p, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(p, v);
#else
  *p |= v;
#endif
}

// ---- the phases of a round; i = the lane's position, n = the text's length ------------------------------------------------
ABM_HD inline void probe(Lane &l, const Shared &sh, const u8 *text, u32 n, u32 i) {
  l.len = l.dist = l.cand = 0;
  l.hash = kNoHash;
  if (i + 4 > n) return;
  l.hash = (load32(text + i) * 2654435761u) >> (32u - kHashBits);
  l.cand = sh.table[l.hash];
}
// One attempt at table[hash] = max(table[hash], i + 1); true: it wrote.  The host calls it once per lane, in any order.
// The device repeats it, a wave_sync() after each, until no lane wrote: of the lanes that store to one entry in the same
// instruction one wins, a lane with a higher position then finds less than its own and stores again, and the entry only
// ever grows -- it ends at the maximum.
ABM_HD inline bool enter_once(const Lane &l, Shared &sh, u32 i) {
  if (l.hash == kNoHash || sh.table[l.hash] >= i + 1) return false;
  sh.table[l.hash] = static_cast<u16>(i + 1);
  return true;
}
// bytes that text[p ...] and text[i ...] share, p < i, at most lim <= n - i
ABM_HD inline u32 match_length(const u8 *text, u32 p, u32 i, u32 lim) {
  u32 k = 0;
  while (k + 8 <= lim) {
    const u64 x = load64(text + p + k) ^ load64(text + i + k);
    if (x) return k + (static_cast<u32>(__builtin_ctzll(x)) >> 3);
    k += 8;
  }
  while (k < lim && text[p + k] == text[i + k]) ++k;
  return k;
}
ABM_HD inline void measure(Lane &l, Shared &sh, u32 lane, const u8 *text, u32 n, u32 i) {
  if (l.hash != kNoHash) {
    const u32 lim = min_u32(kMaxMatch, n - i);
    if (i >= 1) {  // the run candidate first: of two matches of one length the nearer costs fewer bits
      const u32 k = match_length(text, i - 1, i, lim);
      if (k >= kMinMatch) { l.len = k; l.dist = 1; }
    }
    if (l.cand != 0 && i - (l.cand - 1) <= kMaxDist && i - (l.cand - 1) > 1) {  // (a block is longer than the window)
      const u32 k = match_length(text, l.cand - 1, i, lim);
      if (k >= kMinMatch && k > l.len) { l.len = k; l.dist = i - (l.cand - 1); }
    }
  }
  sh.mlen[lane] = static_cast<u16>(l.len);
}
// The greedy parse of a round.  matches: bit k = lane k has a match; from: where the next token starts, relative to the
// round's first position, < 64.  Returns the lanes that emit a token, and in `next` where the token after the round's
// last one starts (>= 64, relative again).
ABM_HD inline u64 walk(const Shared &sh, u64 matches, u32 from, u32 &next) {
  u64 on = 0;
  u32 at = from;
  while (at < kLanes) {
    const u64 ahead = matches >> at;
    if (!ahead) { on |= ~0ull << at; at = kLanes; break; }  // literals to the round's end
    const u32 m = at + static_cast<u32>(__builtin_ctzll(ahead));
    on |= (~0ull << at) & ~(~0ull << m);  // literals [at, m)
    on |= 1ull << m;
    at = m + sh.mlen[m];
  }
  next = at;
  return on;
}
// the fixed code of a literal/length symbol, as it goes into the stream (least significant bit first)
ABM_HD inline u32 fixed_code(u32 s, u32 &bits) {
  if (s < 144) { bits = 8; return rev_bits(0x30 + s, 8); }
  if (s < 256) { bits = 9; return rev_bits(0x190 + (s - 144), 9); }
  if (s < 280) { bits = 7; return rev_bits(s - 256, 7); }
  bits = 8;
  return rev_bits(0xC0 + (s - 280), 8);
}
// a token's bits and their number (<= 8 + 5 + 5 + 13 = 31)
ABM_HD inline u32 token(const Lane &l, u32 byte, u32 &bits) {
  if (!l.len) return fixed_code(byte, bits);
  u32 sym, extra = 0, extra_bits = 0;
  const u32 k = l.len - 3;
  if (l.len == kMaxMatch) sym = 285;
  else if (k < 8) sym = 257 + k;
  else {
    extra_bits = log2_u32(k) - 2;
    sym = 257 + 4 * extra_bits + 4 + ((k >> extra_bits) & 3u);
    extra = k & ((1u << extra_bits) - 1u);
  }
  u32 v = fixed_code(sym, bits);
  v |= extra << bits;
  bits += extra_bits;
  const u32 d = l.dist - 1;
  u32 dsym, dextra = 0, dextra_bits = 0;
  if (d < 4) dsym = d;
  else {
    dextra_bits = log2_u32(d) - 1;
    dsym = 2 * dextra_bits + 2 + ((d >> dextra_bits) & 1u);
    dextra = d & ((1u << dextra_bits) - 1u);
  }
  v |= rev_bits(dsym, 5) << bits;
  bits += 5;
  v |= dextra << bits;
  bits += dextra_bits;
  return v;
}
// `bits` bits of v at bit `at` of the staging area
ABM_HD inline void place(Shared &sh, u32 at, u32 v, u32 bits) {
  if (!bits) return;
  const u64 w = static_cast<u64>(v) << (at & 31u);
  or_word(&sh.stage[at >> 5], static_cast<u32>(w));
  if (w >> 32) or_word(&sh.stage[(at >> 5) + 1], static_cast<u32>(w >> 32));
}
// Would a fixed-Huffman stream of `bits` bits so far (the 3 of the block header included, the end-of-block code not) be
// longer than the stored form?  Bits only grow, so a yes is final.
ABM_HD inline bool would_overflow(u32 bits, u32 n) { return (bits + 7u + 7u) / 8u > n + kStoredExtra; }

// ---- the member around the stream ------------------------------------------------------------------------------------------
ABM_HD inline void put16(u8 *p, u32 v) { p[0] = static_cast<u8>(v); p[1] = static_cast<u8>(v >> 8); }
ABM_HD inline void put32(u8 *p, u32 v) { put16(p, v); put16(p + 2, v >> 16); }
// header and trailer of a member whose stream is stream_bytes long (one lane); returns the member's length
ABM_HD inline u32 frame(u8 *member, u32 stream_bytes, u32 crc, u32 n) {
  const u32 total = kHeader + stream_bytes + kTrailer;
  const u8 head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
  for (u32 k = 0; k < 16; ++k) member[k] = head[k];
  put16(member + 16, total - 1);
  put32(member + kHeader + stream_bytes, crc);
  put32(member + kHeader + stream_bytes + 4, n);
  return total;
}
// the stored form's five bytes (one lane); the text follows them
ABM_HD inline void stored_header(u8 *stream, u32 n) {
  stream[0] = 1;  // BFINAL, BTYPE 00, padding
  put16(stream + 1, n);
  put16(stream + 3, n ^ 0xFFFFu);
}
// one lane's piece of the text's CRC-32, shifted to the text's end: the XOR of the 64, complemented, is the CRC-32
ABM_HD inline u32 crc_piece(u32 lane, const u8 *text, u32 n) {
  const u32 piece = (n + 63) / 64;
  const u32 lo = min_u32(lane * piece, n), hi = min_u32(lo + piece, n);
  u32 r = lane == 0 ? 0xFFFFFFFFu : 0u;
  for (u32 k = lo; k < hi; ++k) r = abm_inflate::crc_byte(r, text[k]);
  return abm_inflate::crc_shift(r, n - hi);
}

// blocks of a text cut every block_bytes, and the bytes that surely hold their members
ABM_HD inline u64 n_blocks_of(u64 text_bytes, u32 block_bytes) { return (text_bytes + block_bytes - 1) / block_bytes; }
ABM_HD inline u64 bound_of(u64 text_bytes, u32 block_bytes) {
  return text_bytes + n_blocks_of(text_bytes, block_bytes) * (kHeader + kStoredExtra + kTrailer);
}

// ---- one member, serially (the host form: every phase in a loop over the lanes) --------------------------------------------
// Reads text[0, n), n <= kMaxText; writes the member at `member` (room for n + 31 bytes) and returns its length.
inline u32 deflate_member(const u8 *text, u32 n, u8 *member, Shared &sh) {
  u8 *stream = member + kHeader;
  u32 crc = 0;
  for (u32 lane = 0; lane < kLanes; ++lane) crc ^= crc_piece(lane, text, n);
  crc = ~crc;
  bool stored = n == 0;
  u32 bits = 3, words = 0;  // bits of the stream so far; whole words of it that have left the staging area
  if (!stored) {
    for (u32 k = 0; k < (1u << kHashBits); ++k) sh.table[k] = 0;
    for (u32 k = 0; k < kStageWords; ++k) sh.stage[k] = 0;
    sh.stage[0] = 3;  // BFINAL = 1, BTYPE = 01
    Lane l[kLanes];
    u32 next = 0;  // where the next token starts
    for (u32 r0 = 0; r0 < n && !stored; r0 += kLanes) {
      if (next >= r0 + kLanes) continue;  // a match covers the whole round
      for (u32 lane = 0; lane < kLanes; ++lane) probe(l[lane], sh, text, n, r0 + lane);
      for (u32 lane = 0; lane < kLanes; ++lane) enter_once(l[lane], sh, r0 + lane);
      u64 matches = 0;
      for (u32 lane = 0; lane < kLanes; ++lane) {
        measure(l[lane], sh, lane, text, n, r0 + lane);
        matches |= static_cast<u64>(l[lane].len != 0) << lane;
      }
      u32 rel = 0;
      u64 on = walk(sh, matches, next - r0, rel);
      if (n - r0 < kLanes) on &= ~(~0ull << (n - r0));  // (positions past the text)
      next = r0 + rel;
      u32 tok[kLanes], tok_bits[kLanes], sum = 0;
      for (u32 lane = 0; lane < kLanes; ++lane) {
        tok[lane] = tok_bits[lane] = 0;
        if (on >> lane & 1u) tok[lane] = token(l[lane], text[r0 + lane], tok_bits[lane]);
        sum += tok_bits[lane];
      }
      if (would_overflow(bits + sum, n)) { stored = true; break; }
      u32 at = bits - 32 * words;
      for (u32 lane = 0; lane < kLanes; ++lane) { place(sh, at, tok[lane], tok_bits[lane]); at += tok_bits[lane]; }
      bits += sum;
      const u32 whole = bits / 32 - words;
      for (u32 k = 0; k < whole; ++k) __builtin_memcpy(stream + 4 * (words + k), &sh.stage[k], 4);
      const u32 carry = sh.stage[whole];
      for (u32 k = 0; k < kStageWords; ++k) sh.stage[k] = 0;
      sh.stage[0] = carry;
      words += whole;
    }
  }
  if (stored) {
    stored_header(stream, n);
    for (u32 k = 0; k < n; ++k) stream[kStoredExtra + k] = text[k];
    return frame(member, kStoredExtra + n, crc, n);
  }
  bits += 7;  // the end-of-block code: seven zero bits
  const u32 stream_bytes = (bits + 7) / 8;
  for (u32 k = 4 * words; k < stream_bytes; ++k) stream[k] = static_cast<u8>(sh.stage[(k - 4 * words) >> 2] >> (8 * (k & 3u)));
  return frame(member, stream_bytes, crc, n);
}

}  // namespace abm_deflate
