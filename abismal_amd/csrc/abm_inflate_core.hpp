// abismal_amd: RFC 1951 inflate of ONE BGZF block (SAM specification 4.1), shared by the device kernel (abm_inflate.hip)
// and by plain host C++ (tests/cpp/inflate_core_check.cpp runs it under sanitizers).  Header parsing, the bit reader,
// the code-length code, the decode tables, symbol decoding, CRC-32 and every bounds check live here and only here.
//
// The three bounds hold by construction:
//   reads   every byte of the block is read through Bits::win[pos - win_base] with win_base <= pos < win_end <= end
//           (refill, stored_header), or through parse_header / le32 with an index checked against the block's length;
//   writes  a token is emitted only after `len <= text_len - out` was checked, and whoever executes the tokens writes
//           [out, out + len) of the block's text and nothing else;
//   matches a match token is emitted only after `dist <= out` was checked.
// The decoder is a producer of TOKENS: round() decodes up to kMaxTok of them (a literal, or a length and a distance) and
// at most one stored run, and its caller executes them -- one after the other on the host (inflate_block below), as a
// wavefront on the device.  The bit stream is read through a WINDOW of the block: the whole block on the host, 2 KB of it
// staged in LDS on the device; round() returns early when what is left of the window might not hold its next step.
#pragma once
#include <stdint.h>

#include "../../include/abismal_amd.h"

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define ABM_HD __host__ __device__
#else
#define ABM_HD
#endif

namespace abm_inflate {

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 kMaxBlock = 65536;   // BSIZE + 1 and ISIZE are at most this
constexpr u32 kFastBitsL = 10;     // first-level table of the literal/length code
constexpr u32 kFastBitsD = 8;      // of the distance code (and of the code-length code, 7 bits at most)
constexpr u32 kMaxTok = 64;        // tokens per round: one per lane
constexpr u32 kWindow = 2048;      // bytes of the block staged at a time for the device's rounds to read their bits from
constexpr u32 kTokenRoom = 8;      // one token: 15 + 5 + 15 + 13 = 48 bits, from a buffer that a refill of 8 bytes fills
// the header of a dynamic block: 3 + 14 + 19 * 3 bits, then 316 code lengths of at most 7 + 7 bits each = 563 bytes.
// round() begins a block's header only in a window that holds this much (or the stream's end): a fresh one does.
constexpr u32 kHeaderBytes = 576;
static_assert(kWindow >= kHeaderBytes + 8, "a fresh window holds a whole dynamic header");

ABM_HD inline u32 le16(const u8 *p) { return static_cast<u32>(p[0]) | (static_cast<u32>(p[1]) << 8); }
ABM_HD inline u32 le32(const u8 *p) { return le16(p) | (le16(p + 2) << 16); }

// ---- gzip / BGZF header: 1f 8b 08 04 | mtime(4) xfl os | xlen(2) | subfields ... 'B' 'C' 02 00 BSIZE(2) ... ----------
// Reads at most `avail` bytes at p.  On ABM_INFLATE_OK: total = BSIZE + 1 (the block's whole length, NOT yet compared with
// anything) and data_off = where the deflate stream begins; total >= data_off + 8 holds.
ABM_HD inline u32 parse_header(const u8 *p, u64 avail, u32 &total, u32 &data_off) {
  if (avail < 20 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return ABM_INFLATE_HEADER;
  const u32 xlen = le16(p + 10);
  if (12ull + xlen + 8 > avail) return ABM_INFLATE_HEADER;
  bool found = false;
  u32 bsize = 0;
  u32 at = 0;
  while (at < xlen) {
    if (at + 4 > xlen) return ABM_INFLATE_HEADER;
    const u8 *sf = p + 12 + at;
    const u32 slen = le16(sf + 2);
    if (at + 4 + slen > xlen) return ABM_INFLATE_HEADER;
    if (!found && sf[0] == 'B' && sf[1] == 'C' && slen == 2) { found = true; bsize = le16(sf + 4); }
    at += 4 + slen;
  }
  if (!found) return ABM_INFLATE_HEADER;
  total = bsize + 1;
  data_off = 12 + xlen;
  return total >= data_off + 8 ? ABM_INFLATE_OK : ABM_INFLATE_HEADER;
}

// ---- CRC-32 (reflected, polynomial 0xEDB88320) in pieces ----------------------------------------------------------------
// The register's update is linear over GF(2), so the text may be cut into pieces: the first piece's register starts at
// 0xFFFFFFFF, every other at 0, each runs crc_byte over its bytes, is multiplied by x^(8 * bytes after the piece) and the
// products are XOR-ed; the complement of that is the CRC-32 (crc_shift is zlib's crc32_combine operator).
constexpr u32 kCrcPoly = 0xEDB88320u;
ABM_HD inline u32 crc_byte(u32 s, u32 byte) {
  s ^= byte;
  for (int k = 0; k < 8; ++k) s = (s >> 1) ^ (kCrcPoly & (0u - (s & 1u)));
  return s;
}
ABM_HD inline u32 crc_mul(u32 a, u32 b) {  // a * b mod P, bit 31 = x^0
  u32 p = 0;
  for (u32 m = 1u << 31; m != 0; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
ABM_HD inline u32 crc_shift(u32 s, u32 n_bytes) {  // s * x^(8 * n_bytes)
  u32 r = 1u << 31, base = 1u << 23;               // x^0, x^8
  for (; n_bytes; n_bytes >>= 1) {
    if (n_bytes & 1u) r = crc_mul(r, base);
    base = crc_mul(base, base);
  }
  return crc_mul(r, s);
}

// ---- the bit reader ---------------------------------------------------------------------------------------------------
// Positions count from the block's first byte; the deflate stream is [data_off, end) with end = len - 8.  win[k] is byte
// win_base + k of the block and win_end <= end: refill reads one byte at a time and only below win_end -- never a word
// that could reach past the block's last byte.
struct Bits {
  const u8 *win;
  u32 win_base, win_end, pos, end;
  u64 buf;
  u32 n;
};
ABM_HD inline void refill(Bits &b) {
  while (b.n <= 56 && b.pos < b.win_end) {
    b.buf |= static_cast<u64>(b.win[b.pos - b.win_base]) << b.n;
    ++b.pos;
    b.n += 8;
  }
}
ABM_HD inline u32 take(Bits &b, u32 k) {  // k <= b.n, k <= 16
  const u32 v = static_cast<u32>(b.buf) & ((1u << k) - 1u);
  b.buf >>= k;
  b.n -= k;
  return v;
}
ABM_HD inline u32 room(const Bits &b) { return b.pos < b.win_end ? b.win_end - b.pos : 0; }
// whole bytes in the buffer go back to the stream (before a new window is placed at pos, and before a stored block)
ABM_HD inline void unread_bytes(Bits &b) {
  b.pos -= b.n >> 3;
  b.n &= 7u;
  b.buf &= (1ull << b.n) - 1ull;
}

// ---- decode tables ------------------------------------------------------------------------------------------------------
// A code = its canonical description (count of codes per length, symbols in code order: what decoding bit by bit needs)
// plus a first-level table indexed by the next fast_bits bits of the stream: symbol | length << 9, 0 = a longer code (or
// none): decode bit by bit.
struct Tables {
  u16 count_l[16], count_d[16];
  u16 sym_l[288], sym_d[32];
  u16 fast_l[1u << kFastBitsL], fast_d[1u << kFastBitsD];
  u8 len[320];  // the code lengths of a block, literal/length first
  u8 cl[19];
};

// false: over-subscribed, or incomplete beyond what RFC 1951 allows (zlib's rule: only a code of one 1-bit symbol, and
// never the code-length code).  A code without any symbol is legal; using it is not (decode fails).
ABM_HD inline bool build_code(const u8 *len, u32 n, u16 *count, u16 *sym, u16 *fast, u32 fast_bits, bool is_cl) {
  for (u32 l = 0; l < 16; ++l) count[l] = 0;
  for (u32 i = 0; i < n; ++i) ++count[len[i] & 15u];
  count[0] = 0;
  int left = 1;
  u32 max_len = 0;
  for (u32 l = 1; l < 16; ++l) {
    left <<= 1;
    left -= count[l];
    if (left < 0) return false;
    if (count[l]) max_len = l;
  }
  if (left > 0 && max_len != 0 && (is_cl || max_len != 1)) return false;
  u16 offs[16], next[16];
  offs[1] = 0;
  next[1] = 0;
  for (u32 l = 1; l < 15; ++l) {
    offs[l + 1] = static_cast<u16>(offs[l] + count[l]);
    next[l + 1] = static_cast<u16>((next[l] + count[l]) << 1);
  }
  for (u32 k = 0; k < (1u << fast_bits); ++k) fast[k] = 0;
  for (u32 i = 0; i < n; ++i) {
    const u32 l = len[i] & 15u;
    if (!l) continue;
    sym[offs[l]++] = static_cast<u16>(i);
    const u32 code = next[l]++;
    if (l > fast_bits) continue;
    u32 rev = 0;
    for (u32 k = 0; k < l; ++k) rev |= ((code >> k) & 1u) << (l - 1 - k);
    for (u32 k = rev; k < (1u << fast_bits); k += 1u << l) fast[k] = static_cast<u16>(i | (l << 9));
  }
  return true;
}

// the next symbol, or -1: no code matches, or the stream ends inside it
ABM_HD inline int decode_sym(Bits &b, const u16 *count, const u16 *sym, const u16 *fast, u32 fast_bits) {
  const u32 e = fast[static_cast<u32>(b.buf) & ((1u << fast_bits) - 1u)];
  if (e) {
    const u32 l = e >> 9;
    if (l > b.n) return -1;
    b.buf >>= l;
    b.n -= l;
    return static_cast<int>(e & 511u);
  }
  u32 code = 0, first = 0, index = 0;
  for (u32 l = 1; l < 16; ++l) {
    if (l > b.n) return -1;
    code |= static_cast<u32>(b.buf >> (l - 1)) & 1u;
    const u32 c = count[l];
    if (code < first + c) {
      b.buf >>= l;
      b.n -= l;
      return sym[index + (code - first)];
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return -1;
}

// ---- the decoder ----------------------------------------------------------------------------------------------------------
enum { kPhaseHeader = 0, kPhaseCodes = 1, kPhaseDone = 2, kPhaseFailed = 3 };
struct State {
  Bits b;
  u32 out, text_len;  // text produced so far (tokens emitted count), and the text's length
  u32 phase, last;
  u32 status;         // ABM_INFLATE_* once phase == kPhaseFailed
};
ABM_HD inline void start(State &s, u32 data_off, u32 len, u32 text_len) {
  s.b.win = nullptr;
  s.b.win_base = s.b.win_end = 0;
  s.b.pos = data_off;
  s.b.end = len - 8;
  s.b.buf = 0;
  s.b.n = 0;
  s.out = 0;
  s.text_len = text_len;
  s.phase = kPhaseHeader;
  s.last = 0;
  s.status = ABM_INFLATE_OK;
}
// a new window: win[k] = byte base + k of the block, n bytes; base must be the reader's position after unread_bytes
ABM_HD inline void place_window(State &s, const u8 *win, u32 base, u32 n) {
  s.b.win = win;
  s.b.win_base = base;
  s.b.win_end = base + n;
}
// Does the reader need a new window before its next round?  Yes when it stands outside the one it has (at the start, and
// after a stored run), or when what is left of it might not hold round()'s next step -- a block's header is the longest.
ABM_HD inline bool window_spent(const Bits &b) {
  if (b.pos < b.win_base || b.pos > b.win_end) return true;
  return b.win_end != b.end && b.win_end - b.pos < kHeaderBytes;
}
ABM_HD inline void fail(State &s, u32 status) { s.phase = kPhaseFailed; s.status = status; }

ABM_HD inline bool fixed_codes(Tables &t) {
  for (u32 i = 0; i < 288; ++i) t.len[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
  for (u32 i = 0; i < 32; ++i) t.len[288 + i] = 5;  // (symbols 286, 287 and 30, 31 take part in the codes; using them is an error)
  return build_code(t.len, 288, t.count_l, t.sym_l, t.fast_l, kFastBitsL, false) &&
         build_code(t.len + 288, 32, t.count_d, t.sym_d, t.fast_d, kFastBitsD, false);
}
ABM_HD inline bool dynamic_codes(State &s, Tables &t) {
  Bits &b = s.b;
  refill(b);
  if (b.n < 14) return false;
  const u32 hlit = take(b, 5) + 257, hdist = take(b, 5) + 1, hclen = take(b, 4) + 4;
  if (hlit > 286 || hdist > 30) return false;
  constexpr u8 order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  for (u32 i = 0; i < 19; ++i) t.cl[i] = 0;
  for (u32 i = 0; i < hclen; ++i) {
    refill(b);
    if (b.n < 3) return false;
    t.cl[order[i]] = static_cast<u8>(take(b, 3));
  }
  if (!build_code(t.cl, 19, t.count_d, t.sym_d, t.fast_d, kFastBitsD, true)) return false;
  const u32 total = hlit + hdist;
  u32 i = 0;
  while (i < total) {
    refill(b);
    const int c = decode_sym(b, t.count_d, t.sym_d, t.fast_d, kFastBitsD);
    if (c < 0) return false;
    if (c < 16) { t.len[i++] = static_cast<u8>(c); continue; }
    u32 value = 0, rep;
    if (c == 16) {
      if (i == 0 || b.n < 2) return false;  // nothing to repeat
      value = t.len[i - 1];
      rep = 3 + take(b, 2);
    }
    else if (c == 17) { if (b.n < 3) return false; rep = 3 + take(b, 3); }
    else { if (b.n < 7) return false; rep = 11 + take(b, 7); }
    if (rep > total - i) return false;
    for (; rep; --rep) t.len[i++] = static_cast<u8>(value);
  }
  if (t.len[256] == 0) return false;  // no end-of-block code
  return build_code(t.len, hlit, t.count_l, t.sym_l, t.fast_l, kFastBitsL, false) &&
         build_code(t.len + hlit, hdist, t.count_d, t.sym_d, t.fast_d, kFastBitsD, false);
}

// Decodes until kMaxTok tokens are there, a stored run is pending, the window might be too short for the next step, or the
// stream is done or broken.  tok[k]: a literal = its byte; a match = length | distance << 9 (distance >= 1).  A stored
// run (copy_len bytes of the BLOCK from byte copy_src, possibly none) follows the tokens.  Afterwards the caller executes
// the tokens and the run in that order, and -- unless the window is the whole stream -- places a new window.
ABM_HD inline void round(State &s, Tables &t, u32 *tok, u32 &n_tok, u32 &copy_src, u32 &copy_len) {
  Bits &b = s.b;
  n_tok = 0;
  copy_src = copy_len = 0;
  const bool whole = b.win_end == b.end;
  while (s.phase == kPhaseHeader || s.phase == kPhaseCodes) {
    if (s.phase == kPhaseHeader) {
      if (!whole && room(b) < kHeaderBytes) return;
      refill(b);
      if (b.n < 3) return fail(s, ABM_INFLATE_DATA);
      s.last = take(b, 1);
      const u32 type = take(b, 2);
      if (type == 0) {
        take(b, b.n & 7u);
        unread_bytes(b);  // (n is 0 now)
        if (room(b) < 4) return fail(s, ABM_INFLATE_DATA);  // (the window holds them unless the stream ends here)
        const u8 *h = b.win + (b.pos - b.win_base);
        const u32 len = le16(h), nlen = le16(h + 2);
        if ((len ^ 0xFFFFu) != nlen) return fail(s, ABM_INFLATE_DATA);
        b.pos += 4;
        if (len > b.end - b.pos) return fail(s, ABM_INFLATE_DATA);
        if (len > s.text_len - s.out) return fail(s, ABM_INFLATE_SIZE);
        copy_src = b.pos;
        copy_len = len;
        b.pos += len;
        s.out += len;
        if (s.last) s.phase = kPhaseDone;
        return;  // (the reader now stands beyond its window)
      }
      if (type == 3) return fail(s, ABM_INFLATE_DATA);
      if (!(type == 1 ? fixed_codes(t) : dynamic_codes(s, t))) return fail(s, ABM_INFLATE_DATA);
      s.phase = kPhaseCodes;
    }
    for (;;) {
      if (n_tok == kMaxTok) return;
      if (!whole && room(b) < kTokenRoom) return;
      refill(b);
      int sym = decode_sym(b, t.count_l, t.sym_l, t.fast_l, kFastBitsL);
      if (sym < 0) return fail(s, ABM_INFLATE_DATA);
      if (sym < 256) {
        if (s.out >= s.text_len) return fail(s, ABM_INFLATE_SIZE);
        tok[n_tok++] = static_cast<u32>(sym);
        ++s.out;
        continue;
      }
      if (sym == 256) { s.phase = s.last ? kPhaseDone : kPhaseHeader; break; }
      sym -= 257;
      if (sym >= 29) return fail(s, ABM_INFLATE_DATA);  // literal/length symbols 286, 287
      u32 len, extra;
      if (sym < 8) { len = 3 + sym; extra = 0; }
      else if (sym == 28) { len = 258; extra = 0; }
      else { extra = (sym >> 2) - 1; len = 3 + ((4u + (sym & 3u)) << extra); }
      if (extra > b.n) return fail(s, ABM_INFLATE_DATA);
      len += take(b, extra);
      refill(b);
      const int ds = decode_sym(b, t.count_d, t.sym_d, t.fast_d, kFastBitsD);
      if (ds < 0 || ds >= 30) return fail(s, ABM_INFLATE_DATA);  // distance symbols 30, 31
      u32 dist;
      if (ds < 4) { dist = 1 + ds; extra = 0; }
      else { extra = (ds >> 1) - 1; dist = 1 + ((2u + (ds & 1u)) << extra); }
      if (extra > b.n) return fail(s, ABM_INFLATE_DATA);
      dist += take(b, extra);
      if (dist > s.out) return fail(s, ABM_INFLATE_DATA);  // before the text's first byte
      if (len > s.text_len - s.out) return fail(s, ABM_INFLATE_SIZE);
      tok[n_tok++] = len | (dist << 9);
      s.out += len;
    }
  }
}

// after the stream: what the member's trailer says, against the text's length and the text's CRC-32
ABM_HD inline u32 check_trailer(const u8 *block, u32 len, u32 produced, u32 text_len, u32 crc) {
  if (produced != text_len || le32(block + len - 4) != text_len) return ABM_INFLATE_SIZE;
  return le32(block + len - 8) == crc ? ABM_INFLATE_OK : ABM_INFLATE_CRC;
}

// ---- one block, serially (the host form; the kernel runs the same round() and executes its tokens as a wave) ---------------
// Reads [block, block + len), writes [text, text + text_len).  `t` is scratch.
inline u32 inflate_block(const u8 *block, u32 len, u8 *text, u32 text_len, Tables &t) {
  if (len > kMaxBlock || text_len > kMaxBlock) return len > kMaxBlock ? ABM_INFLATE_HEADER : ABM_INFLATE_SIZE;
  u32 total = 0, data_off = 0;
  const u32 hs = parse_header(block, len, total, data_off);
  if (hs != ABM_INFLATE_OK) return hs;
  if (total != len) return ABM_INFLATE_HEADER;
  State s;
  start(s, data_off, len, text_len);
  place_window(s, block + data_off, data_off, s.b.end - data_off);
  u32 tok[kMaxTok];
  u32 at = 0;
  while (s.phase == kPhaseHeader || s.phase == kPhaseCodes) {
    u32 n_tok, copy_src, copy_len;
    round(s, t, tok, n_tok, copy_src, copy_len);
    for (u32 k = 0; k < n_tok; ++k) {
      const u32 dist = tok[k] >> 9;
      if (!dist) { text[at++] = static_cast<u8>(tok[k]); continue; }
      for (u32 l = tok[k] & 511u; l; --l, ++at) text[at] = text[at - dist];
    }
    for (u32 k = 0; k < copy_len; ++k) text[at++] = block[copy_src + k];
  }
  if (s.phase == kPhaseFailed) return s.status;
  // (in 64 pieces, as the wave computes it)
  const u32 piece = (text_len + 63) / 64;
  u32 crc = 0;
  for (u32 lane = 0; lane < 64; ++lane) {
    const u32 lo = lane * piece < text_len ? lane * piece : text_len, hi = lo + piece < text_len ? lo + piece : text_len;
    u32 r = lane == 0 ? 0xFFFFFFFFu : 0u;
    for (u32 k = lo; k < hi; ++k) r = crc_byte(r, text[k]);
    crc ^= crc_shift(r, text_len - hi);
  }
  return check_trailer(block, len, s.out, text_len, ~crc);
}

}  // namespace abm_inflate
