// Stand-alone check of abismal_amd/csrc/abm_inflate_core.hpp on the CPU, meant to be built with
//   g++ -O1 -g -fsanitize=address,undefined
// Reads a fixture file: u32 n, then per member  u32 len, u32 text_len, u8 expect, block[len], text[text_len]
// (expect: an ABM_INFLATE_* status, or 255 = "any non-zero status, or OK with this text").  Every block is copied into a
// heap buffer of exactly its length and inflated into a buffer of exactly text_len bytes, twice: through the core's
// serial inflate_block, and through rounds fed from 2 KB windows held in heap buffers of exactly their size and renewed
// when the core says so -- the way the kernel stages the stream in LDS.  Exit status 0 = every member gave what the file
// expects.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../abismal_amd/csrc/abm_inflate_core.hpp"

using namespace abm_inflate;

static u32 inflate_windowed(const u8 *block, u32 len, u8 *text, u32 text_len, Tables &t) {
  if (len > kMaxBlock) return ABM_INFLATE_HEADER;
  if (text_len > kMaxBlock) return ABM_INFLATE_SIZE;
  u32 total = 0, data_off = 0;
  const u32 hs = parse_header(block, len, total, data_off);
  if (hs != ABM_INFLATE_OK) return hs;
  if (total != len) return ABM_INFLATE_HEADER;
  State s;
  start(s, data_off, len, text_len);
  u32 tok[kMaxTok], at = 0;
  std::unique_ptr<u8[]> win;
  while (s.phase == kPhaseHeader || s.phase == kPhaseCodes) {
    if (window_spent(s.b)) {
      unread_bytes(s.b);
      const u32 base = s.b.pos, n = s.b.end - base < kWindow ? s.b.end - base : kWindow;
      win.reset(new u8[n]);
      std::memcpy(win.get(), block + base, n);
      place_window(s, win.get(), base, n);
    }
    const u32 pos0 = s.b.pos, bits0 = s.b.n, phase0 = s.phase;
    u32 n_tok, copy_src, copy_len;
    round(s, t, tok, n_tok, copy_src, copy_len);
    if (n_tok == 0 && copy_len == 0 && s.b.pos == pos0 && s.b.n == bits0 && s.phase == phase0) return 200;  // no progress: a bug
    for (u32 k = 0; k < n_tok; ++k) {
      const u32 dist = tok[k] >> 9;
      if (!dist) { text[at++] = static_cast<u8>(tok[k]); continue; }
      for (u32 l = tok[k] & 511u; l; --l, ++at) text[at] = text[at - dist];
    }
    for (u32 k = 0; k < copy_len; ++k) text[at++] = block[copy_src + k];
  }
  if (s.phase == kPhaseFailed) return s.status;
  u32 crc = 0xFFFFFFFFu;
  for (u32 k = 0; k < text_len; ++k) crc = crc_byte(crc, text[k]);
  return check_trailer(block, len, s.out, text_len, ~crc);
}

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: inflate_core_check <fixtures>\n"); return 2; }
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  u32 n = 0;
  if (std::fread(&n, 4, 1, f) != 1) return 2;
  std::unique_ptr<Tables> t(new Tables);
  int bad = 0;
  for (u32 m = 0; m < n; ++m) {
    u32 len = 0, text_len = 0;
    u8 expect = 0;
    if (std::fread(&len, 4, 1, f) != 1 || std::fread(&text_len, 4, 1, f) != 1 || std::fread(&expect, 1, 1, f) != 1) return 2;
    std::unique_ptr<u8[]> block(new u8[len]), want(new u8[text_len]);
    if (len && std::fread(block.get(), 1, len, f) != len) return 2;
    if (text_len && std::fread(want.get(), 1, text_len, f) != text_len) return 2;
    for (int form = 0; form < 2; ++form) {
      std::unique_ptr<u8[]> text(new u8[text_len]);
      std::memset(text.get(), 0xA5, text_len);
      const u32 st = form == 0 ? inflate_block(block.get(), len, text.get(), text_len, *t)
                               : inflate_windowed(block.get(), len, text.get(), text_len, *t);
      const bool same = text_len == 0 || std::memcmp(text.get(), want.get(), text_len) == 0;
      const bool ok = expect == 255 ? (st != 0 || same) : expect == 0 ? (st == 0 && same) : st == expect;
      if (!ok) {
        std::fprintf(stderr, "member %u (%s): status %u, expected %u%s\n", m, form ? "windowed" : "serial", st, expect,
                     st == 0 && !same ? ", text differs" : "");
        ++bad;
      }
    }
  }
  std::fclose(f);
  std::printf("%u members, %d wrong\n", n, bad);
  return bad ? 1 : 0;
}
