// Stand-alone check of abismal_amd/csrc/abm_deflate_core.hpp on the CPU, meant to be built with
//   g++ -O1 -g -fsanitize=address,undefined
// Reads a fixture file: u32 n, then per text  u32 text_len, text[text_len]  (text_len <= 0xff00).  Every text is copied
// into a heap buffer of exactly its length and encoded into a heap buffer of exactly text_len + 31 bytes -- what a member
// may take at most -- by the core's serial deflate_member; the member is then copied into a buffer of exactly its length
// and inflated again by the project's inflate core, whose status (header, stream, ISIZE, CRC-32) must be OK and whose
// text must be the input.  Exit status 0 = every member came back.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../abismal_amd/csrc/abm_deflate_core.hpp"

using namespace abm_deflate;

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: deflate_core_check <fixtures>\n"); return 2; }
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  u32 n = 0;
  if (std::fread(&n, 4, 1, f) != 1) return 2;
  std::unique_ptr<Shared> sh(new Shared);
  std::unique_ptr<abm_inflate::Tables> t(new abm_inflate::Tables);
  int bad = 0;
  for (u32 m = 0; m < n; ++m) {
    u32 text_len = 0;
    if (std::fread(&text_len, 4, 1, f) != 1 || text_len > kMaxText) return 2;
    std::unique_ptr<u8[]> text(new u8[text_len]);
    if (text_len && std::fread(text.get(), 1, text_len, f) != text_len) return 2;
    const u32 room = text_len + kHeader + kStoredExtra + kTrailer;
    std::unique_ptr<u8[]> slot(new u8[room]);
    std::memset(slot.get(), 0xA5, room);
    const u32 len = deflate_member(text.get(), text_len, slot.get(), *sh);
    if (len > room) { std::fprintf(stderr, "text %u: a member of %u bytes from %u bytes of text\n", m, len, text_len); ++bad; continue; }
    std::unique_ptr<u8[]> member(new u8[len]), back(new u8[text_len]);
    std::memcpy(member.get(), slot.get(), len);
    std::memset(back.get(), 0x5A, text_len);
    const u32 st = abm_inflate::inflate_block(member.get(), len, back.get(), text_len, *t);
    const bool same = text_len == 0 || std::memcmp(back.get(), text.get(), text_len) == 0;
    if (st != ABM_INFLATE_OK || !same) {
      std::fprintf(stderr, "text %u (%u bytes): status %u%s\n", m, text_len, st, st == 0 ? ", text differs" : "");
      ++bad;
    }
  }
  std::fclose(f);
  std::printf("%u members, %d wrong\n", n, bad);
  return bad ? 1 : 0;
}
