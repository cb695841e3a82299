// Test program (CPU only, built with -fsanitize=address,undefined): abm_fastq_core.hpp over a file of cases, with output
// buffers of exactly the needed size, against what the file says each case must give.
//   file:  u32 n; per case: u32 min_letters, u64 text_bytes, the text, 4 x u64 + 2 x u32 of abm_fastq_info (n_records,
//          blob_bytes, line, value, max_len, code), u8 has_outputs; if has_outputs: the blob, (n + 1) x u64 off, n x u64
//          name_at, n x u32 name_len
// Two forms: parse_serial as abm_fastq_parse_host runs it, and every sequence line once more the way a lane group of the
// device takes it -- 16 lanes, four bytes each per step, their SeqScans merged -- which must give seq_rules' answer.
#include <cstdio>
#include <cstring>
#include <memory>

#include "../../abismal_amd/csrc/abm_fastq_core.hpp"

using namespace abm_fastq;

static bool get(std::FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

// one sequence line by 16 lanes; returns true if it agrees with seq_rules
static bool lanes_agree(const u8 *p, u32 len, u32 min_letters) {
  SeqScan lane[16];
  for (u32 l = 0; l < 16; ++l)
    for (u32 q = 4 * l; q < len; q += 64)
      for (u32 b = 0; b < 4 && q + b < len; ++b) seq_byte(lane[l], q + b, p[q + b]);
  for (u32 d = 1; d < 16; d <<= 1) {
    SeqScan next[16];
    for (u32 l = 0; l < 16; ++l) { next[l] = lane[l]; seq_merge(next[l], lane[l ^ d]); }
    std::memcpy(lane, next, sizeof lane);
  }
  u32 at = 0, n = 0, at2 = 0, n2 = 0;
  const u32 code = seq_finish(lane[5], min_letters, at, n), code2 = seq_rules(p, len, min_letters, at2, n2);
  return code == code2 && at == at2 && n == n2;
}

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: fastq_core_check <cases>\n"); return 2; }
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  u32 n_cases = 0;
  if (!get(f, &n_cases, 4)) return 2;
  int bad = 0;
  for (u32 m = 0; m < n_cases; ++m) {
    u32 min_letters = 0, w32[2];
    u64 text_bytes = 0, w64[4];
    u8 has_outputs = 0;
    if (!get(f, &min_letters, 4) || !get(f, &text_bytes, 8)) return 2;
    std::unique_ptr<u8[]> text(new u8[text_bytes]);
    if (!get(f, text.get(), text_bytes) || !get(f, w64, sizeof w64) || !get(f, w32, sizeof w32) || !get(f, &has_outputs, 1)) return 2;
    abm_fastq_info r;
    parse_serial(text.get(), text_bytes, min_letters, false, nullptr, nullptr, nullptr, nullptr, r);
    bool ok = r.n_records == w64[0] && r.code == w32[1] && r.line == w64[2] && r.value == w64[3];
    if (has_outputs) ok = ok && r.blob_bytes == w64[1] && r.max_len == w32[0];
    const u64 n = r.n_records;
    std::unique_ptr<u8[]> blob(new u8[r.blob_bytes]);
    std::unique_ptr<u64[]> off(new u64[n + 1]), name_at(new u64[n]);
    std::unique_ptr<u32[]> name_len(new u32[n]);
    abm_fastq_info again;
    parse_serial(text.get(), text_bytes, min_letters, true, blob.get(), off.get(), name_at.get(), name_len.get(), again);
    ok = ok && std::memcmp(&again, &r, sizeof r) == 0;
    if (has_outputs && ok) {
      std::unique_ptr<u8[]> want_blob(new u8[r.blob_bytes]);
      std::unique_ptr<u64[]> want_off(new u64[n + 1]), want_at(new u64[n]);
      std::unique_ptr<u32[]> want_len(new u32[n]);
      if (!get(f, want_blob.get(), r.blob_bytes) || !get(f, want_off.get(), (n + 1) * 8) || !get(f, want_at.get(), n * 8) || !get(f, want_len.get(), n * 4)) return 2;
      ok = std::memcmp(blob.get(), want_blob.get(), r.blob_bytes) == 0 && std::memcmp(off.get(), want_off.get(), (n + 1) * 8) == 0 &&
           std::memcmp(name_at.get(), want_at.get(), n * 8) == 0 && std::memcmp(name_len.get(), want_len.get(), n * 4) == 0;
    }
    else if (has_outputs) return 2;  // (the file cannot be followed any further)
    // every sequence line, the lanes' way
    u64 at = 0;
    for (u64 k = 0; at < text_bytes; ++k) {
      u64 le = at;
      while (le < text_bytes && text[le] != '\n') ++le;
      if (k % 4 == 1 && !too_long(le - at)) ok = ok && lanes_agree(text.get() + at, static_cast<u32>(le - at), min_letters);
      at = le + 1;
    }
    if (!ok) { std::fprintf(stderr, "case %u is wrong\n", m); ++bad; }
  }
  std::fclose(f);
  std::printf("%u cases, %d wrong\n", n_cases, bad);
  return bad ? 1 : 0;
}
