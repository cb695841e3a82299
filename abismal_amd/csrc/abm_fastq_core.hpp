// abismal_amd: FASTQ text into reads with ReadLoader's rules (src/abismal.cpp:164-201), shared by the CLI's host parser
// (parse_raw, abm_cli_fastq.hpp), by the device kernels (abm_fastq.hip) and by plain host C++ (abm_fastq_parse_host;
// tests/cpp/fastq_core_check.cpp runs it under sanitizers).  What a line is, which record it belongs to, what a name is,
// how a sequence line becomes a read and what counts as an error are written here and only here.
//
// Lines: only '\n' ends a line; a line exists if it starts before the end of the text, so a last line without a newline
// counts.  Line k belongs to record k / 4; L lines are (L + 2) / 4 records (a trailing name line without its sequence
// line is not one).  Lines 4j + 2 and 4j + 3 are never looked at.
// Name (line 4j): an empty line is ABM_FASTQ_EMPTY_NAME; otherwise the bytes after the line's first byte up to the first
// space, tab or end of line (the first byte is not checked, the length may be 0).
// Sequence (line 4j + 1): 32767 bytes or more are ABM_FASTQ_TOO_LONG.  With fewer than min_letters bytes that are not 'N'
// the read is empty; otherwise trailing 'N's go, then everything before the first A, C, G or T; if nothing is left that is
// ABM_FASTQ_NO_BASE.  A '\r' is a byte like any other.
// Errors: the one on the lowest line is the call's (the host throws at the first): a minimum over error_key(line, code).
//
// Bounds: every function here reads [p, p + len) of what it is given and nothing else; parse_serial writes blob[0,
// blob_bytes), off[0, n_records], name_at / name_len[0, n_records) and only when told to (its caller has compared them
// with the capacities).
#pragma once
#include <stdint.h>

#include "../../include/abismal_amd.h"

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define ABM_FQ_HD __host__ __device__
#else
#define ABM_FQ_HD
#endif

namespace abm_fastq {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 kTileBytes = ABM_FASTQ_TILE_BYTES;        // text per tile: the unit newlines are counted and ranked by
constexpr u32 kScanTiles = ABM_FASTQ_SCAN_TILES;        // tile counts (and chunk sums) scanned per step of the one-workgroup scans
constexpr u32 kChunkRecords = ABM_FASTQ_CHUNK_RECORDS;  // records per chunk: the unit read lengths are summed and scanned by
constexpr u32 kMaxRead = 32767;                         // padding_size: a sequence line this long or longer is an error
constexpr u64 kNoError = ~0ull;
constexpr u32 kNoBase = 0xFFFFFFFFu;

ABM_FQ_HD inline u64 records_of(u64 lines) { return (lines + 2) / 4; }
ABM_FQ_HD inline u64 error_key(u64 line, u32 code) { return (line << 2) | code; }
ABM_FQ_HD inline u64 key_line(u64 key) { return key >> 2; }
ABM_FQ_HD inline u32 key_code(u64 key) { return static_cast<u32>(key & 3u); }
ABM_FQ_HD inline bool ends_name(u8 c) { return c == ' ' || c == '\t'; }
ABM_FQ_HD inline bool is_base(u8 c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
ABM_FQ_HD inline bool informative(u8 c) { return c != 'N'; }
ABM_FQ_HD inline bool too_long(u64 len) { return len >= kMaxRead; }

// What a pass over a sequence line gathers, in any order and in any number of pieces: the bytes that are not 'N', one past
// the last of them, the first A/C/G/T.  (An A/C/G/T is not an 'N', so a line with one has first < end.)
struct SeqScan {
  u32 letters = 0, end = 0, first = kNoBase;
};
ABM_FQ_HD inline void seq_byte(SeqScan &s, u32 i, u8 c) {
  if (informative(c)) { ++s.letters; s.end = s.end > i + 1 ? s.end : i + 1; }
  if (is_base(c)) s.first = s.first < i ? s.first : i;
}
ABM_FQ_HD inline void seq_merge(SeqScan &s, const SeqScan &o) {
  s.letters += o.letters;
  s.end = s.end > o.end ? s.end : o.end;
  s.first = s.first < o.first ? s.first : o.first;
}
// the read of a scanned line: bytes [at, at + n) of it; returns the line's code
ABM_FQ_HD inline u32 seq_finish(const SeqScan &s, u32 min_letters, u32 &at, u32 &n) {
  at = n = 0;
  if (s.letters < min_letters) return ABM_FASTQ_OK;
  if (s.first == kNoBase) return ABM_FASTQ_NO_BASE;
  at = s.first;
  n = s.end - s.first;
  return ABM_FASTQ_OK;
}

// ---- one thread, one line ------------------------------------------------------------------------------------------
// the name of a name line of len >= 1 bytes: bytes [1, 1 + the value) of it
ABM_FQ_HD inline u32 name_length(const u8 *p, u64 len) {
  u64 q = 1;
  while (q < len && !ends_name(p[q])) ++q;
  return static_cast<u32>(q - 1);
}
// a sequence line of fewer than kMaxRead bytes, as ReadLoader takes it (the counting loop vectorises; the two trims stop
// at the first byte that stays)
ABM_FQ_HD inline u32 seq_rules(const u8 *p, u32 len, u32 min_letters, u32 &at, u32 &n) {
  SeqScan s;
  for (u32 i = 0; i < len; ++i) s.letters += informative(p[i]);
  if (s.letters >= min_letters) {
    u32 e = len;
    while (e > 0 && !informative(p[e - 1])) --e;
    u32 b = 0;
    while (b < e && !is_base(p[b])) ++b;
    s.end = e;
    s.first = b < e ? b : kNoBase;
  }
  return seq_finish(s, min_letters, at, n);
}

// ---- the whole text, serially: the specification of the device's bytes -----------------------------------------------
// Fills info from the text alone.  write: also the outputs (blob, off, and name_at / name_len unless null), which must hold
// what info says.  A record whose sequence line is an error is an empty read; the walk goes on, so info is the same
// whoever computes it.
inline void parse_serial(const u8 *text, u64 text_bytes, u32 min_letters, bool write, u8 *blob, u64 *off, u64 *name_at, u32 *name_len,
                         abm_fastq_info &info) {
  u64 key = kNoError, value = 0, n = 0, total = 0, at = 0, name_pos = 0;
  u32 max_len = 0, name_n = 0;
  if (write) off[0] = 0;
  for (u64 k = 0; at < text_bytes; ++k) {
    u64 le = at;
    while (le < text_bytes && text[le] != '\n') ++le;
    const u64 len = le - at;
    if (k % 4 == 0) {
      if (len == 0) { const u64 e = error_key(k, ABM_FASTQ_EMPTY_NAME); key = key < e ? key : e; }
      name_pos = at + 1;
      name_n = len ? name_length(text + at, len) : 0u;
    }
    else if (k % 4 == 1) {
      u32 r_at = 0, r_n = 0, code = ABM_FASTQ_OK;
      if (too_long(len)) code = ABM_FASTQ_TOO_LONG;
      else code = seq_rules(text + at, static_cast<u32>(len), min_letters, r_at, r_n);
      if (code != ABM_FASTQ_OK) {
        const u64 e = error_key(k, code);
        if (e < key) { key = e; value = code == ABM_FASTQ_TOO_LONG ? len : 0; }
      }
      if (write) {
        for (u32 i = 0; i < r_n; ++i) blob[total + i] = text[at + r_at + i];
        off[n + 1] = total + r_n;
        if (name_at) name_at[n] = name_pos;
        if (name_len) name_len[n] = name_n;
      }
      total += r_n;
      max_len = max_len > r_n ? max_len : r_n;
      ++n;
    }
    at = le + 1;  // (past the text's end after a last line without a newline)
  }
  info.n_records = n;
  info.blob_bytes = total;
  info.max_len = max_len;
  info.code = key == kNoError ? static_cast<u32>(ABM_FASTQ_OK) : key_code(key);
  info.line = key == kNoError ? 0 : key_line(key);
  info.value = key == kNoError || key_code(key) != ABM_FASTQ_TOO_LONG ? 0 : value;
}

}  // namespace abm_fastq
