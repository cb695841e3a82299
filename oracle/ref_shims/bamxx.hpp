// Stand-in for bamxx.hpp: the reference's input files as plain (uncompressed) text and its output as SAM text, written by
// the SAM specification's rules -- 1-based POS and PNEXT, "=" for a mate on the same chromosome, "*" for none, SEQ through
// the 4-bit code table, QUAL "*", optional fields in the order they were added.  Our own code; no BAM output.
#pragma once
#include <htslib/sam.h>

#include <cstddef>
#include <fstream>
#include <stdexcept>
#include <string>

namespace bamxx {

struct bam_rec {
  bam1_t *b{};
};

struct bam_header {
  sam_hdr_t *h{};
};

struct bgzf_file {
  std::ifstream f;
  bgzf_file() = default;
  bgzf_file(const std::string &fn, const std::string & /*mode*/) : f(fn, std::ios::binary) {}
  operator bool() const { return static_cast<bool>(f); }
  size_t tellg() const { return static_cast<size_t>(const_cast<std::ifstream &>(f).tellg()); }
};

inline bgzf_file &getline(bgzf_file &in, std::string &line) {
  std::getline(in.f, line);
  return in;
}

// A base is stored as a 4-bit code and printed from it: "=ACMGRSVTWYHKDBN", either letter case, and 0-3 for A, C, G, T;
// any other byte has code 15 and prints as N.
inline char seq_text(char c) {
  static const char codes[] = "=ACMGRSVTWYHKDBN";
  switch (c) {
  case '0': return 'A';
  case '1': return 'C';
  case '2': return 'G';
  case '3': return 'T';
  default: break;
  }
  const char u = (c >= 'a' && c <= 'z') ? static_cast<char>(c - 'a' + 'A') : c;
  for (const char *p = codes; *p; ++p)
    if (*p == u) return u;
  return 'N';
}

struct bam_out {
  std::ofstream f;
  std::string line;
  bam_out(const std::string &fn, bool bam_format) : f(fn, std::ios::binary) {
    if (bam_format) throw std::runtime_error("this build of the reference mapper writes SAM text only");
  }
  operator bool() const { return static_cast<bool>(f); }

  bool write(const bam_header &hdr) {
    f << hdr.h->text;
    return static_cast<bool>(f);
  }

  bool write(const bam_header &hdr, const bam_rec &rec) {
    static const char ops[] = "MIDNSHP=XB";
    const bam1_t &b = *rec.b;
    const auto name = [&](int32_t tid) -> const std::string & { return hdr.h->names.at(static_cast<size_t>(tid)); };
    line.clear();
    line += b.qname.empty() ? "*" : b.qname;
    line += '\t' + std::to_string(b.flag) + '\t';
    line += b.tid < 0 ? "*" : name(b.tid);
    line += '\t' + std::to_string(b.pos + 1) + '\t' + std::to_string(b.mapq) + '\t';
    if (b.cigar.empty()) line += '*';
    for (const uint32_t c : b.cigar) {
      line += std::to_string(bam_cigar_oplen(c));
      line += bam_cigar_op(c) < 10 ? ops[bam_cigar_op(c)] : '?';
    }
    line += '\t';
    line += b.mtid < 0 ? "*" : (b.mtid == b.tid ? "=" : name(b.mtid));
    line += '\t' + std::to_string(b.mpos + 1) + '\t' + std::to_string(b.isize) + '\t';
    if (b.seq.empty()) line += '*';
    for (const char c : b.seq) line += seq_text(c);
    line += "\t*";
    line += b.aux;
    line += '\n';
    f << line;
    return static_cast<bool>(f);
  }
};

}  // namespace bamxx
