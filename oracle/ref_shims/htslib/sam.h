// Stand-in for <htslib/sam.h>: exactly what the reference mapper's sources use of it, kept as plain fields that
// ref_shims/bamxx.hpp prints as SAM text.  Our own code, written from the SAM specification; no BAM encoding.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

typedef int64_t hts_pos_t;

enum {
  BAM_FPAIRED = 1, BAM_FPROPER_PAIR = 2, BAM_FUNMAP = 4, BAM_FMUNMAP = 8, BAM_FREVERSE = 16, BAM_FMREVERSE = 32,
  BAM_FREAD1 = 64, BAM_FREAD2 = 128, BAM_FSECONDARY = 256, BAM_FQCFAIL = 512, BAM_FDUP = 1024, BAM_FSUPPLEMENTARY = 2048
};

// CIGAR words: length << 4 | op, ops in the order MIDNSHP=XB; bit 0 of an op's type: consumes the query, bit 1: the reference
#define bam_cigar_op(c) ((c) & 0xfu)
#define bam_cigar_oplen(c) ((c) >> 4)
#define bam_cigar_type(o) (0x3C1A7 >> ((o) << 1) & 3)

struct bam1_t {
  std::string qname, seq;
  uint16_t flag = 0;
  int32_t tid = -1, mtid = -1;
  hts_pos_t pos = -1, mpos = -1, isize = 0;
  uint8_t mapq = 0;
  std::vector<uint32_t> cigar;
  std::string aux;  // the optional fields as SAM text, each with its leading tab, in the order they were added
};

struct sam_hdr_t {
  std::string text;
  std::vector<std::string> names;  // @SQ SN: values, by tid
};

inline bam1_t *bam_init1() { return new bam1_t(); }
inline void bam_destroy1(bam1_t *b) { delete b; }

// (the base qualities are never given by the reference's callers: QUAL prints as "*")
inline int bam_set1(bam1_t *b, size_t l_qname, const char *qname, uint16_t flag, int32_t tid, hts_pos_t pos, uint8_t mapq,
                    size_t n_cigar, const uint32_t *cigar, int32_t mtid, hts_pos_t mpos, hts_pos_t isize, size_t l_seq,
                    const char *seq, const char * /*qual*/, size_t /*l_aux*/) {
  b->qname.assign(qname, l_qname);
  b->flag = flag;
  b->tid = tid;
  b->pos = pos;
  b->mapq = mapq;
  b->cigar.assign(cigar, cigar + n_cigar);
  b->mtid = mtid;
  b->mpos = mpos;
  b->isize = isize;
  b->seq.assign(seq, l_seq);
  b->aux.clear();
  return static_cast<int>(l_qname + l_seq);
}

inline int bam_aux_update_int(bam1_t *b, const char tag[2], int64_t val) {
  b->aux += '\t';
  b->aux.append(tag, 2);
  b->aux += ":i:" + std::to_string(val);
  return 0;
}

inline int bam_aux_append(bam1_t *b, const char tag[2], char type, int len, const uint8_t *data) {
  if (type != 'A' || len != 1) return -1;  // the one type the reference appends
  b->aux += '\t';
  b->aux.append(tag, 2);
  b->aux += ":A:";
  b->aux += static_cast<char>(data[0]);
  return 0;
}

inline sam_hdr_t *sam_hdr_init() { return new sam_hdr_t(); }

inline int sam_hdr_add_lines(sam_hdr_t *h, const char *lines, size_t len) {
  const size_t from = h->text.size();
  h->text.append(lines, len);
  for (size_t p = from; p < h->text.size();) {
    size_t e = h->text.find('\n', p);
    if (e == std::string::npos) e = h->text.size();
    if (h->text.compare(p, 4, "@SQ\t") == 0) {
      const size_t sn = h->text.find("\tSN:", p);
      if (sn == std::string::npos || sn >= e) return -1;
      h->names.push_back(h->text.substr(sn + 4, std::min(h->text.find('\t', sn + 4), e) - (sn + 4)));
    }
    p = e + 1;
  }
  return 0;
}
