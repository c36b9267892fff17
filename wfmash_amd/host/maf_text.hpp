// maf_text.hpp -- the text side of --maf: the header and the paragraph of one block of wfm_maf_rows (include/wfmash_hip.h) on the
// coordinates of the record's line.  Pure host code on the standard library alone, so that it can be built on its own
// (scripts/micro/maf_check.cpp).
//
//   ##maf version=1
//
//   a score=<eq>
//   s <tname> <tstart> <psize> + <tlen_total> <row P>
//   s <qname> <qstart> <tsize> <+|-> <qlen_total> <row T>
//   <empty line>
//
// Single spaces, no padding (UCSC's writers pad the columns; readers split on whitespace).  score = the block's = columns, the quantity
// --chain uses: not a blastz score.  tstart = the line's target start + p.  qstart = the line's query start + t on +, and
// qlen_total - the line's query end + t on -: MAF counts a - row on the reverse-complemented source, and row T IS that strand.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>

namespace maf {

inline const char* header() { return "##maf version=1\n"; }

struct Block { uint64_t off; uint32_t problem, p, t, psize, tsize, cols, eq, x; };  // restates wfm_maf_block_t (wfmash_hip.h)

// the record as its line has it: the forward windows [ts, ..) and [qs, qe) the runs spell, the sequences' lengths, the strand
struct Line {
  const std::string* tname;
  uint64_t ts, tsize;
  const std::string* qname;
  uint64_t qs, qe, qsize;
  bool rev;
};

inline uint64_t target_start(const Line& l, const Block& b) { return l.ts + b.p; }
inline uint64_t query_start(const Line& l, const Block& b) { return (l.rev ? l.qsize - l.qe : l.qs) + b.t; }

// an upper bound of the bytes block() appends for the n blocks of one record: reserve it ONCE per record (a reserve per block would
// copy the record's earlier paragraphs again with every block of a split record)
inline size_t record_bytes(const Line& l, const Block* blocks, size_t n) {
  size_t bytes = 0;
  for (size_t k = 0; k < n; ++k) bytes += 2 * (size_t)blocks[k].cols;
  // per block beside the rows and the names: "a score=" 10 digits, two "s " lines with 20 + 10 + 20 digits each, strands, spaces, newlines
  return bytes + n * (l.tname->size() + l.qname->size() + 160);
}

// one paragraph behind `out`; rows: the call's row bytes (the block's are rows[off .. off + 2 cols))
inline void block(std::string& out, const Line& l, const Block& b, const char* rows) {
  char num[96];
  out.append(num, (size_t)snprintf(num, sizeof num, "a score=%u\ns ", b.eq));
  out += *l.tname;
  out.append(num, (size_t)snprintf(num, sizeof num, " %llu %u + %llu ", (unsigned long long)target_start(l, b), b.psize, (unsigned long long)l.tsize));
  out.append(rows + b.off, b.cols);
  out += "\ns ";
  out += *l.qname;
  out.append(num, (size_t)snprintf(num, sizeof num, " %llu %u %c %llu ", (unsigned long long)query_start(l, b), b.tsize, l.rev ? '-' : '+',
                                   (unsigned long long)l.qsize));
  out.append(rows + b.off + b.cols, b.cols);
  out += "\n\n";
}

}  // namespace maf
