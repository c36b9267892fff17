// chain_text.hpp -- the text side of --chain and --chain-net: which flags a record's device problem carries, the coordinates of the two
// sides of a UCSC chain and the lines of the chain file, from a record's blocks (--chain) or from the pieces the net left it
// (--chain-net).  Pure host code on the standard library alone, so that it can be built on its own (scripts/micro/chain_check.cpp and
// scripts/micro/chain_net_check.cpp run it under the address and undefined-behaviour sanitizers).
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace chain {

// a record as its PAF line has it: the query window [qs, qe) and the target window [ts, te) on the forward strands, the two sequences'
// lengths, the strand
struct Record {
  std::string qname, tname;
  uint64_t qsize = 0, qs = 0, qe = 0, tsize = 0, ts = 0, te = 0;
  bool rev = false;
};

// a block as wfm_chain_runs gives it (wfm_chain_block_t), and what it says of the problem beside its blocks (of wfm_chaincall_t)
struct Block { uint32_t size, dt, dq, eq; };
struct Ends { uint32_t lead_dt = 0, lead_dq = 0, trail_dt = 0, trail_dq = 0, eq = 0; };

// The flags of a record's problem (WFM_CHAIN_SWAP = 1, WFM_CHAIN_REVERSE = 2).  The plain file runs from the target to the query: the
// runs as they are.  The swapped file's first side is the query, which a chain lists on its forward strand: every pair changes places,
// and the blocks of a - record, whose runs walk the query backwards, are taken from the last to the first.
inline uint32_t flags_of(bool swap, bool rev) { return swap ? (rev ? 3u : 1u) : 0u; }

// One chain WITHOUT its id: "chain score tName tSize + tStart tEnd qName qSize qStrand qStart qEnd " (the id and the newline are the
// writer's: number()), one line "size<TAB>dt<TAB>dq" per block, the last block's `size` alone, one empty line.  blocks, ends: what the
// device gave for the problem with flags_of(swap, r.rev).  The first side is always +; the second carries the record's strand and, on -,
// is counted on the reverse strand: [size - end, size - start).  A chain cannot spell the bases before its first and behind its last
// block: both sides begin lead_* later and end trail_* earlier.  score = the record's = columns: an integer that ranks longer and more
// identical chains first, not blastz's score.  Nothing is written for a record without blocks.
inline void chain_body(std::string& out, const Record& r, bool swap, const Ends& e, const Block* blocks, uint64_t n) {
  if (n == 0) return;
  const std::string &aname = swap ? r.qname : r.tname, &bname = swap ? r.tname : r.qname;
  const uint64_t asize = swap ? r.qsize : r.tsize, bsize = swap ? r.tsize : r.qsize;
  uint64_t as = swap ? r.qs : r.ts, ae = swap ? r.qe : r.te, bs = swap ? r.ts : r.qs, be = swap ? r.te : r.qe;
  if (r.rev) { const uint64_t s = bsize - be; be = bsize - bs; bs = s; }
  char num[200];
  out.append(num, (size_t)snprintf(num, sizeof num, "chain %u ", e.eq));
  out += aname;
  out.append(num, (size_t)snprintf(num, sizeof num, " %llu + %llu %llu ", (unsigned long long)asize, (unsigned long long)(as + e.lead_dt),
                                   (unsigned long long)(ae - e.trail_dt)));
  out += bname;
  out.append(num, (size_t)snprintf(num, sizeof num, " %llu %c %llu %llu \n", (unsigned long long)bsize, r.rev ? '-' : '+', (unsigned long long)(bs + e.lead_dq),
                                   (unsigned long long)(be - e.trail_dq)));
  for (uint64_t k = 0; k < n; ++k) {
    const Block& b = blocks[k];
    if (k + 1 < n) out.append(num, (size_t)snprintf(num, sizeof num, "%u\t%u\t%u\n", b.size, b.dt, b.dq));
    else out.append(num, (size_t)snprintf(num, sizeof num, "%u\n\n", b.size));
  }
}

// a piece as wfm_net_table gives it (wfm_net_piece_t): a global target start, the query offset from the first base the record's runs
// spell, in the direction of the runs, and a size
struct Piece { uint64_t order, t; uint32_t q, size; };

// One chain of --chain-net WITHOUT its id, from the n pieces the net left the record, in ascending t (and so ascending q): the header as
// chain_body's with score = the score the record competed with, tStart = the first piece's t - t_offset (the target sequence's place in
// the concatenation), tEnd = the last piece's end, qStart and qEnd from the first and last pieces' q behind where chain_body's second
// side begins (r.qs on +, qsize - r.qe on -: the runs of a - record walk the reverse strand); one line "size<TAB>dt<TAB>dq" per piece
// with the distances to the next piece on both sides (both may be non-zero: what lay between went to other records), the last piece's
// `size` alone, one empty line.  Nothing is written for a record that won nothing.
inline void net_body(std::string& out, const Record& r, uint64_t t_offset, uint32_t score, const Piece* pieces, uint64_t n) {
  if (n == 0) return;
  const uint64_t bs = r.rev ? r.qsize - r.qe : r.qs;
  const Piece &first = pieces[0], &last = pieces[n - 1];
  char num[200];
  out.append(num, (size_t)snprintf(num, sizeof num, "chain %u ", score));
  out += r.tname;
  out.append(num, (size_t)snprintf(num, sizeof num, " %llu + %llu %llu ", (unsigned long long)r.tsize, (unsigned long long)(first.t - t_offset),
                                   (unsigned long long)(last.t + last.size - t_offset)));
  out += r.qname;
  out.append(num, (size_t)snprintf(num, sizeof num, " %llu %c %llu %llu \n", (unsigned long long)r.qsize, r.rev ? '-' : '+', (unsigned long long)(bs + first.q),
                                   (unsigned long long)(bs + last.q + last.size)));
  for (uint64_t k = 0; k < n; ++k) {
    const Piece& p = pieces[k];
    if (k + 1 < n)
      out.append(num, (size_t)snprintf(num, sizeof num, "%u\t%llu\t%llu\n", p.size, (unsigned long long)(pieces[k + 1].t - (p.t + p.size)),
                                       (unsigned long long)((uint64_t)pieces[k + 1].q - ((uint64_t)p.q + p.size))));
    else out.append(num, (size_t)snprintf(num, sizeof num, "%u\n\n", p.size));
  }
}

// The chains of `text` (chain_body's) with their ids, *next, *next + 1, ... in the order they stand in, appended to `out`: a header is the
// line that begins with 'c' (a block line begins with a digit), and its id goes before its newline.  Returns the chains numbered.
inline uint64_t number(const std::string& text, uint64_t* next, std::string& out) {
  uint64_t n = 0;
  char num[32];
  for (size_t at = 0; at < text.size();) {
    size_t nl = text.find('\n', at);
    if (nl == std::string::npos) nl = text.size();
    out.append(text, at, nl - at);
    if (text[at] == 'c') { out.append(num, (size_t)snprintf(num, sizeof num, "%llu", (unsigned long long)(*next)++)); ++n; }
    if (nl < text.size()) out += '\n';
    at = nl + 1;
  }
  return n;
}

// --chain-net: what a record's chain needs beside its pieces, kept on the host under the order the record went to the net object with
struct NetHead {
  uint64_t order = 0;
  uint64_t t_offset = 0;  // where the target sequence begins in the concatenation
  Record rec;
};
// a record of the table as wfm_net_table gives it (wfm_netcall_t)
struct NetCall { uint64_t order; uint32_t score, zero; uint64_t first, count, bases_won, bases_aligned; };

// The file of --chain-net from the table of a net object: heads = what was kept of every record added, sorted by order as per[0, n_rec) is;
// a record's pieces are pieces[first, first + count).  The chains go to `out` (anything that takes << of a string) with their ids, a MiB at
// a time; *chains = the chains written, *lost = the records that won nothing.  false: the table's records are not the records added.
template <class Sink>
inline bool net_file(Sink& out, const std::vector<NetHead>& heads, const NetCall* per, size_t n_rec, const Piece* pieces, uint64_t* chains, uint64_t* lost) {
  *chains = *lost = 0;
  if (heads.size() != n_rec) return false;
  std::string body, text;
  uint64_t next = 1;
  for (size_t i = 0; i < n_rec; ++i) {
    const NetHead& hd = heads[i];
    if (hd.order != per[i].order) return false;
    if (per[i].count == 0) { ++*lost; continue; }
    net_body(body, hd.rec, hd.t_offset, per[i].score, pieces + per[i].first, per[i].count);
    if (body.size() >= ((size_t)1 << 20)) { text.clear(); *chains += number(body, &next, text); out << text; body.clear(); }
  }
  text.clear();
  *chains += number(body, &next, text);
  out << text;
  return true;
}

}  // namespace chain
