// packed_runs.hpp -- what a stage of the across-record passes consumes (run_passes.hpp), and its two sources: the written records of an
// align batch, packed from their ops (pack_ops), and the lines of an existing aligned PAF, packed from their cg:Z: (pack_line,
// read_packed_lines).  A packed record is what its line spells: the runs between the leading and trailing I and D runs (trim_and_filter's
// rule), at base = the target sequence's offset in the concatenation + the target start the line has.  Pure host code on cigar_ops.hpp,
// chain_text.hpp and coverage_text.hpp, so that it can be built on its own (scripts/micro/packed_runs_check.cpp holds the two sources
// against each other under the address and undefined-behaviour sanitizers).
#pragma once

#include <cstdint>
#include <istream>
#include <string>
#include <utility>
#include <vector>

#include "chain_text.hpp"
#include "cigar_ops.hpp"
#include "coverage_text.hpp"

namespace wflign {

// where a packed record's two sequences lie: the column of the query's group (--pav, --genotypes; none: a number no object has), the world
// place of the query sequence's first base (--transitive) and the target sequence's offset in the concatenation
struct Place {
  uint32_t group = 0xffffffffu;
  uint64_t query_world = 0, target_off = 0;
};

struct PackedRuns {
  // in, per packed record
  std::vector<wfm_cov_prob_t> probs;   // base, runs_off, n_runs
  std::vector<uint32_t> runs;          // their trimmed ops as run words
  std::vector<chain::Record> where;    // the record as its line has it: the forward windows [qs, qe) and [ts, te) the runs spell, sizes, strand, names
  std::vector<Place> place;
  std::vector<size_t> rec;             // (an align batch's only) the record's index in the batch
  uint64_t order_base = 0;             // --chain-net: record j's order is order_base + j (an align batch: its number << 32; a PAF: the lines taken before)
  uint64_t unknown = 0;                // records whose ops the runs cannot hold: in no list
  double ms = 0;                       // what the packing took
  // out, per packed record ("" where the stage is off, or the device refused the record), and --chain-net's heads of the records added
  std::vector<std::string> lift, chain;
  std::vector<chain::NetHead> net_heads;

  size_t size() const { return probs.size(); }
  void clear() {
    probs.clear(); runs.clear(); where.clear(); place.clear(); rec.clear(); lift.clear(); chain.clear(); net_heads.clear();
    order_base = unknown = 0; ms = 0;
  }
};

// One record's ops.  cr comes with the record's names, sizes and strand and with its WINDOWS -- [qs, qe) of the query on the forward
// strand, ts of the target -- and is packed with what the runs spell inside them.  1: packed; 0: the ops are I and D alone, nothing is
// packed; -1: an op outside =XID or a count of 0 or of 2^30 and more -- counted in pk.unknown, and no run of it stays behind.
inline int pack_ops(PackedRuns& pk, const CigarOps& ops, chain::Record cr, const Place& place) {
  size_t ob = 0, oe = ops.size();
  uint64_t ta = 0, qa = 0, q_len = 0, t_len = 0;
  while (ob < oe && (ops[ob].second == 'I' || ops[ob].second == 'D')) { (ops[ob].second == 'D' ? ta : qa) += (uint64_t)ops[ob].first; ++ob; }
  while (oe > ob && (ops[oe - 1].second == 'I' || ops[oe - 1].second == 'D')) --oe;
  if (oe == ob) return 0;
  const wfm_cov_prob_t p{place.target_off + cr.ts + ta, (uint64_t)pk.runs.size(), (uint32_t)(oe - ob), 0u};
  for (size_t k = ob; k < oe; ++k) {
    const char c = ops[k].second;
    const uint32_t op = c == '=' ? 0u : c == 'X' ? 1u : c == 'I' ? 2u : c == 'D' ? 3u : 4u;
    if (op > 3u || ops[k].first <= 0 || (uint32_t)ops[k].first >= (1u << 30)) {
      pk.runs.resize((size_t)p.runs_off);
      ++pk.unknown;
      return -1;
    }
    pk.runs.push_back(((uint32_t)ops[k].first << 2) | op);
    if (op != 3u) q_len += (uint64_t)ops[k].first;
    if (op != 2u) t_len += (uint64_t)ops[k].first;
  }
  cr.qs = cr.rev ? cr.qe - qa - q_len : cr.qs + qa;
  cr.qe = cr.qs + q_len;
  cr.ts += ta;
  cr.te = cr.ts + t_len;
  pk.probs.push_back(p);
  pk.where.push_back(std::move(cr));
  pk.place.push_back(place);
  return 1;
}

// One line of an aligned PAF that coverage::classify_line let through: its runs as they stand, at its own coordinates.
inline void pack_line(PackedRuns& pk, const verify::Line& l, const Place& place) {
  pk.probs.push_back(wfm_cov_prob_t{place.target_off + (uint64_t)l.ts, (uint64_t)pk.runs.size(), (uint32_t)l.runs.size(), 0u});
  pk.runs.insert(pk.runs.end(), l.runs.begin(), l.runs.end());
  chain::Record cr;
  cr.qname = l.qname; cr.tname = l.tname; cr.rev = l.rev;
  cr.qsize = (uint64_t)l.qlen; cr.qs = (uint64_t)l.qs; cr.qe = (uint64_t)l.qe;
  cr.tsize = (uint64_t)l.tlen; cr.ts = (uint64_t)l.ts; cr.te = (uint64_t)l.te;
  pk.where.push_back(std::move(cr));
  pk.place.push_back(place);
}

// a batch of lines goes to the device once it holds this many problems or runs
struct BatchLimits { size_t records = 65536, runs = (size_t)16 << 20; };

// The lines of an aligned PAF in batches.  A line is read and skipped by one rule (coverage::classify_line over find(name) -> the target
// sequence's index or a negative number, lengths and offsets: the target's sequences and where each begins); skipped[code] counts what
// the rule left out, by coverage::LINE_*.  hook(line, place) -> false: the caller leaves the line out, and counts it; it fills what of the
// place its stage reads (the target's offset is there).  flush(pk): a batch, its order_base = the lines taken before it.
template <class Find, class Hook, class Flush>
inline void read_packed_lines(std::istream& in, Find find, const std::vector<uint64_t>& lengths, const std::vector<uint64_t>& offsets, const BatchLimits& lim,
                              uint64_t skipped[5], Hook hook, Flush flush) {
  PackedRuns pk;
  uint64_t taken = 0;
  auto flush_batch = [&]() {
    if (pk.probs.empty()) return;
    pk.order_base = taken;
    taken += pk.size();
    flush(pk);
    pk.clear();
  };
  std::string line;
  verify::Line l;
  while (std::getline(in, line)) {
    if (line.empty() || line[0] == '@') continue;
    int ti = -1;
    const int code = coverage::classify_line(line, find, lengths, l, &ti);
    if (code != coverage::LINE_ADD) { skipped[code]++; continue; }
    Place place;
    place.target_off = offsets[(size_t)ti];
    if (!hook(l, place)) continue;
    pack_line(pk, l, place);
    if (pk.probs.size() >= lim.records || pk.runs.size() >= lim.runs) flush_batch();
  }
  flush_batch();
}

}  // namespace wflign
