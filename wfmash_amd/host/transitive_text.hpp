// transitive_text.hpp -- the text side of --transitive: the world the records and seeds live in, the BED file of seed intervals, a
// record's place in the world and the lines of the output file.  Pure host code on the standard library alone, so that it can be built on
// its own (scripts/micro/transitive_check.cpp runs it under the address and undefined-behaviour sanitizers).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <unordered_map>
#include <vector>

#include "lift_text.hpp"

namespace transitive {

// One coordinate space: the target sequences in index order, then the query sequences whose names no target has, in query index order.
// offsets: where each sequence begins, and the world's size behind the last.
struct World {
  std::vector<std::string> names;
  std::vector<uint64_t> lengths, offsets{0};
  std::unordered_map<std::string, int> index;
  int find(const std::string& name) const {
    const auto it = index.find(name);
    return it == index.end() ? -1 : it->second;
  }
  uint64_t n_bases() const { return offsets.back(); }
  bool add(const std::string& name, uint64_t length) {
    if (!index.emplace(name, (int)names.size()).second) return false;
    names.push_back(name);
    lengths.push_back(length);
    offsets.push_back(offsets.back() + length);
    return true;
  }
  // the sequence that holds world base x < n_bases (sequences without bases hold none)
  size_t seq_of(uint64_t x) const { return (size_t)(std::upper_bound(offsets.begin(), offsets.end(), x) - offsets.begin()) - 1; }
};

inline World make_world(const std::vector<std::string>& tnames, const std::vector<uint64_t>& tlengths, const std::vector<std::string>& qnames,
                        const std::vector<uint64_t>& qlengths) {
  World w;
  for (size_t i = 0; i < tnames.size(); ++i) w.add(tnames[i], tlengths[i]);  // (a name the target has twice is its first sequence, as find is)
  for (size_t i = 0; i < qnames.size(); ++i) w.add(qnames[i], qlengths[i]);
  return w;
}

// the seeds: lift::parse_bed's lines with its skip rules and counts, names looked up in the world, in INPUT order
inline lift::Bed parse_seeds(const std::string& text, const World& w) {
  lift::Bed bed = lift::parse_bed(text, [&](const std::string& name) { return w.find(name); }, w.lengths, w.offsets);
  std::sort(bed.iv.begin(), bed.iv.end(), [](const lift::Interval& a, const lift::Interval& b) { return a.order < b.order; });
  return bed;
}

// where the first base of a record's FORWARD query window lies in the world: the window is [qs, qe) of the query sequence that begins at
// q_offset, whatever the strand (on the reverse strand the text is its reverse complement)
inline uint64_t query_world(uint64_t q_offset, uint64_t qs) { return q_offset + qs; }

// [a, b) of the world as lines "seq start end name seed_seq seed_start seed_end", split where it crosses from one sequence into the
// next (the union merges abutting bases of neighbouring sequences).  Returns the lines written.
inline uint64_t lines(std::string& out, const World& w, const lift::Interval& seed, uint64_t a, uint64_t b) {
  uint64_t n = 0;
  char num[200];
  for (size_t s = a < b ? w.seq_of(a) : 0; a < b; ++s) {
    const uint64_t e = std::min(b, w.offsets[s + 1]);
    if (e <= a) continue;  // (a sequence without bases)
    out += w.names[s];
    out.append(num, (size_t)snprintf(num, sizeof num, "\t%llu\t%llu\t", (unsigned long long)(a - w.offsets[s]), (unsigned long long)(e - w.offsets[s])));
    out += seed.name;
    out += '\t';
    out += w.names[(size_t)seed.seq];
    out.append(num, (size_t)snprintf(num, sizeof num, "\t%llu\t%llu\n", (unsigned long long)seed.start, (unsigned long long)seed.end));
    a = e;
    ++n;
  }
  return n;
}

// an interval of the closure and a seed's share of them, as wfm_trans_closure gives them (wfm_trans_iv_t, wfm_trans_seed_t)
struct ClosureIv { uint64_t start, end; uint32_t seed, pad_; };
struct SeedCall { uint64_t first, count, bases; };

// The file of --transitive: per seed, in the order given, the lines of its intervals ivs[first, first + count).  ivs null: no record was
// added, and a seed reaches itself.  The text goes to `out` (anything that takes << of a string) a MiB at a time.  Returns the lines written.
template <class Sink>
inline uint64_t file(Sink& out, const World& w, const std::vector<lift::Interval>& seeds, const SeedCall* per, const ClosureIv* ivs) {
  std::string text;
  uint64_t n = 0;
  for (size_t i = 0; i < seeds.size(); ++i) {
    if (!ivs) n += lines(text, w, seeds[i], seeds[i].gstart, seeds[i].gend);
    else
      for (uint64_t k = per[i].first; k < per[i].first + per[i].count; ++k) n += lines(text, w, seeds[i], ivs[k].start, ivs[k].end);
    if (text.size() >= ((size_t)1 << 20)) { out << text; text.clear(); }
  }
  out << text;
  return n;
}

}  // namespace transitive
