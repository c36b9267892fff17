// coverage_text.hpp -- the text side of --coverage: the bedGraph of a run's depth intervals, and an aligned PAF line as --coverage-paf
// takes it.  Pure host code on verify_parse.hpp alone, so that it can be built on its own (scripts/micro/coverage_check.cpp runs it
// under the address and undefined-behaviour sanitizers).
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "verify_parse.hpp"

namespace coverage {

// an interval of constant depth over the concatenation of the target's sequences; it ends where the next begins
struct Interval { uint64_t start; uint32_t depth; };

// The bedGraph (no track line): name, start, end, depth, separated by tabs.  iv: ascending starts, the first at 0 (none at all: depth 0
// everywhere); the last interval runs to the end of the last sequence.  Sequences in index order; an interval that straddles a sequence
// boundary is split there, a sequence nothing touched is one line of depth 0, a sequence of length 0 has no line: per sequence the
// lines tile [0, length) exactly, and neighbours differ in depth.  *lines: the number of lines written.
inline std::string coverage_bedgraph(const std::vector<std::string>& names, const std::vector<uint64_t>& lengths, const std::vector<Interval>& iv,
                                     uint64_t* lines) {
  std::string out;
  uint64_t n_lines = 0, g0 = 0;
  size_t k = 0;  // the interval that holds the base in hand
  char num[96];
  for (size_t c = 0; c < names.size() && c < lengths.size(); ++c) {
    const uint64_t g1 = g0 + lengths[c];
    uint64_t a = g0, line_a = g0;
    uint32_t line_depth = 0;
    bool open = false;
    auto close = [&]() {
      if (!open) return;
      out += names[c];
      out.append(num, (size_t)snprintf(num, sizeof num, "\t%llu\t%llu\t%u\n", (unsigned long long)(line_a - g0), (unsigned long long)(a - g0), line_depth));
      ++n_lines;
      open = false;
    };
    while (a < g1) {
      while (k + 1 < iv.size() && iv[k + 1].start <= a) ++k;
      const uint32_t depth = iv.empty() || iv[k].start > a ? 0u : iv[k].depth;
      uint64_t b = g1;
      if (!iv.empty() && iv[k].start > a) b = iv[k].start < g1 ? iv[k].start : g1;            // (before the first interval)
      else if (k + 1 < iv.size() && iv[k + 1].start < g1) b = iv[k + 1].start;
      if (open && depth != line_depth) close();
      if (!open) { open = true; line_a = a; line_depth = depth; }
      a = b;
    }
    close();
    g0 = g1;
  }
  if (lines) *lines = n_lines;
  return out;
}

// the same from the intervals as wfm_coverage_intervals gives them (Raw: wfm_cov_interval_t, or anything with its start and depth)
template <class Raw>
inline std::string coverage_bedgraph(const std::vector<std::string>& names, const std::vector<uint64_t>& lengths, const Raw* raw, size_t n, uint64_t* lines) {
  std::vector<Interval> iv(n);
  for (size_t i = 0; i < n; ++i) iv[i] = Interval{raw[i].start, raw[i].depth};
  return coverage_bedgraph(names, lengths, iv, lines);
}

// What --coverage-paf makes of a line.  LINE_ADD: its runs count, at base = the target sequence's offset + ts.  Everything else is
// skipped and counted: no cg:Z: tag or an op outside =XID, a malformed line (verify::parse_line's rules, or a CIGAR whose target
// bases are not te - ts), a target name the file does not have, a tlen that is not the file's.
enum { LINE_ADD = 0, LINE_NO_CIGAR = 1, LINE_MALFORMED = 2, LINE_UNKNOWN_TARGET = 3, LINE_TLEN = 4 };
inline const char* line_reason(int code) {
  static const char* const names[5] = {"added", "no =XID cg:Z:", "malformed", "unknown target", "tlen differs"};
  return code >= 0 && code < 5 ? names[code] : "?";
}

// find(name) -> the index of the target sequence or a negative number; lengths: the file's
template <class Find>
inline int classify_line(const std::string& text, Find find, const std::vector<uint64_t>& lengths, verify::Line& l, int* target) {
  const int st = verify::parse_line(text, l, nullptr);
  if (st == verify::LINE_UNVERIFIABLE) return LINE_NO_CIGAR;
  if (st != verify::LINE_OK) return LINE_MALFORMED;
  uint64_t bases = 0;
  for (uint32_t w : l.runs) if ((w & 3u) != 2u) bases += w >> 2;
  if (bases != (uint64_t)(l.te - l.ts)) return LINE_MALFORMED;
  const int idx = find(l.tname);
  if (idx < 0 || (size_t)idx >= lengths.size()) return LINE_UNKNOWN_TARGET;
  if ((uint64_t)l.tlen != lengths[(size_t)idx]) return LINE_TLEN;
  if (target) *target = idx;
  return LINE_ADD;
}

}  // namespace coverage
