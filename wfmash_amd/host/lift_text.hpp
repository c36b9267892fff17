// lift_text.hpp -- the text side of --lift: the BED file of target intervals as the align phase reads it, the strand arithmetic of a
// lift and the lines of the lift file.  Pure host code on the standard library alone, so that it can be built on its own
// (scripts/micro/lift_check.cpp runs it under the address and undefined-behaviour sanitizers).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace lift {

// a BED line that was kept: [start, end) of target sequence seq, its name ("." without a fourth column), its number among the lines
// kept, and where it lies in the concatenation of the target's sequences
struct Interval {
  int seq = 0;
  uint64_t start = 0, end = 0;
  std::string name;
  uint64_t order = 0;
  uint64_t gstart = 0, gend = 0;
};

// the intervals sorted by (gstart, gend, order) -- what wfm_liftset_create takes -- and the number of lines skipped
struct Bed {
  std::vector<Interval> iv;
  uint64_t skipped = 0;
};

// a plain decimal of 1 .. 18 digits
inline bool decimal(const std::string& s, size_t a, size_t b, uint64_t* v) {
  if (b <= a || b - a > 18) return false;
  uint64_t x = 0;
  for (size_t i = a; i < b; ++i) {
    if (s[i] < '0' || s[i] > '9') return false;
    x = x * 10 + (uint64_t)(s[i] - '0');
  }
  *v = x;
  return true;
}

// Tab-separated, three columns at least; column 4 is the name.  Skipped and counted: blank lines, lines that begin with '#', `track` and
// `browser` lines, fewer than three columns, a start or end that is not a plain decimal, a sequence the target does not have
// (find(name) < 0), start >= end, end beyond the sequence.  A '\r' before the newline is dropped; what follows the last newline is no
// line.  lengths: the target's sequences; offsets: where each begins in their concatenation.
template <class Find>
inline Bed parse_bed(const std::string& text, Find find, const std::vector<uint64_t>& lengths, const std::vector<uint64_t>& offsets) {
  Bed bed;
  for (size_t at = 0; at < text.size();) {
    size_t nl = text.find('\n', at);
    if (nl == std::string::npos) nl = text.size();
    size_t end = nl;
    if (end > at && text[end - 1] == '\r') --end;
    const std::string line = text.substr(at, end - at);
    at = nl + 1;
    bool ok = line.find_first_not_of(" \t") != std::string::npos && line[0] != '#';
    if (ok) {
      const size_t sp = line.find_first_of(" \t");
      const std::string head = line.substr(0, sp);
      ok = head != "track" && head != "browser";
    }
    size_t t1 = std::string::npos, t2 = std::string::npos, t3 = std::string::npos, t4 = std::string::npos;
    if (ok) {
      t1 = line.find('\t');
      if (t1 != std::string::npos) t2 = line.find('\t', t1 + 1);
      ok = t2 != std::string::npos;
    }
    Interval v;
    if (ok) {
      t3 = line.find('\t', t2 + 1);
      if (t3 == std::string::npos) t3 = line.size();
      else { t4 = line.find('\t', t3 + 1); if (t4 == std::string::npos) t4 = line.size(); }
      ok = decimal(line, t1 + 1, t2, &v.start) && decimal(line, t2 + 1, t3, &v.end);
    }
    if (ok) {
      v.seq = find(line.substr(0, t1));
      ok = v.seq >= 0 && (size_t)v.seq < lengths.size() && v.start < v.end && v.end <= lengths[(size_t)v.seq];
    }
    if (!ok) { ++bed.skipped; continue; }
    v.name = t4 != std::string::npos && t4 > t3 + 1 ? line.substr(t3 + 1, t4 - t3 - 1) : std::string(".");
    v.order = (uint64_t)bed.iv.size();
    v.gstart = offsets[(size_t)v.seq] + v.start;
    v.gend = offsets[(size_t)v.seq] + v.end;
    bed.iv.push_back(std::move(v));
  }
  std::sort(bed.iv.begin(), bed.iv.end(), [](const Interval& a, const Interval& b) {
    if (a.gstart != b.gstart) return a.gstart < b.gstart;
    if (a.gend != b.gend) return a.gend < b.gend;
    return a.order < b.order;
  });
  return bed;
}

// what the parser made of a BED, as the test hook spells it
inline std::string bed_dump(const Bed& bed) {
  std::string out = "#skipped\t" + std::to_string(bed.skipped) + "\n";
  char num[200];
  for (const Interval& v : bed.iv) {
    out.append(num, (size_t)snprintf(num, sizeof num, "#iv\t%d\t%llu\t%llu\t", v.seq, (unsigned long long)v.start, (unsigned long long)v.end));
    out += v.name;
    out.append(num, (size_t)snprintf(num, sizeof num, "\t%llu\t%llu\t%llu\n", (unsigned long long)v.order, (unsigned long long)v.gstart, (unsigned long long)v.gend));
  }
  return out;
}

// a record as its PAF line has it: the query window [qs, qe), the strand, the target start
struct Record {
  std::string qname, tname;
  uint64_t qs = 0, qe = 0, ts = 0;
  bool rev = false;
};

// [t0, t1) of the text in query coordinates: on the reverse strand the text is the reverse complement of the query window
inline void query_range(const Record& r, uint32_t t0, uint32_t t1, uint64_t* a, uint64_t* b) {
  if (r.rev) { *a = r.qe - t1; *b = r.qe - t0; }
  else { *a = r.qs + t0; *b = r.qs + t1; }
}

// One line: qname qstart qend name strand tname tstart tend istart iend eq x ins del.  tstart / tend: the part lifted, in the target
// sequence's own coordinates; istart / iend: the input interval.
inline void lift_line(std::string& out, const Record& r, const Interval& v, uint32_t p0, uint32_t p1, uint32_t t0, uint32_t t1, uint32_t eq, uint32_t x) {
  uint64_t a, b;
  query_range(r, t0, t1, &a, &b);
  char num[200];
  out += r.qname;
  out.append(num, (size_t)snprintf(num, sizeof num, "\t%llu\t%llu\t", (unsigned long long)a, (unsigned long long)b));
  out += v.name;
  out += r.rev ? "\t-\t" : "\t+\t";
  out += r.tname;
  const uint64_t m = (uint64_t)eq + x;
  out.append(num, (size_t)snprintf(num, sizeof num, "\t%llu\t%llu\t%llu\t%llu\t%u\t%u\t%llu\t%llu\n", (unsigned long long)(r.ts + p0), (unsigned long long)(r.ts + p1),
                                   (unsigned long long)v.start, (unsigned long long)v.end, eq, x, (unsigned long long)((uint64_t)(t1 - t0) - m),
                                   (unsigned long long)((uint64_t)(p1 - p0) - m)));
}

}  // namespace lift
