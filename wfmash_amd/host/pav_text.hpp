// pav_text.hpp -- the text side of --pav: a query name's group key, the columns of the table, the windows of --pav-window and the file's
// header and rows.  Pure host code on the standard library alone (and lift_text.hpp, which is), so that it can be built on its own
// (scripts/micro/pav_check.cpp runs it under the address and undefined-behaviour sanitizers).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "lift_text.hpp"

namespace pav {

constexpr char DELIM = '#';  // the PanSN delimiter, -Y's default

// the part before the LAST delimiter, else the whole name: sequence_ids.hpp's rule without user prefixes ('\0': no delimiter)
inline std::string group_key(const std::string& name, char delim = DELIM) {
  if (delim == '\0') return name;
  const size_t at = name.rfind(delim);
  return at == std::string::npos ? name : name.substr(0, at);
}

// the distinct keys of ALL the names, sorted bytewise, and every name's column
struct Columns {
  std::vector<std::string> keys;
  std::vector<uint32_t> of_seq;
};

inline Columns columns(const std::vector<std::string>& names, char delim = DELIM) {
  Columns c;
  std::vector<std::string> key(names.size());
  for (size_t i = 0; i < names.size(); ++i) key[i] = group_key(names[i], delim);
  c.keys = key;
  std::sort(c.keys.begin(), c.keys.end(), [](const std::string& a, const std::string& b) {
    return std::lexicographical_compare(a.begin(), a.end(), b.begin(), b.end(), [](char x, char y) { return (unsigned char)x < (unsigned char)y; });
  });
  c.keys.erase(std::unique(c.keys.begin(), c.keys.end()), c.keys.end());
  c.of_seq.resize(names.size());
  for (size_t i = 0; i < names.size(); ++i)
    c.of_seq[i] = (uint32_t)(std::lower_bound(c.keys.begin(), c.keys.end(), key[i], [](const std::string& a, const std::string& b) {
                               return std::lexicographical_compare(a.begin(), a.end(), b.begin(), b.end(), [](char x, char y) { return (unsigned char)x < (unsigned char)y; });
                             }) - c.keys.begin());
  return c;
}

// --pav-window: windows of `size` bases tiling every sequence in index order, the last one shorter, named "."; a sequence of length 0 has
// none.  size >= 1.  lengths: the target's sequences; offsets: where each begins in their concatenation.
inline std::vector<lift::Interval> windows(const std::vector<uint64_t>& lengths, const std::vector<uint64_t>& offsets, uint64_t size) {
  std::vector<lift::Interval> out;
  if (size == 0) return out;
  for (size_t c = 0; c < lengths.size(); ++c)
    for (uint64_t a = 0; a < lengths[c];) {
      const uint64_t b = lengths[c] - a > size ? a + size : lengths[c];
      lift::Interval v;
      v.seq = (int)c; v.start = a; v.end = b; v.name = "."; v.order = (uint64_t)out.size();
      v.gstart = offsets[c] + a; v.gend = offsets[c] + b;
      out.push_back(std::move(v));
      a = b;
    }
  return out;
}

// "#tname tstart tend name len" and the group keys, tab-separated
inline std::string header(const std::vector<std::string>& keys) {
  std::string out = "#tname\ttstart\ttend\tname\tlen";
  for (const std::string& k : keys) { out += '\t'; out += k; }
  out += '\n';
  return out;
}

// one row: the interval, then the covered bases of each of the n_groups groups
inline void row(std::string& out, const std::string& tname, const lift::Interval& v, const uint32_t* cells, size_t n_groups) {
  char num[100];
  out += tname;
  out.append(num, (size_t)snprintf(num, sizeof num, "\t%llu\t%llu\t", (unsigned long long)v.start, (unsigned long long)v.end));
  out += v.name;
  out.append(num, (size_t)snprintf(num, sizeof num, "\t%llu", (unsigned long long)(v.end - v.start)));
  for (size_t g = 0; g < n_groups; ++g) out.append(num, (size_t)snprintf(num, sizeof num, "\t%u", cells[g]));
  out += '\n';
}

// The file of --pav: the header, then one row per interval in the order given; cells: n_iv x n_groups, row-major, as wfm_pav_matrix fills
// them; tnames: the target's sequences.  The text goes to `out` (anything that takes << of a string) a MiB at a time.
template <class Sink>
inline void table(Sink& out, const std::vector<std::string>& keys, const std::vector<std::string>& tnames, const std::vector<lift::Interval>& iv,
                  const uint32_t* cells) {
  const size_t G = keys.size();
  std::string text = header(keys);
  for (size_t j = 0; j < iv.size(); ++j) {
    row(text, tnames[(size_t)iv[j].seq], iv[j], cells + j * G, G);
    if (text.size() >= ((size_t)1 << 20)) { out << text; text.clear(); }
  }
  out << text;
}

}  // namespace pav
