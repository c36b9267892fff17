// verify_parse.hpp -- an aligned PAF line as the verifier reads it (verify_paf.hpp).  Pure host code without dependencies, so that
// the parser can be built on its own (scripts/micro/verify_parse_check.cpp runs it under the address and undefined-behaviour sanitizers).
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace verify {

struct Line {
  std::string qname, tname;
  int64_t qlen = 0, qs = 0, qe = 0, tlen = 0, ts = 0, te = 0;
  bool rev = false;
  std::vector<uint32_t> runs;  // (length << 2) | op, as wfm_align_batch_rle
};
// LINE_UNVERIFIABLE: no cg:Z: tag, or an op outside =XID (a plain M does not say which bases agree) -- counted, not failed.
// LINE_MALFORMED: fewer than 12 fields, a coordinate that is no number or runs backwards, a count of 0 or of 2^30 and more.
enum { LINE_OK = 0, LINE_UNVERIFIABLE = 1, LINE_MALFORMED = 2 };

// a field of decimal digits as a number below 2^62; false for anything else (a sign, a blank, an empty field)
inline bool parse_number(const char* b, const char* e, int64_t* out) {
  if (b == e || e - b > 18) return false;
  int64_t v = 0;
  for (const char* c = b; c < e; ++c) {
    if (*c < '0' || *c > '9') return false;
    v = v * 10 + (*c - '0');
  }
  *out = v;
  return true;
}

inline int parse_line(const std::string& line, Line& out, std::string* why) {
  auto fail = [&](int code, const char* what) { if (why) *why = what; return code; };
  std::vector<std::pair<const char*, const char*>> f;
  const char* b = line.data();
  const char* const end = b + line.size();
  for (const char* c = b;; ++c)
    if (c == end || *c == '\t') { f.emplace_back(b, c); b = c + 1; if (c == end) break; }
  if (f.size() < 12) return fail(LINE_MALFORMED, "fewer than 12 fields");
  out = Line();
  out.qname.assign(f[0].first, f[0].second);
  out.tname.assign(f[5].first, f[5].second);
  if (f[4].second - f[4].first != 1 || (*f[4].first != '+' && *f[4].first != '-')) return fail(LINE_MALFORMED, "strand is neither + nor -");
  out.rev = *f[4].first == '-';
  // the coordinates as they are written: no padding, no clamping
  if (!parse_number(f[1].first, f[1].second, &out.qlen) || !parse_number(f[2].first, f[2].second, &out.qs) || !parse_number(f[3].first, f[3].second, &out.qe) ||
      !parse_number(f[6].first, f[6].second, &out.tlen) || !parse_number(f[7].first, f[7].second, &out.ts) || !parse_number(f[8].first, f[8].second, &out.te))
    return fail(LINE_MALFORMED, "a coordinate is not a number");
  if (out.qs > out.qe || out.ts > out.te || out.qe > out.qlen || out.te > out.tlen) return fail(LINE_MALFORMED, "coordinates run backwards or past the sequence's length");
  const char* cg = nullptr;
  const char* cg_end = nullptr;
  for (size_t i = 12; i < f.size(); ++i)
    if (f[i].second - f[i].first >= 5 && memcmp(f[i].first, "cg:Z:", 5) == 0) { cg = f[i].first + 5; cg_end = f[i].second; break; }
  if (!cg) return fail(LINE_UNVERIFIABLE, "no cg:Z: tag");
  // an op outside =XID makes the line unverifiable whatever else is wrong with it: look for one first
  for (const char* c = cg; c < cg_end; ++c)
    if ((*c < '0' || *c > '9') && *c != '=' && *c != 'X' && *c != 'I' && *c != 'D') return fail(LINE_UNVERIFIABLE, "an op outside =XID");
  for (const char* c = cg; c < cg_end;) {
    const char* d = c;
    while (d < cg_end && *d >= '0' && *d <= '9') ++d;
    int64_t count = 0;
    if (d == cg_end) return fail(LINE_MALFORMED, "a count without an op");
    if (d == c) return fail(LINE_MALFORMED, "an op without a count");
    if (!parse_number(c, d, &count) || count >= ((int64_t)1 << 30)) return fail(LINE_MALFORMED, "a count of 2^30 or more");
    if (count == 0) return fail(LINE_MALFORMED, "a count of 0");
    const uint32_t op = *d == '=' ? 0u : *d == 'X' ? 1u : *d == 'I' ? 2u : 3u;
    out.runs.push_back(((uint32_t)count << 2) | op);
    c = d + 1;
  }
  return LINE_OK;
}

}  // namespace verify
