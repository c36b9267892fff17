// cigar_ops.hpp -- the CIGAR surgery, the patch plan and the record writers of the align path (wflign_hip.cpp), on runs
// (count, op).  The reference compresses the aligner's op string at once (compress_cigar, wflign.cpp:183-208) and every later
// step reads runs out of the text again; here the device hands over runs (wfm_align_batch_rle) and the text is written once,
// at the end: each function is the reference's with "position in the text" read as "index of the run".  Nothing in here
// knows of a device, so scripts/micro/cigar_ops_check.cpp drives it under the sanitizers; tests/test_host_logic_cpu.py
// holds every function against oracle/wflign_host.py, tests/test_ref_wflign_gpu.py the whole pipeline against the
// reference's own wflign.cpp.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "../../include/wfmash_hip.h"

namespace wflign {

using CigarOps = std::vector<std::pair<int, char>>;

// ---- text <-> runs (behaviour of the lambdas at wflign.cpp:174-208) ----
inline CigarOps parse_cigar(const std::string& cigar) {
  CigarOps ops;
  ops.reserve(cigar.size() / 2 + 1);
  size_t i = 0;
  while (i < cigar.size()) {
    long long v = 0;
    while (i < cigar.size() && cigar[i] >= '0' && cigar[i] <= '9') { v = v * 10 + (cigar[i] - '0'); ++i; }
    if (i >= cigar.size()) break;
    ops.emplace_back((int)v, cigar[i++]);
  }
  return ops;
}

inline std::string cigar_to_string(const CigarOps& ops, size_t b, size_t e) {
  std::string s;
  for (size_t i = b; i < e; ++i) { s += std::to_string(ops[i].first); s += ops[i].second; }
  return s;
}
inline std::string cigar_to_string(const CigarOps& ops) { return cigar_to_string(ops, 0, ops.size()); }

// long-form op string {M,X,I,D} -> run-length CIGAR with M written as '='
// (wfa_edit_cigar_to_string, wflign_swizzle.cpp:359-382; compress_cigar, wflign.cpp:183-208)
inline std::string compress_ops(const char* ops, size_t n) {
  std::string out;
  size_t i = 0;
  while (i < n) {
    const char op = ops[i];
    size_t j = i;
    while (j < n && ops[j] == op) ++j;
    out += std::to_string(j - i);
    out += (op == 'M') ? '=' : op;
    i = j;
  }
  return out;
}

// wfm_align_batch_rle runs -> (count, op)
inline void ops_from_runs(const uint32_t* runs, size_t n, CigarOps& out) {
  static const char opc[4] = {'=', 'X', 'I', 'D'};  // M is written '=' (compress_cigar, wflign.cpp:201)
  out.clear();
  out.reserve(n + 8);
  for (size_t i = 0; i < n; ++i) out.emplace_back((int)WFM_RUN_LEN(runs[i]), opc[WFM_RUN_OP(runs[i])]);
}

// Neighbours with the same op become one run, over the whole CIGAR; drop_empty: runs of length 0 go first.
inline void compact(CigarOps& ops, bool drop_empty) {
  size_t o = 0;
  for (size_t i = 0; i < ops.size(); ++i) {
    if (drop_empty && ops[i].first <= 0) continue;
    if (o > 0 && ops[o - 1].second == ops[i].second) ops[o - 1].first += ops[i].first;
    else ops[o++] = ops[i];
  }
  ops.resize(o);
}
inline void merge_cigar_ops(CigarOps& ops) { compact(ops, false); }  // wflign_swizzle.cpp:7-37

// erode_short_matches_in_cigar (wflign.cpp:19-106); a CIGAR of three runs has at least six characters, so the reference's
// length test is implied by its run-count test
inline bool erode_short_matches_in_cigar(CigarOps& ops, int max_match_length, bool is_head_cigar) {
  if (ops.size() < 3) return false;
  size_t first = 1, last = ops.size() - 1;  // candidates are ops[first .. last)
  if (is_head_cigar) last = std::min(last, (size_t)3);
  else first = std::max(first, ops.size() - 3);
  bool modified = false;
  for (size_t i = first; i < last; ++i) {
    const char t = ops[i].second, a = ops[i - 1].second, b = ops[i + 1].second;
    const bool is_match = (t == 'M' || t == '=' || t == 'X');
    const bool opposite_indels = (a == 'I' && b == 'D') || (a == 'D' && b == 'I');
    if (is_match && ops[i].first <= max_match_length && opposite_indels &&
        ops[i - 1].first > ops[i].first && ops[i + 1].first > ops[i].first) {
      ops[i - 1].first += ops[i].first;
      ops[i + 1].first += ops[i].first;
      ops[i].first = 0;
      modified = true;
    }
  }
  if (modified) compact(ops, true);
  return modified;
}

// merge_adjacent_ops (wflign.cpp:211-238): src[from, to) behind dst, only the two runs that meet are fused
inline void merge_adjacent_ops(CigarOps& dst, const CigarOps& src, size_t from, size_t to) {
  if (from >= to) return;
  if (!dst.empty() && dst.back().second == src[from].second) { dst.back().first += src[from].first; ++from; }
  dst.insert(dst.end(), src.begin() + (long)from, src.begin() + (long)to);
}

// ---- erosion scans (wflign.cpp:241-276, 331-364) ----
constexpr uint64_t MIN_PATCH_LENGTH = 128;   // wflign.cpp:169
constexpr uint64_t MAX_ERODE_LENGTH = 4096;  // wflign.cpp:170
constexpr int MIN_CONSECUTIVE_MATCHES = 11;  // wflign.cpp:171

struct Erosion {
  uint64_t query_eroded = 0, target_eroded = 0;
  size_t erode_end_pos = 0;    // head: number of runs eroded
  size_t erode_start_idx = 0;  // tail: index of the first eroded run
};

// The stop rule of both scans (wflign.cpp:252-260, 340-348): the scan ends before a run once a long '=' run has been seen
// (this one counts) and both axes have MIN_PATCH_LENGTH, or once either axis has MAX_ERODE_LENGTH; else the run is eroded.
inline bool erode_run(Erosion& e, bool& found, const std::pair<int, char>& run) {
  const uint64_t count = (uint64_t)run.first;
  const char op = run.second;
  if (op == '=' && run.first >= MIN_CONSECUTIVE_MATCHES) found = true;
  if (found && e.query_eroded >= MIN_PATCH_LENGTH && e.target_eroded >= MIN_PATCH_LENGTH) return false;
  if (e.query_eroded >= MAX_ERODE_LENGTH || e.target_eroded >= MAX_ERODE_LENGTH) return false;
  if (op == 'M' || op == 'X' || op == '=') { e.query_eroded += count; e.target_eroded += count; }
  else if (op == 'I') e.query_eroded += count;
  else if (op == 'D') e.target_eroded += count;
  return true;
}

inline Erosion scan_head_erosion(const CigarOps& ops) {  // wflign.cpp:241-276
  Erosion e;
  bool found = false;
  for (size_t i = 0; i < ops.size() && erode_run(e, found, ops[i]); ++i) e.erode_end_pos = i + 1;
  return e;
}

// wflign.cpp:331-364; *looked_from: how far down the scan LOOKED (the run it stopped at is inspected, not eroded)
inline Erosion scan_tail_erosion(const CigarOps& ops, size_t* looked_from = nullptr) {
  Erosion e;
  e.erode_start_idx = ops.size();
  size_t looked = ops.size();
  bool found = false;
  for (size_t i = ops.size(); i-- > 0;) {
    looked = i;
    if (!erode_run(e, found, ops[i])) break;
    e.erode_start_idx = i;
  }
  if (looked_from) *looked_from = looked;
  return e;
}

// What do_biwfa_alignment does about a record's two ends, from its main CIGAR alone.  The reference patches the head, then
// scans the PATCHED CIGAR for the tail (wflign.cpp:323-364).  The tail scan walks up from the end and stops within 4096
// bases; the head patch replaces the runs before erode_end_pos and may change the count of the one run it meets.  So
// whenever the tail scan of the unpatched CIGAR never looked at a run the head patch can touch -- every record longer than a
// few kilobases -- both scans see what they would have seen in turn, and the two patches can be asked for in one go.
struct PatchPlan {
  Erosion head, tail;            // the scans of the unpatched CIGAR
  bool head_wanted = false;      // a patch is asked for when more than three bases of either axis were eroded
  bool tail_wanted = false;      // (of a tail that is not independent: of the unpatched CIGAR's, which is scanned again)
  bool tail_independent = true;  // of the head patch: there is none, or the tail scan stopped above every run it can touch
};
inline bool patch_wanted(const Erosion& e) { return e.query_eroded > 3 || e.target_eroded > 3; }
inline PatchPlan plan_patches(const CigarOps& ops) {
  PatchPlan p;
  size_t tail_looked_from = 0;
  p.head = scan_head_erosion(ops);
  p.tail = scan_tail_erosion(ops, &tail_looked_from);
  p.head_wanted = patch_wanted(p.head);
  p.tail_wanted = patch_wanted(p.tail);
  p.tail_independent = !p.head_wanted || tail_looked_from > p.head.erode_end_pos;
  return p;
}

// ---- swizzle (wflign_swizzle.cpp:217-299), query_start = target_start = 0 ----
inline bool sequences_match(const char* q, int64_t qn, const char* t, int64_t tn, int64_t qs, int64_t ts, int64_t n) {  // :39-59
  if (qs < 0 || ts < 0) return false;
  if (qs + n > qn || ts + n > tn) return false;
  return std::memcmp(q + qs, t + ts, (size_t)n) == 0;
}

inline bool try_swap_start_pattern(CigarOps& ops, const char* q, int64_t qn, const char* t, int64_t tn) {  // :217-252
  if (ops.size() < 2) return false;
  if (!(ops[0].second == '=' && ops[1].second == 'D')) return false;
  const int64_t n = ops[0].first, dlen = ops[1].first;
  if (!sequences_match(q, qn, t, tn, 0, dlen, n)) return false;
  std::swap(ops[0], ops[1]);
  merge_cigar_ops(ops);
  return true;
}

// :254-299: the swapped CIGAR is only kept when it verifies, and the verification accepts nothing but '=' and 'D' (:61-105)
inline bool try_swap_end_pattern(CigarOps& ops, const char* q, int64_t qn, const char* t, int64_t tn) {
  if (ops.size() < 2) return false;
  const std::pair<int, char> last = ops[ops.size() - 1], prev = ops[ops.size() - 2];
  if (!(prev.second == 'D' && last.second == '=')) return false;
  const int64_t n = last.first, dlen = prev.first;
  int64_t end_q = 0, end_t = 0;  // alignment_end_coords counts only '=' and 'D' (:192-215)
  bool only_eq_del = true;
  for (const auto& o : ops) {
    if (o.second == '=') { end_q += o.first; end_t += o.first; }
    else if (o.second == 'D') end_t += o.first;
    else only_eq_del = false;
  }
  if (!sequences_match(q, qn, t, tn, end_q - n, end_t - n - dlen, n)) return false;
  if (!only_eq_del) return false;  // verify_cigar_alignment would refuse it
  CigarOps sw(ops.begin(), ops.end() - 2);
  sw.emplace_back((int)n, '=');
  sw.emplace_back((int)dlen, 'D');
  merge_cigar_ops(sw);
  int64_t qp = 0, tp = 0;
  for (const auto& o : sw) {
    const int64_t v = o.first;
    if (o.second == '=') {
      if (qp + v > qn || tp + v > tn) return false;
      if (std::memcmp(q + qp, t + tp, (size_t)v) != 0) return false;
      qp += v; tp += v;
    } else {
      if (tp + v > tn) return false;
      tp += v;
    }
  }
  ops.swap(sw);
  return true;
}

// ---- records (wflign_patch.cpp:2480-2734) ----
inline double float2phred(double prob) {  // wflign_patch.cpp:2726-2734
  if (prob == 1) return 255;
  const double p = -10 * std::log10(prob);
  if (p < 0 || p > 255) return 255;
  return p;
}

struct PafParams {
  float min_identity = 0.0f;
  uint64_t min_alignment_length = 32;
  float min_block_identity = 0.1f;
};

struct CigarStats {
  uint64_t matches = 0, mismatches = 0, insertions = 0, inserted_bp = 0, deletions = 0, deleted_bp = 0,
           ref_len = 0, q_len = 0;
};
inline CigarStats cigar_stats(const CigarOps& ops, size_t b, size_t e) {  // process_compressed_cigar, wflign_patch.cpp:226-283
  CigarStats s;
  for (size_t i = b; i < e; ++i) {
    const uint64_t len = (uint64_t)ops[i].first;
    switch (ops[i].second) {
      case 'M': case '=': s.matches += len; s.ref_len += len; s.q_len += len; break;
      case 'X': s.mismatches += len; s.ref_len += len; s.q_len += len; break;
      case 'I': s.insertions++; s.inserted_bp += len; s.q_len += len; break;
      case 'D': s.deletions++; s.deleted_bp += len; s.ref_len += len; break;
      default: break;
    }
  }
  return s;
}

// What both writers do first: trim_indels (wflign_patch.cpp:139-223) strips the leading and trailing I and D runs and shifts
// the starts, the stats are taken of what is left, ops[b, e), and the three filters decide whether there is a record.
struct RecordCore {
  size_t b = 0, e = 0;
  uint64_t ref_start = 0, query_start = 0;
  CigarStats s;
  double gap_compressed_identity = 0, block_identity = 0;
};
inline bool trim_and_filter(const CigarOps& ops, uint64_t target_offset, uint64_t query_offset, const PafParams& pp, RecordCore& c) {
  c.b = 0; c.e = ops.size();
  c.ref_start = target_offset; c.query_start = query_offset;
  while (c.b < c.e && (ops[c.b].second == 'I' || ops[c.b].second == 'D')) {
    if (ops[c.b].second == 'I') c.query_start += (uint64_t)ops[c.b].first; else c.ref_start += (uint64_t)ops[c.b].first;
    ++c.b;
  }
  if (c.b < c.e) while (c.e > c.b && (ops[c.e - 1].second == 'I' || ops[c.e - 1].second == 'D')) --c.e;
  c.s = cigar_stats(ops, c.b, c.e);
  if (c.b >= c.e) return false;
  const CigarStats& s = c.s;
  c.gap_compressed_identity = (double)s.matches / (double)(s.matches + s.mismatches + s.insertions + s.deletions);
  c.block_identity = (double)s.matches / (double)(s.matches + s.mismatches + s.inserted_bp + s.deleted_bp);
  return c.gap_compressed_identity >= pp.min_identity && s.q_len >= pp.min_alignment_length && c.block_identity >= pp.min_block_identity;
}

inline char* put_u64(char* p, uint64_t v) {
  char tmp[24];
  int n = 0;
  do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
  while (n) *p++ = tmp[--n];
  return p;
}

// write_alignment_paf (wflign_patch.cpp:2611-2724), as the line the align driver finally writes: its processMappingRecord
// splits the writer's text at white space and joins the fields with single tabs (computeAlignments.hpp:484-525), so the
// fields go out tab-separated with a closing newline straight away.  Returns true and appends the line if the record passes
// the filters.  Numbers: the reference streams doubles with the default ostream format = printf's %g.
inline bool write_alignment_paf(std::string& out, const CigarOps& ops, const std::string& query_name, uint64_t query_total_length,
                                uint64_t query_offset, uint64_t query_length, bool query_is_rev, const std::string& target_name,
                                uint64_t target_total_length, uint64_t target_offset, const PafParams& pp,
                                float mashmap_estimated_identity, int32_t chain_id, int32_t chain_length, int32_t chain_pos) {
  RecordCore c;
  if (!trim_and_filter(ops, target_offset, query_offset, pp, c)) return false;
  const CigarStats& s = c.s;
  uint64_t q_start, q_end;
  if (query_is_rev) {
    q_start = query_offset + (query_length - (c.query_start - query_offset) - s.q_len);
    q_end = query_offset + (query_length - (c.query_start - query_offset));
  } else {
    q_start = c.query_start;
    q_end = c.query_start + s.q_len;
  }
  char num[512];
  int m = snprintf(num, sizeof num, "\t%llu\t%llu\t%llu\t%c\t", (unsigned long long)query_total_length, (unsigned long long)q_start,
                   (unsigned long long)q_end, query_is_rev ? '-' : '+');
  out.reserve(out.size() + query_name.size() + target_name.size() + 256 + (c.e - c.b) * 6);
  out += query_name;
  out.append(num, (size_t)m);
  out += target_name;
  m = snprintf(num, sizeof num, "\t%llu\t%llu\t%llu\t%llu\t%llu\t%g\tgi:f:%g\tbi:f:%g\tmd:f:%g\t", (unsigned long long)target_total_length,
               (unsigned long long)c.ref_start, (unsigned long long)(c.ref_start + s.ref_len), (unsigned long long)s.matches,
               (unsigned long long)std::max(s.ref_len, s.q_len), std::round(float2phred(1.0 - c.block_identity)),
               c.gap_compressed_identity, c.block_identity, (double)mashmap_estimated_identity);
  out.append(num, (size_t)m);
  if (chain_length > 0) {  // id.LENGTH.pos, wflign_patch.cpp:2708
    m = snprintf(num, sizeof num, "ch:Z:%d.%d.%d\t", chain_id, chain_length, chain_pos);
    out.append(num, (size_t)m);
  }
  out += "cg:Z:";
  char buf[4096];
  char* p = buf;
  for (size_t i = c.b; i < c.e; ++i) {
    p = put_u64(p, (uint64_t)(unsigned)ops[i].first);
    *p++ = ops[i].second;
    if (p > buf + sizeof buf - 32) { out.append(buf, (size_t)(p - buf)); p = buf; }
  }
  *p++ = '\n';
  out.append(buf, (size_t)(p - buf));
  return true;
}

// "MD:Z:..." of ops[b, e) (write_tag_and_md_string, wflign_patch.cpp:2397-2478): every op but the last is handled by the
// "previous op" branch, the last one by the closing branch.
inline std::string md_string(const CigarOps& all, size_t b, size_t e, int target_start, const char* target) {
  std::ostringstream os;
  os << "MD:Z:";
  CigarOps ops(all.begin() + (long)b, all.begin() + (long)e);
  merge_cigar_ops(ops);  // consecutive equal ops are summed by the reference's scanner
  int t_off = target_start, l_md = 0;
  for (size_t i = 0; i < ops.size(); ++i) {
    const int len = ops[i].first;
    const char op = ops[i].second;
    const bool last = (i + 1 == ops.size());
    if (!last) {
      if (op == '=' || op == 'M') { l_md += len; t_off += len; }
      else if (op == 'X') { for (int j = 0; j < len; ++j) { os << l_md << target[t_off + j]; l_md = 0; } t_off += len; }
      else if (op == 'D') { os << l_md << "^"; for (int j = 0; j < len; ++j) os << target[t_off + j]; l_md = 0; t_off += len; }
    } else if (len) {
      if (op == '=' || op == 'M') os << len + l_md;
      else if (op == 'X') { for (int j = 0; j < len; ++j) { os << l_md << target[t_off + j]; l_md = 0; } os << "0"; }
      else if (op == 'I') os << l_md;
      else if (op == 'D') { os << l_md << "^"; for (int j = 0; j < len; ++j) os << target[t_off + j]; os << "0"; }
    }
  }
  return os.str();
}

// SAM record (wflign_patch.cpp:2480-2609) incl. the MD:Z tag.  `query` / `target` are the strand-adjusted query window and
// the target window (target offset 0).
inline bool write_alignment_sam(std::string& out, const CigarOps& ops, const std::string& query_name, uint64_t query_offset,
                                bool query_is_rev, const std::string& target_name, uint64_t target_offset, const PafParams& pp,
                                float mashmap_estimated_identity, bool no_seq_in_sam, bool emit_md_tag, const char* query,
                                const char* target, int32_t chain_id, int32_t chain_length, int32_t chain_pos) {
  RecordCore c;
  if (!trim_and_filter(ops, target_offset, query_offset, pp, c)) return false;
  const CigarStats& s = c.s;
  std::ostringstream os;  // default iostream formatting = the reference's (6 significant digits)
  os << query_name << "\t" << (query_is_rev ? "16" : "0") << "\t" << target_name << "\t" << c.ref_start + 1 << "\t"
     << std::round(float2phred(1.0 - c.block_identity)) << "\t" << cigar_to_string(ops, c.b, c.e) << "\t" << "*\t0\t0\t";
  if (no_seq_in_sam) os << "*";
  else os.write(query + (c.query_start - query_offset), (std::streamsize)s.q_len);
  os << "\t*\t" << "NM:i:" << (s.mismatches + s.inserted_bp + s.deleted_bp) << "\t" << "gi:f:" << c.gap_compressed_identity << "\t"
     << "bi:f:" << c.block_identity << "\t" << "md:f:" << mashmap_estimated_identity;
  if (chain_length > 0) {
    os << "\tci:i:" << chain_id;
    os << "\tch:Z:" << chain_id << "." << chain_length << "." << chain_pos;
  }
  if (emit_md_tag) os << "\t" << md_string(ops, c.b, c.e, 0, target);  // target offset 0 + aln.i (= 0), wflign_patch.cpp:2602-2604
  os << "\n";
  out += os.str();
  return true;
}

}  // namespace wflign
