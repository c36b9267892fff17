// verify_paf.cpp -- the PAF line verifier behind --verify and --verify-paf (verify_paf.hpp; C entry points at the end).
#include "verify_paf.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <mutex>
#include <stdexcept>
#include <thread>

#include "../../include/wfmash_host.h"
#include "../csrc/wfa_handle.h"
#include "aligner.hpp"
#include "coverage_text.hpp"
#include "lift_text.hpp"
#include "transitive_text.hpp"
#include "chain_text.hpp"
#include "maf_text.hpp"
#include "pav_text.hpp"
#include "parallel.hpp"
#include "wflign_hip.hpp"

namespace verify {

namespace {

std::atomic<bool> g_enabled{false};
std::atomic<uint64_t> g_counts[4];

const char* const FLAG_NAMES[7] = {"NOT_CHECKED", "BAD_RUN", "SPANS", "M_DIFFERS", "X_EQUAL", "SCORE", "COUNTS"};
std::string flag_names(uint32_t f) {
  std::string s;
  for (int b = 0; b < 7; ++b)
    if (f & (1u << b)) { if (!s.empty()) s += '|'; s += FLAG_NAMES[b]; }
  return s;
}

// one line of stderr per failed record (several workers verify at once)
std::mutex g_report_mu;
void report(const Line& l, const std::string& what, const std::string& where) {
  std::lock_guard<std::mutex> lk(g_report_mu);
  std::cerr << "[wfmash::verify] FAILED " << l.qname << ' ' << l.qs << '-' << l.qe << ' ' << (l.rev ? '-' : '+') << ' ' << l.tname << ' ' << l.ts << '-' << l.te
            << ": " << what << where << std::endl;
}

constexpr int64_t MAX_PROBLEM_BASES = (int64_t)1 << 29;   // wfm_upload_sequence_refs' limit of plen + tlen
constexpr int64_t BATCH_BASES = (int64_t)256 << 20;       // bases one device call holds
constexpr size_t BATCH_LINES = 8192;

// The lines in hand as problems by reference -- pattern = target [ts, te), text = query [qs, qe), reverse-complemented for '-' -- with their
// runs: by id where the source has a store, else by host pointer, fetched and normalised as the align driver's windows are, on the caller's
// threads.  What verify_batch and maf_batch upload.
struct LineProblems {
  std::vector<wfm_problem_ref_t> refs;
  std::vector<wfm_result_t> res;
  std::vector<std::string> pat, txt;  // the host-pointer sides, normalised
  std::vector<uint32_t> runs;
};
void line_problems(const Source& src, const std::vector<Line>& lines, LineProblems& lp, const char* tag) {
  const size_t n = lines.size();
  std::vector<wfm_problem_ref_t>& refs = lp.refs;
  std::vector<wfm_result_t>& res = lp.res;
  std::vector<std::string>&pat = lp.pat, &txt = lp.txt;
  std::vector<uint32_t>& runs = lp.runs;
  refs.assign(n, wfm_problem_ref_t{});
  res.assign(n, wfm_result_t{});
  pat.assign(n, std::string());
  txt.assign(n, std::string());
  runs.clear();
  for (size_t i = 0; i < n; ++i) {
    const Line& l = lines[i];
    wfm_problem_ref_t& r = refs[i];
    memset(&r, 0, sizeof(r));
    r.plen = (int32_t)(l.te - l.ts); r.tlen = (int32_t)(l.qe - l.qs);
    r.mode = WFM_MODE_END2END_UNI;  // (no reversed copies are made for it)
    r.pattern_seq = r.text_seq = -1;
    const int ti = src.target->find(l.tname), qi = src.query->find(l.qname);
    if (src.store && src.resident_id) {
      if (r.plen) r.pattern_seq = src.resident_id(src.target, ti);
      if (r.tlen) r.text_seq = src.resident_id(src.query, qi);
    }
    if (r.pattern_seq >= 0) r.pattern_off = l.ts;
    if (r.text_seq >= 0) { r.text_off = l.qs; r.text_revcomp = l.rev ? 1 : 0; }
    wfm_result_t& q = res[i];
    memset(&q, 0, sizeof(q));
    q.status = 0; q.score = -1;  // the price is not compared: a PAF line carries none
    q.ops_off = runs.size(); q.n_runs = (uint32_t)l.runs.size();
    uint64_t ops = 0;
    for (uint32_t w : l.runs) ops += WFM_RUN_LEN(w);
    q.ops_len = (uint32_t)std::min<uint64_t>(ops, 0xffffffffu);
    runs.insert(runs.end(), l.runs.begin(), l.runs.end());
  }
  std::atomic<bool> fetch_failed{false};
  wfmash_host::parallel_for(n, std::max(1, src.threads), [&](size_t i) {
    const Line& l = lines[i];
    wfm_problem_ref_t& r = refs[i];
    try {
      if (r.pattern_seq < 0 && r.plen) {
        pat[i] = src.target->fetch(l.tname, l.ts, l.te - 1);
        align::upper_valid_dna(pat[i]);
        r.pattern = pat[i].data();
      }
      if (r.text_seq < 0 && r.tlen) {
        txt[i] = src.query->fetch(l.qname, l.qs, l.qe - 1);
        align::upper_valid_dna(txt[i]);
        if (l.rev) txt[i] = align::revcomp(txt[i]);
        r.text = txt[i].data();
      }
      if ((r.pattern_seq < 0 && (int64_t)pat[i].size() != r.plen) || (r.text_seq < 0 && (int64_t)txt[i].size() != r.tlen)) fetch_failed.store(true);
    } catch (const std::exception&) {
      fetch_failed.store(true);
    }
  });
  if (fetch_failed.load()) throw std::runtime_error(std::string("[wfmash::") + tag + "] cannot fetch the bases of a line's windows");
}

// the lines in hand on the device: upload by reference, check, report
void verify_batch(wfm_handle_t* h, const Source& src, std::vector<Line>& lines, Counts& c) {
  if (lines.empty()) return;
  const size_t n = lines.size();
  LineProblems lp;
  line_problems(src, lines, lp, "verify");
  std::vector<wfm_problem_ref_t>& refs = lp.refs;
  std::vector<wfm_result_t>& res = lp.res;
  std::vector<uint32_t>& runs = lp.runs;
  const wfm_penalties_t pen{5, 8, 2, 24, 1};  // (prices nothing that is compared)
  std::vector<wfm_check_t> out(n);
  {
    std::lock_guard<std::mutex> lk(wflign::handle_lock(h));
    wfm_seqset_t* S = nullptr;
    int rc = wfm_upload_sequence_refs(h, src.store, refs.data(), n, &S);
    if (rc == WFM_OK) {
      rc = wfm_check_runs(h, &pen, S, res.data(), runs.data(), runs.size(), out.data());
      wfm_free_sequences(h, S);
    }
    if (rc < 0) throw std::runtime_error(std::string("[wfmash::verify] device check failed: ") + wfm_last_error(h));
  }
  for (size_t i = 0; i < n; ++i) {
    const Line& l = lines[i];
    const wfm_check_t& k = out[i];
    c.checked++;
    c.bases += (uint64_t)k.matches + k.mismatches;
    if (!(k.flags & ~WFM_CK_NOT_CHECKED)) continue;
    c.failed++;
    std::string where;
    if (k.bad_p >= 0) {
      const int64_t qpos = l.rev ? l.qe - 1 - k.bad_t : l.qs + k.bad_t;
      where = "; first offending base: query " + std::to_string(qpos) + ", target " + std::to_string(l.ts + k.bad_p) + ", CIGAR run " + std::to_string(k.bad_run);
    } else if (k.flags & WFM_CK_BAD_RUN) where = "; first bad CIGAR run " + std::to_string(k.bad_run);
    report(l, flag_names(k.flags), where);
  }
  lines.clear();
}

}  // namespace

void verify_text(wfm_handle_t* h, const Source& src, const std::string& text, Counts& c) {
  std::vector<Line> batch;
  int64_t bases = 0;
  size_t at = 0;
  while (at < text.size()) {
    size_t nl = text.find('\n', at);
    if (nl == std::string::npos) nl = text.size();
    const std::string line = text.substr(at, nl - at);
    at = nl + 1;
    if (line.empty() || line[0] == '@') continue;
    Line l;
    std::string why;
    const int st = parse_line(line, l, &why);
    if (st == LINE_UNVERIFIABLE) { c.unverifiable++; continue; }
    if (st == LINE_MALFORMED) {
      c.checked++; c.failed++;
      std::lock_guard<std::mutex> lk(g_report_mu);
      std::cerr << "[wfmash::verify] FAILED line: " << why << ": " << line.substr(0, 120) << std::endl;
      continue;
    }
    // the sequences the line names, as the files have them
    const int64_t tl = src.target->seq_len(l.tname), ql = src.query->seq_len(l.qname);
    if (tl < 0 || ql < 0) { c.checked++; c.failed++; report(l, "UNKNOWN_SEQUENCE", ""); continue; }
    if (l.te > tl || l.qe > ql) { c.checked++; c.failed++; report(l, "COORDINATES", "; the window leaves its sequence"); continue; }
    if ((l.te - l.ts) + (l.qe - l.qs) > MAX_PROBLEM_BASES) { c.unverifiable++; continue; }
    bases += (l.te - l.ts) + (l.qe - l.qs);
    batch.push_back(std::move(l));
    if (batch.size() >= BATCH_LINES || bases >= BATCH_BASES) { verify_batch(h, src, batch, c); bases = 0; }
  }
  verify_batch(h, src, batch, c);
}

// ---- --maf-paf: the lines in hand on the device: upload by reference, ONE wfm_maf_rows call, the blocks' text through maf_text.hpp ----
namespace {
void maf_batch(wfm_handle_t* h, const Source& src, std::vector<Line>& lines, uint32_t split, std::ostream& out, uint64_t counts[4]) {
  if (lines.empty()) return;
  const size_t n = lines.size();
  LineProblems lp;
  line_problems(src, lines, lp, "maf");
  std::vector<wfm_mafcall_t> per(n);
  wfm_maf_block_t* blocks = nullptr;
  char* rows = nullptr;
  size_t n_blocks = 0, bytes = 0;
  {
    std::lock_guard<std::mutex> lk(wflign::handle_lock(h));
    wfm_seqset_t* S = nullptr;
    int rc = wfm_upload_sequence_refs(h, src.store, lp.refs.data(), n, &S);
    if (rc == WFM_OK) {
      rc = wfm_maf_rows(h, S, lp.res.data(), lp.runs.data(), lp.runs.size(), split, &blocks, &n_blocks, &rows, &bytes, per.data());
      wfm_free_sequences(h, S);
    }
    if (rc < 0) throw std::runtime_error(std::string("[wfmash::maf] device call failed: ") + wfm_last_error(h));
  }
  static_assert(sizeof(maf::Block) == sizeof(wfm_maf_block_t), "maf_text.hpp restates wfm_maf_block_t");
  std::string text;
  for (size_t i = 0; i < n; ++i) {
    const Line& l = lines[i];
    if (per[i].flags || per[i].count == 0) { counts[3]++; continue; }
    const maf::Line line{&l.tname, (uint64_t)l.ts, (uint64_t)l.tlen, &l.qname, (uint64_t)l.qs, (uint64_t)l.qe, (uint64_t)l.qlen, l.rev};
    const maf::Block* mine = reinterpret_cast<const maf::Block*>(blocks) + per[i].first;
    text.clear();
    text.reserve(maf::record_bytes(line, mine, (size_t)per[i].count));
    for (uint64_t k = 0; k < per[i].count; ++k) {
      maf::block(text, line, mine[k], rows);
      counts[2] += mine[k].cols;
    }
    out << text;
    counts[0]++; counts[1] += per[i].count;
  }
  wfm_free_maf(blocks, rows);
  lines.clear();
}
}  // namespace

void maf_text(wfm_handle_t* h, const Source& src, const std::string& text, uint32_t split, std::ostream& out, uint64_t counts[4], uint64_t skipped[4]) {
  std::vector<Line> batch;
  int64_t bases = 0;
  size_t at = 0;
  while (at < text.size()) {
    size_t nl = text.find('\n', at);
    if (nl == std::string::npos) nl = text.size();
    const std::string line = text.substr(at, nl - at);
    at = nl + 1;
    if (line.empty() || line[0] == '@') continue;
    Line l;
    const int st = parse_line(line, l, nullptr);
    if (st == LINE_UNVERIFIABLE) { skipped[0]++; continue; }
    if (st == LINE_MALFORMED) { skipped[1]++; continue; }
    // the sequences the line names, as the files have them
    const int64_t tl = src.target->seq_len(l.tname), ql = src.query->seq_len(l.qname);
    if (tl < 0 || ql < 0) { skipped[2]++; continue; }
    if (l.tlen != tl || l.qlen != ql || l.te > tl || l.qe > ql) { skipped[3]++; continue; }
    if ((l.te - l.ts) + (l.qe - l.qs) > MAX_PROBLEM_BASES) { skipped[1]++; continue; }
    bases += (l.te - l.ts) + (l.qe - l.qs);
    batch.push_back(std::move(l));
    if (batch.size() >= BATCH_LINES || bases >= BATCH_BASES) { maf_batch(h, src, batch, split, out, counts); bases = 0; }
  }
  maf_batch(h, src, batch, split, out, counts);
}

void set_enabled(bool on) {
  g_enabled.store(on);
  for (auto& a : g_counts) a.store(0);
}
bool enabled() { return g_enabled.load(); }
void add_counts(const Counts& c) {
  g_counts[0] += c.checked; g_counts[1] += c.failed; g_counts[2] += c.unverifiable; g_counts[3] += c.bases;
}
Counts total_counts() {
  Counts c;
  c.checked = g_counts[0].load(); c.failed = g_counts[1].load(); c.unverifiable = g_counts[2].load(); c.bases = g_counts[3].load();
  return c;
}

}  // namespace verify

namespace {
// What --coverage-paf, --lift-paf and --pav-paf share: the target's offsets in the concatenation, the lines of an aligned PAF read and
// skipped by one rule (coverage::classify_line), their runs gathered into batches of 65536 problems or 16 Mi runs, and device calls
// that throw.  An entry point supplies what it keeps per line and what a batch is flushed into.
struct PafRuns {
  wfm_handle_t* h;
  const char* tag;                      // "coverage", "lift", "pav": the [wfmash::...] of the texts
  const wfmash_host::FastaStore& target;
  std::vector<std::string> names;
  std::vector<uint64_t> lengths, offsets;
  uint64_t skipped[5] = {0, 0, 0, 0, 0};  // by coverage::LINE_*
  std::vector<wfm_cov_prob_t> probs;    // the batch at hand: base, runs_off, n_runs of every line
  std::vector<uint32_t> runs;

  PafRuns(wfm_handle_t* h_, const char* tag_, const wfmash_host::FastaStore& target_) : h(h_), tag(tag_), target(target_), offsets(1, 0) {
    for (int i = 0; i < target.nseq(); ++i) {
      names.push_back(target.name(i));
      lengths.push_back((uint64_t)target.length(i));
      offsets.push_back(offsets.back() + lengths.back());
    }
  }
  int device(int rc, const char* what) const {
    if (rc < 0) throw std::runtime_error(std::string("[wfmash::") + tag + "] " + what + " failed: " + wfm_last_error(h));
    return rc;
  }
  void refused(uint64_t n) { skipped[coverage::LINE_MALFORMED] += n; }  // (a span that leaves the target: classify_line lets none through)
  uint64_t all_skipped() const { return skipped[1] + skipped[2] + skipped[3] + skipped[4]; }
  // "N skipped (... without an =XID cg:Z:, ... malformed, ...)" of the summaries; no_query: the lines the caller left out for their query
  std::string skipped_clause(const char* noun = "", const uint64_t* no_query = nullptr) const {
    std::string s = std::to_string(all_skipped() + (no_query ? *no_query : 0)) + " " + noun + "skipped (" + std::to_string(skipped[1]) + " without an =XID cg:Z:, " +
                    std::to_string(skipped[2]) + " malformed, " + std::to_string(skipped[3]) + " with an unknown target, " + std::to_string(skipped[4]) + " with another tlen";
    if (no_query) s += ", " + std::to_string(*no_query) + " with an unknown query";
    return s + ")";
  }
  // extra(line) -> false: the line is not taken (the caller counts it); flush(): the batch to the device, whatever extra kept given back
  template <class Extra, class Flush>
  void read(std::istream& in, Extra extra, Flush flush) {
    auto flush_batch = [&]() {
      if (probs.empty()) return;
      flush();
      probs.clear(); runs.clear();
    };
    std::string line;
    verify::Line l;
    while (std::getline(in, line)) {
      if (line.empty() || line[0] == '@') continue;
      int ti = -1;
      const int code = coverage::classify_line(line, [&](const std::string& name) { return target.find(name); }, lengths, l, &ti);
      if (code != coverage::LINE_ADD) { skipped[code]++; continue; }
      if (!extra(l)) continue;
      probs.push_back(wfm_cov_prob_t{offsets[(size_t)ti] + (uint64_t)l.ts, (uint64_t)runs.size(), (uint32_t)l.runs.size(), 0u});
      runs.insert(runs.end(), l.runs.begin(), l.runs.end());
      if (probs.size() >= 65536 || runs.size() >= ((size_t)16 << 20)) flush_batch();
    }
    flush_batch();
  }
};
}  // namespace

extern "C" {

void wfmh_set_verify(int on) { verify::set_enabled(on != 0); }

int wfmh_verify_counts(uint64_t out[4]) {
  if (!out) return WFM_E_ARG;
  const verify::Counts c = verify::total_counts();
  out[0] = c.checked; out[1] = c.failed; out[2] = c.unverifiable; out[3] = c.bases;
  return WFM_OK;
}

int wfmh_verify_paf(wfm_handle_t* h, const char* target_fasta, const char* query_fasta, const char* aligned_paf, uint64_t out[4]) {
  if (!h || !target_fasta || !aligned_paf) return WFM_E_ARG;
  try {
    std::shared_ptr<wfmash_host::FastaStore> target = wfmash_host::open_shared(target_fasta), query_own;
    const std::string qpath = query_fasta ? query_fasta : target_fasta;
    if (qpath != target_fasta) query_own = wfmash_host::open_shared(qpath);
    verify::Source src;
    src.target = target.get();
    src.query = query_own ? query_own.get() : target.get();
    src.threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    std::ifstream in(aligned_paf);
    if (!in.is_open()) throw std::runtime_error(std::string("[wfmash::verify] cannot open ") + aligned_paf);
    verify::Counts c;
    std::string text, line;
    while (std::getline(in, line)) {
      text += line; text += '\n';
      if (text.size() >= ((size_t)64 << 20)) { verify::verify_text(h, src, text, c); text.clear(); }
    }
    verify::verify_text(h, src, text, c);
    if (out) { out[0] = c.checked; out[1] = c.failed; out[2] = c.unverifiable; out[3] = c.bases; }
    return WFM_OK;
  } catch (const std::exception& e) {
    std::cerr << e.what() << std::endl;
    wfm_set_error(h, e.what());
    return WFM_E_ARG;
  }
}

// --maf-paf: the MAF file of an existing aligned PAF, lines parsed as --verify-paf parses them and their windows uploaded as it uploads
// them; a line whose target the target file does not have, or whose query the query file does not (wfmh_verify_paf's lookup),
// or that names another length, is skipped and counted.  Nothing else runs.
int wfmh_maf_paf(wfm_handle_t* h, const char* target_fasta, const char* query_fasta, const char* aligned_paf, const char* out_path, uint32_t split,
                 uint64_t out[4]) {
  if (!h || !target_fasta || !aligned_paf || !out_path) return WFM_E_ARG;
  try {
    std::shared_ptr<wfmash_host::FastaStore> target = wfmash_host::open_shared(target_fasta), query_own;
    const std::string qpath = query_fasta ? query_fasta : target_fasta;
    if (qpath != target_fasta) query_own = wfmash_host::open_shared(qpath);
    verify::Source src;
    src.target = target.get();
    src.query = query_own ? query_own.get() : target.get();
    src.threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    std::ifstream in(aligned_paf);
    if (!in.is_open()) throw std::runtime_error(std::string("[wfmash::maf] cannot open ") + aligned_paf);
    std::ofstream outstream(out_path);
    if (!outstream.is_open()) throw std::runtime_error(std::string("[wfmash::maf] cannot open ") + out_path);
    outstream << maf::header();
    uint64_t counts[4] = {0, 0, 0, 0}, skipped[4] = {0, 0, 0, 0};
    std::string text, line;
    while (std::getline(in, line)) {
      text += line; text += '\n';
      if (text.size() >= ((size_t)64 << 20)) { verify::maf_text(h, src, text, split, outstream, counts, skipped); text.clear(); }
    }
    verify::maf_text(h, src, text, split, outstream, counts, skipped);
    std::cerr << "[wfmash::maf] " << counts[0] << " records, " << counts[1] << " blocks, " << counts[2] << " columns, " << counts[3] << " records left without blocks, "
              << (skipped[0] + skipped[1] + skipped[2] + skipped[3]) << " lines skipped (" << skipped[0] << " without an =XID cg:Z:, " << skipped[1] << " malformed, "
              << skipped[2] << " with an unknown sequence, " << skipped[3] << " with another length)" << std::endl;
    if (out) for (int q = 0; q < 4; ++q) out[q] = counts[q];
    return WFM_OK;
  } catch (const std::exception& e) {
    std::cerr << e.what() << std::endl;
    wfm_set_error(h, e.what());
    return WFM_E_ARG;
  }
}

// --coverage-paf: the depth of an existing aligned PAF.  Lines go to the device in batches of runs; nothing else runs.
int wfmh_coverage_paf(wfm_handle_t* h, const char* target_fasta, const char* aligned_paf, const char* out_path, uint64_t out[4]) {
  if (!h || !target_fasta || !aligned_paf || !out_path) return WFM_E_ARG;
  wfm_coverage_t* cov = nullptr;
  try {
    std::shared_ptr<wfmash_host::FastaStore> target = wfmash_host::open_shared(target_fasta);
    std::ifstream in(aligned_paf);
    if (!in.is_open()) throw std::runtime_error(std::string("[wfmash::coverage] cannot open ") + aligned_paf);
    std::ofstream outstream(out_path);
    if (!outstream.is_open()) throw std::runtime_error(std::string("[wfmash::coverage] cannot open ") + out_path);
    PafRuns pr(h, "coverage", *target);
    std::lock_guard<std::mutex> lk(wflign::handle_lock(h));
    pr.device(wfm_coverage_create(h, pr.offsets.back(), &cov), "create");
    uint64_t added = 0;
    std::vector<uint32_t> flags;
    pr.read(in, [](const verify::Line&) { return true; }, [&]() {
      flags.resize(pr.probs.size());
      const int refused = pr.device(wfm_coverage_add(h, cov, pr.probs.data(), pr.probs.size(), pr.runs.data(), pr.runs.size(), flags.data()), "add");
      added += pr.probs.size() - (uint64_t)refused;
      pr.refused((uint64_t)refused);
    });
    wfm_cov_interval_t* d_iv = nullptr;
    size_t n = 0;
    uint64_t totals[3] = {0, 0, 0};
    pr.device(wfm_coverage_intervals(h, cov, &d_iv, &n, totals), "intervals");
    wfm_coverage_free(cov);
    cov = nullptr;
    uint64_t lines = 0;
    outstream << coverage::coverage_bedgraph(pr.names, pr.lengths, d_iv, n, &lines);
    wfm_coverage_free_list(d_iv);
    std::cerr << "[wfmash::coverage] " << added << " lines added, " << pr.skipped_clause() << ", " << totals[0] << " bases covered, sum of depth " << totals[1]
              << ", max depth " << totals[2] << ", " << lines << " intervals" << std::endl;
    if (out) { out[0] = added; out[1] = pr.all_skipped(); out[2] = totals[0]; out[3] = totals[1]; }
    return WFM_OK;
  } catch (const std::exception& e) {
    if (cov) wfm_coverage_free(cov);
    std::cerr << e.what() << std::endl;
    wfm_set_error(h, e.what());
    return WFM_E_ARG;
  }
}

// --lift-paf: the BED intervals lifted through an existing aligned PAF.  Lines go to the device in batches of runs, read and skipped by
// wfmh_coverage_paf's rules (coverage::classify_line); nothing else runs.
int wfmh_lift_paf(wfm_handle_t* h, const char* target_fasta, const char* aligned_paf, const char* bed_path, const char* out_path, uint64_t out[4]) {
  if (!h || !target_fasta || !aligned_paf || !bed_path || !out_path) return WFM_E_ARG;
  wfm_liftset_t* set = nullptr;
  try {
    std::shared_ptr<wfmash_host::FastaStore> target = wfmash_host::open_shared(target_fasta);
    std::ifstream in(aligned_paf);
    if (!in.is_open()) throw std::runtime_error(std::string("[wfmash::lift] cannot open ") + aligned_paf);
    std::ifstream bedstream(bed_path, std::ios::binary);
    if (!bedstream.is_open()) throw std::runtime_error(std::string("[wfmash::lift] cannot open ") + bed_path);
    const std::string bed_text((std::istreambuf_iterator<char>(bedstream)), std::istreambuf_iterator<char>());
    std::ofstream outstream(out_path);
    if (!outstream.is_open()) throw std::runtime_error(std::string("[wfmash::lift] cannot open ") + out_path);
    PafRuns pr(h, "lift", *target);
    const lift::Bed bed = lift::parse_bed(bed_text, [&](const std::string& name) { return target->find(name); }, pr.lengths, pr.offsets);
    std::lock_guard<std::mutex> lk(wflign::handle_lock(h));
    {
      std::vector<wfm_lift_iv_t> raw(bed.iv.size());
      for (size_t i = 0; i < raw.size(); ++i) raw[i] = wfm_lift_iv_t{bed.iv[i].gstart, bed.iv[i].gend};
      pr.device(wfm_liftset_create(h, raw.data(), raw.size(), pr.offsets.back(), &set), "create");
    }
    uint64_t lifted = 0, n_lines = 0, empty = 0;
    std::vector<lift::Record> where;
    std::vector<wfm_liftcall_t> per;
    std::string text;
    auto flush = [&]() {
      per.resize(pr.probs.size());
      wfm_lift_t* lifts = nullptr;
      size_t n = 0;
      pr.device(wfm_lift_runs(h, set, pr.probs.data(), pr.probs.size(), pr.runs.data(), pr.runs.size(), &lifts, &n, per.data()), "lift");
      text.clear();
      for (size_t j = 0; j < pr.probs.size(); ++j) {
        if (per[j].flags) { pr.refused(1); continue; }
        ++lifted;
        for (uint64_t k = per[j].first; k < per[j].first + per[j].count; ++k) {
          const wfm_lift_t& l = lifts[k];
          lift::lift_line(text, where[j], bed.iv[l.interval], l.p0, l.p1, l.t0, l.t1, l.eq, l.x);
          empty += l.eq + l.x == 0;
        }
        n_lines += per[j].count;
      }
      wfm_free_lifts(lifts);
      outstream << text;
      where.clear();
    };
    pr.read(in, [&](const verify::Line& l) {
      lift::Record r;
      r.qname = l.qname; r.tname = l.tname; r.qs = (uint64_t)l.qs; r.qe = (uint64_t)l.qe; r.ts = (uint64_t)l.ts; r.rev = l.rev;
      where.push_back(std::move(r));
      return true;
    }, flush);
    wfm_liftset_free(set);
    set = nullptr;
    std::cerr << "[wfmash::lift] " << bed.iv.size() << " intervals (" << bed.skipped << " BED lines skipped), " << lifted << " lines lifted, " << pr.skipped_clause()
              << ", " << n_lines << " lifts written, " << empty << " of them empty" << std::endl;
    if (out) { out[0] = lifted; out[1] = n_lines; out[2] = empty; out[3] = bed.skipped; }
    return WFM_OK;
  } catch (const std::exception& e) {
    if (set) wfm_liftset_free(set);
    std::cerr << e.what() << std::endl;
    wfm_set_error(h, e.what());
    return WFM_E_ARG;
  }
}

// --chain-paf: the chain file of an existing aligned PAF.  Lines go to the device in batches of runs, read and skipped by
// wfmh_coverage_paf's rules (coverage::classify_line); nothing else runs.
int wfmh_chain_paf(wfm_handle_t* h, const char* target_fasta, const char* aligned_paf, const char* out_path, int swap, uint64_t out[4]) {
  if (!h || !target_fasta || !aligned_paf || !out_path) return WFM_E_ARG;
  try {
    std::shared_ptr<wfmash_host::FastaStore> target = wfmash_host::open_shared(target_fasta);
    std::ifstream in(aligned_paf);
    if (!in.is_open()) throw std::runtime_error(std::string("[wfmash::chain] cannot open ") + aligned_paf);
    std::ofstream outstream(out_path);
    if (!outstream.is_open()) throw std::runtime_error(std::string("[wfmash::chain] cannot open ") + out_path);
    PafRuns pr(h, "chain", *target);
    std::lock_guard<std::mutex> lk(wflign::handle_lock(h));
    uint64_t chains = 0, n_blocks = 0, refused = 0, next = 1;
    std::vector<chain::Record> where;
    std::vector<wfm_chain_prob_t> probs;
    std::vector<wfm_chaincall_t> per;
    std::string body, text;
    auto flush = [&]() {
      probs.resize(pr.probs.size());
      per.resize(pr.probs.size());
      for (size_t j = 0; j < probs.size(); ++j) probs[j] = wfm_chain_prob_t{pr.probs[j].runs_off, pr.probs[j].n_runs, chain::flags_of(swap != 0, where[j].rev)};
      wfm_chain_block_t* blocks = nullptr;
      size_t n = 0;
      pr.device(wfm_chain_runs(h, probs.data(), probs.size(), pr.runs.data(), pr.runs.size(), &blocks, &n, per.data()), "chain");
      body.clear(); text.clear();
      for (size_t j = 0; j < probs.size(); ++j) {
        if (per[j].flags) { pr.refused(1); ++refused; continue; }
        chain::Ends e;
        e.lead_dt = per[j].lead_dt; e.lead_dq = per[j].lead_dq; e.trail_dt = per[j].trail_dt; e.trail_dq = per[j].trail_dq; e.eq = per[j].eq;
        chain::chain_body(body, where[j], swap != 0, e, (const chain::Block*)blocks + per[j].first, per[j].count);
      }
      wfm_free_chain(blocks);
      chains += chain::number(body, &next, text);
      n_blocks += n;
      outstream << text;
      where.clear();
    };
    pr.read(in, [&](const verify::Line& l) {
      chain::Record r;
      r.qname = l.qname; r.tname = l.tname; r.rev = l.rev;
      r.qsize = (uint64_t)l.qlen; r.qs = (uint64_t)l.qs; r.qe = (uint64_t)l.qe; r.tsize = (uint64_t)l.tlen; r.ts = (uint64_t)l.ts; r.te = (uint64_t)l.te;
      where.push_back(std::move(r));
      return true;
    }, flush);
    std::cerr << "[wfmash::chain] " << chains << " chains written, " << n_blocks << " blocks, " << pr.skipped_clause("lines ") << std::endl;
    if (out) { out[0] = chains; out[1] = n_blocks; out[2] = refused; out[3] = 0; }
    return WFM_OK;
  } catch (const std::exception& e) {
    std::cerr << e.what() << std::endl;
    wfm_set_error(h, e.what());
    return WFM_E_ARG;
  }
}

// --chain-paf with --chain-net: the single-coverage file of an existing aligned PAF.  Lines go to a net object in batches of runs, read and
// skipped by wfmh_coverage_paf's rules; order = the number of the line among those taken; the table once, at the end.
int wfmh_chain_net_paf(wfm_handle_t* h, const char* target_fasta, const char* aligned_paf, const char* out_path, uint64_t out[4]) {
  if (!h || !target_fasta || !aligned_paf || !out_path) return WFM_E_ARG;
  wfm_net_t* net = nullptr;
  try {
    std::shared_ptr<wfmash_host::FastaStore> target = wfmash_host::open_shared(target_fasta);
    std::ifstream in(aligned_paf);
    if (!in.is_open()) throw std::runtime_error(std::string("[wfmash::chain-net] cannot open ") + aligned_paf);
    std::ofstream outstream(out_path);
    if (!outstream.is_open()) throw std::runtime_error(std::string("[wfmash::chain-net] cannot open ") + out_path);
    PafRuns pr(h, "chain-net", *target);
    std::lock_guard<std::mutex> lk(wflign::handle_lock(h));
    pr.device(wfm_net_create(h, pr.offsets.back(), &net), "create");
    std::vector<chain::Record> where;   // of the batch
    std::vector<chain::NetHead> kept;   // of every line added, in the order of their orders
    std::vector<wfm_net_prob_t> probs;
    std::vector<uint32_t> flags;
    uint64_t taken = 0;
    auto flush = [&]() {
      probs.resize(pr.probs.size());
      flags.resize(pr.probs.size());
      for (size_t j = 0; j < probs.size(); ++j) probs[j] = wfm_net_prob_t{pr.probs[j].base, pr.probs[j].runs_off, pr.probs[j].n_runs, WFM_NET_SCORE_EQ, taken + j};
      const int refused = pr.device(wfm_net_add(h, net, probs.data(), probs.size(), pr.runs.data(), pr.runs.size(), flags.data()), "add");
      for (size_t j = 0; j < probs.size(); ++j) {
        if (flags[j]) continue;
        kept.push_back(chain::NetHead{probs[j].order, pr.probs[j].base - where[j].ts, std::move(where[j])});  // (the base is the sequence's offset + the line's target start)
      }
      pr.refused((uint64_t)refused);
      taken += probs.size();
      where.clear();
    };
    pr.read(in, [&](const verify::Line& l) {
      chain::Record r;
      r.qname = l.qname; r.tname = l.tname; r.rev = l.rev;
      r.qsize = (uint64_t)l.qlen; r.qs = (uint64_t)l.qs; r.qe = (uint64_t)l.qe; r.tsize = (uint64_t)l.tlen; r.ts = (uint64_t)l.ts; r.te = (uint64_t)l.te;
      where.push_back(std::move(r));
      return true;
    }, flush);
    wfm_net_piece_t* pieces = nullptr;
    wfm_netcall_t* per = nullptr;
    size_t n_pieces = 0, n_rec = 0;
    pr.device(wfm_net_table(h, net, &pieces, &n_pieces, &per, &n_rec), "table");
    wfm_net_free(net);
    net = nullptr;
    static_assert(sizeof(chain::Piece) == sizeof(wfm_net_piece_t) && sizeof(chain::NetCall) == sizeof(wfm_netcall_t), "chain_text.hpp restates wfm_net_piece_t and wfm_netcall_t");
    uint64_t chains = 0, lost = 0;
    const bool same = chain::net_file(outstream, kept, (const chain::NetCall*)per, n_rec, (const chain::Piece*)pieces, &chains, &lost);
    wfm_net_free_list(pieces); wfm_net_free_list(per);
    if (!same) throw std::runtime_error("[wfmash::chain-net] the table's records are not the lines added");
    std::cerr << "[wfmash::chain-net] " << n_rec << " lines added, " << chains << " chains written, " << n_pieces << " pieces, " << lost << " lines won nothing, "
              << pr.skipped_clause("lines ") << std::endl;
    if (out) { out[0] = n_rec; out[1] = chains; out[2] = n_pieces; out[3] = lost; }
    return WFM_OK;
  } catch (const std::exception& e) {
    if (net) wfm_net_free(net);
    std::cerr << e.what() << std::endl;
    wfm_set_error(h, e.what());
    return WFM_E_ARG;
  }
}

// --pav-paf: the presence table of an existing aligned PAF.  Lines go to the device in batches of runs, read and skipped by
// wfmh_coverage_paf's rules (coverage::classify_line); a line whose query the query FASTA does not have is skipped and counted too.
int wfmh_pav_paf(wfm_handle_t* h, const char* target_fasta, const char* query_fasta_or_null, const char* aligned_paf, const char* bed_path_or_null,
                 uint64_t window, const char* out_path, uint64_t out[4]) {
  const bool with_bed = bed_path_or_null && *bed_path_or_null;
  if (!h || !target_fasta || !aligned_paf || !out_path || with_bed == (window != 0)) return WFM_E_ARG;
  wfm_pav_t* obj = nullptr;
  try {
    std::shared_ptr<wfmash_host::FastaStore> target = wfmash_host::open_shared(target_fasta);
    std::shared_ptr<wfmash_host::FastaStore> query = query_fasta_or_null && *query_fasta_or_null ? wfmash_host::open_shared(query_fasta_or_null) : target;
    std::ifstream in(aligned_paf);
    if (!in.is_open()) throw std::runtime_error(std::string("[wfmash::pav] cannot open ") + aligned_paf);
    PafRuns pr(h, "pav", *target);
    const std::vector<uint64_t>&lengths = pr.lengths, &offsets = pr.offsets;
    std::vector<lift::Interval> iv;
    uint64_t bed_skipped = 0;
    if (with_bed) {
      std::ifstream bedstream(bed_path_or_null, std::ios::binary);
      if (!bedstream.is_open()) throw std::runtime_error(std::string("[wfmash::pav] cannot open ") + bed_path_or_null);
      const std::string bed_text((std::istreambuf_iterator<char>(bedstream)), std::istreambuf_iterator<char>());
      lift::Bed bed = lift::parse_bed(bed_text, [&](const std::string& name) { return target->find(name); }, lengths, offsets);
      iv = std::move(bed.iv);
      bed_skipped = bed.skipped;
    } else {
      iv = pav::windows(lengths, offsets, window);
    }
    std::vector<std::string> qnames;
    for (int i = 0; i < query->nseq(); ++i) qnames.push_back(query->name(i));
    const pav::Columns cols = pav::columns(qnames);
    std::ofstream outstream(out_path);
    if (!outstream.is_open()) throw std::runtime_error(std::string("[wfmash::pav] cannot open ") + out_path);
    std::lock_guard<std::mutex> lk(wflign::handle_lock(h));
    pr.device(wfm_pav_create(h, offsets.back(), (uint32_t)cols.keys.size(), &obj), "create");
    uint64_t added = 0, no_query = 0;
    std::vector<uint32_t> group, flags;  // the column of every line of the batch at hand
    std::vector<wfm_pav_prob_t> probs;
    pr.read(in, [&](const verify::Line& l) {
      const int qi = query->find(l.qname);
      if (qi < 0) { ++no_query; return false; }
      group.push_back(cols.of_seq[(size_t)qi]);
      return true;
    }, [&]() {
      probs.resize(pr.probs.size());
      for (size_t j = 0; j < probs.size(); ++j) probs[j] = wfm_pav_prob_t{pr.probs[j].base, pr.probs[j].runs_off, pr.probs[j].n_runs, group[j]};
      flags.resize(probs.size());
      const int refused = pr.device(wfm_pav_add(h, obj, probs.data(), probs.size(), pr.runs.data(), pr.runs.size(), flags.data()), "add");
      added += probs.size() - (uint64_t)refused;
      pr.refused((uint64_t)refused);
      group.clear();
    });
    const size_t G = cols.keys.size();
    std::vector<uint32_t> cells(G * iv.size(), 0u);
    std::vector<wfm_lift_iv_t> raw(iv.size());
    for (size_t j = 0; j < iv.size(); ++j) raw[j] = wfm_lift_iv_t{iv[j].gstart, iv[j].gend};
    pr.device(wfm_pav_matrix(h, obj, raw.data(), raw.size(), cells.data()), "matrix");
    uint64_t counts[3] = {0, 0, 0};
    wfm_pav_counts(obj, counts);
    wfm_pav_free(obj);
    obj = nullptr;
    pav::table(outstream, cols.keys, pr.names, iv, cells.data());
    std::cerr << "[wfmash::pav] " << iv.size() << " intervals (" << bed_skipped << " BED lines skipped) x " << G << " groups, " << added << " lines added, "
              << pr.skipped_clause("", &no_query) << ", " << counts[1] << " union intervals" << std::endl;
    if (out) { out[0] = added; out[1] = iv.size(); out[2] = counts[1]; out[3] = bed_skipped; }
    return WFM_OK;
  } catch (const std::exception& e) {
    if (obj) wfm_pav_free(obj);
    std::cerr << e.what() << std::endl;
    wfm_set_error(h, e.what());
    return WFM_E_ARG;
  }
}

// --transitive-paf: the closure of the BED's intervals over an existing aligned PAF.  Lines go to a trans object in batches of runs, read
// and skipped by wfmh_coverage_paf's rules (coverage::classify_line); a line whose query neither FASTA has is skipped and counted too; the
// closure once, at the end.
int wfmh_transitive_paf(wfm_handle_t* h, const char* target_fasta, const char* query_fasta_or_null, const char* aligned_paf, const char* bed_path,
                        const char* out_path, uint32_t depth, uint64_t out[4]) {
  if (!h || !target_fasta || !aligned_paf || !bed_path || !out_path) return WFM_E_ARG;
  wfm_trans_t* obj = nullptr;
  try {
    std::shared_ptr<wfmash_host::FastaStore> target = wfmash_host::open_shared(target_fasta);
    std::shared_ptr<wfmash_host::FastaStore> query = query_fasta_or_null && *query_fasta_or_null ? wfmash_host::open_shared(query_fasta_or_null) : target;
    std::ifstream in(aligned_paf);
    if (!in.is_open()) throw std::runtime_error(std::string("[wfmash::transitive] cannot open ") + aligned_paf);
    std::ifstream bedstream(bed_path, std::ios::binary);
    if (!bedstream.is_open()) throw std::runtime_error(std::string("[wfmash::transitive] cannot open ") + bed_path);
    const std::string bed_text((std::istreambuf_iterator<char>(bedstream)), std::istreambuf_iterator<char>());
    PafRuns pr(h, "transitive", *target);
    std::vector<std::string> qnames;
    std::vector<uint64_t> qlengths;
    for (int i = 0; i < query->nseq(); ++i) { qnames.push_back(query->name(i)); qlengths.push_back((uint64_t)query->length(i)); }
    const transitive::World world = transitive::make_world(pr.names, pr.lengths, qnames, qlengths);
    if (world.n_bases() >= ((uint64_t)1 << 40)) throw std::runtime_error("[wfmash::transitive] the sequences hold 2^40 bases or more");
    const lift::Bed seeds = transitive::parse_seeds(bed_text, world);
    if (seeds.iv.size() >= ((size_t)1 << 24)) throw std::runtime_error("[wfmash::transitive] the BED holds 2^24 seeds or more");
    std::ofstream outstream(out_path);
    if (!outstream.is_open()) throw std::runtime_error(std::string("[wfmash::transitive] cannot open ") + out_path);
    std::lock_guard<std::mutex> lk(wflign::handle_lock(h));
    pr.device(wfm_trans_create(h, world.n_bases(), &obj), "create");
    uint64_t added = 0, no_query = 0;
    std::vector<std::pair<uint64_t, bool>> where;  // of the batch at hand: the world place of the line's forward query window, its strand
    std::vector<wfm_trans_prob_t> probs;
    std::vector<uint32_t> flags;
    pr.read(in, [&](const verify::Line& l) {
      const int qi = world.find(l.qname);
      if (qi < 0 || (uint64_t)l.qe > world.lengths[(size_t)qi]) { ++no_query; return false; }
      where.emplace_back(transitive::query_world(world.offsets[(size_t)qi], (uint64_t)l.qs), l.rev);
      return true;
    }, [&]() {
      probs.resize(pr.probs.size());
      flags.resize(probs.size());
      for (size_t j = 0; j < probs.size(); ++j)
        probs[j] = wfm_trans_prob_t{pr.probs[j].base, where[j].first, pr.probs[j].runs_off, pr.probs[j].n_runs, where[j].second ? WFM_TRANS_REVERSE : 0u};
      const int refused = pr.device(wfm_trans_add(h, obj, probs.data(), probs.size(), pr.runs.data(), pr.runs.size(), flags.data()), "add");
      added += probs.size() - (uint64_t)refused;
      pr.refused((uint64_t)refused);
      where.clear();
    });
    std::vector<wfm_lift_iv_t> raw(seeds.iv.size());
    for (size_t i = 0; i < raw.size(); ++i) raw[i] = wfm_lift_iv_t{seeds.iv[i].gstart, seeds.iv[i].gend};
    std::vector<wfm_trans_seed_t> per(raw.size());
    wfm_trans_iv_t* ivs = nullptr;
    size_t n_ivs = 0;
    pr.device(wfm_trans_closure(h, obj, raw.data(), raw.size(), depth, &ivs, &n_ivs, per.data()), "closure");
    uint64_t counts[6] = {0, 0, 0, 0, 0, 0};
    wfm_trans_counts(obj, counts);
    wfm_trans_free(obj);
    obj = nullptr;
    static_assert(sizeof(transitive::ClosureIv) == sizeof(wfm_trans_iv_t) && sizeof(transitive::SeedCall) == sizeof(wfm_trans_seed_t),
                  "transitive_text.hpp restates wfm_trans_iv_t and wfm_trans_seed_t");
    const uint64_t lines = transitive::file(outstream, world, seeds.iv, (const transitive::SeedCall*)per.data(), (const transitive::ClosureIv*)ivs);
    wfm_trans_free_list(ivs);
    std::cerr << "[wfmash::transitive] " << seeds.iv.size() << " seeds (" << seeds.skipped << " BED lines skipped), " << added << " lines added, "
              << pr.skipped_clause("", &no_query) << ", " << counts[3] << " rounds, " << lines << " lines written" << std::endl;
    if (out) { out[0] = added; out[1] = lines; out[2] = counts[3]; out[3] = seeds.skipped; }
    return WFM_OK;
  } catch (const std::exception& e) {
    if (obj) wfm_trans_free(obj);
    std::cerr << e.what() << std::endl;
    wfm_set_error(h, e.what());
    return WFM_E_ARG;
  }
}

// test hook (no GPU): the bedGraph of n_iv intervals over n_seq sequences, as the align phase writes it.  malloc'd, wfmh_free.
char* wfmh_test_coverage_bedgraph(const char* const* names, const uint64_t* lengths, int n_seq, const uint64_t* starts, const uint32_t* depths, int64_t n_iv) {
  std::vector<std::string> nm;
  std::vector<uint64_t> len;
  std::vector<coverage::Interval> iv;
  for (int i = 0; i < n_seq; ++i) { nm.push_back(names[i]); len.push_back(lengths[i]); }
  for (int64_t i = 0; i < n_iv; ++i) iv.push_back(coverage::Interval{starts[i], depths[i]});
  const std::string s = coverage::coverage_bedgraph(nm, len, iv, nullptr);
  char* p = (char*)malloc(s.size() + 1);
  if (p) memcpy(p, s.c_str(), s.size() + 1);
  return p;
}

// test hook (no GPU): a line as the verifier reads it.  "ok <TAB> qname qs qe strand tname ts te runs" with the runs spelled
// back as a CIGAR over =XID, or "unverifiable <TAB> reason" / "malformed <TAB> reason".  Release with wfmh_free.
char* wfmh_test_verify_parse(const char* line) {
  if (!line) return nullptr;
  verify::Line l;
  std::string why;
  const int st = verify::parse_line(line, l, &why);
  std::string s;
  if (st == verify::LINE_UNVERIFIABLE) s = "unverifiable\t" + why;
  else if (st == verify::LINE_MALFORMED) s = "malformed\t" + why;
  else {
    s = "ok\t" + l.qname + "\t" + std::to_string(l.qs) + "\t" + std::to_string(l.qe) + "\t" + (l.rev ? "-" : "+") + "\t" + l.tname + "\t" +
        std::to_string(l.ts) + "\t" + std::to_string(l.te) + "\t";
    for (uint32_t w : l.runs) { s += std::to_string(WFM_RUN_LEN(w)); s += "=XID"[WFM_RUN_OP(w)]; }
  }
  char* p = (char*)malloc(s.size() + 1);
  if (p) memcpy(p, s.c_str(), s.size() + 1);
  return p;
}

}  // extern "C"
