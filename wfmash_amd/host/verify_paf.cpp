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
#include "maf_text.hpp"
#include "parallel.hpp"
#include "run_passes.hpp"

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
// What --verify-paf and --maf-paf share: the two files (the query's only where it is another), the source of the bases, the PAF open, and
// its text in chunks of 64 MiB of whole lines.  tag: the [wfmash::...] of "cannot open".
struct PafText {
  std::shared_ptr<wfmash_host::FastaStore> target, query_own;
  verify::Source src;
  std::ifstream in;
  PafText(const char* tag, const char* target_fasta, const char* query_fasta, const char* aligned_paf) {
    target = wfmash_host::open_shared(target_fasta);
    const std::string qpath = query_fasta ? query_fasta : target_fasta;
    if (qpath != target_fasta) query_own = wfmash_host::open_shared(qpath);
    src.target = target.get();
    src.query = query_own ? query_own.get() : target.get();
    src.threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    in.open(aligned_paf);
    if (!in.is_open()) throw std::runtime_error(std::string("[wfmash::") + tag + "] cannot open " + aligned_paf);
  }
  template <class Chunk>
  void chunks(Chunk chunk) {
    std::string text, line;
    while (std::getline(in, line)) {
      text += line; text += '\n';
      if (text.size() >= ((size_t)64 << 20)) { chunk(text); text.clear(); }
    }
    chunk(text);
  }
};

// a --*-paf entry point's body: what it throws is printed, left as the handle's error and returned as WFM_E_ARG
template <class Body>
int guarded(wfm_handle_t* h, Body body) {
  try {
    body();
    return WFM_OK;
  } catch (const std::exception& e) {
    std::cerr << e.what() << std::endl;
    wfm_set_error(h, e.what());
    return WFM_E_ARG;
  }
}

// "N skipped (... without an =XID cg:Z:, ... malformed, ...)" of the summaries; with_query: the lines left out for their query as well
std::string skipped_clause(const wflign::PafPassResult& r, const char* noun = "", bool with_query = false) {
  std::string s = std::to_string(r.all_skipped() + r.no_query) + " " + noun + "skipped (" + std::to_string(r.skipped[1]) + " without an =XID cg:Z:, " +
                  std::to_string(r.skipped[2]) + " malformed, " + std::to_string(r.skipped[3]) + " with an unknown target, " + std::to_string(r.skipped[4]) + " with another tlen";
  if (with_query) s += ", " + std::to_string(r.no_query) + " with an unknown query";
  return s + ")";
}
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
  return guarded(h, [&] {
    PafText paf("verify", target_fasta, query_fasta, aligned_paf);
    verify::Counts c;
    paf.chunks([&](const std::string& text) { verify::verify_text(h, paf.src, text, c); });
    if (out) { out[0] = c.checked; out[1] = c.failed; out[2] = c.unverifiable; out[3] = c.bases; }
  });
}

// --maf-paf: the MAF file of an existing aligned PAF, lines parsed as --verify-paf parses them and their windows uploaded as it uploads
// them; a line whose target the target file does not have, or whose query the query file does not (wfmh_verify_paf's lookup),
// or that names another length, is skipped and counted.  Nothing else runs.
int wfmh_maf_paf(wfm_handle_t* h, const char* target_fasta, const char* query_fasta, const char* aligned_paf, const char* out_path, uint32_t split,
                 uint64_t out[4]) {
  if (!h || !target_fasta || !aligned_paf || !out_path) return WFM_E_ARG;
  return guarded(h, [&] {
    PafText paf("maf", target_fasta, query_fasta, aligned_paf);
    std::ofstream outstream(out_path);
    if (!outstream.is_open()) throw std::runtime_error(std::string("[wfmash::maf] cannot open ") + out_path);
    outstream << maf::header();
    uint64_t counts[4] = {0, 0, 0, 0}, skipped[4] = {0, 0, 0, 0};
    paf.chunks([&](const std::string& text) { verify::maf_text(h, paf.src, text, split, outstream, counts, skipped); });
    std::cerr << "[wfmash::maf] " << counts[0] << " records, " << counts[1] << " blocks, " << counts[2] << " columns, " << counts[3] << " records left without blocks, "
              << (skipped[0] + skipped[1] + skipped[2] + skipped[3]) << " lines skipped (" << skipped[0] << " without an =XID cg:Z:, " << skipped[1] << " malformed, "
              << skipped[2] << " with an unknown sequence, " << skipped[3] << " with another length)" << std::endl;
    if (out) for (int q = 0; q < 4; ++q) out[q] = counts[q];
  });
}

// ---- the modes that make an across-record output of an existing aligned PAF: the lines are the second source of packed runs for the
// pass and the stage the align driver has (run_passes.hpp: run_paf_pass); nothing else runs.  Here: the argument checks, the summary, out[4]. ----
using wflign::PafPassCall;
using wflign::PafPassResult;

// --coverage-paf: the depth of an existing aligned PAF
int wfmh_coverage_paf(wfm_handle_t* h, const char* target_fasta, const char* aligned_paf, const char* out_path, uint64_t out[4]) {
  if (!h || !target_fasta || !aligned_paf || !out_path) return WFM_E_ARG;
  return guarded(h, [&] {
    const PafPassResult r = wflign::run_paf_pass(h, PafPassCall{wflign::SW_COVERAGE, "coverage", target_fasta, nullptr, aligned_paf, nullptr, out_path, 0});
    std::cerr << "[wfmash::coverage] " << r.counts[0] << " lines added, " << skipped_clause(r) << ", " << r.end.c[0] << " bases covered, sum of depth " << r.end.c[1]
              << ", max depth " << r.end.extra << ", " << r.end.c[2] << " intervals" << std::endl;
    if (out) { out[0] = r.counts[0]; out[1] = r.all_skipped(); out[2] = r.end.c[0]; out[3] = r.end.c[1]; }
  });
}

// --lift-paf: the BED intervals lifted through an existing aligned PAF
int wfmh_lift_paf(wfm_handle_t* h, const char* target_fasta, const char* aligned_paf, const char* bed_path, const char* out_path, uint64_t out[4]) {
  if (!h || !target_fasta || !aligned_paf || !bed_path || !out_path) return WFM_E_ARG;
  return guarded(h, [&] {
    const PafPassResult r = wflign::run_paf_pass(h, PafPassCall{wflign::SW_LIFT, "lift", target_fasta, nullptr, aligned_paf, bed_path, out_path, 0});
    std::cerr << "[wfmash::lift] " << r.end.extra << " intervals (" << r.end.c[2] << " BED lines skipped), " << r.counts[0] << " lines lifted, " << skipped_clause(r)
              << ", " << r.counts[1] << " lifts written, " << r.counts[2] << " of them empty" << std::endl;
    if (out) { out[0] = r.counts[0]; out[1] = r.counts[1]; out[2] = r.counts[2]; out[3] = r.end.c[2]; }
  });
}

// --chain-paf: the chain file of an existing aligned PAF
int wfmh_chain_paf(wfm_handle_t* h, const char* target_fasta, const char* aligned_paf, const char* out_path, int swap, uint64_t out[4]) {
  if (!h || !target_fasta || !aligned_paf || !out_path) return WFM_E_ARG;
  return guarded(h, [&] {
    const PafPassResult r = wflign::run_paf_pass(h, PafPassCall{wflign::SW_CHAIN, "chain", target_fasta, nullptr, aligned_paf, nullptr, out_path, swap != 0});
    std::cerr << "[wfmash::chain] " << r.counts[0] << " chains written, " << r.counts[1] << " blocks, " << skipped_clause(r, "lines ") << std::endl;
    if (out) { out[0] = r.counts[0]; out[1] = r.counts[1]; out[2] = r.counts[2]; out[3] = 0; }
  });
}

// --chain-paf with --chain-net: the single-coverage file of an existing aligned PAF; order = the number of the line among those taken
int wfmh_chain_net_paf(wfm_handle_t* h, const char* target_fasta, const char* aligned_paf, const char* out_path, uint64_t out[4]) {
  if (!h || !target_fasta || !aligned_paf || !out_path) return WFM_E_ARG;
  return guarded(h, [&] {
    const PafPassResult r = wflign::run_paf_pass(h, PafPassCall{wflign::SW_CHAIN_NET, "chain-net", target_fasta, nullptr, aligned_paf, nullptr, out_path, 0});
    std::cerr << "[wfmash::chain-net] " << r.counts[0] << " lines added, " << r.end.c[0] << " chains written, " << r.end.c[1] << " pieces, " << r.end.c[2]
              << " lines won nothing, " << skipped_clause(r, "lines ") << std::endl;
    if (out) { out[0] = r.counts[0]; out[1] = r.end.c[0]; out[2] = r.end.c[1]; out[3] = r.end.c[2]; }
  });
}

// --pav-paf: the presence table of an existing aligned PAF; a line whose query the query FASTA does not have is skipped and counted too
int wfmh_pav_paf(wfm_handle_t* h, const char* target_fasta, const char* query_fasta_or_null, const char* aligned_paf, const char* bed_path_or_null,
                 uint64_t window, const char* out_path, uint64_t out[4]) {
  const bool with_bed = bed_path_or_null && *bed_path_or_null;
  if (!h || !target_fasta || !aligned_paf || !out_path || with_bed == (window != 0)) return WFM_E_ARG;
  return guarded(h, [&] {
    const PafPassResult r = wflign::run_paf_pass(h, PafPassCall{wflign::SW_PAV, "pav", target_fasta, query_fasta_or_null, aligned_paf, bed_path_or_null, out_path, window});
    std::cerr << "[wfmash::pav] " << r.end.c[0] << " intervals (" << r.end.c[2] << " BED lines skipped) x " << r.groups << " groups, " << r.counts[0] << " lines added, "
              << skipped_clause(r, "", true) << ", " << r.end.c[1] << " union intervals" << std::endl;
    if (out) { out[0] = r.counts[0]; out[1] = r.end.c[0]; out[2] = r.end.c[1]; out[3] = r.end.c[2]; }
  });
}

// --transitive-paf: the closure of the BED's intervals over an existing aligned PAF; a line whose query neither FASTA has is skipped and
// counted too
int wfmh_transitive_paf(wfm_handle_t* h, const char* target_fasta, const char* query_fasta_or_null, const char* aligned_paf, const char* bed_path,
                        const char* out_path, uint32_t depth, uint64_t out[4]) {
  if (!h || !target_fasta || !aligned_paf || !bed_path || !out_path) return WFM_E_ARG;
  return guarded(h, [&] {
    const PafPassResult r =
        wflign::run_paf_pass(h, PafPassCall{wflign::SW_TRANSITIVE, "transitive", target_fasta, query_fasta_or_null, aligned_paf, bed_path, out_path, depth});
    std::cerr << "[wfmash::transitive] " << r.end.extra << " seeds (" << r.end.c[2] << " BED lines skipped), " << r.counts[0] << " lines added, "
              << skipped_clause(r, "", true) << ", " << r.end.c[1] << " rounds, " << r.end.c[0] << " lines written" << std::endl;
    if (out) { out[0] = r.counts[0]; out[1] = r.end.c[0]; out[2] = r.end.c[1]; out[3] = r.end.c[2]; }
  });
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
