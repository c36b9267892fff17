#include "aligner.hpp"
#include "verify_paf.hpp"
#include "coverage_text.hpp"
#include "lift_text.hpp"
#include "chain_text.hpp"
#include "pav_text.hpp"
#include "genotype_text.hpp"
#include "transitive_text.hpp"
#include "map_queue.hpp"
#include "parallel.hpp"
#include "../csrc/wfa_handle.h"

#include <algorithm>
#include <thread>
#include <atomic>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <map>
#include <mutex>
#include <sstream>
#include <stdexcept>

namespace align {

namespace {

std::vector<std::string> tokenize(const std::string& s) {  // whitespace split (computeAlignments.hpp:54-72)
  std::vector<std::string> t;
  size_t pos = 0;
  while (pos < s.size()) {
    while (pos < s.size() && std::isspace((unsigned char)s[pos])) ++pos;
    if (pos >= s.size()) break;
    const size_t st = pos;
    while (pos < s.size() && !std::isspace((unsigned char)s[pos])) ++pos;
    t.emplace_back(s.substr(st, pos - st));
  }
  return t;
}

std::vector<std::string> split(const std::string& s, char d) {  // computeAlignments.hpp:35-51
  std::vector<std::string> r;
  size_t pos = 0, f;
  while ((f = s.find(d, pos)) != std::string::npos) { r.emplace_back(s.substr(pos, f - pos)); pos = f + 1; }
  if (pos <= s.size()) r.emplace_back(s.substr(pos));
  return r;
}

bool is_a_number(const std::string& s) {  // utils.cpp:9-11
  return !s.empty() && s.find_first_not_of("0123456789.") == std::string::npos && std::count(s.begin(), s.end(), '.') < 2;
}

}  // namespace

// makeUpperCaseAndValidDNA (commonFunc.hpp:132-142)
void upper_valid_dna(std::string& s) {
  for (auto& c : s) {
    if (c > 96 && c < 123) c -= 32;
    if (!(c == 'A' || c == 'C' || c == 'G' || c == 'T')) c = 'N';
  }
}

// reverseComplement (commonFunc.hpp:74-83) on validated DNA
std::string revcomp(const std::string& s) {
  std::string r(s.size(), 'N');
  for (size_t i = 0; i < s.size(); ++i) {
    char c = s[i], o;
    switch (c) { case 'A': o = 'T'; break; case 'C': o = 'G'; break; case 'G': o = 'C'; break; case 'T': o = 'A'; break; default: o = c; }
    r[s.size() - 1 - i] = o;
  }
  return r;
}

struct Aligner::Fetched {
  MappingBoundaryRow row;
  std::string ref;    // padded reference window
  std::string qry;    // strand-adjusted query window
  uint64_t ref_start = 0, ref_total = 0, q_total = 0;
  uint64_t row_no = 0;  // the row's number in the mapping file
  int32_t ref_seq = -1, qry_seq = -1;  // resident_sequences: the sides' ids in the device's store (-1: by host pointer)
  bool lazy = false;                   // ... both are there and the output is PAF: the bases are fetched only on demand
};

Aligner::Aligner(const Parameters& p, wfm_handle_t* g) : Aligner(p, std::vector<wfm_handle_t*>{g}) {}

Aligner::Aligner(const Parameters& p, const std::vector<wfm_handle_t*>& g) : param(p), gpus(g) {
  if (gpus.empty() || std::find(gpus.begin(), gpus.end(), nullptr) != gpus.end()) throw std::runtime_error("[wfmash::align] no GPU handle");
  if (param.refSequences.size() != 1 || param.querySequences.size() != 1)
    throw std::runtime_error("[wfmash::align] exactly one target and one query FASTA are expected");
  // (shared with whoever has the file open -- a map phase just before this leaves its sequences loaded: fasta.hpp, keep_until_next)
  ref = wfmash_host::open_shared(param.refSequences.front());
  if (param.querySequences.front() == param.refSequences.front()) query = ref.get();
  else { query_own = wfmash_host::open_shared(param.querySequences.front()); query = query_own.get(); }
}

Aligner::~Aligner() {
  for (auto& kv : stores) if (kv.second && kv.second->store) wfm_seqstore_free(kv.second->store);
}

Aligner::DeviceStore* Aligner::device_store(wfm_handle_t* h) {
  std::lock_guard<std::mutex> lk(stores_mu);
  auto& ds = stores[wfm_device(h)];
  if (!ds) {
    ds.reset(new DeviceStore());
    if (wfm_seqstore_create(h, &ds->store) != WFM_OK) throw std::runtime_error("[wfmash::align] cannot create the device sequence store");
    // (the figure the host side uses for the sequences it keeps, WFM_FASTA_KEEP_GB; a decimal, so that a test can ask for kilobytes)
    const char* g = getenv("WFM_SEQSTORE_GB");
    const double gb = g && *g ? atof(g) : 32.0;
    ds->budget = gb > 0 ? (int64_t)(gb * 1073741824.0) : 0;
  }
  return ds.get();
}

int32_t Aligner::resident_id(wfm_handle_t* h, DeviceStore& ds, const wfmash_host::FastaStore* fa, int idx) {
  if (idx < 0) return -1;
  std::lock_guard<std::mutex> lk(ds.mu);
  const auto key = std::make_pair(fa, idx);
  auto it = ds.ids.find(key);
  if (it != ds.ids.end()) return it->second;
  int32_t id = -1;
  const int64_t len = fa->length(idx);
  if (len > 0 && len <= ds.budget - ds.used) {
    const wfmash_host::SeqView v = fa->sequence(idx);
    std::lock_guard<std::mutex> hl(wflign::handle_lock(h));
    id = wfm_seqstore_add(h, ds.store, v.data(), (int64_t)v.size());
    if (id >= 0) ds.used += len;
    else { std::cerr << "[wfmash::align] " << fa->name(idx) << " stays on the host: " << wfm_last_error(h) << std::endl; id = -1; }
  }
  ds.ids.emplace(key, id);
  return id;
}

void Aligner::parseMashmapRow(const std::string& line, MappingBoundaryRow& row, uint64_t target_padding, uint64_t query_padding) {
  const auto tokens = tokenize(line);
  if (tokens.size() < 13)
    throw std::runtime_error("[wfmash::align::parseMashmapRow] Error! Invalid mashmap mapping record: " + line);
  const auto idv = split(tokens[12], ':');
  const float mm_id = (!idv.empty() && is_a_number(idv.back())) ? std::stof(idv.back()) : 0.70f;  // fixed::percentage_identity
  int64_t chain_id = -1, chain_length = 1, chain_pos = 1;
  // only tokens 12 and 14 are read (computeAlignments.hpp:203-230): the cg:Z / st:Z tags an -K record carries after ch:Z are passed over
  if (tokens.size() > 14) {
    const auto cv = split(tokens[14], ':');
    if (cv.size() == 3 && cv[0] == "ch" && cv[1] == "Z") {
      const auto parts = split(cv[2], '.');
      if (parts.size() == 3) {  // ch:Z:id.pos.len as the mapper writes it (mappingOutput.hpp:121)
        chain_id = std::stoll(parts[0]); chain_pos = std::stoll(parts[1]); chain_length = std::stoll(parts[2]);
      }
    }
  }
  row.qId = tokens[0];
  row.qStartPos = std::stoll(tokens[2]);
  row.qEndPos = std::stoll(tokens[3]);
  row.strand = tokens[4] == "+" ? FWD : REV;
  row.refId = tokens[5];
  const uint64_t ref_len = std::stoull(tokens[6]);
  row.chain_id = (int32_t)chain_id; row.chain_length = (int32_t)chain_length; row.chain_pos = (int32_t)chain_pos;
  uint64_t rs = (uint64_t)std::stoll(tokens[7]), re = (uint64_t)std::stoll(tokens[8]);
  uint64_t qs = (uint64_t)row.qStartPos, qe = (uint64_t)row.qEndPos;
  const uint64_t query_len = std::stoull(tokens[1]);
  if (target_padding > 0) {
    rs = rs >= target_padding ? rs - target_padding : 0;
    re = re + target_padding <= ref_len ? re + target_padding : ref_len;
  }
  if (query_padding > 0) {
    // padding only at the chain ends, and only STORED for the last piece (computeAlignments.hpp:268-289)
    if (chain_pos == 1) qs = qs >= query_padding ? qs - query_padding : 0;
    if (chain_pos == chain_length) {
      qe = qe + query_padding <= query_len ? qe + query_padding : query_len;
      row.qStartPos = (int64_t)qs;
      row.qEndPos = (int64_t)qe;
    }
  }
  if (rs >= ref_len || re > ref_len)
    throw std::runtime_error("[wfmash::align::parseMashmapRow] Error! Coordinates exceed reference length: " +
                             std::to_string(rs) + "-" + std::to_string(re) + " (ref_len=" + std::to_string(ref_len) + ")");
  row.rStartPos = (int64_t)rs;
  row.rEndPos = (int64_t)re;
  row.mashmap_estimated_identity = mm_id;
}

// One batch of mapping rows through the wflign pipeline on one GPU: createSeqRecord + processAlignment
// (computeAlignments.hpp:582-723) for every row, then the records' output text in row order.
namespace {
// WFM_RECORD_TAGS=<file>: one line per aligned record -- the row's number in the mapping file (0-based, empty lines not counted), the record's
// WFM_PF_* bits (main alignment | head patch << 8 | tail patch << 16) and its score.  The parity tests and bench.py draw their samples from it.
std::mutex g_tags_mu;
void write_record_tags(const std::vector<uint64_t>& row_no, const std::vector<wflign::BiwfaRecord>& recs) {
  const char* path = getenv("WFM_RECORD_TAGS");
  if (!path || !*path) return;
  std::lock_guard<std::mutex> lk(g_tags_mu);
  if (FILE* f = fopen(path, "a")) {
    for (size_t k = 0; k < recs.size(); ++k) fprintf(f, "%llu\t%u\t%d\t%d\n", (unsigned long long)row_no[k], recs[k].tags, recs[k].score, recs[k].ok ? 1 : 0);
    fclose(f);
  }
}

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point a) { return std::chrono::duration<double, std::milli>(Clock::now() - a).count(); }

wflign::wflign_penalties_t penalties_of(const Parameters& param) {
  wflign::wflign_penalties_t pen;
  pen.match = 0;
  pen.mismatch = param.wfa_patching_mismatch_score;
  pen.gap_opening1 = param.wfa_patching_gap_opening_score1;
  pen.gap_extension1 = param.wfa_patching_gap_extension_score1;
  pen.gap_opening2 = param.wfa_patching_gap_opening_score2;
  pen.gap_extension2 = param.wfa_patching_gap_extension_score2;
  return pen;
}
wflign::PafParams filters_of(const Parameters& param) {
  wflign::PafParams pp;
  pp.min_identity = param.min_identity;
  pp.min_alignment_length = param.min_alignment_length;
  pp.min_block_identity = param.min_block_identity;
  return pp;
}
wflign::OutputFormat format_of(const Parameters& param, int threads) {
  wflign::OutputFormat fmt;
  fmt.paf_format_else_sam = !param.sam_format;
  fmt.no_seq_in_sam = param.no_seq_in_sam;
  fmt.emit_md_tag = param.emit_md_tag;
  fmt.threads = threads;
  return fmt;
}
}  // namespace

// the stages' times of one batch: lap() is the time since the lap before
struct Aligner::BatchTimes {
  Clock::time_point at = Clock::now();
  double rows = 0, fetch = 0, wflign = 0, text = 0;
  double lap() {
    const auto now = Clock::now();
    const double ms = std::chrono::duration<double, std::milli>(now - at).count();
    at = now;
    return ms;
  }
};

// rows first (cheap, in order); a row that does not parse or names an unknown sequence is reported and skipped
std::vector<Aligner::Fetched> Aligner::parse_rows(std::vector<std::string>& lines, uint64_t first_row, Summary& sum) const {
  std::vector<Fetched> rows;
  uint64_t row_no = first_row;
  for (const std::string& line : lines) {
    if (line.empty()) continue;
    Fetched f;
    f.row_no = row_no++;
    try {
      parseMashmapRow(line, f.row, param.target_padding, param.query_padding);
      const int64_t ref_size = ref->seq_len(f.row.refId);
      if (ref_size < 0) throw std::runtime_error("Reference sequence not found: " + f.row.refId);
      const int64_t query_size = query->seq_len(f.row.qId);
      if (query_size < 0) throw std::runtime_error("Query sequence not found: " + f.row.qId);
      f.ref_total = (uint64_t)ref_size; f.q_total = (uint64_t)query_size;
      rows.push_back(std::move(f));
    } catch (const std::exception& e) {
      std::cerr << "[wfmash::align] Error processing record: " << e.what() << std::endl;
      sum.skipped++;
    }
  }
  std::vector<std::string>().swap(lines);
  return rows;
}

// resident_sequences: the sides' ids in the device's store, each sequence added on first use.  A record with both sides there
// is not fetched up front when the output is PAF (SAM needs the bases for SEQ and MD).
void Aligner::assign_resident_ids(wfm_handle_t* gpu_handle, DeviceStore& ds, std::vector<Fetched>& rows) {
  for (Fetched& f : rows) {
    if (f.row.rStartPos >= 0 && f.row.rEndPos > f.row.rStartPos && (uint64_t)f.row.rEndPos <= f.ref_total)
      f.ref_seq = resident_id(gpu_handle, ds, ref.get(), ref->find(f.row.refId));
    if (f.row.qStartPos >= 0 && f.row.qEndPos > f.row.qStartPos && (uint64_t)f.row.qEndPos <= f.q_total)
      f.qry_seq = resident_id(gpu_handle, ds, query, query->find(f.row.qId));
    f.lazy = f.ref_seq >= 0 && f.qry_seq >= 0 && !param.sam_format;
  }
}

// the padded reference window and the strand-adjusted query window of a row, normalised
void Aligner::fetch_windows(Fetched& f) const {
  const int64_t ref_size = (int64_t)f.ref_total;
  const uint64_t head_pad = (uint64_t)f.row.rStartPos >= param.wflign_max_len_minor ? param.wflign_max_len_minor : (uint64_t)f.row.rStartPos;
  const uint64_t tail_pad = (uint64_t)(ref_size - f.row.rEndPos) >= param.wflign_max_len_minor ? param.wflign_max_len_minor : (uint64_t)(ref_size - f.row.rEndPos);
  f.ref = ref->fetch(f.row.refId, f.row.rStartPos - (int64_t)head_pad, f.row.rEndPos + (int64_t)tail_pad - 1);
  if (f.ref.empty()) throw std::runtime_error("Failed to fetch reference sequence");
  std::string q = query->fetch(f.row.qId, f.row.qStartPos, f.row.qEndPos - 1);
  if (q.empty()) throw std::runtime_error("Failed to fetch query sequence");
  f.ref_start = (uint64_t)f.row.rStartPos - head_pad;
  upper_valid_dna(f.ref);
  upper_valid_dna(q);
  f.qry = f.row.strand == FWD ? std::move(q) : revcomp(q);
}

// the sequence fetches of the whole batch on `threads` threads (lazy rows aside); a row whose fetch fails is reported and skipped
std::vector<Aligner::Fetched> Aligner::fetch_eager(std::vector<Fetched>& rows, int threads, Summary& sum) const {
  std::vector<std::string> fetch_error(rows.size());
  std::atomic<size_t> next{0};
  const int nt = (int)std::min<size_t>((size_t)std::max(1, threads), rows.size());
  // (helpers from the process's pool, parallel.hpp: every one of them shares the rows out by the one counter)
  wfmash_host::parallel_for((size_t)nt, nt, [&](size_t) {
    for (size_t k; (k = next.fetch_add(1)) < rows.size();) {
      if (rows[k].lazy) continue;
      try {
        fetch_windows(rows[k]);
      } catch (const std::exception& e) {
        fetch_error[k] = *e.what() ? e.what() : "error";
      }
    }
  });
  std::vector<Fetched> fetched;
  fetched.reserve(rows.size());
  for (size_t k = 0; k < rows.size(); ++k) {
    if (!fetch_error[k].empty()) {
      std::cerr << "[wfmash::align] Error processing record: " << fetch_error[k] << std::endl;
      sum.skipped++;
      continue;
    }
    fetched.push_back(std::move(rows[k]));
  }
  return fetched;
}

// the host pointers of a record whose windows have been fetched
void Aligner::point_at(wflign::BiwfaRecord& r, const Fetched& f) {
  const uint64_t skip = (uint64_t)f.row.rStartPos - f.ref_start;
  r.query = f.qry.data();
  r.target = f.ref.data() + skip;
  r.target_avail = f.ref.size() - skip;
}

std::vector<wflign::BiwfaRecord> Aligner::make_records(const std::vector<Fetched>& fetched) {
  std::vector<wflign::BiwfaRecord> recs(fetched.size());
  for (size_t k = 0; k < fetched.size(); ++k) {
    const Fetched& f = fetched[k];
    wflign::BiwfaRecord& r = recs[k];
    r.query_name = f.row.qId;
    r.query_total_length = f.q_total;
    r.query_offset = (uint64_t)f.row.qStartPos;
    r.query_length = f.lazy ? (uint64_t)(f.row.qEndPos - f.row.qStartPos) : f.qry.size();
    r.query_is_rev = f.row.strand != FWD;
    r.target_name = f.row.refId;
    r.target_total_length = f.ref_total;
    r.target_offset = (uint64_t)f.row.rStartPos;
    r.target_length = (uint64_t)(f.row.rEndPos - f.row.rStartPos);
    if (!f.lazy) point_at(r, f);
    r.target_seq = f.ref_seq; r.target_win_off = f.row.rStartPos;
    r.query_seq = f.qry_seq; r.query_win_off = f.row.qStartPos;
    r.mashmap_estimated_identity = f.row.mashmap_estimated_identity;
    r.chain_id = f.row.chain_id; r.chain_length = f.row.chain_length; r.chain_pos = f.row.chain_pos;
  }
  return recs;
}

// what the device call did, into the summary; the records' tags where they are asked for
void Aligner::account(Summary& sum, const wflign::BiwfaStats& st, const wflign::ResidentSeqs& resident, const std::vector<Fetched>& fetched,
                      const std::vector<wflign::BiwfaRecord>& recs) {
  sum.lazy_fetches += resident.lazy_fetches.load();
  sum.cells += st.cells; sum.ms_gpu += st.ms_gpu;
  sum.cells_tile += st.cells_tile; sum.tile_launches += st.tile_launches; sum.ms_tile += st.ms_tile;
  sum.busy.insert(sum.busy.end(), st.busy.begin(), st.busy.end());
  if (getenv("WFM_RECORD_TAGS")) {
    const auto tt = Clock::now();
    std::vector<uint64_t> rn(fetched.size());
    for (size_t k = 0; k < fetched.size(); ++k) rn[k] = fetched[k].row_no;
    write_record_tags(rn, recs);
    sum.ms_tags += ms_since(tt);
  }
}

std::string Aligner::gather_text(Summary& sum, const std::vector<Fetched>& fetched, const std::vector<wflign::BiwfaRecord>& recs) {
  std::string out;
  for (size_t k = 0; k < recs.size(); ++k) {
    sum.records++;
    sum.records_resident += recs[k].target_seq >= 0 && recs[k].query_seq >= 0;
    sum.aligned_bp += (uint64_t)(fetched[k].row.qEndPos - fetched[k].row.qStartPos);
    if (recs[k].paf.empty()) continue;
    // PAF: the record is already in the form processMappingRecord gives it (fields re-joined with single tabs,
    // computeAlignments.hpp:484-525); SAM: no cg:Z: field -> the writer's line passes through unchanged
    out += recs[k].paf;
    sum.written++;
  }
  return out;
}

std::string Aligner::align_batch(wfm_handle_t* gpu_handle, std::vector<std::string>& lines, int threads, Summary& sum, uint64_t first_row,
                                 std::string* vcf, wfm_coverage_t* coverage, const std::vector<uint64_t>* seq_offsets, std::string* lift,
                                 const wfm_liftset_t* liftset, const std::vector<lift::Interval>* lift_intervals, wfm_pav_t* pav,
                                 const std::vector<uint32_t>* pav_columns, std::string* chain, bool chain_swap, wfm_sites_t* sites,
                                 uint32_t sites_groups, wfm_net_t* net, uint64_t net_batch, std::vector<wflign::NetHead>* net_heads, wfm_trans_t* trans,
                                 const std::vector<uint64_t>* query_world) {
  const bool dbg = getenv("WFM_DEBUG") != nullptr;
  BatchTimes t;
  std::vector<Fetched> rows = parse_rows(lines, first_row, sum);
  t.rows = t.lap();
  DeviceStore* ds = param.resident_sequences ? device_store(gpu_handle) : nullptr;
  if (ds) assign_resident_ids(gpu_handle, *ds, rows);
  std::vector<Fetched> fetched = fetch_eager(rows, threads, sum);
  if (fetched.empty()) return std::string();
  std::vector<wflign::BiwfaRecord> recs = make_records(fetched);
  if (coverage || liftset || pav || sites || net || trans)
    for (wflign::BiwfaRecord& r : recs) r.target_global = (*seq_offsets)[(size_t)ref->find(r.target_name)];  // (parse_rows has found every name)
  if (pav || sites)
    for (wflign::BiwfaRecord& r : recs) {
      const int qi = query->find(r.query_name);
      r.pav_group = qi >= 0 ? (*pav_columns)[(size_t)qi] : 0xffffffffu;  // (no column: the device flags the record and adds nothing)
    }
  if (trans)
    for (wflign::BiwfaRecord& r : recs) r.query_global = (*query_world)[(size_t)query->find(r.query_name)];  // (parse_rows has found every name)
  wflign::ResidentSeqs resident;
  if (ds) {
    resident.store = ds->store;
    // (from the pipeline's worker threads, one record each: exactly the eager fetch)
    resident.fetch = [&](size_t k) {
      try {
        fetch_windows(fetched[k]);
        point_at(recs[k], fetched[k]);
      } catch (const std::exception& e) {
        std::cerr << "[wfmash::align] Error fetching the bases of a record: " << e.what() << std::endl;
      }
    };
  }
  t.fetch = t.lap();
  wflign::BiwfaStats st;
  wflign::OutputFormat fmt = format_of(param, threads);
  fmt.coverage = coverage;
  fmt.pav = pav;
  fmt.sites = sites;
  fmt.sites_groups = sites_groups;
  fmt.liftset = liftset;
  fmt.lift_intervals = lift_intervals;
  fmt.chain = chain ? (chain_swap ? 2 : 1) : 0;
  fmt.net = net;
  fmt.net_batch = net_batch;
  fmt.net_heads = net_heads;
  fmt.trans = trans;
  const int rc = wflign::do_biwfa_alignment_batch(gpu_handle, recs, penalties_of(param), param.disable_chain_patching, filters_of(param), &st,
                                                  fmt, ds ? &resident : nullptr);
  if (rc < 0) throw std::runtime_error(std::string("[wfmash::align] GPU alignment failed: ") + st.error);
  account(sum, st, resident, fetched, recs);
  t.wflign = t.lap();
  std::string out = gather_text(sum, fetched, recs);
  if (vcf)
    for (const auto& r : recs) *vcf += r.vcf;  // (a record without a line has no VCF lines: write_record)
  if (lift)
    for (const auto& r : recs) *lift += r.lift;  // (in the order of the records' lines: gather_text's)
  if (chain)
    for (const auto& r : recs) *chain += r.chain;  // (likewise; the ids are the writer's)
  t.text = t.lap();
  if (verify::enabled() && !param.sam_format) {  // --verify: the finished lines, before they are written (SAM records carry no =/X CIGAR)
    verify::Source src;
    src.target = ref.get(); src.query = query; src.threads = threads;
    if (ds) {
      src.store = ds->store;
      src.resident_id = [&](const wfmash_host::FastaStore* fa, int idx) { return resident_id(gpu_handle, *ds, fa, idx); };
    }
    verify::Counts vc;
    verify::verify_text(gpu_handle, src, out, vc);
    verify::add_counts(vc);
    if (dbg) fprintf(stderr, "[wfmash::align] verify: %llu lines, %llu failed, %.1f ms\n", (unsigned long long)vc.checked, (unsigned long long)vc.failed, t.lap());
  }
  sum.ms_rows += t.rows; sum.ms_fetch += t.fetch; sum.ms_wflign += t.wflign; sum.ms_text += t.text; sum.batches++;
  if (dbg)
    fprintf(stderr, "[wfmash::align] batch of %zu records on %d threads: rows %.1f ms, fetch %.1f ms, wflign %.1f ms (device busy %.1f), text %.1f ms\n",
            recs.size(), threads, t.rows, t.fetch, t.wflign, st.ms_gpu, t.text);
  return out;
}

std::string Aligner::align_lines(const std::vector<std::string>& lines, Summary& sum) {
  std::string out;
  size_t i = 0;
  while (i < lines.size()) {
    std::vector<std::string> batch;
    uint64_t bases = 0;
    while (i < lines.size() && batch.size() < param.batch_records && bases < param.batch_bases) {
      bases += row_bases(lines[i]);
      batch.push_back(lines[i++]);
    }
    const uint64_t first_row = i - batch.size();
    out += align_batch(gpus.front(), batch, param.threads, sum, first_row);
  }
  return out;
}

// ---------------------------------------------------------------------------
// The reference streams records from a reader through a pool of workers to a writer
// (computeAlignments.hpp:318-455).  Here the reader hands out batches of mapping rows, one worker per GPU
// takes the next batch whenever its device is free (the greedy least-loaded assignment of
// scripts/split_approx_mappings_in_chunks.py:19-27,47, taken at run time instead of from predicted weights),
// and finished batches are written in the order they were read: the output does not depend on the number of
// GPUs, and host memory holds the batches in flight, not the run.
// ---------------------------------------------------------------------------
namespace {
// Every worker beyond the first of a device works on a handle of its own (own stream, own arenas): its batch's device
// calls then really run beside the other workers' -- the few-workgroup tails of one batch (the patches that overflow
// their score budget, the last leaves) under the wide levels of another -- instead of taking turns on one handle.
// The extra handles stay with the process (two per device at most, or a worker's number less one) and serve the next run as
// well: their arenas are what a first use pays for, and a handle given back to the driver costs the next hipMalloc its scrubbing.
class HandlePool {
 public:
  // what one run has borrowed: given back when it goes out of scope
  class Loan {
   public:
    explicit Loan(HandlePool& p) : pool_(p) {}
    Loan(const Loan&) = delete;
    Loan& operator=(const Loan&) = delete;
    ~Loan() {
      std::lock_guard<std::mutex> lk(pool_.mu_);
      for (auto& x : borrowed_) pool_.by_device_[x.first][(size_t)x.second].second = false;
    }
    // a free handle of the device, or a new one while the device would then have fewer than `limit`; null: none is to be had
    wfm_handle_t* borrow(int dev, size_t limit) {
      std::lock_guard<std::mutex> lk(pool_.mu_);
      auto& v = pool_.by_device_[dev];
      int slot = -1;
      for (size_t q = 0; q < v.size(); ++q) if (!v[q].second) { slot = (int)q; break; }
      if (slot < 0 && v.size() + 1 < limit) {
        wfm_handle_t* nh = nullptr;
        if (wfm_create(dev, &nh) == WFM_OK) { v.emplace_back(nh, false); slot = (int)v.size() - 1; }
      }
      if (slot < 0) return nullptr;
      v[(size_t)slot].second = true;
      borrowed_.emplace_back(dev, slot);
      return v[(size_t)slot].first;
    }

   private:
    HandlePool& pool_;
    std::vector<std::pair<int, int>> borrowed_;  // (device, slot)
  };

 private:
  std::mutex mu_;
  std::map<int, std::vector<std::pair<wfm_handle_t*, bool>>> by_device_;  // handle, in use
};

// the ordered writer's sink: the output file, flushed once per put
struct TextSink {
  std::ofstream* out;
  void write(std::string& text) { *out << text; }
  void flush() { out->flush(); }
};
// --chain: the chains of a batch come without their ids; the writer numbers them 1, 2, 3 ... as it writes them, in file order
struct ChainSink {
  std::ofstream* out;
  uint64_t next = 1;
  std::string numbered;
  void write(std::string& text) {
    numbered.clear();
    chain::number(text, &next, numbered);
    *out << numbered;
  }
  void flush() { out->flush(); }
};
}  // namespace

struct Aligner::Run {
  Run(const Parameters& p, const RunPlan& pl, size_t n_gpu, Clock::time_point start, std::ifstream& i, std::ofstream& o)
      : param(p), plan(pl), ngpu(n_gpu), t0(start), in(i), writer(TextSink{&o}), in_flight(n_gpu), first_taken(n_gpu), use(pl.nworkers, nullptr),
        part(pl.nworkers), threads_each(std::max(1, p.threads / (int)pl.nworkers)) {
    for (auto& a : in_flight) a.store(0);
    for (auto& a : first_taken) a.store(0);
  }
  const Parameters& param;
  const RunPlan plan;
  const size_t ngpu;
  const Clock::time_point t0;
  std::ifstream& in;
  skch::OrderedWriter<std::string, TextSink> writer;
  std::unique_ptr<skch::OrderedWriter<std::string, TextSink>> vcf_writer;  // --variants: the second file, keyed by the same batch numbers
  // --lift: the third file, keyed by the same batch numbers; the BED's intervals sorted as the device takes them, and the liftset of every
  // handle the run has used so far, made at the handle's first batch
  std::unique_ptr<skch::OrderedWriter<std::string, TextSink>> lift_writer;
  std::vector<lift::Interval> lift_iv;
  std::mutex lift_mu;
  std::vector<std::pair<wfm_handle_t*, wfm_liftset_t*>> liftsets;
  const wfm_liftset_t* liftset_of(wfm_handle_t* h) {
    if (!lift_writer) return nullptr;
    std::lock_guard<std::mutex> lk(lift_mu);
    for (auto& hs : liftsets) if (hs.first == h) return hs.second;
    std::vector<wfm_lift_iv_t> raw(lift_iv.size());
    for (size_t i = 0; i < raw.size(); ++i) raw[i] = wfm_lift_iv_t{lift_iv[i].gstart, lift_iv[i].gend};
    wfm_liftset_t* s = nullptr;
    std::lock_guard<std::mutex> hl(wflign::handle_lock(h));
    if (wfm_liftset_create(h, raw.data(), raw.size(), seq_offsets.back(), &s) != WFM_OK) throw std::runtime_error(std::string("[wfmash::align] --lift: ") + wfm_last_error(h));
    liftsets.emplace_back(h, s);
    return s;
  }
  // --chain: the fourth file, keyed by the same batch numbers
  std::unique_ptr<skch::OrderedWriter<std::string, ChainSink>> chain_writer;
  bool chain_swap = false;
  // --pav: the intervals of the table in the file's order, the columns (and every query sequence's), and the presence object of every
  // handle the run has used so far, made at the handle's first batch
  bool pav_on = false;
  std::vector<lift::Interval> pav_iv;
  pav::Columns pav_cols;
  std::mutex pav_mu;
  std::vector<std::pair<wfm_handle_t*, wfm_pav_t*>> pavs;
  wfm_pav_t* pav_of(wfm_handle_t* h) {
    if (!pav_on) return nullptr;
    std::lock_guard<std::mutex> lk(pav_mu);
    for (auto& hp : pavs) if (hp.first == h) return hp.second;
    wfm_pav_t* p = nullptr;
    std::lock_guard<std::mutex> hl(wflign::handle_lock(h));
    if (wfm_pav_create(h, seq_offsets.back(), (uint32_t)pav_cols.keys.size(), &p) != WFM_OK) throw std::runtime_error(std::string("[wfmash::align] --pav: ") + wfm_last_error(h));
    pavs.emplace_back(h, p);
    return p;
  }
  // --genotypes: the columns (pav_cols, as --pav makes them) and the sites object of every handle the run has used so far, made at the
  // handle's first batch
  bool sites_on = false;
  std::mutex sites_mu;
  std::vector<std::pair<wfm_handle_t*, wfm_sites_t*>> sites;
  wfm_sites_t* sites_of(wfm_handle_t* h) {
    if (!sites_on) return nullptr;
    std::lock_guard<std::mutex> lk(sites_mu);
    for (auto& hs : sites) if (hs.first == h) return hs.second;
    wfm_sites_t* p = nullptr;
    std::lock_guard<std::mutex> hl(wflign::handle_lock(h));
    if (wfm_sites_create(h, seq_offsets.back(), (uint32_t)pav_cols.keys.size(), &p) != WFM_OK) throw std::runtime_error(std::string("[wfmash::align] --genotypes: ") + wfm_last_error(h));
    sites.emplace_back(h, p);
    return p;
  }
  // --chain-net: the net object of every handle the run has used so far, made at the handle's first batch, and what the chains' headers
  // need of every record added, in no order (finish_chain_net sorts them by their orders)
  bool net_on = false;
  std::mutex net_mu;
  std::vector<std::pair<wfm_handle_t*, wfm_net_t*>> nets;
  std::vector<wflign::NetHead> net_heads;
  wfm_net_t* net_of(wfm_handle_t* h) {
    if (!net_on) return nullptr;
    std::lock_guard<std::mutex> lk(net_mu);
    for (auto& hn : nets) if (hn.first == h) return hn.second;
    wfm_net_t* p = nullptr;
    std::lock_guard<std::mutex> hl(wflign::handle_lock(h));
    if (wfm_net_create(h, seq_offsets.back(), &p) != WFM_OK) throw std::runtime_error(std::string("[wfmash::align] --chain-net: ") + wfm_last_error(h));
    nets.emplace_back(h, p);
    return p;
  }
  // --transitive: the world, the seeds in input order, where each query sequence begins in the world, the depth, and the trans object of
  // every handle the run has used so far, made at the handle's first batch
  bool trans_on = false;
  transitive::World world;
  lift::Bed trans_seeds;
  std::vector<uint64_t> query_world;
  uint32_t trans_depth = 2;
  std::mutex trans_mu;
  std::vector<std::pair<wfm_handle_t*, wfm_trans_t*>> trans;
  wfm_trans_t* trans_of(wfm_handle_t* h) {
    if (!trans_on) return nullptr;
    std::lock_guard<std::mutex> lk(trans_mu);
    for (auto& ht : trans) if (ht.first == h) return ht.second;
    wfm_trans_t* p = nullptr;
    std::lock_guard<std::mutex> hl(wflign::handle_lock(h));
    if (wfm_trans_create(h, world.n_bases(), &p) != WFM_OK) throw std::runtime_error(std::string("[wfmash::align] --transitive: ") + wfm_last_error(h));
    trans.emplace_back(h, p);
    return p;
  }
  // --coverage, --lift, --pav, --genotypes, --chain-net: where each target sequence begins in the concatenation (nseq + 1 values; empty: all are off).  --coverage: the depth object
  // of every handle the run has used so far, made at the handle's first batch
  std::vector<uint64_t> seq_offsets;
  bool coverage_on = false;
  std::mutex coverage_mu;
  std::vector<std::pair<wfm_handle_t*, wfm_coverage_t*>> coverage;
  ~Run() {
    for (auto& hc : coverage) {
      std::lock_guard<std::mutex> lk(wflign::handle_lock(hc.first));
      wfm_coverage_free(hc.second);
    }
    for (auto& hs : liftsets) {
      std::lock_guard<std::mutex> lk(wflign::handle_lock(hs.first));
      wfm_liftset_free(hs.second);
    }
    for (auto& hp : pavs) {
      std::lock_guard<std::mutex> lk(wflign::handle_lock(hp.first));
      wfm_pav_free(hp.second);
    }
    for (auto& hs : sites) {
      std::lock_guard<std::mutex> lk(wflign::handle_lock(hs.first));
      wfm_sites_free(hs.second);
    }
    for (auto& hn : nets) {
      std::lock_guard<std::mutex> lk(wflign::handle_lock(hn.first));
      wfm_net_free(hn.second);
    }
    for (auto& ht : trans) {
      std::lock_guard<std::mutex> lk(wflign::handle_lock(ht.first));
      wfm_trans_free(ht.second);
    }
  }
  wfm_coverage_t* coverage_of(wfm_handle_t* h) {
    if (!coverage_on) return nullptr;
    std::lock_guard<std::mutex> lk(coverage_mu);
    for (auto& hc : coverage) if (hc.first == h) return hc.second;
    wfm_coverage_t* c = nullptr;
    std::lock_guard<std::mutex> hl(wflign::handle_lock(h));
    if (wfm_coverage_create(h, seq_offsets.back(), &c) != WFM_OK) throw std::runtime_error(std::string("[wfmash::align] --coverage: ") + wfm_last_error(h));
    coverage.emplace_back(h, c);
    return c;
  }
  std::mutex read_mu;
  uint64_t next_seq = 0;   // (under read_mu) the next batch's number
  uint64_t rows_read = 0;  // (under read_mu) non-empty rows handed out so far
  bool more_rows = true;   // (under read_mu) rows are left behind the batch handed out last
  std::vector<std::atomic<int>> in_flight;    // batches on the device right now, per device
  std::vector<std::atomic<int>> first_taken;  // the device's first batch has been handed out (or there is none)
  std::mutex error_mu;
  std::string first_error;
  std::atomic<bool> failed{false};
  std::vector<wfm_handle_t*> use;  // the handle of each worker
  std::vector<Summary> part;
  const int threads_each;

  double ms() const { return ms_since(t0); }
  // the next batch's number, or -1 at the end
  int64_t read_batch(std::vector<std::string>& batch, uint64_t& first_row) {
    std::lock_guard<std::mutex> lk(read_mu);
    batch.clear();
    first_row = rows_read;
    uint64_t bases = 0, bytes = 0;
    std::string line;
    while (batch.size() < param.batch_records && bases < param.batch_bases && bytes < plan.batch_bytes && std::getline(in, line)) {
      if (line.empty()) continue;
      bases += row_bases(line);
      bytes += line.size() + 1;
      batch.push_back(std::move(line));
    }
    rows_read += batch.size();
    more_rows = !batch.empty() && in.peek() != std::char_traits<char>::eof();
    return batch.empty() ? -1 : (int64_t)next_seq++;
  }
};

// Workers and batch size from the host's threads, the file's size and its first rows (unknown for a stream).
Aligner::RunPlan Aligner::plan_run(std::ifstream& in) const {
  const size_t ngpu = gpus.size();
  static const size_t workers_env = getenv("WFM_ALIGN_WORKERS") ? (size_t)std::max(1, atoi(getenv("WFM_ALIGN_WORKERS"))) : 0;  // A/B runs
  static const uint64_t min_batches = getenv("WFM_ALIGN_MIN_BATCHES") ? (uint64_t)std::max(1, atoi(getenv("WFM_ALIGN_MIN_BATCHES"))) : 1;
  static const bool level_batches = !(getenv("WFM_ALIGN_LEVEL") && atoi(getenv("WFM_ALIGN_LEVEL")) == 0);
  RunPlan plan;
  plan.per_gpu = workers_per_gpu((size_t)param.threads, ngpu, workers_env);
  const size_t nworkers_max = ngpu * plan.per_gpu;
  // (a mapping file that cannot be rewound -- a FIFO, /dev/stdin -- is read as it comes: no size, no look ahead)
  in.seekg(0, std::ios::end);
  const std::streamoff end_at = in.fail() ? (std::streamoff)-1 : (std::streamoff)in.tellg();
  in.clear();
  if (end_at >= 0) in.seekg(0, std::ios::beg);
  const bool seekable = end_at >= 0 && !in.fail();
  in.clear();
  const uint64_t file_bytes = seekable ? (uint64_t)end_at : 0;
  uint64_t rows = 0, bytes = 0, bases = 0;
  if (level_batches && nworkers_max > 1 && file_bytes > 0) {
    std::string line;
    while (rows < 256 && std::getline(in, line)) {
      if (line.empty()) continue;
      ++rows; bytes += line.size() + 1; bases += row_bases(line);
    }
    in.clear();
    in.seekg(0, std::ios::beg);
  }
  plan.batch_bytes = plan_batch_bytes(file_bytes, rows, bytes, bases, param.batch_records, param.batch_bases, nworkers_max, ngpu, min_batches, level_batches);
  // (no more workers than the file has batches: a worker beyond the first of a device brings a handle with arenas of its own, and the host threads are shared
  // out over the workers -- a mapping file of one batch keeps them all)
  const uint64_t est_batches = estimate_batches(file_bytes, rows, bytes, bases, param.batch_records, param.batch_bases, plan.batch_bytes);
  plan.nworkers = (size_t)std::max<uint64_t>(ngpu, std::min<uint64_t>(nworkers_max, est_batches));
  return plan;
}

void Aligner::run_worker(Run& run, size_t wk) {
  const size_t dev = wk % run.ngpu;
  try {
    std::vector<std::string> batch;
    // (the first batch of a device goes to its first worker, the one on the caller's handle: a file of one batch then runs
    // on arenas that are most likely there already)
    if (wk >= run.ngpu) while (!run.first_taken[dev].load() && !run.failed.load()) std::this_thread::yield();
    uint64_t first_row = 0;
    for (int64_t seq; !run.failed.load() && (seq = run.read_batch(batch, first_row)) >= 0;) {
      run.first_taken[dev].store(1);
      const double at0 = run.ms();
      // a batch that has its device to itself -- none beside it, none to come -- is cut into parts by the device layer
      // (wfm_set_concurrent_calls: its levels are chains of short launches, and one chain does not fill a device)
      // (both under the readers' lock: two workers that start together must not each see the device as theirs alone)
      bool more;
      int beside;
      { std::lock_guard<std::mutex> lk(run.read_mu); more = run.more_rows; beside = run.in_flight[dev].fetch_add(1); }
      wfm_set_concurrent_calls(run.use[wk], beside + (more && run.plan.per_gpu > 1 ? 1 : 0));
      struct Leave { std::atomic<int>& a; ~Leave() { a.fetch_sub(1); } } leave{run.in_flight[dev]};
      std::string vcf, lifted, chains;
      std::vector<wflign::NetHead> heads;
      std::string text = align_batch(run.use[wk], batch, run.threads_each, run.part[wk], first_row, run.vcf_writer ? &vcf : nullptr,
                                     run.coverage_of(run.use[wk]), &run.seq_offsets, run.lift_writer ? &lifted : nullptr, run.liftset_of(run.use[wk]),
                                     &run.lift_iv, run.pav_of(run.use[wk]), &run.pav_cols.of_seq, run.chain_writer ? &chains : nullptr, run.chain_swap,
                                     run.sites_of(run.use[wk]), (uint32_t)run.pav_cols.keys.size(), run.net_of(run.use[wk]), (uint64_t)seq, &heads,
                                     run.trans_of(run.use[wk]), &run.query_world);
      if (!heads.empty()) {
        std::lock_guard<std::mutex> lk(run.net_mu);
        for (auto& hd : heads) run.net_heads.push_back(std::move(hd));
      }
      const double at1 = run.ms();
      run.writer.put((uint64_t)seq, std::move(text));
      if (run.vcf_writer) run.vcf_writer->put((uint64_t)seq, std::move(vcf));
      if (run.lift_writer) run.lift_writer->put((uint64_t)seq, std::move(lifted));
      if (run.chain_writer) run.chain_writer->put((uint64_t)seq, std::move(chains));
      if (getenv("WFM_DEBUG"))
        fprintf(stderr, "[wfmash::align] worker %zu: batch %lld from +%.0f ms to +%.0f ms, written at +%.0f ms\n", wk, (long long)seq, at0, at1, run.ms());
    }
  } catch (const std::exception& e) {
    std::lock_guard<std::mutex> lk(run.error_mu);
    if (run.first_error.empty()) run.first_error = e.what();
    run.failed.store(true);
  }
  run.first_taken[dev].store(1);  // (nothing left for this device's first worker either: the others must not wait)
}

// the workers' parts into the run's summary; per device, the time during which a kernel of any of its workers' calls was
// running (their calls overlap)
void Aligner::sum_up(Summary& sum, const std::vector<Summary>& part, std::chrono::steady_clock::time_point t0) const {
  const size_t ngpu = gpus.size();
  std::vector<std::vector<Interval>> iv(ngpu);
  for (size_t wk = 0; wk < part.size(); ++wk) {
    const Summary& p = part[wk];
    sum.records += p.records; sum.aligned_bp += p.aligned_bp; sum.written += p.written; sum.skipped += p.skipped;
    sum.cells += p.cells;
    sum.records_resident += p.records_resident; sum.lazy_fetches += p.lazy_fetches;
    sum.cells_tile += p.cells_tile; sum.tile_launches += p.tile_launches; sum.ms_tile += p.ms_tile; sum.ms_tags += p.ms_tags;
    sum.ms_rows += p.ms_rows; sum.ms_fetch += p.ms_fetch; sum.ms_wflign += p.ms_wflign; sum.ms_text += p.ms_text; sum.batches += p.batches;
    iv[wk % ngpu].insert(iv[wk % ngpu].end(), p.busy.begin(), p.busy.end());
  }
  for (auto& v : iv) {
    const std::vector<Interval> busy = interval_union(v);
    const double total = total_length(busy);
    sum.ms_gpu = std::max(sum.ms_gpu, total);
    if (getenv("WFM_DEBUG") && !v.empty()) {
      // where the device had no kernel running: its busy share per twentieth of the span from its first kernel to its last (the intervals
      // are on the device's own clock; the run's wall time less that span is the head before the first kernel plus the tail after the last)
      const double wall = ms_since(t0);
      const double d_lo = span_of(v).first, span = span_of(v).second;
      const std::vector<double> busy20 = covered_per_bin(busy, d_lo, span, 20);
      fprintf(stderr, "[wfmash::align] device: first kernel to last %.1f ms of the run's %.1f (head + tail %.1f), busy %.1f; busy share per twentieth of that span:", span, wall, wall - span, total);
      for (int q = 0; q < 20; ++q) fprintf(stderr, " %.2f", busy20[(size_t)q] / (span / 20));
      fprintf(stderr, "\n");
    }
  }
  // (a worker's own calls follow one another: the sum of their busy times is a lower bound of its device's)
  for (const Summary& p : part) sum.ms_gpu = std::max(sum.ms_gpu, p.ms_gpu);
}

// --coverage: every other handle's object exported and imported into the first (integer adds: the order does not matter), the intervals of
// the sum taken once on the device, the file through coverage_bedgraph
void Aligner::finish_coverage(Run& run, std::ofstream& out) {
  const auto t0 = Clock::now();
  auto fail = [](wfm_handle_t* h, const char* what) { throw std::runtime_error(std::string("[wfmash::align] --coverage: ") + what + ": " + wfm_last_error(h)); };
  std::vector<coverage::Interval> iv;
  uint64_t totals[3] = {0, 0, 0};
  if (!run.coverage.empty()) {
    wfm_handle_t* h0 = run.coverage.front().first;
    wfm_coverage_t* c0 = run.coverage.front().second;
    for (size_t k = 1; k < run.coverage.size(); ++k) {
      wfm_cov_entry_t* list = nullptr;
      size_t n = 0;
      {
        std::lock_guard<std::mutex> lk(wflign::handle_lock(run.coverage[k].first));
        if (wfm_coverage_export(run.coverage[k].first, run.coverage[k].second, &list, &n) != WFM_OK) fail(run.coverage[k].first, "export");
      }
      std::lock_guard<std::mutex> lk(wflign::handle_lock(h0));
      const int rc = wfm_coverage_import(h0, c0, list, n);
      wfm_coverage_free_list(list);
      if (rc != WFM_OK) fail(h0, "import");
    }
    wfm_cov_interval_t* d_iv = nullptr;
    size_t n = 0;
    std::lock_guard<std::mutex> lk(wflign::handle_lock(h0));
    if (wfm_coverage_intervals(h0, c0, &d_iv, &n, totals) != WFM_OK) fail(h0, "intervals");
    iv.resize(n);
    for (size_t i = 0; i < n; ++i) iv[i] = coverage::Interval{d_iv[i].start, d_iv[i].depth};
    wfm_coverage_free_list(d_iv);
  }
  std::vector<std::string> names;
  std::vector<uint64_t> lengths;
  for (int i = 0; i < ref->nseq(); ++i) { names.push_back(ref->name(i)); lengths.push_back((uint64_t)ref->length(i)); }
  uint64_t lines = 0;
  out << coverage::coverage_bedgraph(names, lengths, iv, &lines);
  wflign::coverage_finished(totals[0], totals[1], lines);
  if (getenv("WFM_DEBUG"))
    fprintf(stderr, "[wfmash::align] coverage: %zu objects merged, %zu intervals, %llu lines, %.1f ms\n", run.coverage.size(), iv.size(), (unsigned long long)lines, ms_since(t0));
}

// --pav: every other handle's object exported and imported into the first (a union of unions: the order does not matter), the table of
// the merged object taken once on the device, the file through pav_text.hpp
void Aligner::finish_pav(Run& run, std::ofstream& out, uint64_t bed_skipped) {
  const auto t0 = Clock::now();
  auto fail = [](wfm_handle_t* h, const char* what) { throw std::runtime_error(std::string("[wfmash::align] --pav: ") + what + ": " + wfm_last_error(h)); };
  const size_t G = run.pav_cols.keys.size(), n_iv = run.pav_iv.size();
  std::vector<uint32_t> cells(G * n_iv, 0u);
  uint64_t counts[3] = {0, 0, 0};
  if (!run.pavs.empty()) {
    wfm_handle_t* h0 = run.pavs.front().first;
    wfm_pav_t* p0 = run.pavs.front().second;
    for (size_t k = 1; k < run.pavs.size(); ++k) {
      wfm_pav_seg_t* list = nullptr;
      size_t n = 0;
      {
        std::lock_guard<std::mutex> lk(wflign::handle_lock(run.pavs[k].first));
        if (wfm_pav_export(run.pavs[k].first, run.pavs[k].second, &list, &n) != WFM_OK) fail(run.pavs[k].first, "export");
      }
      std::lock_guard<std::mutex> lk(wflign::handle_lock(h0));
      const int rc = wfm_pav_import(h0, p0, list, n);
      wfm_pav_free_list(list);
      if (rc != WFM_OK) fail(h0, "import");
    }
    std::vector<wfm_lift_iv_t> raw(n_iv);
    for (size_t j = 0; j < n_iv; ++j) raw[j] = wfm_lift_iv_t{run.pav_iv[j].gstart, run.pav_iv[j].gend};
    std::lock_guard<std::mutex> lk(wflign::handle_lock(h0));
    if (wfm_pav_matrix(h0, p0, raw.data(), n_iv, cells.data()) != WFM_OK) fail(h0, "matrix");
    wfm_pav_counts(p0, counts);
  }
  const auto t1 = Clock::now();
  std::string text = pav::header(run.pav_cols.keys);
  for (size_t j = 0; j < n_iv; ++j) {
    pav::row(text, ref->name(run.pav_iv[j].seq), run.pav_iv[j], cells.data() + j * G, G);
    if (text.size() >= ((size_t)1 << 20)) { out << text; text.clear(); }
  }
  out << text;
  wflign::pav_finished(n_iv, counts[1], bed_skipped);
  if (getenv("WFM_DEBUG"))
    fprintf(stderr, "[wfmash::align] pav: %zu objects merged, %llu segments added, %llu union intervals, %zu rows x %zu groups, merge + union + matrix %.1f ms, text %.1f ms\n",
            run.pavs.size(), (unsigned long long)counts[0], (unsigned long long)counts[1], n_iv, G, std::chrono::duration<double, std::milli>(t1 - t0).count(), ms_since(t1));
}

// --genotypes: every other handle's object exported and imported into the first (the table is a set function: the order does not matter),
// the table of the merged object taken once on the device, the file through genotype_text.hpp
void Aligner::finish_genotypes(Run& run, std::ofstream& out) {
  const auto t0 = Clock::now();
  auto fail = [](wfm_handle_t* h, const char* what) { throw std::runtime_error(std::string("[wfmash::align] --genotypes: ") + what + ": " + wfm_last_error(h)); };
  const size_t G = run.pav_cols.keys.size();
  wfm_site_t* rows = nullptr;
  char *alleles = nullptr, *gt = nullptr;
  size_t n_sites = 0, bytes = 0;
  uint64_t counts[4] = {0, 0, 0, 0};
  if (!run.sites.empty()) {
    wfm_handle_t* h0 = run.sites.front().first;
    wfm_sites_t* s0 = run.sites.front().second;
    for (size_t k = 1; k < run.sites.size(); ++k) {
      wfm_site_var_t* vars = nullptr;
      char* a = nullptr;
      wfm_pav_seg_t* segs = nullptr;
      size_t n = 0, nb = 0, ns = 0;
      {
        std::lock_guard<std::mutex> lk(wflign::handle_lock(run.sites[k].first));
        if (wfm_sites_export(run.sites[k].first, run.sites[k].second, &vars, &n, &a, &nb, &segs, &ns) != WFM_OK) fail(run.sites[k].first, "export");
      }
      std::lock_guard<std::mutex> lk(wflign::handle_lock(h0));
      const int rc = wfm_sites_import(h0, s0, vars, n, a, nb, segs, ns);
      wfm_sites_free_list(vars); wfm_sites_free_list(a); wfm_sites_free_list(segs);
      if (rc != WFM_OK) fail(h0, "import");
    }
    std::lock_guard<std::mutex> lk(wflign::handle_lock(h0));
    if (wfm_sites_table(h0, s0, &rows, &n_sites, &alleles, &bytes, &gt) != WFM_OK) fail(h0, "table");
    wfm_sites_counts(s0, counts);
  }
  const auto t1 = Clock::now();
  std::vector<std::string> names;
  std::vector<uint64_t> lengths;
  for (int i = 0; i < ref->nseq(); ++i) { names.push_back(ref->name(i)); lengths.push_back((uint64_t)ref->length(i)); }
  std::vector<genotype::Site> sites(n_sites);
  for (size_t i = 0; i < n_sites; ++i) sites[i] = genotype::Site{rows[i].pos, rows[i].ref_len, rows[i].alt_len, rows[i].off};
  std::string text = genotype::header(WFMASH_HIP_VERSION, names, lengths, run.pav_cols.keys);
  for (size_t i : genotype::order(sites, alleles)) {
    genotype::site_line(text, sites, i, alleles, gt, G, names, run.seq_offsets);
    if (text.size() >= ((size_t)1 << 20)) { out << text; text.clear(); }
  }
  out << text;
  wfm_sites_free_list(rows); wfm_sites_free_list(alleles); wfm_sites_free_list(gt);
  wflign::genotypes_finished(counts[0], n_sites);
  if (getenv("WFM_DEBUG"))
    fprintf(stderr, "[wfmash::align] genotypes: %zu objects merged, %llu variants, %zu sites x %zu groups, %llu = intervals, merge + table %.1f ms, text %.1f ms\n",
            run.sites.size(), (unsigned long long)counts[0], n_sites, G, (unsigned long long)counts[2], std::chrono::duration<double, std::milli>(t1 - t0).count(), ms_since(t1));
}

// --chain-net: every other handle's object exported and imported into the first (the net is a set function: the order does not matter),
// the table of the merged object taken once on the device, the file through chain_text.hpp's net_body in the order of the orders, which
// is the order of the PAF's records
void Aligner::finish_chain_net(Run& run, std::ofstream& out) {
  const auto t0 = Clock::now();
  auto fail = [](wfm_handle_t* h, const char* what) { throw std::runtime_error(std::string("[wfmash::align] --chain-net: ") + what + ": " + wfm_last_error(h)); };
  wfm_net_piece_t* pieces = nullptr;
  wfm_netcall_t* per = nullptr;
  size_t n_pieces = 0, n_rec = 0;
  uint64_t counts[6] = {0, 0, 0, 0, 0, 0};
  if (!run.nets.empty()) {
    wfm_handle_t* h0 = run.nets.front().first;
    wfm_net_t* n0 = run.nets.front().second;
    for (size_t k = 1; k < run.nets.size(); ++k) {
      wfm_net_block_t* blocks = nullptr;
      wfm_net_rec_t* recs = nullptr;
      size_t nb = 0, nr = 0;
      {
        std::lock_guard<std::mutex> lk(wflign::handle_lock(run.nets[k].first));
        if (wfm_net_export(run.nets[k].first, run.nets[k].second, &blocks, &nb, &recs, &nr) != WFM_OK) fail(run.nets[k].first, "export");
      }
      std::lock_guard<std::mutex> lk(wflign::handle_lock(h0));
      const int rc = wfm_net_import(h0, n0, blocks, nb, recs, nr);
      wfm_net_free_list(blocks); wfm_net_free_list(recs);
      if (rc != WFM_OK) fail(h0, "import");
    }
    std::lock_guard<std::mutex> lk(wflign::handle_lock(h0));
    if (wfm_net_table(h0, n0, &pieces, &n_pieces, &per, &n_rec) != WFM_OK) fail(h0, "table");
    wfm_net_counts(n0, counts);
  }
  const auto t1 = Clock::now();
  static_assert(sizeof(chain::Piece) == sizeof(wfm_net_piece_t), "chain_text.hpp restates wfm_net_piece_t");
  std::sort(run.net_heads.begin(), run.net_heads.end(), [](const wflign::NetHead& a, const wflign::NetHead& b) { return a.order < b.order; });
  if (run.net_heads.size() != n_rec) throw std::runtime_error("[wfmash::align] --chain-net: the table's records are not the records added");
  std::string body, text;
  uint64_t next = 1, chains = 0, lost = 0;
  for (size_t i = 0; i < n_rec; ++i) {  // (per is sorted by order too)
    const wflign::NetHead& hd = run.net_heads[i];
    if (hd.order != per[i].order) throw std::runtime_error("[wfmash::align] --chain-net: the table's records are not the records added");
    if (per[i].count == 0) { ++lost; continue; }
    chain::net_body(body, hd.rec, hd.t_offset, per[i].score, (const chain::Piece*)pieces + per[i].first, per[i].count);
    if (body.size() >= ((size_t)1 << 20)) { text.clear(); chains += chain::number(body, &next, text); out << text; body.clear(); }
  }
  text.clear();
  chains += chain::number(body, &next, text);
  out << text;
  wfm_net_free_list(pieces); wfm_net_free_list(per);
  wflign::chain_net_finished(chains, n_pieces, lost);
  if (getenv("WFM_DEBUG"))
    fprintf(stderr, "[wfmash::align] chain-net: %zu objects merged, %llu records, %llu blocks, %llu elementary intervals, %zu pieces, %llu chains, %llu records won nothing, merge + table %.1f ms, text %.1f ms\n",
            run.nets.size(), (unsigned long long)counts[0], (unsigned long long)counts[1], (unsigned long long)counts[2], n_pieces, (unsigned long long)chains,
            (unsigned long long)lost, std::chrono::duration<double, std::milli>(t1 - t0).count(), ms_since(t1));
}

// --transitive: every other handle's object exported and imported into the first (the closure is a set function: the order does not
// matter), the closure of the seeds taken once on the device, the file through transitive_text.hpp in the order of the BED's lines
void Aligner::finish_transitive(Run& run, std::ofstream& out) {
  const auto t0 = Clock::now();
  auto fail = [](wfm_handle_t* h, const char* what) { throw std::runtime_error(std::string("[wfmash::align] --transitive: ") + what + ": " + wfm_last_error(h)); };
  const std::vector<lift::Interval>& seeds = run.trans_seeds.iv;
  wfm_trans_iv_t* ivs = nullptr;
  size_t n_ivs = 0;
  std::vector<wfm_trans_seed_t> per(seeds.size());
  uint64_t counts[6] = {0, 0, 0, 0, 0, 0};
  if (!run.trans.empty() && !seeds.empty()) {
    wfm_handle_t* h0 = run.trans.front().first;
    wfm_trans_t* o0 = run.trans.front().second;
    for (size_t k = 1; k < run.trans.size(); ++k) {
      wfm_trans_rec_t* recs = nullptr;
      wfm_trans_word_t* words = nullptr;
      size_t nr = 0, nw = 0;
      {
        std::lock_guard<std::mutex> lk(wflign::handle_lock(run.trans[k].first));
        if (wfm_trans_export(run.trans[k].first, run.trans[k].second, &recs, &nr, &words, &nw) != WFM_OK) fail(run.trans[k].first, "export");
      }
      std::lock_guard<std::mutex> lk(wflign::handle_lock(h0));
      const int rc = wfm_trans_import(h0, o0, recs, nr, words, nw);
      wfm_trans_free_list(recs); wfm_trans_free_list(words);
      if (rc != WFM_OK) fail(h0, "import");
    }
    std::vector<wfm_lift_iv_t> raw(seeds.size());
    for (size_t i = 0; i < raw.size(); ++i) raw[i] = wfm_lift_iv_t{seeds[i].gstart, seeds[i].gend};
    std::lock_guard<std::mutex> lk(wflign::handle_lock(h0));
    if (wfm_trans_closure(h0, o0, raw.data(), raw.size(), run.trans_depth, &ivs, &n_ivs, per.data()) != WFM_OK) fail(h0, "closure");
    wfm_trans_counts(o0, counts);
  }
  const auto t1 = Clock::now();
  std::string text;
  uint64_t lines = 0;
  for (size_t i = 0; i < seeds.size(); ++i) {
    if (!ivs) lines += transitive::lines(text, run.world, seeds[i], seeds[i].gstart, seeds[i].gend);  // (no record was added: a seed reaches itself)
    else
      for (uint64_t k = per[i].first; k < per[i].first + per[i].count; ++k) lines += transitive::lines(text, run.world, seeds[i], ivs[k].start, ivs[k].end);
    if (text.size() >= ((size_t)1 << 20)) { out << text; text.clear(); }
  }
  out << text;
  wfm_trans_free_list(ivs);
  wflign::transitive_finished(lines, counts[3], run.trans_seeds.skipped);
  if (getenv("WFM_DEBUG"))
    fprintf(stderr, "[wfmash::align] transitive: %zu objects merged, %llu records, %llu prefix words, %zu seeds at depth %u, %llu rounds, %llu pairs, %zu intervals, %llu lines, merge + closure %.1f ms, text %.1f ms\n",
            run.trans.size(), (unsigned long long)counts[0], (unsigned long long)counts[1], seeds.size(), run.trans_depth, (unsigned long long)counts[3],
            (unsigned long long)counts[5], n_ivs, (unsigned long long)lines, std::chrono::duration<double, std::milli>(t1 - t0).count(), ms_since(t1));
}

Summary Aligner::compute() {
  Summary sum;
  const auto t0 = Clock::now();
  std::ifstream in(param.mashmapPafFile);
  if (!in.is_open()) throw std::runtime_error("[wfmash::align] Error! Failed to open input mapping file: " + param.mashmapPafFile);
  std::ofstream outstream(param.pafOutputFile);
  if (!outstream.is_open()) throw std::runtime_error("[wfmash::align] Error! Failed to open output file: " + param.pafOutputFile);
  if (param.sam_format) {  // write_sam_header (computeAlignments.hpp:725-736)
    for (int i = 0; i < ref->nseq(); ++i) outstream << "@SQ\tSN:" << ref->name(i) << "\tLN:" << ref->length(i) << "\n";
    outstream << "@PG\tID:wfmash\tPN:wfmash\tVN:" WFMASH_HIP_VERSION "\tCL:wfmash\n";
  }
  const size_t ngpu = gpus.size();
  Run run(param, plan_run(in), ngpu, t0, in, outstream);
  std::ofstream vcfstream;
  const std::string vcf_path = wflign::variants_path();
  if (!vcf_path.empty()) {  // --variants: the header here, the batches' lines through a second ordered writer
    vcfstream.open(vcf_path);
    if (!vcfstream.is_open()) throw std::runtime_error("[wfmash::align] Error! Failed to open the variants file: " + vcf_path);
    vcfstream << "##fileformat=VCFv4.2\n##source=wfmash-hip " WFMASH_HIP_VERSION "\n";
    for (int i = 0; i < ref->nseq(); ++i) vcfstream << "##contig=<ID=" << ref->name(i) << ",length=" << ref->length(i) << ">\n";
    vcfstream << "##INFO=<ID=QNAME,Number=1,Type=String,Description=\"Query sequence name\">\n"
                 "##INFO=<ID=QSTART,Number=1,Type=Integer,Description=\"Start of the query bases in ALT, 0-based, forward strand\">\n"
                 "##INFO=<ID=QEND,Number=1,Type=Integer,Description=\"End of the query bases in ALT, exclusive, forward strand\">\n"
                 "##INFO=<ID=QSTRAND,Number=1,Type=String,Description=\"Strand of the query in the alignment\">\n"
                 "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
    run.vcf_writer.reset(new skch::OrderedWriter<std::string, TextSink>(TextSink{&vcfstream}));
  }
  std::ofstream covstream;
  const std::string cov_path = wflign::coverage_path();
  if (!cov_path.empty()) {  // --coverage: the file is opened before anything is aligned, and written once the workers are done
    covstream.open(cov_path);
    if (!covstream.is_open()) throw std::runtime_error("[wfmash::align] Error! Failed to open the coverage file: " + cov_path);
    run.coverage_on = true;
  }
  std::ofstream liftstream;
  std::string lift_bed, lift_out;
  wflign::lift_paths(lift_bed, lift_out);
  std::ofstream chainstream;
  std::string chain_out;
  wflign::chain_path(chain_out, run.chain_swap);
  if (!chain_out.empty()) {  // --chain: the batches' chains go through a fourth ordered writer, which numbers them
    chainstream.open(chain_out);
    if (!chainstream.is_open()) throw std::runtime_error("[wfmash::align] Error! Failed to open the chain file: " + chain_out);
    run.chain_writer.reset(new skch::OrderedWriter<std::string, ChainSink>(ChainSink{&chainstream}));
  }
  std::ofstream netstream;
  const std::string net_out = wflign::chain_net_path();
  if (!net_out.empty()) {  // --chain-net: the file is opened before anything is aligned, and written once the workers are done
    netstream.open(net_out);
    if (!netstream.is_open()) throw std::runtime_error("[wfmash::align] Error! Failed to open the chain-net file: " + net_out);
    run.net_on = true;
  }
  std::ofstream transstream;
  std::string trans_bed, trans_out;
  wflign::transitive_paths(trans_bed, trans_out, run.trans_depth);
  std::ofstream pavstream;
  std::string pav_bed, pav_out;
  uint64_t pav_window = 0, pav_skipped = 0;
  wflign::pav_paths(pav_bed, pav_window, pav_out);
  std::ofstream gtstream;
  const std::string gt_path = wflign::genotypes_path();
  if (!cov_path.empty() || !lift_out.empty() || !pav_out.empty() || !gt_path.empty() || !net_out.empty() || !trans_out.empty()) {
    run.seq_offsets.assign(1, 0);
    for (int i = 0; i < ref->nseq(); ++i) run.seq_offsets.push_back(run.seq_offsets.back() + (uint64_t)ref->length(i));
  }
  if (!lift_out.empty()) {  // --lift: the BED is read once, here; the batches' lines go through a third ordered writer
    std::ifstream bed(lift_bed, std::ios::binary);
    if (!bed.is_open()) throw std::runtime_error("[wfmash::align] Error! Failed to open the BED file of --lift: " + lift_bed);
    const std::string text((std::istreambuf_iterator<char>(bed)), std::istreambuf_iterator<char>());
    std::vector<uint64_t> lengths;
    for (int i = 0; i < ref->nseq(); ++i) lengths.push_back((uint64_t)ref->length(i));
    lift::Bed parsed = lift::parse_bed(text, [&](const std::string& name) { return ref->find(name); }, lengths, run.seq_offsets);
    run.lift_iv = std::move(parsed.iv);
    wflign::lift_bed_read(parsed.skipped);
    liftstream.open(lift_out);
    if (!liftstream.is_open()) throw std::runtime_error("[wfmash::align] Error! Failed to open the lift file: " + lift_out);
    run.lift_writer.reset(new skch::OrderedWriter<std::string, TextSink>(TextSink{&liftstream}));
  }
  if (!trans_out.empty()) {  // --transitive: the world and the seeds are known before anything is aligned; the file is written once the workers are done
    std::vector<std::string> tnames, qnames;
    std::vector<uint64_t> tlengths, qlengths;
    for (int i = 0; i < ref->nseq(); ++i) { tnames.push_back(ref->name(i)); tlengths.push_back((uint64_t)ref->length(i)); }
    for (int i = 0; i < query->nseq(); ++i) { qnames.push_back(query->name(i)); qlengths.push_back((uint64_t)query->length(i)); }
    run.world = transitive::make_world(tnames, tlengths, qnames, qlengths);
    if (run.world.n_bases() >= ((uint64_t)1 << 40)) throw std::runtime_error("[wfmash::align] --transitive: the sequences hold 2^40 bases or more");
    for (const std::string& name : qnames) run.query_world.push_back(run.world.offsets[(size_t)run.world.find(name)]);
    std::ifstream bed(trans_bed, std::ios::binary);
    if (!bed.is_open()) throw std::runtime_error("[wfmash::align] Error! Failed to open the BED file of --transitive: " + trans_bed);
    const std::string text((std::istreambuf_iterator<char>(bed)), std::istreambuf_iterator<char>());
    run.trans_seeds = transitive::parse_seeds(text, run.world);
    if (run.trans_seeds.iv.size() >= ((size_t)1 << 24)) throw std::runtime_error("[wfmash::align] --transitive: the BED holds 2^24 seeds or more");
    transstream.open(trans_out);
    if (!transstream.is_open()) throw std::runtime_error("[wfmash::align] Error! Failed to open the transitive file: " + trans_out);
    run.trans_on = true;
  }
  if (!pav_out.empty()) {  // --pav: the intervals and the columns are known before anything is aligned; the file is written once the workers are done
    std::vector<uint64_t> lengths;
    for (int i = 0; i < ref->nseq(); ++i) lengths.push_back((uint64_t)ref->length(i));
    if (!pav_bed.empty()) {
      std::ifstream bed(pav_bed, std::ios::binary);
      if (!bed.is_open()) throw std::runtime_error("[wfmash::align] Error! Failed to open the BED file of --pav: " + pav_bed);
      const std::string text((std::istreambuf_iterator<char>(bed)), std::istreambuf_iterator<char>());
      lift::Bed parsed = lift::parse_bed(text, [&](const std::string& name) { return ref->find(name); }, lengths, run.seq_offsets);
      run.pav_iv = std::move(parsed.iv);
      pav_skipped = parsed.skipped;
    } else {
      run.pav_iv = pav::windows(lengths, run.seq_offsets, pav_window);
    }
    std::vector<std::string> qnames;
    for (int i = 0; i < query->nseq(); ++i) qnames.push_back(query->name(i));
    run.pav_cols = pav::columns(qnames);
    pavstream.open(pav_out);
    if (!pavstream.is_open()) throw std::runtime_error("[wfmash::align] Error! Failed to open the pav file: " + pav_out);
    run.pav_on = true;
  }
  if (!gt_path.empty()) {  // --genotypes: the columns are --pav's; the file is written once the workers are done
    if (!run.pav_on) {
      std::vector<std::string> qnames;
      for (int i = 0; i < query->nseq(); ++i) qnames.push_back(query->name(i));
      run.pav_cols = pav::columns(qnames);
    }
    gtstream.open(gt_path);
    if (!gtstream.is_open()) throw std::runtime_error("[wfmash::align] Error! Failed to open the genotypes file: " + gt_path);
    run.sites_on = true;
  }
  const size_t nworkers = run.plan.nworkers;
  static const bool own_handles = !(getenv("WFM_ALIGN_OWN_HANDLES") && atoi(getenv("WFM_ALIGN_OWN_HANDLES")) == 0);
  static HandlePool pool;
  HandlePool::Loan loan(pool);
  for (size_t wk = 0; wk < nworkers; ++wk) {
    run.use[wk] = gpus[wk % ngpu];
    if (wk < ngpu || !own_handles) continue;
    if (wfm_handle_t* own = loan.borrow(wfm_device(gpus[wk % ngpu]), std::max<size_t>(3, run.plan.per_gpu))) run.use[wk] = own;
  }
  {
    std::vector<std::thread> threads;
    for (size_t wk = 1; wk < nworkers; ++wk) threads.emplace_back([this, &run, wk] { run_worker(run, wk); });
    run_worker(run, 0);
    for (auto& t : threads) t.join();
  }
  if (run.failed.load()) throw std::runtime_error(run.first_error);
  if (covstream.is_open()) { finish_coverage(run, covstream); covstream.close(); }
  if (pavstream.is_open()) { finish_pav(run, pavstream, pav_skipped); pavstream.close(); }
  if (gtstream.is_open()) { finish_genotypes(run, gtstream); gtstream.close(); }
  if (netstream.is_open()) { finish_chain_net(run, netstream); netstream.close(); }
  if (transstream.is_open()) { finish_transitive(run, transstream); transstream.close(); }
  sum_up(sum, run.part, t0);
  outstream.close();
  if (vcfstream.is_open()) vcfstream.close();
  if (liftstream.is_open()) liftstream.close();
  if (chainstream.is_open()) chainstream.close();
  sum.ms_total = ms_since(t0);
  std::cerr << "[wfmash::align] total aligned records = " << sum.records << ", total aligned bp = " << sum.aligned_bp
            << ", completed in " << (uint64_t)(sum.ms_total / 1000.0) << " seconds" << std::endl;
  return sum;
}

}  // namespace align
