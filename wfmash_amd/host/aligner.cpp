#include "aligner.hpp"
#include "run_passes.hpp"
#include "verify_paf.hpp"
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

wflign::BatchTexts Aligner::align_batch(wfm_handle_t* gpu_handle, std::vector<std::string>& lines, int threads, Summary& sum, uint64_t first_row,
                                        const wflign::BatchPasses& passes) {
  wflign::BatchTexts texts;
  const bool dbg = getenv("WFM_DEBUG") != nullptr;
  BatchTimes t;
  std::vector<Fetched> rows = parse_rows(lines, first_row, sum);
  t.rows = t.lap();
  DeviceStore* ds = param.resident_sequences ? device_store(gpu_handle) : nullptr;
  if (ds) assign_resident_ids(gpu_handle, *ds, rows);
  std::vector<Fetched> fetched = fetch_eager(rows, threads, sum);
  if (fetched.empty()) return texts;
  std::vector<wflign::BiwfaRecord> recs = make_records(fetched);
  if (const wflign::RunTables* tb = passes.tables)  // (parse_rows has found every name)
    for (wflign::BiwfaRecord& r : recs) {
      r.target_global = tb->seq_offsets[(size_t)ref->find(r.target_name)];
      if (tb->columns.of_seq.empty() && tb->query_world.empty()) continue;
      const int qi = query->find(r.query_name);
      if (!tb->columns.of_seq.empty()) r.pav_group = qi >= 0 ? tb->columns.of_seq[(size_t)qi] : 0xffffffffu;  // (no column: the device flags the record and adds nothing)
      if (!tb->query_world.empty()) r.query_global = tb->query_world[(size_t)qi];
    }
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
  const int rc = wflign::do_biwfa_alignment_batch(gpu_handle, recs, penalties_of(param), param.disable_chain_patching, filters_of(param), &st,
                                                  format_of(param, threads), ds ? &resident : nullptr, &passes, &texts);
  if (rc < 0) throw std::runtime_error(std::string("[wfmash::align] GPU alignment failed: ") + st.error);
  account(sum, st, resident, fetched, recs);
  t.wflign = t.lap();
  std::string& out = texts.paf = gather_text(sum, fetched, recs);
  // (a record without a line has no VCF lines, write_record; lift lines and chains are there already, in the order of the records' lines: take_texts)
  for (const auto& r : recs) { texts.text[wflign::SW_VARIANTS] += r.vcf; texts.text[wflign::SW_MAF] += r.maf; }
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
  return texts;
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
    out += align_batch(gpus.front(), batch, param.threads, sum, first_row).paf;
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

// what: "output file", "the BED file of --lift", ...
template <class Stream>
void open_or_throw(Stream& s, const std::string& path, const char* what, std::ios::openmode mode = std::ios::openmode()) {
  s.open(path, mode);
  if (!s.is_open()) throw std::runtime_error(std::string("[wfmash::align] Error! Failed to open ") + what + ": " + path);
}
std::string read_whole_file(const std::string& path, const char* what) {
  std::ifstream f;
  open_or_throw(f, path, what, std::ios::binary);
  return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
}  // namespace

struct Aligner::Run {
  Run(const Parameters& p, const RunPlan& pl, size_t n_gpu, Clock::time_point start, std::ifstream& i, std::ofstream& o)
      : param(p), plan(pl), ngpu(n_gpu), t0(start), in(i), writer(wflign::TextSink{&o}), in_flight(n_gpu), first_taken(n_gpu), use(pl.nworkers, nullptr),
        part(pl.nworkers), threads_each(std::max(1, p.threads / (int)pl.nworkers)) {
    for (auto& a : in_flight) a.store(0);
    for (auto& a : first_taken) a.store(0);
  }
  ~Run() { for (auto& p : passes) p->free_objects(); }
  const Parameters& param;
  const RunPlan plan;
  const size_t ngpu;
  const Clock::time_point t0;
  std::ifstream& in;
  wflign::TextWriter writer;
  // the passes that are on, in their order, and the tables they share (filled before the first of them is made)
  wflign::RunTables tables;
  std::vector<std::unique_ptr<std::ofstream>> pass_files;  // (each outlives its pass)
  std::vector<std::unique_ptr<wflign::Pass>> passes;
  // a batch's view of them: the handle's objects, each made at the handle's first batch
  wflign::BatchPasses batch_passes(wfm_handle_t* h, uint64_t seq) {
    wflign::BatchPasses bp;
    if (passes.empty()) return bp;
    bp.batch = seq;
    bp.tables = &tables;
    for (auto& p : passes) { bp.on[p->id] = true; bp.object[p->id] = p->object_of(h); }
    return bp;
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
      wflign::BatchTexts texts = align_batch(run.use[wk], batch, run.threads_each, run.part[wk], first_row, run.batch_passes(run.use[wk], (uint64_t)seq));
      const double at1 = run.ms();
      run.writer.put((uint64_t)seq, std::move(texts.paf));
      for (auto& p : run.passes) p->take((uint64_t)seq, texts);
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

// the passes whose switches are on, each with its file open and the BED it reads read; the run's tables before the first of them
void Aligner::make_passes(Run& run) const {
  static const char* const kNames[wflign::N_PASSES] = {"variants", "coverage", "lift", "chain", "pav", "genotypes", "chain-net", "transitive", "maf"};
  for (int id = 0; id < wflign::N_PASSES; ++id) {
    const wflign::SwitchSetting s = wflign::switch_setting((wflign::SwitchId)id);
    if (s.out.empty()) continue;
    if (run.passes.empty()) wflign::fill_tables(run.tables, *ref, *query);
    const std::string name = kNames[id];
    run.pass_files.emplace_back(new std::ofstream());
    open_or_throw(*run.pass_files.back(), s.out, ("the " + name + " file").c_str());
    wflign::PassInput in;
    in.prefix = "[wfmash::align] --" + name + ":";
    in.out = run.pass_files.back().get();
    in.has_bed = !s.bed.empty();
    if (in.has_bed) in.bed = read_whole_file(s.bed, ("the BED file of --" + name).c_str());
    in.option = s.option;
    run.passes.push_back(wflign::make_pass((wflign::SwitchId)id, run.tables, in));
  }
}

Summary Aligner::compute() {
  Summary sum;
  const auto t0 = Clock::now();
  std::ifstream in;
  open_or_throw(in, param.mashmapPafFile, "input mapping file");
  std::ofstream outstream;
  open_or_throw(outstream, param.pafOutputFile, "output file");
  if (param.sam_format) {  // write_sam_header (computeAlignments.hpp:725-736)
    for (int i = 0; i < ref->nseq(); ++i) outstream << "@SQ\tSN:" << ref->name(i) << "\tLN:" << ref->length(i) << "\n";
    outstream << "@PG\tID:wfmash\tPN:wfmash\tVN:" WFMASH_HIP_VERSION "\tCL:wfmash\n";
  }
  const size_t ngpu = gpus.size();
  Run run(param, plan_run(in), ngpu, t0, in, outstream);
  make_passes(run);
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
  for (size_t k = 0; k < run.passes.size(); ++k) {  // (the files the workers did not write, each from its handles' objects merged into one)
    const wflign::Pass::Finished end = run.passes[k]->finish();
    wflign::switch_finished(run.passes[k]->id, end.c[0], end.c[1], end.c[2]);
    if (!end.debug.empty()) fputs(end.debug.c_str(), stderr);
    run.pass_files[k]->close();
  }
  sum_up(sum, run.part, t0);
  outstream.close();
  sum.ms_total = ms_since(t0);
  std::cerr << "[wfmash::align] total aligned records = " << sum.records << ", total aligned bp = " << sum.aligned_bp
            << ", completed in " << (uint64_t)(sum.ms_total / 1000.0) << " seconds" << std::endl;
  return sum;
}

}  // namespace align
