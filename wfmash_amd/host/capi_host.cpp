// capi_host.cpp -- C entry points of the host-side align driver (include/wfmash_host.h).
#include <algorithm>
#include <exception>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/wfmash_host.h"
#include "../csrc/wfa_handle.h"
#include "../csrc/wfa_pack.h"
#include "../csrc/wfa_plan.h"
#include "../csrc/wfa_optband.h"
#include "aligner.hpp"
#include "fasta.hpp"
#include "chain_text.hpp"
#include "lift_text.hpp"
#include "transitive_text.hpp"
#include "pav_text.hpp"
#include "genotype_text.hpp"
#include "map_stats.hpp"

extern "C" {

// CPU test hook of the packed extension (csrc/wfa_pack.h): both buffers are packed as wfm_upload_sequences' mirror is, the
// sequences begin at byte start_p / start_t of their buffers (any alignment), and the staged comparison of the tile kernel --
// 16 bases, 64, then 32 at a time, from window origins rounded down to a word -- is run from (v, h).  Returns the run length.
int wfmh_test_packed_lce(const uint8_t* buf_p, int64_t n_p, int64_t start_p, const uint8_t* buf_t, int64_t n_t, int64_t start_t, int v, int h, int maxn) {
  if (!buf_p || !buf_t || n_p < 0 || n_t < 0 || start_p < 0 || start_t < 0 || v < 0 || h < 0) return -1;
  std::vector<uint32_t> wp((size_t)(n_p + 15) / 16 + 16, 0u), wt((size_t)(n_t + 15) / 16 + 16, 0u);
  wfm::pack_words_model(buf_p, n_p, wp.data());
  wfm::pack_words_model(buf_t, n_t, wt.data());
  const int64_t ori_p = start_p & ~(int64_t)15, ori_t = start_t & ~(int64_t)15;
  return wfm::pk_lce_model(wp.data() + (ori_p >> 4), wt.data() + (ori_t >> 4), (uint32_t)(v + (start_p - ori_p)), (uint32_t)(h + (start_t - ori_t)), maxn);
}
// 1 when every byte is one of A C G T (upper case): the problems the packed kernels take
int wfmh_test_is_acgt(const uint8_t* seq, int64_t n) {
  for (int64_t i = 0; i < n; ++i) if (!wfm::pack_is_acgt(seq[i])) return 0;
  return 1;
}

void wfmh_align_default_params(wfmh_align_params_t* p) {
  if (!p) return;
  p->mismatch = 5; p->gap_open1 = 8; p->gap_ext1 = 2; p->gap_open2 = 24; p->gap_ext2 = 1;
  p->min_identity = 0.0f; p->min_alignment_length = 32; p->min_block_identity = 0.1f;
  p->target_padding = 1000; p->query_padding = 1000; p->wflign_max_len_minor = 128000;
  p->disable_chain_patching = 0;
  p->sam_format = 0; p->emit_md_tag = 0; p->no_seq_in_sam = 0;
  p->threads = 0; p->resident_sequences = 0;
}

int wfmh_align_paf(wfm_handle_t* h, const char* target_fasta, const char* query_fasta, const char* mapping_paf,
                   const char* out_paf, const wfmh_align_params_t* params, wfmh_align_summary_t* summary) {
  return wfmh_align_paf_multi(&h, 1, target_fasta, query_fasta, mapping_paf, out_paf, params, summary);
}

int wfmh_align_paf_multi(wfm_handle_t* const* handles, int n, const char* target_fasta, const char* query_fasta, const char* mapping_paf,
                         const char* out_paf, const wfmh_align_params_t* params, wfmh_align_summary_t* summary) {
  if (!handles || n < 1 || !target_fasta || !mapping_paf || !out_paf) return WFM_E_ARG;
  for (int i = 0; i < n; ++i) if (!handles[i]) return WFM_E_ARG;
  wfm_handle_t* h = handles[0];
  wfmh_align_params_t d;
  wfmh_align_default_params(&d);
  if (params) d = *params;
  try {
    align::Parameters ap;
    ap.refSequences.push_back(target_fasta);
    ap.querySequences.push_back(query_fasta ? query_fasta : target_fasta);
    ap.mashmapPafFile = mapping_paf;
    ap.pafOutputFile = out_paf;
    ap.wfa_patching_mismatch_score = d.mismatch;
    ap.wfa_patching_gap_opening_score1 = d.gap_open1;
    ap.wfa_patching_gap_extension_score1 = d.gap_ext1;
    ap.wfa_patching_gap_opening_score2 = d.gap_open2;
    ap.wfa_patching_gap_extension_score2 = d.gap_ext2;
    ap.min_identity = d.min_identity;
    ap.min_alignment_length = d.min_alignment_length;
    ap.min_block_identity = d.min_block_identity;
    ap.target_padding = d.target_padding;
    ap.query_padding = d.query_padding;
    ap.wflign_max_len_minor = d.wflign_max_len_minor;
    ap.disable_chain_patching = d.disable_chain_patching != 0;
    ap.sam_format = d.sam_format != 0; ap.emit_md_tag = d.emit_md_tag != 0; ap.no_seq_in_sam = d.no_seq_in_sam != 0;
    ap.resident_sequences = d.resident_sequences != 0;
    ap.threads = d.threads > 0 ? d.threads : (int)std::max(1u, std::thread::hardware_concurrency());
    align::Aligner aligner(ap, std::vector<wfm_handle_t*>(handles, handles + n));
    const align::Summary s = aligner.compute();
    if (summary) {
      summary->records = s.records; summary->aligned_bp = s.aligned_bp; summary->written = s.written;
      summary->skipped = s.skipped; summary->cells = s.cells; summary->ms_gpu = s.ms_gpu; summary->ms_total = s.ms_total;
      summary->ms_rows = s.ms_rows; summary->ms_fetch = s.ms_fetch; summary->ms_wflign = s.ms_wflign; summary->ms_text = s.ms_text;
      summary->batches = s.batches;
      summary->cells_tile = s.cells_tile; summary->tile_launches = s.tile_launches; summary->ms_tile = s.ms_tile;
      summary->ms_tags = s.ms_tags;
      summary->records_resident = s.records_resident; summary->lazy_fetches = s.lazy_fetches;
    }
    return WFM_OK;
  } catch (const std::exception& e) {
    std::cerr << e.what() << std::endl;
    wfm_set_error(h, e.what());
    return WFM_E_ARG;
  }
}

}  // extern "C"

// ---- test hooks: expose the pure host-side CIGAR functions to the CPU test-suite ----
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <vector>

extern "C" {

void wfmh_free(char* p) { free(p); }

// test hook (no GPU): the text side of --lift (lift_text.hpp): what the parser makes of a BED, and the lines of given lifts
char* wfmh_test_lift_lines(const char* const* names, const uint64_t* lengths, int n_seq, const char* bed, const char* spec) {
  if (n_seq < 0 || (n_seq && (!names || !lengths)) || !bed || !spec) return nullptr;
  std::vector<std::string> nm;
  std::vector<uint64_t> len, off(1, 0);
  for (int i = 0; i < n_seq; ++i) { nm.push_back(names[i]); len.push_back(lengths[i]); off.push_back(off.back() + lengths[i]); }
  const lift::Bed parsed = lift::parse_bed(std::string(bed), [&](const std::string& name) {
    for (size_t i = 0; i < nm.size(); ++i) if (nm[i] == name) return (int)i;
    return -1;
  }, len, off);
  std::string out = lift::bed_dump(parsed);
  std::vector<lift::Record> recs;
  std::istringstream in(spec);
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::vector<std::string> f;
    for (size_t at = 0;;) {
      const size_t tab = line.find('\t', at);
      f.push_back(line.substr(at, tab == std::string::npos ? std::string::npos : tab - at));
      if (tab == std::string::npos) break;
      at = tab + 1;
    }
    uint64_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (f[0] == "R" && f.size() == 7) {
      lift::Record r;
      r.qname = f[1]; r.tname = f[5]; r.rev = f[4] == "-";
      if (!lift::decimal(f[2], 0, f[2].size(), &r.qs) || !lift::decimal(f[3], 0, f[3].size(), &r.qe) || !lift::decimal(f[6], 0, f[6].size(), &r.ts)) return nullptr;
      recs.push_back(r);
    } else if (f[0] == "L" && f.size() == 9) {
      for (int k = 0; k < 8; ++k)
        if (!lift::decimal(f[(size_t)k + 1], 0, f[(size_t)k + 1].size(), &v[k]) || v[k] > 0xffffffffull) return nullptr;
      if (v[0] >= recs.size() || v[1] >= parsed.iv.size()) return nullptr;
      lift::lift_line(out, recs[(size_t)v[0]], parsed.iv[(size_t)v[1]], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5], (uint32_t)v[6], (uint32_t)v[7]);
    } else {
      return nullptr;
    }
  }
  char* p = (char*)malloc(out.size() + 1);
  if (p) memcpy(p, out.c_str(), out.size() + 1);
  return p;
}

// test hook (no GPU): the text side of --transitive (transitive_text.hpp): the world, the seeds the parser keeps, the lines of given intervals
char* wfmh_test_transitive_lines(const char* const* tnames, const uint64_t* tlengths, int n_t, const char* const* qnames, const uint64_t* qlengths,
                                 int n_q, const char* bed, const char* spec) {
  if (n_t < 0 || n_q < 0 || (n_t && (!tnames || !tlengths)) || (n_q && (!qnames || !qlengths)) || !bed || !spec) return nullptr;
  std::vector<std::string> tn, qn;
  std::vector<uint64_t> tl, ql;
  for (int i = 0; i < n_t; ++i) { tn.push_back(tnames[i]); tl.push_back(tlengths[i]); }
  for (int i = 0; i < n_q; ++i) { qn.push_back(qnames[i]); ql.push_back(qlengths[i]); }
  const transitive::World w = transitive::make_world(tn, tl, qn, ql);
  const lift::Bed seeds = transitive::parse_seeds(std::string(bed), w);
  std::string out = lift::bed_dump(seeds);
  std::istringstream in(spec);
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    uint64_t v[3] = {0, 0, 0};
    size_t at = 2;
    if (line.compare(0, 2, "I\t") != 0) return nullptr;
    for (int k = 0; k < 3; ++k) {
      const size_t tab = line.find('\t', at), end = tab == std::string::npos ? line.size() : tab;
      if (!lift::decimal(line, at, end, &v[k]) || ((tab == std::string::npos) != (k == 2))) return nullptr;
      at = end + 1;
    }
    if (v[0] >= seeds.iv.size() || v[1] > v[2] || v[2] > w.n_bases()) return nullptr;
    transitive::lines(out, w, seeds.iv[(size_t)v[0]], v[1], v[2]);
  }
  char* p = (char*)malloc(out.size() + 1);
  if (p) memcpy(p, out.c_str(), out.size() + 1);
  return p;
}

// test hook (no GPU): the text side of --chain (chain_text.hpp): the flags of the records' problems and the file of given blocks
char* wfmh_test_chain_lines(const char* spec, int swap, uint32_t* flags_out) {
  if (!spec) return nullptr;
  std::string body;
  chain::Record r;
  chain::Ends e;
  std::vector<chain::Block> blocks;
  bool open = false;
  size_t n_rec = 0;
  auto close = [&]() {
    if (open) chain::chain_body(body, r, swap != 0, e, blocks.data(), blocks.size());
    blocks.clear();
  };
  std::istringstream in(spec);
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::vector<std::string> f;
    for (size_t at = 0;;) {
      const size_t tab = line.find('\t', at);
      f.push_back(line.substr(at, tab == std::string::npos ? std::string::npos : tab - at));
      if (tab == std::string::npos) break;
      at = tab + 1;
    }
    uint64_t v[5] = {0, 0, 0, 0, 0};
    if (f[0] == "R" && f.size() == 15) {
      close();
      open = true;
      r = chain::Record();
      r.qname = f[1]; r.tname = f[6]; r.rev = f[5] == "-";
      if (!lift::decimal(f[2], 0, f[2].size(), &r.qsize) || !lift::decimal(f[3], 0, f[3].size(), &r.qs) || !lift::decimal(f[4], 0, f[4].size(), &r.qe) ||
          !lift::decimal(f[7], 0, f[7].size(), &r.tsize) || !lift::decimal(f[8], 0, f[8].size(), &r.ts) || !lift::decimal(f[9], 0, f[9].size(), &r.te))
        return nullptr;
      for (int k = 0; k < 5; ++k)
        if (!lift::decimal(f[(size_t)k + 10], 0, f[(size_t)k + 10].size(), &v[k]) || v[k] > 0xffffffffull) return nullptr;
      e.eq = (uint32_t)v[0]; e.lead_dt = (uint32_t)v[1]; e.lead_dq = (uint32_t)v[2]; e.trail_dt = (uint32_t)v[3]; e.trail_dq = (uint32_t)v[4];
      if (flags_out) flags_out[n_rec] = chain::flags_of(swap != 0, r.rev);
      ++n_rec;
    } else if (f[0] == "B" && f.size() == 4 && open) {
      for (int k = 0; k < 3; ++k)
        if (!lift::decimal(f[(size_t)k + 1], 0, f[(size_t)k + 1].size(), &v[k]) || v[k] > 0xffffffffull) return nullptr;
      blocks.push_back(chain::Block{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], 0u});
    } else {
      return nullptr;
    }
  }
  close();
  std::string out;
  uint64_t next = 1;
  chain::number(body, &next, out);
  char* p = (char*)malloc(out.size() + 1);
  if (p) memcpy(p, out.c_str(), out.size() + 1);
  return p;
}

// test hook (no GPU): the text side of --chain-net (chain_text.hpp's net_body): the file of given records and pieces
char* wfmh_test_chain_net_lines(const char* spec) {
  if (!spec) return nullptr;
  std::string body;
  chain::Record r;
  uint64_t t_offset = 0, score = 0;
  std::vector<chain::Piece> pieces;
  bool open = false;
  auto close = [&]() {
    if (open) chain::net_body(body, r, t_offset, (uint32_t)score, pieces.data(), pieces.size());
    pieces.clear();
  };
  std::istringstream in(spec);
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::vector<std::string> f;
    for (size_t at = 0;;) {
      const size_t tab = line.find('\t', at);
      f.push_back(line.substr(at, tab == std::string::npos ? std::string::npos : tab - at));
      if (tab == std::string::npos) break;
      at = tab + 1;
    }
    uint64_t v[3] = {0, 0, 0};
    if (f[0] == "R" && f.size() == 10) {
      close();
      open = true;
      r = chain::Record();
      r.qname = f[1]; r.tname = f[6]; r.rev = f[5] == "-";
      if (!lift::decimal(f[2], 0, f[2].size(), &r.qsize) || !lift::decimal(f[3], 0, f[3].size(), &r.qs) || !lift::decimal(f[4], 0, f[4].size(), &r.qe) ||
          !lift::decimal(f[7], 0, f[7].size(), &r.tsize) || !lift::decimal(f[8], 0, f[8].size(), &t_offset) || !lift::decimal(f[9], 0, f[9].size(), &score) ||
          score > 0xffffffffull)
        return nullptr;
    } else if (f[0] == "P" && f.size() == 4 && open) {
      for (int k = 0; k < 3; ++k)
        if (!lift::decimal(f[(size_t)k + 1], 0, f[(size_t)k + 1].size(), &v[k])) return nullptr;
      if (v[1] > 0xffffffffull || v[2] > 0xffffffffull) return nullptr;
      pieces.push_back(chain::Piece{0, v[0], (uint32_t)v[1], (uint32_t)v[2]});
    } else {
      return nullptr;
    }
  }
  close();
  std::string out;
  uint64_t next = 1;
  chain::number(body, &next, out);
  char* p = (char*)malloc(out.size() + 1);
  if (p) memcpy(p, out.c_str(), out.size() + 1);
  return p;
}

// test hook (no GPU): the text side of --pav (pav_text.hpp): the names' keys and columns, the header, the windows' rows
char* wfmh_test_pav_text(const char* const* names, int n_q, const char* const* tnames, const uint64_t* lengths, int n_t, uint64_t window) {
  if (n_q < 0 || n_t < 0 || (n_q && !names) || (n_t && (!tnames || !lengths))) return nullptr;
  std::vector<std::string> nm;
  for (int i = 0; i < n_q; ++i) nm.push_back(names[i]);
  std::vector<uint64_t> len, off(1, 0);
  for (int i = 0; i < n_t; ++i) { len.push_back(lengths[i]); off.push_back(off.back() + lengths[i]); }
  const pav::Columns cols = pav::columns(nm);
  std::string out;
  for (size_t i = 0; i < nm.size(); ++i) out += "#key\t" + nm[i] + "\t" + pav::group_key(nm[i]) + "\t" + std::to_string(cols.of_seq[i]) + "\n";
  out += pav::header(cols.keys);
  const std::vector<lift::Interval> win = pav::windows(len, off, window);
  std::vector<uint32_t> cells(cols.keys.size());
  for (size_t j = 0; j < win.size(); ++j) {
    for (size_t g = 0; g < cells.size(); ++g) cells[g] = (uint32_t)(j + g);
    pav::row(out, tnames[win[j].seq], win[j], cells.data(), cells.size());
  }
  char* p = (char*)malloc(out.size() + 1);
  if (p) memcpy(p, out.c_str(), out.size() + 1);
  return p;
}

// test hook (no GPU): the text side of --genotypes (genotype_text.hpp): the header, the order of the lines, the lines
char* wfmh_test_genotype_text(const char* version, const char* const* tnames, const uint64_t* lengths, int n_t, const char* const* keys, int n_groups,
                              const uint64_t* sites, size_t n_sites, const char* alleles, const char* gt) {
  if (!version || n_t < 0 || n_groups < 0 || (n_t && (!tnames || !lengths)) || (n_groups && !keys) || (n_sites && (!sites || !alleles || (n_groups && !gt)))) return nullptr;
  std::vector<std::string> names, cols;
  std::vector<uint64_t> len, off(1, 0);
  for (int i = 0; i < n_t; ++i) { names.push_back(tnames[i]); len.push_back(lengths[i]); off.push_back(off.back() + lengths[i]); }
  for (int g = 0; g < n_groups; ++g) cols.push_back(keys[g]);
  std::vector<genotype::Site> ss(n_sites);
  for (size_t i = 0; i < n_sites; ++i) ss[i] = genotype::Site{sites[4 * i], (uint32_t)sites[4 * i + 1], (uint32_t)sites[4 * i + 2], sites[4 * i + 3]};
  std::string out = genotype::header(version, names, len, cols);
  for (size_t i : genotype::order(ss, alleles)) genotype::site_line(out, ss, i, alleles, gt, (size_t)n_groups, names, off);
  char* p = (char*)malloc(out.size() + 1);
  if (p) memcpy(p, out.c_str(), out.size() + 1);
  return p;
}

// test hook: the sub-window translation of the problems by reference (wflign::sub_window_off)
void wfmh_test_subwindow(int64_t win_start, int64_t win_end, int rev, int64_t a, int64_t b, int64_t* out_start, int64_t* out_end) {
  const int64_t off = wflign::sub_window_off(win_start, win_end - win_start, rev != 0, a, b);
  if (out_start) *out_start = off;
  if (out_end) *out_end = off + (b - a);
}

// test hook: the align driver's batch plan (plan_batch_bytes, host/align_plan.hpp), pure arithmetic
unsigned long long wfmh_test_plan_batch_bytes(unsigned long long file_bytes, unsigned long long rows, unsigned long long row_bytes,
                                              unsigned long long row_bases_sum, unsigned long long batch_records, unsigned long long batch_bases,
                                              unsigned long long nworkers, unsigned long long ngpu, unsigned long long min_batches, int level) {
  return align::plan_batch_bytes(file_bytes, rows, row_bytes, row_bases_sum, batch_records, batch_bases, nworkers, ngpu, min_batches, level != 0);
}

// test hook: the align driver's other plans (host/align_plan.hpp), pure arithmetic on doubles (-1 stands for "none" / "no limit").
// op 0: workers_per_gpu -- in = threads, ngpu, override; out = {workers}
// op 1: estimate_batches -- in = file_bytes, rows, row_bytes, row_bases_sum, batch_records, batch_bases, batch_bytes; out = {batches or -1}
// op 2: interval_union -- in = n x (from, to); out = {intervals of the union, their total length, then the intervals}
// op 3: the twenty-bin histogram of the union over span_of the sorted input (n >= 1) -- out = {total, span, then 20 bins}
int wfmh_test_align_plan(int op, const double* in, int64_t n, double* out) {
  auto u64 = [](double v) { return v < 0 ? ~0ull : (uint64_t)v; };
  if (op == 0) { out[0] = (double)align::workers_per_gpu((size_t)in[0], (size_t)in[1], (size_t)in[2]); return 0; }
  if (op == 1) {
    const uint64_t b = align::estimate_batches(u64(in[0]), u64(in[1]), u64(in[2]), u64(in[3]), u64(in[4]), u64(in[5]), u64(in[6]));
    out[0] = b == ~0ull ? -1.0 : (double)b;
    return 0;
  }
  if (op != 2 && op != 3) return -1;
  std::vector<align::Interval> v;
  for (int64_t i = 0; i < n; ++i) v.emplace_back(in[2 * i], in[2 * i + 1]);
  const std::vector<align::Interval> u = align::interval_union(v);
  if (op == 2) {
    out[0] = (double)u.size(); out[1] = align::total_length(u);
    for (size_t i = 0; i < u.size(); ++i) { out[2 + 2 * i] = u[i].first; out[3 + 2 * i] = u[i].second; }
    return 0;
  }
  if (v.empty()) return -1;
  const align::Interval sp = align::span_of(v);
  const std::vector<double> bins = align::covered_per_bin(u, sp.first, sp.second, 20);
  out[0] = align::total_length(u); out[1] = sp.second;
  std::copy(bins.begin(), bins.end(), out + 2);
  return 0;
}

// test hook: which ring a BiWFA job gets (csrc/wfa_plan.h, plan_ring), pure arithmetic.  node: pl, tl, score_rem, sub, noband, band;
// rules: tiles enabled, min_len, min_score, chunk, T, RR, use_band, over_budget, roots_off, band_root.  Returns 0 and
// out = {width, koff, band, tile_it, grown, need}, or WFM_ST_OOM.
int wfmh_test_ring_plan(const int32_t* node, const int32_t* rules, unsigned long long mem_budget, int64_t* out) {
  wfm::Node nd{};
  nd.pl = node[0]; nd.tl = node[1]; nd.score_rem = node[2]; nd.sub = node[3]; nd.noband = node[4]; nd.band = node[5];
  wfm::RingRules r{rules[0] != 0, rules[1], rules[2], rules[3], rules[4], rules[5], (size_t)mem_budget, rules[9], rules[6] != 0, rules[7] != 0, rules[8] != 0};
  const wfm::RingPlan p = wfm::plan_ring(nd, r);
  if (!p.fits) return WFM_ST_OOM;
  const int64_t v[6] = {(int64_t)p.width, p.koff, p.band, p.tile_it, p.grown, (int64_t)p.need};
  std::copy(v, v + 6, out);
  return 0;
}

// test hook: a problem's runs into its op string (csrc/wfa_plan.h, expand_runs).  rle == 0: op bytes into ops[0 .. ops_cap); else the
// merged runs go behind the *n_runs_io entries runs_io already holds (room for runs_cap), *n_runs_io = what it holds afterwards.
// res = {score, n_runs, ops_len}.  Returns expand_runs' code: 0, 1 spans do not match, 2 arena too small, 3 run too long.
int wfmh_test_expand_runs(const uint32_t* runs, int n, const wfm_penalties_t* pen, int plen, int tlen, int rle, char* ops, size_t ops_cap,
                          uint32_t* runs_io, size_t* n_runs_io, size_t runs_cap, int64_t* res) {
  std::vector<uint32_t> v;
  if (rle) v.assign(runs_io, runs_io + *n_runs_io);
  wfm::Expanded ex;
  const int rc = wfm::expand_runs(runs, n, *pen, plen, tlen, ops, ops_cap, rle ? &v : nullptr, &ex);
  if (rle) { std::copy(v.begin(), v.begin() + std::min(v.size(), runs_cap), runs_io); *n_runs_io = v.size(); }
  res[0] = ex.score; res[1] = ex.n_runs; res[2] = ex.ops_len;
  return rc;
}

// test hook: the row arithmetic of csrc/wfa_rows.h and csrc/wfa_plan.h, n queries of 7 numbers (op, then its arguments), two results each.
// op 0: cells_sum(pl, tl, sub, a, b); 1: rng_block(pl, tl, sub, s_from, s_to) -> L, R; 2: tile_span(L, R, idx, core) -> lo, hi;
// 3: tiles_for(L, R, core); 4: tile_job_leaves(pl, tl, sub, s0, band, chunk) with T = 100, 5: the same with T = 32
// 6: tile_job_beyond_limit(pl, tl, sub, limit, s0) with T = 100, 7: the same with T = 32
int wfmh_test_rows(const int32_t* q, int64_t n, int64_t* out) {
  for (int64_t i = 0; i < n; ++i, q += 7, out += 2) {
    int a = 0, b = 0;
    out[0] = out[1] = 0;
    switch (q[0]) {
      case 0: out[0] = wfm::cells_sum(q[1], q[2], q[3], q[4], q[5]); break;
      case 1: wfm::rng_block(wfm::make_rng(q[1], q[2], q[3]), q[4], q[5], a, b); out[0] = a; out[1] = b; break;
      case 2: wfm::tile_span(q[1], q[2], q[3], q[4], &a, &b); out[0] = a; out[1] = b; break;
      case 3: out[0] = wfm::tiles_for(q[1], q[2], q[3]); break;
      case 4: case 5: out[0] = wfm::tile_job_leaves(q[1], q[2], q[3], q[4], q[5], q[6], q[0] == 4 ? 100 : 32); break;
      case 6: case 7: out[0] = wfm::tile_job_beyond_limit(q[1], q[2], q[3], q[4], q[5], q[0] == 6 ? 100 : 32); break;
      default: return -1;
    }
  }
  return 0;
}

// test hook: the interior test of csrc/wfa_rows.h, n queries of 7 numbers (pl, tl, sub, first diagonal, last diagonal, first score, last score),
// three results each: rng_interior's answer, then rng_lo and rng_hi at the FIRST score (a brute force asks about one score at a time)
int wfmh_test_tile_interior(const int32_t* q, int64_t n, int32_t* out) {
  for (int64_t i = 0; i < n; ++i, q += 7, out += 3) {
    const wfm::Rng r = wfm::make_rng(q[0], q[1], q[2]);
    out[0] = wfm::rng_interior(r, q[3], q[4], q[5], q[6]) ? 1 : 0;
    out[1] = wfm::rng_lo(r, q[5]);
    out[2] = wfm::rng_hi(r, q[5]);
  }
  return 0;
}

// test hook: the waves of the packed tile kernel (csrc/wfa_tile2.hip) that take the lean snapshot paths in ONE block of one direction of a job:
// in = pl, tl, sub, s0 (the score the block starts from), T, Tn (the steps it takes: T, or fewer in the run up to the meeting point), core, threads.
// The block's range cut into tile_span's tiles, each tile's waves as the kernel lays them out (a halo of T diagonals on either side unless the
// block is one tile; two diagonals a lane), and tile_wave_lean_load / tile_wave_lean_store on each -- the predicate the kernel evaluates, no
// counter of the kernel's.  out = {tiles, waves, waves that pass the load test, waves that pass the store test, tiles that hold waves of both kinds
// at the load}
int wfmh_test_tile_lean_waves(const int32_t* in, int64_t* out) {
  const wfm::Rng r = wfm::make_rng(in[0], in[1], in[2]);
  const int s0 = in[3], T = in[4], Tn = in[5], core = in[6], threads = in[7];
  if (T < 1 || core < 1 || threads < 64) return -1;
  int L, R;
  wfm::rng_block(r, s0, s0 + T, L, R);
  const int nt = wfm::tiles_for(L, R, core);
  out[0] = nt; out[1] = out[2] = out[3] = out[4] = 0;
  for (int idx = 0; idx < nt; ++idx) {
    int lo, hi;
    wfm::tile_span(L, R, idx, core, &lo, &hi);
    const int halo = (lo == L && hi == R) ? 0 : T;
    const int kA = lo - halo, kmax = hi + halo;
    const int nw = std::min(threads / 64, (kmax - kA) / wfm::WAVE_DIAGS + 1);
    int lean_here = 0;
    for (int w = 0; w < nw; ++w) {
      const int kw = kA + w * wfm::WAVE_DIAGS;
      out[1] += 1;
      lean_here += wfm::tile_wave_lean_load(r, kw, kmax, s0) ? 1 : 0;
      out[3] += wfm::tile_wave_lean_store(r, kw, lo, hi, s0 + Tn, Tn) ? 1 : 0;
    }
    out[2] += lean_here;
    out[4] += (lean_here > 0 && lean_here < nw) ? 1 : 0;
  }
  return 0;
}

// the band of wfm_check_optimal (csrc/wfa_optband.h): in = {x, o1, e1, o2, e2, plen, tlen, pbf, pef, tbf, tef, S}, out = {band_lo, band_hi, cells}
int wfmh_test_opt_band(const int64_t* in, int64_t* out) {
  if (!in || !out || in[5] < 0 || in[6] < 0 || in[11] < 0) return -1;
  const wfm::OptBand b = wfm::opt_band(wfm::OptPen{in[0], in[1], in[2], in[3], in[4]}, in[5], in[6], in[7], in[8], in[9], in[10], in[11]);
  out[0] = b.lo; out[1] = b.hi; out[2] = (int64_t)b.cells;
  return 0;
}

// test hook: plan_tile_chunk (csrc/wfa_plan.h).  jobs: n x (pl, tl, sub, s0, mode, fine_s, packed, active); rules: threads, C, T, chunk, core, reg,
// fine, coarse_on.  per_block: threads_b then variants_b (chunk each); tasks: (job, dir, tile, core) each, at most tasks_cap of them are written;
// scalars = {core_c, tasks, n_pk}
int wfmh_test_tile_plan(const int32_t* jobs, int64_t n, const int32_t* rules, int32_t* per_block, int32_t* tasks, int64_t tasks_cap, int64_t* scalars) {
  static_assert(sizeof(wfm::TilePlanJob) == 8 * sizeof(int32_t) && sizeof(wfm::TileTask) == 4 * sizeof(int32_t), "the hooks copy these as rows of int32");
  wfm::TilePlanRules r{rules[0], rules[1], rules[2], rules[3], rules[4], rules[5] != 0, rules[6] != 0, rules[7] != 0};
  if (r.chunk < 1 || r.T < 1 || r.threads < 1 || r.C < 1 || r.core < 1) return -1;
  wfm::TileChunkPlan p;
  wfm::plan_tile_chunk(reinterpret_cast<const wfm::TilePlanJob*>(jobs), (size_t)n, r, p);
  std::copy(p.threads_b.begin(), p.threads_b.end(), per_block);
  std::copy(p.variants_b.begin(), p.variants_b.end(), per_block + r.chunk);
  memcpy(tasks, p.tasks.data(), std::min<size_t>(p.tasks.size(), (size_t)tasks_cap) * sizeof(wfm::TileTask));
  scalars[0] = p.core_c; scalars[1] = (int64_t)p.tasks.size(); scalars[2] = (int64_t)p.n_pk;
  return 0;
}

// test hook: the planning of parent reuse (csrc/wfa_plan.h), pure arithmetic.
// op 0: reuse_pick_keep -- in = score_rem, T, fine_margin, min_blocks, then n kept scores; out = {index picked or -1, reuse_resume_limit}
// op 1: reuse_eligible -- in = child pl, tl, score_rem, the sub its job runs under (the node's bound is score_rem + 56, none without a score), keep; its ring plan: fits, tile_it, band, grown; the keeping job's
//       pl, tl, sub; s_k; T (n is not used); out = {0 / 1}
// op 2: the cadence -- in = every, chunk, T, cap in bytes, then n x (pl, tl, upto); out = {reuse_cadence, reuse_fit_cadence from it}
// op 3: reuse_keep_wanted on reuse_meet_estimate -- in = s0, es, mak, A, cadence, T; out = {0 / 1, the estimate}
int wfmh_test_reuse_plan(int op, const int64_t* in, int64_t n, int64_t* out) {
  if (op == 0) {
    std::vector<int32_t> kept((size_t)n);
    for (int64_t i = 0; i < n; ++i) kept[(size_t)i] = (int32_t)in[4 + i];
    out[0] = wfm::reuse_pick_keep(kept.data(), kept.size(), (int)in[0], (int)in[1], (int)in[2], (int)in[3]);
    out[1] = in[0] == INT_MAX ? -1 : wfm::reuse_resume_limit((int)in[0], (int)in[1], (int)in[2]);
    return 0;
  }
  if (op == 1) {
    wfm::Node nd{};
    nd.pl = (int32_t)in[0]; nd.tl = (int32_t)in[1]; nd.score_rem = (int32_t)in[2]; nd.keep = (int32_t)in[4];
    nd.sub = nd.score_rem == INT_MAX ? wfm::SUB_NONE : nd.score_rem + 56;
    wfm::RingPlan rp;
    rp.fits = in[5] != 0; rp.tile_it = in[6] != 0; rp.band = (int)in[7]; rp.grown = in[8] != 0;
    out[0] = wfm::reuse_eligible(nd, rp, (int)in[9], (int)in[10], (int)in[11], (int)in[3], (int)in[12], (int)in[13]);
    return 0;
  }
  if (op == 2) {
    if (in[0] < 1 || in[1] < 1 || in[2] < 1) return -1;
    std::vector<wfm::ReuseKeeper> kp((size_t)n);
    for (int64_t i = 0; i < n; ++i) kp[(size_t)i] = wfm::ReuseKeeper{(int)in[4 + 3 * i], (int)in[5 + 3 * i], (int)in[6 + 3 * i]};
    out[0] = wfm::reuse_cadence((int)in[0], (int)in[1]);
    out[1] = wfm::reuse_fit_cadence(kp.data(), kp.size(), (int)out[0], (int)in[2], (size_t)in[3]);
    return 0;
  }
  if (op == 3) {  // reuse_keep_wanted with reuse_meet_estimate: in = s0, es, mak, A, cadence, T
    out[1] = wfm::reuse_meet_estimate((int)in[0], in[2], in[3]);
    out[0] = wfm::reuse_keep_wanted((int)in[1], out[1], (int)in[4], (int)in[5]);
    return 0;
  }
  return -1;
}

// test hook: the planned end of phase 1 (csrc/wfa_plan.h), pure arithmetic, n queries of 16 numbers, 8 results each.
// in = x, o1, e1, o2, e2; score_rem, comp_begin, comp_end, second child (0 / 1); then for the eligibility test: the node's bound (sub, 1 << 29: none),
// its ring plan: fits, tile_it, grown; packed; the score of the keep it resumes from (0: none); T
// out = {sf + sr, sf, sr, last_fwd, the score the block of the planned end begins at, tf, tr, planned_meet_eligible}
int wfmh_test_planned_meet(const int64_t* in, int64_t n, int64_t* out) {
  for (int64_t i = 0; i < n; ++i, in += 16, out += 8) {
    wfm_penalties_t pen{};
    pen.x = (int)in[0]; pen.o1 = (int)in[1]; pen.e1 = (int)in[2]; pen.o2 = (int)in[3]; pen.e2 = (int)in[4];
    const int T = (int)in[15];
    if (T < 1) return -1;
    const int sum = wfm::planned_meet_sum((int)in[5], pen, (int)in[6], (int)in[7], in[8] != 0);
    const wfm::PlannedMeet m = wfm::planned_meet((int)in[5], pen, (int)in[6], (int)in[7], in[8] != 0);
    const int b0 = wfm::planned_meet_block(sum, T);
    wfm::Node nd{};
    nd.score_rem = (int32_t)in[5]; nd.cb = (int32_t)in[6]; nd.ce = (int32_t)in[7]; nd.sub = (int32_t)in[9]; nd.meet = sum;
    wfm::RingPlan rp;
    rp.fits = in[10] != 0; rp.tile_it = in[11] != 0; rp.grown = in[12] != 0;
    out[0] = sum; out[1] = m.sf; out[2] = m.sr; out[3] = m.last_fwd; out[4] = b0; out[5] = m.sf - b0; out[6] = m.sr - b0;
    out[7] = wfm::planned_meet_eligible(nd, rp, in[13] != 0, (int)in[14], T) ? 1 : 0;
  }
  return 0;
}

// test hook: plan_tile_chunk with a direction mask per job (dirs: n bytes, bit 0 forward, bit 1 reverse); everything else as wfmh_test_tile_plan
int wfmh_test_tile_plan_dirs(const int32_t* jobs, int64_t n, const int32_t* rules, const uint8_t* dirs, int32_t* per_block, int32_t* tasks, int64_t tasks_cap,
                             int64_t* scalars) {
  wfm::TilePlanRules r{rules[0], rules[1], rules[2], rules[3], rules[4], rules[5] != 0, rules[6] != 0, rules[7] != 0};
  if (r.chunk < 1 || r.T < 1 || r.threads < 1 || r.C < 1 || r.core < 1) return -1;
  wfm::TileChunkPlan p;
  wfm::plan_tile_chunk(reinterpret_cast<const wfm::TilePlanJob*>(jobs), (size_t)n, r, p, dirs);
  std::copy(p.threads_b.begin(), p.threads_b.end(), per_block);
  std::copy(p.variants_b.begin(), p.variants_b.end(), per_block + r.chunk);
  memcpy(tasks, p.tasks.data(), std::min<size_t>(p.tasks.size(), (size_t)tasks_cap) * sizeof(wfm::TileTask));
  scalars[0] = p.core_c; scalars[1] = (int64_t)p.tasks.size(); scalars[2] = (int64_t)p.n_pk;
  return 0;
}

// test hook: plan_p2_chunk (csrc/wfa_plan.h) with P2K = rows and P2ROWS = rows_bm.  cand: n x (pl, tl, sub, sf, sr, packed); geo: per job taken
// (koff2, w2, nblk, p2_off, bm_off); scalars = {jobs taken, elems, bm_elems, maxw2, threads_c, core_c, tasks, n_pk}
int wfmh_test_p2_plan(const int32_t* cand, int64_t n, int64_t i0, int rows, int rows_bm, unsigned long long budget, int threads, int core, int64_t* geo,
                      int32_t* tasks, int64_t tasks_cap, int64_t* scalars) {
  static_assert(sizeof(wfm::P2PlanJob) == 6 * sizeof(int32_t), "the hook copies these as rows of int32");
  if (i0 < 0 || i0 >= n || rows < 1 || threads < 1 || core < 1) return -1;
  wfm::P2ChunkPlan p;
  wfm::plan_p2_chunk(reinterpret_cast<const wfm::P2PlanJob*>(cand), (size_t)n, (size_t)i0, rows, rows_bm, (size_t)budget, threads, core, p);
  for (size_t q = 0; q < p.geo.size(); ++q) {
    const wfm::P2Geometry& g = p.geo[q];
    const int64_t v[5] = {g.koff2, (int64_t)g.w2, (int64_t)g.nblk, (int64_t)g.p2_off, (int64_t)g.bm_off};
    std::copy(v, v + 5, geo + 5 * q);
  }
  memcpy(tasks, p.tiles.tasks.data(), std::min<size_t>(p.tiles.tasks.size(), (size_t)tasks_cap) * sizeof(wfm::TileTask));
  const int64_t v[8] = {(int64_t)p.geo.size(), (int64_t)p.elems, (int64_t)p.bm_elems, (int64_t)p.maxw2, p.threads_c, p.tiles.core_c,
                        (int64_t)p.tiles.tasks.size(), (int64_t)p.tiles.n_pk};
  std::copy(v, v + 8, scalars);
  return 0;
}

// test hook: the base jobs' planners (csrc/wfa_plan.h).  op 0: base_kind -- in = n x (width, pl, tl, tries, acgt, base_v2, base_tiles, force_tiles,
// few_jobs, wide_from), out = the kind of each; op 1: plan_base_tiles -- in = T, threads, then n x (width, smax), out = core, nblocks, then ntiles of each
int wfmh_test_base_plan(int op, const int32_t* in, int64_t n, int32_t* out) {
  if (op == 0) {
    for (int64_t i = 0; i < n; ++i, in += 10)
      out[i] = wfm::base_kind(in[0], in[1], in[2], in[3], in[4] != 0, wfm::BaseRules{in[5] != 0, in[6] != 0, in[7] != 0, in[8] != 0, in[9]});
    return 0;
  }
  if (op != 1 || in[0] < 1 || in[1] * 2 <= 2 * in[0]) return -1;
  std::vector<int32_t> width((size_t)n), smax((size_t)n);
  for (int64_t i = 0; i < n; ++i) { width[(size_t)i] = in[2 + 2 * i]; smax[(size_t)i] = in[3 + 2 * i]; }
  const wfm::BaseTilePlan p = wfm::plan_base_tiles(width.data(), smax.data(), (size_t)n, in[0], in[1]);
  out[0] = p.core; out[1] = p.nblocks;
  std::copy(p.ntiles.begin(), p.ntiles.end(), out + 2);
  return 0;
}

char* wfmh_test_cigar(const char* fn, const char* a, const char* b, const char* query, const char* target,
                      long long i0, long long i1) {
  std::string f = fn ? fn : "", sa = a ? a : "", sb = b ? b : "", q = query ? query : "", t = target ? target : "";
  std::string r;
  const wflign::CigarOps o2 = wflign::parse_cigar(sb);
  wflign::CigarOps o = wflign::parse_cigar(sa);  // every CIGAR helper: parse, the run form, text
  auto erosion = [](const wflign::Erosion& e, size_t third) { return std::to_string(e.query_eroded) + "," + std::to_string(e.target_eroded) + "," + std::to_string(third); };
  if (f == "erode") { wflign::erode_short_matches_in_cigar(o, (int)i0, i1 != 0); r = wflign::cigar_to_string(o); }
  else if (f == "merge") { wflign::merge_adjacent_ops(o, o2, 0, o2.size()); r = wflign::cigar_to_string(o); }
  else if (f == "compress") r = wflign::compress_ops(sa.data(), sa.size());
  else if (f == "swap_start") { wflign::try_swap_start_pattern(o, q.data(), (int64_t)q.size(), t.data(), (int64_t)t.size()); r = wflign::cigar_to_string(o); }
  else if (f == "swap_end") { wflign::try_swap_end_pattern(o, q.data(), (int64_t)q.size(), t.data(), (int64_t)t.size()); r = wflign::cigar_to_string(o); }
  else if (f == "head_erosion") {  // third value: the text position behind the eroded runs
    const wflign::Erosion e = wflign::scan_head_erosion(o);
    r = erosion(e, wflign::cigar_to_string(o, 0, e.erode_end_pos).size());
  } else if (f == "tail_erosion") {
    const wflign::Erosion e = wflign::scan_tail_erosion(o);
    r = erosion(e, e.erode_start_idx);
  } else if (f == "patch_plan") {  // head erosion (third value: runs eroded), tail erosion, head wanted, tail wanted, tail independent
    const wflign::PatchPlan pl = wflign::plan_patches(o);
    r = erosion(pl.head, pl.head.erode_end_pos) + "," + erosion(pl.tail, pl.tail.erode_start_idx) + "," + std::to_string((int)pl.head_wanted) + "," +
        std::to_string((int)pl.tail_wanted) + "," + std::to_string((int)pl.tail_independent);
  } else if (f == "runs") {  // a = runs as decimal numbers separated by commas -> CIGAR text
    std::vector<uint32_t> runs;
    std::stringstream ss(sa);
    std::string item;
    while (std::getline(ss, item, ',')) if (!item.empty()) runs.push_back((uint32_t)std::stoul(item));
    wflign::ops_from_runs(runs.data(), runs.size(), o);
    r = wflign::cigar_to_string(o);
  } else if (f == "paf") {
    // b = qname|qtotal|qoff|qlen|qrev|tname|ttotal|toff|mmid|chain_id|chain_len|chain_pos
    std::vector<std::string> p;
    std::stringstream ss(sb);
    std::string item;
    while (std::getline(ss, item, '|')) p.push_back(item);
    if (p.size() == 12) {
      wflign::PafParams pp;
      wflign::write_alignment_paf(r, o, p[0], std::stoull(p[1]), std::stoull(p[2]), std::stoull(p[3]), p[4] == "1", p[5],
                                  std::stoull(p[6]), std::stoull(p[7]), pp, std::stof(p[8]), std::stoi(p[9]), std::stoi(p[10]),
                                  std::stoi(p[11]));
    }
  } else if (f == "min_hits") {   // a = "s,k,identity,ci"
    int sk = 0, k = 0; float id = 0, ci = 0;
    if (sscanf(sa.c_str(), "%d,%d,%f,%f", &sk, &k, &id, &ci) == 4)
      r = std::to_string(skch::Stat::estimateMinimumHits(sk, k, id)) + "," + std::to_string(skch::Stat::estimateMinimumHitsRelaxed(sk, k, id, ci));
  } else if (f == "sketch_cutoffs") {   // a = "s,k,ANIDiff,ANIDiffConf"
    int sk = 0, k = 0; float ad = 0, ac = 0;
    if (sscanf(sa.c_str(), "%d,%d,%f,%f", &sk, &k, &ad, &ac) == 4)
      for (int v : skch::Stat::sketch_cutoffs(sk, k, ad, ac)) { if (!r.empty()) r += ","; r += std::to_string(v); }
  } else if (f == "l2_tables") {   // a = "S,k,identity,ci": keep bits and nucIdentity x 1e4 for every (Q.sketchSize, shared)
    int S = 0, k = 0; float id = 0, ci = 0;
    if (sscanf(sa.c_str(), "%d,%d,%f,%f", &S, &k, &id, &ci) == 4) {
      std::vector<uint8_t> keep;
      std::vector<uint16_t> ident;
      skch::Stat::l2_identity_tables(S, k, id, true, ci, keep, ident);
      for (size_t i = 0; i < keep.size(); ++i) { if (i) r += ","; r += std::to_string((int)keep[i]) + ":" + std::to_string((int)ident[i]); }
    }
  } else if (f == "md") {
    r = wflign::md_string(o, 0, o.size(), (int)i0, t.c_str());
  } else if (f == "parse_row") {
    try {
      align::MappingBoundaryRow row;
      align::Aligner::parseMashmapRow(sa, row, (uint64_t)i0, (uint64_t)i1);
      std::ostringstream os;
      os << row.qId << "," << row.qStartPos << "," << row.qEndPos << "," << (row.strand == align::FWD ? "+" : "-") << ","
         << row.refId << "," << row.rStartPos << "," << row.rEndPos << "," << row.mashmap_estimated_identity << ","
         << row.chain_id << "," << row.chain_length << "," << row.chain_pos;
      r = os.str();
    } catch (const std::exception& e) { r = std::string("ERROR"); }
  }
  char* out = (char*)malloc(r.size() + 1);
  memcpy(out, r.c_str(), r.size() + 1);
  return out;
}

char* wfmh_test_fasta(const char* path, const char* name, int64_t start, int64_t end_inclusive, int whole) {
  std::string r;
  try {
    wfmash_host::FastaStore fa(path ? path : "");
    if (!name) {
      std::ostringstream os;
      os << (fa.indexed() ? "indexed" : "in-memory") << "\n";
      for (int i = 0; i < fa.nseq(); ++i) os << fa.name(i) << "\t" << fa.length(i) << "\n";
      r = os.str();
    } else {
      const int i = fa.find(name);
      if (i < 0) r = "ERROR: no such sequence";
      else {
        if (whole) fa.preload({i}, std::max(2, whole));  // whole > 1: that many reader threads
        r = fa.fetch(name, start, end_inclusive);
      }
    }
  } catch (const std::exception& e) {
    r = std::string("ERROR: ") + e.what();
  }
  char* out = (char*)malloc(r.size() + 1);
  if (!out) return nullptr;
  memcpy(out, r.data(), r.size());
  out[r.size()] = 0;
  return out;
}

}  // extern "C"

void wfmh_release_sequences(void) { wfmash_host::release_kept(); }

char* wfmh_test_fasta_shared(const char* path, const char* name) {
  std::string r;
  try {
    std::shared_ptr<wfmash_host::FastaStore> fa = wfmash_host::open_shared(path ? path : "");
    const int i = name ? fa->find(name) : -1;
    if (i < 0) r = "ERROR: no such sequence";
    else { const wfmash_host::SeqView v = fa->sequence(i, 1); r.assign(v.data(), v.size()); }
    wfmash_host::keep_until_next({fa});
  } catch (const std::exception& e) {
    r = std::string("ERROR: ") + e.what();
  }
  char* out = (char*)malloc(r.size() + 1);
  if (!out) return nullptr;
  memcpy(out, r.data(), r.size());
  out[r.size()] = 0;
  return out;
}
