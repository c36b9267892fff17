// capi_map.cpp -- C entry points of the map phase's host side (include/wfmash_host.h).
#include <chrono>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/wfmash_host.h"
#include "../csrc/wfa_handle.h"
#include "ani_estimate.hpp"
#include "capi_map.hpp"
#include "external_seeds.hpp"
#include "fasta.hpp"
#include "index_file.hpp"
#include "map_filter.hpp"
#include "map_plan.hpp"
#include "mapper.hpp"
#include "sequence_ids.hpp"

namespace wfmash_host {

skch::Parameters to_parameters(const wfmh_map_params_t& c) {
  skch::Parameters p;
  p.kmerSize = c.kmer_size;
  p.windowLength = c.window_length;
  p.block_length = c.block_length;
  p.chain_gap = c.chain_gap;
  p.max_mapping_length = c.max_mapping_length;
  p.percentageIdentity = c.percentage_identity;
  p.sketchSize = c.sketch_size;
  p.filterMode = c.filter_mode;
  p.numMappingsForSegment = c.num_mappings_for_segment;
  p.numMappingsForScaffold = c.num_mappings_for_scaffold;
  p.dropRand = c.drop_rand != 0;
  p.split = c.split != 0;
  p.mergeMappings = c.merge_mappings != 0;
  p.skip_self = c.skip_self != 0;
  p.skip_prefix = c.skip_prefix != 0;
  p.lower_triangular = c.lower_triangular != 0;
  p.prefix_delim = c.prefix_delim;
  p.filterLengthMismatches = c.filter_length_mismatches != 0;
  p.sparsity_hash_threshold = c.sparsity_hash_threshold;
  p.overlap_threshold = c.overlap_threshold;
  p.scaffold_overlap_threshold = c.scaffold_overlap_threshold;
  p.scaffold_max_deviation = c.scaffold_max_deviation;
  p.scaffold_gap = c.scaffold_gap;
  p.scaffold_min_length = c.scaffold_min_length;
  p.legacy_output = c.legacy_output != 0;
  p.minimum_hits = c.minimum_hits;
  p.max_kmer_freq = c.max_kmer_freq;
  p.index_by_size = c.index_by_size;
  p.kmerComplexityThreshold = c.kmer_complexity_threshold;
  p.stage1_topANI_filter = c.stage1_topani_filter != 0;
  p.stage2_full_scan = c.stage2_full_scan != 0;
  p.ANIDiff = c.ani_diff;
  p.ANIDiffConf = c.ani_diff_conf;
  p.hgNumerator = c.hg_numerator;
  p.threads = c.threads;
  p.auto_pct_identity = c.auto_pct_identity != 0;
  p.ani_percentile = c.ani_percentile;
  p.ani_adjustment = c.ani_adjustment;
  if (c.target_prefix) p.target_prefix = c.target_prefix;
  if (c.target_list) p.target_list = c.target_list;
  if (c.query_list) p.query_list = c.query_list;
  if (c.index_file) { p.indexFilename = c.index_file; p.create_index_only = c.write_index != 0; }
  if (c.scaffold_out) p.scaffold_output_file = c.scaffold_out;
  p.use_streaming_minhash = c.streaming_minhash != 0;
  if (c.query_prefix) {  // CommonFunc::split(args::get(query_prefix), ',') (parse_args.hpp:204)
    std::stringstream ss(c.query_prefix);
    for (std::string tok; std::getline(ss, tok, ',');) p.query_prefix.push_back(tok);
  }
  return p;
}

namespace {
skch::SequenceIdManager make_id_manager(const skch::Parameters& p) {
  std::vector<std::string> target_prefix_vec;
  if (!p.target_prefix.empty()) target_prefix_vec.push_back(p.target_prefix);
  return skch::SequenceIdManager(p.querySequences, p.refSequences, p.query_prefix, target_prefix_vec, std::string(1, p.prefix_delim), p.query_list,
                                 p.target_list);
}

void write_text_file(const std::string& path, const std::string& text) {
  std::ofstream f(path, std::ios::binary);
  if (!f.is_open()) throw std::runtime_error("cannot open " + path + " for writing");
  f << text;
  f.close();
  if (!f) throw std::runtime_error("writing " + path + " failed");
}

// wfmh_set_ani_matrix: where the next map call writes the ANI table (empty: nowhere)
std::mutex g_ani_out_mu;
std::string g_ani_out;
std::string take_ani_matrix_out() {
  std::lock_guard<std::mutex> lk(g_ani_out_mu);
  std::string s;
  s.swap(g_ani_out);
  return s;
}

// what wfmh_map_multi does up to its sketches, then the table instead of the mapping
std::vector<skch::Stat::AniRow> ani_matrix_of_files(wfm_handle_t* const* handles, int n, const char* target_fasta, const char* query_fasta,
                                                    const wfmh_map_params_t* params) {
  wfmh_map_params_t def;
  wfmh_map_default_params(&def);
  skch::Parameters p = to_parameters(params ? *params : def);
  p.refSequences = {std::string(target_fasta)};
  p.querySequences = {std::string(query_fasta ? query_fasta : target_fasta)};
  std::vector<std::shared_ptr<FastaStore>> files;
  for (const auto& f : p.refSequences) files.push_back(open_shared(f));
  for (const auto& f : p.querySequences) files.push_back(open_shared(f));
  const skch::SequenceIdManager ids = make_id_manager(p);
  return skch::Stat::ani_matrix(p, ids, std::vector<wfm_handle_t*>(handles, handles + n));
}
}  // namespace

}  // namespace wfmash_host

extern "C" {

void wfmh_map_default_params(wfmh_map_params_t* c) {
  if (!c) return;
  const skch::Parameters p;  // the defaults live in one place (map_types.hpp)
  std::memset(c, 0, sizeof(*c));
  c->kmer_size = p.kmerSize;
  c->window_length = p.windowLength;
  c->block_length = p.block_length;
  c->chain_gap = p.chain_gap;
  c->max_mapping_length = p.max_mapping_length;
  c->percentage_identity = p.percentageIdentity;
  c->sketch_size = p.sketchSize;
  c->filter_mode = p.filterMode;
  c->num_mappings_for_segment = p.numMappingsForSegment;
  c->num_mappings_for_scaffold = p.numMappingsForScaffold;
  c->drop_rand = p.dropRand;
  c->split = p.split;
  c->merge_mappings = p.mergeMappings;
  c->skip_self = p.skip_self;
  c->skip_prefix = p.skip_prefix;
  c->lower_triangular = p.lower_triangular;
  c->prefix_delim = p.prefix_delim;
  c->filter_length_mismatches = p.filterLengthMismatches;
  c->sparsity_hash_threshold = p.sparsity_hash_threshold;
  c->overlap_threshold = p.overlap_threshold;
  c->scaffold_overlap_threshold = p.scaffold_overlap_threshold;
  c->scaffold_max_deviation = p.scaffold_max_deviation;
  c->scaffold_gap = p.scaffold_gap;
  c->scaffold_min_length = p.scaffold_min_length;
  c->legacy_output = p.legacy_output;
  c->minimum_hits = p.minimum_hits;
  c->max_kmer_freq = p.max_kmer_freq;
  c->index_by_size = p.index_by_size;
  c->kmer_complexity_threshold = p.kmerComplexityThreshold;
  c->stage1_topani_filter = p.stage1_topANI_filter;
  c->stage2_full_scan = p.stage2_full_scan;
  c->ani_diff = p.ANIDiff;
  c->ani_diff_conf = p.ANIDiffConf;
  c->hg_numerator = p.hgNumerator;
  c->threads = p.threads;
  c->auto_pct_identity = p.auto_pct_identity;
  c->ani_percentile = p.ani_percentile;
  c->ani_adjustment = p.ani_adjustment;
  c->streaming_minhash = p.use_streaming_minhash;
}

int wfmh_map(wfm_handle_t* h, const char* target_fasta, const char* query_fasta, const char* out_paf, const wfmh_map_params_t* params,
             wfmh_map_summary_t* summary) {
  return wfmh_map_multi(&h, 1, target_fasta, query_fasta, out_paf, params, summary);
}

int wfmh_map_multi(wfm_handle_t* const* handles, int n, const char* target_fasta, const char* query_fasta, const char* out_paf,
                   const wfmh_map_params_t* params, wfmh_map_summary_t* summary) {
  if (!handles || n < 1 || !target_fasta || !out_paf) return WFM_E_ARG;
  for (int i = 0; i < n; ++i) if (!handles[i]) return WFM_E_ARG;
  wfm_handle_t* h = handles[0];
  try {
    wfmh_map_params_t def;
    wfmh_map_default_params(&def);
    skch::Parameters p = wfmash_host::to_parameters(params ? *params : def);
    p.refSequences = {std::string(target_fasta)};
    p.querySequences = {std::string(query_fasta ? query_fasta : target_fasta)};
    p.outFileName = out_paf;
    const auto t_open = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    int rc;
    double ms_opened = 0, ms_mapped = 0;
    {
      // the files stay open (and what is loaded of them stays loaded) from the identity estimate through the mapping
      std::vector<std::shared_ptr<wfmash_host::FastaStore>> files;
      for (const auto& f : p.refSequences) files.push_back(wfmash_host::open_shared(f));
      for (const auto& f : p.querySequences) files.push_back(wfmash_host::open_shared(f));
      ms_opened = ms_since(t_open);
      const auto t_call = std::chrono::steady_clock::now();
      double ms_identity = 0;
      // the normalised device copies of the chromosomes stay from the identity estimate's sketches to the index build and the queries' fragments
      // (wfm_map_sequence_cache); the scope ends before the files are let go
      // -- on every handle: each device sketches its share of the index and finds there what its share of the estimate left
      struct SeqCacheScope {
        wfm_handle_t* const* hs; int n;
        SeqCacheScope(wfm_handle_t* const* hh, int nn) : hs(hh), n(nn) { for (int i = 0; i < n; ++i) (void)wfm_map_sequence_cache(hs[i], 1); }
        ~SeqCacheScope() { for (int i = n - 1; i >= 0; --i) (void)wfm_map_sequence_cache(hs[i], 0); }
      } seq_cache_scope(handles, n);
      const std::string ani_tsv_out = wfmash_host::take_ani_matrix_out();  // wfmh_set_ani_matrix: empty unless asked for
      if (p.auto_pct_identity || !ani_tsv_out.empty()) {
        // main.cpp:72-128: estimate, then derive the sketch size from the estimate unless -s was given
        const skch::SequenceIdManager ids = wfmash_host::make_id_manager(p);
        const skch::Stat::GroupSketches gs = skch::Stat::sketch_groups(p, ids, std::vector<wfm_handle_t*>(handles, handles + n));
        // the table and the estimate are made from the same sketches; the table changes nothing the mapping reads
        if (!ani_tsv_out.empty()) wfmash_host::write_text_file(ani_tsv_out, skch::Stat::ani_tsv(skch::Stat::ani_matrix_from(gs, ids, h)));
        if (p.auto_pct_identity) p.percentageIdentity = skch::Stat::estimate_identity_from(gs, p);
        ms_identity = ms_since(t_call);
      }
      skch::Map mapper(p, std::vector<wfm_handle_t*>(handles, handles + n));
      skch::MapSummary s;
      rc = mapper.mapQuery(&s);
      if (summary) {
        summary->targets = s.targets; summary->queries = s.queries; summary->subsets = s.subsets;
        summary->target_bp = s.target_bp; summary->query_bp = s.query_bp; summary->index_windows = s.index_windows;
        summary->fragments = s.fragments; summary->l2_mappings = s.l2_mappings; summary->written = s.written;
        summary->percentage_identity = mapper.parameters().percentageIdentity;
        summary->sketch_size = mapper.parameters().sketchSize;
        summary->ms_index = s.ms_index; summary->ms_map = s.ms_map; summary->ms_filter = s.ms_filter; summary->ms_total = s.ms_total;
        summary->ms_replicate = s.ms_replicate;
        summary->index_parts = s.index_parts; summary->pad_ = 0;
        summary->ms_index_sketch = s.ms_index_sketch; summary->ms_index_merge = s.ms_index_merge;
        summary->ms_identity = ms_identity;
        summary->ms_wall = ms_since(t_call);
      }
      ms_mapped = ms_since(t_open);
      // the sequences (gigabytes for a pangenome) stay loaded for the call that follows -- the align phase, as a rule, which
      // fetches its windows from the same files -- and what was kept before goes back to the system on a thread of its own
      wfmash_host::keep_until_next(std::move(files));
    }
    if (getenv("WFM_DEBUG"))
      fprintf(stderr, "[wfm] map call: files opened after %.1f ms, mapped after %.1f ms, returning after %.1f ms\n", ms_opened, ms_mapped, ms_since(t_open));
    return rc;
  } catch (const std::exception& e) {
    wfm_set_error(h, e.what());
    return WFM_E_ARG;
  }
}

void wfmh_set_ani_matrix(const char* out_tsv) {
  std::lock_guard<std::mutex> lk(wfmash_host::g_ani_out_mu);
  wfmash_host::g_ani_out = out_tsv ? out_tsv : "";
}

int wfmh_ani_matrix(wfm_handle_t* const* handles, int n, const char* target_fasta, const char* query_fasta, const wfmh_map_params_t* params,
                    const char* out_tsv) {
  if (!handles || n < 1 || !target_fasta || !out_tsv) return WFM_E_ARG;
  for (int i = 0; i < n; ++i) if (!handles[i]) return WFM_E_ARG;
  try {
    wfmash_host::write_text_file(out_tsv, skch::Stat::ani_tsv(wfmash_host::ani_matrix_of_files(handles, n, target_fasta, query_fasta, params)));
    return WFM_OK;
  } catch (const std::exception& e) {
    wfm_set_error(handles[0], e.what());
    return WFM_E_ARG;
  }
}

int wfmh_ani_matrix_rows(wfm_handle_t* const* handles, int n, const char* target_fasta, const char* query_fasta, const wfmh_map_params_t* params,
                         wfmh_ani_row_t** rows, int64_t* n_rows) {
  if (!handles || n < 1 || !target_fasta || !rows || !n_rows) return WFM_E_ARG;
  for (int i = 0; i < n; ++i) if (!handles[i]) return WFM_E_ARG;
  *rows = nullptr;
  *n_rows = 0;
  try {
    const std::vector<skch::Stat::AniRow> r = wfmash_host::ani_matrix_of_files(handles, n, target_fasta, query_fasta, params);
    wfmh_ani_row_t* out = (wfmh_ani_row_t*)std::calloc(std::max<size_t>(r.size(), 1), sizeof(wfmh_ani_row_t));
    if (!out) return WFM_E_NOMEM;
    for (size_t i = 0; i < r.size(); ++i) {
      out[i].query_group = strdup(r[i].query_group.c_str());
      out[i].target_group = strdup(r[i].target_group.c_str());
      out[i].query_hashes = r[i].query_hashes; out[i].target_hashes = r[i].target_hashes; out[i].shared = r[i].shared;
      out[i].jaccard = r[i].jaccard; out[i].ani = r[i].ani;
    }
    *rows = out;
    *n_rows = (int64_t)r.size();
    return WFM_OK;
  } catch (const std::exception& e) {
    wfm_set_error(handles[0], e.what());
    return WFM_E_ARG;
  }
}

void wfmh_free_ani_rows(wfmh_ani_row_t* rows, int64_t n_rows) {
  if (!rows) return;
  for (int64_t i = 0; i < n_rows; ++i) { std::free(rows[i].query_group); std::free(rows[i].target_group); }
  std::free(rows);
}

char* wfmh_test_ani_tsv(const char* const* query_groups, const char* const* target_groups, const uint64_t* query_hashes, const uint64_t* target_hashes,
                        const uint64_t* shared, int64_t n) {
  std::vector<skch::Stat::AniRow> rows;
  for (int64_t i = 0; i < n; ++i) rows.push_back(skch::Stat::ani_row(query_groups[i], target_groups[i], query_hashes[i], target_hashes[i], shared[i]));
  return strdup(skch::Stat::ani_tsv(rows).c_str());
}

int wfmh_seed_paf(const char* target_fasta, const char* query_fasta, const char* seeds_paf, const char* out_paf, const wfmh_map_params_t* params,
                  wfmh_map_summary_t* summary) {
  if (!target_fasta || !seeds_paf || !out_paf) return WFM_E_ARG;
  const auto t_call = std::chrono::steady_clock::now();
  try {
    wfmh_map_params_t def;
    wfmh_map_default_params(&def);
    skch::Parameters p = wfmash_host::to_parameters(params ? *params : def);
    p.refSequences = {std::string(target_fasta)};
    p.querySequences = {std::string(query_fasta ? query_fasta : target_fasta)};
    p.outFileName = out_paf;
    // the id manager the reference's -K branch makes (main.cpp:172-188): names and lengths only, no index
    std::vector<std::string> target_prefix_vec;
    if (!p.target_prefix.empty()) target_prefix_vec.push_back(p.target_prefix);
    const skch::SequenceIdManager ids(p.querySequences, p.refSequences, p.query_prefix, target_prefix_vec, std::string(1, p.prefix_delim),
                                      p.query_list, p.target_list);
    const bool to_stdout = p.outFileName == "/dev/stdout" || p.outFileName == "-";
    std::ofstream file;
    if (!to_stdout) {
      file.open(p.outFileName);
      if (!file.is_open()) throw std::runtime_error("Could not open output file: " + p.outFileName);
    }
    std::ofstream scaffolds;
    if (!p.scaffold_output_file.empty()) {
      scaffolds.open(p.scaffold_output_file);
      if (!scaffolds.is_open()) throw std::runtime_error("cannot open scaffold output file " + p.scaffold_output_file);
    }
    skch::SeedSummary s;
    skch::processExternalSeeds(p, seeds_paf, ids, to_stdout ? static_cast<std::ostream&>(std::cout) : file,
                               scaffolds.is_open() ? &scaffolds : nullptr, &s);
    if ((!to_stdout && !file) || (scaffolds.is_open() && !scaffolds)) throw std::runtime_error("writing the output failed");
    if (summary) {
      std::memset(summary, 0, sizeof(*summary));
      summary->targets = ids.getTargetSequenceNames().size();
      summary->queries = s.queries;
      summary->l2_mappings = s.seeds;
      summary->written = s.written;
      summary->percentage_identity = p.percentageIdentity;
      summary->sketch_size = p.sketchSize;
      summary->ms_map = s.ms_read;
      summary->ms_filter = s.ms_filter;
      summary->ms_total = summary->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    }
    return WFM_OK;
  } catch (const std::bad_alloc&) {
    fprintf(stderr, "[wfmash::externalSeeder] ERROR: out of host memory\n");
    return WFM_E_NOMEM;
  } catch (const std::exception& e) {
    fprintf(stderr, "[wfmash::externalSeeder] ERROR: %s\n", e.what());
    return WFM_E_ARG;
  }
}

int wfmh_test_deal(const int64_t* lengths, int64_t n, int n_parts, int32_t* out_part) {
  if (n < 0 || n_parts < 1 || (n && (!lengths || !out_part))) return WFM_E_ARG;
  const std::vector<int> part = skch::deal_longest_first(lengths, n, n_parts);
  for (int64_t i = 0; i < n; ++i) out_part[i] = part[(size_t)i];
  return WFM_OK;
}

int wfmh_test_map_plan(int op, const int64_t* in, int64_t n, int64_t* out) {
  namespace mp = skch::map_plan;
  if (!in || !out || n < 0) return WFM_E_ARG;
  auto spans = [&](int64_t nq, const int64_t* v) {
    std::vector<mp::BatchQuery> bq((size_t)nq);
    for (int64_t i = 0; i < nq; ++i) bq[(size_t)i] = {(size_t)i, (skch::seqno_t)i, 0, 0, v[2 * i], (int)v[2 * i + 1]};
    return bq;
  };
  switch (op) {
    case 0: {  // layout_fragments
      if (n != 4 || in[1] < 1) return WFM_E_ARG;
      const mp::FragLayout fl = mp::layout_fragments(in[0], in[1], in[2], in[3]);
      out[0] = fl.nfrag;
      std::copy(fl.offsets.begin(), fl.offsets.end(), out + 1);
      return WFM_OK;
    }
    case 1: {  // target_subsets; the names are their positions
      if (n < 1) return WFM_E_ARG;
      std::vector<std::string> names;
      for (int64_t i = 1; i < n; ++i) names.push_back(std::to_string(i - 1));
      const auto subsets = mp::target_subsets(names, std::vector<int64_t>(in + 1, in + n), in[0]);
      int64_t next = 0;
      out[0] = (int64_t)subsets.size();
      for (size_t s = 0; s < subsets.size(); ++s) {
        for (const auto& name : subsets[s]) if (name != std::to_string(next++)) return WFM_E_ARG;  // (in order, each once)
        out[1 + s] = (int64_t)subsets[s].size();
      }
      return WFM_OK;
    }
    case 2: {  // plan_batch
      if (n < 2 || in[1] < 0 || in[1] > n - 2) return WFM_E_ARG;
      const mp::BatchPlan p = mp::plan_batch(in + 2, (size_t)(n - 2), (size_t)in[1], in[0]);
      out[0] = (int64_t)p.next; out[1] = p.in_place; out[2] = p.n_bases; out[3] = (int64_t)p.members.size();
      for (size_t i = 0; i < p.members.size(); ++i) out[4 + i] = (int64_t)p.members[i];
      return WFM_OK;
    }
    case 3:  // batch_bases_for, mapping_cap, spare_hint and the thresholds
      if (n != 4 || in[0] < 1) return WFM_E_ARG;
      out[0] = mp::batch_bases_for((size_t)in[0], (uint64_t)in[1]);
      out[1] = mp::mapping_cap(in[2], in[3]);
      out[2] = (int64_t)mp::spare_hint((size_t)in[2], in[3]);
      out[3] = mp::kBatchBases; out[4] = mp::kCopyBases; out[5] = (int64_t)mp::kEarlyFilterFrags; out[6] = (int64_t)mp::kSpareMappings;
      return WFM_OK;
    case 4: {  // split_by_query
      if (n < 1 || in[0] < 0 || n < 1 + 2 * in[0]) return WFM_E_ARG;
      const int64_t nq = in[0], nm = n - 1 - 2 * nq;
      std::vector<int32_t> mfrag(in + 1 + 2 * nq, in + n);
      const std::vector<size_t> first = mp::split_by_query(mfrag.data(), (size_t)nm, spans(nq, in + 1));
      for (size_t i = 0; i < first.size(); ++i) out[i] = (int64_t)first[i];
      return WFM_OK;
    }
    case 5: {  // query_results
      if (n < 7) return WFM_E_ARG;
      const int64_t first_frag = in[0], w = in[1], m0 = in[2], nq = in[3], threads = in[4], has_perm = in[5], nm = in[6];
      if (nm < 0 || n != 7 + 3 * nm || m0 < 0 || nq < 0 || m0 + nq > nm) return WFM_E_ARG;
      std::vector<wfm_mapping_t> maps((size_t)nm);
      std::vector<int32_t> mfrag((size_t)nm);
      std::vector<uint32_t> perm((size_t)nm);
      for (int64_t i = 0; i < nm; ++i) {
        std::memset(&maps[(size_t)i], 0, sizeof(wfm_mapping_t));
        mfrag[(size_t)i] = (int32_t)in[7 + i];
        perm[(size_t)i] = (uint32_t)in[7 + nm + i];
        maps[(size_t)i].queryStartPos = (uint32_t)in[7 + 2 * nm + i];
        maps[(size_t)i].refStartPos = (uint32_t)i;  // which mapping a result was
      }
      skch::MappingResultsVector_t res(3);  // (stale content, as a reused vector has)
      std::vector<uint32_t> orig(2, 7u);
      mp::query_results(maps.data(), mfrag.data(), has_perm ? perm.data() : nullptr, (size_t)m0, (size_t)nq, first_frag, w, res, orig, (int)threads);
      if ((int64_t)res.size() != nq || !(orig.empty() || (int64_t)orig.size() == nq)) return WFM_E_ARG;
      out[0] = (int64_t)orig.size();
      for (int64_t i = 0; i < nq; ++i) { out[1 + i] = res[(size_t)i].refStartPos; out[1 + nq + i] = res[(size_t)i].queryStartPos; }
      for (size_t i = 0; i < orig.size(); ++i) out[1 + 2 * nq + (int64_t)i] = orig[i];
      return WFM_OK;
    }
    default:
      return WFM_E_ARG;
  }
}

namespace {

// the body of wfmh_test_filter and wfmh_test_filter_ordered
char* test_filter(const char* stage, const wfm_mapping_t* maps, int64_t n, const uint32_t* orig, const char* fasta, const char* query_name,
                  const wfmh_map_params_t* prm) {
  if (!stage || !fasta || !query_name || !prm || n < 0 || (n && !maps)) return nullptr;
  std::string text;
  try {
    const skch::Parameters p = wfmash_host::to_parameters(*prm);
    const std::string delim = p.prefix_delim ? std::string(1, p.prefix_delim) : std::string();
    const skch::SequenceIdManager ids({std::string(fasta)}, {std::string(fasta)}, {}, {std::string()}, delim);
    skch::MappingResultsVector_t v((size_t)n);
    if (n) std::memcpy(v.data(), maps, (size_t)n * sizeof(wfm_mapping_t));
    skch::set_filter_threads(getenv("WFM_FILTER_THREADS") ? atoi(getenv("WFM_FILTER_THREADS")) : 1);  // tests: the split passes
    const skch::seqno_t qid = ids.getSequenceId(query_name);
    const skch::offset_t qlen = ids.getSequenceLength(qid);
    std::ostringstream os;
    const std::string st(stage);
    if (st == "subset") {
      skch::MappingOutput::mappingBoundarySanityCheck(qlen, v, ids);
      skch::FilteredMappingsResult r = skch::filterSubsetMappings(v, p, ids, qlen, orig);
      const bool merged = p.mergeMappings && p.split;
      skch::MappingOutput::reportReadMappings(merged ? r.mergedMappings : r.nonMergedMappings, merged ? r.mergedChainInfo : r.nonMergedChainInfo,
                                              query_name, os, ids, p, qlen);
    } else if (st == "onetoone" && !orig) {
      skch::MappingResultsVector_t kept;
      skch::MappingFilterUtils::filterByGroup(v, kept, p.numMappingsForSegment - 1, true, ids, p);
      skch::MappingOutput::reportReadMappings(kept, query_name, os, ids, p, qlen);
    } else {
      return nullptr;
    }
    text = os.str();
  } catch (const std::exception& e) {
    text = std::string("ERROR: ") + e.what();
  }
  char* out = (char*)malloc(text.size() + 1);
  if (out) std::memcpy(out, text.c_str(), text.size() + 1);
  return out;
}

}  // namespace

char* wfmh_test_filter(const char* stage, const wfm_mapping_t* maps, int64_t n, const char* fasta, const char* query_name,
                       const wfmh_map_params_t* prm) {
  return test_filter(stage, maps, n, nullptr, fasta, query_name, prm);
}

char* wfmh_test_filter_ordered(const char* stage, const wfm_mapping_t* maps, int64_t n, const uint32_t* orig, const char* fasta,
                               const char* query_name, const wfmh_map_params_t* prm) {
  if (n && !orig) return nullptr;
  return test_filter(stage, maps, n, n ? orig : nullptr, fasta, query_name, prm);
}

// Test hook for the on-disk index (host/index_file.cpp; no GPU needed).  op "ids": the id section alone
// (SequenceIdManager::exportIdMapping) of `fasta`'s sequences into out_path.  op "rewrite": every sub-index of
// in_path is read (read_sub_index, ids imported) and written again (write_sub_index) into out_path.
// Returns 0, or -1 with the message on stderr.
int wfmh_test_index_file(const char* op, const char* fasta, char prefix_delim, const char* in_path, const char* out_path) {
  if (!op || !fasta || !out_path) return -1;
  try {
    const std::string delim = prefix_delim ? std::string(1, prefix_delim) : std::string();
    skch::SequenceIdManager ids({std::string(fasta)}, {std::string(fasta)}, {}, {std::string()}, delim);
    std::ofstream out(out_path, std::ios::binary);
    if (!out) throw std::runtime_error("cannot open the output file");
    const std::string o(op);
    if (o == "ids") {
      ids.exportIdMapping(out);
    } else if (o == "rewrite") {
      if (!in_path) return -1;
      std::ifstream in(in_path, std::ios::binary);
      if (!in) throw std::runtime_error("cannot open the input file");
      uint64_t total = 1;
      for (uint64_t b = 0; b < total; ++b) {
        skch::SubIndex sub;
        skch::read_sub_index(in, sub, ids);
        total = sub.total_batches;
        skch::write_sub_index(out, sub, ids);
      }
    } else {
      return -1;
    }
    return out ? 0 : -1;
  } catch (const std::exception& e) {
    fprintf(stderr, "wfmh_test_index_file: %s\n", e.what());
    return -1;
  }
}

}  // extern "C"
