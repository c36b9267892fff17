// run_passes.cpp -- see run_passes.hpp: the stages over packed runs, the passes, and an aligned PAF through one of them.
#include "run_passes.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "../csrc/wfa_handle.h"
#include "genotype_text.hpp"
#include "maf_text.hpp"
#include "transitive_text.hpp"

namespace wflign {

namespace {
// a stage's or a pass's WFM_DEBUG line ("" where that is not set): its caller prints it or drops it
template <class... Args>
std::string debug_line(const char* fmt, Args... args) {
  if (!getenv("WFM_DEBUG")) return std::string();
  char buf[640];
  snprintf(buf, sizeof buf, fmt, args...);
  return buf;
}

// the frame of the stages that add to the object of the batch's handle: the call's return is the number of records it refused.  What
// differs between them beside that is how a problem is made of a packed record and which wfm_*_add takes them.
template <class Call>
StageOutcome add_stage(wfm_handle_t* h, size_t n, Clock::time_point& t1, Call call) {
  StageOutcome o;
  const int rc = device_call(h, n, t1, o.error, call);
  if (rc < 0) { o.rc = rc; return o; }
  o.counts[0] = n - (uint64_t)rc;
  o.refused = (uint64_t)rc;
  return o;
}
}  // namespace

// ---- --coverage: the packed runs into the depth object of the batch's handle (wfm_coverage_add) ----
StageOutcome coverage_records(wfm_handle_t* h, int, const BatchPasses& bp, PackedRuns& pk) {
  auto t0 = Clock::now(), t1 = t0;
  const size_t n = pk.size();
  std::vector<uint32_t> flags(n);
  StageOutcome o = add_stage(h, n, t1, [&] {
    return wfm_coverage_add(h, bp.get<wfm_coverage_t>(SW_COVERAGE), pk.probs.data(), n, pk.runs.data(), pk.runs.size(), flags.data());
  });
  if (o.rc >= 0)
    o.debug = debug_line("[wflign] coverage: %zu records, %zu runs, %d flagged, %.1f ms\n", n, pk.runs.size(), (int)o.refused, pk.ms + ms_between(t0, Clock::now()));
  return o;
}
// ---- --pav: the same problems into the presence object of the batch's handle, each with the column of its query's group (wfm_pav_add) ----
StageOutcome pav_records(wfm_handle_t* h, int, const BatchPasses& bp, PackedRuns& pk) {
  auto t0 = Clock::now(), t1 = t0;
  const size_t n = pk.size();
  std::vector<wfm_pav_prob_t> probs(n);
  for (size_t j = 0; j < n; ++j) probs[j] = wfm_pav_prob_t{pk.probs[j].base, pk.probs[j].runs_off, pk.probs[j].n_runs, pk.place[j].group};
  std::vector<uint32_t> flags(n);
  StageOutcome o = add_stage(h, n, t1, [&] {
    return wfm_pav_add(h, bp.get<wfm_pav_t>(SW_PAV), probs.data(), n, pk.runs.data(), pk.runs.size(), flags.data());
  });
  if (o.rc >= 0)
    o.debug = debug_line("[wflign] pav: %zu records, %zu runs, %d flagged, %.1f ms (runs %.1f, device call %.1f)\n", n, pk.runs.size(), (int)o.refused,
                         pk.ms + ms_between(t0, Clock::now()), pk.ms + ms_between(t0, t1), ms_between(t1, Clock::now()));
  return o;
}
// ---- --lift: the BED intervals through the same problems (wfm_lift_runs).  The lines of a record go into pk.lift in the order the device
// gives them: ascending interval.  A record the device refuses has no lines. ----
StageOutcome lift_records(wfm_handle_t* h, int threads, const BatchPasses& bp, PackedRuns& pk) {
  auto t0 = Clock::now(), t1 = t0;
  const size_t n = pk.size();
  pk.lift.assign(n, std::string());
  std::vector<lift::Record> where(n);
  for (size_t j = 0; j < n; ++j) {
    const chain::Record& cr = pk.where[j];
    lift::Record& lr = where[j];
    lr.qname = cr.qname; lr.tname = cr.tname; lr.rev = cr.rev;
    lr.qs = cr.qs; lr.qe = cr.qe; lr.ts = cr.ts;
  }
  wfm_lift_t* lifts = nullptr;
  size_t n_lifts = 0;
  std::vector<wfm_liftcall_t> per(n);
  StageOutcome o;
  o.rc = device_call(h, n, t1, o.error, [&] {
    return wfm_lift_runs(h, bp.get<const wfm_liftset_t>(SW_LIFT), pk.probs.data(), n, pk.runs.data(), pk.runs.size(), &lifts, &n_lifts, per.data());
  });
  if (o.rc < 0) return o;
  const auto t2 = Clock::now();
  const std::vector<lift::Interval>& iv = bp.tables->lift_iv;
  std::atomic<uint64_t> lines{0}, empty{0}, refused{0};
  for_each_record(n, threads, [&](size_t j) {
    if (per[j].flags) { refused += 1; return; }
    std::string& out = pk.lift[j];
    uint64_t e = 0;
    for (uint64_t k = per[j].first; k < per[j].first + per[j].count; ++k) {
      const wfm_lift_t& l = lifts[k];
      lift::lift_line(out, where[j], iv[l.interval], l.p0, l.p1, l.t0, l.t1, l.eq, l.x);
      e += l.eq + l.x == 0;
    }
    lines += per[j].count; empty += e;
  });
  wfm_free_lifts(lifts);
  o.refused = refused.load();
  o.counts[0] = n - o.refused; o.counts[1] = lines.load(); o.counts[2] = empty.load();
  o.debug = debug_line("[wflign] lift: %zu records, %zu runs, %zu lifts, %.1f ms (runs %.1f, device call %.1f, text %.1f)\n", n, pk.runs.size(), n_lifts,
                       pk.ms + ms_between(t0, Clock::now()), pk.ms + ms_between(t0, t1), ms_between(t1, t2), ms_between(t2, Clock::now()));
  return o;
}
// ---- --chain: the same problems compacted to the blocks and gaps of a UCSC chain (wfm_chain_runs).  swap: the query is the chain's first
// side (chain_text.hpp).  A record's chain goes into pk.chain without its id, which the ordered writer gives it.  A record the device
// refuses has no chain. ----
static_assert(sizeof(chain::Block) == sizeof(wfm_chain_block_t), "chain_text.hpp restates wfm_chain_block_t");
StageOutcome chain_records(wfm_handle_t* h, int threads, const BatchPasses& bp, PackedRuns& pk) {
  auto t0 = Clock::now(), t1 = t0;
  const bool swap = bp.tables->chain_swap;
  const size_t n = pk.size();
  pk.chain.assign(n, std::string());
  std::vector<wfm_chain_prob_t> probs(n);
  for (size_t j = 0; j < n; ++j) probs[j] = wfm_chain_prob_t{pk.probs[j].runs_off, pk.probs[j].n_runs, chain::flags_of(swap, pk.where[j].rev)};
  wfm_chain_block_t* blocks = nullptr;
  size_t n_blocks = 0;
  std::vector<wfm_chaincall_t> per(n);
  StageOutcome o;
  o.rc = device_call(h, n, t1, o.error, [&] { return wfm_chain_runs(h, probs.data(), n, pk.runs.data(), pk.runs.size(), &blocks, &n_blocks, per.data()); });
  if (o.rc < 0) return o;
  const auto t2 = Clock::now();
  std::atomic<uint64_t> chains{0}, refused{0};
  for_each_record(n, threads, [&](size_t j) {
    if (per[j].flags) { refused += 1; return; }
    chain::Ends e;
    e.lead_dt = per[j].lead_dt; e.lead_dq = per[j].lead_dq; e.trail_dt = per[j].trail_dt; e.trail_dq = per[j].trail_dq; e.eq = per[j].eq;
    chain::chain_body(pk.chain[j], pk.where[j], swap, e, (const chain::Block*)blocks + per[j].first, per[j].count);
    chains += per[j].count != 0;
  });
  wfm_free_chain(blocks);
  o.refused = refused.load();
  o.counts[0] = chains.load(); o.counts[1] = n_blocks; o.counts[2] = o.refused;
  o.debug = debug_line("[wflign] chain: %zu records, %zu runs, %zu blocks, %.1f ms (runs %.1f, device call %.1f, text %.1f)\n", n, pk.runs.size(), n_blocks,
                       pk.ms + ms_between(t0, Clock::now()), pk.ms + ms_between(t0, t1), ms_between(t1, t2), ms_between(t2, Clock::now()));
  return o;
}
// ---- --chain-net: the same problems into the net object of the batch's handle (wfm_net_add), each with score = its = columns (counted
// on the device) and order = the batch's order base + its index among the records packed: the key the file is sorted by.  What the chain's
// header needs of every record added goes to pk.net_heads. ----
StageOutcome net_records(wfm_handle_t* h, int, const BatchPasses& bp, PackedRuns& pk) {
  auto t0 = Clock::now(), t1 = t0;
  const size_t n = pk.size();
  std::vector<wfm_net_prob_t> probs(n);
  for (size_t j = 0; j < n; ++j)
    probs[j] = wfm_net_prob_t{pk.probs[j].base, pk.probs[j].runs_off, pk.probs[j].n_runs, WFM_NET_SCORE_EQ, pk.order_base + (uint64_t)j};
  std::vector<uint32_t> flags(n);
  StageOutcome o = add_stage(h, n, t1, [&] {
    return wfm_net_add(h, bp.get<wfm_net_t>(SW_CHAIN_NET), probs.data(), n, pk.runs.data(), pk.runs.size(), flags.data());
  });
  if (o.rc < 0) return o;
  for (size_t j = 0; j < n; ++j)
    if (!flags[j]) pk.net_heads.push_back(NetHead{probs[j].order, pk.place[j].target_off, pk.where[j]});
  o.debug = debug_line("[wflign] chain-net: %zu records, %zu runs, %d flagged, %.1f ms (runs %.1f, device call %.1f)\n", n, pk.runs.size(), (int)o.refused,
                       pk.ms + ms_between(t0, Clock::now()), pk.ms + ms_between(t0, t1), ms_between(t1, Clock::now()));
  return o;
}
// ---- --transitive: the same problems into the trans object of the batch's handle (wfm_trans_add), each with the world position of its
// first target base (the problem's base: the world begins with the target's sequences) and of the first base of its forward query window
// (in the query sequence's place in the world). ----
StageOutcome trans_records(wfm_handle_t* h, int, const BatchPasses& bp, PackedRuns& pk) {
  auto t0 = Clock::now(), t1 = t0;
  const size_t n = pk.size();
  std::vector<wfm_trans_prob_t> probs(n);
  for (size_t j = 0; j < n; ++j)
    probs[j] = wfm_trans_prob_t{pk.probs[j].base, transitive::query_world(pk.place[j].query_world, pk.where[j].qs), pk.probs[j].runs_off,
                                pk.probs[j].n_runs, pk.where[j].rev ? WFM_TRANS_REVERSE : 0u};
  std::vector<uint32_t> flags(n);
  StageOutcome o = add_stage(h, n, t1, [&] {
    return wfm_trans_add(h, bp.get<wfm_trans_t>(SW_TRANSITIVE), probs.data(), n, pk.runs.data(), pk.runs.size(), flags.data());
  });
  if (o.rc >= 0)
    o.debug = debug_line("[wflign] transitive: %zu records, %zu runs, %d flagged, %.1f ms (runs %.1f, host %.1f, device call %.1f)\n", n, pk.runs.size(),
                         (int)o.refused, pk.ms + ms_between(t0, Clock::now()), pk.ms, ms_between(t0, t1), ms_between(t1, Clock::now()));
  return o;
}

Stage stage_of(SwitchId id) {
  switch (id) {
    case SW_COVERAGE: return coverage_records;
    case SW_PAV: return pav_records;
    case SW_LIFT: return lift_records;
    case SW_CHAIN: return chain_records;
    case SW_CHAIN_NET: return net_records;
    case SW_TRANSITIVE: return trans_records;
    default: return nullptr;  // (--variants, --genotypes and --maf work on the align batch's windows)
  }
}

void take_texts(PackedRuns& pk, BatchTexts& t) {
  for (const std::string& s : pk.lift) t.text[SW_LIFT] += s;
  for (const std::string& s : pk.chain) t.text[SW_CHAIN] += s;
  t.net_heads = std::move(pk.net_heads);
}

// ---------------------------------------------------------------------------
// passes
// ---------------------------------------------------------------------------
void* Pass::object_of(wfm_handle_t* h) {
  if (!per_handle) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  for (auto& ho : objects) if (ho.first == h) return ho.second;
  void* o = nullptr;
  std::lock_guard<std::mutex> hl(handle_lock(h));
  if (create(h, &o) != WFM_OK) fail(wfm_last_error(h));
  objects.emplace_back(h, o);
  return o;
}
void Pass::free_objects() {
  for (auto& ho : objects) {
    std::lock_guard<std::mutex> lk(handle_lock(ho.first));
    destroy(ho.second);
  }
  objects.clear();
}
// every other handle's object exported and imported into the first's (integer adds, unions and set functions: the order does not matter)
void Pass::merge() {
  for (size_t k = 1; k < objects.size(); ++k) {
    {
      std::lock_guard<std::mutex> lk(handle_lock(objects[k].first));
      if (export_lists(objects[k].first, objects[k].second) != WFM_OK) fail(objects[k].first, "export");
    }
    std::lock_guard<std::mutex> lk(handle_lock(h0()));
    const int rc = import_lists(h0(), objects.front().second);
    free_lists();
    if (rc != WFM_OK) fail(h0(), "import");
  }
}

namespace {
std::vector<wfm_lift_iv_t> raw_intervals(const std::vector<lift::Interval>& iv) {
  std::vector<wfm_lift_iv_t> raw(iv.size());
  for (size_t i = 0; i < raw.size(); ++i) raw[i] = wfm_lift_iv_t{iv[i].gstart, iv[i].gend};
  return raw;
}

// --variants: the header here, the batches' lines through the ordered writer
struct VariantsPass : Pass {
  VariantsPass(RunTables& tb, const PassInput& in) : Pass(SW_VARIANTS, false, tb, in) {
    out << "##fileformat=VCFv4.2\n##source=wfmash-hip " WFMASH_HIP_VERSION "\n";
    for (size_t i = 0; i < tb.tnames.size(); ++i) out << "##contig=<ID=" << tb.tnames[i] << ",length=" << tb.tlengths[i] << ">\n";
    out << "##INFO=<ID=QNAME,Number=1,Type=String,Description=\"Query sequence name\">\n"
           "##INFO=<ID=QSTART,Number=1,Type=Integer,Description=\"Start of the query bases in ALT, 0-based, forward strand\">\n"
           "##INFO=<ID=QEND,Number=1,Type=Integer,Description=\"End of the query bases in ALT, exclusive, forward strand\">\n"
           "##INFO=<ID=QSTRAND,Number=1,Type=String,Description=\"Strand of the query in the alignment\">\n"
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
    writes_per_batch();
  }
};

// --coverage: the depth objects; the intervals of their sum taken once on the device, the file through coverage_bedgraph
struct CoveragePass : Pass {
  CoveragePass(RunTables& tb, const PassInput& in) : Pass(SW_COVERAGE, true, tb, in) {}
  wfm_cov_entry_t* list = nullptr;
  size_t n_list = 0;
  int create(wfm_handle_t* h, void** o) override {
    wfm_coverage_t* c = nullptr;
    const int rc = wfm_coverage_create(h, tables.seq_offsets.back(), &c);
    *o = c;
    return rc;
  }
  void destroy(void* o) override { wfm_coverage_free((wfm_coverage_t*)o); }
  int export_lists(wfm_handle_t* h, void* o) override { return wfm_coverage_export(h, (wfm_coverage_t*)o, &list, &n_list); }
  int import_lists(wfm_handle_t* h, void* o) override { return wfm_coverage_import(h, (wfm_coverage_t*)o, list, n_list); }
  void free_lists() override { wfm_coverage_free_list(list); }
  Finished finish() override {
    const auto t0 = Clock::now();
    merge();
    wfm_cov_interval_t* iv = nullptr;
    size_t n = 0;
    uint64_t totals[3] = {0, 0, 0};
    if (!objects.empty()) {
      std::lock_guard<std::mutex> lk(handle_lock(h0()));
      if (wfm_coverage_intervals(h0(), first<wfm_coverage_t>(), &iv, &n, totals) != WFM_OK) fail(h0(), "intervals");
    }
    uint64_t lines = 0;
    out << coverage::coverage_bedgraph(tables.tnames, tables.tlengths, iv, n, &lines);
    wfm_coverage_free_list(iv);
    return Finished{{totals[0], totals[1], lines}, totals[2],
                    debug_line("[wfmash::align] coverage: %zu objects merged, %zu intervals, %llu lines, %.1f ms\n", objects.size(), n, (unsigned long long)lines,
                               ms_between(t0, Clock::now()))};
  }
};

// --lift: the BED's intervals sorted as the device takes them; a liftset per handle; the batches' lines through the ordered writer
struct LiftPass : Pass {
  LiftPass(RunTables& tb, const PassInput& in) : Pass(SW_LIFT, true, tb, in) {
    lift::Bed parsed = lift::parse_bed(in.bed, tb.find_target, tb.tlengths, tb.seq_offsets);
    tb.lift_iv = std::move(parsed.iv);
    bed_skipped = parsed.skipped;
    writes_per_batch();
  }
  uint64_t bed_skipped = 0;
  int create(wfm_handle_t* h, void** o) override {
    const std::vector<wfm_lift_iv_t> raw = raw_intervals(tables.lift_iv);
    wfm_liftset_t* set = nullptr;
    const int rc = wfm_liftset_create(h, raw.data(), raw.size(), tables.seq_offsets.back(), &set);
    *o = set;
    return rc;
  }
  void destroy(void* o) override { wfm_liftset_free((wfm_liftset_t*)o); }
  Finished finish() override { return Finished{{0, 0, bed_skipped}, tables.lift_iv.size(), std::string()}; }
};

// --chain: the batches' chains through the ordered writer, which numbers them
struct ChainPass : Pass {
  ChainPass(RunTables& tb, const PassInput& in) : Pass(SW_CHAIN, false, tb, in) {
    tb.chain_swap = in.option != 0;
    writes_per_batch(true);
  }
};

// --maf: the header here, the batches' blocks through the ordered writer (no device object, no merge)
struct MafPass : Pass {
  MafPass(RunTables& tb, const PassInput& in) : Pass(SW_MAF, false, tb, in) {
    out << maf::header();
    writes_per_batch();
  }
};

// --pav: the intervals of the table in the file's order and the columns are known before anything is added; the presence objects; the
// table of their union taken once on the device, the file through pav_text.hpp
struct PavPass : Pass {
  PavPass(RunTables& tb, const PassInput& in) : Pass(SW_PAV, true, tb, in) {
    if (in.has_bed) {
      lift::Bed parsed = lift::parse_bed(in.bed, tb.find_target, tb.tlengths, tb.seq_offsets);
      iv = std::move(parsed.iv);
      bed_skipped = parsed.skipped;
    } else {
      iv = pav::windows(tb.tlengths, tb.seq_offsets, in.option);
    }
    if (tb.columns.of_seq.empty()) tb.columns = pav::columns(tb.qnames);
  }
  std::vector<lift::Interval> iv;
  uint64_t bed_skipped = 0;
  wfm_pav_seg_t* list = nullptr;
  size_t n_list = 0;
  int create(wfm_handle_t* h, void** o) override {
    wfm_pav_t* p = nullptr;
    const int rc = wfm_pav_create(h, tables.seq_offsets.back(), (uint32_t)tables.columns.keys.size(), &p);
    *o = p;
    return rc;
  }
  void destroy(void* o) override { wfm_pav_free((wfm_pav_t*)o); }
  int export_lists(wfm_handle_t* h, void* o) override { return wfm_pav_export(h, (wfm_pav_t*)o, &list, &n_list); }
  int import_lists(wfm_handle_t* h, void* o) override { return wfm_pav_import(h, (wfm_pav_t*)o, list, n_list); }
  void free_lists() override { wfm_pav_free_list(list); }
  Finished finish() override {
    const auto t0 = Clock::now();
    const size_t G = tables.columns.keys.size();
    std::vector<uint32_t> cells(G * iv.size(), 0u);
    uint64_t counts[3] = {0, 0, 0};
    merge();
    if (!objects.empty()) {
      const std::vector<wfm_lift_iv_t> raw = raw_intervals(iv);
      std::lock_guard<std::mutex> lk(handle_lock(h0()));
      if (wfm_pav_matrix(h0(), first<wfm_pav_t>(), raw.data(), raw.size(), cells.data()) != WFM_OK) fail(h0(), "matrix");
      wfm_pav_counts(first<wfm_pav_t>(), counts);
    }
    const auto t1 = Clock::now();
    pav::table(out, tables.columns.keys, tables.tnames, iv, cells.data());
    return Finished{{iv.size(), counts[1], bed_skipped}, 0,
                    debug_line("[wfmash::align] pav: %zu objects merged, %llu segments added, %llu union intervals, %zu rows x %zu groups, merge + union + matrix %.1f ms, text %.1f ms\n",
                               objects.size(), (unsigned long long)counts[0], (unsigned long long)counts[1], iv.size(), G, ms_between(t0, t1), ms_between(t1, Clock::now()))};
  }
};

// --genotypes: the columns are --pav's; the sites objects; the table of their merge taken once on the device, the file through
// genotype_text.hpp
struct GenotypesPass : Pass {
  GenotypesPass(RunTables& tb, const PassInput& in) : Pass(SW_GENOTYPES, true, tb, in) {
    if (tb.columns.of_seq.empty()) tb.columns = pav::columns(tb.qnames);
  }
  wfm_site_var_t* vars = nullptr;
  char* alleles = nullptr;
  wfm_pav_seg_t* segs = nullptr;
  size_t n_vars = 0, n_bytes = 0, n_segs = 0;
  int create(wfm_handle_t* h, void** o) override {
    wfm_sites_t* p = nullptr;
    const int rc = wfm_sites_create(h, tables.seq_offsets.back(), (uint32_t)tables.columns.keys.size(), &p);
    *o = p;
    return rc;
  }
  void destroy(void* o) override { wfm_sites_free((wfm_sites_t*)o); }
  int export_lists(wfm_handle_t* h, void* o) override { return wfm_sites_export(h, (wfm_sites_t*)o, &vars, &n_vars, &alleles, &n_bytes, &segs, &n_segs); }
  int import_lists(wfm_handle_t* h, void* o) override { return wfm_sites_import(h, (wfm_sites_t*)o, vars, n_vars, alleles, n_bytes, segs, n_segs); }
  void free_lists() override { wfm_sites_free_list(vars); wfm_sites_free_list(alleles); wfm_sites_free_list(segs); }
  Finished finish() override {
    const auto t0 = Clock::now();
    wfm_site_t* rows = nullptr;
    char *table_alleles = nullptr, *gt = nullptr;
    size_t n_sites = 0, bytes = 0;
    uint64_t counts[4] = {0, 0, 0, 0};
    merge();
    if (!objects.empty()) {
      std::lock_guard<std::mutex> lk(handle_lock(h0()));
      if (wfm_sites_table(h0(), first<wfm_sites_t>(), &rows, &n_sites, &table_alleles, &bytes, &gt) != WFM_OK) fail(h0(), "table");
      wfm_sites_counts(first<wfm_sites_t>(), counts);
    }
    const auto t1 = Clock::now();
    genotype::vcf(out, WFMASH_HIP_VERSION, tables.tnames, tables.tlengths, tables.seq_offsets, tables.columns.keys, rows, n_sites, table_alleles, gt);
    wfm_sites_free_list(rows); wfm_sites_free_list(table_alleles); wfm_sites_free_list(gt);
    return Finished{{n_sites, counts[0] - n_sites, 0}, 0,
                    debug_line("[wfmash::align] genotypes: %zu objects merged, %llu variants, %zu sites x %zu groups, %llu = intervals, merge + table %.1f ms, text %.1f ms\n",
                               objects.size(), (unsigned long long)counts[0], n_sites, tables.columns.keys.size(), (unsigned long long)counts[2], ms_between(t0, t1),
                               ms_between(t1, Clock::now()))};
  }
};

// --chain-net: the net objects, and what the chains' headers need of every record added, in no order; the table of the merged object
// taken once on the device, the file through chain_text.hpp's net_file in the order of the orders, which is the order of the PAF's records
struct ChainNetPass : Pass {
  ChainNetPass(RunTables& tb, const PassInput& in) : Pass(SW_CHAIN_NET, true, tb, in), unit(in.unit) {}
  const std::string unit;
  std::vector<NetHead> heads;  // (under mu)
  wfm_net_block_t* blocks = nullptr;
  wfm_net_rec_t* recs = nullptr;
  size_t n_blocks = 0, n_recs = 0;
  void take(uint64_t, BatchTexts& t) override {
    if (t.net_heads.empty()) return;
    std::lock_guard<std::mutex> lk(mu);
    for (auto& hd : t.net_heads) heads.push_back(std::move(hd));
  }
  int create(wfm_handle_t* h, void** o) override {
    wfm_net_t* p = nullptr;
    const int rc = wfm_net_create(h, tables.seq_offsets.back(), &p);
    *o = p;
    return rc;
  }
  void destroy(void* o) override { wfm_net_free((wfm_net_t*)o); }
  int export_lists(wfm_handle_t* h, void* o) override { return wfm_net_export(h, (wfm_net_t*)o, &blocks, &n_blocks, &recs, &n_recs); }
  int import_lists(wfm_handle_t* h, void* o) override { return wfm_net_import(h, (wfm_net_t*)o, blocks, n_blocks, recs, n_recs); }
  void free_lists() override { wfm_net_free_list(blocks); wfm_net_free_list(recs); }
  Finished finish() override {
    const auto t0 = Clock::now();
    wfm_net_piece_t* pieces = nullptr;
    wfm_netcall_t* per = nullptr;
    size_t n_pieces = 0, n_rec = 0;
    uint64_t counts[6] = {0, 0, 0, 0, 0, 0};
    merge();
    if (!objects.empty()) {
      std::lock_guard<std::mutex> lk(handle_lock(h0()));
      if (wfm_net_table(h0(), first<wfm_net_t>(), &pieces, &n_pieces, &per, &n_rec) != WFM_OK) fail(h0(), "table");
      wfm_net_counts(first<wfm_net_t>(), counts);
    }
    const auto t1 = Clock::now();
    static_assert(sizeof(chain::Piece) == sizeof(wfm_net_piece_t) && sizeof(chain::NetCall) == sizeof(wfm_netcall_t), "chain_text.hpp restates wfm_net_piece_t and wfm_netcall_t");
    std::sort(heads.begin(), heads.end(), [](const NetHead& a, const NetHead& b) { return a.order < b.order; });
    uint64_t chains = 0, lost = 0;
    const bool same = chain::net_file(out, heads, (const chain::NetCall*)per, n_rec, (const chain::Piece*)pieces, &chains, &lost);
    wfm_net_free_list(pieces); wfm_net_free_list(per);
    if (!same) fail("the table's records are not the " + unit + " added");
    return Finished{{chains, n_pieces, lost}, 0,
                    debug_line("[wfmash::align] chain-net: %zu objects merged, %llu records, %llu blocks, %llu elementary intervals, %zu pieces, %llu chains, %llu records won nothing, merge + table %.1f ms, text %.1f ms\n",
                               objects.size(), (unsigned long long)counts[0], (unsigned long long)counts[1], (unsigned long long)counts[2], n_pieces, (unsigned long long)chains,
                               (unsigned long long)lost, ms_between(t0, t1), ms_between(t1, Clock::now()))};
  }
};

// --transitive: the world and the seeds in input order are known before anything is added; the trans objects; the closure of the seeds
// over their merge taken once on the device, the file through transitive_text.hpp in the order of the BED's lines
struct TransitivePass : Pass {
  TransitivePass(RunTables& tb, const PassInput& in) : Pass(SW_TRANSITIVE, true, tb, in), depth((uint32_t)in.option) {
    tb.world = transitive::make_world(tb.tnames, tb.tlengths, tb.qnames, tb.qlengths);
    if (tb.world.n_bases() >= ((uint64_t)1 << 40)) fail("the sequences hold 2^40 bases or more");
    for (const std::string& name : tb.qnames) tb.query_world.push_back(tb.world.offsets[(size_t)tb.world.find(name)]);
    seeds = transitive::parse_seeds(in.bed, tb.world);
    if (seeds.iv.size() >= ((size_t)1 << 24)) fail("the BED holds 2^24 seeds or more");
  }
  lift::Bed seeds;
  const uint32_t depth;
  wfm_trans_rec_t* recs = nullptr;
  wfm_trans_word_t* words = nullptr;
  size_t n_recs = 0, n_words = 0;
  int create(wfm_handle_t* h, void** o) override {
    wfm_trans_t* p = nullptr;
    const int rc = wfm_trans_create(h, tables.world.n_bases(), &p);
    *o = p;
    return rc;
  }
  void destroy(void* o) override { wfm_trans_free((wfm_trans_t*)o); }
  int export_lists(wfm_handle_t* h, void* o) override { return wfm_trans_export(h, (wfm_trans_t*)o, &recs, &n_recs, &words, &n_words); }
  int import_lists(wfm_handle_t* h, void* o) override { return wfm_trans_import(h, (wfm_trans_t*)o, recs, n_recs, words, n_words); }
  void free_lists() override { wfm_trans_free_list(recs); wfm_trans_free_list(words); }
  Finished finish() override {
    const auto t0 = Clock::now();
    const transitive::World& world = tables.world;
    wfm_trans_iv_t* ivs = nullptr;
    size_t n_ivs = 0;
    std::vector<wfm_trans_seed_t> per(seeds.iv.size());
    uint64_t counts[6] = {0, 0, 0, 0, 0, 0};
    if (!objects.empty() && !seeds.iv.empty()) {
      merge();
      const std::vector<wfm_lift_iv_t> raw = raw_intervals(seeds.iv);
      std::lock_guard<std::mutex> lk(handle_lock(h0()));
      if (wfm_trans_closure(h0(), first<wfm_trans_t>(), raw.data(), raw.size(), depth, &ivs, &n_ivs, per.data()) != WFM_OK) fail(h0(), "closure");
      wfm_trans_counts(first<wfm_trans_t>(), counts);
    }
    const auto t1 = Clock::now();
    static_assert(sizeof(transitive::ClosureIv) == sizeof(wfm_trans_iv_t) && sizeof(transitive::SeedCall) == sizeof(wfm_trans_seed_t),
                  "transitive_text.hpp restates wfm_trans_iv_t and wfm_trans_seed_t");
    const uint64_t lines = transitive::file(out, world, seeds.iv, (const transitive::SeedCall*)per.data(), (const transitive::ClosureIv*)ivs);
    wfm_trans_free_list(ivs);
    return Finished{{lines, counts[3], seeds.skipped}, seeds.iv.size(),
                    debug_line("[wfmash::align] transitive: %zu objects merged, %llu records, %llu prefix words, %zu seeds at depth %u, %llu rounds, %llu pairs, %zu intervals, %llu lines, merge + closure %.1f ms, text %.1f ms\n",
                               objects.size(), (unsigned long long)counts[0], (unsigned long long)counts[1], seeds.iv.size(), depth, (unsigned long long)counts[3],
                               (unsigned long long)counts[5], n_ivs, (unsigned long long)lines, ms_between(t0, t1), ms_between(t1, Clock::now()))};
  }
};

// the passes in their order: SwitchId's first N_PASSES
template <class P>
Pass* new_pass(RunTables& tb, const PassInput& in) { return new P(tb, in); }
Pass* (*const kMakePass[N_PASSES])(RunTables&, const PassInput&) = {
    new_pass<VariantsPass>, new_pass<CoveragePass>,  new_pass<LiftPass>,     new_pass<ChainPass>,
    new_pass<PavPass>,      new_pass<GenotypesPass>, new_pass<ChainNetPass>, new_pass<TransitivePass>,
    new_pass<MafPass>};
}  // namespace

std::unique_ptr<Pass> make_pass(SwitchId id, RunTables& tb, const PassInput& in) { return std::unique_ptr<Pass>(kMakePass[id](tb, in)); }

void fill_tables(RunTables& tb, const wfmash_host::FastaStore& target, const wfmash_host::FastaStore& query) {
  tb.seq_offsets.assign(1, 0);
  for (int i = 0; i < target.nseq(); ++i) {
    tb.tnames.push_back(target.name(i));
    tb.tlengths.push_back((uint64_t)target.length(i));
    tb.seq_offsets.push_back(tb.seq_offsets.back() + tb.tlengths.back());
  }
  for (int i = 0; i < query.nseq(); ++i) { tb.qnames.push_back(query.name(i)); tb.qlengths.push_back((uint64_t)query.length(i)); }
  tb.find_target = [&target](const std::string& name) { return target.find(name); };
}

// ---------------------------------------------------------------------------
// an aligned PAF through one pass
// ---------------------------------------------------------------------------
PafPassResult run_paf_pass(wfm_handle_t* h, const PafPassCall& c) {
  const std::string tag = std::string("[wfmash::") + c.tag + "]";
  auto open = [&](auto& s, const char* path, std::ios::openmode mode) {
    s.open(path, mode);
    if (!s.is_open()) throw std::runtime_error(tag + " cannot open " + path);
  };
  const std::shared_ptr<wfmash_host::FastaStore> target = wfmash_host::open_shared(c.target_fasta);
  const std::shared_ptr<wfmash_host::FastaStore> query = c.query_fasta_or_null && *c.query_fasta_or_null ? wfmash_host::open_shared(c.query_fasta_or_null) : target;
  std::ifstream in;
  open(in, c.aligned_paf, std::ios::in);
  std::ofstream out;  // (opened behind the pass's constructor, which reads and refuses before a file is made)
  PassInput input;
  input.prefix = tag; input.unit = "lines"; input.out = &out; input.option = c.option;
  if (c.bed_path_or_null && *c.bed_path_or_null) {
    std::ifstream bed;
    open(bed, c.bed_path_or_null, std::ios::in | std::ios::binary);
    input.has_bed = true;
    input.bed.assign((std::istreambuf_iterator<char>(bed)), std::istreambuf_iterator<char>());
  }
  RunTables tables;
  fill_tables(tables, *target, *query);
  const std::unique_ptr<Pass> pass = make_pass(c.id, tables, input);
  open(out, c.out_path, std::ios::out);
  struct Free { Pass& p; ~Free() { p.free_objects(); } } free_at_end{*pass};
  BatchPasses bp;
  bp.on[c.id] = true;
  bp.tables = &tables;
  bp.object[c.id] = pass->object_of(h);  // (before the first line: a PAF without lines leaves an empty object, not none)
  BatchLimits lim;
  if (const char* e = getenv("WFM_PAF_BATCH_RECORDS")) lim.records = (size_t)std::max(1, atoi(e));
  PafPassResult r;
  const Stage stage = stage_of(c.id);
  uint64_t seq = 0;
  // the rules only these modes have: --pav-paf leaves out a line whose query the query file does not have, --transitive-paf one whose
  // query neither file has or whose qe lies behind its end
  auto hook = [&](const verify::Line& l, Place& place) {
    if (c.id == SW_PAV) {
      const int qi = query->find(l.qname);
      if (qi < 0) { ++r.no_query; return false; }
      place.group = tables.columns.of_seq[(size_t)qi];
    } else if (c.id == SW_TRANSITIVE) {
      const int qi = tables.world.find(l.qname);
      if (qi < 0 || (uint64_t)l.qe > tables.world.lengths[(size_t)qi]) { ++r.no_query; return false; }
      place.query_world = tables.world.offsets[(size_t)qi];
    }
    return true;
  };
  read_packed_lines(in, tables.find_target, tables.tlengths, tables.seq_offsets, lim, r.skipped, hook, [&](PackedRuns& pk) {
    const StageOutcome o = stage(h, 1, bp, pk);
    if (o.rc < 0) pass->fail("device call: " + o.error);
    for (int k = 0; k < 3; ++k) r.counts[k] += o.counts[k];
    r.skipped[coverage::LINE_MALFORMED] += o.refused;
    BatchTexts texts;
    take_texts(pk, texts);
    pass->take(seq++, texts);
  });
  r.end = pass->finish();
  r.groups = tables.columns.keys.size();
  return r;
}

}  // namespace wflign
