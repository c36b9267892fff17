// wflign_hip.cpp -- see wflign_hip.hpp.  The batch form of do_biwfa_alignment: its device calls and the stages between them.
// The CIGAR surgery, the patch plan and the record writers are in cigar_ops.hpp; all wavefront arithmetic is done on the GPU
// through wfm_align_batch (no CPU fallback).
#include "wflign_hip.hpp"
#include "run_passes.hpp"
#include "maf_text.hpp"
#include "../csrc/wfa_handle.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>

namespace wflign {

// ---------------------------------------------------------------------------
// batch pipeline
// ---------------------------------------------------------------------------
// A handle runs one batch at a time; several host threads may feed the same GPU (the align driver keeps up to three
// batches per device in flight so that the host stages of one overlap the device stages of another): calls are
// serialised here.
std::mutex& handle_lock(wfm_handle_t* h) {
  static std::mutex reg;
  static std::map<wfm_handle_t*, std::unique_ptr<std::mutex>> locks;
  std::lock_guard<std::mutex> lk(reg);
  auto& m = locks[h];
  if (!m) m.reset(new std::mutex());
  return *m;
}
namespace {

// One process-wide switch (wflign_hip.hpp names them): whether it is on, what wfmh_set_* named -- up to two paths under the mutex, one
// integer -- and four counts since it was set.  The counts: --verify-optimal {problems checked (the skipped among them), failed, skipped,
// cells}; --left-align {records handed to the device, their interior gaps, gaps moved, records left alone}; --cs {records spelled, bytes
// spelled, records left without a string, 0}; --variants {records called, variants written, SNVs masked, records left alone}; --coverage
// {records added, target bases with depth >= 1, sum of depth, intervals written}; --lift {records lifted, lines written, empty lifts, BED
// lines skipped}; --chain {chains written, blocks, records refused, 0}; --chain-net {records added, chains written, pieces, records that
// won nothing}; --transitive {records added, lines written, rounds run, BED lines skipped}; --pav {records added, rows written, union
// intervals, BED lines skipped}; --genotypes {records added, sites written, variants merged away, records left alone}.
struct Switch {
  std::atomic<bool> on{false};
  std::mutex mu;
  std::string out, bed;
  std::atomic<uint64_t> option{0};  // --verify-optimal: the cap of one problem's DP cells (0: none); --cs: 1 short, 2 long; SwitchSetting's otherwise
  std::atomic<uint64_t> counts[4];
};
Switch g_switch[N_SWITCHES];
bool is_on(SwitchId id) { return g_switch[id].on.load(std::memory_order_relaxed); }
std::atomic<uint64_t>* counts_of(SwitchId id) { return g_switch[id].counts; }

// The problems of one device call, always written by reference (a side without a store id carries its host pointer); without a
// store they go to the device as plain wfm_problem_t, as they always have.
struct GpuBatch {
  std::vector<wfm_problem_ref_t> probs;
  const wfm_seqstore_t* store = nullptr;
  std::vector<wfm_result_t> res;
  std::vector<uint32_t> flags;  // WFM_PF_* per problem (wfm_get_problem_flags), fetched while the handle is still ours
  uint32_t* runs = nullptr;
  std::string err;  // the handle's message, copied while the handle is still ours
  // --verify-optimal: what a failed problem is reported as -- its record and what of it the problem is
  const std::vector<BiwfaRecord>* recs = nullptr;
  std::vector<std::pair<size_t, const char*>> who;  // per problem (or empty: problem i is the main alignment of record i)
  ~GpuBatch() { wfm_free_runs(runs); }
  // upload -> wfm_align_resident_rle -> wfm_check_optimal -> free: what wfm_align_refs_rle / wfm_align_batch_rle do, with the check
  // between the last two.  The results and runs are the unchecked call's; the check only reads the seqset and the scores.
  int run_checked(wfm_handle_t* h, const wfm_penalties_t& pen, const std::vector<wfm_problem_t>& plain) {
    wfm_seqset_t* S = nullptr;
    int rc = store ? wfm_upload_sequence_refs(h, store, probs.data(), probs.size(), &S) : wfm_upload_sequences(h, plain.data(), plain.size(), &S);
    if (rc != WFM_OK) return rc;
    rc = wfm_align_resident_rle(h, &pen, S, res.data(), &runs, nullptr);
    if (rc >= 0) {
      std::vector<wfm_optcheck_t> oc(probs.size());
      const int crc = wfm_check_optimal(h, &pen, S, res.data(), g_switch[SW_VERIFY_OPTIMAL].option.load(), oc.data());
      if (crc < 0) rc = crc;
      else report_optimal(oc);
    }
    wfm_free_sequences(h, S);
    return rc;
  }
  void report_optimal(const std::vector<wfm_optcheck_t>& oc) const {
    uint64_t checked = 0, failed = 0, skipped = 0, cells = 0;
    for (size_t i = 0; i < oc.size(); ++i) {
      const wfm_optcheck_t& o = oc[i];
      if (o.flags & WFM_OPT_NOT_CHECKED) continue;  // (a problem without a score: the driver drops or keeps the record as ever)
      ++checked;
      cells += o.cells;
      if (o.flags & WFM_OPT_SKIPPED) { ++skipped; continue; }
      if (!(o.flags & (WFM_OPT_CHEAPER | WFM_OPT_UNREACHED))) continue;
      ++failed;
      const size_t ri = who.empty() ? i : who[i].first;
      const char* part = who.empty() ? "main alignment" : who[i].second;
      const int mode = probs[i].mode & WFM_MODE_MASK;
      const char* mname = mode == WFM_MODE_ENDSFREE ? "ends-free" : mode == WFM_MODE_END2END_UNI ? "end-to-end (uni)" : "end-to-end (BiWFA)";
      std::string where = "problem " + std::to_string(i);
      if (recs && ri < recs->size()) {
        const BiwfaRecord& r = (*recs)[ri];
        where = r.query_name + ":" + std::to_string(r.query_offset) + "-" + std::to_string(r.query_offset + r.query_length) + (r.query_is_rev ? " - " : " + ") +
                r.target_name + ":" + std::to_string(r.target_offset) + "-" + std::to_string(r.target_offset + r.target_length);
      }
      fprintf(stderr, "[wfmash::verify] %s %s (%s, %s, %d x %d bases): claimed score %d, DP score %d\n", (o.flags & WFM_OPT_CHEAPER) ? "NOT OPTIMAL" : "UNREACHED",
              where.c_str(), part, mname, probs[i].plen, probs[i].tlen, res[i].score, o.dp_score);
    }
    std::atomic<uint64_t>* c = counts_of(SW_VERIFY_OPTIMAL);
    c[0] += checked; c[1] += failed; c[2] += skipped; c[3] += cells;
  }
  int run(wfm_handle_t* h, const wfm_penalties_t& pen, BiwfaStats* st) {
    res.assign(probs.size(), wfm_result_t{});
    wfm_free_runs(runs);
    runs = nullptr;
    if (probs.empty()) return 0;
    std::lock_guard<std::mutex> lk(handle_lock(h));
    int rc;
    std::vector<wfm_problem_t> plain;
    if (!store) {
      plain.resize(probs.size());
      for (size_t i = 0; i < probs.size(); ++i) {
        const wfm_problem_ref_t& r = probs[i];
        plain[i] = wfm_problem_t{r.pattern, r.plen, r.text, r.tlen, r.mode, r.pattern_begin_free, r.pattern_end_free,
                                 r.text_begin_free, r.text_end_free, r.score_hint, 0};
      }
    }
    if (is_on(SW_VERIFY_OPTIMAL)) rc = run_checked(h, pen, plain);  // --verify-optimal: the same call in its parts, the seqset kept for the check
    else if (store) rc = wfm_align_refs_rle(h, &pen, store, probs.data(), probs.size(), res.data(), &runs, nullptr);
    else rc = wfm_align_batch_rle(h, &pen, plain.data(), plain.size(), res.data(), &runs, nullptr);
    if (rc < 0) err = wfm_last_error(h);
    flags.assign(probs.size(), 0u);
    if (rc >= 0) wfm_get_problem_flags(h, flags.data(), flags.size());
    if (rc >= 0 && st) {
      wfm_stats_t s;
      if (wfm_get_stats(h, &s) == WFM_OK) {
        st->cells += s.cells; st->ms_gpu += s.ms_any_busy;
        st->cells_tile += s.cells_tile_unique; st->tile_launches += s.tile_launches; st->ms_tile += s.ms_tile;
      }
      const size_t ni = wfm_get_busy_intervals(h, nullptr, 0);
      if (ni) {
        std::vector<double> iv(2 * ni);
        wfm_get_busy_intervals(h, iv.data(), ni);
        for (size_t q = 0; q < ni; ++q) st->busy.emplace_back(iv[2 * q], iv[2 * q + 1]);
      }
    }
    return rc;
  }
  void ops(size_t i, CigarOps& out) const { ops_from_runs(runs + res[i].ops_off, res[i].n_runs, out); }
};

// A guess of an upper bound of the score, for the device to cut its wavefronts with (wfm_problem_t::score_hint): the
// target window is the mapped range plus padding, so the alignment opens with and ends in a gap -- two gap openings
// and the length difference -- and in between it pays for the divergence mashmap estimated, at 6 per differing base
// (a mismatch costs 5), with 0.1 % and 1000 on top.  Too small a guess only costs that record a second run.
int32_t score_hint(const BiwfaRecord& r, const wflign_penalties_t& penalties) {
  double id = r.mashmap_estimated_identity > 1.0f ? r.mashmap_estimated_identity / 100.0 : r.mashmap_estimated_identity;
  id = std::min(1.0, std::max(0.5, id));
  const double len = (double)std::min(r.target_length, r.query_length);
  const double dl = std::fabs((double)r.target_length - (double)r.query_length);
  static const double per_base = getenv("WFM_HINT_PER_BASE") ? atof(getenv("WFM_HINT_PER_BASE")) : 6.0;
  static const double id_slack = getenv("WFM_HINT_ID_SLACK") ? atof(getenv("WFM_HINT_ID_SLACK")) : 0.001;
  // (1000 since round 5, 200 before: a root that runs past its guess is run again from scratch, and with the device time of a batch made of chains
  // of launches a second chain costs more than the cells a looser bound adds -- C2 55 -> 53 ms, scaled C4 rank 48.3 -> 46.5, 40 Mbp rank 214 -> 207 ms
  // of device time, gpurun_out: the hint sweep of round 5; 2000 gains nothing more)
  static const double konst = getenv("WFM_HINT_CONST") ? atof(getenv("WFM_HINT_CONST")) : 1000.0;
  const double hint = 2.0 * penalties.gap_opening2 + penalties.gap_extension2 * dl + (1.0 - id + id_slack) * len * per_base + konst;
  return hint < 1e9 ? (int32_t)hint : 0;
}

// bases [ta, ta + plen) of the record's target window against [qa, qa + tlen) of its (strand-adjusted) query window: by host
// pointer, or -- where the record names its sides in the device's store -- as the sub-windows of the stored sequences
wfm_problem_ref_t window_problem(const BiwfaRecord& r, uint64_t ta, uint64_t plen, uint64_t qa, uint64_t tlen) {
  wfm_problem_ref_t p{};
  p.plen = (int32_t)plen; p.tlen = (int32_t)tlen;
  p.pattern_seq = r.target_seq; p.text_seq = r.query_seq;
  if (r.target_seq >= 0) p.pattern_off = sub_window_off(r.target_win_off, (int64_t)r.target_length, false, (int64_t)ta, (int64_t)(ta + plen));
  else p.pattern = r.target + ta;
  if (r.query_seq >= 0) {
    p.text_off = sub_window_off(r.query_win_off, (int64_t)r.query_length, r.query_is_rev, (int64_t)qa, (int64_t)(qa + tlen));
    p.text_revcomp = r.query_is_rev ? 1 : 0;
  } else p.text = r.query + qa;
  return p;
}

wfm_problem_ref_t head_problem(const BiwfaRecord& r, const Erosion& e) {  // wflign.cpp:280-305
  wfm_problem_ref_t p = window_problem(r, 0, e.target_eroded, 0, e.query_eroded);
  p.mode = WFM_MODE_ENDSFREE;
  p.pattern_begin_free = (int32_t)e.target_eroded; p.pattern_end_free = 0;
  p.text_begin_free = (int32_t)e.query_eroded; p.text_end_free = 0;
  return p;
}
wfm_problem_ref_t tail_problem(const BiwfaRecord& r, const Erosion& e) {  // wflign.cpp:368-397
  wfm_problem_ref_t p = window_problem(r, r.target_length - e.target_eroded, e.target_eroded, r.query_length - e.query_eroded, e.query_eroded);
  p.mode = WFM_MODE_ENDSFREE;
  p.pattern_begin_free = 0; p.pattern_end_free = (int32_t)e.target_eroded;
  p.text_begin_free = 0; p.text_end_free = (int32_t)e.query_eroded;
  return p;
}

struct WindowSet;  // the records' final runs as device problems (left_align_records, cs_records, variant_records, maf_records)

// --genotypes: what wfm_call_variants returned for the batch, kept until the filters have spoken (genotype_records)
struct KeptCalls {
  wfm_variant_t* vars = nullptr;
  char* alleles = nullptr;
  std::vector<wfm_varcall_t> per;  // per part of the window set
  std::vector<size_t> rec;         // the part's record in the batch
  ~KeptCalls() { wfm_free_variants(vars, alleles); }
};

// One call of do_biwfa_alignment_batch: what its stages share.
struct BiwfaBatch {
  wfm_handle_t* h;
  std::vector<BiwfaRecord>& recs;
  const wflign_penalties_t& penalties;
  const wfm_penalties_t pen;
  const PafParams& pp;
  BiwfaStats* stats;
  const OutputFormat& fmt;
  ResidentSeqs* resident;
  const wfm_seqstore_t* store;
  const BatchPasses* passes;  // the align driver's passes: which are on, their objects on this handle, the run's tables
  BatchTexts* texts;          // ... and where what they leave per batch goes (null: nowhere)
  struct Work {
    PatchPlan plan;
    int head_slot = -1, tail_slot = -1;  // problem index in the patch call
  };
  std::vector<Work> wk;
  std::vector<char> over_budget;  // WFM_ST_OOM: dropped like every record whose main alignment fails, but not silently
  size_t later = 0;               // records whose tail is scanned on the head-patched CIGAR
  std::atomic<uint64_t> n_head{0}, n_tail{0};
  int cs_form = 0;                // --cs as the batch found it: 0 off, 1 short, 2 long
  bool variants = false;          // --variants as the batch found it
  bool maf = false;               // --maf as the batch found it
  uint32_t maf_split = 0;         // ... and --maf-split
  std::unique_ptr<KeptCalls> calls;  // --genotypes: variant_records' records and alleles, for genotype_records
  std::unique_ptr<WindowSet> windows;  // what left_align_records leaves for cs_records and variant_records, and cs_records for variant_records
  // the handle's message was copied while the handle was still this thread's (another batch may be using it by now)
  int fail(const GpuBatch& g, int rc) const { if (stats) stats->error = g.err; return rc; }
};

// ---- main end-to-end BiWFA (wflign.cpp:136-165): the problems, the call, results and runs, the patch plan ----
int align_main(BiwfaBatch& b, bool plan) {
  const size_t n = b.recs.size();
  GpuBatch g;
  g.store = b.store;
  g.recs = &b.recs;
  g.probs.reserve(n);
  for (const auto& r : b.recs) {
    wfm_problem_ref_t p = window_problem(r, 0, r.target_length, 0, r.query_length);
    p.mode = WFM_MODE_END2END_BIWFA;
    p.score_hint = score_hint(r, b.penalties);
    g.probs.push_back(p);
  }
  const int rc = g.run(b.h, b.pen, b.stats);
  if (rc < 0) return b.fail(g, rc);
  for_each_record(n, b.fmt.threads, [&](size_t i) {
    BiwfaRecord& r = b.recs[i];
    r.ok = (g.res[i].status == 0);  // status != 0: the reference drops the record silently (wflign.cpp:150-152)
    b.over_budget[i] = g.res[i].status == WFM_ST_OOM;
    r.score = g.res[i].score;
    r.tags = g.flags[i] & 0xffu;
    r.paf.clear();
    r.cs.clear();
    r.vcf.clear();
    r.vcf_called = false; r.vcf_masked = 0;
    r.maf.clear();
    r.maf_called = false; r.maf_blocks = 0; r.maf_cols = 0;
    r.ops.clear();
    if (!r.ok) return;
    g.ops(i, r.ops);
    if (plan) b.wk[i].plan = plan_patches(r.ops);
  });
  if (b.stats)
    for (const auto& r : b.recs) b.stats->main_failed += !r.ok;
  return 0;
}

// (the one status the reference does not have: its memory follows the score as well, but has no budget to run out of)
void warn_over_budget(const BiwfaBatch& b) {
  for (size_t i = 0; i < b.recs.size(); ++i) {
    const BiwfaRecord& r = b.recs[i];
    if (b.over_budget[i])
      fprintf(stderr, "[wfmash] WARNING: %s:%llu-%llu -> %s:%llu-%llu not aligned: its wavefronts do not fit the device memory budget\n", r.query_name.c_str(),
              (unsigned long long)r.query_offset, (unsigned long long)(r.query_offset + r.query_length), r.target_name.c_str(),
              (unsigned long long)r.target_offset, (unsigned long long)(r.target_offset + r.target_length));
  }
}

// a tail patch's runs, eroded, behind the record's runs before erode_start_idx
void splice_tail(CigarOps& out, const GpuBatch& g, size_t slot) {
  CigarOps patch;
  g.ops(slot, patch);
  erode_short_matches_in_cigar(patch, 3, false);
  merge_adjacent_ops(out, patch, 0, patch.size());
}

// ---- head patches (wflign.cpp:241-320) and the tail patches that do not depend on them (wflign.cpp:323-418): the two
// patches of all records of the batch go to the device in ONE call (plan_patches), and are spliced in ----
int patch_ends(BiwfaBatch& b, GpuBatch& g) {
  const size_t n = b.recs.size();
  g.store = b.store;
  g.recs = &b.recs;
  for (size_t i = 0; i < n; ++i) {
    if (!b.recs[i].ok) continue;
    BiwfaBatch::Work& w = b.wk[i];
    if (w.plan.head_wanted) { w.head_slot = (int)g.probs.size(); g.probs.push_back(head_problem(b.recs[i], w.plan.head)); g.who.emplace_back(i, "head patch"); }
    if (!w.plan.tail_independent) { ++b.later; continue; }
    if (w.plan.tail_wanted) { w.tail_slot = (int)g.probs.size(); g.probs.push_back(tail_problem(b.recs[i], w.plan.tail)); g.who.emplace_back(i, "tail patch"); }
  }
  const int rc = g.run(b.h, b.pen, b.stats);
  if (rc < 0) return b.fail(g, rc);
  for_each_record(n, b.fmt.threads, [&](size_t i) {
    BiwfaRecord& r = b.recs[i];
    const BiwfaBatch::Work& w = b.wk[i];
    if (!r.ok || (w.head_slot < 0 && w.tail_slot < 0)) return;
    const bool head_ok = w.head_slot >= 0 && g.res[(size_t)w.head_slot].status == 0;
    const bool tail_ok = w.tail_slot >= 0 && g.res[(size_t)w.tail_slot].status == 0;
    if (w.head_slot >= 0) r.tags |= (g.flags[(size_t)w.head_slot] & 0xffu) << 8;
    if (w.tail_slot >= 0) r.tags |= (g.flags[(size_t)w.tail_slot] & 0xffu) << 16;
    if (!head_ok && !tail_ok) return;
    CigarOps out;
    size_t from = 0, to = r.ops.size();
    if (head_ok) {
      g.ops((size_t)w.head_slot, out);
      erode_short_matches_in_cigar(out, 3, true);
      from = w.plan.head.erode_end_pos;
      ++b.n_head;
    }
    if (tail_ok) to = w.plan.tail.erode_start_idx;
    out.reserve(out.size() + (to - from) + 64);
    merge_adjacent_ops(out, r.ops, from, to);
    if (tail_ok) { splice_tail(out, g, (size_t)w.tail_slot); ++b.n_tail; }
    r.ops.swap(out);
  });
  return 0;
}

// ---- short records, where the scans overlap: the tail scan on the head-patched CIGAR, as the reference runs it, and a
// second, small call for their patches ----
int patch_late_tails(BiwfaBatch& b) {
  GpuBatch g;
  g.store = b.store;
  g.recs = &b.recs;
  std::vector<size_t> owner;
  std::vector<size_t> cut;  // erode_start_idx of the owner's new tail scan
  for (size_t i = 0; i < b.recs.size(); ++i) {
    if (!b.recs[i].ok || b.wk[i].plan.tail_independent) continue;
    const Erosion te = scan_tail_erosion(b.recs[i].ops);
    if (patch_wanted(te)) { owner.push_back(i); cut.push_back(te.erode_start_idx); g.probs.push_back(tail_problem(b.recs[i], te)); g.who.emplace_back(i, "late tail patch"); }
  }
  const int rc = g.run(b.h, b.pen, b.stats);
  if (rc < 0) return b.fail(g, rc);
  for_each_record(owner.size(), b.fmt.threads, [&](size_t j) {
    BiwfaRecord& r = b.recs[owner[j]];
    r.tags |= (g.flags[j] & 0xffu) << 16;
    if (g.res[j].status != 0) return;
    r.ops.resize(cut[j]);
    splice_tail(r.ops, g, j);
    ++b.n_tail;
  });
  return 0;
}

// ---- swizzle (wflign.cpp:423-433) ----
void swizzle(BiwfaBatch& b, size_t ri) {
  BiwfaRecord& r = b.recs[ri];
  if (!r.ok) return;
  if (!r.query || !r.target) {
    // a record that came by reference, without its bases: the two swaps read bases only behind these two patterns
    const size_t no = r.ops.size();
    const bool may_swap = no >= 2 && ((r.ops[0].second == '=' && r.ops[1].second == 'D') || (r.ops[no - 2].second == 'D' && r.ops[no - 1].second == '='));
    if (may_swap && b.resident && b.resident->fetch) { b.resident->fetch(ri); b.resident->lazy_fetches.fetch_add(1); }
  }
  if (r.query && r.target) {
    const int64_t qn = (int64_t)r.query_length, tn = (int64_t)(r.target_avail ? r.target_avail : r.target_length);
    try_swap_start_pattern(r.ops, r.query, qn, r.target, tn);
    try_swap_end_pattern(r.ops, r.query, qn, r.target, tn);
  }
}

// ---- the records' final runs as device problems of their own: what --left-align, --cs and --variants work on.  What goes to the device is what the
// writers spell: both of them begin by stripping the leading and trailing I and D runs and shifting the start coordinates
// (trim_and_filter), so a record's problem is the runs ops[b, e) that remain against the sub-windows they cover.  Records go by reference
// where the batch has a store.  The ops of an ok record always span its windows (an end-to-end alignment does, a patch replaces eroded
// runs by an alignment of exactly their bases, erosion and the swaps keep both totals). ----
struct WindowSet {
  struct Part { size_t rec, b, e; };
  std::vector<Part> parts;
  std::vector<wfm_problem_ref_t> probs;
  std::vector<wfm_result_t> res;   // locates every part's runs in cur()
  std::vector<uint32_t> runs;      // as built from the records' ops
  uint32_t* la_runs = nullptr;     // wfm_left_align_runs' output once it has run: res locates the parts there from then on
  size_t n_la_runs = 0;
  size_t unknown = 0;              // records with an op or a length the device's runs cannot hold: left out
  wfm_seqset_t* S = nullptr;       // the sub-windows on the device, uploaded once for all the calls
  const uint32_t* cur() const { return la_runs ? la_runs : runs.data(); }
  size_t n_cur() const { return la_runs ? n_la_runs : runs.size(); }
};

// every ok record whose trimmed part has at least min_runs runs
std::unique_ptr<WindowSet> window_parts(const BiwfaBatch& b, size_t min_runs) {
  std::unique_ptr<WindowSet> w(new WindowSet());
  for (size_t i = 0; i < b.recs.size(); ++i) {
    const BiwfaRecord& r = b.recs[i];
    if (!r.ok) continue;
    const CigarOps& ops = r.ops;
    size_t ob = 0, oe = ops.size();
    uint64_t ta = 0, qa = 0;
    while (ob < oe && (ops[ob].second == 'I' || ops[ob].second == 'D')) { (ops[ob].second == 'I' ? qa : ta) += (uint64_t)ops[ob].first; ++ob; }
    while (oe > ob && (ops[oe - 1].second == 'I' || ops[oe - 1].second == 'D')) --oe;
    if (oe - ob < min_runs) continue;
    const CigarStats cs = cigar_stats(ops, ob, oe);
    wfm_problem_ref_t p = window_problem(r, ta, cs.ref_len, qa, cs.q_len);
    p.mode = WFM_MODE_END2END_UNI;  // (no reversed copies are made for it)
    wfm_result_t q{};
    q.status = 0; q.score = -1;
    q.ops_off = w->runs.size(); q.n_runs = (uint32_t)(oe - ob);
    bool known = true;
    for (size_t k = ob; k < oe; ++k) {
      const char c = ops[k].second;
      const uint32_t op = c == '=' ? 0u : c == 'X' ? 1u : c == 'I' ? 2u : c == 'D' ? 3u : 4u;
      if (op > 3u || ops[k].first <= 0 || (uint32_t)ops[k].first >= (1u << 30)) { known = false; break; }
      w->runs.push_back(((uint32_t)ops[k].first << 2) | op);
    }
    if (!known) { w->runs.resize((size_t)q.ops_off); ++w->unknown; continue; }
    q.ops_len = (uint32_t)std::min<uint64_t>(cs.ref_len + cs.q_len, 0xffffffffu);
    w->parts.push_back(WindowSet::Part{i, ob, oe});
    w->probs.push_back(p);
    w->res.push_back(q);
  }
  return w;
}

// the parts' sub-windows to the device (the caller holds the handle's lock)
int upload_windows(BiwfaBatch& b, WindowSet& w) {
  const size_t n = w.parts.size();
  if (b.store) return wfm_upload_sequence_refs(b.h, b.store, w.probs.data(), n, &w.S);
  std::vector<wfm_problem_t> plain(n);
  for (size_t i = 0; i < n; ++i) plain[i] = wfm_problem_t{w.probs[i].pattern, w.probs[i].plen, w.probs[i].text, w.probs[i].tlen, w.probs[i].mode, 0, 0, 0, 0, 0, 0};
  return wfm_upload_sequences(b.h, plain.data(), n, &w.S);
}

void release_windows(BiwfaBatch& b) {
  if (!b.windows) return;
  if (b.windows->S) {
    std::lock_guard<std::mutex> lk(handle_lock(b.h));
    wfm_free_sequences(b.h, b.windows->S);
  }
  wfm_free_runs(b.windows->la_runs);
  b.windows.reset();
}

// ---- --left-align: the interior gaps of every record's final ops moved to their leftmost placement, ONE device call per batch
// (wfm_left_align_runs).  The line's first and last runs are the problem's first and last, which the rule never touches -- no
// coordinate moves, and the CIGAR of the line is the rule applied to the line.  A record left alone is a defect; it is written as it is
// and counted.  Alone, the stage takes the records with an interior run; with --cs or --variants as well (keep) it takes every record
// those stages will work on, and leaves the uploaded windows and the new runs in b.windows for them. ----
int left_align_records(BiwfaBatch& b, bool keep) {
  const auto t0 = Clock::now();
  b.windows = window_parts(b, keep ? 1 : 3);
  WindowSet& w = *b.windows;
  std::atomic<uint64_t>* c = counts_of(SW_LEFT_ALIGN);
  c[0] += w.unknown; c[3] += w.unknown;
  if (w.parts.empty()) return 0;
  const size_t n = w.parts.size();
  std::vector<wfm_leftalign_t> la(n);
  int rc;
  {
    std::lock_guard<std::mutex> lk(handle_lock(b.h));
    rc = upload_windows(b, w);
    if (rc == WFM_OK) rc = wfm_left_align_runs(b.h, w.S, w.res.data(), w.runs.data(), w.runs.size(), &w.la_runs, &w.n_la_runs, la.data());
    if (rc < 0 && b.stats) b.stats->error = wfm_last_error(b.h);
  }
  if (rc < 0) return rc;
  std::atomic<uint64_t> gaps{0}, moved{0}, alone{0};
  for_each_record(n, b.fmt.threads, [&](size_t j) {
    const WindowSet::Part& pt = w.parts[j];
    const wfm_leftalign_t& l = la[j];
    if (l.flags) { alone.fetch_add(1); return; }
    gaps.fetch_add(l.gaps);
    if (!l.moved) return;
    moved.fetch_add(l.moved);
    CigarOps& ops = b.recs[pt.rec].ops;
    CigarOps mid;
    ops_from_runs(w.la_runs + w.res[j].ops_off, w.res[j].n_runs, mid);
    CigarOps all(ops.begin(), ops.begin() + (long)pt.b);
    all.insert(all.end(), mid.begin(), mid.end());
    all.insert(all.end(), ops.begin() + (long)pt.e, ops.end());
    ops.swap(all);
  });
  c[0] += n; c[1] += gaps.load(); c[2] += moved.load(); c[3] += alone.load();
  if (getenv("WFM_DEBUG"))
    fprintf(stderr, "[wflign] left-align: %zu records, %zu runs, %llu gaps, %llu moved, %llu left alone, %.1f ms (upload, device call, splice)\n", n, w.runs.size(),
            (unsigned long long)gaps.load(), (unsigned long long)moved.load(), (unsigned long long)alone.load(), ms_between(t0, Clock::now()));
  return 0;
}

// ---- --cs: the cs difference string of every record's line, ONE device call per batch (wfm_cs_strings) on the runs the line spells
// -- behind left_align_records, the normalised ones on the windows it uploaded.  Every ok record whose trimmed part is not empty takes
// part.  A record the device flags (its runs do not span its windows) is a defect: it is written without the field and counted. ----
int cs_records(BiwfaBatch& b) {
  const auto t0 = Clock::now();
  if (!b.windows) b.windows = window_parts(b, 1);
  WindowSet& w = *b.windows;
  if (w.parts.empty()) return 0;
  const size_t n = w.parts.size();
  std::vector<wfm_cs_t> per(n);
  char* text = nullptr;
  size_t bytes = 0;
  int rc = WFM_OK;
  auto t1 = t0;
  {
    std::lock_guard<std::mutex> lk(handle_lock(b.h));
    if (!w.S) rc = upload_windows(b, w);
    t1 = Clock::now();
    if (rc == WFM_OK) rc = wfm_cs_strings(b.h, w.S, w.res.data(), w.cur(), w.n_cur(), b.cs_form == 2 ? WFM_CS_LONG : WFM_CS_SHORT, &text, &bytes, per.data());
    if (rc < 0 && b.stats) b.stats->error = wfm_last_error(b.h);
  }
  if (rc < 0) return rc;
  const auto t2 = Clock::now();
  for_each_record(n, b.fmt.threads, [&](size_t j) {
    if (per[j].flags == 0 && per[j].len) b.recs[w.parts[j].rec].cs.assign(text + per[j].off, (size_t)per[j].len);
  });
  wfm_free_cs(text);
  if (getenv("WFM_DEBUG"))
    fprintf(stderr, "[wflign] cs (%s): %zu records, %zu runs, %zu bytes, %d flagged, %.1f ms (upload %.1f, device call %.1f, splice %.1f)\n", b.cs_form == 2 ? "long" : "short",
            n, w.n_cur(), bytes, rc, ms_between(t0, Clock::now()), ms_between(t0, t1), ms_between(t1, t2), ms_between(t2, Clock::now()));
  return 0;
}

// ---- --variants: the VCF lines of every record's line, ONE device call per batch (wfm_call_variants) on the runs the line spells --
// behind left_align_records the normalised ones -- on the windows the stages before uploaded, if any did.  Every ok record whose trimmed
// part is not empty takes part; a part begins and ends with an = or X run, so it has no end gaps and every gap of it is called.  The
// line's coordinates are the writer's (write_alignment_paf): POS = the target start it writes + p + 1; [QSTART, QEND) = the span
// [t, t + n) of the line's text -- n = 1 for an SNV, the inserted bases for an INS, 0 for a DEL -- on the query's forward strand.  Masked
// SNVs are left out and counted.  A record the device flags is a defect: it has no lines and is counted.  With --genotypes the records and
// their alleles stay in the batch (b.calls) for genotype_records; with --genotypes alone no line is spelled. ----
int variant_records(BiwfaBatch& b) {
  const auto t0 = Clock::now();
  if (!b.windows) b.windows = window_parts(b, 1);
  WindowSet& w = *b.windows;
  if (w.parts.empty()) return 0;
  const size_t n = w.parts.size();
  std::vector<wfm_varcall_t> per(n);
  wfm_variant_t* vars = nullptr;
  char* alleles = nullptr;
  size_t n_vars = 0, bytes = 0;
  int rc = WFM_OK;
  auto t1 = t0;
  {
    std::lock_guard<std::mutex> lk(handle_lock(b.h));
    if (!w.S) rc = upload_windows(b, w);
    t1 = Clock::now();
    if (rc == WFM_OK) rc = wfm_call_variants(b.h, w.S, w.res.data(), w.cur(), w.n_cur(), &vars, &n_vars, &alleles, &bytes, per.data());
    if (rc < 0 && b.stats) b.stats->error = wfm_last_error(b.h);
  }
  if (rc < 0) return rc;
  const auto t2 = Clock::now();
  if (b.variants) for_each_record(n, b.fmt.threads, [&](size_t j) {
    if (per[j].flags) return;
    const WindowSet::Part& pt = w.parts[j];
    BiwfaRecord& r = b.recs[pt.rec];
    r.vcf_called = true;
    // where the part begins in the record's windows, as trim_and_filter will find it
    uint64_t ta = 0, qa = 0;
    for (size_t k = 0; k < pt.b; ++k) (r.ops[k].second == 'I' ? qa : ta) += (uint64_t)r.ops[k].first;
    const uint64_t ts = r.target_offset + ta, q_len = (uint64_t)w.probs[j].tlen;
    const uint64_t qs = r.query_is_rev ? r.query_offset + (r.query_length - qa - q_len) : r.query_offset + qa, qe = qs + q_len;
    std::string tail = "\t.\t.\tQNAME=" + r.query_name + ";QSTART=";
    char num[64];
    for (uint64_t k = per[j].first; k < per[j].first + per[j].count; ++k) {
      const wfm_variant_t& v = vars[k];
      if (v.kind & WFM_VAR_MASKED) { ++r.vcf_masked; continue; }
      const uint32_t kind = v.kind & 255u;
      const uint64_t span = kind == WFM_VAR_SNV ? 1u : kind == WFM_VAR_INS ? v.alt_len - 1u : 0u;
      const uint64_t a = r.query_is_rev ? qe - v.t - span : qs + v.t;
      r.vcf += r.target_name;
      r.vcf.append(num, (size_t)snprintf(num, sizeof num, "\t%llu\t.\t", (unsigned long long)(ts + v.p + 1)));
      r.vcf.append(alleles + v.off, v.ref_len);
      r.vcf += '\t';
      r.vcf.append(alleles + v.off + v.ref_len, v.alt_len);
      r.vcf += tail;
      r.vcf.append(num, (size_t)snprintf(num, sizeof num, "%llu;QEND=%llu;QSTRAND=%c\n", (unsigned long long)a, (unsigned long long)(a + span),
                                         r.query_is_rev ? '-' : '+'));
    }
  });
  if (b.passes->on[SW_GENOTYPES]) {
    b.calls.reset(new KeptCalls());
    b.calls->vars = vars; b.calls->alleles = alleles;
    b.calls->per = std::move(per);
    b.calls->rec.resize(n);
    for (size_t j = 0; j < n; ++j) b.calls->rec[j] = w.parts[j].rec;
  } else {
    wfm_free_variants(vars, alleles);
  }
  if (getenv("WFM_DEBUG"))
    fprintf(stderr, "[wflign] variants: %zu records, %zu runs, %zu variants, %zu allele bytes, %d flagged, %.1f ms (upload %.1f, device call %.1f, text %.1f)\n",
            n, w.n_cur(), n_vars, bytes, rc, ms_between(t0, Clock::now()), ms_between(t0, t1), ms_between(t1, t2), ms_between(t2, Clock::now()));
  return 0;
}

// ---- --maf: the two gapped rows of every record's line in the blocks of a pairwise MAF, ONE device call per batch (wfm_maf_rows) on the
// runs the line spells -- behind left_align_records the normalised ones -- on the windows the stages before uploaded, if any did.  Every
// ok record whose trimmed part is not empty takes part; a part begins and ends with an = or X run, so every block begins and ends with an
// aligned column.  The coordinates are the writer's (variant_records' ts, qs, qe) through maf_text.hpp.  A record the device flags is a
// defect: it has no blocks and is counted. ----
static_assert(sizeof(maf::Block) == sizeof(wfm_maf_block_t), "maf_text.hpp restates wfm_maf_block_t");
int maf_records(BiwfaBatch& b) {
  const auto t0 = Clock::now();
  if (!b.windows) b.windows = window_parts(b, 1);
  WindowSet& w = *b.windows;
  if (w.parts.empty()) return 0;
  const size_t n = w.parts.size();
  std::vector<wfm_mafcall_t> per(n);
  wfm_maf_block_t* blocks = nullptr;
  char* rows = nullptr;
  size_t n_blocks = 0, bytes = 0;
  int rc = WFM_OK;
  auto t1 = t0;
  {
    std::lock_guard<std::mutex> lk(handle_lock(b.h));
    if (!w.S) rc = upload_windows(b, w);
    t1 = Clock::now();
    if (rc == WFM_OK) rc = wfm_maf_rows(b.h, w.S, w.res.data(), w.cur(), w.n_cur(), b.maf_split, &blocks, &n_blocks, &rows, &bytes, per.data());
    if (rc < 0 && b.stats) b.stats->error = wfm_last_error(b.h);
  }
  if (rc < 0) return rc;
  const auto t2 = Clock::now();
  for_each_record(n, b.fmt.threads, [&](size_t j) {
    if (per[j].flags) return;
    const WindowSet::Part& pt = w.parts[j];
    BiwfaRecord& r = b.recs[pt.rec];
    r.maf_called = true;
    // where the part begins in the record's windows, as trim_and_filter will find it
    uint64_t ta = 0, qa = 0;
    for (size_t k = 0; k < pt.b; ++k) (r.ops[k].second == 'I' ? qa : ta) += (uint64_t)r.ops[k].first;
    const uint64_t q_len = (uint64_t)w.probs[j].tlen;
    const uint64_t qs = r.query_is_rev ? r.query_offset + (r.query_length - qa - q_len) : r.query_offset + qa;
    const maf::Line line{&r.target_name, r.target_offset + ta, r.target_total_length, &r.query_name, qs, qs + q_len, r.query_total_length, r.query_is_rev};
    const maf::Block* mine = reinterpret_cast<const maf::Block*>(blocks) + per[j].first;
    r.maf.reserve(maf::record_bytes(line, mine, (size_t)per[j].count));
    for (uint64_t k = 0; k < per[j].count; ++k) {
      maf::block(r.maf, line, mine[k], rows);
      r.maf_cols += mine[k].cols;
    }
    r.maf_blocks = (uint32_t)per[j].count;
  });
  wfm_free_maf(blocks, rows);
  if (getenv("WFM_DEBUG"))
    fprintf(stderr, "[wflign] maf (split %u): %zu records, %zu runs, %zu blocks, %zu row bytes, %d flagged, %.1f ms (upload %.1f, device call %.1f, text %.1f)\n",
            b.maf_split, n, w.n_cur(), n_blocks, bytes, rc, ms_between(t0, Clock::now()), ms_between(t0, t1), ms_between(t1, t2), ms_between(t2, Clock::now()));
  return 0;
}

// --maf: a record's blocks go out with its line or not at all
void account_maf(BiwfaRecord& r, bool written) {
  if (!written) { r.maf.clear(); return; }
  std::atomic<uint64_t>* c = counts_of(SW_MAF);
  if (!r.maf_called || r.maf_blocks == 0) { c[3] += 1; return; }  // (flagged by the device, or runs it cannot hold)
  c[0] += 1; c[1] += r.maf_blocks; c[2] += r.maf_cols;
}

// --variants: a record's lines go out with its line or not at all
void account_variants(BiwfaRecord& r, bool written) {
  if (!written) { r.vcf.clear(); return; }
  std::atomic<uint64_t>* c = counts_of(SW_VARIANTS);
  if (!r.vcf_called) { c[3] += 1; return; }  // (flagged by the device, or runs it cannot hold)
  c[0] += 1; c[2] += r.vcf_masked;
  c[1] += (uint64_t)std::count(r.vcf.begin(), r.vcf.end(), '\n');
}

// ---- record (wflign.cpp:434-454) ----
void write_record(BiwfaBatch& b, size_t ri) {
  BiwfaRecord& r = b.recs[ri];
  r.written = false;
  if (!r.ok) return;
  bool written;
  if (b.fmt.paf_format_else_sam)
    written = write_alignment_paf(r.paf, r.ops, r.query_name, r.query_total_length, r.query_offset, r.query_length, r.query_is_rev,
                        r.target_name, r.target_total_length, r.target_offset, b.pp, r.mashmap_estimated_identity, r.chain_id,
                        r.chain_length, r.chain_pos);
  else
    written = write_alignment_sam(r.paf, r.ops, r.query_name, r.query_offset, r.query_is_rev, r.target_name, r.target_offset, b.pp,
                        r.mashmap_estimated_identity, b.fmt.no_seq_in_sam, b.fmt.emit_md_tag, r.query, r.target, r.chain_id,
                        r.chain_length, r.chain_pos);
  r.written = written;
  if (b.variants) account_variants(r, written);
  if (b.maf) account_maf(r, written);
  if (!b.cs_form || !written) return;
  if (r.cs.empty()) { counts_of(SW_CS)[2] += 1; return; }  // (flagged by the device, or runs it cannot hold)
  // the last field of the line, before its closing newline
  r.paf.pop_back();
  r.paf.reserve(r.paf.size() + r.cs.size() + 7);
  r.paf += "\tcs:Z:";
  r.paf += r.cs;
  r.paf += '\n';
  counts_of(SW_CS)[0] += 1; counts_of(SW_CS)[1] += r.cs.size();
}
// ---- the written records of a batch as the align driver's passes take them, packed ONCE per batch (packed_runs.hpp).  It runs behind
// write_record, where the filters have spoken.  A record's base = the target sequence's offset in the concatenation + the target start
// the writer wrote -- variant_records' ts.  A record whose ops the runs cannot hold is a defect: it is in no list, and every stage counts
// and reports it.  The names go along where a pass that writes them is on (--lift, --chain, --chain-net). ----
PackedRuns pack_written(const BiwfaBatch& b) {
  const auto t0 = Clock::now();
  PackedRuns pk;
  pk.order_base = b.passes->batch << 32;
  const bool with_names = b.passes->on[SW_LIFT] || b.passes->on[SW_CHAIN] || b.passes->on[SW_CHAIN_NET];
  for (size_t ri = 0; ri < b.recs.size(); ++ri) {
    const BiwfaRecord& r = b.recs[ri];
    if (!r.ok || !r.written) continue;
    chain::Record cr;
    if (with_names) { cr.qname = r.query_name; cr.tname = r.target_name; }
    cr.rev = r.query_is_rev;
    cr.qsize = r.query_total_length; cr.tsize = r.target_total_length;
    cr.qs = r.query_offset; cr.qe = r.query_offset + r.query_length; cr.ts = r.target_offset;
    if (pack_ops(pk, r.ops, std::move(cr), Place{r.pav_group, r.query_global, r.target_global}) == 1) pk.rec.push_back(ri);
  }
  pk.ms = ms_between(t0, Clock::now());
  return pk;
}

// ---- --genotypes: the variants variant_records called for the records WRITTEN (masked SNVs left out), each at its global position --
// the problem's base + p -- under the column of its query's group, and the same records' runs for the = union: one wfm_sites_add_variants
// and one wfm_sites_add_ref call per batch.  A record without calls (the device flagged it) or without a column never goes to the device;
// it adds nothing, is counted and reported, as one the device refuses. ----
int genotype_records(BiwfaBatch& b, const PackedRuns& pk) {
  auto t0 = Clock::now(), t1 = t0;
  const KeptCalls* kc = b.calls.get();
  const uint32_t n_groups = (uint32_t)b.passes->tables->columns.keys.size();
  wfm_sites_t* sites = b.passes->get<wfm_sites_t>(SW_GENOTYPES);
  std::vector<size_t> part_of(b.recs.size(), (size_t)-1);
  if (kc) for (size_t j = 0; j < kc->rec.size(); ++j) part_of[kc->rec[j]] = j;
  std::vector<wfm_site_var_t> vars;
  std::string alleles;
  std::vector<wfm_pav_prob_t> probs;
  uint64_t alone = pk.unknown;
  for (size_t j = 0; j < pk.probs.size(); ++j) {
    const uint32_t group = pk.place[j].group;
    const size_t part = part_of[pk.rec[j]];
    if (part == (size_t)-1 || kc->per[part].flags || group >= n_groups) { ++alone; continue; }
    probs.push_back(wfm_pav_prob_t{pk.probs[j].base, pk.probs[j].runs_off, pk.probs[j].n_runs, group});
    const wfm_varcall_t& pc = kc->per[part];
    for (uint64_t k = pc.first; k < pc.first + pc.count; ++k) {
      const wfm_variant_t& v = kc->vars[k];
      if (v.kind & WFM_VAR_MASKED) continue;
      vars.push_back(wfm_site_var_t{pk.probs[j].base + v.p, v.kind & 255u, group, v.ref_len, v.alt_len, (uint64_t)alleles.size()});
      alleles.append(kc->alleles + v.off, (size_t)v.ref_len + v.alt_len);
    }
  }
  std::vector<uint32_t> flags(probs.size());
  std::string error;
  const int rc = device_call(b.h, probs.size(), t1, error, [&] {
    const int rv = wfm_sites_add_variants(b.h, sites, vars.data(), vars.size(), alleles.data(), alleles.size());
    return rv != WFM_OK ? rv : wfm_sites_add_ref(b.h, sites, probs.data(), probs.size(), pk.runs.data(), pk.runs.size(), flags.data());
  });
  if (rc < 0) { if (b.stats) b.stats->error = error; return rc; }
  std::atomic<uint64_t>* c = counts_of(SW_GENOTYPES);
  c[0] += probs.size() - (uint64_t)rc; c[3] += alone + (uint64_t)rc;
  if (rc > 0 || alone)
    fprintf(stderr, "[wflign] genotypes: %llu records of a batch were NOT added (no calls, runs that leave the target or cannot be held, or a query without a column)\n",
            (unsigned long long)((uint64_t)rc + alone));
  if (getenv("WFM_DEBUG"))
    fprintf(stderr, "[wflign] genotypes: %zu records, %zu variants, %zu allele bytes, %zu runs, %d flagged, %.1f ms (host lists %.1f, device calls %.1f)\n", probs.size(),
            vars.size(), alleles.size(), pk.runs.size(), rc, ms_between(t0, Clock::now()), ms_between(t0, t1), ms_between(t1, Clock::now()));
  return 0;
}

// the stages behind pack_written, in the order they run, and what the align driver says of the records a stage left out: those the device
// refused and those that never went to it (pk.unknown)
const struct { SwitchId id; const char* tag; const char* left_out; } kRunStages[] = {
    {SW_COVERAGE, "coverage", "were NOT added to the depth (their runs leave the target or cannot be held)"},
    {SW_PAV, "pav", "were NOT added (their runs leave the target or cannot be held, or their query has no column)"},
    {SW_GENOTYPES, "genotypes", nullptr},  // (genotype_records: it needs variant_records' kept calls, and reports for itself)
    {SW_LIFT, "lift", "were NOT lifted (their runs leave the target or cannot be held)"},
    {SW_CHAIN, "chain", "have NO chain (their runs cannot be held)"},
    {SW_CHAIN_NET, "chain-net", "were NOT added (their runs leave the target or cannot be held)"},
    {SW_TRANSITIVE, "transitive", "were NOT added (their runs leave their sequences or cannot be held)"}};

// a stage of run_passes.hpp on the batch, reported the align driver's way: its counts into the switch's, the warning, the WFM_DEBUG line
int run_stage(BiwfaBatch& b, SwitchId id, const char* tag, const char* left_out, PackedRuns& pk) {
  const StageOutcome o = stage_of(id)(b.h, b.fmt.threads, *b.passes, pk);
  if (o.rc < 0) { if (b.stats) b.stats->error = o.error; return o.rc; }
  std::atomic<uint64_t>* c = counts_of(id);
  for (int k = 0; k < 3; ++k) c[k] += o.counts[k];
  if (o.refused || pk.unknown) fprintf(stderr, "[wflign] %s: %llu records of a batch %s\n", tag, (unsigned long long)(o.refused + pk.unknown), left_out);
  if (!o.debug.empty()) fputs(o.debug.c_str(), stderr);
  return 0;
}

void set_switch(SwitchId id, bool on, const char* out, const char* bed, uint64_t option) {
  Switch& s = g_switch[id];
  for (auto& a : s.counts) a.store(0);
  {
    std::lock_guard<std::mutex> lk(s.mu);
    s.out = on && out ? out : "";
    s.bed = on && bed ? bed : "";
    s.option.store(option);
  }
  s.on.store(on);
}
int switch_counts(SwitchId id, uint64_t out[4]) {
  if (!out) return WFM_E_ARG;
  for (int q = 0; q < 4; ++q) out[q] = g_switch[id].counts[q].load();
  return WFM_OK;
}
bool named(const char* path) { return path && *path; }
}  // namespace

SwitchSetting switch_setting(SwitchId id) {
  Switch& s = g_switch[id];
  std::lock_guard<std::mutex> lk(s.mu);
  const bool on = s.on.load();
  return SwitchSetting{on ? s.out : std::string(), on ? s.bed : std::string(), s.option.load()};
}

void switch_finished(SwitchId id, uint64_t c1, uint64_t c2, uint64_t c3) {
  std::atomic<uint64_t>* c = counts_of(id);
  c[1] += c1; c[2] += c2; c[3] += c3;
}

int do_biwfa_alignment_batch(wfm_handle_t* h, std::vector<BiwfaRecord>& recs, const wflign_penalties_t& penalties,
                             bool disable_chain_patching, const PafParams& pp, BiwfaStats* stats, const OutputFormat& fmt,
                             ResidentSeqs* resident, const BatchPasses* passes, BatchTexts* texts) {
  const bool dbg = getenv("WFM_DEBUG") != nullptr;
  const auto ts0 = Clock::now();
  const size_t n = recs.size();
  static const BatchPasses no_passes;
  BiwfaBatch b{h, recs, penalties,
               wfm_penalties_t{penalties.mismatch, penalties.gap_opening1, penalties.gap_extension1, penalties.gap_opening2, penalties.gap_extension2},
               pp, stats, fmt, resident, resident ? resident->store : nullptr, passes ? passes : &no_passes, texts,
               std::vector<BiwfaBatch::Work>(n), std::vector<char>(n, 0)};
  int rc = align_main(b, !disable_chain_patching);
  if (rc < 0) return rc;
  warn_over_budget(b);
  const auto ts1 = Clock::now();
  if (!disable_chain_patching) {
    GpuBatch g;  // (its runs are freed behind the late tails' call)
    if ((rc = patch_ends(b, g)) < 0) return rc;
    if (b.later && (rc = patch_late_tails(b)) < 0) return rc;
    if (stats) { stats->head_patches += b.n_head.load(); stats->tail_patches += b.n_tail.load(); }
  }
  const auto ts2 = Clock::now();
  const bool left = is_on(SW_LEFT_ALIGN);
  b.cs_form = is_on(SW_CS) ? (int)g_switch[SW_CS].option.load(std::memory_order_relaxed) : 0;
  b.variants = is_on(SW_VARIANTS);
  const bool calls = b.variants || b.passes->on[SW_GENOTYPES];  // (--genotypes takes variant_records' calls, with or without the file of --variants)
  b.maf = is_on(SW_MAF);
  b.maf_split = b.maf ? (uint32_t)g_switch[SW_MAF].option.load(std::memory_order_relaxed) : 0;
  if (left || b.cs_form || calls || b.maf) {  // the two halves with the device calls between them
    for_each_record(n, fmt.threads, [&](size_t ri) { swizzle(b, ri); });
    if (left) rc = left_align_records(b, b.cs_form != 0 || calls || b.maf);
    if (rc >= 0 && b.cs_form) rc = cs_records(b);
    if (rc >= 0 && calls) rc = variant_records(b);
    if (rc >= 0 && b.maf) rc = maf_records(b);
    release_windows(b);
    if (rc < 0) return rc;
    for_each_record(n, fmt.threads, [&](size_t ri) { write_record(b, ri); });
  } else {
    for_each_record(n, fmt.threads, [&](size_t ri) { swizzle(b, ri); write_record(b, ri); });
  }
  bool any = false;
  for (const auto& s : kRunStages) any = any || b.passes->on[s.id];
  if (any) {  // one packing for the stages that are on; each makes its own device call
    PackedRuns pk = pack_written(b);
    for (const auto& s : kRunStages)
      if (b.passes->on[s.id] && (rc = s.left_out ? run_stage(b, s.id, s.tag, s.left_out, pk) : genotype_records(b, pk)) < 0) return rc;
    if (b.texts) take_texts(pk, *b.texts);
  }
  if (dbg)
    fprintf(stderr, "[wflign] %zu records: main alignment + runs + scans %.1f ms (incl. waiting for the device), patches %.1f ms (%zu tails scanned after their heads), swizzle + records %.1f ms\n",
            n, ms_between(ts0, ts1), ms_between(ts1, ts2), b.later, ms_between(ts2, Clock::now()));
  return 0;
}

}  // namespace wflign

extern "C" {

using namespace wflign;

void wfmh_set_verify_optimal(int on, uint64_t max_cells) { set_switch(SW_VERIFY_OPTIMAL, on != 0, nullptr, nullptr, on ? max_cells : 0); }
void wfmh_set_left_align(int on) { set_switch(SW_LEFT_ALIGN, on != 0, nullptr, nullptr, 0); }
void wfmh_set_cs(int form) { set_switch(SW_CS, form == 1 || form == 2, nullptr, nullptr, (uint64_t)form); }
void wfmh_set_variants(const char* path_or_null) { set_switch(SW_VARIANTS, named(path_or_null), path_or_null, nullptr, 0); }
void wfmh_set_genotypes(const char* path_or_null) { set_switch(SW_GENOTYPES, named(path_or_null), path_or_null, nullptr, 0); }
void wfmh_set_coverage(const char* path_or_null) { set_switch(SW_COVERAGE, named(path_or_null), path_or_null, nullptr, 0); }
void wfmh_set_chain_net(const char* path_or_null) { set_switch(SW_CHAIN_NET, named(path_or_null), path_or_null, nullptr, 0); }
void wfmh_set_lift(const char* bed_path_or_null, const char* out_path_or_null) {
  set_switch(SW_LIFT, named(bed_path_or_null) && named(out_path_or_null), out_path_or_null, bed_path_or_null, 0);
}
void wfmh_set_chain(const char* path_or_null, int swap) { set_switch(SW_CHAIN, named(path_or_null), path_or_null, nullptr, named(path_or_null) && swap != 0); }
void wfmh_set_maf(const char* path_or_null, uint32_t split) { set_switch(SW_MAF, named(path_or_null), path_or_null, nullptr, named(path_or_null) ? split : 0); }
void wfmh_set_transitive(const char* bed_path_or_null, const char* out_path_or_null, uint32_t depth) {
  set_switch(SW_TRANSITIVE, named(bed_path_or_null) && named(out_path_or_null), out_path_or_null, bed_path_or_null, depth);
}
void wfmh_set_pav(const char* bed_path_or_null, uint64_t window, const char* out_path_or_null) {
  const bool bed = named(bed_path_or_null);
  const bool on = named(out_path_or_null) && (bed != (window != 0));  // (one of the two, never both)
  set_switch(SW_PAV, on, out_path_or_null, bed ? bed_path_or_null : nullptr, on && !bed ? window : 0);
}

int wfmh_verify_optimal_counts(uint64_t out[4]) { return switch_counts(SW_VERIFY_OPTIMAL, out); }
int wfmh_left_align_counts(uint64_t out[4]) { return switch_counts(SW_LEFT_ALIGN, out); }
int wfmh_cs_counts(uint64_t out[4]) { return switch_counts(SW_CS, out); }
int wfmh_variants_counts(uint64_t out[4]) { return switch_counts(SW_VARIANTS, out); }
int wfmh_genotypes_counts(uint64_t out[4]) { return switch_counts(SW_GENOTYPES, out); }
int wfmh_coverage_counts(uint64_t out[4]) { return switch_counts(SW_COVERAGE, out); }
int wfmh_lift_counts(uint64_t out[4]) { return switch_counts(SW_LIFT, out); }
int wfmh_chain_counts(uint64_t out[4]) { return switch_counts(SW_CHAIN, out); }
int wfmh_chain_net_counts(uint64_t out[4]) { return switch_counts(SW_CHAIN_NET, out); }
int wfmh_transitive_counts(uint64_t out[4]) { return switch_counts(SW_TRANSITIVE, out); }
int wfmh_pav_counts(uint64_t out[4]) { return switch_counts(SW_PAV, out); }
int wfmh_maf_counts(uint64_t out[4]) { return switch_counts(SW_MAF, out); }

}  // extern "C"
