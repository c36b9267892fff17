// wflign_hip.hpp -- host side of the align path above the C ABI.
//
// Mirrors the live part of the reference's wflign layer
// (src/common/wflign/src/wflign.cpp:19-483, wflign_swizzle.cpp:7-299,
// wflign_patch.cpp:139-283,2611-2734), re-organised for batches: the reference
// aligns one mapping record per Taskflow task; here every stage of
// do_biwfa_alignment runs over a whole batch so each stage is one
// wfm_align_batch call on the GPU:
//   align_main         main BiWFA alignment, runs, plan_patches      (wflign.cpp:136-165)
//   patch_ends         ends-free head and tail patches, one call for both
//                                                            (wflign.cpp:241-320, 323-418)
//   patch_late_tails   the tails whose scan has to see the patched head  (wflign.cpp:323-418)
//   swizzle            the two end swaps                       (wflign.cpp:423-433)
//   left_align_records --left-align only: every interior gap to its leftmost placement, one wfm_left_align_runs call
//   cs_records         --cs only: the cs difference string of every record's line, one wfm_cs_strings call (on the windows
//                      left_align_records uploaded, where both are on)
//   variant_records    --variants and --genotypes only: the VCF lines of every record's line, one wfm_call_variants call (on the same
//                      windows, uploaded once whichever of the switches are on); --genotypes keeps the calls for genotype_records
//   write_record       PAF / SAM record (+ cs:Z: as its last field)   (wflign.cpp:434-454)
//   pack_written      the records WRITTEN as packed runs (packed_runs.hpp), once per batch, for the stages below: nothing goes up but runs, and
//                      whether a record is written is only known behind write_record
//   genotype_records   --genotypes only: the kept calls of every record WRITTEN at their global positions, and the records' runs, into
//                      the handle's sites object, one wfm_sites_add_variants and one wfm_sites_add_ref call
//   the stages of run_passes.hpp, which an aligned PAF feeds as well (the --*-paf modes), each wrapped here by what the align driver
//   reports -- the switch's counts, the warning about records left out, the WFM_DEBUG line:
//     coverage_records   --coverage: the runs into the handle's depth object, one wfm_coverage_add call
//     pav_records        --pav: the runs, with the column of the query's group, into the handle's presence object, one wfm_pav_add call
//     lift_records       --lift: the BED intervals lifted through the runs, one wfm_lift_runs call, the record's lines into PackedRuns::lift
//     chain_records      --chain: the runs compacted to the blocks and gaps of a UCSC chain, one wfm_chain_runs call, the record's chain
//                        without its id into PackedRuns::chain
//     net_records        --chain-net: the runs into the handle's net object, one wfm_net_add call, each with score = its = columns and
//                        order = batch << 32 | its index among the batch's records packed; what the chain's header needs stays on the
//                        host, keyed by the order
//     trans_records      --transitive: the runs into the handle's trans object with the record's two places in the world, one
//                        wfm_trans_add call
// and CIGARs are runs (count, op) from the device to the record's text: nothing is expanded to one byte per base.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <functional>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/wfmash_hip.h"
#include "chain_text.hpp"
#include "cigar_ops.hpp"  // CigarOps, the CIGAR helpers, plan_patches, PafParams and the two record writers
#include "lift_text.hpp"
#include "pav_text.hpp"
#include "transitive_text.hpp"

namespace wflign {

// wflign_penalties_t (wflign_alignment.hpp:21)
struct wflign_penalties_t {
  int match = 0;
  int mismatch = 5;
  int gap_opening1 = 8;
  int gap_extension1 = 2;
  int gap_opening2 = 24;
  int gap_extension2 = 1;
};

// ---- batch form of do_biwfa_alignment (wflign.cpp:108-483) ----
struct BiwfaRecord {
  std::string query_name;
  const char* query = nullptr;       // strand-adjusted, upper-case, length query_length
  uint64_t query_total_length = 0, query_offset = 0, query_length = 0;
  bool query_is_rev = false;
  std::string target_name;
  const char* target = nullptr;      // points at rStartPos inside the fetched (padded) buffer
  uint64_t target_total_length = 0, target_offset = 0, target_length = 0;
  uint64_t target_avail = 0;         // bytes readable from `target` (length incl. tail padding)
  float mashmap_estimated_identity = 0;
  int32_t chain_id = -1, chain_length = 1, chain_pos = 1;
  // The two windows by reference (ResidentSeqs): id in the device's sequence store (-1: the side goes by its host pointer), forward
  // offset of the window in that sequence; the query's strand is query_is_rev.  With both ids set `query` and `target` may be null
  // (PAF output): the record's bases are then fetched on the host only if the swizzle asks for them.
  int32_t target_seq = -1, query_seq = -1;
  int64_t target_win_off = 0, query_win_off = 0;
  // outputs
  bool ok = false;
  int32_t score = -1;
  CigarOps ops;                      // final CIGAR as runs (after patching + swizzle)
  std::string paf;                   // the record's line incl. newline, as the align driver writes it ("" if filtered)
  std::string cs;                    // --cs: the cs string of the line's runs, without its tag ("" if off, or if the record has none)
  std::string vcf;                   // --variants: the VCF lines of the line's variants, each with its newline ("" if off, filtered, or none)
  bool vcf_called = false;           // ... the device called the record's variants (false: off, or the record was left alone)
  uint32_t vcf_masked = 0;           // ... SNVs left out of `vcf` because a base of theirs is not one of ACGT
  uint64_t target_global = 0;        // --coverage, --lift: where the target sequence begins in the concatenation of the target's sequences
  bool written = false;              // the filters let the record's line through (write_record)
  uint32_t pav_group = 0;            // --pav, --genotypes: the column of the query sequence's group
  uint64_t query_global = 0;         // --transitive: where the query sequence begins in the world (target_global is the target's place in it)
  std::string maf;                   // --maf: the paragraphs of the record's blocks (maf_text.hpp; "" if off, filtered, or the record has none)
  bool maf_called = false;           // ... the device spelled the record's rows (false: off, or the record was left alone)
  uint32_t maf_blocks = 0;           // ... the blocks in `maf`
  uint64_t maf_cols = 0;             // ... and their columns
  uint32_t tags = 0;                 // WFM_PF_* of the main alignment | of the head patch << 8 | of the tail patch << 16 (diagnostics: WFM_RECORD_TAGS)
};

struct BiwfaStats {
  uint64_t cells = 0;
  double ms_gpu = 0;
  uint64_t cells_tile = 0, tile_launches = 0;  // the tile kernels' share: unique cells, launches, summed launch durations
  double ms_tile = 0;
  uint64_t main_failed = 0, head_patches = 0, tail_patches = 0;
  std::string error;                 // the device call's message when do_biwfa_alignment_batch returns < 0
  std::vector<std::pair<double, double>> busy;  // when kernels of this batch's device calls ran (ms on the device's clock, wfm_get_busy_intervals)
};

// The sub-window [a, b) of a side that is the window of win_len bases at forward offset win_off of a stored sequence,
// reverse-complemented when rev: the forward offset of the same bases (their length stays b - a, the strand flag stays rev).
// For a '-' record the sub-window [a, b) of the reverse-complemented query window [qs, qe) is the forward window [qe - b, qe - a).
inline int64_t sub_window_off(int64_t win_off, int64_t win_len, bool rev, int64_t a, int64_t b) {
  (void)a;
  return rev ? win_off + win_len - b : win_off + a;
}

// Problems by reference for a batch (wfmh_align_params_t::resident_sequences): the store of the handle's device, and how the host
// gets at the bases of a record that came without them -- fetch(i) fills recs[i].query / target / target_avail exactly as the
// eager path does (fetch + makeUpperCaseAndValidDNA + reverse complement); it is called from the batch's worker threads.
struct ResidentSeqs {
  const wfm_seqstore_t* store = nullptr;
  std::function<void(size_t)> fetch;
  std::atomic<uint64_t> lazy_fetches{0};
};

// A handle runs one call at a time; the mutex every caller of a handle's device entry points holds meanwhile.
std::mutex& handle_lock(wfm_handle_t* h);

// --chain-net: what a record's chain needs beside its pieces, kept on the host under the order the record went to the net object with
using NetHead = chain::NetHead;

struct OutputFormat {
  bool paf_format_else_sam = true;   // wflign.cpp:434
  bool no_seq_in_sam = false;
  bool emit_md_tag = false;
  int threads = 1;                   // host threads for the per-record CIGAR / PAF work of a batch
};

// ---- the process-wide switches: one record each (wflign_hip.cpp), named by these ids ----
enum SwitchId {
  SW_VARIANTS, SW_COVERAGE, SW_LIFT, SW_CHAIN, SW_PAV, SW_GENOTYPES, SW_CHAIN_NET, SW_TRANSITIVE, SW_MAF,  // the align driver's passes, in their order
  SW_LEFT_ALIGN, SW_CS, SW_VERIFY_OPTIMAL,
  N_SWITCHES,
  N_PASSES = SW_MAF + 1
};

// What wfmh_set_* named: the file the align phase writes ("" while the switch is off), the BED it reads ("" while off, or without one) and
// the switch's integer (--pav: the window size, 0 with a BED; --chain: 1 if the two sides change places; --transitive: the depth; --maf: the split)
struct SwitchSetting {
  std::string out, bed;
  uint64_t option = 0;
};
SwitchSetting switch_setting(SwitchId id);
// what the align phase adds to the switch's counts 1, 2 and 3 once it has read a BED or written the file (count 0 is the stages')
void switch_finished(SwitchId id, uint64_t c1, uint64_t c2, uint64_t c3);

// ---- the align driver's passes as a batch sees them ----
// The run's constant tables: the two files' names and lengths, where each target sequence begins in the concatenation (nseq + 1 values),
// and what single passes look up per record.
struct RunTables {
  std::vector<std::string> tnames, qnames;
  std::vector<uint64_t> tlengths, qlengths, seq_offsets;
  std::function<int(const std::string&)> find_target;  // a target name's index, or a negative number
  pav::Columns columns;                 // --pav, --genotypes: the groups and the column of every query sequence
  std::vector<lift::Interval> lift_iv;   // --lift: the BED's intervals in the order of the handle's liftset
  bool chain_swap = false;               // --chain: the query is the chain's first side
  transitive::World world;               // --transitive: the target's sequences, then the query's that no target names
  std::vector<uint64_t> query_world;     // ... and where each query sequence begins in it
};
// in: which passes are on, the object of the batch's handle for each pass that has one, the batch's number and the tables
struct BatchPasses {
  bool on[N_PASSES] = {};
  void* object[N_PASSES] = {};
  uint64_t batch = 0;
  const RunTables* tables = nullptr;
  template <class T>
  T* get(SwitchId id) const { return static_cast<T*>(object[id]); }
  bool any() const { return std::any_of(on, on + N_PASSES, [](bool b) { return b; }); }
};
// out: the batch's PAF / SAM text (an align batch's), the text of each pass that writes per batch (--variants, --lift, --chain, --maf; in the order
// of the records' lines), and --chain-net's heads of the records added
struct BatchTexts {
  std::string paf;
  std::string text[N_PASSES];
  std::vector<NetHead> net_heads;
};

int do_biwfa_alignment_batch(wfm_handle_t* h, std::vector<BiwfaRecord>& recs, const wflign_penalties_t& penalties,
                             bool disable_chain_patching, const PafParams& pp, BiwfaStats* stats,
                             const OutputFormat& fmt = OutputFormat(), ResidentSeqs* resident = nullptr, const BatchPasses* passes = nullptr,
                             BatchTexts* texts = nullptr);

}  // namespace wflign
