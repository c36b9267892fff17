// aligner.hpp -- align driver above the C ABI: counterpart of align::Aligner
// (src/align/include/computeAlignments.hpp:142-738).  Same call surface
// (Parameters, MappingBoundaryRow, parseMashmapRow, compute) but records are
// processed in batches so that every wflign stage is one GPU launch set instead
// of one Taskflow task per record (computeAlignments.hpp:398-435).
#pragma once

#include <chrono>
#include <cstdint>
#include <iosfwd>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/wfmash_hip.h"
#include "align_plan.hpp"
#include "fasta.hpp"
#include "wflign_hip.hpp"

namespace align {

enum strnd : int16_t { FWD = 1, AMBIG = 0, REV = -1 };  // skch::strnd (base_types.hpp)

// align::Parameters (align_parameters.hpp:16), fields the live path reads
struct Parameters {
  int threads = 1;
  float min_identity = 0;                 // parse_args.hpp:566
  uint64_t min_alignment_length = 32;     // parse_args.hpp:572
  float min_block_identity = 0.1f;        // parse_args.hpp:583
  int wfa_patching_mismatch_score = 5;    // parse_args.hpp:290-294
  int wfa_patching_gap_opening_score1 = 8;
  int wfa_patching_gap_extension_score1 = 2;
  int wfa_patching_gap_opening_score2 = 24;
  int wfa_patching_gap_extension_score2 = 1;
  uint64_t wflign_max_len_minor = 128000; // windowLength * 128, parse_args.hpp:594
  std::vector<std::string> refSequences;
  std::vector<std::string> querySequences;
  std::string mashmapPafFile;
  std::string pafOutputFile;
  bool emit_md_tag = false;
  bool sam_format = false;
  bool no_seq_in_sam = false;
  bool disable_chain_patching = false;
  uint64_t target_padding = 1000;         // min(w, 5000), parse_args.hpp:608
  uint64_t query_padding = 1000;          // parse_args.hpp:620
  // batching (not in the reference): a batch is bounded by bases and by records.  1536 records of 50 kb fill the device
  // level by level (3 k workgroups per launch) and leave a mid-sized mapping file -- one rank's share of a pangenome,
  // 6 k records -- in enough batches for the workers' host stages to overlap the device (measured: 2 batches of 2.9 k
  // records 0.63 s, 6 batches 0.51 s; a 1.2 k-record file is best left whole)
  uint64_t batch_bases = 160ull << 20;
  size_t batch_records = 1536;
  // (not in the reference) whole sequences stay on the device and the problems name their windows by reference
  // (wfmh_align_params_t::resident_sequences); off by default
  bool resident_sequences = false;
};

// MappingBoundaryRow (align_types.hpp:17)
struct MappingBoundaryRow {
  std::string qId, refId;
  int64_t qStartPos = 0, qEndPos = 0, rStartPos = 0, rEndPos = 0;
  int16_t strand = FWD;
  float mashmap_estimated_identity = 0;
  int32_t chain_id = -1, chain_length = 1, chain_pos = 1;
};

struct Summary {
  uint64_t records = 0;            // "total aligned records"
  uint64_t aligned_bp = 0;         // "total aligned bp" = sum of query spans (computeAlignments.hpp:481,528)
  uint64_t written = 0;            // PAF lines emitted
  uint64_t skipped = 0;            // invalid mapping rows
  uint64_t cells = 0;
  uint64_t cells_tile = 0, tile_launches = 0;  // the tile kernels' share of it (unique cells), their launches and summed launch durations
  double ms_tile = 0;
  double ms_gpu = 0, ms_total = 0;
  double ms_rows = 0, ms_fetch = 0, ms_wflign = 0, ms_text = 0;  // host stages, summed over the batches
  double ms_tags = 0;  // WFM_RECORD_TAGS (a diagnostic): writing the records' tags, lock wait included, summed over the batches
  uint64_t batches = 0;
  uint64_t records_resident = 0;   // resident_sequences: records whose two sides both came from the device's store
  uint64_t lazy_fetches = 0;       // ... and of those, the ones whose bases the host fetched after all (for the swizzle)
  std::vector<std::pair<double, double>> busy;  // a worker's device-busy intervals (merged per device at the end of compute())
};

// makeUpperCaseAndValidDNA (commonFunc.hpp:132-142) in place, and reverseComplement (commonFunc.hpp:74-83) on validated DNA: the
// form every window the driver fetches is brought into (the PAF verifier fetches through them as well)
void upper_valid_dna(std::string& s);
std::string revcomp(const std::string& s);

class Aligner {
 public:
  Aligner(const Parameters& p, wfm_handle_t* gpu);
  // one handle per GPU of the node: batches of records go to whichever device is free
  Aligner(const Parameters& p, const std::vector<wfm_handle_t*>& gpus);
  ~Aligner();
  // throws std::runtime_error on malformed rows (computeAlignments.hpp:199-201,292-297)
  static void parseMashmapRow(const std::string& line, MappingBoundaryRow& row, uint64_t target_padding,
                              uint64_t query_padding = 0);
  Summary compute();  // streams param.mashmapPafFile through the GPUs into param.pafOutputFile
  // Aligns mapping lines already in memory on the first GPU; returns the PAF text.
  std::string align_lines(const std::vector<std::string>& lines, Summary& sum);

 private:
  // ---- one batch of mapping rows on one handle (aligner.cpp: align_batch and its stages) ----
  struct Fetched;     // a row, its windows and where its sides are
  struct BatchTimes;  // the stages' times, into the Summary at the end
  // (passes: which of the driver's passes are on, this handle's objects for them, the batch's number and the run's tables -- the default:
  // none.  Returns the batch's text and what the passes leave per batch)
  wflign::BatchTexts align_batch(wfm_handle_t* gpu, std::vector<std::string>& lines, int threads, Summary& sum, uint64_t first_row = 0,
                                 const wflign::BatchPasses& passes = wflign::BatchPasses());
  std::vector<Fetched> parse_rows(std::vector<std::string>& lines, uint64_t first_row, Summary& sum) const;
  void fetch_windows(Fetched& f) const;
  std::vector<Fetched> fetch_eager(std::vector<Fetched>& rows, int threads, Summary& sum) const;
  static void point_at(wflign::BiwfaRecord& r, const Fetched& f);
  static std::vector<wflign::BiwfaRecord> make_records(const std::vector<Fetched>& fetched);
  static void account(Summary& sum, const wflign::BiwfaStats& st, const wflign::ResidentSeqs& resident, const std::vector<Fetched>& fetched,
                      const std::vector<wflign::BiwfaRecord>& recs);
  static std::string gather_text(Summary& sum, const std::vector<Fetched>& fetched, const std::vector<wflign::BiwfaRecord>& recs);
  // ---- the run over the mapping file (aligner.cpp: compute and its stages) ----
  struct Run;  // what the workers of one compute() share
  struct RunPlan { size_t per_gpu = 1, nworkers = 1; uint64_t batch_bytes = ~0ull; };
  RunPlan plan_run(std::ifstream& in) const;
  void make_passes(Run& run) const;  // the across-record outputs whose switches are on (--variants ... --transitive), in their order
  void run_worker(Run& run, size_t wk);
  void sum_up(Summary& sum, const std::vector<Summary>& part, std::chrono::steady_clock::time_point t0) const;
  const Parameters& param;
  std::vector<wfm_handle_t*> gpus;
  std::shared_ptr<wfmash_host::FastaStore> ref, query_own;
  const wfmash_host::FastaStore* query = nullptr;
  // resident_sequences: one store per device, shared by all of that device's workers.  A sequence is added on first use; one that
  // does not fit what is left of the budget (WFM_SEQSTORE_GB, read when the store is made) never is -- there is no eviction -- and
  // its windows stay host-pointer sides.
  struct DeviceStore {
    wfm_seqstore_t* store = nullptr;
    std::mutex mu;
    int64_t budget = 0, used = 0;
    std::map<std::pair<const wfmash_host::FastaStore*, int>, int32_t> ids;  // -1: did not fit
  };
  std::mutex stores_mu;
  std::map<int, std::unique_ptr<DeviceStore>> stores;  // by device
  DeviceStore* device_store(wfm_handle_t* h);
  void assign_resident_ids(wfm_handle_t* gpu, DeviceStore& ds, std::vector<Fetched>& rows);
  int32_t resident_id(wfm_handle_t* h, DeviceStore& ds, const wfmash_host::FastaStore* fa, int idx);
};

}  // namespace align
