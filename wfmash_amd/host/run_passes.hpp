// run_passes.hpp -- the across-record outputs (--coverage, --pav, --lift, --chain, --chain-net, --transitive, and the align-only --variants,
// --genotypes, --maf) above the C ABI, once for their two callers: the align driver (aligner.cpp, wflign_hip.cpp), whose batches of
// written records are one source of packed runs, and the --*-paf modes (verify_paf.cpp), whose lines of an existing aligned PAF are the
// other (packed_runs.hpp).  A STAGE takes a batch of packed runs to the device, one call under the handle's lock, and makes what text
// the batch has; a PASS owns what lives across the batches: the tables read before the first, a device object per handle, the output
// file, and what is done once at the end.  Neither counts into the process-wide switches nor warns: a stage returns its outcome and a
// pass its numbers, and the caller reports them its own way.
#pragma once

#include <chrono>
#include <cstdint>
#include <memory>
#include <mutex>
#include <ostream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "fasta.hpp"
#include "map_queue.hpp"
#include "packed_runs.hpp"
#include "parallel.hpp"
#include "wflign_hip.hpp"

namespace wflign {

using Clock = std::chrono::steady_clock;
inline double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// fn(i) for i in [0, n) on up to `threads` threads; records are independent of each other (the reference runs one
// Taskflow task per record, computeAlignments.hpp:391-435)
template <typename F>
void for_each_record(size_t n, int threads, F&& fn) {
  const int nt = (int)std::min<size_t>((size_t)std::max(1, threads), (n + 7) / 8);  // no thread for fewer than 8 records
  wfmash_host::parallel_for(n, nt, fn);  // (the process's pool: a pass used to start and join its own threads, 2 - 4 ms each -- parallel.hpp)
}

// ---- stages ----
// What a stage did with a batch.  rc < 0: its device call failed, and `error` is the handle's message, copied while the handle was still
// the caller's; nothing else is set then.  counts: what the switch's counts 0, 1, 2 get -- --coverage, --pav, --chain-net, --transitive
// {records added, 0, 0}; --lift {records lifted, lines, lines without an = or X}; --chain {chains, blocks, records refused}.  refused:
// the records the device flagged (pk.unknown never went to it).  debug: the stage's WFM_DEBUG line, made only where that is set.
struct StageOutcome {
  int rc = 0;
  std::string error;
  uint64_t counts[3] = {0, 0, 0};
  uint64_t refused = 0;
  std::string debug;
};

// the frame of a stage's device call: under the handle's lock (t1: when it was had), the message kept.  Without problems nothing is called.
template <class Call>
int device_call(wfm_handle_t* h, size_t n, Clock::time_point& t1, std::string& error, Call call) {
  if (!n) return WFM_OK;
  std::lock_guard<std::mutex> lk(handle_lock(h));
  t1 = Clock::now();
  const int rc = call();
  if (rc < 0) error = wfm_last_error(h);
  return rc;
}

// (handle, host threads of the text step, the passes that are on with this handle's objects and the run's tables, the batch).  lift_records
// and chain_records fill pk.lift / pk.chain, net_records pk.net_heads.
using Stage = StageOutcome (*)(wfm_handle_t*, int, const BatchPasses&, PackedRuns&);
StageOutcome coverage_records(wfm_handle_t* h, int threads, const BatchPasses& bp, PackedRuns& pk);
StageOutcome pav_records(wfm_handle_t* h, int threads, const BatchPasses& bp, PackedRuns& pk);
StageOutcome lift_records(wfm_handle_t* h, int threads, const BatchPasses& bp, PackedRuns& pk);
StageOutcome chain_records(wfm_handle_t* h, int threads, const BatchPasses& bp, PackedRuns& pk);
StageOutcome net_records(wfm_handle_t* h, int threads, const BatchPasses& bp, PackedRuns& pk);
StageOutcome trans_records(wfm_handle_t* h, int threads, const BatchPasses& bp, PackedRuns& pk);
// a pass's stage (null: --variants, --genotypes and --maf work on the align batch's windows)
Stage stage_of(SwitchId id);
// what lift_records, chain_records and net_records left in the batch, to where a pass takes it from
void take_texts(PackedRuns& pk, BatchTexts& t);

// ---- passes ----
// the ordered writer's sink: the output stream, flushed once per put.  number (--chain): the chains of a batch come without their ids; the
// writer numbers them 1, 2, 3 ... as it writes them, in file order
struct TextSink {
  std::ostream* out;
  bool number = false;
  uint64_t next = 1;
  std::string numbered;
  void write(std::string& text) {
    if (!number) { *out << text; return; }
    numbered.clear();
    chain::number(text, &next, numbered);
    *out << numbered;
  }
  void flush() { out->flush(); }
};
using TextWriter = skch::OrderedWriter<std::string, TextSink>;

// the run's tables from its two files (query: the target's, where there is no query file), before the first pass is made
void fill_tables(RunTables& tb, const wfmash_host::FastaStore& target, const wfmash_host::FastaStore& query);

// What a pass is made of: the caller's prefix of every message ("[wfmash::align] --pav:", "[wfmash::pav]"), its word for what it feeds the
// pass with, the stream the file goes to -- the caller's, open before the pass writes: at once for --variants and --maf, from the first
// take on for the others -- the BED's text where the switch reads one, and the switch's integer (SwitchSetting::option).
struct PassInput {
  std::string prefix;
  const char* unit = "records";
  std::ostream* out = nullptr;
  bool has_bed = false;
  std::string bed;
  uint64_t option = 0;
};

// One pass of a run: a switch that is on, and the file it writes -- per batch through an ordered writer keyed by the batches' numbers
// (--variants, --lift, --chain, --maf), or once the batches are done (finish: the others).  A pass with a device object keeps one per
// handle the run has used so far, made at the handle's first batch; finish merges them into the first handle's.  A pass's constructor
// reads what it needs before anything is added and adds to the run's tables what its stage looks up per record.
struct Pass {
  Pass(SwitchId i, bool with_object, RunTables& tb, const PassInput& in) : id(i), prefix(in.prefix), per_handle(with_object), tables(tb), out(*in.out) {}
  virtual ~Pass() {}
  const SwitchId id;
  const std::string prefix;
  const bool per_handle;
  RunTables& tables;
  std::ostream& out;
  std::unique_ptr<TextWriter> writer;
  std::mutex mu;  // of objects (and of what a pass gathers from the batches)
  std::vector<std::pair<wfm_handle_t*, void*>> objects;

  void* object_of(wfm_handle_t* h);
  void free_objects();
  // the batch's share: its text to the ordered writer
  virtual void take(uint64_t seq, BatchTexts& t) { if (writer) writer->put(seq, std::move(t.text[id])); }
  // What the end of the run adds to the switch's counts 1, 2 and 3 (switch_finished), and one number more for a summary: --coverage {bases
  // covered, sum of depth, intervals written; max depth}, --lift {0, 0, BED lines skipped; intervals}, --pav {rows, union intervals, BED
  // lines skipped}, --genotypes {sites, variants merged away, 0}, --chain-net {chains, pieces, records that won nothing}, --transitive
  // {lines written, rounds, BED lines skipped; seeds}.
  struct Finished { uint64_t c[3] = {0, 0, 0}; uint64_t extra = 0; std::string debug; };
  virtual Finished finish() { return Finished(); }
  [[noreturn]] void fail(const std::string& what) const { throw std::runtime_error(prefix + " " + what); }

 protected:
  virtual int create(wfm_handle_t*, void**) { return WFM_OK; }
  virtual void destroy(void*) {}
  // the lists of an object (kept by the pass between the two), into another, freed
  virtual int export_lists(wfm_handle_t*, void*) { return WFM_OK; }
  virtual int import_lists(wfm_handle_t*, void*) { return WFM_OK; }
  virtual void free_lists() {}

  wfm_handle_t* h0() const { return objects.front().first; }
  template <class T>
  T* first() const { return static_cast<T*>(objects.front().second); }
  [[noreturn]] void fail(wfm_handle_t* h, const char* what) const { fail(std::string(what) + ": " + wfm_last_error(h)); }
  void merge();
  void writes_per_batch(bool number = false) { writer.reset(new TextWriter(TextSink{&out, number})); }
};
// the pass of one of SwitchId's first N_PASSES
std::unique_ptr<Pass> make_pass(SwitchId id, RunTables& tb, const PassInput& in);

// ---- an aligned PAF through one pass: what a --*-paf mode does between its argument checks and its summary ----
struct PafPassCall {
  SwitchId id;
  const char* tag;  // "coverage": the [wfmash::coverage] of the texts
  const char *target_fasta, *query_fasta_or_null, *aligned_paf, *bed_path_or_null, *out_path;
  uint64_t option;
};
struct PafPassResult {
  uint64_t counts[3] = {0, 0, 0};          // the stage's, over all batches
  uint64_t skipped[5] = {0, 0, 0, 0, 0};   // lines, by coverage::LINE_*; what the device refused is under LINE_MALFORMED (a span that leaves the target: classify_line lets none through)
  uint64_t no_query = 0;                   // lines left out for their query (--pav-paf, --transitive-paf)
  uint64_t groups = 0;                     // --pav-paf: the table's columns
  Pass::Finished end;
  uint64_t all_skipped() const { return skipped[1] + skipped[2] + skipped[3] + skipped[4]; }
};
// Opens the files (throws "[wfmash::TAG] cannot open PATH"), makes the tables and the pass, reads the PAF in batches of 65536 lines or
// 16 Mi runs (WFM_PAF_BATCH_RECORDS, read per call: another number of lines), runs the pass's stage on every batch with ONE host thread
// and finishes the pass.  Throws what the pass throws.
PafPassResult run_paf_pass(wfm_handle_t* h, const PafPassCall& call);

}  // namespace wflign
