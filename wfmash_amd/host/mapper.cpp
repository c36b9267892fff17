#include "mapper.hpp"
#include "parallel.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <deque>
#include <condition_variable>
#include <fstream>
#include <iostream>
#include <map>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <thread>
#include <unordered_map>

#include "../csrc/map_device.h"
#include "../csrc/wfa_handle.h"
#include "fasta.hpp"
#include "index_file.hpp"
#include "map_filter.hpp"
#include "map_plan.hpp"
#include "map_queue.hpp"
#include "map_stats.hpp"

namespace skch {

namespace {

constexpr float kConfidenceInterval = 0.95f;  // fixed::confidence_interval (map_parameters.hpp:125)
// (what a batch's mappings come back in: sized for the most a batch can yield -- 16 per fragment and more --, filled by the copy from the device up to
// what it did yield.  A std::vector writes all of it first: 144 MB of zeros and page faults per chromosome-sized query, on the device thread, before the
// mapping it waits for begins.  Raw memory, untouched beyond what the copy writes)
template <class T>
struct RawVec {
  T* p = nullptr; size_t n = 0, cap = 0;
  RawVec() = default;
  RawVec(const RawVec&) = delete;
  RawVec& operator=(const RawVec&) = delete;
  ~RawVec() { free(p); }
  void resize(size_t k) {
    if (k > cap) { free(p); p = (T*)malloc(k * sizeof(T)); if (!p) { cap = n = 0; throw std::bad_alloc(); } cap = k; }  // (never grown with content to keep: sized, then filled)
    n = k;
  }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
  T* data() { return p; }
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
};

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// all FASTA files of a run, loaded once; name -> sequence
class SequenceSource {
 public:
  void add(const std::string& path) {
    if (stores_.count(path)) return;
    stores_.emplace(path, wfmash_host::open_shared(path));
    order_.push_back(path);
  }
  // the first file holding `name`, restricted to `files`
  bool find(const std::vector<std::string>& files, const std::string& name, wfmash_host::SeqView* seq) const {
    for (const auto& f : files) {
      const auto& st = *stores_.at(f);
      const int i = st.find(name);
      if (i >= 0) { *seq = st.sequence(i); return true; }
    }
    return false;
  }
  // indexed files: read the sequences find() will be asked for, side by side
  void preload(const std::vector<std::string>& files, const std::vector<std::string>& names, int threads) const {
    std::unordered_map<std::string, bool> seen;
    for (const auto& f : files) {
      const auto& st = *stores_.at(f);
      std::vector<int> which;
      for (const auto& n : names) {
        const int i = st.find(n);
        if (i >= 0 && !seen[n]) { which.push_back(i); seen[n] = true; }
      }
      if (!which.empty()) st.preload(which, threads);
    }
  }

 private:
  std::unordered_map<std::string, std::shared_ptr<wfmash_host::FastaStore>> stores_;
  std::vector<std::string> order_;
};

struct DeviceTables {
  std::vector<int32_t> ref_group, min_hits, cutoffs;
  std::vector<uint8_t> keep;
  std::vector<uint16_t> ident;
  std::vector<double> cutoff_j;
  wfm_map_params_t prm;
};

// Sketch::build of one subset over several handles: the sequences are dealt over hs, one host thread per handle that got
// any sketches its share (wfm_sketch_part), the index stage runs on hs[0] on the union in the order given (wfm_index_build_parts).
// Errors are reported on hs[0]; the parts are freed on every way out.
int build_index_sharded(const std::vector<wfm_handle_t*>& hs, const std::vector<const char*>& sp, const std::vector<int64_t>& sl,
                        const std::vector<int32_t>& si, int k, int w, int s, int threads, double max_kmer_freq, wfm_index_t** ix,
                        int64_t* n_windows, int* parts_used, double* ms_sketch, double* ms_merge) {
  const size_t nh = hs.size(), n = sp.size();
  const std::vector<int> part_of = deal_longest_first(sl.data(), (int64_t)n, (int)nh);
  struct Share {
    std::vector<const char*> sp;
    std::vector<int64_t> sl;
    std::vector<int32_t> si;
    wfm_minmer_part_t* part = nullptr;
    int rc = WFM_OK;
    double ms = 0;
  };
  std::vector<Share> shares(nh);
  struct FreeParts {
    std::vector<Share>& v;
    ~FreeParts() { for (Share& sh : v) { wfm_minmer_part_free(sh.part); sh.part = nullptr; } }
  } free_parts{shares};
  std::vector<wfm_part_seq_t> order(n);
  for (size_t i = 0; i < n; ++i) {
    Share& sh = shares[(size_t)part_of[i]];
    order[i].part = part_of[i];  // (the handle's index for now: the parts are numbered below)
    order[i].seq = (int32_t)sh.sp.size();
    sh.sp.push_back(sp[i]); sh.sl.push_back(sl[i]); sh.si.push_back(si[i]);
  }
  const int threads_each = std::max(1, threads / (int)nh);
  {
    std::vector<std::thread> sketchers;
    for (size_t g = 0; g < nh; ++g) {
      if (shares[g].sp.empty()) continue;
      sketchers.emplace_back([&, g] {
        Share& sh = shares[g];
        const double t0 = now_ms();
        sh.rc = wfm_sketch_part(hs[g], sh.sp.data(), sh.sl.data(), sh.si.data(), (int64_t)sh.sp.size(), k, w, s, threads_each, &sh.part);
        sh.ms = now_ms() - t0;
      });
    }
    for (auto& t : sketchers) t.join();
  }
  std::vector<const wfm_minmer_part_t*> parts;
  std::vector<int> number(nh, -1);
  for (size_t g = 0; g < nh; ++g) {
    if (shares[g].sp.empty()) continue;
    if (shares[g].rc != WFM_OK) {
      wfm_set_error(hs[0], "index sketching failed on handle " + std::to_string(g) + ": " + wfm_last_error(hs[g]));
      return shares[g].rc;
    }
    number[g] = (int)parts.size();
    parts.push_back(shares[g].part);
    *ms_sketch = std::max(*ms_sketch, shares[g].ms);
  }
  for (auto& o : order) o.part = number[(size_t)o.part];
  *parts_used = (int)parts.size();
  return map_index_build_parts(hs[0], parts.data(), (int)parts.size(), order.data(), (int64_t)order.size(), max_kmer_freq, ix, n_windows, ms_merge);
}

// the switches of the environment, read once per mapQuery call
struct MapKnobs {
  int index_sharded = -1;      // WFM_INDEX_SHARDED: -1 unset; 0: handles[0] builds alone as before; 1: the two-step path with a single handle as well, which times its steps
  bool filter_overlap = true;  // WFM_FILTER_OVERLAP=0: a batch's post-processing after its mapping, on the device thread, as before
  size_t filter_workers = 2;   // WFM_FILTER_WORKERS: filter threads per device thread, 1 .. 4
  bool device_order = true;    // WFM_FILTER_DEVICE_ORDER=0: the chaining order is sorted on the host
  bool filter_times = false;   // WFM_FILTER_TIMES: [filter] lines on stderr
  static MapKnobs read() {
    MapKnobs k;
    if (const char* e = getenv("WFM_INDEX_SHARDED")) k.index_sharded = atoi(e);
    if (const char* e = getenv("WFM_FILTER_OVERLAP")) k.filter_overlap = atoi(e) != 0;
    if (const char* e = getenv("WFM_FILTER_WORKERS")) k.filter_workers = (size_t)std::max(1, std::min(4, atoi(e)));
    if (const char* e = getenv("WFM_FILTER_DEVICE_ORDER")) k.device_order = atoi(e) != 0;
    k.filter_times = getenv("WFM_FILTER_TIMES") != nullptr;
    return k;
  }
};

// a subset's index on every handle; freed on every way out
struct IndexSet {
  const std::vector<wfm_handle_t*>& hs;
  std::vector<wfm_index_t*> ix;
  explicit IndexSet(const std::vector<wfm_handle_t*>& handles) : hs(handles), ix(handles.size(), nullptr) {}
  IndexSet(const IndexSet&) = delete;
  IndexSet& operator=(const IndexSet&) = delete;
  ~IndexSet() { release(); }
  void release() {
    for (size_t g = 0; g < hs.size(); ++g) if (ix[g]) { wfm_index_free(hs[g], ix[g]); ix[g] = nullptr; }
  }
};

struct QueryOut { MappingResultsVector_t keep; std::string text; };
struct BatchOut { std::vector<seqno_t> ids; std::vector<QueryOut> q; };

// everything one mapQuery call works on
struct MapRun {
  const Parameters& P;
  SequenceIdManager& ids;  // (-I imports the file's ids into it)
  const std::vector<wfm_handle_t*>& hs;
  wfm_handle_t* h;  // hs[0]: builds the index, carries the error message
  MapKnobs knobs;
  std::vector<std::string> queryNames, targetNames;
  std::vector<std::vector<std::string>> subsets;
  SequenceSource src;
  std::vector<wfmash_host::SeqView> query_seq;  // per query name; empty: "not found or empty, skipping" (computeMap.hpp:534-537)
  std::vector<int64_t> query_len;
  DeviceTables T;
  std::ofstream file;                 // the PAF, unless it goes to stdout
  std::ostream* out = nullptr;
  // --scaffold-out: one file for the run, every query and every target subset; queries are post-processed on several threads, each
  // query's lines are written at once under the lock (the reference writes from its worker threads as well: the line order is not fixed)
  std::ofstream scaffold_file;
  std::mutex scaffold_mu;
  std::ifstream index_in;             // -I: the sub-indexes are read in file order, one per subset
  std::map<seqno_t, MappingResultsVector_t> combined;  // one-to-one mode: everything is held back
  MapSummary sum;
  // an exception on a worker thread (FASTA I/O, bad_alloc, a filter throw) must come back as a WFM_E_* code like
  // everything else: the first message is kept, every thread is joined (Aligner::compute does the same)
  std::atomic<int> error_rc{WFM_OK};
  std::mutex err_mu;

  MapRun(const Parameters& p, SequenceIdManager& i, const std::vector<wfm_handle_t*>& handles)
      : P(p), ids(i), hs(handles), h(handles.front()), knobs(MapKnobs::read()) {}
  int fail(int rc, const std::string& what) {
    std::lock_guard<std::mutex> lk(err_mu);
    int expected = WFM_OK;
    if (error_rc.compare_exchange_strong(expected, rc)) wfm_set_error(h, what);
    return rc;
  }
  // outside the worker threads: the message, and the code to return
  int error(int rc, const std::string& what) { wfm_set_error(h, what); return rc; }
};

struct GuardText { const char *nomem, *prefix; };
constexpr GuardText kPostProcessing{"out of host memory while post-processing mappings", "post-processing failed: "};
constexpr GuardText kMapDriver{"out of host memory in the map driver", "map driver: "};

template <class F>
void run_guarded(MapRun& R, const GuardText& what, F&& fn) {
  try {
    fn();
  } catch (const std::bad_alloc&) {
    R.fail(WFM_E_NOMEM, what.nomem);
  } catch (const std::exception& e) {
    R.fail(WFM_E_ARG, std::string(what.prefix) + e.what());
  } catch (...) {
    R.fail(WFM_E_ARG, std::string(what.prefix) + "unknown exception");
  }
}

// thresholds and tables the kernels take
void make_tables(MapRun& R, int cached_minimum_hits) {
  const Parameters& P = R.P;
  DeviceTables& T = R.T;
  const int S = P.sketchSize, k = P.kmerSize;
  const int64_t w = P.windowLength;
  T.ref_group = R.ids.refGroupTable();
  T.min_hits.assign((size_t)S + 1, 0);
  for (int q = 1; q <= S; ++q)
    T.min_hits[q] = std::max(P.minimum_hits, Stat::estimateMinimumHitsRelaxed(q, k, P.percentageIdentity, kConfidenceInterval));
  if (P.stage1_topANI_filter) {
    const std::vector<int> c = Stat::sketch_cutoffs(S, k, P.ANIDiff, P.ANIDiffConf);
    T.cutoffs.assign(c.begin(), c.end());
  } else {
    T.cutoffs.assign((size_t)std::min<double>(S, 1000.0) + 1, 1);
  }
  Stat::l2_identity_tables(S, k, P.percentageIdentity, P.keep_low_pct_id, kConfidenceInterval, T.keep, T.ident);
  T.cutoff_j.assign((size_t)S + 1, 0.0);
  for (int q = 1; q <= S; ++q) T.cutoff_j[q] = Stat::l2_cutoff_j(q, k, P.ANIDiff, P.hgNumerator);
  std::memset(&T.prm, 0, sizeof(T.prm));
  T.prm.kmer_size = k;
  T.prm.kmer_complexity_threshold = P.kmerComplexityThreshold;
  wfm_l1_params_t& l1 = T.prm.l1;
  l1.window_length = (int32_t)w; l1.sketch_size = S; l1.min_hits_cached = cached_minimum_hits; l1.cached_segment_length = (int32_t)w;
  l1.skip_self = P.skip_self; l1.skip_prefix = P.skip_prefix; l1.lower_triangular = P.lower_triangular;
  l1.stage1_topANI_filter = P.stage1_topANI_filter; l1.stage2_full_scan = P.stage2_full_scan;
  l1.n_seq = (int32_t)T.ref_group.size(); l1.ref_group = T.ref_group.data(); l1.min_hits_by_qsketch = T.min_hits.data();
  l1.sketch_cutoffs = T.cutoffs.data(); l1.n_cutoffs = (int32_t)T.cutoffs.size();
  wfm_l2_params_t& l2 = T.prm.l2;
  l2.window_length = (int32_t)w; l2.sketch_size = S; l2.stage1_topANI_filter = P.stage1_topANI_filter;
  l2.keep_table = T.keep.data(); l2.ident_table = T.ident.data(); l2.cutoff_j = T.cutoff_j.data();
}

// names, sequences, subsets and the summary's counts of them
int select_and_load(MapRun& R) {
  const Parameters& P = R.P;
  const SequenceIdManager& ids = R.ids;
  R.queryNames = map_plan::select_by_prefix(ids.getQuerySequenceNames(), P.query_prefix);
  R.targetNames = map_plan::select_by_prefix(ids.getTargetSequenceNames(),
                                             P.target_prefix.empty() ? std::vector<std::string>{} : std::vector<std::string>{P.target_prefix});
  for (const auto& f : P.refSequences) R.src.add(f);
  for (const auto& f : P.querySequences) R.src.add(f);
  R.src.preload(P.refSequences, R.targetNames, P.threads);
  R.src.preload(P.querySequences, R.queryNames, P.threads);
  R.query_seq.resize(R.queryNames.size());
  R.query_len.assign(R.queryNames.size(), 0);
  for (size_t i = 0; i < R.queryNames.size(); ++i)
    if (R.src.find(P.querySequences, R.queryNames[i], &R.query_seq[i])) R.query_len[i] = (int64_t)R.query_seq[i].size();

  int64_t index_by_size = P.index_by_size;
  if (!P.indexFilename.empty() && !P.create_index_only) {
    // "Using batch size N from index file" (computeMap.hpp:349-376)
    int64_t bs = 0;
    try { peek_index_file(P.indexFilename, &bs, nullptr); } catch (const std::exception& e) { return R.error(WFM_E_ARG, e.what()); }
    if (bs > 0) index_by_size = bs;
  }
  std::vector<int64_t> target_len;
  for (const auto& n : R.targetNames) target_len.push_back(ids.getSequenceLength(ids.getSequenceId(n)));
  R.subsets = map_plan::target_subsets(R.targetNames, target_len, index_by_size > 0 ? index_by_size : map_plan::kDefaultSubsetBases);
  R.sum.targets = R.targetNames.size();
  R.sum.queries = R.queryNames.size();
  R.sum.subsets = R.subsets.size();
  for (int64_t l : target_len) R.sum.target_bp += l;
  for (const auto& n : R.queryNames) R.sum.query_bp += ids.getSequenceLength(ids.getSequenceId(n));
  return WFM_OK;
}

int open_outputs(MapRun& R) {
  const Parameters& P = R.P;
  const bool to_stdout = P.outFileName == "/dev/stdout" || P.outFileName == "-";
  if (!to_stdout) {
    R.file.open(P.outFileName);
    if (!R.file.is_open()) return R.error(WFM_E_ARG, "cannot open output file " + P.outFileName);
  }
  R.out = to_stdout ? static_cast<std::ostream*>(&std::cout) : &R.file;
  if (!P.scaffold_output_file.empty()) {
    R.scaffold_file.open(P.scaffold_output_file);
    if (!R.scaffold_file.is_open()) return R.error(WFM_E_ARG, "cannot open scaffold output file " + P.scaffold_output_file);
  }
  if (!P.indexFilename.empty() && !P.create_index_only) {
    R.index_in.open(P.indexFilename, std::ios::binary);
    if (!R.index_in) return R.error(WFM_E_ARG, "unable to open index file for reading: " + P.indexFilename);
  }
  return WFM_OK;
}

// -I: Sketch::readIndex of the next sub-index of the file, onto the first handle
int load_sub_index(MapRun& R, size_t si, IndexSet& ixs) {
  const Parameters& P = R.P;
  SubIndex sub;
  try { read_sub_index(R.index_in, sub, R.ids); } catch (const std::exception& e) { return R.error(WFM_E_ARG, e.what()); }
  if (sub.windowLength != P.windowLength || sub.sketchSize != P.sketchSize || sub.kmerSize != P.kmerSize)  // readParameters (winSketch.hpp:713-737)
    return R.error(WFM_E_ARG, "parameters of the indexed sketch differ from the current ones: index w=" + std::to_string(sub.windowLength) + " s=" +
                                  std::to_string(sub.sketchSize) + " k=" + std::to_string(sub.kmerSize));
  if (sub.names != R.subsets[si]) std::cerr << "[wfmash::mashmap] Warning: the sequences of index subset " << si + 1 << " differ from the expected targets\n";
  if (!sub.minmers.empty()) {
    const int rc = wfm_index_upload(R.h, sub.uhash.data(), sub.poff.data(), (int64_t)sub.uhash.size(), sub.points.data(), sub.minmers.data(),
                                    (int64_t)sub.minmers.size(), &ixs.ix[0]);
    if (rc != WFM_OK) return rc;
  }
  R.sum.index_windows += sub.minmers.size();
  return WFM_OK;
}

// Sketch::build of one subset, onto the first handle
int build_sub_index(MapRun& R, size_t si, IndexSet& ixs) {
  const Parameters& P = R.P;
  MapSummary& sum = R.sum;
  const int S = P.sketchSize, k = P.kmerSize;
  const int64_t w = P.windowLength;
  std::vector<const char*> sp;
  std::vector<int64_t> sl;
  std::vector<int32_t> si_ids;
  for (const auto& name : R.subsets[si]) {
    wfmash_host::SeqView seq;
    if (!R.src.find(P.refSequences, name, &seq)) return R.error(WFM_E_ARG, "target sequence not found in FASTA: " + name);
    if ((int64_t)seq.size() < w) continue;  // "skipping short sequence" (winSketch.hpp:216-229)
    sp.push_back(seq.data()); sl.push_back((int64_t)seq.size()); si_ids.push_back(R.ids.getSequenceId(name));
  }
  // minmer intervals (GPU hashing + thinning, host winnowing) and the index stage; the intervals never
  // sit in one host array.  --streaming-minhash: one bottom-S MinHash per sequence instead (winSketch.hpp:474-485)
  int64_t n_windows = 0;
  const bool streaming = P.use_streaming_minhash && S > 0;
  int rc;
  if ((R.hs.size() > 1 || R.knobs.index_sharded == 1) && !streaming && !sp.empty() && R.knobs.index_sharded != 0) {
    // every device sketches its share of the subset; the index stage runs on the first device on the union in subset order
    int parts_used = 0;
    double ms_sketch = 0, ms_merge = 0;
    rc = build_index_sharded(R.hs, sp, sl, si_ids, k, (int)w, S, P.threads, P.max_kmer_freq, &ixs.ix[0], &n_windows, &parts_used, &ms_sketch, &ms_merge);
    sum.index_parts = std::max(sum.index_parts, parts_used);
    sum.ms_index_sketch += ms_sketch;
    sum.ms_index_merge += ms_merge;
  } else {
    rc = streaming ? wfm_index_build_streaming(R.h, sp.data(), sl.data(), si_ids.data(), (int64_t)sp.size(), k, (int)w, S, P.max_kmer_freq, &ixs.ix[0], &n_windows)
                   : wfm_index_build_sequences(R.h, sp.data(), sl.data(), si_ids.data(), (int64_t)sp.size(), k, (int)w, S, P.threads,
                                               P.max_kmer_freq, &ixs.ix[0], &n_windows);
    sum.index_parts = std::max(sum.index_parts, 1);
  }
  if (rc != WFM_OK) return rc;
  sum.index_windows += (uint64_t)n_windows;
  return WFM_OK;
}

// -W: write the sub-index, appended after the previous ones (computeMap.hpp:405-415); the device's copy is freed before the file is written
int write_sub_index_file(MapRun& R, size_t si, IndexSet& ixs) {
  const Parameters& P = R.P;
  SubIndex sub;
  sub.batch_idx = si; sub.total_batches = R.subsets.size(); sub.batch_size = P.index_by_size;
  sub.names = R.subsets[si]; sub.windowLength = P.windowLength; sub.sketchSize = P.sketchSize; sub.kmerSize = P.kmerSize;
  if (ixs.ix[0]) {
    wfm_index_info_t inf;
    wfm_index_info(ixs.ix[0], &inf);
    sub.uhash.resize((size_t)inf.n_unique); sub.poff.resize((size_t)inf.n_unique + 1);
    sub.points.resize((size_t)inf.n_points); sub.minmers.resize((size_t)inf.n_kept);
    const int rc = wfm_index_download(R.h, ixs.ix[0], sub.uhash.data(), sub.poff.data(), sub.points.data(), sub.minmers.data());
    ixs.release();
    if (rc != WFM_OK) return rc;
  } else {
    sub.poff.assign(1, 0);
  }
  std::ofstream index_out(P.indexFilename, si ? std::ios::binary | std::ios::app : std::ios::binary);
  if (!index_out) return R.error(WFM_E_ARG, "unable to open index file for writing: " + P.indexFilename);
  try { write_sub_index(index_out, sub, R.ids); } catch (const std::exception& e) { return R.error(WFM_E_ARG, e.what()); }
  return WFM_OK;
}

// the other GPUs of the node receive a copy of the finished index (it is read-only from here on,
// computeMap.hpp:431-484): built once per node, not once per GPU
int replicate_index(MapRun& R, IndexSet& ixs) {
  if (!ixs.ix[0]) return WFM_OK;
  const double t0 = now_ms();
  // every device pulls its copy at the same time (the source's xGMI links to its peers are separate)
  std::vector<int> rcs(R.hs.size(), WFM_OK);
  {
    std::vector<std::thread> pulls;
    for (size_t g = 1; g < R.hs.size(); ++g) pulls.emplace_back([&, g] { rcs[g] = wfm_index_replicate(R.h, ixs.ix[0], R.hs[g], &ixs.ix[g]); });
    for (auto& t : pulls) t.join();
  }
  for (size_t g = 1; g < R.hs.size(); ++g)
    if (rcs[g] != WFM_OK) return R.error(rcs[g], std::string("index replication failed: ") + wfm_last_error(R.hs[g]));
  R.sum.ms_replicate += now_ms() - t0;
  return WFM_OK;
}

// (a batch of one sequence -- a chromosome -- is mapped where the FASTA store holds it; several are laid end to end in `buffer`)
struct Batch {
  std::vector<map_plan::BatchQuery> bq;
  std::string buffer;
  const char* bases = nullptr;
  int64_t n_bases = 0;
  std::vector<int64_t> frag_off;
  std::vector<int32_t> frag_seq;
};

// finished batches reach the output in the order they were formed
struct BatchSink {
  MapRun* R;
  void write(BatchOut& o) {
    for (size_t qn = 0; qn < o.q.size(); ++qn) {
      if (R->P.filterMode == filter::ONETOONE) {
        auto& dst = R->combined[o.ids[qn]];
        dst.insert(dst.end(), o.q[qn].keep.begin(), o.q[qn].keep.end());
      } else {
        *R->out << o.q[qn].text;
        R->sum.written += o.q[qn].keep.size();
      }
    }
  }
  void flush() { R->out->flush(); }
};

// what the devices of one subset share: queries are taken in batches of whole sequences, a GPU takes the next batch when it is free
struct SubsetRun {
  const std::vector<std::string>& subset;
  const IndexSet& ixs;
  int64_t batch_bases;
  int threads_each;
  std::mutex read_mu;
  size_t qi = 0;
  uint64_t next_seq = 0;
  OrderedWriter<BatchOut, BatchSink> writer;
  std::vector<MapSummary> part;
  SubsetRun(MapRun& R, size_t si, const IndexSet& ix)
      : subset(R.subsets[si]), ixs(ix), batch_bases(map_plan::batch_bases_for(R.hs.size(), R.sum.query_bp)),
        threads_each(std::max(1, R.P.threads / (int)R.hs.size())), writer(BatchSink{&R}), part(R.hs.size()) {}
};

// the next batch and its number, or -1 when the queries are used up
int64_t read_batch(MapRun& R, SubsetRun& S, Batch& b) {
  std::lock_guard<std::mutex> lk(S.read_mu);
  b = Batch();
  const map_plan::BatchPlan plan = map_plan::plan_batch(R.query_len.data(), R.query_len.size(), S.qi, S.batch_bases);
  S.qi = plan.next;
  if (!plan.in_place) b.buffer.reserve((size_t)plan.n_bases);
  for (const size_t qi : plan.members) {
    const wfmash_host::SeqView& seq = R.query_seq[qi];
    map_plan::BatchQuery q{qi, R.ids.getSequenceId(R.queryNames[qi]), (offset_t)seq.size(), b.n_bases, (int64_t)b.frag_off.size(), 0};
    const map_plan::FragLayout fl = map_plan::layout_fragments(q.len, R.P.windowLength, q.base, q.first_frag);
    q.nfrag = fl.nfrag;
    b.frag_off.insert(b.frag_off.end(), fl.offsets.begin(), fl.offsets.end());
    b.frag_seq.insert(b.frag_seq.end(), (size_t)q.nfrag, q.id);
    if (!plan.in_place) b.buffer.append(seq.data(), seq.size());
    b.n_bases += (int64_t)seq.size();
    b.bq.push_back(q);
  }
  b.bases = plan.in_place ? R.query_seq[plan.members[0]].data() : b.buffer.data();
  return b.bq.empty() ? -1 : (int64_t)S.next_seq++;
}

// one batch on its way from the device thread to a filter thread
struct Work {
  Batch b;
  RawVec<wfm_mapping_t> maps;
  RawVec<int32_t> mfrag;
  RawVec<uint32_t> perm;  // the batch's mappings in chaining order (wfm_map_fragments_ordered), or perm[0] = ~0u
  int64_t seq = -1;
  MappingResultsVector_t* spare = nullptr;  // the spare vector of the thread that filters it (one filter stage runs at a time per thread)
};

// One device of a subset: maps batch after batch (map_batch) and hands each to its filter threads.
// (round 6, f3's other half: SURVEY 8f-3) a batch's post-processing -- boundary check, chaining, sweep, scaffolds, PAF text: host work of
// 70 ms per chromosome-sized query -- runs on a thread of its own BESIDE the device's mapping of the next batch (the reference runs a
// query's filters inside that query's task, computeMap.hpp:634-688, while other queries' tasks map): one batch may wait, so memory
// stays at two batches' mappings per GPU.  WFM_FILTER_OVERLAP=0: one after the other, as before.
// (two filter threads per device thread since the mapping of a chromosome-sized query became shorter than its post-processing -- 52 against 60 ms:
// the batches' texts are written in the batches' order whichever thread finishes first; WFM_FILTER_WORKERS=1: one, as before)
class DeviceWorker {
 public:
  DeviceWorker(MapRun& run, SubsetRun& subset, size_t g) : R(run), S(subset), hg(run.hs[g]), ix(subset.ixs.ix[g]), ps(subset.part[g]), queue_(run.error_rc) {}
  void run();

 private:
  // a batch in post-processing: what its queries' tasks share
  struct FilterJob {
    Work& W;
    double tb;                      // when the stage began
    std::vector<size_t> first_map;  // split_by_query
    const uint32_t* perm;           // the device's order for the whole batch, or null
    std::vector<QueryOut>& qout;
    int nt_filter;                  // threads that share the batch's queries out
  };
  bool map_batch(Work& W);
  void filter_batch(Work& W);
  void filter_query(const FilterJob& J, size_t qn);
  void filter_loop();

  MapRun& R;
  SubsetRun& S;
  wfm_handle_t* const hg;
  wfm_index_t* const ix;
  MapSummary& ps;
  std::mutex ps_mu;                      // ms_filter is summed by the filter threads
  MappingResultsVector_t spare_results;  // (see filter_query: a chromosome-sized query's vector serves the next one; the filter threads have one each)
  // (what a chromosome-sized query's vector will about hold, told by the device thread before its mapping call: a filter thread that has no
  // vector from a query before it makes one while the device maps -- resize() writes every element and faults every page in, 9 ms that were
  // the first thing the post-processing did)
  std::atomic<size_t> spare_hint{0};
  StageQueue<Work> queue_;  // last: its threads are joined before anything above goes
};

void DeviceWorker::run() {
  for (;;) {
    std::unique_ptr<Work> wk(new Work());
    if (R.error_rc.load() != WFM_OK) break;
    wk->seq = read_batch(R, S, wk->b);
    if (wk->seq < 0) break;
    wk->spare = &spare_results;
    if (!map_batch(*wk)) return;
    if (!R.knobs.filter_overlap) { filter_batch(*wk); continue; }
    if (queue_.consumers() < R.knobs.filter_workers) queue_.start_one([this] { filter_loop(); });  // (one more per batch until there are filter_workers: a call of one batch starts one)
    queue_.push(std::move(wk));
  }
}

// wfm_map_fragments[_ordered] of one batch, again with more room if the room was too small; false: failed, the error is set
bool DeviceWorker::map_batch(Work& W) {
  const Batch& b = W.b;
  const double tb = now_ms();
  std::vector<int32_t> frag_first;  // per fragment: the first fragment of its query
  if (ix && !b.frag_off.empty()) {
    if (R.knobs.device_order && R.P.split) {
      frag_first.resize(b.frag_off.size());
      for (const auto& q : b.bq)
        for (int64_t f = q.first_frag; f < q.first_frag + q.nfrag; ++f) frag_first[(size_t)f] = (int32_t)q.first_frag;
    }
    int64_t cap = map_plan::mapping_cap((int64_t)b.frag_off.size(), (int64_t)S.subset.size());
    if (R.knobs.filter_overlap && b.bq.size() == 1 && b.frag_off.size() >= map_plan::kEarlyFilterFrags) {
      spare_hint.store(map_plan::spare_hint(b.frag_off.size(), (int64_t)S.subset.size()));
      if (queue_.consumers() == 0) queue_.start_one([this] { filter_loop(); });
    }
    for (;;) {
      W.maps.resize((size_t)cap); W.mfrag.resize((size_t)cap);
      if (!frag_first.empty()) W.perm.resize((size_t)cap);
      const int64_t n = frag_first.empty()
                            ? wfm_map_fragments(hg, ix, b.bases, b.n_bases, b.frag_off.data(), b.frag_seq.data(), (int64_t)b.frag_off.size(), &R.T.prm,
                                                W.maps.data(), W.mfrag.data(), cap)
                            : wfm_map_fragments_ordered(hg, ix, b.bases, b.n_bases, b.frag_off.data(), b.frag_seq.data(), (int64_t)b.frag_off.size(),
                                                        &R.T.prm, W.maps.data(), W.mfrag.data(), cap, frag_first.data(), W.perm.data());
      if (n < 0) { R.fail((int)n, wfm_last_error(hg)); return false; }
      if (n <= cap) { W.maps.resize((size_t)n); W.mfrag.resize((size_t)n); if (!W.perm.empty()) W.perm.resize((size_t)n); break; }  // (shrinking: the content stays)
      cap = n;
    }
  }
  ps.fragments += b.frag_off.size();
  ps.l2_mappings += W.maps.size();
  ps.ms_map += now_ms() - tb;
  return true;
}

// a filter thread: batches from the queue until it is closed; after an error they are only taken out
void DeviceWorker::filter_loop() {
  MappingResultsVector_t spare_own;
  run_guarded(R, kPostProcessing, [&] {
    for (;;) {
      const size_t hint = spare_hint.load();
      if (hint && spare_own.capacity() < hint) spare_own.resize(hint);
      std::unique_ptr<Work> wk = queue_.pop();
      if (!wk) return;
      wk->spare = &spare_own;
      if (R.error_rc.load() == WFM_OK) filter_batch(*wk);
    }
  });
}

// per query: boundary check, filters, output (processFragment :124-128; query task :634-688).  Queries are independent here (the
// reference runs one Taskflow task per query); results are written in query order afterwards
void DeviceWorker::filter_batch(Work& W) {
  const double tb = now_ms();
  const std::vector<map_plan::BatchQuery>& bq = W.b.bq;
  BatchOut bo;
  bo.q.resize(bq.size());
  for (const auto& q : bq) bo.ids.push_back(q.id);
  const bool have_perm = !W.perm.empty() && W.perm.size() == W.maps.size();
  const FilterJob J{W, tb, map_plan::split_by_query(W.mfrag.data(), W.maps.size(), bq), have_perm ? W.perm.data() : nullptr, bo.q,
                    (int)std::min<size_t>((size_t)S.threads_each, bq.size())};
  std::atomic<size_t> next{0};
  // (every thread shares the queries out by the counter and sets its own filter threads)
  wfmash_host::parallel_for((size_t)J.nt_filter, J.nt_filter, [&](size_t) {
    run_guarded(R, kPostProcessing, [&] {
      set_filter_threads(std::max(1, S.threads_each / std::max(1, J.nt_filter)));  // few queries: each may use the idle threads
      for (size_t qn; R.error_rc.load() == WFM_OK && (qn = next.fetch_add(1)) < bq.size();) filter_query(J, qn);
    });
  });
  if (R.error_rc.load() != WFM_OK) return;
  const double tw0 = now_ms();
  S.writer.put((uint64_t)W.seq, std::move(bo));
  { std::lock_guard<std::mutex> lk(ps_mu); ps.ms_filter += now_ms() - tb; }
  if (R.knobs.filter_times && W.maps.size() >= 100000)
    fprintf(stderr, "[filter] stage of %zu mappings: %.1f ms in all, writing %.1f\n", W.maps.size(), now_ms() - tb, now_ms() - tw0);
}

void DeviceWorker::filter_query(const FilterJob& J, size_t qn) {
  const Parameters& P = R.P;
  Work& W = J.W;
  const map_plan::BatchQuery& q = W.b.bq[qn];
  const std::string& name = R.queryNames[q.qi];
  const double tq0 = now_ms();
  MappingResultsVector_t results;
  const size_t m0 = J.first_map[qn], nq = J.first_map[qn + 1] - J.first_map[qn];
  // (a chromosome-sized query is a batch of its own: its 48 MB vector is the one the query before it left behind -- resize() of a fresh
  // vector writes every element on this thread and faults every page in, 9 of the 13 ms this step took)
  const bool reuse = W.b.bq.size() == 1 && nq >= map_plan::kSpareMappings;
  if (reuse) results.swap(*W.spare);
  std::vector<uint32_t> orig;  // (device order) position of every mapping in fragment order, within the query
  map_plan::query_results(W.maps.data(), W.mfrag.data(), J.perm, m0, nq, q.first_frag, P.windowLength, results, orig,
                          std::min(32, S.threads_each / std::max(1, J.nt_filter)));
  const double tq1 = now_ms();
  MappingOutput::mappingBoundarySanityCheck(q.len, results, R.ids);
  const double tq2 = now_ms();
  FilteredMappingsResult fr = filterSubsetMappings(results, P, R.ids, q.len, orig.empty() ? nullptr : orig.data());
  const double tq3 = now_ms();
  if (!fr.scaffoldChains.empty()) {
    const std::string st = MappingOutput::scaffoldText(fr.scaffoldChains, name, q.len, R.ids);
    std::lock_guard<std::mutex> lk(R.scaffold_mu);
    R.scaffold_file << st;
  }
  const bool merged = P.mergeMappings && P.split;
  MappingResultsVector_t& keep = merged ? fr.mergedMappings : fr.nonMergedMappings;
  const ChainInfoVector_t& chains = merged ? fr.mergedChainInfo : fr.nonMergedChainInfo;
  if (P.filterMode != filter::ONETOONE) {
    std::ostringstream os;
    MappingOutput::reportReadMappings(keep, chains, name, os, R.ids, P, q.len);
    J.qout[qn].text = os.str();
  }
  J.qout[qn].keep = std::move(keep);
  if (reuse && merged) W.spare->swap(fr.nonMergedMappings);  // (the filters' input, handed back: nobody reads it after this)
  if (R.knobs.filter_times && nq >= 100000)
    fprintf(stderr, "[filter] query of %zu mappings: vector %.1f, boundary check %.1f, filterSubsetMappings %.1f, text %.1f ms (stage began %.1f ms before)\n", nq, tq1 - tq0, tq2 - tq1,
            tq3 - tq2, now_ms() - tq3, tq0 - J.tb);
}

// every query against one subset's index: one DeviceWorker per handle, side by side
int map_subset(MapRun& R, size_t si, const IndexSet& ixs) {
  SubsetRun S(R, si, ixs);
  auto worker = [&](size_t g) { run_guarded(R, kMapDriver, [&] { DeviceWorker(R, S, g).run(); }); };
  {
    std::vector<std::thread> pool;
    try {
      for (size_t g = 1; g < R.hs.size(); ++g) pool.emplace_back(worker, g);
    } catch (const std::exception& e) {
      R.fail(WFM_E_NOMEM, std::string("map driver: could not start a device thread: ") + e.what());
    }
    worker(0);
    for (auto& t : pool) t.join();
  }
  if (R.error_rc.load() != WFM_OK) return R.error_rc.load();
  // the GPUs work side by side: the phase times of a subset are those of its slowest device
  double mm = 0, mf = 0;
  for (const MapSummary& ps : S.part) {
    R.sum.fragments += ps.fragments; R.sum.l2_mappings += ps.l2_mappings;
    mm = std::max(mm, ps.ms_map); mf = std::max(mf, ps.ms_filter);
  }
  R.sum.ms_map += mm; R.sum.ms_filter += mf;
  return WFM_OK;
}

// one-to-one mode: the final reference-axis pass (computeMap.hpp:790-866).  The reference walks unordered maps here;
// ids ascending is used instead, which fixes the order of the output records.
void one_to_one_pass(MapRun& R) {
  const double t0 = now_ms();
  std::map<seqno_t, MappingResultsVector_t> byTarget, final_;
  for (auto& [qid, v] : R.combined)
    for (auto& r : v) byTarget[(seqno_t)r.refSeqId].push_back(r);
  for (auto& [tid, v] : byTarget) {
    MappingResultsVector_t kept;
    MappingFilterUtils::filterByGroup(v, kept, R.P.numMappingsForSegment - 1, true, R.ids, R.P);
    for (const auto& r : kept)
      for (auto& [qid, orig] : R.combined)
        for (const auto& o : orig)
          if (o.refSeqId == r.refSeqId && o.refStartPos == r.refStartPos && o.queryStartPos == r.queryStartPos) { final_[qid].push_back(r); break; }
  }
  for (auto& [qid, v] : final_) {
    MappingOutput::reportReadMappings(v, R.ids.getSequenceName(qid), *R.out, R.ids, R.P, R.ids.getSequenceLength(qid));
    R.sum.written += v.size();
  }
  R.out->flush();
  R.sum.ms_filter += now_ms() - t0;
}

}  // namespace

std::vector<int> deal_longest_first(const int64_t* lengths, int64_t n, int n_parts) {
  std::vector<int> part((size_t)std::max<int64_t>(n, 0), 0);
  if (n_parts < 1) return part;
  std::vector<int64_t> by_length(part.size());
  for (size_t i = 0; i < by_length.size(); ++i) by_length[i] = (int64_t)i;
  std::stable_sort(by_length.begin(), by_length.end(), [&](int64_t a, int64_t b) { return lengths[a] > lengths[b]; });  // equal lengths: the lower index first
  std::vector<int64_t> load((size_t)n_parts, 0);
  for (int64_t i : by_length) {
    const int p = (int)(std::min_element(load.begin(), load.end()) - load.begin());  // the first of the least loaded
    part[(size_t)i] = p;
    load[(size_t)p] += lengths[i];
  }
  return part;
}

Map::Map(const Parameters& p, wfm_handle_t* h) : Map(p, std::vector<wfm_handle_t*>{h}) {}

Map::Map(const Parameters& p, const std::vector<wfm_handle_t*>& hs) : param_(p), h_(hs.empty() ? nullptr : hs.front()), hs_(hs) {
  if (!h_ || std::find(hs_.begin(), hs_.end(), nullptr) != hs_.end()) throw std::runtime_error("no GPU handle");
  if (param_.querySequences.empty()) param_.querySequences = param_.refSequences;  // all-vs-all
  if (param_.sketchSize <= 0) {
    const double md = 1 - param_.percentageIdentity;
    const double dens = 0.02 * (1 + (md / 0.1));
    param_.sketchSize = dens * (param_.windowLength - param_.kmerSize);
  }
  if (param_.sketchSize < 1 || param_.sketchSize > param_.windowLength) throw std::runtime_error("sketch size must be in 1..window size");
  idManager_ = std::make_unique<SequenceIdManager>(param_.querySequences, param_.refSequences, param_.query_prefix,
                                                   std::vector<std::string>{param_.target_prefix}, std::string(1, param_.prefix_delim),
                                                   param_.query_list, param_.target_list);
  cached_minimum_hits_ = std::max(param_.minimum_hits, Stat::estimateMinimumHitsRelaxed(param_.sketchSize, param_.kmerSize,
                                                                                         param_.percentageIdentity, kConfidenceInterval));
}

int Map::mapQuery(MapSummary* summary) {
  const double t_begin = now_ms();
  MapRun R(param_, *idManager_, hs_);
  int rc = select_and_load(R);
  if (rc != WFM_OK) return rc;
  make_tables(R, cached_minimum_hits_);
  if ((rc = open_outputs(R)) != WFM_OK) return rc;
  for (size_t si = 0; si < R.subsets.size(); ++si) {
    IndexSet ixs(hs_);
    // the index of this subset (Sketch::build, or Sketch::readIndex with -I), then every query against it
    const double t0 = now_ms();
    rc = R.index_in.is_open() ? load_sub_index(R, si, ixs) : build_sub_index(R, si, ixs);
    if (rc == WFM_OK && param_.create_index_only) rc = write_sub_index_file(R, si, ixs);
    if (rc != WFM_OK) return rc;
    R.sum.ms_index += now_ms() - t0;
    if (param_.create_index_only) continue;
    if ((rc = replicate_index(R, ixs)) != WFM_OK) return rc;
    if ((rc = map_subset(R, si, ixs)) != WFM_OK) return rc;
  }
  if (param_.filterMode == filter::ONETOONE) one_to_one_pass(R);
  if (R.scaffold_file.is_open() && !R.scaffold_file.flush()) return R.error(WFM_E_ARG, "cannot write scaffold output file " + param_.scaffold_output_file);
  R.sum.ms_total = now_ms() - t_begin;
  if (summary) *summary = R.sum;
  return WFM_OK;
}

}  // namespace skch
