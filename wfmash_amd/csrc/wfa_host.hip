// wfa_host.hip -- host driver + C ABI of the align path (see include/wfmash_hip.h).
//
// Restates the control flow WFA2-lib runs on the CPU for
// WFAlignerGapAffine2Pieces::alignEnd2End(MemoryUltralow) (wflign.cpp:136-148):
// recursive BiWFA -- find breakpoint, split, recurse; sub-problems whose
// remaining score is <= 250 (or trivially empty) go to the unidirectional base
// aligner -- but breadth-first: every recursion level of every problem of the
// batch is ONE launch of wfa_bp_kernel plus ONE launch of wfa_base_kernel.
// Ends-free patches (wflign.cpp:280-305,368-397) are base jobs directly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/wfmash_hip.h"
#include "wfa_host_shared.h"
#include "wfa_plan.h"
#include "wfa_optband.h"

#ifdef WFM_PROFILE_SECTIONS
namespace wfm { void read_sections(long long* out); }
#endif
namespace wfm { void p2_counters(unsigned long long* out); }
namespace {

using namespace wfm;
static_assert(OP_M == 0 && OP_X == 1 && OP_I == 2 && OP_D == 3, "wfa_plan.h spells these out (it includes no HIP header)");

constexpr int BIALIGN_FALLBACK_MIN_SCORE = 250;   // WFA2-lib WF_BIALIGN_FALLBACK_MIN_SCORE
constexpr int BIALIGN_FALLBACK_MIN_LENGTH = 100;  // WFA2-lib WF_BIALIGN_FALLBACK_MIN_LENGTH
constexpr int SEQ_PAD = 64;  // extension reads up to 40 bytes past a sub-range end

// The state of a tiled job that ran out of its narrow ring, kept in a device block of its own until the job has its wider ring: the columns
// |k| <= s0 + 8 of every row of the snapshot of score s0 (both directions stand there), and the running maxima of the two directions
struct GrownSnap {
  int32_t* d = nullptr;
  int32_t w = 0, koff = 0;
  int32_t s0 = 0, fmax = 0, rmax = 0;
};
struct GrownSnaps {  // (the blocks of a call that ends early go back as well)
  std::vector<GrownSnap> v;
  void drop(int32_t id) { if (id > 0 && v[(size_t)id - 1].d) { wfm_dfree(v[(size_t)id - 1].d); v[(size_t)id - 1].d = nullptr; } }
  ~GrownSnaps() { for (size_t q = 0; q < v.size(); ++q) drop((int32_t)q + 1); }
};

// Parent reuse (wfa_plan.h): one direction of a job's snapshot at a block boundary, kept compact for the child that starts where that direction
// started.  The rows lie in slabs of the device heap; a slab goes back when the last of its keeps has.  pl / tl / sub: the keeping job's box
// and the bound its rows were cut to (what the child's ranges are checked against).
struct KeptRows {
  int32_t* d = nullptr;
  int32_t slab = -1;
  int32_t s0 = 0, mx = 0;      // the keep's score; the direction's running maximum there
  int32_t kmin = 0, n = 0;     // diagonals kmin .. kmin + n - 1
  int32_t pl = 0, tl = 0, sub = 0;
};
struct KeepStore {  // (the slabs of a call that ends early go back as well)
  struct Slab { int32_t* d = nullptr; size_t cap = 0, used = 0; int64_t live = 0; };
  std::vector<Slab> slabs;
  std::vector<KeptRows> v;     // Node::keep = 1 + index
  size_t cap_bytes = 0, held = 0, peak = 0;  // what the call's slabs may take; take now; took at most
  // elems of the newest slab, or of a fresh one while the cap allows; nullptr: the store is full (or the device is)
  int32_t* take(size_t elems, int32_t* slab_out) {
    if (slabs.empty() || slabs.back().used + elems > slabs.back().cap) {
      if (!slabs.empty() && slabs.back().live == 0) release((int32_t)slabs.size() - 1);
      const size_t want = std::max<size_t>(elems, (size_t)16 << 20);  // 64 MB at least
      if (held + want * 4 > cap_bytes) return nullptr;
      Slab sl;
      if (wfm_dmalloc((void**)&sl.d, want * sizeof(int32_t)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
      sl.cap = want;
      held += want * 4; peak = std::max(peak, held);
      slabs.push_back(sl);
    }
    Slab& sl = slabs.back();
    int32_t* p = sl.d + sl.used;
    sl.used += elems; sl.live += 1;
    *slab_out = (int32_t)slabs.size() - 1;
    return p;
  }
  // (a keep is dropped behind a wait for the call's stream, which its only writer and its only reader ran on: the slab goes back without
  // another wait -- one for the whole device would hold up the other parts of the batch.  Not so when the call ends early.)
  void release(int32_t i, bool wait = false) {
    Slab& sl = slabs[(size_t)i];
    if (!sl.d) return;
    if (wait) wfm_dfree(sl.d); else wfm_dfree_nosync(sl.d);
    held -= sl.cap * 4;
    sl.d = nullptr;
  }
  // a keep nobody will take any more; the slab behind it once it holds none (the newest slab is still being filled: it only starts over)
  void drop(int32_t id) {
    if (id <= 0 || !v[(size_t)id - 1].d) return;
    KeptRows& kr = v[(size_t)id - 1];
    kr.d = nullptr;
    Slab& sl = slabs[(size_t)kr.slab];
    if (--sl.live > 0) return;
    if ((size_t)kr.slab + 1 == slabs.size()) sl.used = 0; else release(kr.slab);
  }
  ~KeepStore() { for (size_t q = 0; q < slabs.size(); ++q) release((int32_t)q, true); }
};

}  // namespace

// wfm_seqstore_t: whole sequences on one device, normalised, one block of the device heap each.  `mu` guards the table (a block
// never moves, so a reader copies the entries it needs under the lock and reads the device memory without it); `add_mu` lets one
// add at a time use the pinned chunks.
struct wfm_seqstore {
  int device = 0;
  struct Seq { uint8_t* block = nullptr; uint8_t* data = nullptr; int64_t len = 0; size_t block_bytes = 0; };
  mutable std::mutex mu;
  std::vector<Seq> seqs;
  int64_t bytes = 0;
  std::mutex add_mu;
  uint8_t* pin[2] = {nullptr, nullptr};  // pinned chunks the raw bytes go through
  hipEvent_t pin_ev[2] = {nullptr, nullptr};
};

namespace {
// one time origin per device for the whole process: the busy intervals of calls on different handles of a device (the align
// driver keeps several batches in flight, each on a handle of its own) are reported against it and can be merged
std::mutex g_base_mu;
hipEvent_t g_dev_base[64] = {};
int g_dev_handles[64] = {};  // live handles per device (wfm_create / wfm_destroy)
// The origin as (event, milliseconds from the process's first origin on that device to the event).  hipEventElapsedTime
// returns a float: against an origin hours old its resolution is a millisecond or worse, so the origin is moved up every few
// minutes and the distance it has moved is kept as a double.
double g_dev_base_off[64] = {};
hipEvent_t device_base_event(int device, double* off_ms) {
  std::lock_guard<std::mutex> lk(g_base_mu);
  if (off_ms) *off_ms = 0;
  if (device < 0 || device >= 64) return nullptr;
  static hipStream_t clock_stream[64] = {};  // (a stream of its own, non-blocking: an event on the null stream would wait for every handle's work)
  if (!clock_stream[device] && hipStreamCreateWithFlags(&clock_stream[device], hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); clock_stream[device] = nullptr; }
  hipStream_t cs = clock_stream[device];
  auto fresh = [cs] {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) == hipSuccess && hipEventRecord(e, cs) == hipSuccess && hipEventSynchronize(e) == hipSuccess) return e;
    if (e) (void)hipEventDestroy(e);
    (void)hipGetLastError();
    return (hipEvent_t) nullptr;
  };
  if (!g_dev_base[device]) g_dev_base[device] = fresh();
  else {
    // (the age is taken with an event of the moment: cheap, and only on the rare calls that ask for the origin)
    hipEvent_t now = fresh();
    float age = 0;
    if (now && hipEventElapsedTime(&age, g_dev_base[device], now) == hipSuccess && age > 240000.0f) {
      // (handles that recorded their call's origin against the old event keep working: the old event is left alive)
      g_dev_base_off[device] += (double)age;
      g_dev_base[device] = now;
    } else if (now) (void)hipEventDestroy(now);
  }
  if (off_ms) *off_ms = g_dev_base_off[device];
  return g_dev_base[device];
}
}  // namespace

namespace { void (*g_last_handle_hook)() = nullptr; }
void wfm_set_last_handle_hook(void (*f)()) { g_last_handle_hook = f; }

namespace {

inline int gapcost(const wfm_penalties_t& p, int L) {
  if (L <= 0) return 0;
  return std::min(p.o1 + p.e1 * L, p.o2 + p.e2 * L);
}

// rows of a wavefront ring for penalties of this scope: 32 (the default penalties: scope 26) or 128
inline int ring_rows_for(int scope) { return scope <= RING - 2 ? RING : RING_BIG; }

struct LevelTimer {
  double bp_ms = 0, base_ms = 0, tile_ms = 0;
};

// the widest row of a base job (0 for the trivial all-gap jobs) and its columns: base_columns of wfa_plan.h on the job's problem
inline void job_columns(const Node& nd, const ProbMeta& pm, int64_t* kmin_out, int64_t* kmax_out) {
  // (a once-per-process switch: it stays static)
  static const bool corner_band = !(getenv("WFM_BASE_CORNER_BAND") && atoi(getenv("WFM_BASE_CORNER_BAND")) == 0);
  base_columns(nd, pm.pbf, pm.pef, pm.tbf, pm.tef, corner_band, kmin_out, kmax_out);
}
inline int64_t base_row_width(const Node& nd, const ProbMeta& pm) {
  if (nd.tl == 0 || nd.pl == 0) return 0;
  int64_t kmin, kmax;
  job_columns(nd, pm, &kmin, &kmax);
  return kmax - kmin + 1;
}

// ---- base jobs: run_base_jobs (at the end) is the loop over chunks of one kind, the stages before it do the work ----

// The switches of the base jobs, read from the environment once per call (the tests run both forms in one process)
struct BaseCfg {
  bool base_v2 = true, base_tiles = true, force_tiles = false;  // BaseRules' of the same names
  int debug = 0;                                                  // WFM_DEBUG (0: unset)
};
BaseCfg base_cfg(const wfm_penalties_t& pen) {
  BaseCfg c;
  const bool dflt_pen = pen.x == 5 && pen.o1 == 8 && pen.e1 == 2 && pen.o2 == 24 && pen.e2 == 1;
  c.base_v2 = dflt_pen && env_num("WFM_BASE_V2", 1) != 0 && env_num("WFM_TILE_V2", 1) != 0;
  c.base_tiles = env_num("WFM_BASE_TILES", 1) != 0;
  c.force_tiles = env_num("WFM_BASE_TILES", 1) == 2;
  c.debug = env_debug();
  return c;
}

// One call of run_base_jobs and the chunk at hand: jobs of one kind (base_kind) whose arenas share the budget
struct BaseChunk {
  wfm_handle* h; wfm_seqset* S; const wfm_penalties_t& pen; const BaseCfg& cfg;  // run_base_jobs' arguments
  std::vector<Node>& nodes; std::vector<Node>& retry; std::vector<int32_t>& prob_status; std::vector<uint64_t>& prob_cells;
  LevelTimer& tm; uint32_t* pflags;
  std::vector<int32_t>& prob_score;  // score-only problems: the score their base job found
  int RR;
  BaseRules rules;
  std::vector<BaseJob> jobs;  // BaseJob::pad_: the job's node
  std::vector<BaseResult> res;
  size_t n32 = 0, n8 = 0;     // elements of base32 / bytes of base8 the chunk's jobs take
  size_t end = 0;             // the first node behind the chunk
  int kind = 3;
  float ms = 0;
};

inline bool is_acgt(const wfm_seqset* S, int32_t prob) { return (size_t)prob < S->acgt.size() && S->acgt[(size_t)prob]; }
inline int base_kind_of(const BaseChunk& c, const Node& a) {
  return base_kind(base_row_width(a, c.S->meta[a.prob]), a.pl, a.tl, a.tries, is_acgt(c.S, a.prob), c.rules);
}

// The chunk that begins at node i0: jobs of one kind, as many as the budget holds; their geometry and their places in the arenas
void fill_base_chunk(BaseChunk& c, size_t i0) {
  wfm_handle* h = c.h;
  c.jobs.clear();
  c.n32 = 0; c.n8 = 0; c.kind = 3;
  size_t i = i0;
  for (; i < c.nodes.size(); ++i) {
    const Node& nd = c.nodes[i];
    const ProbMeta& pm = c.S->meta[nd.prob];
    {  // a chunk holds jobs of one kind
      const int kind = base_kind_of(c, nd);
      if (c.jobs.empty()) c.kind = kind;
      else if (kind != c.kind) break;
    }
    BaseJob j{};
    j.p_off = pm.p_fwd + nd.pb;
    j.t_off = pm.t_fwd + nd.tb;
    j.pl = nd.pl; j.tl = nd.tl;
    j.comp_begin = nd.cb; j.comp_end = nd.ce;
    j.endsfree = nd.endsfree;
    j.pbf = pm.pbf; j.pef = pm.pef; j.tbf = pm.tbf; j.tef = pm.tef;
    j.rle_end = pm.rle_off + nd.pb + nd.tb + nd.pl + nd.tl;
    j.pad_ = (int32_t)i;
    j.score_only = pm.score_only() ? 1 : 0;  // (such a problem's base jobs are its roots: a score-only BiWFA root has no children)
    if (nd.tl == 0 || nd.pl == 0) {
      j.type = nd.tl == 0 ? 1 : 2;
      if (nd.tl == 0 && nd.pl == 0) { j.type = 1; }
      c.jobs.push_back(j);
      continue;
    }
    j.type = 0;
    j.smax = nd.smax;
    int64_t kmin64, kmax64;
    job_columns(nd, pm, &kmin64, &kmax64);
    const int kmin = (int)kmin64, kmax = (int)kmax64;
    j.kmin = kmin;
    j.width = kmax - kmin + 1;
    const size_t rows = (size_t)nd.smax + 1;
    const size_t need32 = rows * (size_t)j.width + (size_t)5 * c.RR * (size_t)j.width;
    const size_t need8 = rows * (size_t)j.width;
    // (a chunk of base jobs stops at 4 GB of arenas even where the budget allows more, like a chunk of rings: with the leaves of all levels going out
    // together a batch of divergent records asked for 18 GB blocks -- 0.6 s each as a first allocation, gpurun_out/r5u_c1.err -- and thousands of
    // leaves fill the device long before that)
    static const size_t base_chunk_bytes = (size_t)(getenv("WFM_BASE_CHUNK_GB") ? std::max(1, atoi(getenv("WFM_BASE_CHUNK_GB"))) : 4) << 30;
    if (!c.jobs.empty() && (c.n32 + need32) * 4 + (c.n8 + need8) > std::min(h->mem_budget, base_chunk_bytes)) break;
    if (need32 * 4 + need8 > h->mem_budget) {  // a single job beyond the budget
      c.prob_status[nd.prob] = WFM_ST_OOM;
      continue;
    }
    j.pre_off = (int64_t)c.n32;
    j.ring_off = (int64_t)(c.n32 + rows * (size_t)j.width);
    j.bt_off = (int64_t)c.n8;
    c.n32 += need32; c.n8 += need8;
    c.jobs.push_back(j);
  }
  c.end = i;
}

// Kind 5, the register kernel's step on tiles: blocks of T scores, every block one launch over the tiles of all jobs and a one-thread-per-job
// kernel behind it; the host looks at the number of jobs still running every few blocks (a launch whose jobs are all over costs microseconds)
int launch_base_tiles(BaseChunk& c) {
  wfm_handle* h = c.h;
  const std::vector<BaseJob>& jobs = c.jobs;
  // (a once-per-process switch: it stays static)
  static const int T = getenv("WFM_BASE_TILE_T") ? std::max(5, std::min(400, atoi(getenv("WFM_BASE_TILE_T")) / 5 * 5)) : 125;
  std::vector<int32_t> widths(jobs.size()), smaxs(jobs.size());
  for (size_t q = 0; q < jobs.size(); ++q) { widths[q] = jobs[q].width; smaxs[q] = jobs[q].smax; }
  const BaseTilePlan plan = plan_base_tiles(widths.data(), smaxs.data(), jobs.size(), T, B2T_THREADS);
  std::vector<Base2TJob> tj(jobs.size());
  std::vector<Base2TTask> tasks;
  for (size_t q = 0; q < jobs.size(); ++q) {
    Base2TJob& t = tj[q];
    t.b = jobs[q];
    t.snap_in = jobs[q].ring_off; t.snap_out = jobs[q].ring_off + (int64_t)B2T_ROWS * jobs[q].width;
    t.core = plan.core; t.ntiles = plan.ntiles[q]; t.task0 = (int32_t)tasks.size();
    t.s0 = 0; t.done = 0; t.end_s = 0; t.end_k = 0; t.end_off = 0;
    for (int ti = 0; ti < t.ntiles; ++ti) tasks.push_back(Base2TTask{(int32_t)q, ti});
  }
  const int nblocks = plan.nblocks;
  if (h->b2tjobs.ensure(tj.size()) || h->b2ttasks.ensure(tasks.size()) || h->b2tkeys.ensure(tasks.size()) || h->b2toffs.ensure(tasks.size()) || h->b2tactive.ensure((size_t)nblocks)) {
    h->err = "out of device memory (base tiles)";
    return WFM_E_NOMEM;
  }
  HIPCHK(h, hipMemcpyAsync(h->b2tjobs.p, tj.data(), tj.size() * sizeof(Base2TJob), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->b2ttasks.p, tasks.data(), tasks.size() * sizeof(Base2TTask), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(h->b2tactive.p, 0, (size_t)nblocks * sizeof(int32_t), h->stream));
  constexpr int LOOK = 6;
  for (int b = 0; b < nblocks; ) {
    const int upto = std::min(nblocks, b + LOOK);
    for (; b < upto; ++b) {
      launch_base2t_block(c.S->d_pk, h->base32.p, h->base8.p, h->b2tjobs.p, h->b2ttasks.p, h->b2tkeys.p, h->b2toffs.p, (int)tasks.size(), T, h->stream);
      launch_base2t_advance(h->b2tjobs.p, h->b2tkeys.p, h->b2toffs.p, (int)tj.size(), T, h->b2tactive.p + b, h->stream);
    }
    int32_t still = 0;
    HIPCHK(h, hipMemcpyAsync(&still, h->b2tactive.p + (b - 1), sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!still) break;
  }
  launch_base2t_finish(h->base32.p, h->base8.p, h->rle.p, h->b2tjobs.p, h->bsres.p, (int)tj.size(), h->stream);
  return WFM_OK;
}

// The chunk on the device: its jobs up, the launch its kind asks for, the results back; the time it took
int run_base_chunk(BaseChunk& c) {
  wfm_handle* h = c.h;
  const std::vector<BaseJob>& jobs = c.jobs;
  if (h->base32.ensure(c.n32 + 16) || h->base8.ensure(c.n8 + 16) || h->bsjobs.ensure(jobs.size()) || h->bsres.ensure(jobs.size())) {
    h->err = "out of device memory (base arena)";
    return WFM_E_NOMEM;
  }
  HIPCHK(h, hipMemcpyAsync(h->bsjobs.p, jobs.data(), jobs.size() * sizeof(BaseJob), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipEventRecord(h->ev2, h->stream));
  // (jobs arrive sorted: the wide ones -- long patches, retries with a larger budget -- in chunks of their own)
  if (c.kind == 5) {
    const int rc = launch_base_tiles(c);
    if (rc != WFM_OK) return rc;
  } else if (c.kind <= 2) {
    int64_t wmax = 1;
    for (const BaseJob& bj : jobs) if (bj.type == 0) wmax = std::max<int64_t>(wmax, bj.width);
    const int threads = (int)std::min<int64_t>(1024, ((wmax + 1) / 2 + 63) / 64 * 64);
    launch_base2(c.S->d_pk, h->base32.p, h->base8.p, h->rle.p, h->bsjobs.p, h->bsres.p, (int)jobs.size(), threads, h->stream);
  } else {
    const DevPen dp{c.pen.x, c.pen.o1, c.pen.e1, c.pen.o2, c.pen.e2};
    launch_base(c.S->d_seq, h->base32.p, h->base8.p, h->rle.p, h->bsjobs.p, h->bsres.p, (int)jobs.size(), dp, c.kind == 4, c.RR, h->stream);
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev3, h->stream));
  c.res.resize(jobs.size());
  HIPCHK(h, hipMemcpyAsync(c.res.data(), h->bsres.p, jobs.size() * sizeof(BaseResult), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipEventElapsedTime(&c.ms, h->ev2, h->ev3));
  c.tm.base_ms += c.ms;
  if (h->call_base) {
    float t0 = 0;
    HIPCHK(h, hipEventElapsedTime(&t0, h->call_base, h->ev2));
    h->base_iv.emplace_back(t0, t0 + c.ms);
  }
  h->stats.base_launches++;
  h->stats.base_jobs += (uint32_t)jobs.size();
  return WFM_OK;
}

// WFM_DEBUG=2: the chunk's launch in a line or two
void print_base_chunk(const BaseChunk& c) {
  const std::vector<BaseJob>& jobs = c.jobs;
  const std::vector<BaseResult>& res = c.res;
  const int chunk_kind = c.kind;
  int64_t wsum = 0, wmax = 0, smx = 0; int over = 0, ef = 0;
  for (size_t q = 0; q < jobs.size(); ++q) { wsum += jobs[q].width; wmax = std::max<int64_t>(wmax, jobs[q].width); smx = std::max<int64_t>(smx, jobs[q].smax); over += res[q].status == WFM_DEV_OVERFLOW; ef += jobs[q].endsfree; }
  fprintf(stderr, "[wfm] base launch: %zu jobs (%d ends-free), %d threads, rows %lld wide on average (max %lld), score budget up to %lld, %.3f ms, %d overflowed\n", jobs.size(), ef,
          chunk_kind == 5 ? B2T_THREADS : (chunk_kind == 4 ? 1024 : 256), (long long)(wsum / (int64_t)jobs.size()), (long long)wmax, (long long)smx, c.ms, over);
  if (chunk_kind <= 2) {
    double fw = 0, bk = 0; int fwm = 0, bkm = 0, scm = 0; double scs = 0;
    for (size_t q = 0; q < jobs.size(); ++q) { const int f = (res[q].pad_ >> 16) & 0xffff, b = res[q].pad_ & 0xffff; fw += f; bk += b; fwm = std::max(fwm, f); bkm = std::max(bkm, b); scs += res[q].score; scm = std::max(scm, res[q].score); }
    fprintf(stderr, "[wfm]   register kernel (kind %d): forward %.0f us on average (max %d), walk back %.0f us (max %d), score %.0f on average (max %d)\n", chunk_kind, fw / jobs.size(), fwm, bk / jobs.size(), bkm, scs / jobs.size(), scm);
  }
  else {
    double scs = 0; int scm = 0, scn = INT_MAX;
    for (size_t q = 0; q < jobs.size(); ++q) { scs += res[q].score; scm = std::max(scm, res[q].score); scn = std::min(scn, res[q].score); }
    fprintf(stderr, "[wfm]   %s (kind %d): score %.0f on average (min %d, max %d)\n", chunk_kind == 5 ? "register kernel on tiles" : "ring kernel", chunk_kind, scs / jobs.size(), scn, scm);
  }
}

// The chunk's results: cells and flags, and the jobs that overflowed their score budget once more with a larger one (into retry)
void settle_base_chunk(BaseChunk& c) {
  wfm_handle* h = c.h;
  const wfm_penalties_t& pen = c.pen;
  for (size_t q = 0; q < c.jobs.size(); ++q) {
    const Node& nd = c.nodes[(size_t)c.jobs[q].pad_];
    const BaseResult& r = c.res[q];
    c.prob_cells[nd.prob] += r.cells;
    h->stats.cells_base += r.cells;
    if (c.pflags && (c.kind == 3 || c.kind == 4) && c.jobs[q].type == 0) c.pflags[nd.prob] |= WFM_PF_RING_KERNEL;
    if (c.pflags && c.kind == 5) c.pflags[nd.prob] |= WFM_PF_BASE_TILES;
    // The score of a problem whose root is this job: a score-only problem's, and an ends-free problem's either way (what its op string
    // costs run by run counts the free end gaps as well; the job's own score does not).  The all-gap jobs report no score of their own:
    // theirs is the gap's -- of an ends-free problem, what its side's two free lengths leave of it
    if (r.status == 0 && (c.jobs[q].score_only || nd.endsfree)) {
      const ProbMeta& pm = c.S->meta[nd.prob];
      const int all_gap = nd.endsfree ? gapcost(pen, nd.pl - pm.pbf - pm.pef) + gapcost(pen, nd.tl - pm.tbf - pm.tef)
                                      : gapcost(pen, nd.pl) + gapcost(pen, nd.tl);
      c.prob_score[nd.prob] = c.jobs[q].type == 0 ? r.score : all_gap;
    }
    if (r.status == WFM_DEV_OVERFLOW && nd.limit > 0 && nd.smax >= nd.limit) {  // the budget was the problem's hard limit: final
      c.prob_status[nd.prob] = WFM_ST_MAX_SCORE; continue;
    }
    if (r.status == WFM_DEV_OVERFLOW) {
      if (c.pflags) c.pflags[nd.prob] |= nd.tries == 0 ? WFM_PF_BASE_RETRY : WFM_PF_BASE_RETRY2;
      Node again = nd;
      again.tries = nd.tries + 1;
      // No alignment costs more than the all-gap one.  A job whose begin or end component is a gap state is held to a
      // PIECE there (a BiWFA child that ends inside a D2 gap pays o2 + e2 per base for it, however short it is --
      // its parent counted that gap's opening on the other side of the breakpoint, so the child's own forward score
      // exceeds the score_rem it was handed): the bound takes the dearer piece for both gaps then.
      const bool constrained = nd.cb != C_M || nd.ce != C_M;
      const int64_t bound = constrained
          ? (int64_t)2 * std::max(pen.o1, pen.o2) + (int64_t)std::max(pen.e1, pen.e2) * ((int64_t)nd.pl + nd.tl) + 8
          : (int64_t)gapcost(pen, nd.pl) + gapcost(pen, nd.tl) + 8;
      if (nd.smax >= bound) {
        if (c.cfg.debug) fprintf(stderr, "[wfm] problem %d: base job pl %d tl %d cb %d ce %d overflowed its score bound %d\n", nd.prob, nd.pl, nd.tl, nd.cb, nd.ce, nd.smax);
        c.prob_status[nd.prob] = WFM_ST_UNREACHABLE; continue;
      }
      // (x 8; it was x 2 until round 3 and x 4 for a while: every retry is a launch that a few jobs hold up, a budget that is too large costs
      // memory only -- 20 MB for a 2 k-wide patch at 2 k scores -- and a patch that passed 256 is as likely to need 1500 as 500)
      again.smax = (int32_t)std::min<int64_t>((int64_t)nd.smax * 8 + 32, bound);
      // ... but the second attempt stops at 1020: with the band around the end corner's diagonal the rows of a job with that budget are at most
      // 2041 diagonals wide and fit the register kernel (wfa_base2_kernel: 2048), where a budget of 2080 put two dozen patches of an LPA batch
      // on the ring kernel with rows of 2.6 - 3.4 k diagonals (9.7 ms of the batch's 83); the few that need more take a third attempt
      // (round 6: a job the tiles of the register kernel take -- wfa_base2t_kernel, rows of any width -- has no use for the stop: its second attempt
      // runs with the eightfold budget at once, 2.0 ms of an LPA batch's patch chain less)
      const bool to_tiles = c.rules.base_v2 && c.rules.base_tiles && is_acgt(c.S, nd.prob);
      if (nd.smax < 1020 && again.smax > 1020 && !to_tiles) again.smax = 1020;
      if (nd.limit > 0) again.smax = std::min(again.smax, nd.limit);
      c.retry.push_back(again);
    } else if (r.status != 0) {
      if (c.cfg.debug) fprintf(stderr, "[wfm] problem %d: base job pl %d tl %d status %d\n", nd.prob, nd.pl, nd.tl, r.status);
      c.prob_status[nd.prob] = WFM_ST_UNREACHABLE;
    }
  }
}

// Runs all base jobs of `nodes` (chunked to the memory budget, every kind of job in chunks of its own); appends
// overflowed nodes (with a larger budget) to `retry`.
int run_base_jobs(wfm_handle* h, wfm_seqset* S, const wfm_penalties_t& pen, const BaseCfg& cfg, std::vector<Node>& nodes,
                  std::vector<Node>& retry, std::vector<int32_t>& prob_status, std::vector<uint64_t>& prob_cells,
                  LevelTimer& tm, uint32_t* pflags, std::vector<int32_t>& prob_score) {
  if (nodes.empty()) return WFM_OK;
  BaseChunk c{h, S, pen, cfg, nodes, retry, prob_status, prob_cells, tm, pflags, prob_score,
              ring_rows_for(std::max(pen.x, std::max(pen.o1 + pen.e1, pen.o2 + pen.e2)) + 1)};
  // rows beyond 2 k diagonals get 1024 threads -- and rows beyond 512 when the launch is too small to fill the device anyway
  // (the retries of the few patches that overflowed their first budget: one workgroup each, a thousand steps deep)
  c.rules = BaseRules{cfg.base_v2, cfg.base_tiles, cfg.force_tiles, nodes.size() < 128, nodes.size() < 128 ? 512 : 2048};
  std::stable_sort(nodes.begin(), nodes.end(), [&](const Node& a, const Node& b) { return base_kind_of(c, a) < base_kind_of(c, b); });
  for (size_t i0 = 0; i0 < nodes.size(); i0 = c.end) {
    fill_base_chunk(c, i0);
    if (c.jobs.empty()) continue;
    const int rc = run_base_chunk(c);
    if (rc != WFM_OK) return rc;
    if (cfg.debug > 1) print_base_chunk(c);
    settle_base_chunk(c);
  }
  return WFM_OK;
}


struct TileCfg {
  bool exact = true;  // register tiles: re-run the block that holds the meeting point up to that point only, so the step
                      // kernel starts at phase 2 (WFM_TILE_EXACT=0: it redoes the block step by step instead)
  int T_refine = 0;   // optional second pass over the block that holds the meeting point, in finer blocks (WFM_TILE_T_REFINE;
                      // measured neutral on C3: what the step kernel saves, the small tiles cost)
  int chunk = 2;  // tile blocks launched back to back between two looks of the host (WFM_TILE_CHUNK); more only adds idle tiles
  int T = 100, Wt = 1024, threads = 512;  // T: scores per tile block (measured optimum 96-100 on C3: halo 2T of 1024 columns vs per-tile snapshot cost)
  int min_len = 128, min_score = 64;  // shorter problems go to the step kernel whole (they are base jobs at <= 100 anyway).  600 until round 2: the
                                      // short, high-score children a 1 kb end gap leaves behind then queued up as one-workgroup step jobs
  bool enabled = true;
  bool reg = false;  // register-resident tile kernel (default penalty lags only)
  int C = 2;
  bool fine = true;  // WFM_TILE_FINE: the blocks of a single-tile chunk get workgroups as small as their own widest range allows
  int debug = 0;     // WFM_DEBUG (0: unset)
  bool p2_dump_on = false;  // WFM_P2_DUMP (diagnosis): the row maxima of job p2_dump of every chunk of phase 2
  int p2_dump = 0;
};

TileCfg tile_cfg(const wfm_penalties_t& pen, int scope) {
  TileCfg c;
  if (const char* e = getenv("WFM_TILE")) c.enabled = atoi(e) != 0;
  if (const char* e = getenv("WFM_TILE_T")) c.T = atoi(e);
  if (const char* e = getenv("WFM_TILE_T_REFINE")) c.T_refine = atoi(e);
  if (const char* e = getenv("WFM_TILE_EXACT")) c.exact = atoi(e) != 0;
  if (const char* e = getenv("WFM_TILE_W")) c.Wt = atoi(e);
  if (const char* e = getenv("WFM_TILE_THREADS")) c.threads = atoi(e);
  if (const char* e = getenv("WFM_TILE_MIN_LEN")) c.min_len = atoi(e);
  if (const char* e = getenv("WFM_TILE_MIN_SCORE")) c.min_score = atoi(e);
  c.fine = env_num("WFM_TILE_FINE", 1) != 0;
  c.debug = env_debug();
  if (const char* e = getenv("WFM_P2_DUMP")) { c.p2_dump_on = true; c.p2_dump = atoi(e); }
  const int RR = ring_rows_for(scope);
  c.T = std::max(c.T, RR);  // the output snapshot needs `scope` rows of the block itself
  if (c.T_refine > 0) c.T_refine = std::max(c.T_refine, RR);
  const bool dflt = pen.x == 5 && pen.o1 + pen.e1 == 10 && pen.o2 + pen.e2 == 25 && pen.e1 == 2 && pen.e2 == 1;
  c.reg = dflt && !(getenv("WFM_TILE_REG") && atoi(getenv("WFM_TILE_REG")) == 0);
  if (c.reg) {
    if (!getenv("WFM_TILE_THREADS")) c.threads = 512;
    // (the FINE instantiation of the packed kernel keeps T + 1 scores' maxima, tile_fine_slots words each, in dynamic LDS beside ~24 KB of static:
    // a WFM_TILE_T that would not fit 64 KB is cut here instead of failing the launch -- at the slots of the widest workgroups, whatever c.threads)
    c.T = std::min(c.T, (int)((40 * 1024) / (4 * TILE_SLOTS_WIDE)) - 1);
    // (a tile beside others keeps Wt - 2 T diagonals of its own between its halos: a WFM_TILE_THREADS too small to keep any is raised, wave by
    // wave, to the first that does -- 64 threads at T = 100 run as 128)
    while (c.threads * c.C <= 2 * c.T && c.threads < 1024) c.threads += 64;
    // (two diagonals per lane, always: the phase-2 rows, the single-tile sizing and the packed kernel are built for it.  The WFM_TILE_C=4
    // switch of round 1 sized the tasks for four while those stages went on with two -- wrong results; it is gone)
    if (const char* e = getenv("WFM_TILE_CHUNK")) c.chunk = std::max(1, atoi(e));
    c.Wt = c.threads * c.C;
    return c;
  }
  const size_t rows = (size_t)scope + 2 * (pen.e1 + 1) + 2 * (pen.e2 + 1);
  while ((rows * c.Wt + c.T + 1) * 4 > 160 * 1024 && c.Wt > 4 * c.T) c.Wt -= 64;
  if (c.Wt < 4 * c.T || (rows * c.Wt + c.T + 1) * 4 > 160 * 1024) c.enabled = false;  // (a scope beyond ~60 rows: the step kernel does it all)
  return c;
}

// ---- the tile phase: run_tiled_phase (at the end) is the loop over chunks of blocks, the stages before it do the work ----

// What the tile kernels need of a breakpoint job.  The caller sets what differs between the tile phase and the phase-2 rows:
// ring_out, mode, tf / tr, last_fwd, fine_s, ring_prev, p2_off / w2 / koff2
inline TileJob tile_job_from(const BpJob& j) {
  TileJob t{};
  t.p_fwd = j.p_fwd; t.t_fwd = j.t_fwd; t.p_rev = j.p_rev; t.t_rev = j.t_rev;
  t.ring_in = j.ring_off;
  t.pl = j.pl; t.tl = j.tl; t.comp_begin = j.comp_begin; t.comp_end = j.comp_end;
  t.width = j.width; t.koff = j.koff; t.active = 1; t.packed = j.packed; t.sub = j.sub;
  return t;
}

// Parent reuse, as the tile phase sees it: which of its jobs take a direction from a keep, which keep their own directions for their
// children, and what became of both (entries follow `tiled`)
struct ReuseUse { int32_t keep = 0, dir = 0, s_k = 0; };  // keep: Node::keep (0: both directions start at score 0), the direction it is of, its score
struct ReuseCtl {
  KeepStore* store = nullptr;
  int cadence = 0;             // blocks between two keeps (whole chunks); 0: nobody keeps
  int slack = 0;               // WFM_REUSE_TOUCH_SLACK
  int min_blocks = 1;          // WFM_REUSE_MIN_BLOCKS: no keep below this many blocks
  std::vector<ReuseUse> use;
  std::vector<int32_t> upto;   // the last score the job keeps at (0: it keeps nothing)
  std::vector<int32_t> meet;   // the score its directions meet at, where the job knows its score (half of it); 0: to be read off its progress
  std::vector<char> bad;       // out: the job gave its keep up after it had begun: it is run again, both directions from score 0
  std::vector<std::vector<int32_t>> kept[2];  // out: the keeps the job wrote (Node::keep values), per direction
  uint64_t keep_bytes = 0, restore_bytes = 0;  // out: what the two kernels moved (read + written)
};

// One pass of the tile phase over the jobs listed in `tiled`, and the chunk of blocks at hand
struct TilePhase {
  wfm_handle* h; wfm_seqset* S; const DevPen& dp; int scope; const TileCfg& cfg; int T; bool refine;  // run_tiled_phase's arguments
  std::vector<BpJob>& jobs; const std::vector<int>& tiled; std::vector<int64_t>& ring2; double& tile_ms; uint64_t& tile_cells;
  size_t n;
  std::vector<TileJob> tj, got;          // the jobs as the host last saw them; as the chunk left them
  std::vector<int> fmax, rmax, s_begin;  // running maxima of the two directions; score the jobs start this pass at
  std::vector<char> active;
  size_t n_active = 0;
  bool any_cut = false;  // the kernel form with the score bounds' bookkeeping is only launched when a job carries one
  bool any_planned = false;  // jobs with a planned end run on the instantiation without per-score maxima (TilePlanRules::planned)
  bool plan_deep = env_num("WFM_TILE_PLANNED_DEEP", 1) != 0;  // TileJob::plan_deep (read per call)
  int chunk = 1;         // blocks launched back to back between two looks of the host
  TilePlanRules rules;
  std::vector<TilePlanJob> pjobs;
  TileChunkPlan plan;
  uint32_t blocks = 0;
  uint32_t launches_coarse = 0, launches_fine = 0, reruns5 = 0, reruns6 = 0;  // this phase's share of the call's tile counters (the WFM_DEBUG line)
  double lane_cells = 0;  // threads x diagonals per thread x scores over all tiles launched (diagnostics)
  // parent reuse (ru == nullptr: none of it)
  ReuseCtl* ru = nullptr;
  std::vector<uint8_t> dirs, own;   // per job: the directions that get tiles (bit 0 forward, bit 1 reverse); those it has computed from score 0 itself
  std::vector<int32_t> resumed_at;  // the score the job took its keep at (0: it has not), -1 once it is a block past it
  std::vector<KeepTask> ktasks;     // the keeps behind the chunk at hand, their Node::keep values
  std::vector<int32_t> kids;
  std::vector<RestoreTask> rtasks;
  std::vector<int32_t> rres;
};

// A job gives up the keep it began with: it leaves the tile phase here (mode 3, as a job that ran out of its band) and the host runs it again
// without one.  It drops no record: the node goes to the next level as it came, less the keep.
void reuse_fall_back(TilePhase& p, size_t i, bool touched = false) {
  if (p.active[i]) { p.active[i] = 0; --p.n_active; }
  p.tj[i].active = 0; p.tj[i].mode = 3;
  p.dirs[i] = 3; p.resumed_at[i] = -1;
  p.ru->bad[i] = 1;
  p.ru->store->drop(p.ru->use[i].keep);
  p.h->tile_ctr[WFM_TC_REUSE_FALLBACKS] += 1;
  p.h->tile_ctr[touched ? WFM_TC_REUSE_TOUCHED : WFM_TC_REUSE_FELL_OTHER] += 1;
}

// The jobs' TileJobs, and where they stand: at score 0 after the init kernel, or (refine) where a pass before left them
int init_tile_jobs(TilePhase& p, const std::vector<int32_t>* fine_from, const std::vector<int64_t>* ring3, const std::vector<int32_t>* plan_from) {
  wfm_handle* h = p.h;
  const TileCfg& cfg = p.cfg;
  const size_t n = p.n;
  const int T = p.T;
  p.tj.resize(n); p.fmax.assign(n, 0); p.rmax.assign(n, 0); p.active.assign(n, 1); p.s_begin.assign(n, 0);
  p.dirs.assign(n, 3); p.own.assign(n, 3); p.resumed_at.assign(n, 0);
  if (p.ru) { p.ru->bad.assign(n, 0); p.ru->kept[0].assign(n, {}); p.ru->kept[1].assign(n, {}); }
  for (size_t i = 0; i < n; ++i) {
    const BpJob& j = p.jobs[(size_t)p.tiled[i]];
    TileJob& t = p.tj[i];
    t = tile_job_from(j);
    t.ring_out = p.ring2[i];
    t.fine_s = (fine_from && i < fine_from->size()) ? (*fine_from)[i] : INT_MAX;  // (TileJob::fine_s; a job whose score nobody knows finds its meeting block by running it again)
    // a third ring (TileJob::ring_prev): packed jobs of the exact tile phase only -- the byte kernel and the step kernel's fall-backs read gap rows
    // 26 deep from any snapshot
    t.ring_prev = (ring3 && i < ring3->size() && (*ring3)[i] >= 0 && (j.packed & 1) && cfg.reg && cfg.exact && !p.refine) ? (*ring3)[i] : -1;
    h->tile_ctr[WFM_TC_RING3] += t.ring_prev >= 0;
    // the planned end (TileJob::plan_sum): the exact tile phase's first pass only
    t.plan_sum = (plan_from && i < plan_from->size() && !p.refine && cfg.reg && cfg.exact && (j.packed & 1)) ? (*plan_from)[i] : 0;
    t.plan_deep = (t.plan_sum > 0 && p.plan_deep) ? 1 : 0;
    p.any_planned |= t.plan_sum > 0 && t.fine_s == INT_MAX;
  }
  if (!p.refine || T == cfg.T) h->tile_ctr[WFM_TC_JOBS] += n;  // (a WFM_TILE_T_REFINE pass goes on with jobs already counted; a resumed job enters)
  for (size_t i = 0; i < n; ++i) p.any_cut |= p.tj[i].sub != SUB_NONE;
  if (h->tilejobs.ensure(n) || h->tilemak.ensure(n * 2 * (size_t)std::max(T, 2))) { h->err = "out of device memory (tiles)"; return WFM_E_NOMEM; }
  if (!p.refine) {
    HIPCHK(h, hipMemcpyAsync(h->tilejobs.p, p.tj.data(), n * sizeof(TileJob), hipMemcpyHostToDevice, h->stream));
    launch_tile_init(p.S->d_seq, h->ring.p, h->tilejobs.p, h->tilemak.p, (int)n, ring_rows_for(p.scope), h->stream);
    HIPCHK(h, hipGetLastError());
    std::vector<int32_t> mak(n * 4);
    HIPCHK(h, hipMemcpyAsync(mak.data(), h->tilemak.p, n * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; ++i) {
      p.fmax[i] = mak[(i * 2 + 0) * 2]; p.rmax[i] = mak[(i * 2 + 1) * 2];
      const bool ended = mak[(i * 2 + 0) * 2 + 1] || mak[(i * 2 + 1) * 2 + 1];
      const int A = p.tj[i].pl + p.tj[i].tl - 1;
      if (ended || p.fmax[i] + p.rmax[i] >= A) p.active[i] = 0;  // wfa_bp_kernel handles it from score 0
      p.n_active += p.active[i];
      p.tj[i].active = p.active[i]; p.tj[i].fmax = p.fmax[i]; p.tj[i].rmax = p.rmax[i]; p.tj[i].nblocks = 0;
    }
    // jobs that take their outer direction from a keep run the inner one alone for now; the outer one's maximum stands at the keep's meanwhile,
    // an upper bound of all its earlier rows (the advance kernel finds no maxima of a direction without tiles and leaves it there)
    for (size_t i = 0; p.ru && i < n; ++i) {
      ReuseUse& u = p.ru->use[i];
      if (u.keep <= 0) continue;
      const int A = p.tj[i].pl + p.tj[i].tl - 1;
      const int kept_max = p.ru->store->v[(size_t)u.keep - 1].mx;
      if (!p.active[i] || kept_max + (u.dir == 0 ? p.rmax[i] : p.fmax[i]) >= A) {  // nothing has run yet: the job simply starts both directions
        p.ru->store->drop(u.keep); u.keep = 0;
        h->tile_ctr[WFM_TC_REUSE_FALLBACKS] += 1;
        h->tile_ctr[WFM_TC_REUSE_FELL_OTHER] += 1;
        continue;
      }
      (u.dir == 0 ? p.fmax[i] : p.rmax[i]) = kept_max;
      p.tj[i].fmax = p.fmax[i]; p.tj[i].rmax = p.rmax[i];
      p.dirs[i] = (uint8_t)(1 << (1 - u.dir)); p.own[i] = p.dirs[i];
    }
    // a planned end in the first block: that block is the run up to it (the advance kernel does the same between two blocks)
    for (size_t i = 0; i < n; ++i) if (p.active[i]) tile_plan_enter(p.tj[i], T);
  } else {
    for (size_t i = 0; i < n; ++i) {
      const BpJob& j = p.jobs[(size_t)p.tiled[i]];
      const int A = p.tj[i].pl + p.tj[i].tl - 1;
      p.fmax[i] = j.fmax0; p.rmax[i] = j.rmax0;
      p.s_begin[i] = j.resume_s;
      p.active[i] = (char)(p.fmax[i] + p.rmax[i] < A);  // jobs that were over before their first block stay where they are
      p.n_active += p.active[i];
      p.tj[i].s0 = j.resume_s; p.tj[i].active = p.active[i]; p.tj[i].fmax = p.fmax[i]; p.tj[i].rmax = p.rmax[i]; p.tj[i].nblocks = 0;
    }
  }
  return WFM_OK;
}

// The jobs that may not start this chunk (tile_job_leaves): they leave the tile phase here and the host runs them again
int drop_leavers(TilePhase& p) {
  wfm_handle* h = p.h;
  bool left = false;
  for (size_t i = 0; i < p.n; ++i) {
    const TileJob& t = p.tj[i];
    const BpJob& bj = p.jobs[(size_t)p.tiled[i]];
    // (a job under a hard limit of its score gets no block whose first score passes the limit: tile_job_beyond_limit)
    if (!p.active[i] || !(tile_job_leaves(t.pl, t.tl, t.sub, t.s0, bj.band, p.chunk, p.T) || tile_job_beyond_limit(t.pl, t.tl, t.sub, bj.limit, t.s0, p.T))) continue;
    p.active[i] = 0; p.tj[i].active = 0; p.tj[i].mode = 3; left = true; --p.n_active;
  }
  if (left) HIPCHK(h, hipMemcpyAsync(h->tilejobs.p, p.tj.data(), p.n * sizeof(TileJob), hipMemcpyHostToDevice, h->stream));
  return WFM_OK;
}

// The chunk's task list (plan_tile_chunk), built for the widest range the chunk can reach, onto the device
int plan_tile_tasks(TilePhase& p) {
  wfm_handle* h = p.h;
  for (size_t i = 0; i < p.n; ++i) {
    const TileJob& t = p.tj[i];
    p.pjobs[i] = TilePlanJob{t.pl, t.tl, t.sub, t.s0, t.mode, t.fine_s, t.packed, p.active[i]};
  }
  plan_tile_chunk(p.pjobs.data(), p.n, p.rules, p.plan, p.dirs.data());
  const std::vector<TileTask>& tasks = p.plan.tasks;
  if (tasks.empty()) { h->err = "tile phase: active jobs without a tile"; return WFM_E_HIP; }
  if (h->tiletasks.ensure(tasks.size())) { h->err = "out of device memory (tile tasks)"; return WFM_E_NOMEM; }
  HIPCHK(h, hipMemcpyAsync(h->tiletasks.p, tasks.data(), tasks.size() * sizeof(TileTask), hipMemcpyHostToDevice, h->stream));
  return WFM_OK;
}

// Behind the chunk's last advance kernel: the snapshot every keeping job will stand at if it simply moves on, where that score is one of the
// cadence -- the directions the job has computed from score 0 itself, each into rows of the store.  A job that did not get there keeps nothing
// (the kernel checks; settle_keeps gives the rows back).
int launch_keeps(TilePhase& p) {
  wfm_handle* h = p.h;
  p.ktasks.clear(); p.kids.clear();
  if (!p.ru || p.ru->cadence <= 0) return WFM_OK;
  ReuseCtl& ru = *p.ru;
  int max_n = 0;
  for (size_t i = 0; i < p.n && ru.cadence > 0; ++i) {
    const TileJob& t = p.tj[i];
    const int64_t es = (int64_t)t.s0 + (int64_t)p.chunk * p.T;
    if (!p.active[i] || t.mode != 0 || es > ru.upto[i] || es < (int64_t)ru.min_blocks * p.T || es % ((int64_t)ru.cadence * p.T) != 0) continue;
    if (!reuse_keep_wanted((int)es, ru.meet[i] > 0 ? ru.meet[i] : reuse_meet_estimate(t.s0, (int64_t)p.fmax[i] + p.rmax[i], t.pl + t.tl - 1), ru.cadence, p.T)) continue;
    for (int d = 0; d < 2; ++d) {
      if (!((p.own[i] >> d) & 1)) continue;
      KeptRows kr;
      kr.s0 = (int32_t)es; kr.kmin = reuse_keep_kmin(t.pl, (int)es); kr.n = reuse_keep_cols(t.pl, t.tl, (int)es);
      kr.pl = t.pl; kr.tl = t.tl; kr.sub = t.sub;
      kr.d = ru.store->take(reuse_keep_elems(t.pl, t.tl, (int)es), &kr.slab);
      if (!kr.d) {  // the store is full: half as many keeps from here on (the ones held stay)
        ru.cadence = ru.cadence * 2 <= (1 << 20) ? ru.cadence * 2 : 0;
        break;
      }
      ru.store->v.push_back(kr);
      p.kids.push_back((int32_t)ru.store->v.size());
      p.ktasks.push_back(KeepTask{kr.d, (int32_t)i, d, kr.s0, kr.kmin, kr.n, 0});
      max_n = std::max(max_n, kr.n);
      ru.keep_bytes += 2ull * 4ull * (uint64_t)KEEP_ROWS * (uint64_t)kr.n;
    }
  }
  if (p.ktasks.empty()) return WFM_OK;
  if (h->keeptasks.ensure(p.ktasks.size())) { h->err = "out of device memory (keeps)"; return WFM_E_NOMEM; }
  HIPCHK(h, hipMemcpyAsync(h->keeptasks.p, p.ktasks.data(), p.ktasks.size() * sizeof(KeepTask), hipMemcpyHostToDevice, h->stream));
  launch_keep(h->ring.p, h->tilejobs.p, h->keeptasks.p, (int)p.ktasks.size(), max_n, h->stream);
  HIPCHK(h, hipGetLastError());
  return WFM_OK;
}

// The keeps the chunk really wrote (the job stands where the host expected it), with the direction's running maximum there
void settle_keeps(TilePhase& p) {
  for (size_t q = 0; q < p.ktasks.size(); ++q) {
    const KeepTask& kt = p.ktasks[q];
    const TileJob& t = p.tj[(size_t)kt.job];
    if (t.active && t.mode == 0 && t.s0 == kt.expect_s) {
      p.ru->store->v[(size_t)p.kids[q] - 1].mx = kt.dir == 0 ? t.fmax : t.rmax;
      p.ru->kept[kt.dir][(size_t)kt.job].push_back(p.kids[q]);
      p.h->tile_ctr[WFM_TC_REUSE_KEEPS] += 1;
    } else p.ru->store->drop(p.kids[q]);
  }
  p.ktasks.clear(); p.kids.clear();
}

// At a look of the host: the jobs that wait for their keep and stand at its score take it (wfa_restore_kernel: the rows into the outer direction's
// planes of ring_in, the touch flag, the direction's maximum over the job's own rows) and are tiled jobs like the others from here on -- unless a
// kept cell touches the job's box, or the maxima fired while one direction stood still, or the job meets in the very block after the restore
// (whose input holds no gap rows as deep as a short run up to the meeting point hands on): those give the keep up (reuse_fall_back).
int restore_kept(TilePhase& p) {
  wfm_handle* h = p.h;
  if (!p.ru) return WFM_OK;
  ReuseCtl& ru = *p.ru;
  bool changed = false;
  p.rtasks.clear();
  int max_n = 0;
  for (size_t i = 0; i < p.n; ++i) {
    const TileJob& t = p.tj[i];
    if (p.resumed_at[i] > 0) {  // took its keep at the last look or the one before
      if (t.s0 > p.resumed_at[i]) p.resumed_at[i] = -1;
      else if (!t.active || t.mode != 0) { reuse_fall_back(p, i); changed = true; }
      continue;
    }
    if (p.dirs[i] == 3 || ru.bad[i]) continue;
    const ReuseUse& u = ru.use[i];
    if (!t.active || t.mode != 0 || t.s0 > u.s_k || (u.s_k - t.s0) % (p.chunk * p.T) != 0) { reuse_fall_back(p, i); changed = true; continue; }
    if (t.s0 < u.s_k) continue;
    const KeptRows& kr = ru.store->v[(size_t)u.keep - 1];
    p.rtasks.push_back(RestoreTask{kr.d, (int32_t)i, u.dir, u.s_k, kr.kmin, kr.n, ru.slack});
    max_n = std::max(max_n, kr.n);
    ru.restore_bytes += 2ull * 4ull * (uint64_t)KEEP_ROWS * (uint64_t)kr.n;
  }
  if (!p.rtasks.empty()) {
    p.rres.assign(p.rtasks.size() * 2, 0);
    if (h->restoretasks.ensure(p.rtasks.size()) || h->restoreres.ensure(p.rres.size())) { h->err = "out of device memory (keeps)"; return WFM_E_NOMEM; }
    HIPCHK(h, hipMemcpyAsync(h->restoretasks.p, p.rtasks.data(), p.rtasks.size() * sizeof(RestoreTask), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->restoreres.p, 0, p.rres.size() * sizeof(int32_t), h->stream));
    launch_restore(h->ring.p, h->tilejobs.p, h->restoretasks.p, h->restoreres.p, (int)p.rtasks.size(), max_n, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(p.rres.data(), h->restoreres.p, p.rres.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t q = 0; q < p.rtasks.size(); ++q) {
      const size_t i = (size_t)p.rtasks[q].job;
      changed = true;
      if (p.rres[2 * q]) { reuse_fall_back(p, i, true); continue; }  // a kept cell touches the job's box
      const ReuseUse& u = ru.use[i];
      (u.dir == 0 ? p.fmax[i] : p.rmax[i]) = p.rres[2 * q + 1];
      p.tj[i].fmax = p.fmax[i]; p.tj[i].rmax = p.rmax[i];
      p.tj[i].prev_ok = 0;  // (ring_prev holds one direction's rows only)
      p.dirs[i] = 3; p.resumed_at[i] = u.s_k;
      ru.store->drop(u.keep);
      h->tile_ctr[WFM_TC_REUSE_RESUMED] += 1;
    }
  }
  if (changed) HIPCHK(h, hipMemcpyAsync(h->tilejobs.p, p.tj.data(), p.n * sizeof(TileJob), hipMemcpyHostToDevice, h->stream));
  return WFM_OK;
}

// The chunk's blocks, each a launch of the tile kernels and the tiny kernel that replays the termination checks; the jobs' state back
int launch_chunk(TilePhase& p) {
  wfm_handle* h = p.h;
  wfm_seqset* S = p.S;
  const TileCfg& cfg = p.cfg;
  const int T = p.T;
  const std::vector<TileTask>& tasks = p.plan.tasks;
  const size_t n_pk = p.plan.n_pk;
  const std::vector<int>&threads_b = p.plan.threads_b, &variants_b = p.plan.variants_b;
  const size_t lds = ((size_t)(p.scope + 2 * (p.dp.e1 + 1) + 2 * (p.dp.e2 + 1)) * cfg.Wt + T + 1) * 4;
  for (int b = 0; b < p.chunk; ++b) {
    HIPCHK(h, hipEventRecord(h->tile_ev[2 * b], h->stream));
    if (cfg.reg) {
      if (n_pk) {
        launch_tile2(S->d_pk, h->ring.p, h->tilejobs.p, h->tiletasks.p, h->tilemak.p, (int)n_pk, threads_b[(size_t)b], T, variants_b[(size_t)b], h->stream);
        h->tile_ctr[WFM_TC_BLOCKS_COARSE] += (variants_b[(size_t)b] & 1) != 0;
        h->tile_ctr[WFM_TC_BLOCKS_FINE] += (variants_b[(size_t)b] & 2) != 0;
        p.launches_coarse += (variants_b[(size_t)b] & 1) != 0; p.launches_fine += (variants_b[(size_t)b] & 2) != 0;
      }
      if (tasks.size() > n_pk)
        launch_tile_reg(S->d_seq, h->ring.p, h->tilejobs.p, h->tiletasks.p + n_pk, h->tilemak.p, (int)(tasks.size() - n_pk), threads_b[(size_t)b], T, cfg.C, p.any_cut, h->stream);
    } else launch_tile(S->d_seq, h->ring.p, h->tilejobs.p, h->tiletasks.p, h->tilemak.p, (int)tasks.size(), cfg.threads, T, cfg.Wt, lds, p.dp, p.scope, ring_rows_for(p.scope), h->stream);
    HIPCHK(h, hipEventRecord(h->tile_ev[2 * b + 1], h->stream));
    launch_tile_advance(h->tilejobs.p, h->tilemak.p, (int)p.n, T, p.dp, (cfg.reg && cfg.exact) ? 1 : 0, p.rules.coarse_on ? 1 : 0, variants_b[(size_t)b], h->stream);
  }
  HIPCHK(h, hipGetLastError());
  const int rc = launch_keeps(p);
  if (rc != WFM_OK) return rc;
  HIPCHK(h, hipMemcpyAsync(p.got.data(), h->tilejobs.p, p.n * sizeof(TileJob), hipMemcpyDeviceToHost, h->stream));
  return WFM_OK;
}

// The device time of the chunk's blocks, and what was launched
int time_chunk(TilePhase& p) {
  wfm_handle* h = p.h;
  const size_t ntasks = p.plan.tasks.size();
  for (int b = 0; b < p.chunk; ++b) {
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->tile_ev[2 * b], h->tile_ev[2 * b + 1]));
    p.tile_ms += ms;
    if (h->call_base) {
      float t0 = 0;
      HIPCHK(h, hipEventElapsedTime(&t0, h->call_base, h->tile_ev[2 * b]));
      h->tile_iv.emplace_back(t0, t0 + ms);
    }
  }
  p.blocks += (uint32_t)p.chunk;
  for (int b = 0; b < p.chunk; ++b) p.lane_cells += (double)ntasks * p.plan.threads_b[(size_t)b] * p.cfg.C * p.T;
  h->stats.tile_launches += (uint32_t)p.chunk;
  h->stats.tile_tasks += (uint32_t)(ntasks * (size_t)p.chunk);
  return WFM_OK;
}

// The cells of the blocks every job ran since the last look, and the jobs as the chunk left them
void account_chunk(TilePhase& p) {
  wfm_handle* h = p.h;
  const int T = p.T;
  p.n_active = 0;
  for (size_t i = 0; i < p.n; ++i) {
    const TileJob& was = p.tj[i];
    const TileJob& got = p.got[i];
    // cells of the blocks this job ran since the last look (the block that found the meeting point included)
    for (int bl = was.nblocks; bl < got.nblocks; ++bl) {
      const bool last_exact = got.mode == 2 && bl == got.nblocks - 1;    // the block that stopped at the meeting point
      // it re-ran the block before it -- unless the job came with its planned end: no block of it ran twice
      const int base = p.s_begin[i] + ((last_exact && got.plan_sum <= 0) ? bl - 1 : bl) * T;
      for (int d = 0; d < 2; ++d) {
        if (!((p.dirs[i] >> d) & 1)) continue;  // (a direction that waits for its keep had no tiles)
        const int steps = last_exact ? (d == 0 ? got.tf : got.tr) : T;
        p.tile_cells += (uint64_t)cells_sum(was.pl, was.tl, was.sub, base + 1, base + steps);
      }
    }
    if (got.fine_s == -1 && was.fine_s != -1) {  // the block in which the directions met ran once more, for its per-score maxima (TileJob::fine_s)
      for (int d = 0; d < 2; ++d) if ((p.dirs[i] >> d) & 1) p.tile_cells += (uint64_t)cells_sum(was.pl, was.tl, was.sub, got.s0 + 1, got.s0 + T);
      h->tile_ctr[WFM_TC_FINE_RERUNS] += 1;
      p.reruns5 += 1;
    }
    if (got.reran > was.reran) {  // the block before the meeting block ran once more, for its gap rows (TileJob::ring_prev)
      for (int d = 0; d < 2; ++d) if ((p.dirs[i] >> d) & 1) p.tile_cells += (uint64_t)cells_sum(was.pl, was.tl, was.sub, got.s0 - T + 1, got.s0);
      h->tile_ctr[WFM_TC_GAP_RERUNS] += (uint64_t)(got.reran - was.reran);
      p.reruns6 += (uint32_t)(got.reran - was.reran);
    }
    p.tj[i] = got;
    p.active[i] = (char)(got.active != 0);
    p.fmax[i] = got.fmax; p.rmax[i] = got.rmax;
    p.n_active += p.active[i];
  }
}

// The jobs back into their BpJobs, positioned at the last snapshot for what follows; the cells that went into the result
void hand_back(TilePhase& p, uint32_t level, double cells_before) {
  wfm_handle* h = p.h;
  // cells that went into the result: both directions up to where the tile phase leaves the job (the full block in which
  // the wavefronts met was computed as well, and then again up to the meeting point: tile_cells counts it, this does not)
  uint64_t unique_level = 0;
  for (size_t i = 0; i < p.n; ++i) {
    const TileJob& t = p.tj[i];
    const int sf_end = t.mode == 2 ? t.s0 + t.tf : t.s0, sr_end = t.mode == 2 ? t.s0 + t.tr : t.s0;
    if (p.ru && p.ru->bad[i]) continue;  // (gave its keep up: what it computed goes into no result)
    // (the rows a direction took from a keep are in the job's result as its own would be: they count here, where cells_tile -- the cells
    // the tile kernels computed -- leaves them out)
    unique_level += (uint64_t)cells_sum(t.pl, t.tl, t.sub, p.s_begin[i] + 1, sf_end) + (uint64_t)cells_sum(t.pl, t.tl, t.sub, p.s_begin[i] + 1, sr_end);
  }
  h->stats.cells_tile_unique += unique_level;
  for (size_t i = 0; i < p.n; ++i) {
    const TileJob& t = p.tj[i];
    BpJob& j = p.jobs[(size_t)p.tiled[i]];
    j.ring_off = t.ring_in;
    p.ring2[i] = t.ring_out;
    j.resume_s = t.s0;
    j.resume_sr = -1; j.last_fwd = 0;
    h->tile_ctr[WFM_TC_EXACT_ENDS] += t.mode == 2;
    h->tile_ctr[WFM_TC_PLANNED_ENDS] += t.mode == 2 && t.plan_sum > 0;
    h->tile_ctr[WFM_TC_LEFT_BAND] += t.mode == 3 && !(p.ru && p.ru->bad[i]);
    if (t.mode == 3) {  // ran out of its band: wfa_bp_kernel reports WFM_DEV_BAND
      // (where it stands, for the host: a job that goes on from this snapshot on a wider ring resumes at resume_sr with these maxima)
      j.resume_s = -3; j.resume_sr = t.s0; j.fmax0 = p.fmax[i]; j.rmax0 = p.rmax[i];
      continue;
    }
    if (t.mode == 2) {  // stopped exactly at the meeting point: the step kernel goes straight to phase 2
      j.resume_s = t.s0 + t.tf;
      j.resume_sr = t.s0 + t.tr;
      j.last_fwd = t.last_fwd;
    }
    j.fmax0 = p.fmax[i]; j.rmax0 = p.rmax[i];
  }
  if (p.cfg.debug) fprintf(stderr, "[wfm] level %u: tiled %zu jobs, %u blocks of %d scores (Wt %d), %.3f ms; %.3e cells computed on %.3e lane-steps (%.0f %% of the lanes hold a cell), %.3e of them in the result (the block in which a job's wavefronts meet runs twice); launches of the packed kernel without / with per-score maxima %u / %u, mode-5 reruns %u, mode-6 reruns %u\n", level, p.n, p.blocks, p.T, p.cfg.Wt, p.tile_ms,
                           (double)p.tile_cells - cells_before, p.lane_cells, p.lane_cells > 0 ? 100.0 * ((double)p.tile_cells - cells_before) / p.lane_cells : 0.0, (double)unique_level,
                           p.launches_coarse, p.launches_fine, p.reruns5, p.reruns6);
}

// Advances the jobs listed in `tiled` (indices into jobs) in blocks of T scores with the
// time-tiled kernel until their forward/reverse antidiagonals meet inside a block; then
// leaves them positioned at the last snapshot for wfa_bp_kernel (resume_s/fmax0/rmax0/ring_off).
// With `refine` the jobs continue from where a coarser pass left them (blocks of T scores again, T smaller),
// so that the step-by-step kernel has at most the finer T steps to redo.
int run_tiled_phase(wfm_handle* h, wfm_seqset* S, const DevPen& dp, int scope, const TileCfg& cfg, int T, bool refine,
                    std::vector<BpJob>& jobs, const std::vector<int>& tiled, std::vector<int64_t>& ring2,
                    double& tile_ms, uint64_t& tile_cells, uint32_t level, const std::vector<int32_t>* fine_from = nullptr,
                    const std::vector<int64_t>* ring3 = nullptr, ReuseCtl* reuse = nullptr, const std::vector<int32_t>* plan_from = nullptr) {
  const size_t n = tiled.size();
  if (n == 0) return WFM_OK;
  const double cells_before = (double)tile_cells;
  TilePhase p{h, S, dp, scope, cfg, T, refine, jobs, tiled, ring2, tile_ms, tile_cells, n};
  p.ru = refine ? nullptr : reuse;
  int rc = init_tile_jobs(p, fine_from, ring3, plan_from);
  if (rc != WFM_OK) return rc;
  if (p.n_active) {
    // The per-job state lives on the device and a tiny kernel between two blocks replays the termination
    // checks, so the host only looks every `chunk` blocks.  The task list is built per chunk for the widest
    // range the chunk can reach; a block's tiles outside its current range, and all tiles of jobs that
    // finished earlier in the chunk, exit at once.
    HIPCHK(h, hipMemcpyAsync(h->tilejobs.p, p.tj.data(), n * sizeof(TileJob), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->tilemak.p, 0, n * 2 * (size_t)T * sizeof(int32_t), h->stream));
    p.chunk = std::max(1, std::min(cfg.chunk, (int)h->tile_ev.size() / 2));
    p.got.resize(n); p.pjobs.resize(n);
    p.rules = TilePlanRules{cfg.threads, cfg.C, T, p.chunk, cfg.Wt - 2 * T, cfg.reg, cfg.fine, cfg.reg && cfg.exact && tile2_coarse_maxima(), p.any_planned};
    auto clk = [] { return std::chrono::steady_clock::now(); };
    auto msd = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    double ms_prep = 0, ms_launch = 0, ms_wait = 0, ms_post = 0;
    while (p.n_active) {
      const auto tq0 = clk();
      if ((rc = drop_leavers(p)) != WFM_OK) return rc;
      if (!p.n_active) break;
      if ((rc = plan_tile_tasks(p)) != WFM_OK) return rc;
      const auto tq1 = clk();
      if ((rc = launch_chunk(p)) != WFM_OK) return rc;
      const auto tq2 = clk();
      HIPCHK(h, hipStreamSynchronize(h->stream));
      const auto tq3 = clk();
      if ((rc = time_chunk(p)) != WFM_OK) return rc;
      account_chunk(p);
      settle_keeps(p);
      if ((rc = restore_kept(p)) != WFM_OK) return rc;
      ms_prep += msd(tq0, tq1); ms_launch += msd(tq1, tq2); ms_wait += msd(tq2, tq3); ms_post += msd(tq3, clk());
    }
    if (cfg.debug > 1)
      fprintf(stderr, "[wfm] level %u tile phase, host side: task lists %.2f ms, launches %.2f ms, waiting for the device %.2f ms, bookkeeping %.2f ms\n", level, ms_prep, ms_launch, ms_wait, ms_post);
  }
  hand_back(p, level, cells_before);
  return WFM_OK;
}

// ---- phase 2 from rows computed ahead: run_p2_phase (at the end) is the loop over chunks of candidates, the stages before it do the work ----

// One call of run_p2_phase and the chunk at hand: the candidates i0 .. i0 + n, as many as the budget of the rows holds
struct P2Chunk {
  wfm_handle* h; wfm_seqset* S; const DevPen& dp; int scope; const TileCfg& cfg; std::vector<BpJob>& jobs;  // run_p2_phase's arguments
  const std::vector<int>& cand; const std::vector<int64_t>& ring_other; std::vector<BpResult>& res; double& ms_out;
  std::vector<BpResult>& carry; std::vector<char>& has_carry; bool may_continue; std::vector<int>& again;
  const std::vector<int32_t>& exact_of;  // per candidate: P2Job::exact (0: the job searches)
  std::vector<P2PlanJob> pcand;  // what plan_p2_chunk needs of every candidate
  std::vector<char> pexact;      // exact_of[i] > 0
  P2ChunkPlan plan;
  size_t i0 = 0, n = 0;
  std::vector<TileJob> tj;
  std::vector<P2Job> pj;
  // the order of the P2Jobs on the device: the jobs that search first (positions 0 .. ns), then the exact ones; at[q] is job q's position,
  // pj_dev[at[q]] = pj[q].  The maxima, wfa_p2_blockmax_kernel and wfa_p2_overlap_kernel are the search jobs' alone.
  std::vector<int> at;
  std::vector<P2Job> pj_dev;
  size_t ns = 0, ns_dump = 0;  // ns_dump: search jobs whose row maxima are still in p2max behind the launch (WFM_P2_DUMP)
  std::vector<BpResult> got;
  float ms = 0;
};

// The chunk that begins at candidate i0: its geometry and task list (plan_p2_chunk), its TileJobs (mode 4) and P2Jobs
void fill_p2_chunk(P2Chunk& c, size_t i0) {
  // the rows of a chunk of jobs may take a quarter of the budget (the rings hold the rest)
  const size_t budget = std::max<size_t>(c.h->mem_budget / 4, (size_t)64 << 20);
  plan_p2_chunk(c.pcand.data(), c.pcand.size(), i0, P2K, P2ROWS, budget, c.cfg.threads, c.cfg.Wt - 2 * P2K, c.plan, c.pexact.data());
  c.i0 = i0; c.n = c.plan.geo.size();
  c.tj.clear(); c.pj.clear();
  c.at.assign(c.n, 0); c.ns = 0;
  for (size_t q = 0; q < c.n; ++q) c.ns += !c.pexact[i0 + q];
  for (size_t q = 0, s = 0, e = c.ns; q < c.n; ++q) c.at[q] = (int)(c.pexact[i0 + q] ? e++ : s++);
  for (size_t q = 0; q < c.n; ++q) {
    const BpJob& j = c.jobs[(size_t)c.cand[i0 + q]];
    const P2Geometry& g = c.plan.geo[q];
    TileJob t = tile_job_from(j);
    t.ring_out = c.ring_other[i0 + q];
    t.mode = 4; t.tf = j.resume_s; t.tr = j.resume_sr; t.last_fwd = j.last_fwd;
    t.p2_off = (int64_t)g.p2_off; t.w2 = (int32_t)g.w2; t.koff2 = g.koff2;
    P2Job pq{};
    pq.ring_in = j.ring_off; pq.p2_off = (int64_t)g.p2_off; pq.width = j.width; pq.koff = j.koff; pq.w2 = (int32_t)g.w2; pq.koff2 = g.koff2;
    pq.pl = j.pl; pq.tl = j.tl; pq.sf = j.resume_s; pq.sr = j.resume_sr; pq.last_fwd = j.last_fwd; pq.sub = j.sub; pq.best0 = j.best0;
    pq.nblk = (int32_t)g.nblk; pq.bm_off = (int64_t)g.bm_off; pq.exact = c.exact_of[i0 + q];
    c.tj.push_back(t); c.pj.push_back(pq);
  }
  c.pj_dev.resize(c.n);
  for (size_t q = 0; q < c.n; ++q) c.pj_dev[(size_t)c.at[q]] = c.pj[q];
}

// The chunk on the device: the rows computed ahead, their maxima, the walk; the results back and the time it took
int launch_p2_chunk(P2Chunk& c) {
  wfm_handle* h = c.h;
  wfm_seqset* S = c.S;
  const size_t n = c.n, ns = c.ns, elems = c.plan.elems, bm_elems = c.plan.bm_elems, n_pk = c.plan.tiles.n_pk;
  const std::vector<TileTask>& tasks = c.plan.tiles.tasks;
  const int threads_c = c.plan.threads_c;
  if (h->p2rows.ensure(elems + 16) || h->p2max.ensure(ns * 2 * P2ROWS * 5) || h->p2bmax.ensure(bm_elems + 16) ||
      h->p2jobs.ensure(n) || h->tilejobs.ensure(n) || h->tiletasks.ensure(tasks.size()) || h->bpres.ensure(std::max(n, c.jobs.size()))) {
    h->err = "out of device memory (phase-2 rows)"; return WFM_E_NOMEM;
  }
  HIPCHK(h, hipMemcpyAsync(h->tilejobs.p, c.tj.data(), n * sizeof(TileJob), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->p2jobs.p, c.pj_dev.data(), n * sizeof(P2Job), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->tiletasks.p, tasks.data(), tasks.size() * sizeof(TileTask), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  bool any_cut = false;
  for (const TileJob& t : c.tj) any_cut |= t.sub != SUB_NONE;
  if (n_pk) launch_tile2_p2(S->d_pk, h->ring.p, h->tilejobs.p, h->tiletasks.p, (int)n_pk, threads_c, h->p2rows.p, h->stream);
  if (tasks.size() > n_pk) launch_tile_p2(S->d_seq, h->ring.p, h->tilejobs.p, h->tiletasks.p + n_pk, (int)(tasks.size() - n_pk), threads_c, h->p2rows.p, any_cut, h->stream);
  static const int p2_threads = getenv("WFM_P2_THREADS") ? atoi(getenv("WFM_P2_THREADS")) : 0;  // (a once-per-process switch: it stays static)
  static const int p2x_threads = getenv("WFM_P2_EXACT_THREADS") ? atoi(getenv("WFM_P2_EXACT_THREADS")) : 0;  // (likewise)
  // the jobs that search (positions 0 .. ns of p2jobs): their maxima, then the walk that prunes by them.  16 waves over the 5 x P2G (test, component) scans of a round and their rows
  auto launch_search = [&](size_t cnt) {
    launch_p2_blockmax(h->ring.p, h->p2rows.p, h->p2jobs.p, h->p2bmax.p, h->p2max.p, (int)cnt, h->stream);
    launch_p2_overlap(h->ring.p, h->p2rows.p, h->p2jobs.p, h->p2max.p, h->p2bmax.p, h->bpres.p, (int)cnt,
                      p2_threads > 0 ? p2_threads : 1024, (int)(c.plan.maxw2 >> 6) + 1, c.dp, c.scope, h->stream);
  };
  if (ns) launch_search(ns);
  // the exact jobs behind them: no maxima
  launch_p2_exact(h->ring.p, h->p2rows.p, h->p2jobs.p + ns, h->bpres.p + ns, (int)(n - ns), p2x_threads > 0 ? p2x_threads : p2_exact_threads(c.plan.maxw2), c.dp, c.scope, h->stream);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  std::vector<BpResult> dev(n);
  HIPCHK(h, hipMemcpyAsync(dev.data(), h->bpres.p, n * sizeof(BpResult), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipEventElapsedTime(&c.ms, h->ev0, h->ev1));
  auto note_busy = [&](float ms) {  // (between ev0 and ev1, as just recorded)
    if (!h->call_base) return hipSuccess;
    float t0 = 0;
    const hipError_t e = hipEventElapsedTime(&t0, h->call_base, h->ev0);
    if (e == hipSuccess) h->bp_iv.emplace_back(t0, t0 + ms);
    return e;
  };
  HIPCHK(h, note_busy(c.ms));
  c.got.resize(n);
  for (size_t q = 0; q < n; ++q) c.got[q] = dev[(size_t)c.at[q]];
  c.ns_dump = ns;
  h->tile_ctr[WFM_TC_P2_EXACT] += n - ns;
  // An exact job without a hit within its reach: once more from the same state as a job that searches (exact = 0, so this cannot come round
  // again), over the rows that are still there.  The maxima of the chunk's search jobs have been read; theirs take the buffers' front.
  std::vector<size_t> miss;
  for (size_t q = 0; q < n; ++q) if (c.got[q].status == WFM_DEV_P2_EXACT_MISS) miss.push_back(q);
  if (!miss.empty()) {
    h->tile_ctr[WFM_TC_P2_EXACT_MISSES] += miss.size();
    std::vector<P2Job> mj;
    size_t bm = 0;
    for (size_t q : miss) {
      P2Job& pq = c.pj[q];
      pq.exact = 0; pq.bm_off = (int64_t)bm;
      bm += (size_t)pq.nblk * 2 * P2ROWS * 5;
      mj.push_back(pq);
    }
    if (h->p2max.ensure(mj.size() * 2 * P2ROWS * 5) || h->p2bmax.ensure(bm + 16)) { h->err = "out of device memory (phase-2 maxima)"; return WFM_E_NOMEM; }
    HIPCHK(h, hipMemcpyAsync(h->p2jobs.p, mj.data(), mj.size() * sizeof(P2Job), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    launch_search(mj.size());
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipMemcpyAsync(dev.data(), h->bpres.p, mj.size() * sizeof(BpResult), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float ms2 = 0;
    HIPCHK(h, hipEventElapsedTime(&ms2, h->ev0, h->ev1));
    HIPCHK(h, note_busy(ms2));
    c.ms += ms2;
    for (size_t m = 0; m < miss.size(); ++m) c.got[miss[m]] = dev[m];
    c.ns_dump = 0;  // (the maxima at the buffers' front are no longer the chunk's search jobs')
  }
  c.ms_out += c.ms;
  return WFM_OK;
}

// WFM_P2_DUMP (diagnosis): the row maxima of one job of the chunk
int dump_p2_job(P2Chunk& c) {
  wfm_handle* h = c.h;
  const std::vector<BpResult>& got = c.got;
  // (only a job that searches has maxima: the one at position p2_dump among them, in the order of the device)
  if (c.ns_dump == 0) { fprintf(stderr, "[wfm] p2 dump: no job of this chunk of %zu searches with its row maxima at hand (%zu take the exact walk)\n", c.n, c.n - c.ns); return WFM_OK; }
  const size_t pos = std::min<size_t>((size_t)c.cfg.p2_dump, c.ns_dump - 1);
  size_t q = 0;
  while ((size_t)c.at[q] != pos) ++q;
  std::vector<int32_t> rm((size_t)2 * P2ROWS * 5);
  HIPCHK(h, hipMemcpy(rm.data(), h->p2max.p + pos * 2 * P2ROWS * 5, rm.size() * 4, hipMemcpyDeviceToHost));
  const P2Job& pjq = c.pj[q];
  fprintf(stderr, "[wfm] p2 dump job %zu: pl %d tl %d sf %d sr %d last_fwd %d sub %d w2 %d nblk %d -> status %d score %d (fwd %d rev %d comp %d k %d) rounds %d\n", q, pjq.pl, pjq.tl, pjq.sf,
          pjq.sr, pjq.last_fwd, pjq.sub, pjq.w2, pjq.nblk, got[q].status, got[q].score, got[q].score_fwd, got[q].score_rev, got[q].comp, got[q].k_fwd, got[q].pad_);
  for (int d = 0; d < 2; ++d)
    for (int r = 0; r < P2ROWS; r += 3) {
      const int32_t* m = rm.data() + ((size_t)d * P2ROWS + r) * 5;
      fprintf(stderr, "[wfm]   dir %d row %d (s = %d): max M %d I1 %d I2 %d D1 %d D2 %d\n", d, r, (d == 0 ? pjq.sf : pjq.sr) - RNG_BACK + r, m[0], m[1], m[2], m[3], m[4]);
    }
  return WFM_OK;
}

// WFM_DEBUG: the chunk's launch and its slowest walk
void print_p2_chunk(const P2Chunk& c) {
  const std::vector<BpResult>& got = c.got;
  const std::vector<P2Job>& pj = c.pj;
  const size_t n = c.n;
  int more = 0;
  double tk = 0, tc = 0, rd = 0; uint32_t tkmax = 0; int rdmax = 0;
  for (const BpResult& r : got) { more += r.status == WFM_DEV_P2_MORE; tk += r.ticks_p2; tc += r.ticks_p1; rd += r.pad_; tkmax = std::max(tkmax, r.ticks_p2); rdmax = std::max(rdmax, r.pad_); }
  double tests = 0; int tests_max = 0;  // the rows the walk went through behind the state it began at
  for (const BpResult& r : got) { tests += r.steps - r.steps_p1; tests_max = std::max(tests_max, r.steps - r.steps_p1); }
  size_t missed = 0;  // (a job that missed has searched since: pj[q].exact is 0 again, and it was not among the chunk's search jobs)
  for (size_t q = 0; q < n; ++q) missed += pj[q].exact == 0 && (size_t)c.at[q] >= c.ns;
  fprintf(stderr, "[wfm] phase 2 from rows computed ahead: %zu jobs, widest %zu columns, %zu tiles of %d threads, %.3f ms, %d left to the step kernel; walk per job: %.1f rounds (max %d), %.0f us (max %.0f), of which cells stage %.0f us; "
          "%.1f tests (max %d); exact walk %.1f %% of the jobs, missed %.1f %%\n",
          n, c.plan.maxw2, c.plan.tiles.tasks.size(), c.plan.threads_c, c.ms, more, rd / n, rdmax, tk / n / 100.0, tkmax / 100.0, tc / n / 100.0, tests / n, tests_max,
          100.0 * (n - c.ns) / n, 100.0 * missed / n);
  size_t qs = 0;
  for (size_t q = 0; q < n; ++q) if (got[q].ticks_p2 > got[qs].ticks_p2) qs = q;
  fprintf(stderr, "[wfm]   slowest walk: pl %d tl %d sub %d w2 %d nblk %d: %d rounds, %.0f us = listing %.0f + cells %.0f (incl. listing) + pick %.0f, %u blocks listed, status %d\n", pj[qs].pl, pj[qs].tl,
          pj[qs].sub == SUB_NONE ? -1 : pj[qs].sub, pj[qs].w2, pj[qs].nblk, got[qs].pad_, got[qs].ticks_p2 / 100.0, got[qs].ticks_list / 100.0, got[qs].ticks_p1 / 100.0, got[qs].ticks_pick / 100.0,
          got[qs].work_items, got[qs].status);
}

// Another round for the jobs whose walk ran out of rows (while their rings have room for its rows); the chunk's results into res
int continue_p2_chunk(P2Chunk& c) {
  wfm_handle* h = c.h;
  std::vector<BpResult>& got = c.got;
  std::vector<P2Job> mj;
  for (size_t q = 0; q < c.n; ++q) {
    const size_t jq = (size_t)c.cand[c.i0 + q];
    BpJob& j = c.jobs[jq];
    if (got[q].status == WFM_DEV_P2_NOTHING) { got[q] = c.carry[jq]; continue; }  // nothing better than what an earlier round found
    if (got[q].status != WFM_DEV_P2_MORE) continue;
    if (got[q].comp >= 0) {  // a breakpoint so far (better than the one handed in, if any)
      c.carry[jq] = got[q]; c.carry[jq].status = 0; c.has_carry[jq] = 1;
      j.best0 = got[q].score;
    }
    if (!c.may_continue || (j.band > 0 && std::max(j.resume_s, j.resume_sr) + 2 * P2K + 2 > j.band)) continue;  // wfa_bp_kernel goes on from here
    mj.push_back(c.pj[q]);
    j.resume_s += P2K; j.resume_sr += P2K;  // 2 * P2K tests: both directions P2K rows further, the same one stepped last
    c.again.push_back((int)(c.i0 + q));
  }
  if (!mj.empty()) {
    HIPCHK(h, hipMemcpyAsync(h->p2jobs.p, mj.data(), mj.size() * sizeof(P2Job), hipMemcpyHostToDevice, h->stream));
    launch_p2_to_ring(h->ring.p, h->p2rows.p, h->p2jobs.p, (int)mj.size(), h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));  // (mj is read by the copy above)
  }
  for (size_t q = 0; q < c.n; ++q) c.res[(size_t)c.cand[c.i0 + q]] = got[q];
  return WFM_OK;
}

// Phase 2 (overlap detection) of the jobs whose tile phase stopped exactly at the meeting point, without the
// step-by-step kernel: P2K more rows of both directions by the tile kernel, all rows kept (P2Job in wfa_device.h), then
// the reference's loop with only the tests left in it (wfa_p2_overlap_kernel).  cand: indices into jobs; res[q] is filled for every
// candidate, with status WFM_DEV_P2_MORE where the loop had not ended after 2 * P2K tests (wfa_bp_kernel takes those).
// A job whose walk ran out of rows goes another round when `may_continue`: its last RING rows of both directions are copied
// from the P2 rows into its ring (wfa_p2_to_ring_kernel) -- the state the sequential loop is in after 2 * P2K tests -- the
// breakpoint found so far is kept in carry[] and handed on as BpJob::best0, and the job's position in cand is appended to
// `again`.  (On divergent records a few jobs per level take 120 - 230 tests from the first touch of the wavefronts to a shared
// diagonal; finishing them step by step in wfa_bp_kernel was half of C2's device time.)
int run_p2_phase(wfm_handle* h, wfm_seqset* S, const DevPen& dp, int scope, const TileCfg& cfg, std::vector<BpJob>& jobs,
                 const std::vector<int>& cand, const std::vector<int64_t>& ring_other, std::vector<BpResult>& res, double& ms_out,
                 std::vector<BpResult>& carry, std::vector<char>& has_carry, bool may_continue, std::vector<int>& again, const std::vector<int32_t>& exact_of) {
  if (cand.empty()) return WFM_OK;
  P2Chunk c{h, S, dp, scope, cfg, jobs, cand, ring_other, res, ms_out, carry, has_carry, may_continue, again, exact_of};
  for (size_t i = 0; i < cand.size(); ++i) {
    const BpJob& j = jobs[(size_t)cand[i]];
    c.pcand.push_back(P2PlanJob{j.pl, j.tl, j.sub, j.resume_s, j.resume_sr, j.packed});
    c.pexact.push_back((char)(exact_of[i] > 0));
  }
  for (size_t i0 = 0; i0 < cand.size(); i0 += c.n) {
    fill_p2_chunk(c, i0);
    int rc = launch_p2_chunk(c);
    if (rc != WFM_OK) return rc;
    if (cfg.p2_dump_on && (rc = dump_p2_job(c)) != WFM_OK) return rc;
    h->stats.p2_launches++;
    h->stats.p2_jobs += (uint32_t)c.n;
    if (cfg.debug) print_p2_chunk(c);
    if ((rc = continue_p2_chunk(c)) != WFM_OK) return rc;
  }
  return WFM_OK;
}

// ---- the BiWFA level driver: align_resident_impl (at the end) is the loop over levels and chunks, the stages before it do the work ----

// The call's switches, read from the environment once per call (not once per process: the tests run both forms of most of them in
// one process).  tile_cfg() reads the tile kernels' own.
struct Knobs {
  static int num(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
  bool use_hints = num("WFM_SCORE_HINT", 1) != 0;
  bool use_bound = use_hints && num("WFM_BOUND", 1) != 0;
  int slack_env = num("WFM_SUB_SLACK", -1);  // tests: < 0 default, >= 2^28 none
  bool ring3_on = num("WFM_TILE_RING3", 1) != 0, p2_on = num("WFM_P2", 1) != 0;
  bool p2_exact = num("WFM_P2_EXACT", 1) != 0;  // 0: every job of phase 2 searches (wfa_p2_overlap_kernel), also the ones that stand at their own score (P2Job::exact)
  int p2_rounds = std::max(1, num("WFM_P2_ROUNDS", 64));
  int fine_margin = num("WFM_TILE_FINE_MARGIN", 48);
  int coarse_min_blocks = num("WFM_TILE_COARSE_MIN_BLOCKS", 32), coarse_max_jobs = num("WFM_TILE_COARSE_MAX_JOBS", 128);
  // a job whose score is known ends phase 1 at the state planned from it (wfa_plan.h, planned_meet) instead of searching for its meeting point;
  // not in the unbounded configuration of the tests (children without their parents' scores)
  bool planned_end = num("WFM_TILE_PLANNED_END", 1) != 0 && slack_env < (1 << 28);
  bool tile_v2 = num("WFM_TILE_V2", 1) != 0;  // 0: every tile on the byte kernel (wfa_tile_reg_kernel) -- the A/B switch of the packed kernel (wfa_tile2.hip)
  bool band_on = num("WFM_BAND", 1) != 0;
  int band_root = std::max(64, num("WFM_BAND_ROOT", 4096));
  int resume_margin = num("WFM_RESUME_MARGIN", SNAP_ROWS);  // (tests: a large value sends every resumed job back to score 0)
  // parent reuse (wfa_plan.h): 0 = no job keeps, no child resumes; blocks between two keeps; how close to its box a kept cell may come (tests: a
  // large value makes every resume fall back); the levels whose jobs keep (1: the roots alone, the children of deeper jobs start at score 0; 8 is
  // what was measured: C3 56.9 - 57.4 ms a step with the roots' keeps, 56.1 - 56.2 with every level's, profiles/parent_reuse.md section 4)
  bool reuse = num("WFM_REUSE", 1) != 0 && slack_env < (1 << 28);  // (children without their parents' scores may not resume: nobody keeps for them)
  int reuse_min_blocks = std::max(1, num("WFM_REUSE_MIN_BLOCKS", 8));  // a keep, and a resume, fewer blocks deep is not worth its look of the host (C2, the scaled C4 rank)
  int reuse_every = std::max(1, num("WFM_REUSE_EVERY", 2)), reuse_slack = std::max(0, num("WFM_REUSE_TOUCH_SLACK", 0));  // (never below 0: that would switch the check off and let a restored row hold offsets outside the job's box)
  int reuse_levels = num("WFM_REUSE_LEVELS", 8);
  int debug = env_debug();  // 0: unset
};

// One chunk of a level: the breakpoint jobs whose rings share the arena, and what the stages hand on about them
struct Chunk {
  std::vector<BpJob> jobs;
  std::vector<int32_t> node_of;    // the job's node in bp_nodes
  size_t ring_elems = 0, end = 0;  // elements of the chunk's rings; the first node behind the chunk
  int maxw = 0;
  std::vector<int> tiled, tiled_r;  // jobs of the tile phase (indices into jobs); _r: those that go on from a snapshot.  Their second and third rings, their fine_s:
  std::vector<int64_t> ring2, ring3, ring2_r;
  std::vector<int32_t> fine_from, fine_r, snap_r;
  std::vector<int32_t> plan_from;  // per entry of `tiled`: sf + sr of the planned end the job takes (TileJob::plan_sum), 0: it searches
  std::vector<size_t> ring_third;  // elements of one ring of every tiled job of the chunk
  std::vector<char> grown_job, resume_bad, has_carry;
  // parent reuse, per entry of `tiled` (plan_chunk): the keep the job resumes from, the last score it keeps at for its own children;
  // per job (run_chunk_tiles): it gave its keep up, the keeps it wrote per direction
  std::vector<ReuseUse> reuse;
  std::vector<int32_t> keep_upto;
  std::vector<char> reuse_bad;
  std::vector<std::vector<int32_t>> kept[2];
  std::vector<BpResult> res, carry;  // carry: breakpoints found by rounds of phase 2 that did not end the walk
  std::vector<int> rest, more_set;   // rest: jobs for the step kernel -- not tiled, not exact, or not finished by the rows computed ahead
  void clear() {
    jobs.clear(); node_of.clear(); ring_elems = 0; maxw = 0;
    tiled.clear(); ring2.clear(); ring3.clear(); ring_third.clear(); fine_from.clear();
    tiled_r.clear(); ring2_r.clear(); fine_r.clear(); snap_r.clear(); grown_job.clear();
    reuse.clear(); keep_upto.clear(); plan_from.clear();
  }
};

// The state of one align call, handed from stage to stage
struct AlignCall {
  wfm_handle* h;
  const wfm_penalties_t* pen;
  wfm_seqset* S;
  size_t first, last;
  wfm_result_t* out;
  char* ops_arena;
  size_t arena_bytes, arena_base;
  std::vector<uint32_t>* runs_out;
  uint32_t* pflags;
  int scope;
  DevPen dp;
  const Knobs knobs;
  TileCfg tcfg;
  BaseCfg bcfg;
  int RR;           // rows of every ring of this call
  RingRules rules;  // what plan_ring decides by: the call's, the level's (use_band, over_budget) and roots_off
  std::vector<int32_t> prob_status;  // indexed by problem id
  std::vector<uint64_t> prob_cells;
  std::vector<int32_t> prob_score;   // score-only problems: the score, taken where the device first knows it (a root's meeting point, a base job's forward pass)
  std::vector<Node> bp_nodes, base_nodes, next_bp;
  uint32_t level = 0;
  Chunk ck;
  LevelTimer tm;
  double wall_tile = 0, wall_base = 0;
  uint64_t band_retries = 0, band_jobs = 0, roots_banded = 0, roots_out = 0, hint_retries = 0, limit_out = 0;
  // Rings that grow with the score: a job whose full ring does not fit the budget runs on bands b, 4 b, 16 b ...
  uint64_t grown_jobs = 0, grown_widened = 0, grown_restarts = 0;
  int64_t grown_maxband = 0;
  size_t ring_peak = 0;  // most elements a chunk's ring arena held
  GrownSnaps snaps;
  KeepStore keeps;       // parent reuse: the rows jobs keep for their children
  uint64_t reuse_children = 0, reuse_found = 0, reuse_taken = 0;  // children of keeping jobs; that found a keep; that were let run from it
  uint64_t keep_bytes = 0, restore_bytes = 0;
  uint64_t reuse_full_rings = 0;  // nodes that got a full ring in place of a narrow one to run from their keep
};

void make_roots(AlignCall& c) {
  for (size_t i = c.first; i < c.last; ++i) {
    const ProbMeta& pm = c.S->meta[i];
    Node nd{};
    nd.prob = (int32_t)i; nd.pb = 0; nd.pl = pm.plen; nd.tb = 0; nd.tl = pm.tlen;
    nd.cb = C_M; nd.ce = C_M; nd.score_rem = INT_MAX; nd.endsfree = 0;
    nd.sub = SUB_NONE; nd.hinted = 0;
    if (c.pflags && (pm.mode == WFM_MODE_END2END_BIWFA || pm.mode == WFM_MODE_ENDSFREE) && !((size_t)i < c.S->acgt.size() && c.S->acgt[i])) c.pflags[i] |= WFM_PF_BYTE_KERNEL;
    if (c.knobs.use_hints && pm.hint > 0 && pm.mode == WFM_MODE_END2END_BIWFA) { nd.sub = pm.hint; nd.hinted = 1; }
    // a hard limit of the score is the root's bound whatever the switches say about guesses (bound_roots may still lower it: its bound is rigorous)
    if (pm.limit > 0) { nd.limit = pm.limit; nd.sub = pm.limit; nd.hinted = 1; }
    int64_t bound = (int64_t)gapcost(*c.pen, pm.plen) + gapcost(*c.pen, pm.tlen) + 8;
    if (pm.limit > 0 && (pm.plen == 0 || pm.tlen == 0) && bound - 8 > pm.limit) { c.prob_status[i] = WFM_ST_MAX_SCORE; continue; }  // (the all-gap jobs have no budget to overflow)
    if (pm.limit > 0) bound = std::min<int64_t>(bound, pm.limit);  // a limited short problem's base job: the limit is its budget, its overflow final
    if (pm.mode == WFM_MODE_ENDSFREE) {
      nd.endsfree = 1;
      // ends-free score is bounded by the cheaper all-gap alignment; start small, double on overflow
      nd.smax = (int32_t)std::min<int64_t>(bound, 256);
      c.base_nodes.push_back(nd);
    } else if (pm.mode == WFM_MODE_END2END_UNI || std::max(pm.plen, pm.tlen) <= BIALIGN_FALLBACK_MIN_LENGTH ||
               pm.plen == 0 || pm.tlen == 0) {
      nd.smax = (int32_t)std::min<int64_t>(bound, 256);
      c.base_nodes.push_back(nd);
    } else {
      c.bp_nodes.push_back(nd);
    }
  }
}

// An upper bound of every long root's score, from one greedy walk per root (wfa_bound_kernel): rigorous, so the root's
// wavefronts are cut to what an alignment of at most that score can touch -- usually a fifth of what the caller's guess
// leaves.  The guess stays where the walk gives up (divergent records, structural differences).
int bound_roots(AlignCall& c) {
  wfm_handle* h = c.h;
  std::vector<BoundJob> bj;
  std::vector<size_t> owner;
  if (c.knobs.use_bound)
    for (size_t q = 0; q < c.bp_nodes.size(); ++q) {
      const Node& nd = c.bp_nodes[q];
      const ProbMeta& pm = c.S->meta[nd.prob];
      // only where a bound can bind: the end diagonal far from the start diagonal (see BpJob::sub below)
      if (pm.mode != WFM_MODE_END2END_BIWFA || std::min(nd.pl, nd.tl) < 1024 || std::abs(nd.tl - nd.pl) < 64) continue;
      bj.push_back(BoundJob{pm.p_fwd, pm.t_fwd, nd.pl, nd.tl});
      owner.push_back(q);
    }
  if (bj.empty()) return WFM_OK;
  uint64_t bounded_roots = 0, bound_gain = 0;
  const auto tb0 = std::chrono::steady_clock::now();
  if (h->bndjobs.ensure(bj.size()) || h->bndres.ensure(bj.size())) { h->err = "out of device memory (score bounds)"; return WFM_E_NOMEM; }
  HIPCHK(h, hipMemcpyAsync(h->bndjobs.p, bj.data(), bj.size() * sizeof(BoundJob), hipMemcpyHostToDevice, h->stream));
  launch_bound(c.S->d_seq, h->bndjobs.p, h->bndres.p, (int)bj.size(), c.dp, h->stream);
  HIPCHK(h, hipGetLastError());
  std::vector<int32_t> ub(bj.size());
  HIPCHK(h, hipMemcpyAsync(ub.data(), h->bndres.p, bj.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (size_t q = 0; q < bj.size(); ++q) {
    if (ub[q] < 0) continue;
    Node& nd = c.bp_nodes[owner[q]];
    if (nd.sub == SUB_NONE || ub[q] < nd.sub) {
      if (nd.sub != SUB_NONE) bound_gain += (uint64_t)(nd.sub - ub[q]);
      nd.sub = ub[q];
      nd.hinted = 1;  // (cannot fail; the retry of a root that runs past its bound stays as the safety net it is)
      ++bounded_roots;
    }
  }
  const double bound_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count();
  if (c.knobs.debug)
    fprintf(stderr, "[wfm] score bounds: %zu roots walked in %.2f ms, %llu bounded (on average %.0f below the caller's guess)\n", bj.size(), bound_ms,
            (unsigned long long)bounded_roots, bounded_roots ? (double)bound_gain / (double)bounded_roots : 0.0);
  return WFM_OK;
}

// Rings cover every diagonal of a job ((pl + tl) columns of 1280 B, twice for tiled jobs): fine for a batch of
// few deep problems, wasteful for thousands of long low-divergence records, whose wavefronts stay within a few
// thousand diagonals and which would otherwise be worked off in many small chunks.  When the level does not fit
// the budget, jobs get rings for |k| <= band only: a child's total score is known (half of it per direction,
// plus the overlap phase), a root gets WFM_BAND_ROOT scores; whoever runs out of its band is run again on a
// full ring.  WFM_BAND=0 switches this off.
void level_budget(AlignCall& c) {
  size_t total = 0;
  for (const Node& nd : c.bp_nodes) total += ring_elems(ring_full_width(nd.pl, nd.tl), c.RR, 2);
  // (narrow rings whenever full ones would take more than 2 GB, not only when they would not fit: every fresh GB of a
  // first hipMalloc costs ~30 ms on this driver, scripts/micro/malloc_cost2.hip, and a one-shot run pays it)
  c.rules.use_band = c.knobs.band_on && total * 4 > std::min<size_t>(c.h->mem_budget, (size_t)2 << 30);
  c.rules.over_budget = total * 4 > c.h->mem_budget;
}

// The jobs of the chunk that begins at node i0: a ring for each (plan_ring), until the chunk's byte limit is reached
void plan_chunk(AlignCall& c, size_t i0) {
  wfm_handle* h = c.h;
  Chunk& k = c.ck;
  const TileCfg& tcfg = c.tcfg;
  // (once per process)
  static const size_t ring_chunk_bytes = (size_t)(getenv("WFM_RING_CHUNK_GB") ? std::max(1, atoi(getenv("WFM_RING_CHUNK_GB"))) : 4) << 30;
  k.clear();
  size_t i = i0;
  int64_t fine_min_blocks_r = INT64_MAX;
  int64_t fine_min_blocks = INT64_MAX;  // fewest blocks any tiled job of the chunk is expected to run before its directions meet
  for (; i < c.bp_nodes.size(); ++i) {
    const Node& nd = c.bp_nodes[i];
    const ProbMeta& pm = c.S->meta[nd.prob];
    RingPlan rp = plan_ring(nd, c.rules);
    // the bound the job's rows are cut to (set into the job below)
    // (under a hard limit always: the limit has to stop the job wherever its end diagonal lies)
    const int32_t job_sub = (nd.sub != SUB_NONE && (nd.limit > 0 || (int64_t)std::abs(nd.tl - nd.pl) * 8 >= (int64_t)nd.sub)) ? nd.sub : SUB_NONE;
    const bool reuse_on = c.knobs.reuse && tcfg.reg && tcfg.exact && c.RR == RING;
    if (nd.keep > 0 && reuse_on && rp.fits && rp.band > 0 && !rp.grown) {
      // A node that came with a keep takes it on a full ring only (a narrow one is out of parent reuse's scope).  Where the level chose a narrow
      // one it gets the full one instead -- its parent ran on rings twice as wide in this arena -- but only if it will then really run from the keep:
      // eligibility is decided on the full ring's plan first, and a node that fails it keeps the ring it would have had (and loses the keep below)
      RingRules full = c.rules;
      full.use_band = false;
      const RingPlan fp = plan_ring(nd, full);
      const KeptRows& kr = c.keeps.v[(size_t)nd.keep - 1];
      if (kr.d && kr.s0 % (tcfg.chunk * tcfg.T) == 0 && reuse_eligible(nd, fp, kr.pl, kr.tl, kr.sub, job_sub, kr.s0, tcfg.T)) { rp = fp; ++c.reuse_full_rings; }
    }
    if (!rp.fits) { c.prob_status[nd.prob] = WFM_ST_OOM; c.snaps.drop(nd.snap); c.keeps.drop(nd.keep); continue; }
    const size_t width = rp.width, need = rp.need; const int band = rp.band; const bool tile_it = rp.tile_it, grown = rp.grown;
    // (a chunk of a level stops at 4 GB of rings even when the budget allows more: hundreds of jobs fill the device
    // long before that, and every GB of a first allocation costs 30 - 70 ms.  C1 substitute, three handles in a fresh
    // process: 8 GB chunks 8.3 s cold / 5.33 s warm, 4 GB 5.67 / 5.52, 2 GB 6.22 / 6.06 -- scripts/c1_cold.sh.  A chunk of
    // fewer than 128 jobs may grow to 8 GB: C3's 21 roots of a part are 5.4 GB of full rings, and cut in two they fill the device worse.
    // Tried and dropped: two launches per block, jobs without a score bound apart from those with one -- the plain kernel form
    // has 7 % fewer instructions, the second launch cost more: C2 0.18 -> 0.21 s, C1 no better)
    if (!k.jobs.empty() && (k.ring_elems + need) * 4 > std::min<size_t>(h->mem_budget, k.jobs.size() >= 128 ? ring_chunk_bytes : std::max(ring_chunk_bytes, (size_t)8 << 30))) break;
    BpJob j{};
    j.p_fwd = pm.p_fwd + nd.pb;
    j.t_fwd = pm.t_fwd + nd.tb;
    j.p_rev = pm.p_rev + (pm.plen - nd.pb - nd.pl);
    j.t_rev = pm.t_rev + (pm.tlen - nd.tb - nd.tl);
    j.ring_off = (int64_t)k.ring_elems;
    j.pl = nd.pl; j.tl = nd.tl;
    j.comp_begin = nd.cb; j.comp_end = nd.ce;
    j.width = (int32_t)width;
    j.koff = rp.koff;
    j.resume_s = -1; j.resume_sr = -1; j.last_fwd = 0; j.fmax0 = 0; j.rmax0 = 0;
    j.band = band;
    // a bound only earns its keep when the end diagonal is far from the start diagonal relative to the score (padded
    // records and their children): for a balanced problem it starts to bind where the wavefronts meet, and costs the
    // tile kernel its bookkeeping all the way there
    j.sub = job_sub;
    j.limit = nd.limit;
    j.best0 = 0;
    j.packed = (c.knobs.tile_v2 && tcfg.reg && tcfg.C == 2 && (size_t)nd.prob < c.S->acgt.size() && c.S->acgt[(size_t)nd.prob]) ? 1 : 0;
    // bit 1: near-identical sequences -- the job's score is known (a child's, a bounded or hinted root's) to be under a sixteenth of its length; the packed
    // tile kernel then hands a lone long run to the whole wave at once (wfa_tile2.hip, tail_direct).  Whether the bound also CUTS the rows (sub below) is another matter.
    if (j.packed && nd.sub != SUB_NONE && (int64_t)nd.sub * 16 < (int64_t)nd.pl + nd.tl) j.packed |= 2;
    c.band_jobs += band > 0 && !grown;
    k.grown_job.push_back((char)grown);
    const bool resumes = grown && tile_it && nd.snap > 0;  // (a snapshot is the tile kernels' own: no gap rows as deep as the step kernel reads)
    if (nd.snap > 0 && !resumes) c.snaps.drop(nd.snap);
    if (grown) {
      ++c.grown_jobs;
      c.grown_maxband = std::max<int64_t>(c.grown_maxband, band);
      if (resumes) ++c.grown_widened; else if (nd.noband || nd.band > 0) ++c.grown_restarts;
      if (c.pflags) c.pflags[nd.prob] |= WFM_PF_RING_GROWN;
      if (c.knobs.debug)
        fprintf(stderr, "[wfm] grown ring: problem %d, %s of %d x %d: band %d, %zu columns on the %s%s\n", nd.prob, nd.score_rem == INT_MAX ? "root" : "child", nd.pl, nd.tl, band, width,
                tile_it ? "tile kernels" : "step kernel alone", resumes ? ", widened from its snapshot" : ((nd.noband || nd.band > 0) ? ", from score 0 again" : ""));
    }
    if (resumes) {
      // the job's rule for per-score maxima is the one it started with (below); its blocks until the directions meet are counted from the snapshot
      const GrownSnap& sn = c.snaps.v[(size_t)nd.snap - 1];
      k.tiled_r.push_back((int)k.jobs.size()); k.ring2_r.push_back((int64_t)(k.ring_elems + need / 2)); k.snap_r.push_back(nd.snap);
      const int64_t est = nd.score_rem != INT_MAX ? (int64_t)nd.score_rem : (int64_t)nd.pl + nd.tl;
      fine_min_blocks_r = std::min<int64_t>(fine_min_blocks_r, std::max<int64_t>(0, est / 2 - sn.s0) / tcfg.T);
      k.fine_r.push_back(nd.score_rem != INT_MAX ? std::max(0, nd.score_rem / 2 - c.knobs.fine_margin) : INT_MAX);
    } else if (tile_it) {
      k.tiled.push_back((int)k.jobs.size()); k.ring2.push_back((int64_t)(k.ring_elems + need / 2)); k.ring_third.push_back(need / 2);
      // per-score maxima from here on (TileJob::fine_s): a child's directions meet near half its score (the trigger -- the sum of the two largest
      // antidiagonals -- can fire a little earlier, never later); a root's score is anybody's guess: it finds its meeting block with one maximum
      // per block and runs it again (whether the chunk uses any of this is decided below, once its jobs are known)
      const int64_t est = nd.score_rem != INT_MAX ? (int64_t)nd.score_rem : (nd.sub != SUB_NONE ? (int64_t)nd.sub : (int64_t)nd.pl + nd.tl);  // its score / the guess or bound / the worst case
      fine_min_blocks = std::min<int64_t>(fine_min_blocks, est / 2 / tcfg.T);
      k.fine_from.push_back(nd.score_rem != INT_MAX ? std::max(0, nd.score_rem / 2 - c.knobs.fine_margin) : INT_MAX);
      // parent reuse: the keep the node came with, if it may run from it; the scores it keeps at itself
      ReuseUse use;
      if (nd.keep > 0 && reuse_on) {
        const KeptRows& kr = c.keeps.v[(size_t)nd.keep - 1];
        if (kr.d && kr.s0 % (tcfg.chunk * tcfg.T) == 0 && reuse_eligible(nd, rp, kr.pl, kr.tl, kr.sub, j.sub, kr.s0, tcfg.T)) { use.keep = nd.keep; use.dir = nd.keep_dir; use.s_k = kr.s0; ++c.reuse_taken; }
      }
      if (nd.keep > 0 && use.keep == 0) c.keeps.drop(nd.keep);
      k.reuse.push_back(use);
      // the planned end (wfa_plan.h): a job that knows its score, on the packed kernel, on a ring no budget shaped, ends phase 1 where its score says
      const bool planned = c.knobs.planned_end && tcfg.reg && tcfg.exact && c.RR == RING &&
                           planned_meet_eligible(nd, rp, (j.packed & 1) != 0, use.keep > 0 ? use.s_k : 0, tcfg.T);
      k.plan_from.push_back(planned ? nd.meet : 0);
      // (no keep beyond the score a child could still resume at: a child's score is at most its parent's, which is at most the bound where one is known)
      int32_t upto = 0;
      // (a score-only root has no children: nobody would resume from its keeps)
      if (reuse_on && band == 0 && !grown && (int)c.level <= c.knobs.reuse_levels && !(nd.score_rem == INT_MAX && pm.score_only())) {
        const int known = nd.score_rem != INT_MAX ? nd.score_rem : (nd.sub != SUB_NONE ? nd.sub : INT_MAX);
        // (the two directions meet at scores a step apart: a child has half the job's score, give or take the rows the overlap phase reads)
        upto = known != INT_MAX ? std::max(0, reuse_resume_limit(known / 2 + 2 * SNAP_ROWS, tcfg.T, c.knobs.fine_margin)) : INT_MAX;
      }
      k.keep_upto.push_back(upto);
    } else c.keeps.drop(nd.keep);
    if (resumes) c.keeps.drop(nd.keep);
    k.node_of.push_back((int32_t)i);
    k.ring_elems += need;
    // widest wavefront this job can reach: 2 diagonals per score of one direction (~half the total score)
    const int64_t est_w = nd.score_rem == INT_MAX ? (int64_t)width : std::min<int64_t>((int64_t)width, (int64_t)nd.score_rem + 128);
    k.maxw = std::max(k.maxw, (int)est_w);
    k.jobs.push_back(j);
  }
  k.end = i;
  // One maximum per block instead of one per score (TileJob::fine_s) pays where a launch is a few deep jobs that move in step -- C3: 21 roots
  // of 78 blocks each, -3.7 % per step -- and costs where it is hundreds of jobs of all depths: their blocks need both instantiations of the
  // kernel side by side (two launches per block), and a root runs its meeting block a third time behind one more look of the host: C2 +10 %
  // device time, the scaled C4 rank +3 % (gpurun_out/r6r/ab2.log).  So: only chunks of at most coarse_max_jobs jobs, every one of them
  // at least coarse_min_blocks blocks deep; everybody else keeps the per-score maxima from the first block on (one launch per block, as before).
  if (k.tiled.size() > (size_t)c.knobs.coarse_max_jobs || fine_min_blocks < (int64_t)c.knobs.coarse_min_blocks) std::fill(k.fine_from.begin(), k.fine_from.end(), 0);
  if (k.tiled_r.size() > (size_t)c.knobs.coarse_max_jobs || fine_min_blocks_r < (int64_t)c.knobs.coarse_min_blocks) std::fill(k.fine_r.begin(), k.fine_r.end(), 0);
  // (a job with a planned end reads no maxima score by score: where the chunk launches the instantiation without them it never counts for the
  // other one; in a chunk that keeps per-score maxima from the first block on it rides along in that one launch per block, at the same price)
  for (size_t q = 0; q < k.tiled.size(); ++q) if (k.plan_from[q] > 0 && k.fine_from[q] > 0) k.fine_from[q] = INT_MAX;
  // third rings behind the chunk's rings (TileJob::ring_prev), for all of its tiled jobs or for none: where half as much again still fits the
  // budget (and 12 GB: fresh memory is 30 ms per GB).  The chunk's composition does not depend on it.
  size_t third = 0;
  for (size_t x : k.ring_third) third += x;
  const bool give = c.knobs.ring3_on && tcfg.reg && tcfg.exact && third > 0 && (k.ring_elems + third) * 4 <= std::min<size_t>(h->mem_budget, (size_t)12 << 30);
  k.ring3.assign(k.tiled.size(), -1);
  if (give)
    for (size_t q = 0; q < k.tiled.size(); ++q) { k.ring3[q] = (int64_t)k.ring_elems; k.ring_elems += k.ring_third[q]; }
}

// The chunk's arena; then the snapshots of the jobs that go on where they stood, out of their blocks into the chunk's (wider)
// rings; the blocks go back
int widen_resumed(AlignCall& c) {
  wfm_handle* h = c.h;
  Chunk& k = c.ck;
  if (h->ring.ensure(k.ring_elems + 16) || h->bpjobs.ensure(k.jobs.size()) || h->bpres.ensure(k.jobs.size())) {
    h->err = "out of device memory (ring arena)"; return WFM_E_NOMEM;
  }
  c.ring_peak = std::max(c.ring_peak, k.ring_elems);
  k.resume_bad.assign(k.jobs.size(), 0);
  if (k.tiled_r.empty()) return WFM_OK;
  std::vector<RingWidenJob> wj;
  int maxw_dst = 0;
  for (size_t q = 0; q < k.tiled_r.size(); ++q) {
    BpJob& j = k.jobs[(size_t)k.tiled_r[q]];
    const GrownSnap& sn = c.snaps.v[(size_t)k.snap_r[q] - 1];
    wj.push_back(RingWidenJob{sn.d, h->ring.p + j.ring_off, sn.w, sn.koff, j.width, j.koff, -(sn.s0 + 8), sn.s0 + 8});
    maxw_dst = std::max(maxw_dst, j.width);
    j.resume_s = sn.s0; j.resume_sr = -1; j.fmax0 = sn.fmax; j.rmax0 = sn.rmax;
  }
  if (h->widenjobs.ensure(wj.size())) { h->err = "out of device memory (ring arena)"; return WFM_E_NOMEM; }
  HIPCHK(h, hipMemcpyAsync(h->widenjobs.p, wj.data(), wj.size() * sizeof(RingWidenJob), hipMemcpyHostToDevice, h->stream));
  launch_ring_widen(h->widenjobs.p, (int)wj.size(), maxw_dst, c.RR, h->stream);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int32_t id : k.snap_r) c.snaps.drop(id);
  return WFM_OK;
}

// The tile phase of the chunk: its tiled jobs, the optional finer pass, then the resumed jobs from their snapshots
int run_chunk_tiles(AlignCall& c) {
  wfm_handle* h = c.h;
  Chunk& k = c.ck;
  const TileCfg& tcfg = c.tcfg;
  double tms = 0; uint64_t tcells = 0;
  const auto tw0 = std::chrono::steady_clock::now();
  // parent reuse: the cadence under the store's cap -- an eighth of the part's budget -- from what the chunk's jobs would keep; a root whose score nobody
  // knows is guessed to meet within a sixteenth of its bases (its keeps stop where it ends; should the store fill up all the same, launch_keeps thins them)
  ReuseCtl ru;
  ru.store = &c.keeps; ru.slack = c.knobs.reuse_slack; ru.min_blocks = c.knobs.reuse_min_blocks;
  ru.use = k.reuse; ru.upto = k.keep_upto;
  for (size_t q = 0; q < k.tiled.size(); ++q) {
    const Node& nd = c.bp_nodes[(size_t)k.node_of[(size_t)k.tiled[q]]];
    ru.meet.push_back(nd.score_rem != INT_MAX ? nd.score_rem / 2 : 0);
  }
  {
    std::vector<ReuseKeeper> kp;
    for (size_t q = 0; q < k.tiled.size(); ++q) {
      const BpJob& j = k.jobs[(size_t)k.tiled[q]];
      if (k.keep_upto[q] > 0) kp.push_back(ReuseKeeper{j.pl, j.tl, k.keep_upto[q] == INT_MAX ? (j.pl + j.tl) / 16 : k.keep_upto[q]});
    }
    c.keeps.cap_bytes = h->mem_budget / 8;
    const int chunk_blocks = std::max(1, std::min(tcfg.chunk, (int)h->tile_ev.size() / 2));
    ru.cadence = kp.empty() ? 0 : reuse_fit_cadence(kp.data(), kp.size(), reuse_cadence(c.knobs.reuse_every, chunk_blocks), tcfg.T, c.keeps.cap_bytes);
  }
  const bool any_reuse = ru.cadence > 0 || std::any_of(ru.use.begin(), ru.use.end(), [](const ReuseUse& u) { return u.keep > 0; });
  int rc = run_tiled_phase(h, c.S, c.dp, c.scope, tcfg, tcfg.T, false, k.jobs, k.tiled, k.ring2, tms, tcells, c.level, &k.fine_from, &k.ring3, any_reuse ? &ru : nullptr, &k.plan_from);
  k.reuse_bad.assign(k.jobs.size(), 0);
  k.kept[0].assign(k.jobs.size(), {}); k.kept[1].assign(k.jobs.size(), {});
  if (any_reuse && !ru.bad.empty())
    for (size_t q = 0; q < k.tiled.size(); ++q) {
      k.reuse_bad[(size_t)k.tiled[q]] = ru.bad[q];
      for (int d = 0; d < 2; ++d) k.kept[d][(size_t)k.tiled[q]].swap(ru.kept[d][q]);
    }
  c.keep_bytes += ru.keep_bytes; c.restore_bytes += ru.restore_bytes;
  if (rc == WFM_OK && tcfg.T_refine > 0 && tcfg.T_refine < tcfg.T && !(tcfg.reg && tcfg.exact))
    rc = run_tiled_phase(h, c.S, c.dp, c.scope, tcfg, tcfg.T_refine, true, k.jobs, k.tiled, k.ring2, tms, tcells, c.level);
  if (rc == WFM_OK && !k.tiled_r.empty()) {
    std::vector<int> from_s(k.tiled_r.size());
    for (size_t q = 0; q < k.tiled_r.size(); ++q) from_s[q] = k.jobs[(size_t)k.tiled_r[q]].resume_s;
    rc = run_tiled_phase(h, c.S, c.dp, c.scope, tcfg, tcfg.T, true, k.jobs, k.tiled_r, k.ring2_r, tms, tcells, c.level, &k.fine_r);
    for (size_t q = 0; rc == WFM_OK && q < k.tiled_r.size(); ++q) {
      BpJob& j = k.jobs[(size_t)k.tiled_r[q]];
      // The snapshot a job goes on from was written by a block of the tile kernels for the next block of the tile kernels: with a third ring
      // in play (TileJob::ring_prev) it holds the gap components two rows and one row deep, not the 26 the overlap phase and the step kernel
      // read.  A job whose directions meet within 26 scores of that snapshot would hand such rows on: it starts again on this band instead
      // (26 scores out of the thousands the wider ring was made for).
      const bool exact_end = j.resume_s >= 0 && j.resume_sr >= 0;
      if (tcfg.reg && tcfg.exact && ((exact_end && std::min(j.resume_s, j.resume_sr) - from_s[q] < c.knobs.resume_margin) || (j.resume_s >= 0 && j.resume_sr < 0 && j.resume_s == from_s[q]))) {
        j.resume_s = -3; j.resume_sr = -1;
        k.resume_bad[(size_t)k.tiled_r[q]] = 1;
      }
      k.tiled.push_back(k.tiled_r[q]); k.ring2.push_back(k.ring2_r[q]);  // (from here on a tiled job like the others)
    }
  }
  c.wall_tile += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count();
  if (rc != WFM_OK) return rc;
  c.tm.bp_ms += tms; c.tm.tile_ms += tms;
  h->stats.cells_bp += tcells; h->stats.cells_tile += tcells;
  return WFM_OK;
}

// Phase 2 of the jobs the tile phase left exactly at their meeting point: rows computed ahead + scan + replay.  Leaves the
// step kernel's jobs in rest.
int run_chunk_p2(AlignCall& c) {
  wfm_handle* h = c.h;
  Chunk& k = c.ck;
  k.res.assign(k.jobs.size(), BpResult{});
  k.rest.clear(); k.more_set.clear();
  std::vector<int> cand;
  std::vector<int64_t> other;
  std::vector<int32_t> exact_of;  // per candidate: P2Job::exact in the first round of rows (a later round starts behind the planned end: it searches)
  std::vector<char> is_cand(k.jobs.size(), 0);
  if (c.knobs.p2_on && c.tcfg.reg && c.tcfg.exact)
    for (size_t q = 0; q < k.tiled.size(); ++q) {
      const BpJob& j = k.jobs[(size_t)k.tiled[q]];
      if (j.resume_s >= 0 && j.resume_sr >= 0) {
        cand.push_back(k.tiled[q]); other.push_back(k.ring2[q]); is_cand[(size_t)k.tiled[q]] = 1;
        // the exact walk (P2Job::exact): the job left the tile phase at its planned end, the state whose scores sum to its own score (only jobs
        // on the packed kernel, on a ring no budget shaped, with their bound are planned: plan_chunk).  The pick's order is the reference's under
        // o2 >= o1 >= 0 (wfa_p2_overlap_kernel); other penalties search.  (A job that resumed on a wider ring sits behind plan_from's end.)
        const bool exact = c.knobs.p2_exact && q < k.plan_from.size() && k.plan_from[q] > 0 && j.resume_s + j.resume_sr == k.plan_from[q] && j.best0 == 0 &&
                           c.dp.o2 >= c.dp.o1 && c.dp.o1 >= 0;
        exact_of.push_back(exact ? k.plan_from[q] : 0);
      }
    }
  double pms = 0;
  k.carry.assign(k.jobs.size(), BpResult{});
  k.has_carry.assign(k.jobs.size(), 0);
  std::vector<int> cand_r = cand, again;
  std::vector<int64_t> other_r = other;
  for (int round = 1; !cand_r.empty(); ++round) {
    again.clear();
    if (round > 1) exact_of.assign(cand_r.size(), 0);
    const int rc = run_p2_phase(h, c.S, c.dp, c.scope, c.tcfg, k.jobs, cand_r, other_r, k.res, pms, k.carry, k.has_carry, round < c.knobs.p2_rounds, again, exact_of);
    if (rc != WFM_OK) return rc;
    std::vector<int> c2; std::vector<int64_t> o2;
    for (int a : again) {
      c2.push_back(cand_r[(size_t)a]); o2.push_back(other_r[(size_t)a]);
      if (c.pflags) c.pflags[c.bp_nodes[(size_t)k.node_of[(size_t)cand_r[(size_t)a]]].prob] |= WFM_PF_P2_ROUNDS;
    }
    h->stats.p2_again += (uint32_t)again.size();
    cand_r.swap(c2); other_r.swap(o2);
  }
  c.tm.bp_ms += pms;
  for (size_t q = 0; q < k.jobs.size(); ++q)
    if (!is_cand[q] || k.res[q].status == WFM_DEV_P2_MORE) { k.rest.push_back((int)q); h->stats.p2_more += is_cand[q]; if (is_cand[q]) k.more_set.push_back((int)q); }
  if (c.pflags)  // jobs whose overlap walk went past the first round of rows computed ahead (or was finished by the step kernel)
    for (size_t q = 0; q < k.jobs.size(); ++q)
      if (is_cand[q] && k.res[q].status == WFM_DEV_P2_MORE) c.pflags[c.bp_nodes[(size_t)k.node_of[q]].prob] |= WFM_PF_P2_ROUNDS;
  return WFM_OK;
}

// The step kernel (wfa_bp_kernel) for the jobs in rest
int run_chunk_step(AlignCall& c) {
  wfm_handle* h = c.h;
  Chunk& k = c.ck;
  const std::vector<int>& rest = k.rest;
  if (rest.empty()) return WFM_OK;
  auto is_more = [&](int q) { return std::find(k.more_set.begin(), k.more_set.end(), q) != k.more_set.end(); };
  // workgroup size: wide wavefronts want all 16 waves of a CU
  int threads = 1024;
  if (k.maxw <= 1024) threads = 256;
  else if (k.maxw <= 8192) threads = 512;
  std::vector<BpJob> rj(rest.size());
  for (size_t q = 0; q < rest.size(); ++q) rj[q] = k.jobs[(size_t)rest[q]];
  HIPCHK(h, hipMemcpyAsync(h->bpjobs.p, rj.data(), rj.size() * sizeof(BpJob), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  launch_bp(c.S->d_seq, h->ring.p, h->bpjobs.p, h->bpres.p, (int)rj.size(), threads, c.dp, c.scope, c.RR, h->stream);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  std::vector<BpResult> rr(rj.size());
  HIPCHK(h, hipMemcpyAsync(rr.data(), h->bpres.p, rr.size() * sizeof(BpResult), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  c.tm.bp_ms += ms;
  if (h->call_base) {
    float t0 = 0;
    HIPCHK(h, hipEventElapsedTime(&t0, h->call_base, h->ev0));
    h->bp_iv.emplace_back(t0, t0 + ms);
  }
  h->stats.bp_launches++;
  for (size_t q = 0; q < rest.size(); ++q) {
    if (rr[q].status == WFM_DEV_P2_NOTHING) {  // (only jobs that carry a breakpoint are handed a best0)
      const uint64_t cl = rr[q].cells; const int32_t st = rr[q].steps;
      rr[q] = k.carry[(size_t)rest[q]]; rr[q].cells = cl; rr[q].steps = st;
    }
    k.res[(size_t)rest[q]] = rr[q];
  }
  if (c.knobs.debug) {
    uint64_t cl = 0; double t1 = 0, t2 = 0; int64_t st1 = 0, st = 0; uint32_t m1 = 0, m2 = 0;
    for (const BpResult& r : rr) { cl += r.cells; t1 += r.ticks_p1; t2 += r.ticks_p2; st1 += r.steps_p1; st += r.steps; m1 = std::max(m1, r.ticks_p1); m2 = std::max(m2, r.ticks_p2); }
    fprintf(stderr, "[wfm] level %u: %zu bp jobs (step kernel), %d thr, %.3f ms, cells %.3e, avg steps p1 %.0f p2 %.0f, avg ms p1 %.3f p2 %.3f, max ms p1 %.3f p2 %.3f\n", c.level, rr.size(), threads, ms,
            (double)cl, (double)st1 / rr.size(), (double)(st - st1) / rr.size(), t1 / rr.size() / 1e5, t2 / rr.size() / 1e5, m1 / 1e5, m2 / 1e5);
    if (c.knobs.debug > 1) {  // the slowest three
      std::vector<size_t> ord(rr.size());
      for (size_t q = 0; q < ord.size(); ++q) ord[q] = q;
      std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return rr[a].ticks_p1 + rr[a].ticks_p2 > rr[b].ticks_p1 + rr[b].ticks_p2; });
      for (size_t q = 0; q < std::min<size_t>(3, ord.size()); ++q) {
        const BpResult& r = rr[ord[q]];
        const BpJob& j = rj[ord[q]];
        fprintf(stderr, "[wfm]   slow step-kernel job: pl %d tl %d width %d band %d sub %d resume %d/%d (%s), status %d score %d = %d + %d, steps p1 %d p2 %d, ms p1 %.3f p2 %.3f\n", j.pl, j.tl, j.width,
                j.band, j.sub == SUB_NONE ? -1 : j.sub, j.resume_s, j.resume_sr, is_more(rest[ord[q]]) ? "phase-2 walk ran out of rows" : (j.resume_sr >= 0 ? "exact" : "not exact"), r.status,
                r.score, r.score_fwd, r.score_rev, r.steps_p1, r.steps - r.steps_p1, r.ticks_p1 / 1e5, r.ticks_p2 / 1e5);
      }
    }
  }
  return WFM_OK;
}

// A tiled job that simply ran out of its band stands at a block boundary s0 <= band with both directions complete -- a row of score s
// spans |k| <= s, nothing was cut by the ring's edge -- and goes on from there: the columns |k| <= s0 + 8 of its snapshot wait in a block of
// their own for the job's wider ring (the chunk's arena is the next chunk's).  Not so a job under a bound of its score (rows cut to
// |k - (tl - pl)| <= sub - s: no state of the unbounded problem) or one the step kernel stopped: those start again from score 0.
int keep_snapshot(AlignCall& c, size_t q, Node& again) {
  wfm_handle* h = c.h;
  const BpJob& j = c.ck.jobs[q];
  if (c.ck.resume_bad[q] || c.ck.res[q].status != WFM_DEV_BAND || j.resume_s != -3 || j.resume_sr < 0 || j.sub != SUB_NONE || j.band <= 0) return WFM_OK;
  GrownSnap sn;
  sn.s0 = j.resume_sr; sn.fmax = j.fmax0; sn.rmax = j.rmax0;
  const int reach = sn.s0 + 8;
  sn.koff = reach + 4;
  sn.koff += ((j.koff - sn.koff) % 4 + 4) % 4;  // whole 16-byte chunks apart from the ring's columns, and from those of the ring to come
  sn.w = (sn.koff + reach + 5 + 3) & ~3;
  if (wfm_dmalloc((void**)&sn.d, ring_elems((size_t)sn.w, c.RR) * sizeof(int32_t)) != hipSuccess) { (void)hipGetLastError(); sn.d = nullptr; }
  if (!sn.d) return WFM_OK;  // (no block to be had: the job starts again)
  const RingWidenJob wj{h->ring.p + j.ring_off, sn.d, j.width, j.koff, sn.w, sn.koff, -reach, reach};
  c.snaps.v.push_back(sn);
  again.snap = (int32_t)c.snaps.v.size();
  if (h->widenjobs.ensure(1)) { h->err = "out of device memory (ring arena)"; return WFM_E_NOMEM; }
  HIPCHK(h, hipMemcpyAsync(h->widenjobs.p, &wj, sizeof(wj), hipMemcpyHostToDevice, h->stream));
  launch_ring_widen(h->widenjobs.p, 1, sn.w, c.RR, h->stream);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return WFM_OK;
}

// The two halves of a job on either side of its breakpoint: leaves to the base aligner, the others to the next level
void push_children(AlignCall& c, const Node& nd, const BpResult& r, int bp_v, int bp_h, size_t q) {
  const wfm_penalties_t* pen = c.pen;
  Node a{}, b{};
  a.prob = nd.prob; a.pb = nd.pb; a.pl = bp_v; a.tb = nd.tb; a.tl = bp_h;
  // what a child can cost: the score its parent found for it, plus the opening of a gap it begins or ends in
  // (counted on the other side of the breakpoint)
  const int slack = c.knobs.slack_env >= 0 ? c.knobs.slack_env : 2 * std::max(pen->o1, pen->o2) + 8;
  a.sub = (int)std::min<int64_t>((int64_t)r.score_fwd + slack, SUB_NONE);
  b.sub = (int)std::min<int64_t>((int64_t)r.score_rev + slack, SUB_NONE);
  a.hinted = 0; b.hinted = 0;
  a.cb = nd.cb; a.ce = r.comp; a.score_rem = r.score_fwd;
  b.prob = nd.prob; b.pb = nd.pb + bp_v; b.pl = nd.pl - bp_v; b.tb = nd.tb + bp_h; b.tl = nd.tl - bp_h;
  b.cb = r.comp; b.ce = nd.ce; b.score_rem = r.score_rev;
  // where phase 1 of either may end without a search (Node::meet; whether the job takes it is plan_chunk's decision)
  a.meet = planned_meet_sum(a.score_rem, *pen, a.cb, a.ce, false);
  b.meet = planned_meet_sum(b.score_rem, *pen, b.cb, b.ce, true);
  for (Node* ch : {&a, &b}) {
    if (ch->pl == 0 || ch->tl == 0) { ch->smax = 0; c.base_nodes.push_back(*ch); }
    else if (ch->score_rem <= BIALIGN_FALLBACK_MIN_SCORE) {
      // the leaf's own forward score: what the breakpoint credited it with, plus the opening of a gap it has
      // to end in (counted on the other side of that breakpoint)
      const int open_end = ch->ce == C_M ? 0 : ((ch->ce == C_I1 || ch->ce == C_D1) ? pen->o1 : pen->o2);
      ch->smax = std::max(ch->score_rem, 0) + open_end;
      c.base_nodes.push_back(*ch);
    }
    else {
      // parent reuse: the first child's forward direction starts where the job's did, the second child's reverse direction where its reverse
      // one did -- the newest of the job's keeps of that direction the child may still resume at goes with it
      const int d = ch == &a ? 0 : 1;
      std::vector<int32_t>& kept = c.ck.kept[d][q];
      if (!kept.empty()) {
        ++c.reuse_children;
        std::vector<int32_t> kept_s(kept.size());
        for (size_t x = 0; x < kept.size(); ++x) kept_s[x] = c.keeps.v[(size_t)kept[x] - 1].s0;
        const int pick = ch->sub != SUB_NONE ? reuse_pick_keep(kept_s.data(), kept_s.size(), ch->score_rem, c.tcfg.T, c.knobs.fine_margin, c.knobs.reuse_min_blocks) : -1;
        if (pick >= 0) { ch->keep = kept[(size_t)pick]; ch->keep_dir = d; kept[(size_t)pick] = 0; ++c.reuse_found; }
      }
      c.next_bp.push_back(*ch);
    }
  }
}

// diagnosis (WFM_DUMP_FAIL): the whole problem's sequences, for a replay
void dump_failed_problem(AlignCall& c, const Node& nd, const char* dd) {
  const ProbMeta& pm = c.S->meta[nd.prob];
  std::vector<char> pb((size_t)pm.plen), tb((size_t)pm.tlen);
  (void)hipMemcpy(pb.data(), c.S->d_seq + pm.p_fwd, pb.size(), hipMemcpyDeviceToHost);
  (void)hipMemcpy(tb.data(), c.S->d_seq + pm.t_fwd, tb.size(), hipMemcpyDeviceToHost);
  static std::atomic<int> nfail{0};
  const std::string fn = std::string(dd) + "/fail_" + std::to_string(nfail.fetch_add(1)) + ".txt";
  if (FILE* f = fopen(fn.c_str(), "w")) {
    fprintf(f, "%d %d %d\n", pm.plen, pm.tlen, pm.hint);
    fwrite(pb.data(), 1, pb.size(), f); fputc('\n', f);
    fwrite(tb.data(), 1, tb.size(), f); fputc('\n', f);
    fclose(f);
  }
}

// What became of the chunk's jobs: run again (with a snapshot where one can be kept), children, a leaf, or the problem's failure
int settle_chunk(AlignCall& c) {
  wfm_handle* h = c.h;
  Chunk& k = c.ck;
  h->stats.bp_jobs += (uint32_t)k.jobs.size();
  for (size_t q = 0; q < k.jobs.size(); ++q) {
    const Node nd = c.bp_nodes[(size_t)k.node_of[q]];  // a copy: retries are appended to bp_nodes below
    const BpResult& r = k.res[q];
    c.prob_cells[nd.prob] += r.cells;
    h->stats.cells_bp += r.cells;
    if (nd.score_rem == INT_MAX && k.jobs[q].band > 0 && !k.grown_job[q]) { ++c.roots_banded; c.roots_out += r.status == WFM_DEV_BAND; }
    c.keeps.drop(nd.keep);  // (taken or given up long since as a rule; a job that left the tile phase otherwise still holds it)
    if (k.reuse_bad[q]) {   // gave its keep up (restore_kept): the same node once more, both directions from score 0
      Node again = nd; again.keep = 0; again.keep_dir = 0;
      c.next_bp.push_back(again);
      continue;
    }
    if (nd.limit > 0 && !(r.status == 1 || (r.status == 0 && r.score <= nd.limit))) {
      // A root under a hard limit of its score that did not end within it.  Whatever the limit itself stopped is the problem's verdict: the step
      // kernel at the limit (WFM_DEV_LIMIT), a walk that found nothing within the bound or a job the tile phase let go on a ring without a band
      // (no alignment of a score within the bound leaves the rows the bound cuts), and on any ring a job that left the tile phase where
      // tile_job_beyond_limit says so.  A band that ran out says nothing about the score -- the band of a root is a guess: once more without
      // it, still under the limit, never without a bound.
      const BpJob& j = k.jobs[q];
      const bool beyond = r.status == WFM_DEV_LIMIT || r.status == 0 || (r.status == WFM_DEV_BAND && j.band == 0) ||
                          (r.status == WFM_DEV_BAND && j.resume_s == -3 && j.resume_sr >= 0 && !k.resume_bad[q] &&
                           tile_job_beyond_limit(j.pl, j.tl, j.sub, j.limit, j.resume_sr, c.tcfg.T));
      if (beyond) { c.prob_status[nd.prob] = WFM_ST_MAX_SCORE; ++c.limit_out; continue; }
      if (r.status == WFM_DEV_BAND) {
        Node again = nd; again.noband = 1; again.band = j.band; again.snap = 0; again.keep = 0; again.keep_dir = 0;
        if (c.pflags) c.pflags[nd.prob] |= WFM_PF_ROOT_AGAIN;
        const bool full_fits = ring_elems(ring_full_width(nd.pl, nd.tl), c.RR) * 4 <= h->mem_budget;
        if (!full_fits && c.pflags) c.pflags[nd.prob] |= WFM_PF_RING_GROWN;  // (its next band grows from this one: plan_ring)
        c.next_bp.push_back(again);
        c.band_retries += full_fits;
        continue;
      }
    }
    const bool guessed = nd.hinted && k.jobs[q].sub != SUB_NONE;  // the job really ran under the caller's guess
    if (r.status == WFM_DEV_BAND || (guessed && (r.status < 0 || (r.status == 0 && r.score > nd.sub)))) {
      // ran out of its narrow ring, or past the caller's guess of its score: once more, at the end of this level, on
      // a full ring and without the guess
      Node again = nd; again.noband = 1; again.sub = SUB_NONE; again.hinted = 0;
      again.band = k.jobs[q].band; again.snap = 0; again.keep = 0; again.keep_dir = 0;
      if (c.pflags) c.pflags[nd.prob] |= nd.score_rem == INT_MAX ? WFM_PF_ROOT_AGAIN : WFM_PF_JOB_AGAIN;
      // where the full ring does not fit, the job's next ring grows from the band it had (plan_ring)
      const bool full_fits = ring_elems(ring_full_width(nd.pl, nd.tl), c.RR) * 4 <= h->mem_budget;
      if (!full_fits) {
        if (c.pflags) c.pflags[nd.prob] |= WFM_PF_RING_GROWN;
        if (k.resume_bad[q]) again.band = nd.band;  // (the same band once more, from score 0)
        const int rc = keep_snapshot(c, q, again);
        if (rc != WFM_OK) return rc;
      }
      // (it joins the next level's jobs instead of holding this level up on its own: nodes are independent, only the gather at
      // the end waits for all of them.  Until round 5 a job that ran out of its ring was run again at the end of its own level --
      // three chains of 30 - 40 tile blocks one after the other in the first level of an LPA batch, 19 of its 50 ms of tile time;
      // WFM_RETRY_SAME_LEVEL=1 restores that for A/B runs; once per process)
      static const bool same_level = getenv("WFM_RETRY_SAME_LEVEL") && atoi(getenv("WFM_RETRY_SAME_LEVEL")) != 0;
      if (guessed || !same_level) c.next_bp.push_back(again); else c.bp_nodes.push_back(again);
      c.band_retries += full_fits;
      c.hint_retries += guessed;
      continue;
    }
    const bool score_root = nd.score_rem == INT_MAX && c.S->meta[nd.prob].score_only();  // the score is all the problem asks for: a root's meeting point is it
    if (r.status == 1 && score_root) {  // end reached at score 0
      c.prob_score[nd.prob] = 0;
    } else if (r.status == 1) {  // end reached at score 0 -> base aligner
      Node b = nd; b.smax = 0; b.keep = 0; c.base_nodes.push_back(b);
    } else if (r.status != 0) {
      if (c.knobs.debug) fprintf(stderr, "[wfm] problem %d: bialign job pl %d tl %d cb %d ce %d score_rem %d status %d (steps %d)\n", nd.prob, nd.pl, nd.tl, nd.cb, nd.ce, nd.score_rem, r.status, r.steps);
      c.prob_status[nd.prob] = WFM_ST_UNREACHABLE;
    } else {
      const int bp_h = r.off_fwd, bp_v = r.off_fwd - r.k_fwd;
      if (bp_h < 0 || bp_v < 0 || bp_h > nd.tl || bp_v > nd.pl) {
        if (c.knobs.debug) fprintf(stderr, "[wfm] problem %d: bialign job pl %d tl %d (at %d, %d of the problem; level %u, begin / end components %d %d, bound %d%s): breakpoint (%d, %d) outside, score %d = %d + %d comp %d k %d\n", nd.prob, nd.pl, nd.tl, nd.pb, nd.tb, c.level, nd.cb, nd.ce, k.jobs[q].sub, nd.hinted ? " guessed" : "", bp_v, bp_h, r.score, r.score_fwd, r.score_rev, r.comp, r.k_fwd);
        if (const char* dd = getenv("WFM_DUMP_FAIL")) dump_failed_problem(c, nd, dd);
        c.prob_status[nd.prob] = WFM_ST_UNREACHABLE; continue;
      }
      if (c.knobs.debug > 1) fprintf(stderr, "[wfm] problem %d level %u: job pl %d tl %d cb %d ce %d rem %d -> bp v %d h %d score %d = %d + %d comp %d\n", nd.prob, c.level, nd.pl, nd.tl, nd.cb, nd.ce, nd.score_rem, bp_v, bp_h, r.score, r.score_fwd, r.score_rev, r.comp);
      if (score_root) c.prob_score[nd.prob] = r.score;  // (no children, no leaves; the keeps it may have written go back below)
      else push_children(c, nd, r, bp_v, bp_h, q);
    }
  }
  // the keeps no child took go back
  for (int d = 0; d < 2; ++d)
    for (std::vector<int32_t>& kept : k.kept[d]) { for (int32_t id : kept) c.keeps.drop(id); kept.clear(); }
  return WFM_OK;
}

// The base jobs collected so far (incl. retries with a larger budget)
int run_leaves(AlignCall& c) {
  std::vector<Node> retry;
  while (!c.base_nodes.empty()) {
    retry.clear();
    const auto tb0 = std::chrono::steady_clock::now();
    const int rc = run_base_jobs(c.h, c.S, *c.pen, c.bcfg, c.base_nodes, retry, c.prob_status, c.prob_cells, c.tm, c.pflags, c.prob_score);
    c.wall_base += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count();
    if (rc != WFM_OK) return rc;
    c.base_nodes.swap(retry);
  }
  return WFM_OK;
}

void print_level_totals(const AlignCall& c) {
  if (getenv("WFM_P2_COUNT") && atoi(getenv("WFM_P2_COUNT"))) {
    unsigned long long n[8];
    wfm::p2_counters(n);
    fprintf(stderr, "[wfm] p2 overlap (cumulative): tests %llu, with candidates %llu, pairs listed %llu, blocks tested cell by cell %llu, pairs that met %llu; most pairs in a round %llu, most blocks one wave tested in a round %llu\n",
            n[0], n[1], n[2], n[3], n[4], n[5], n[6]);
  }
  if (!c.knobs.debug) return;
  if (c.hint_retries) fprintf(stderr, "[wfm] score hints: %llu roots ran past their hint and were run again without it\n", (unsigned long long)c.hint_retries);
  if (c.limit_out) fprintf(stderr, "[wfm] score limits: %llu roots ended beyond their hard limit\n", (unsigned long long)c.limit_out);
  if (c.band_jobs) fprintf(stderr, "[wfm] narrow rings: %llu jobs, %llu ran out of their band and were run again on full rings\n", (unsigned long long)c.band_jobs, (unsigned long long)c.band_retries);
  if (c.grown_jobs)
    fprintf(stderr, "[wfm] grown rings: %llu jobs, %llu widened and resumed, %llu started again, largest band %lld\n", (unsigned long long)c.grown_jobs,
            (unsigned long long)c.grown_widened, (unsigned long long)c.grown_restarts, (long long)c.grown_maxband);
  if (c.reuse_children || c.h->tile_ctr[WFM_TC_REUSE_KEEPS])
    fprintf(stderr, "[wfm] parent reuse: %llu keeps written (%.1f MB moved, store at most %.1f MB), %llu children of keeping jobs, %llu found a keep, %llu ran from it (%llu on a full ring in place of a narrow one): %llu resumed (%.1f MB moved), %llu fell back; ring arena at most %.1f MB in a chunk\n",
            (unsigned long long)c.h->tile_ctr[WFM_TC_REUSE_KEEPS], (double)c.keep_bytes / 1048576.0, (double)c.keeps.peak / 1048576.0, (unsigned long long)c.reuse_children,
            (unsigned long long)c.reuse_found, (unsigned long long)c.reuse_taken, (unsigned long long)c.reuse_full_rings, (unsigned long long)c.h->tile_ctr[WFM_TC_REUSE_RESUMED],
            (double)c.restore_bytes / 1048576.0, (unsigned long long)c.h->tile_ctr[WFM_TC_REUSE_FALLBACKS], (double)c.ring_peak * 4.0 / 1048576.0);
  if (c.knobs.debug > 1) fprintf(stderr, "[wfm] ring arena: at most %.1f MB in a chunk\n", (double)c.ring_peak * 4.0 / 1048576.0);
}

// The RLE pieces of every problem, compacted on the device: the runs, and where each problem's begin and how many they are
struct GatheredRuns { std::vector<uint32_t> runs; std::vector<int64_t> ostart; std::vector<int32_t> ocount; };
int gather_runs(AlignCall& c, GatheredRuns& g) {
  wfm_handle* h = c.h;
  const size_t n = c.last - c.first;
  std::vector<int64_t> poff(n), pcap(n);
  for (size_t i = 0; i < n; ++i) {  // (a score-only problem has no slots)
    const ProbMeta& pm = c.S->meta[c.first + i];
    poff[i] = pm.rle_off; pcap[i] = pm.score_only() ? 0 : (int64_t)pm.plen + pm.tlen;
  }
  if (h->i64a.ensure(n) || h->i64b.ensure(n) || h->i64c.ensure(n) || h->i32a.ensure(n) || h->total.ensure(1)) {
    h->err = "out of device memory"; return WFM_E_NOMEM;
  }
  HIPCHK(h, hipMemcpyAsync(h->i64a.p, poff.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->i64b.p, pcap.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(h->total.p, 0, sizeof(unsigned long long), h->stream));
  launch_compact(h->rle.p, h->i64a.p, h->i64b.p, h->rle_out.p, h->total.p, h->i64c.p, h->i32a.p, (int)n, h->stream);
  HIPCHK(h, hipGetLastError());
  g.ostart.resize(n);
  g.ocount.resize(n);
  unsigned long long total = 0;
  HIPCHK(h, hipMemcpyAsync(g.ostart.data(), h->i64c.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(g.ocount.data(), h->i32a.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(&total, h->total.p, sizeof(total), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  g.runs.resize((size_t)total + 1);
  if (total) HIPCHK(h, hipMemcpy(g.runs.data(), h->rle_out.p, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return WFM_OK;
}

// Every problem's result: its runs expanded into the caller's arena (or merged into *runs_out).  Returns the number of problems
// that failed, or an error.
int write_results(AlignCall& c, const GatheredRuns& g, uint64_t* cells_total) {
  std::vector<uint32_t>* runs_out = c.runs_out;
  size_t arena_pos = runs_out ? runs_out->size() : c.arena_base;
  if (runs_out && !g.runs.empty()) runs_out->reserve(runs_out->size() + g.runs.size() - 1);
  int failed = 0;
  for (size_t i = 0; i < c.last - c.first; ++i) {
    const size_t gi = c.first + i;  // problem id
    const ProbMeta& pm = c.S->meta[gi];
    wfm_result_t& r = c.out[gi];
    r.status = c.prob_status[gi];
    r.cells = c.prob_cells[gi];
    *cells_total += c.prob_cells[gi];
    r.ops_off = arena_pos; r.ops_len = 0; r.n_runs = 0; r.score = -1;
    if (r.status != WFM_ST_OK) { ++failed; continue; }
    if (pm.score_only()) { r.score = c.prob_score[gi]; continue; }  // (nothing of it in the arena or the runs)
    Expanded ex;
    const int err = expand_runs(g.runs.data() + g.ostart[i], g.ocount[i], *c.pen, pm.plen, pm.tlen, runs_out ? nullptr : c.ops_arena + arena_pos,
                                c.arena_bytes > arena_pos ? c.arena_bytes - arena_pos : 0, runs_out, &ex);
    if (err == EXPAND_RUN_TOO_LONG) { c.h->err = "run too long"; return WFM_E_ARG; }
    if (err == EXPAND_ARENA) { c.h->err = "ops arena too small"; return WFM_E_ARENA; }
    if (err == EXPAND_SPANS) {
      if (c.knobs.debug) fprintf(stderr, "[wfm] problem %zu: CIGAR spans %llu x %llu, sequences %d x %d\n", gi, (unsigned long long)ex.pc, (unsigned long long)ex.tc, pm.plen, pm.tlen);
      r.status = WFM_ST_UNREACHABLE;  // internal inconsistency: never report a broken CIGAR as ok
      ++failed;
      continue;
    }
    // (the runs' own price is the score of an end-to-end alignment; an ends-free problem reports its base job's score, full or score-only)
    r.ops_len = ex.ops_len; r.n_runs = ex.n_runs; r.score = pm.mode == WFM_MODE_ENDSFREE ? c.prob_score[gi] : ex.score;
    arena_pos = runs_out ? runs_out->size() : arena_pos + ex.ops_len;
  }
  return failed;
}

// Aligns problems [first, last) of S; their op strings go to ops_arena from byte arena_base on.
// runs_out != nullptr: run-length output (wfm_align_batch_rle) -- the part's merged runs are appended to *runs_out and
// ops_off counts from the part's first run (the caller shifts the parts into one buffer); ops_arena is not touched
int align_resident_impl(wfm_handle* h, const wfm_penalties_t* pen, wfm_seqset* S, size_t first, size_t last, wfm_result_t* out,
                        char* ops_arena, size_t arena_bytes, size_t arena_base, std::vector<uint32_t>* runs_out = nullptr,
                        uint32_t* pflags = nullptr) {
  int scope = 0;
  int rc = validate_pen(pen, &scope);
  if (rc != WFM_OK) { h->err = "unsupported penalties"; return rc; }
  const auto t_start = std::chrono::steady_clock::now();
  HIPCHK(h, hipSetDevice(h->device));
  h->stats = wfm_stats_t{};
  std::fill(h->tile_ctr, h->tile_ctr + WFM_TILE_COUNTERS, (uint64_t)0);
  if (last == first) return 0;
  AlignCall c{h, pen, S, first, last, out, ops_arena, arena_bytes, arena_base, runs_out, pflags, scope, DevPen{pen->x, pen->o1, pen->e1, pen->o2, pen->e2}};
  c.prob_status.assign(S->meta.size(), WFM_ST_OK);
  c.prob_cells.assign(S->meta.size(), 0);
  c.prob_score.assign(S->meta.size(), -1);
  // RLE slot buffer (zero = empty)
  if (h->rle.ensure((size_t)S->rle_total + 16) || h->rle_out.ensure((size_t)S->rle_total + 16)) {
    h->err = "out of device memory (rle)"; return WFM_E_NOMEM;
  }
  HIPCHK(h, hipMemsetAsync(h->rle.p, 0, ((size_t)S->rle_total + 16) * sizeof(uint32_t), h->stream));
  make_roots(c);
  if ((rc = bound_roots(c)) != WFM_OK) return rc;
  c.tcfg = tile_cfg(*pen, scope);
  c.bcfg = base_cfg(*pen);
  c.RR = ring_rows_for(scope);
  c.rules = RingRules{c.tcfg.enabled, c.tcfg.min_len, c.tcfg.min_score, c.tcfg.chunk, c.tcfg.T, c.RR, h->mem_budget, c.knobs.band_root};

  while (!c.bp_nodes.empty() || !c.base_nodes.empty()) {
    ++c.level;
    // ---- breakpoint jobs of this level (chunked to the memory budget) ----
    c.next_bp.clear();
    level_budget(c);
    for (size_t i0 = 0; i0 < c.bp_nodes.size(); i0 = c.ck.end) {
      plan_chunk(c, i0);
      if (!c.ck.jobs.empty()) {
        if ((rc = widen_resumed(c)) != WFM_OK || (rc = run_chunk_tiles(c)) != WFM_OK || (rc = run_chunk_p2(c)) != WFM_OK ||
            (rc = run_chunk_step(c)) != WFM_OK || (rc = settle_chunk(c)) != WFM_OK) return rc;
      }
      // a root's band is a guess (its score is not known): when the guess keeps failing -- a batch of divergent
      // records -- the remaining roots get full rings right away instead of paying for the attempt
      if (!c.rules.roots_off && c.roots_banded >= 16 && c.roots_out * 4 > c.roots_banded) c.rules.roots_off = true;
    }
    c.bp_nodes.swap(c.next_bp);
    // Leaves do not feed the recursion: while bialign jobs are left they wait (round 5), and all levels' leaves go out together behind the
    // last level -- two launches of thousands of leaves instead of two of hundreds per level, each with its wait for the device in the chain of
    // the batch's launches (C2: 12 launches + waits per part -> 3).  WFM_LEAVES_PER_LEVEL=1: the round-4 order; a quarter of a million leaves
    // waiting are run anyway (their arenas are chunked to the budget either way).  (Once per process.)
    static const bool leaves_per_level = getenv("WFM_LEAVES_PER_LEVEL") && atoi(getenv("WFM_LEAVES_PER_LEVEL")) != 0;
    if (!leaves_per_level && !c.bp_nodes.empty() && c.base_nodes.size() < ((size_t)1 << 18)) continue;
    if ((rc = run_leaves(c)) != WFM_OK) return rc;
  }
  h->stats.levels = c.level;
  print_level_totals(c);
  const auto t_levels = std::chrono::steady_clock::now();

  GatheredRuns g;
  bool any_full = false;  // (a call of score-only problems has no runs to gather)
  for (size_t i = first; i < last && !any_full; ++i) any_full = !S->meta[i].score_only();
  if (any_full && (rc = gather_runs(c, g)) != WFM_OK) return rc;
  uint64_t cells_total = 0;
  const int failed = write_results(c, g, &cells_total);
  if (failed < 0) return failed;
  cells_total += h->stats.cells_tile;
  h->stats.cells = cells_total;
  uint64_t range_bases = 0;
  for (size_t i = first; i < last; ++i) range_bases += (uint64_t)S->meta[i].plen + (uint64_t)S->meta[i].tlen;
  h->stats.bytes_algorithmic = 48ull * cells_total + range_bases;
  h->stats.ms_breakpoint = c.tm.bp_ms;
  h->stats.ms_tile = c.tm.tile_ms;
  h->stats.ms_base = c.tm.base_ms;
  h->stats.ms_kernels = c.tm.bp_ms + c.tm.base_ms;
  h->stats.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  if (c.knobs.debug)
    fprintf(stderr, "[wfm] wall: total %.2f ms | levels %.2f (tile phase %.2f incl. kernels %.2f; base phase %.2f incl. kernels %.2f; bp kernels %.2f) | gather+expand %.2f\n",
            h->stats.ms_total, std::chrono::duration<double, std::milli>(t_levels - t_start).count(), c.wall_tile, c.tm.tile_ms, c.wall_base, c.tm.base_ms,
            c.tm.bp_ms - c.tm.tile_ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_levels).count());
  return failed;
}

}  // namespace

extern "C" {

int wfm_device_count(void) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return ndev < 0 ? 0 : ndev;
}

int wfm_create(int device, wfm_handle_t** out) {
  if (!out) return WFM_E_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return WFM_E_NODEVICE;
  if (device < 0 || device >= ndev) return WFM_E_ARG;
  if (hipSetDevice(device) != hipSuccess) return WFM_E_HIP;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return WFM_E_HIP;
  // The kernels are written for the GFX9 / CDNA wave model and nothing else: DPP wave_shr / wave_shl / row_bcast, 64-lane waves, and waves that have
  // ended dropping out of s_barrier (wfa_tile2.hip lets the waves a narrow tile does not need return before its first barrier).  Any other
  // target fails here, loudly, instead of hanging in a kernel; wfm_selftest_dpp checks both properties on the device itself.
  if (strncmp(prop.gcnArchName, "gfx9", 4) != 0 || prop.warpSize != 64) return WFM_E_NODEVICE;
  wfm_handle* h = new wfm_handle();
  h->device = device;
  // (hipDeviceProp_t::name is empty on some boxes of the pool: the architecture name alone then)
  h->name = prop.name[0] ? std::string(prop.name) + " (" + prop.gcnArchName + ")" : std::string(prop.gcnArchName);
  if (hipStreamCreate(&h->stream) != hipSuccess) { delete h; return WFM_E_HIP; }
  (void)hipEventCreate(&h->ev0); (void)hipEventCreate(&h->ev1); (void)hipEventCreate(&h->ev2); (void)hipEventCreate(&h->ev3);
  h->tile_ev.resize(64);
  for (auto& e : h->tile_ev) (void)hipEventCreate(&e);
  (void)hipEventCreate(&h->ev_base);
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) { fr = (size_t)16 << 30; }
  // the device's heap (dev_cache.hip) exists from the first handle on, with its first gigabytes mapped: no call of either path meets memory
  // the process has never had before it has used those (the budgets below are taken from what was free BEFORE, the heap's pool is theirs)
  wfm_dcache_warm();
  // 40 % of the free HBM, but no more than 32 GB: on this driver a first hipMalloc beyond a few tens of GB costs 35-40 ms
  // per GB (64 GB: 2.5-4.4 s, 110 GB: 3.9 s, 16 GB: 0.3 ms -- scripts/micro/malloc_cost.hip, profiles/r3_cold_start.md), which a
  // one-shot run pays in full: LPA all-vs-all (C2) aligned in 3.3 s cold and 0.33 s warm with rings sized for 115 GB.  A
  // level that needs more is worked off in chunks and on narrow rings
  // Handles of one device share it (the align driver keeps up to three per device): a further handle takes its 40 % of what
  // is free divided by the handles that are there already, so that on a smaller GPU the budgets together stay inside the memory
  int live = 0;
  { std::lock_guard<std::mutex> lk(g_base_mu); if (device < 64) live = g_dev_handles[device]++; }
  h->mem_budget = std::min<size_t>((size_t)((double)fr * 0.40 / (double)(1 + live)), (size_t)32 << 30);
  const char* env = getenv("WFM_MEM_BUDGET_MB");
  if (env) h->mem_budget = (size_t)atoll(env) << 20;
  h->mem_budget_full = h->mem_budget;
  *out = h;
  return WFM_OK;
}

void wfm_destroy(wfm_handle_t* h) {
  if (!h) return;
  for (wfm_handle* p : h->peers) wfm_destroy(p);
  h->peers.clear();
  bool last_of_process = false;
  if (!h->is_peer) {
    std::lock_guard<std::mutex> lk(g_base_mu);
    if (h->device < 64 && g_dev_handles[h->device] > 0) --g_dev_handles[h->device];
    last_of_process = true;
    for (int d = 0; d < 64; ++d) last_of_process &= g_dev_handles[d] == 0;
  }
  (void)hipSetDevice(h->device);
  h->ring.release(); h->base32.release(); h->base8.release(); h->rle.release(); h->rle_out.release();
  h->tilejobs.release(); h->tiletasks.release(); h->tilemak.release();
  h->revjobs.release(); h->bndjobs.release(); h->bndres.release();
  if (h->stage) { (void)hipHostFree(h->stage); h->stage = nullptr; h->stage_cap = 0; }
  for (int k = 0; k < 2; ++k)
    if (h->cspin[k]) { (void)hipHostFree(h->cspin[k]); h->cspin[k] = nullptr; }
  h->p2rows.release(); h->p2max.release(); h->p2bmax.release(); h->p2jobs.release(); h->widenjobs.release(); h->keeptasks.release(); h->restoretasks.release(); h->restoreres.release();
  h->bpjobs.release(); h->bpres.release(); h->bsjobs.release(); h->bsres.release();
  h->b2tjobs.release(); h->b2ttasks.release(); h->b2tkeys.release(); h->b2toffs.release(); h->b2tactive.release();
  h->i64a.release(); h->i64b.release(); h->i64c.release(); h->i32a.release(); h->seqflags.release(); h->flagjobs.release(); h->gathertasks.release(); h->scratch.release(); h->outblk.release(); h->optrows.release(); h->total.release();
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->ev2) (void)hipEventDestroy(h->ev2);
  if (h->ev3) (void)hipEventDestroy(h->ev3);
  for (auto& e : h->tile_ev) if (e) (void)hipEventDestroy(e);
  if (h->ev_base) (void)hipEventDestroy(h->ev_base);
  if (h->attachment && h->attachment_free) h->attachment_free(h->attachment);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  // the last handle of the process: the sequence stores a map call left open for the call after it (host/fasta.cpp, keep_until_next: up to
  // 32 GB of host memory) are let go.  The device block cache stays -- a process that creates and destroys handles in turn (the test-suite)
  // would pay every block's first hipMalloc again -- and goes back to the driver with wfm_trim_device_cache(), see INTEGRATION.md.
  if (last_of_process && g_last_handle_hook) {
    // (counted again under the lock, and the hook runs under it: a wfm_create on another thread in between keeps the stores its map call is about to ask for)
    std::lock_guard<std::mutex> lk(g_base_mu);
    bool still_last = true;
    for (int d = 0; d < 64; ++d) still_last &= g_dev_handles[d] == 0;
    if (still_last) g_last_handle_hook();
  }
}

const char* wfm_last_error(const wfm_handle_t* h) { return h ? h->err.c_str() : "null handle"; }

void wfm_set_concurrent_calls(wfm_handle_t* h, int other_calls) { if (h) h->other_calls = other_calls > 0 ? other_calls : 0; }

size_t wfm_get_problem_flags(const wfm_handle_t* h, uint32_t* out, size_t n) {
  if (!h) return 0;
  const size_t have = h->prob_flags.empty() ? 0 : h->prob_flags.size() - 1;
  if (out) for (size_t i = 0; i < n && i < have; ++i) out[i] = h->prob_flags[i];
  return have;
}

size_t wfm_get_tile_counters(const wfm_handle_t* h, uint64_t* out, size_t n) {
  if (!h) return 0;
  if (out) for (size_t i = 0; i < n && i < (size_t)WFM_TILE_COUNTERS; ++i) out[i] = h->tile_ctr[i];
  return (size_t)WFM_TILE_COUNTERS;
}

int wfm_device_name(const wfm_handle_t* h, char* buf, size_t buflen) {
  if (!h || !buf || !buflen) return WFM_E_ARG;
  snprintf(buf, buflen, "%s", h->name.c_str());
  return WFM_OK;
}

size_t wfm_align_arena_bytes(const wfm_problem_t* problems, size_t n) {
  size_t t = 0;
  for (size_t i = 0; i < n; ++i)
    if (!(problems[i].mode & WFM_MODE_SCORE_ONLY)) t += (size_t)problems[i].plen + (size_t)problems[i].tlen + 1;
  return t;
}

}  // extern "C"
namespace {
// The layout of a seqset, shared by wfm_upload_sequences and wfm_upload_sequence_refs (P: wfm_problem_t or wfm_problem_ref_t, lengths
// validated by the caller): SEQ_PAD zero bytes, the forward copies -- the only part that crosses PCIe where the sides are host
// pointers -- each followed by SEQ_PAD zero bytes, SEQ_PAD more, then the reversed copies of the BiWFA problems and a last SEQ_PAD.
// `mode` of every problem of an upload: one of the three modes under the mask, no bit beyond the mask and the two flags, a hard limit only
// on a BiWFA problem and only with a limit to go by.  The message names the first problem that fails.
template <typename P>
int check_modes(wfm_handle* h, const P* problems, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const int32_t mode = problems[i].mode, m = mode & WFM_MODE_MASK;
    const char* what = nullptr;
    if (mode & ~(WFM_MODE_MASK | WFM_MODE_SCORE_ONLY | WFM_MODE_SCORE_LIMIT)) what = "unknown bits in mode";
    else if (m != WFM_MODE_END2END_BIWFA && m != WFM_MODE_ENDSFREE && m != WFM_MODE_END2END_UNI) what = "unknown mode";
    else if ((mode & WFM_MODE_SCORE_LIMIT) && m != WFM_MODE_END2END_BIWFA) what = "WFM_MODE_SCORE_LIMIT takes END2END_BIWFA";
    else if ((mode & WFM_MODE_SCORE_LIMIT) && problems[i].score_hint <= 0) what = "WFM_MODE_SCORE_LIMIT takes a score_hint > 0";
    if (what) { h->err = "problem " + std::to_string(i) + ": " + what; return WFM_E_ARG; }
  }
  return WFM_OK;
}

template <typename P>
void layout_seqset(wfm_seqset* S, const P* problems, size_t n, size_t* fwd_bytes_out) {
  S->meta.resize(n);
  size_t bytes = SEQ_PAD, rev_bytes = 0;
  int64_t rle = 0;
  for (size_t i = 0; i < n; ++i) {
    const P& p = problems[i];
    ProbMeta& m = S->meta[i];
    m.plen = p.plen; m.tlen = p.tlen; m.mode = p.mode & WFM_MODE_MASK; m.flags = p.mode & ~WFM_MODE_MASK;  // (check_modes has seen them)
    m.limit = (m.flags & WFM_MODE_SCORE_LIMIT) ? p.score_hint : 0;
    m.hint = (m.mode == WFM_MODE_END2END_BIWFA && p.score_hint > 0 && !m.limit) ? p.score_hint : 0;
    m.pbf = std::min(std::max(p.pattern_begin_free, 0), p.plen); m.pef = std::min(std::max(p.pattern_end_free, 0), p.plen);
    m.tbf = std::min(std::max(p.text_begin_free, 0), p.tlen);    m.tef = std::min(std::max(p.text_end_free, 0), p.tlen);
    if (m.mode != WFM_MODE_ENDSFREE) { m.pbf = m.pef = m.tbf = m.tef = 0; }
    m.p_fwd = (int64_t)bytes; bytes += (size_t)p.plen + SEQ_PAD;
    m.t_fwd = (int64_t)bytes; bytes += (size_t)p.tlen + SEQ_PAD;
    const bool need_rev = (m.mode == WFM_MODE_END2END_BIWFA);
    if (need_rev) {
      m.p_rev = (int64_t)rev_bytes; rev_bytes += (size_t)p.plen + SEQ_PAD;   // relative to the end of the forward part for now
      m.t_rev = (int64_t)rev_bytes; rev_bytes += (size_t)p.tlen + SEQ_PAD;
    } else { m.p_rev = -1; m.t_rev = -1; }
    m.rle_off = rle;
    if (!m.score_only()) rle += (int64_t)p.plen + p.tlen + 1;
    S->seq_bases += (uint64_t)p.plen + (uint64_t)p.tlen;
  }
  bytes += SEQ_PAD;
  const size_t fwd_bytes = bytes;
  for (size_t i = 0; i < n; ++i) {
    ProbMeta& m = S->meta[i];
    if (m.p_rev < 0) { m.p_rev = m.p_fwd; m.t_rev = m.t_fwd; }
    else { m.p_rev += (int64_t)fwd_bytes; m.t_rev += (int64_t)fwd_bytes; }
  }
  S->bytes = fwd_bytes + rev_bytes + SEQ_PAD;
  S->rle_total = rle;
  *fwd_bytes_out = fwd_bytes;
}
}  // namespace
extern "C" {

int wfm_upload_sequences(wfm_handle_t* h, const wfm_problem_t* problems, size_t n, wfm_seqset_t** out) {
  if (!h || !out || (n && !problems)) return WFM_E_ARG;
  *out = nullptr;
  HIPCHK(h, hipSetDevice(h->device));
  for (size_t i = 0; i < n; ++i) {
    const wfm_problem_t& p = problems[i];
    if (p.plen < 0 || p.tlen < 0 || (int64_t)p.plen + p.tlen > (1 << 29) || (p.plen && !p.pattern) || (p.tlen && !p.text)) {
      h->err = "bad problem"; return WFM_E_ARG;
    }
  }
  if (const int mrc = check_modes(h, problems, n)) return mrc;
  wfm_seqset* S = new wfm_seqset();
  size_t fwd_bytes = 0;
  layout_seqset(S, problems, n, &fwd_bytes);
  const size_t bytes = S->bytes;
  const int64_t rle = S->rle_total;
  // Only the forward sequences (with their zero padding) are written on the host and cross PCIe; the reversed copies
  // BiWFA's reverse direction reads are made on the device after the upload (half the bytes, no byte-wise host loop).
  // The forward part is assembled in a pinned staging buffer kept with the handle, by a few threads.
  if (h->stage_cap < fwd_bytes) {
    if (h->stage) (void)hipHostFree(h->stage);
    h->stage = nullptr; h->stage_cap = 0;
    const size_t want = fwd_bytes + fwd_bytes / 4 + (1 << 20);
    if (hipHostMalloc((void**)&h->stage, want, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      h->stage = nullptr;
    } else h->stage_cap = want;
  }
  std::vector<uint8_t> pageable;
  uint8_t* host = h->stage;
  if (!host) { pageable.resize(fwd_bytes); host = pageable.data(); }
  {
    const int nt = (int)std::min<size_t>(8, std::max<size_t>(1, n / 64));
    auto fill = [&](size_t i0, size_t i1) {
      for (size_t i = i0; i < i1; ++i) {
        const wfm_problem_t& p = problems[i];
        const ProbMeta& m = S->meta[i];
        // sequence, then SEQ_PAD zero bytes (the extension reads up to 40 bytes past a sub-range end)
        if (p.plen) memcpy(host + m.p_fwd, p.pattern, (size_t)p.plen);
        memset(host + m.p_fwd + p.plen, 0, SEQ_PAD);
        if (p.tlen) memcpy(host + m.t_fwd, p.text, (size_t)p.tlen);
        memset(host + m.t_fwd + p.tlen, 0, SEQ_PAD);
      }
    };
    memset(host, 0, SEQ_PAD);
    memset(host + fwd_bytes - SEQ_PAD, 0, SEQ_PAD);
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(fill, n * (size_t)t / nt, n * (size_t)(t + 1) / nt);
    fill(0, n / (size_t)nt);
    for (auto& t : th) t.join();
  }
  // (from the block cache, like the arenas: a batch's sequences are about as long as the last batch's, and the block it freed serves)
  if (wfm_dmalloc((void**)&S->d_seq, bytes) != hipSuccess) { (void)hipGetLastError(); delete S; h->err = "out of device memory (sequences)"; return WFM_E_NOMEM; }
  S->bytes = bytes;
  S->rle_total = rle;
  // the 2-bit mirror the tile kernel extends on (wfa_tile2.hip): a quarter of a byte per base, made on the device
  const int64_t pk_words = ((int64_t)bytes + 15) / 16;
  if (wfm_dmalloc((void**)&S->d_pk, (size_t)(pk_words + PK_PAD_WORDS) * 4) != hipSuccess) {
    (void)hipGetLastError();
    wfm_dfree(S->d_seq); delete S; h->err = "out of device memory (packed sequences)"; return WFM_E_NOMEM;
  }
  hipError_t e = hipMemcpyAsync(S->d_seq, host, fwd_bytes, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(S->d_seq + bytes - SEQ_PAD, 0, SEQ_PAD, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(S->d_pk + pk_words, 0, (size_t)PK_PAD_WORDS * 4, h->stream);
  if (e == hipSuccess) {
    std::vector<SeqRev> rv;
    rv.reserve(n);
    for (size_t i = 0; i < n; ++i) {
      const ProbMeta& m = S->meta[i];
      if (m.mode == WFM_MODE_END2END_BIWFA) rv.push_back(SeqRev{m.p_fwd, m.p_rev, m.t_fwd, m.t_rev, m.plen, m.tlen});
    }
    if (!rv.empty()) {
      if (h->revjobs.ensure(rv.size())) e = hipErrorOutOfMemory;
      if (e == hipSuccess) e = hipMemcpyAsync(h->revjobs.p, rv.data(), rv.size() * sizeof(SeqRev), hipMemcpyHostToDevice, h->stream);
      if (e == hipSuccess) { launch_reverse(S->d_seq, h->revjobs.p, (int)rv.size(), SEQ_PAD, h->stream); e = hipGetLastError(); }
    }
    // the mirror of everything (forward and reversed copies), and which problems are pure ACGT
    std::vector<int32_t> flags(n, 1);
    std::vector<SeqRev> fj(n);
    for (size_t i = 0; i < n; ++i) { const ProbMeta& m = S->meta[i]; fj[i] = SeqRev{m.p_fwd, m.p_fwd, m.t_fwd, m.t_fwd, m.plen, m.tlen}; }
    if (e == hipSuccess && n && (h->seqflags.ensure(n) || h->flagjobs.ensure(n))) e = hipErrorOutOfMemory;
    if (e == hipSuccess && n) e = hipMemsetAsync(h->seqflags.p, 1, n * sizeof(int32_t), h->stream);
    if (e == hipSuccess && n) e = hipMemcpyAsync(h->flagjobs.p, fj.data(), n * sizeof(SeqRev), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
      launch_seq_pack(S->d_seq, S->d_pk, pk_words, (int64_t)bytes, h->flagjobs.p, (int)n, n ? h->seqflags.p : nullptr, h->stream);
      e = hipGetLastError();
    }
    if (e == hipSuccess && n) e = hipMemcpyAsync(flags.data(), h->seqflags.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // (fj is read by the copy above)
    if (e == hipSuccess) {
      S->acgt.assign(flags.begin(), flags.end());
      if (getenv("WFM_DEBUG") && atoi(getenv("WFM_DEBUG")) > 1) {
        size_t bad = 0;
        for (int32_t f : flags) bad += f == 0;
        fprintf(stderr, "[wfm] upload: %zu problems, %zu of them with something other than upper-case ACGT (byte kernels)\n", n, bad);
      }
    }
  }
  if (e != hipSuccess) { wfm_dfree(S->d_seq); wfm_dfree(S->d_pk); delete S; h->err = hipGetErrorString(e); return WFM_E_HIP; }
  *out = S;
  return WFM_OK;
}

void wfm_free_sequences(wfm_handle_t* h, wfm_seqset_t* s) {
  if (!s) return;
  if (h) (void)hipSetDevice(h->device);
  // back to the block cache; one wait for the device serves both (hipFree waited once per block)
  if (s->d_seq || s->d_pk) (void)hipDeviceSynchronize();
  if (s->d_seq) wfm_dfree_nosync(s->d_seq);
  if (s->d_pk) wfm_dfree_nosync(s->d_pk);
  delete s;
}


// ---- sequences resident on the device, problems by reference (wfmash_hip.h) ----
namespace {
constexpr size_t STORE_SLACK = 64;            // bytes before and behind a stored sequence (the gather kernel reads up to 15 beyond a window)
constexpr size_t STORE_PIN_CHUNK = 8u << 20;  // raw bytes per pinned chunk of wfm_seqstore_add
}  // namespace

int wfm_seqstore_create(wfm_handle_t* h, wfm_seqstore_t** out) {
  if (!h || !out) return WFM_E_ARG;
  wfm_seqstore* s = new wfm_seqstore();
  s->device = h->device;
  *out = s;
  return WFM_OK;
}

void wfm_seqstore_free(wfm_seqstore_t* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  (void)hipDeviceSynchronize();  // one wait serves every block
  for (auto& q : s->seqs) if (q.block) wfm_dfree_nosync(q.block);
  for (int k = 0; k < 2; ++k) {
    if (s->pin[k]) (void)hipHostFree(s->pin[k]);
    if (s->pin_ev[k]) (void)hipEventDestroy(s->pin_ev[k]);
  }
  delete s;
}

int wfm_seqstore_info(const wfm_seqstore_t* s, int64_t* n_seqs, int64_t* bytes) {
  if (!s) return WFM_E_ARG;
  std::lock_guard<std::mutex> lk(s->mu);
  if (n_seqs) *n_seqs = (int64_t)s->seqs.size();
  if (bytes) *bytes = s->bytes;
  return WFM_OK;
}

int32_t wfm_seqstore_add(wfm_handle_t* h, wfm_seqstore_t* s, const char* seq, int64_t len) {
  if (!h || !s || len < 0 || (len && !seq)) return WFM_E_ARG;
  if (s->device != h->device) { h->err = "the sequence store belongs to another device"; return WFM_E_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  std::lock_guard<std::mutex> add_lk(s->add_mu);
  wfm_seqstore::Seq q;
  q.len = len;
  q.block_bytes = (((size_t)len + 15) & ~(size_t)15) + 2 * STORE_SLACK;
  if (wfm_dmalloc((void**)&q.block, q.block_bytes) != hipSuccess) {
    (void)hipGetLastError();
    h->err = "out of device memory (sequence store)";
    return WFM_E_NOMEM;
  }
  q.data = q.block + STORE_SLACK;  // (16-byte aligned as the block is)
  auto fail = [&](hipError_t e) { (void)hipStreamSynchronize(h->stream); wfm_dfree(q.block); h->err = hipGetErrorString(e); return (int32_t)WFM_E_HIP; };
  hipError_t e = hipMemsetAsync(q.block, 0, q.block_bytes, h->stream);
  // the raw bytes in chunks through two pinned buffers (a chromosome in a pageable block must not be one pageable hipMemcpy)
  for (int k = 0; k < 2 && e == hipSuccess && len > 0; ++k) {
    if (!s->pin[k]) e = hipHostMalloc((void**)&s->pin[k], STORE_PIN_CHUNK, hipHostMallocDefault);
    if (e == hipSuccess && !s->pin_ev[k]) e = hipEventCreateWithFlags(&s->pin_ev[k], hipEventDisableTiming);
  }
  int turn = 0;
  for (int64_t at = 0; at < len && e == hipSuccess; at += (int64_t)STORE_PIN_CHUNK, turn ^= 1) {
    const size_t nb = (size_t)std::min<int64_t>((int64_t)STORE_PIN_CHUNK, len - at);
    if (at >= 2 * (int64_t)STORE_PIN_CHUNK) e = hipEventSynchronize(s->pin_ev[turn]);  // the copy that last read this buffer
    if (e != hipSuccess) break;
    memcpy(s->pin[turn], seq + at, nb);
    e = hipMemcpyAsync(q.data + at, s->pin[turn], nb, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipEventRecord(s->pin_ev[turn], h->stream);
  }
  if (e == hipSuccess && len > 0) { launch_seq_normalize(q.data, len, h->stream); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(e);
  std::lock_guard<std::mutex> lk(s->mu);
  if (s->seqs.size() >= (size_t)INT32_MAX) { wfm_dfree(q.block); h->err = "sequence store is full"; return WFM_E_ARG; }
  s->seqs.push_back(q);
  s->bytes += (int64_t)q.block_bytes;
  return (int32_t)(s->seqs.size() - 1);
}

int wfm_upload_sequence_refs(wfm_handle_t* h, const wfm_seqstore_t* store, const wfm_problem_ref_t* refs, size_t n, wfm_seqset_t** out) {
  if (!h || !out || (n && !refs)) return WFM_E_ARG;
  *out = nullptr;
  if (store && store->device != h->device) { h->err = "the sequence store belongs to another device"; return WFM_E_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  // the table as it stands (blocks never move: the pointers stay good without the lock)
  std::vector<wfm_seqstore::Seq> table;
  if (store) { std::lock_guard<std::mutex> lk(store->mu); table = store->seqs; }
  size_t host_bytes = 0;
  auto bad = [&](size_t i, const char* what) { h->err = "problem " + std::to_string(i) + ": " + what; return WFM_E_ARG; };
  for (size_t i = 0; i < n; ++i) {
    const wfm_problem_ref_t& p = refs[i];
    if (p.plen < 0 || p.tlen < 0) return bad(i, "negative length");
    if ((int64_t)p.plen + p.tlen > (1 << 29)) return bad(i, "plen + tlen exceeds 2^29");
    const int32_t ids[2] = {p.pattern_seq, p.text_seq};
    const int64_t offs[2] = {p.pattern_off, p.text_off};
    const int32_t lens[2] = {p.plen, p.tlen};
    const char* ptrs[2] = {p.pattern, p.text};
    for (int side = 0; side < 2; ++side) {
      if (ids[side] == -1) {
        if (lens[side] && !ptrs[side]) return bad(i, "null host pointer for a side of non-zero length");
        host_bytes += (size_t)lens[side];
      } else {
        if (ids[side] < 0 || (size_t)ids[side] >= table.size()) return bad(i, "unknown sequence id");
        if (offs[side] < 0 || offs[side] > table[(size_t)ids[side]].len || (int64_t)lens[side] > table[(size_t)ids[side]].len - offs[side])
          return bad(i, "window leaves its sequence");
      }
    }
  }
  if (const int mrc = check_modes(h, refs, n)) return mrc;
  wfm_seqset* S = new wfm_seqset();
  size_t fwd_bytes = 0;
  layout_seqset(S, refs, n, &fwd_bytes);
  const size_t bytes = S->bytes;
  uint8_t* d_host = nullptr;  // the host-pointer sides end to end, STORE_SLACK before and behind them
  auto drop = [&](int rc, const std::string& msg) {
    (void)hipStreamSynchronize(h->stream);
    if (S->d_seq) wfm_dfree_nosync(S->d_seq);
    if (S->d_pk) wfm_dfree_nosync(S->d_pk);
    if (d_host) wfm_dfree_nosync(d_host);
    delete S;
    h->err = msg;
    return rc;
  };
  // Only the host-pointer sides are assembled in the pinned staging buffer and cross PCIe, end to end into a block of their own;
  // from there they are laid out by the same tasks as the windows of the store.
  uint8_t* host = nullptr;
  std::vector<uint8_t> pageable;
  if (host_bytes) {
    if (h->stage_cap < host_bytes) {
      if (h->stage) (void)hipHostFree(h->stage);
      h->stage = nullptr; h->stage_cap = 0;
      const size_t want = host_bytes + host_bytes / 4 + (1 << 20);
      if (hipHostMalloc((void**)&h->stage, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); h->stage = nullptr; }
      else h->stage_cap = want;
    }
    host = h->stage;
    if (!host) { pageable.resize(host_bytes); host = pageable.data(); }
    if (wfm_dmalloc((void**)&d_host, host_bytes + 2 * STORE_SLACK) != hipSuccess) { (void)hipGetLastError(); d_host = nullptr; return drop(WFM_E_NOMEM, "out of device memory (staged sequences)"); }
  }
  if (wfm_dmalloc((void**)&S->d_seq, bytes) != hipSuccess) { (void)hipGetLastError(); S->d_seq = nullptr; return drop(WFM_E_NOMEM, "out of device memory (sequences)"); }
  const int64_t pk_words = ((int64_t)bytes + 15) / 16;
  if (wfm_dmalloc((void**)&S->d_pk, (size_t)(pk_words + PK_PAD_WORDS) * 4) != hipSuccess) { (void)hipGetLastError(); S->d_pk = nullptr; return drop(WFM_E_NOMEM, "out of device memory (packed sequences)"); }
  // the tasks: per side the forward copy and, for a BiWFA problem, the reversed one, each cut into chunks; the last chunk writes the pad
  std::vector<SeqGatherTask> tasks;
  tasks.reserve(4 * n + 16);
  auto add_copy = [&](const uint8_t* src, int64_t dst_off, int32_t len, bool reverse, bool complement) {
    int32_t at = 0;
    do {
      const int32_t nb = std::min<int32_t>(len - at, WFM_SEQ_GATHER_CHUNK);
      const bool last = at + nb == len;
      // (read backwards, chunk [at, at + nb) of the copy comes from the window's bytes [len - at - nb, len - at))
      tasks.push_back(SeqGatherTask{src + (reverse ? len - at - nb : at), S->d_seq + dst_off + at, nb, last ? SEQ_PAD : 0, reverse ? 1 : 0, complement ? 1 : 0});
      at += nb;
    } while (at < len);
  };
  size_t host_at = 0;
  for (size_t i = 0; i < n; ++i) {
    const wfm_problem_ref_t& p = refs[i];
    const ProbMeta& m = S->meta[i];
    const bool biwfa = m.mode == WFM_MODE_END2END_BIWFA;
    for (int side = 0; side < 2; ++side) {
      const int32_t id = side ? p.text_seq : p.pattern_seq, len = side ? p.tlen : p.plen;
      const int64_t fwd = side ? m.t_fwd : m.p_fwd, rev = side ? m.t_rev : m.p_rev;
      const uint8_t* src;
      bool rc = false;
      if (id == -1) {
        if (len) memcpy(host + host_at, side ? p.text : p.pattern, (size_t)len);
        src = d_host ? d_host + STORE_SLACK + host_at : nullptr;
        host_at += (size_t)len;
      } else {
        src = table[(size_t)id].data + (side ? p.text_off : p.pattern_off);
        rc = (side ? p.text_revcomp : p.pattern_revcomp) != 0;
      }
      add_copy(src, fwd, len, rc, rc);            // '+': (0, 0), '-': (1, 1)
      if (biwfa) add_copy(src, rev, len, !rc, rc);  // '+': (1, 0), '-': (0, 1)
    }
  }
  hipError_t e = hipSuccess;
  if (host_bytes) e = hipMemcpyAsync(d_host + STORE_SLACK, host, host_bytes, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(S->d_seq, 0, SEQ_PAD, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(S->d_seq + fwd_bytes - SEQ_PAD, 0, SEQ_PAD, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(S->d_seq + bytes - SEQ_PAD, 0, SEQ_PAD, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(S->d_pk + pk_words, 0, (size_t)PK_PAD_WORDS * 4, h->stream);
  const bool timed = getenv("WFM_DEBUG") != nullptr;
  if (e == hipSuccess && !tasks.empty()) {
    if (h->gathertasks.ensure(tasks.size())) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipMemcpyAsync(h->gathertasks.p, tasks.data(), tasks.size() * sizeof(SeqGatherTask), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && timed) e = hipEventRecord(h->ev0, h->stream);
    if (e == hipSuccess) { launch_seq_gather(h->gathertasks.p, (int64_t)tasks.size(), h->stream); e = hipGetLastError(); }
    if (e == hipSuccess && timed) e = hipEventRecord(h->ev1, h->stream);
  }
  // the mirror of everything (forward and reversed copies), and which problems are pure ACGT: as wfm_upload_sequences
  std::vector<int32_t> flags(n, 1);
  std::vector<SeqRev> fj(n);
  for (size_t i = 0; i < n; ++i) { const ProbMeta& m = S->meta[i]; fj[i] = SeqRev{m.p_fwd, m.p_fwd, m.t_fwd, m.t_fwd, m.plen, m.tlen}; }
  if (e == hipSuccess && n && (h->seqflags.ensure(n) || h->flagjobs.ensure(n))) e = hipErrorOutOfMemory;
  if (e == hipSuccess && n) e = hipMemsetAsync(h->seqflags.p, 1, n * sizeof(int32_t), h->stream);
  if (e == hipSuccess && n) e = hipMemcpyAsync(h->flagjobs.p, fj.data(), n * sizeof(SeqRev), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    launch_seq_pack(S->d_seq, S->d_pk, pk_words, (int64_t)bytes, h->flagjobs.p, (int)n, n ? h->seqflags.p : nullptr, h->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess && n) e = hipMemcpyAsync(flags.data(), h->seqflags.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return drop(WFM_E_HIP, hipGetErrorString(e));
  if (d_host) { wfm_dfree_nosync(d_host); d_host = nullptr; }
  S->acgt.assign(flags.begin(), flags.end());
  if (timed && !tasks.empty()) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess)
      fprintf(stderr, "[wfm] upload by reference: %zu problems, %zu gather tasks, %zu bytes written (%zu of them from host pointers) in %.3f ms = %.1f GB/s\n", n,
              tasks.size(), bytes, host_bytes, ms, ms > 0 ? (double)bytes / (ms * 1e6) : 0.0);
    else (void)hipGetLastError();
  }
  *out = S;
  return WFM_OK;
}

int64_t wfm_download_sequences(wfm_handle_t* h, const wfm_seqset_t* s, uint8_t* out, int64_t cap) {
  if (!h || !s || cap < 0) return WFM_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t nb = std::min<size_t>((size_t)cap, s->bytes);
  if (out && nb) {
    HIPCHK(h, hipMemcpyAsync(out, s->d_seq, nb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return (int64_t)s->bytes;
}

namespace {
// both output forms: ops_arena (one byte per op) or, with runs != nullptr, one malloc'd buffer of merged runs
int align_resident_any(wfm_handle_t* h, const wfm_penalties_t* pen, wfm_seqset_t* s, wfm_result_t* out,
                       char* ops_arena, size_t arena_bytes, uint32_t** runs, size_t* n_runs_total) {
  if (!h || !s || !out || (!runs && !ops_arena && arena_bytes)) return WFM_E_ARG;
  if (runs) *runs = nullptr;
  if (n_runs_total) *n_runs_total = 0;
  const size_t n = s->meta.size();
  std::vector<std::vector<uint32_t>> part_runs(1);
  // the parts' runs side by side in one buffer; ops_off of part k's problems shifted by what lies before it
  auto hand_over_runs = [&](const std::vector<size_t>& cut) -> int {
    if (!runs) return WFM_OK;
    size_t total = 0;
    for (const auto& v : part_runs) total += v.size();
    uint32_t* buf = (uint32_t*)malloc((total + 1) * sizeof(uint32_t));
    if (!buf) { h->err = "out of host memory (CIGAR runs)"; return WFM_E_NOMEM; }
    size_t at = 0;
    for (size_t k = 0; k < part_runs.size(); ++k) {
      if (!part_runs[k].empty()) memcpy(buf + at, part_runs[k].data(), part_runs[k].size() * sizeof(uint32_t));
      if (at) for (size_t i = cut[k]; i < cut[k + 1]; ++i) out[i].ops_off += at;
      at += part_runs[k].size();
    }
    *runs = buf;
    if (n_runs_total) *n_runs_total = total;
    return WFM_OK;
  };
  const bool overlap = !(getenv("WFM_OVERLAP") && atoi(getenv("WFM_OVERLAP")) == 0);  // read per call: bench.py times both forms
  if (hipSetDevice(h->device) != hipSuccess || hipEventRecord(h->ev_base, h->stream) != hipSuccess ||
      hipEventSynchronize(h->ev_base) != hipSuccess) { h->err = "hipEventRecord failed"; return WFM_E_HIP; }
  h->call_base = h->ev_base;
  h->prob_flags.assign(n + 1, 0u);  // (the parts of a call each write their own problems' entries)
  h->tile_iv.clear(); h->bp_iv.clear(); h->base_iv.clear();
  auto busy_ms = [](std::vector<std::pair<float, float>> iv) {  // length of the union of the intervals
    std::sort(iv.begin(), iv.end());
    double total = 0, lo = 0, hi = -1;
    for (const auto& x : iv) {
      if (x.first > hi) { if (hi > lo) total += hi - lo; lo = x.first; hi = x.second; }
      else hi = std::max<double>(hi, x.second);
    }
    if (hi > lo) total += hi - lo;
    return total;
  };
  h->mem_budget = h->mem_budget_full;
  auto keep_abs = [&](std::vector<std::pair<float, float>> iv) {  // the union as intervals on the device's own clock
    h->busy_abs.clear();
    double moved = 0;
    hipEvent_t db = device_base_event(h->device, &moved);
    float off_f = 0;
    const hipError_t ee = db ? hipEventElapsedTime(&off_f, db, h->ev_base) : hipErrorInvalidValue;
    const double off = moved + (double)off_f;
    if (ee != hipSuccess) {
      (void)hipGetLastError();
      if (getenv("WFM_DEBUG")) fprintf(stderr, "[wfm] busy intervals: no common clock (%s)\n", hipGetErrorString(ee));
      return;
    }
    std::sort(iv.begin(), iv.end());
    double lo = 0, hi = -1;
    for (const auto& x : iv) {
      if (x.first > hi) { if (hi > lo) h->busy_abs.emplace_back(off + lo, off + hi); lo = x.first; hi = x.second; }
      else hi = std::max<double>(hi, x.second);
    }
    if (hi > lo) h->busy_abs.emplace_back(off + lo, off + hi);
  };
  auto finish_single = [&](int rc) {
    h->stats.ms_tile_busy = busy_ms(h->tile_iv);
    h->stats.ms_bp_busy = busy_ms(h->bp_iv);
    h->stats.ms_base_busy = busy_ms(h->base_iv);
    std::vector<std::pair<float, float>> all = h->tile_iv;
    all.insert(all.end(), h->bp_iv.begin(), h->bp_iv.end());
    all.insert(all.end(), h->base_iv.begin(), h->base_iv.end());
    h->stats.ms_any_busy = busy_ms(all);
    keep_abs(all);
    h->stats.streams = 1;
    return rc;
  };
  auto run_single = [&]() {
    const int rc = finish_single(align_resident_impl(h, pen, s, 0, n, out, ops_arena, arena_bytes, 0, runs ? &part_runs[0] : nullptr, h->prob_flags.data()));
    if (rc < 0) return rc;
    const int hrc = hand_over_runs(std::vector<size_t>{0, n});
    return hrc != WFM_OK ? hrc : rc;
  };
  if (!overlap || n < 8) return run_single();
  // Parts of the batch side by side, each with its own stream and arenas (peer handles on the same device)
  // and its own host thread: while one part sits in the few-workgroup levels of the step kernel or waits for
  // the host, the other parts' tiles fill the machine.  Problems are independent, the parts only share the
  // (read-only) sequences and the caller's output buffers.
  static const int want = [] { const char* e = getenv("WFM_STREAMS"); return e ? std::max(1, std::min(8, atoi(e))) : 3; }();  // measured: 2 -> 124, 3 -> 120, 4 -> 160 ms on C3
  // every part needs room for its own arenas: no split below 256 MB per part
  size_t parts = std::min<size_t>(std::min<size_t>((size_t)want, n / 4), h->mem_budget_full >> 28);
  // A batch of hundreds of problems fills the device on its own -- its levels are thousands of workgroups wide -- and the
  // align driver keeps further batches in flight on handles of their own: such a batch runs as one part
  // -- when its problems come with score hints, i.e. from a driver that knows them to be near-identical records.  Hundreds of
  // problems nobody has said anything about (the strong-scaling bench at N = 1: 512 pairs at 5 %) are deep, run in many
  // chunks of full rings, and gain from parts as 64 of them do (512 pairs: 1136 ms as one part)
  if (!getenv("WFM_STREAMS") && n >= 512) {
    size_t hinted = 0, biwfa = 0;  // (patch calls -- ends-free problems only -- stay one part)
    for (size_t i = 0; i < n; ++i) { biwfa += s->meta[i].mode == WFM_MODE_END2END_BIWFA; hinted += s->meta[i].hint > 0; }
    // ... and only then: a batch that has the device to itself (a mapping file of one batch: LPA all-vs-all, a scaled pangenome rank) is a
    // chain of short launches per level and chunk, and three such chains side by side took its device time from 80 to 58 ms (C2) and from
    // 66 to 49 ms (scaled C4 rank) -- gpurun_out/r5b_ab.log, r5f_ab.log.  Patch calls are chains as well (budget 256 -> 1020 -> the rest).
    if (h->other_calls > 0 && (biwfa == 0 || hinted * 2 >= biwfa)) parts = 1;
  }
  if (!getenv("WFM_STREAMS") && parts > 2) {
    // a batch whose full rings would not fit the budget -- thousands of long records, which then run on narrow
    // rings -- is bound by the host's work between the many small launches: measured best with two parts
    // (C4-like records, 60 Mbp of queries: 2 -> 2.6 s, 3 -> 3.5 s)
    size_t ring_bytes = 0;
    for (size_t i = 0; i < n && ring_bytes <= h->mem_budget_full; ++i)
      // (an estimate of its own, not ring_elems of wfa_plan.h: the default depth whatever the penalties, no rounding to 16-byte chunks)
      ring_bytes += ((size_t)s->meta[i].plen + (size_t)s->meta[i].tlen + 9) * 2 * 5 * RING * 2 * 4;
    if (ring_bytes > h->mem_budget_full) parts = 2;
  }
  if (parts < 2) return run_single();
  while (h->peers.size() + 1 < parts) {
    wfm_handle_t* p = nullptr;
    if (wfm_create(h->device, &p) != WFM_OK) break;
    p->is_peer = true;
    { std::lock_guard<std::mutex> lk(g_base_mu); if (h->device < 64 && g_dev_handles[h->device] > 0) --g_dev_handles[h->device]; }
    h->peers.push_back(p);
  }
  const size_t np = h->peers.size() + 1;
  h->mem_budget = h->mem_budget_full / np;  // the parts share the primary handle's budget
  for (wfm_handle* pk : h->peers) pk->mem_budget = h->mem_budget;
  // contiguous parts of equal WFA cost, sum of (plen + tlen)^2
  std::vector<double> cost(n + 1, 0.0);
  for (size_t i = 0; i < n; ++i) {
    const double l = (double)s->meta[i].plen + (double)s->meta[i].tlen;
    cost[i + 1] = cost[i] + l * l;
  }
  std::vector<size_t> cut(np + 1, n);
  cut[0] = 0;
  for (size_t k = 1, i = 0; k < np; ++k) {
    while (i < n && cost[i] < cost[n] * (double)k / (double)np) ++i;
    cut[k] = std::min(std::max(i, cut[k - 1] + 1), n - (np - k));
  }
  std::vector<size_t> base(np, 0);
  for (size_t k = 1; k < np; ++k) {
    base[k] = base[k - 1];
    for (size_t i = cut[k - 1]; i < cut[k]; ++i) if (!s->meta[i].score_only()) base[k] += (size_t)s->meta[i].plen + (size_t)s->meta[i].tlen + 1;
  }
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<int> rcs(np, 0);
  std::vector<std::thread> th;
  part_runs.resize(np);
  for (size_t k = 1; k < np; ++k) {
    wfm_handle* pk = h->peers[k - 1];
    pk->call_base = h->ev_base;
    pk->tile_iv.clear(); pk->bp_iv.clear(); pk->base_iv.clear();
    th.emplace_back([&, k, pk] { rcs[k] = align_resident_impl(pk, pen, s, cut[k], cut[k + 1], out, ops_arena, arena_bytes, base[k], runs ? &part_runs[k] : nullptr, h->prob_flags.data()); });
  }
  rcs[0] = align_resident_impl(h, pen, s, cut[0], cut[1], out, ops_arena, arena_bytes, 0, runs ? &part_runs[0] : nullptr, h->prob_flags.data());
  for (auto& t : th) t.join();
  int failed = 0;
  for (size_t k = 0; k < np; ++k) {
    if (rcs[k] < 0) { if (k) h->err = h->peers[k - 1]->err; return rcs[k]; }
    failed += rcs[k];
  }
  {
    const int hrc = hand_over_runs(cut);
    if (hrc != WFM_OK) return hrc;
  }
  wfm_stats_t& a = h->stats;
  std::vector<std::pair<float, float>> iv = h->tile_iv, ivb = h->bp_iv, ivs = h->base_iv;
  for (size_t k = 1; k < np; ++k) {
    const wfm_stats_t& b = h->peers[k - 1]->stats;
    a.cells += b.cells; a.bytes_algorithmic += b.bytes_algorithmic; a.ms_kernels += b.ms_kernels; a.ms_breakpoint += b.ms_breakpoint;
    a.ms_base += b.ms_base; a.levels = std::max(a.levels, b.levels); a.bp_jobs += b.bp_jobs; a.base_jobs += b.base_jobs;
    a.bp_launches += b.bp_launches; a.base_launches += b.base_launches; a.cells_bp += b.cells_bp; a.cells_base += b.cells_base;
    a.p2_launches += b.p2_launches; a.p2_jobs += b.p2_jobs; a.p2_more += b.p2_more;
    a.cells_tile += b.cells_tile; a.ms_tile += b.ms_tile; a.tile_launches += b.tile_launches; a.tile_tasks += b.tile_tasks;
    a.cells_tile_unique += b.cells_tile_unique;
    for (int c = 0; c < WFM_TILE_COUNTERS; ++c) h->tile_ctr[c] += h->peers[k - 1]->tile_ctr[c];
    iv.insert(iv.end(), h->peers[k - 1]->tile_iv.begin(), h->peers[k - 1]->tile_iv.end());
    ivb.insert(ivb.end(), h->peers[k - 1]->bp_iv.begin(), h->peers[k - 1]->bp_iv.end());
    ivs.insert(ivs.end(), h->peers[k - 1]->base_iv.begin(), h->peers[k - 1]->base_iv.end());
  }
  a.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  a.ms_tile_busy = busy_ms(iv);
  a.ms_bp_busy = busy_ms(ivb);
  a.ms_base_busy = busy_ms(ivs);
  iv.insert(iv.end(), ivb.begin(), ivb.end());
  iv.insert(iv.end(), ivs.begin(), ivs.end());
  a.ms_any_busy = busy_ms(iv);
  keep_abs(iv);
  a.streams = (uint32_t)np;
  return failed;
}

int align_batch_any(wfm_handle_t* h, const wfm_penalties_t* pen, const wfm_problem_t* problems, size_t n,
                    wfm_result_t* out, char* ops_arena, size_t arena_bytes, uint32_t** runs, size_t* n_runs_total);
}  // namespace

int wfm_align_resident(wfm_handle_t* h, const wfm_penalties_t* pen, wfm_seqset_t* s, wfm_result_t* out,
                       char* ops_arena, size_t arena_bytes) {
  return align_resident_any(h, pen, s, out, ops_arena, arena_bytes, nullptr, nullptr);
}

int wfm_align_resident_rle(wfm_handle_t* h, const wfm_penalties_t* pen, wfm_seqset_t* s, wfm_result_t* out,
                           uint32_t** runs, size_t* n_runs_total) {
  if (!runs) return WFM_E_ARG;
  return align_resident_any(h, pen, s, out, nullptr, 0, runs, n_runs_total);
}

int wfm_align_refs_rle(wfm_handle_t* h, const wfm_penalties_t* pen, const wfm_seqstore_t* store, const wfm_problem_ref_t* refs, size_t n,
                       wfm_result_t* out, uint32_t** runs, size_t* n_runs_total) {
  if (!h || !runs) return WFM_E_ARG;
  *runs = nullptr;
  if (n_runs_total) *n_runs_total = 0;
  wfm_seqset_t* S = nullptr;
  int rc = wfm_upload_sequence_refs(h, store, refs, n, &S);
  if (rc != WFM_OK) return rc;
  rc = align_resident_any(h, pen, S, out, nullptr, 0, runs, n_runs_total);
  wfm_free_sequences(h, S);
  return rc;
}

int wfm_align_batch(wfm_handle_t* h, const wfm_penalties_t* pen, const wfm_problem_t* problems, size_t n,
                    wfm_result_t* out, char* ops_arena, size_t arena_bytes) {
  return align_batch_any(h, pen, problems, n, out, ops_arena, arena_bytes, nullptr, nullptr);
}

int wfm_align_batch_rle(wfm_handle_t* h, const wfm_penalties_t* pen, const wfm_problem_t* problems, size_t n,
                        wfm_result_t* out, uint32_t** runs, size_t* n_runs_total) {
  if (!runs) return WFM_E_ARG;
  return align_batch_any(h, pen, problems, n, out, nullptr, 0, runs, n_runs_total);
}

void wfm_free_runs(uint32_t* runs) { free(runs); }

// Self-test of the arenas' growth policy (DevBuf::ensure): capacities after ensure(n0), ensure(cap + 1), ensure(what fits): out3[0..2] in elements.
// A regrowth must at least double (every regrowth is a fresh hipMalloc at 30 - 70 ms per GB), a request that fits must not allocate.
int wfm_selftest_arena_growth(wfm_handle_t* h, size_t n0, size_t* out3) {
  if (!h || !out3 || n0 == 0) return WFM_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf<int32_t> b;
  if (b.ensure(n0)) return WFM_E_NOMEM;
  out3[0] = b.cap;
  if (b.ensure(b.cap + 1)) { b.release(); return WFM_E_NOMEM; }
  out3[1] = b.cap;
  const int32_t* before = b.p;
  if (b.ensure(b.cap - 1) || b.p != before) { b.release(); return WFM_E_HIP; }
  out3[2] = b.cap;
  b.release();
  return WFM_OK;
}

int wfm_selftest_dpp(wfm_handle_t* h, int32_t* out128) {
  if (!h || !out128) return WFM_E_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  return selftest_dpp(out128, h->stream) == 0 ? WFM_OK : WFM_E_HIP;
}

int wfm_score_bounds(wfm_handle_t* h, const wfm_penalties_t* pen, const wfm_problem_t* problems, size_t n, int32_t* out) {
  if (!h || !pen || !out || (n && !problems)) return WFM_E_ARG;
  if (n == 0) return WFM_OK;
  wfm_seqset_t* S = nullptr;
  int rc = wfm_upload_sequences(h, problems, n, &S);
  if (rc != WFM_OK) return rc;
  std::vector<BoundJob> bj(n);
  for (size_t i = 0; i < n; ++i) bj[i] = BoundJob{S->meta[i].p_fwd, S->meta[i].t_fwd, S->meta[i].plen, S->meta[i].tlen};
  auto run = [&]() -> int {
    if (h->bndjobs.ensure(n) || h->bndres.ensure(n)) { h->err = "out of device memory (score bounds)"; return WFM_E_NOMEM; }
    HIPCHK(h, hipMemcpyAsync(h->bndjobs.p, bj.data(), n * sizeof(BoundJob), hipMemcpyHostToDevice, h->stream));
    launch_bound(S->d_seq, h->bndjobs.p, h->bndres.p, (int)n, DevPen{pen->x, pen->o1, pen->e1, pen->o2, pen->e2}, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, h->bndres.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return WFM_OK;
  };
  rc = run();
  wfm_free_sequences(h, S);
  return rc;
}

namespace {
int align_batch_any(wfm_handle_t* h, const wfm_penalties_t* pen, const wfm_problem_t* problems, size_t n,
                    wfm_result_t* out, char* ops_arena, size_t arena_bytes, uint32_t** runs, size_t* n_runs_total) {
  if (!h) return WFM_E_ARG;
  if (runs) *runs = nullptr;
  if (n_runs_total) *n_runs_total = 0;
  wfm_seqset_t* S = nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  int rc = wfm_upload_sequences(h, problems, n, &S);
  if (rc != WFM_OK) return rc;
  const auto t1 = std::chrono::steady_clock::now();
  rc = align_resident_any(h, pen, S, out, ops_arena, arena_bytes, runs, n_runs_total);
  const auto t2 = std::chrono::steady_clock::now();
  wfm_free_sequences(h, S);
  if (getenv("WFM_DEBUG"))
    fprintf(stderr, "[wfm] align_batch: %zu problems, upload %.2f ms, align %.2f ms, free %.2f ms\n", n,
            std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count(),
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count());
  return rc;
}
}  // namespace

size_t wfm_get_busy_intervals(const wfm_handle_t* h, double* start_end_ms, size_t cap) {
  if (!h) return 0;
  const size_t n = h->busy_abs.size();
  for (size_t i = 0; i < n && i < cap && start_end_ms; ++i) { start_end_ms[2 * i] = h->busy_abs[i].first; start_end_ms[2 * i + 1] = h->busy_abs[i].second; }
  return n;
}

int wfm_get_stats(const wfm_handle_t* h, wfm_stats_t* out) {
  if (!h || !out) return WFM_E_ARG;
  *out = h->stats;
  return WFM_OK;
}

}  // extern "C"

#include "wfa_handle.h"
hipStream_t wfm_stream(wfm_handle_t* h) { return h->stream; }
int wfm_device(const wfm_handle_t* h) { return h->device; }
void wfm_set_error(wfm_handle_t* h, const std::string& msg) {
  static std::mutex mu;  // several host threads may work on one handle (the device winnower next to the hashing thread)
  std::lock_guard<std::mutex> lk(mu);
  h->err = msg;
}
void* wfm_attachment(wfm_handle_t* h) { return h->attachment; }
void wfm_set_attachment(wfm_handle_t* h, void* p, void (*destroy)(void*)) {
  if (h->attachment && h->attachment_free && h->attachment != p) h->attachment_free(h->attachment);
  h->attachment = p;
  h->attachment_free = destroy;
}
