// wfa_passes.hip -- the record passes of the C ABI (see include/wfmash_hip.h): host code that takes the final runs of a batch and
// produces something from them -- the check against the bases, left-aligned gaps, cs strings, variants, the rows of a MAF, target depth, lifted
// intervals, the blocks of a chain, presence per group, the sites and genotypes of many records, the net across records, the closure of
// intervals over all records, the proof of optimality.
// The kernels are in wfa_check.hip, wfa_leftalign.hip, wfa_cs.hip, wfa_variants.hip, wfa_coverage.hip, wfa_lift.hip, wfa_chain.hip,
// wfa_pav.hip, wfa_sites.hip, wfa_net.hip, wfa_trans.hip, wfa_maf.hip and wfa_optcheck.hip.
//
// Every pass has the same frame, written once below: it validates the run ranges before anything is launched, carves what the
// call has on the device out of one block, launches, writes its output in chunks that fit a cap, and waits for the stream before
// it returns (so one scratch block and one output block of the handle serve all of them).  The adds of the accumulating objects open with
// add_preface; the five passes that emit lists (cs, variants, maf, lift, chain) are callers of emit_lists, which owns the sequence from the
// carve to the caller's buffers; the chunk plan itself is wfa_emit_plan.h, without a device header.
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "wfa_emit_plan.h"
#include "wfa_host_shared.h"
#include "wfa_optband.h"

namespace {

using namespace wfm;

double env_decimal(const char* name, double dflt) { const char* e = getenv(name); return e && *e ? atof(e) : dflt; }
// a cap given in MiB by the environment (a fraction is fine), in units of `unit` bytes, `least` at least
unsigned long long cap_units(const char* name, size_t unit, unsigned long long least) {
  return std::max<unsigned long long>(least, (unsigned long long)(std::max(0.0, env_decimal(name, 256.0)) * 1048576.0) / unit);
}

// ---- the frame ----

// Typed, 8-byte aligned pieces of one device block: piece() notes where each will lie, commit() sizes the block for their sum and
// sets the pointers.  `pass` is what the out-of-memory text names.
struct Carver {
  DevBuf<uint64_t>& buf;
  const char* pass;
  struct Slot { void* pp; size_t at; void (*set)(void* pp, uint64_t* at); };
  Slot slots[16];
  int n = 0;
  size_t words = 0;
  static size_t words64(size_t bytes) { return (bytes + 7) / 8; }
  template <class T>
  void piece(T** p, size_t count) {
    slots[n++] = Slot{p, words, [](void* pp, uint64_t* at) { *(T**)pp = (T*)at; }};
    words += words64(count * sizeof(T));
  }
  int commit(wfm_handle_t* h) {
    if (buf.ensure(words + 8)) { h->err = std::string("out of device memory (") + pass + ")"; return WFM_E_NOMEM; }
    for (int k = 0; k < n; ++k) slots[k].set(slots[k].pp, buf.p + slots[k].at);
    return WFM_OK;
  }
};

// room for `need` elements of a block that holds `have`; what it holds moves with it
template <class T>
int grow_block(wfm_handle_t* h, T** blk, size_t* cap, size_t have, size_t need, const char* what) {
  if (need <= *cap) return WFM_OK;
  const size_t ncap = std::max<size_t>(need + need / 2, 4096);
  T* nb = nullptr;
  if (wfm_dmalloc((void**)&nb, ncap * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); h->err = std::string("out of device memory (") + what + ")"; return WFM_E_NOMEM; }
  if (have) {
    hipError_t e = hipMemcpyAsync(nb, *blk, have * sizeof(T), hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { wfm_dfree(nb); h->err = std::string(what) + ": " + hipGetErrorString(e); return WFM_E_HIP; }
  }
  if (*blk) wfm_dfree(*blk);
  *blk = nb;
  *cap = ncap;
  return WFM_OK;
}

inline bool runs_inside(uint64_t off, uint64_t n_runs, size_t n_runs_total) { return off <= n_runs_total && n_runs <= n_runs_total - off; }
int runs_leave(wfm_handle_t* h, size_t i) {
  h->err = "problem " + std::to_string(i) + ": its runs leave the run buffer";
  return WFM_E_ARG;
}
// every problem's range of a list of wfm_cov_prob_t / wfm_pav_prob_t, before anything is launched
template <class P>
int all_runs_inside(wfm_handle_t* h, const P* probs, size_t n, size_t n_runs_total) {
  for (size_t i = 0; i < n; ++i)
    if (!runs_inside(probs[i].runs_off, probs[i].n_runs, n_runs_total)) return runs_leave(h, i);
  return WFM_OK;
}

// What CheckProb, LaProb, CsProb and OptProb share: the forward copies and their lengths; whether the problem has nothing for the pass
// (score-only, status != 0, and for all but the check a result without runs)
template <class P>
void fill_seq(P& c, const ProbMeta& m) { c.p_off = m.p_fwd; c.t_off = m.t_fwd; c.plen = m.plen; c.tlen = m.tlen; }
template <class P>
void fill_ends(P& c, const ProbMeta& m) { c.pbf = m.pbf; c.pef = m.pef; c.tbf = m.tbf; c.tef = m.tef; }  // (0 unless the mode is ENDSFREE: layout_seqset)
template <class P>
void fill_prob(P& c, const ProbMeta& m, const wfm_result_t& r, bool skip_without_runs) {
  fill_seq(c, m);
  c.skip = (m.score_only() || r.status != 0 || (skip_without_runs && r.n_runs == 0)) ? 1 : 0;
}

// An object of a device: usable() refuses a handle of another device; a guard makes the object's device current while it is freed
struct DeviceGuard {
  int cur = 0;
  bool swap = false;
  explicit DeviceGuard(int device) { swap = hipGetDevice(&cur) == hipSuccess && cur != device; if (swap) (void)hipSetDevice(device); }
  ~DeviceGuard() { if (swap) (void)hipSetDevice(cur); }
  static int usable(wfm_handle_t* h, int device, const char* what) {
    if (device == h->device) return WFM_OK;
    h->err = std::string(what) + " lives on device " + std::to_string(device) + ", the handle on " + std::to_string(h->device);
    return WFM_E_ARG;
  }
};

// What the adds that take runs (wfm_coverage_add, wfm_pav_add, wfm_net_add, wfm_trans_add; fn names the one) open with: the argument and
// size checks, the object on the handle's device, every problem's runs inside the buffer, the device made current, the problems (DevProb
// restates P for the kernels) and the runs carved first out of cv's block and uploaded.  more(): what the pass checks and carves beside
// them, before the block is sized.  Without problems *d_probs stays null and the caller returns.
template <class DevProb, class P, class More>
int add_preface(wfm_handle_t* h, const void* obj, int device, const char* what, const char* fn, Carver& cv, const P* probs, size_t n, const uint32_t* runs,
                size_t n_runs_total, const uint32_t* flags_out, DevProb** d_probs, uint32_t** d_runs, More more) {
  static_assert(sizeof(DevProb) == sizeof(P), "the kernels' problem restates the header's");
  *d_probs = nullptr;
  if (!h || !obj || (n && (!probs || !flags_out)) || (n_runs_total && !runs)) return WFM_E_ARG;
  if (n == 0) return WFM_OK;
  if (n > (size_t)INT32_MAX || n_runs_total > ((size_t)1 << 31)) { h->err = std::string(fn) + ": too many problems or runs for one call"; return WFM_E_ARG; }
  if (int rc = DeviceGuard::usable(h, device, what)) return rc;
  if (int rc = all_runs_inside(h, probs, n, n_runs_total)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  cv.piece(d_probs, n); cv.piece(d_runs, n_runs_total);
  if (int rc = more()) return rc;
  if (int rc = cv.commit(h)) return rc;
  HIPCHK(h, hipMemcpyAsync(*d_probs, probs, n * sizeof(DevProb), hipMemcpyHostToDevice, h->stream));
  if (n_runs_total) HIPCHK(h, hipMemcpyAsync(*d_runs, runs, n_runs_total * 4, hipMemcpyHostToDevice, h->stream));
  return WFM_OK;
}
inline int count_flagged(const uint32_t* flags, size_t n, uint32_t bit) { return (int)std::count_if(flags, flags + n, [bit](uint32_t f) { return (f & bit) != 0; }); }

// The union of n intervals given by their start keys ks and end keys ke (below 2^end_bit): sorted by start into (sks, ske), the ends to
// their running maximum, the union's intervals to (uks, uke) and their number to *m, read back behind a wait for the stream.  aux: n /
// WFM_PAV_SCAN_BLOCK rounded up, + 1; tmp: the sort's own (oom: the text where it cannot grow).  between(): what the caller does once the
// running maximum is launched, before the compaction.
template <class Between>
int interval_union(wfm_handle_t* h, DevBuf<uint64_t>& tmp, const char* oom, const unsigned long long* ks, const unsigned long long* ke, unsigned long long* sks,
                   unsigned long long* ske, size_t n, unsigned end_bit, unsigned long long* aux, unsigned long long* uks, unsigned long long* uke,
                   unsigned long long* m, Between between) {
  size_t tmp_bytes = 0;
  HIPCHK(h, pav_sort(nullptr, &tmp_bytes, ks, sks, ke, ske, n, end_bit, h->stream));
  if (tmp.ensure(tmp_bytes / 8 + 2)) { h->err = oom; return WFM_E_NOMEM; }
  HIPCHK(h, pav_sort(tmp.p, &tmp_bytes, ks, sks, ke, ske, n, end_bit, h->stream));
  launch_pav_runmax(ske, n, aux, h->stream);
  HIPCHK(h, hipGetLastError());
  if (int rc = between()) return rc;
  launch_pav_compact(sks, ske, n, aux, uks, uke, h->stream);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(m, aux + (n + WFM_PAV_SCAN_BLOCK - 1) / WFM_PAV_SCAN_BLOCK, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return WFM_OK;
}

// The times of the [wfm] lines: the host clock from the construction or the last lap(), and the handle's two events around a launch.
// on: WFM_DEBUG is set; without it nothing is recorded.
struct PassTimer {
  wfm_handle_t* h;
  bool on = env_debug() != 0;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), t_lap = t0;
  explicit PassTimer(wfm_handle_t* h_) : h(h_) {}
  bool pending = false;  // the events were recorded and not read since
  hipError_t begin() { pending = on; return on ? hipEventRecord(h->ev0, h->stream) : hipSuccess; }
  hipError_t end() { return on ? hipEventRecord(h->ev1, h->stream) : hipSuccess; }
  // launch() between the two events; the first error of the three
  template <class Launch>
  hipError_t timed(Launch launch) {
    hipError_t e = begin();
    if (e != hipSuccess) return e;
    launch();
    e = hipGetLastError();
    return e != hipSuccess ? e : end();
  }
  bool event_ms(float* ms) {  // (behind a wait for the stream; false where nothing was recorded since the last reading)
    if (!pending) return false;
    pending = false;
    if (hipEventElapsedTime(ms, h->ev0, h->ev1) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
  }
  double host_ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
  double lap() {
    const auto t = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(t - t_lap).count();
    t_lap = t;
    return ms;
  }
};

// How a device block reaches the caller's buffer: the chunks of the five emitting passes (emit_lists below), the exports and tables of the
// accumulating objects and wfm_pav_matrix.
constexpr size_t PIN_PIECE = (size_t)4 << 20;

// the handle's two pinned pieces, allocated at first use; false: there are none, and a block goes down in one pageable copy
bool pin_pieces(wfm_handle_t* h) {
  for (int k = 0; k < 2; ++k)
    if (!h->cspin[k] && hipHostMalloc((void**)&h->cspin[k], PIN_PIECE, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); h->cspin[k] = nullptr; return false; }
  return true;
}

// bytes of the device block src to dst, finished on return.  Down in pieces through the two pinned buffers: piece j + 1 crosses PCIe while
// piece j is copied to its place (one pageable hipMemcpy of a fresh block took 2 ms for 3.7 MB, and 18 - 28 ms every other call:
// profiles/cs_tag.md)
hipError_t copy_down(wfm_handle_t* h, bool pinned, char* dst, const uint8_t* src, size_t bytes) {
  if (bytes == 0) return hipSuccess;
  hipError_t e = hipSuccess;
  const size_t pieces = pinned ? (bytes + PIN_PIECE - 1) / PIN_PIECE : 0;
  auto piece_len = [&](size_t j) { return std::min<size_t>(PIN_PIECE, bytes - j * PIN_PIECE); };
  if (!pinned) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream);
  if (pinned) e = hipMemcpyAsync(h->cspin[0], src, piece_len(0), hipMemcpyDeviceToHost, h->stream);
  for (size_t j = 0; j < pieces && e == hipSuccess; ++j) {
    e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess && j + 1 < pieces)
      e = hipMemcpyAsync(h->cspin[(j + 1) & 1], src + (j + 1) * PIN_PIECE, piece_len(j + 1), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) memcpy(dst + j * PIN_PIECE, h->cspin[j & 1], piece_len(j));
  }
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  return e;
}

// ---- the emit frame: the passes that index their problems, learn from the totals how much each one emits, and write lists in chunks
// (wfm_cs_strings, wfm_call_variants, wfm_maf_rows, wfm_lift_runs, wfm_chain_runs) ----

inline int hip_rc(wfm_handle_t* h, const char* fn, hipError_t e) {
  if (e == hipSuccess) return WFM_OK;
  h->err = std::string(fn) + ": " + hipGetErrorString(e);
  return WFM_E_HIP;
}
inline char* plain_alloc(size_t bytes) { return (char*)malloc(bytes); }
struct FreeHost { void operator()(char* p) const { free(p); } };

// One list a pass emits.  A chunk's part of it lies in the output block behind the streams before it, on `round` bytes of its own
struct EmitStream {
  const std::vector<unsigned long long>& off;  // n + 1 offsets in elements: the host's prefix sums, valid once offsets() has run
  size_t elem;                                 // bytes an element
  size_t round;                                // its part of the block is a whole number of these
  char* (*alloc)(size_t);                      // the caller's buffer (released with free)
  void** out;                                  // where the caller receives it ...
  size_t* count;                               // ... and its number of elements
};
struct EmitSpec {
  const char* fn;                              // the entry point, in the texts of HIP errors
  const char *tag, *host_tag, *out_tag;        // what the out-of-memory texts name: the scratch block, the caller's buffers, the output block
  DevBuf<uint64_t>&scratch, &outblk;
  unsigned long long cap;                      // bytes of the streams a chunk may hold (one problem may exceed it alone)
};
struct EmitStats { size_t chunks = 0; float ms_index = 0, ms_write = 0; };  // (the times: device events, 0 without WFM_DEBUG or where a pass records none)

// carve(cv): the pieces of the scratch block (those read 16 bytes at a time first: Carver aligns to 8).  index(down): the uploads, the index
// launch, and down(dst, src, bytes) for what the host needs of it; the frame waits for that.  offsets(): the totals to prefix sums and per[],
// the offsets' upload where there is output; below 0 an error, otherwise what the call returns.  A call without output ends there, its
// outputs as the caller cleared them.  Otherwise: the caller's buffers, the plan of chunks under the cap, the output block sized once for
// the widest, and per chunk write(ka, kb, d), which launches with stream s at d[s] and returns WFM_OK or its error, then every stream down
// to its place.  The buffers are the caller's only when all of it succeeded.  A pass that records no events has no event times.
template <size_t S, class Carve, class Index, class Offsets, class Write>
int emit_lists(wfm_handle_t* h, PassTimer& tm, const EmitSpec& sp, size_t n, const EmitStream (&streams)[S], Carve carve, Index index, Offsets offsets,
               Write write, EmitStats* st) {
  Carver cv{sp.scratch, sp.tag};
  carve(cv);
  if (int rc = cv.commit(h)) return rc;
  hipError_t e_down = hipSuccess;
  auto down = [&](void* dst, const void* src, size_t bytes) { if (e_down == hipSuccess) e_down = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream); };
  if (int rc = index(down)) return rc;
  if (int rc = hip_rc(h, sp.fn, e_down)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  (void)tm.event_ms(&st->ms_index);
  const int ret = offsets();
  if (ret < 0) return ret;
  auto bytes_of = [&](size_t s, size_t ka, size_t kb) { return (size_t)(streams[s].off[kb] - streams[s].off[ka]) * streams[s].elem; };
  auto part_of = [&](size_t s, size_t ka, size_t kb) { return (bytes_of(s, ka, kb) + streams[s].round - 1) / streams[s].round * streams[s].round; };
  auto cost = [&](size_t ka, size_t kb) { unsigned long long c = 0; for (size_t s = 0; s < S; ++s) c += bytes_of(s, ka, kb); return c; };
  auto block = [&](size_t ka, size_t kb) { unsigned long long b = 0; for (size_t s = 0; s < S; ++s) b += part_of(s, ka, kb); return b; };
  if (cost(0, n) == 0) return ret;
  std::unique_ptr<char, FreeHost> host[S];
  bool got = true;
  for (size_t s = 0; s < S; ++s) { host[s].reset(streams[s].alloc(bytes_of(s, 0, n))); got = got && host[s]; }
  if (!got) { (void)hipStreamSynchronize(h->stream); h->err = std::string("out of host memory (") + sp.host_tag + ")"; return WFM_E_NOMEM; }
  const EmitPlan plan = emit_plan(n, sp.cap, cost, block);
  if (sp.outblk.ensure((size_t)(plan.widest + 7) / 8)) { h->err = std::string("out of device memory (") + sp.out_tag + ")"; return WFM_E_NOMEM; }
  const bool pinned = pin_pieces(h);
  for (const auto& c : plan.chunks) {
    const size_t ka = c.first, kb = c.second;
    uint8_t* d[S];
    size_t at = 0;
    for (size_t s = 0; s < S; ++s) { d[s] = (uint8_t*)sp.outblk.p + at; at += part_of(s, ka, kb); }
    if (int rc = write(ka, kb, d)) return rc;
    hipError_t e = hipSuccess;
    for (size_t s = 0; s < S && e == hipSuccess; ++s)  // (the block is the next chunk's)
      e = copy_down(h, pinned, host[s].get() + streams[s].off[ka] * streams[s].elem, d[s], bytes_of(s, ka, kb));
    if (int rc = hip_rc(h, sp.fn, e)) return rc;
    float ms = 0;
    if (tm.event_ms(&ms)) st->ms_write += ms;
  }
  st->chunks = plan.chunks.size();
  for (size_t s = 0; s < S; ++s) { *streams[s].count = (size_t)streams[s].off[n]; *streams[s].out = host[s].release(); }
  return ret;
}

}  // namespace

extern "C" {

// ---- every run held against its bases (wfmash_hip.h; the kernels: wfa_check.hip) ----
int wfm_check_runs(wfm_handle_t* h, const wfm_penalties_t* pen, const wfm_seqset_t* s, const wfm_result_t* res, const uint32_t* runs,
                   size_t n_runs_total, wfm_check_t* out) {
  if (!h || !s || !out || !res || (n_runs_total && !runs)) return WFM_E_ARG;
  int scope = 0;
  if (const int prc = validate_pen(pen, &scope)) { h->err = "unsupported penalties"; return prc; }
  const size_t n = s->meta.size();
  if (n == 0) return 0;
  if (n > (size_t)INT32_MAX || n_runs_total > ((size_t)1 << 32)) { h->err = "wfm_check_runs: too many problems or runs for one call"; return WFM_E_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  // the problems as the kernels see them; the run ranges are validated here, before anything is launched
  std::vector<CheckProb> probs(n);
  std::vector<CheckTask> tasks;
  for (size_t i = 0; i < n; ++i) {
    const ProbMeta& m = s->meta[i];
    CheckProb& c = probs[i];
    fill_prob(c, m, res[i], false);  // (a result without runs is checked like any other)
    fill_ends(c, m);
    c.res_score = res[i].score; c.res_ops_len = res[i].ops_len;
    c.run_off = 0; c.n_runs = 0;
    if (c.skip) continue;
    if (!runs_inside(res[i].ops_off, res[i].n_runs, n_runs_total)) return runs_leave(h, i);
    c.run_off = res[i].ops_off; c.n_runs = res[i].n_runs;
    // (compared runs spell at most plen + tlen ops: a slice beyond what the scan finds ends at once)
    const int64_t slices = ((int64_t)m.plen + m.tlen + WFM_CHECK_SLICE - 1) / WFM_CHECK_SLICE;
    for (int64_t q = 0; q < slices; ++q) tasks.push_back(CheckTask{(int32_t)i, (int32_t)q});
  }
  // one block: [runs | ops_pre | p_pre | t_pre | cmp_ops] as 32-bit words, then keys, results, problems and tasks (8-byte aligned each)
  const size_t nr = n_runs_total;
  uint32_t *d_runs, *d_opre, *d_ppre, *d_tpre, *d_cmp;
  unsigned long long* d_keys;
  wfm_check_t* d_out;
  CheckProb* d_probs;
  CheckTask* d_tasks;
  Carver cv{h->scratch, "run check"};
  cv.piece(&d_runs, nr); cv.piece(&d_opre, nr); cv.piece(&d_ppre, nr); cv.piece(&d_tpre, nr); cv.piece(&d_cmp, n);
  cv.piece(&d_keys, n); cv.piece(&d_out, n); cv.piece(&d_probs, n); cv.piece(&d_tasks, tasks.size());
  if (int rc = cv.commit(h)) return rc;
  if (nr) HIPCHK(h, hipMemcpyAsync(d_runs, runs, nr * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_probs, probs.data(), n * sizeof(CheckProb), hipMemcpyHostToDevice, h->stream));
  if (!tasks.empty()) HIPCHK(h, hipMemcpyAsync(d_tasks, tasks.data(), tasks.size() * sizeof(CheckTask), hipMemcpyHostToDevice, h->stream));
  PassTimer tm(h);
  HIPCHK(h, tm.begin());
  launch_check(s->d_seq, d_runs, d_probs, (int)n, d_tasks, (int64_t)tasks.size(), d_opre, d_ppre, d_tpre, d_cmp, d_keys, d_out,
               DevPen{pen->x, pen->o1, pen->e1, pen->o2, pen->e2}, h->stream);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, tm.end());
  HIPCHK(h, hipMemcpyAsync(out, d_out, n * sizeof(wfm_check_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0;
  if (tm.event_ms(&ms))
    fprintf(stderr, "[wfm] run check: %zu problems, %zu runs, %zu compare tasks, %llu bases of sequence in %.3f ms\n", n, nr, tasks.size(),
            (unsigned long long)s->seq_bases, ms);
  int flagged = 0;
  for (size_t i = 0; i < n; ++i) flagged += (out[i].flags & ~WFM_CK_NOT_CHECKED) != 0;
  return flagged;
}

// ---- every interior gap moved to its leftmost placement (wfmash_hip.h; the kernels: wfa_leftalign.hip) ----
int wfm_left_align_runs(wfm_handle_t* h, const wfm_seqset_t* s, wfm_result_t* res, const uint32_t* runs, size_t n_runs_total, uint32_t** runs_out,
                        size_t* n_runs_out_total, wfm_leftalign_t* out) {
  if (!h || !s || !out || !res || !runs_out || (n_runs_total && !runs)) return WFM_E_ARG;
  *runs_out = nullptr;
  if (n_runs_out_total) *n_runs_out_total = 0;
  const size_t n = s->meta.size();
  if (n == 0) return 0;
  if (n > (size_t)INT32_MAX || n_runs_total > ((size_t)1 << 31)) { h->err = "wfm_left_align_runs: too many problems or runs for one call"; return WFM_E_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  // the problems as the kernels see them; the run ranges are validated here, before anything is launched.  The interior gaps are counted on the
  // way (the runs are in host memory and are read once for the upload anyway): a problem's slots in the output and in the gap list follow from it
  std::vector<LaProb> probs(n);
  uint64_t out_total = 0, gap_total = 0;
  for (size_t i = 0; i < n; ++i) {
    const ProbMeta& m = s->meta[i];
    LaProb& c = probs[i];
    memset(&c, 0, sizeof(c));
    fill_prob(c, m, res[i], true);
    const bool inside = runs_inside(res[i].ops_off, res[i].n_runs, n_runs_total);
    if (!c.skip && !inside) return runs_leave(h, i);
    if (inside) { c.run_off = res[i].ops_off; c.n_runs = res[i].n_runs; }  // (a problem that is not done keeps the runs it names, if it names any)
    if (!c.skip)
      for (uint32_t r = 1; r + 1 < c.n_runs; ++r) c.n_gaps += WFM_RUN_OP(runs[c.run_off + r]) >= 2u;
    c.out_off = out_total; c.gap_off = gap_total;
    out_total += (uint64_t)c.n_runs + c.n_gaps;
    gap_total += c.n_gaps;
  }
  // one block: [runs | rot | dval] one word per run, [out] one per output slot, [flags] one per problem, [long list] one per gap, the counter;
  // then the gap records, the problems and the results (8-byte aligned each)
  const size_t nr = n_runs_total;
  uint32_t *d_runs, *d_rot, *d_dval, *d_out, *d_flags, *d_count;
  LaGap* d_gaps;
  LaProb* d_probs;
  wfm_leftalign_t* d_stats;
  Carver cv{h->scratch, "left-align"};
  cv.piece(&d_runs, nr); cv.piece(&d_rot, nr); cv.piece(&d_dval, nr); cv.piece(&d_out, out_total); cv.piece(&d_flags, n);
  cv.piece(&d_count, gap_total + 2);  // (the counter's 8 bytes, then the long list)
  cv.piece(&d_gaps, gap_total); cv.piece(&d_probs, n); cv.piece(&d_stats, n);
  if (int rc = cv.commit(h)) return rc;
  uint32_t* d_long = d_count + 2;
  if (nr) HIPCHK(h, hipMemcpyAsync(d_runs, runs, nr * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_probs, probs.data(), n * sizeof(LaProb), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(d_count, 0, 8, h->stream));
  if (gap_total) HIPCHK(h, hipMemsetAsync(d_gaps, 0xff, gap_total * sizeof(LaGap), h->stream));  // (a record nobody writes names no problem)
  PassTimer tm(h);
  const uint32_t lane_max = (uint32_t)std::max(8, env_num("WFM_LA_LANE_MAX", 256));
  HIPCHK(h, tm.begin());
  launch_left_align(s->d_seq, d_runs, d_probs, (int)n, d_rot, d_dval, d_gaps, gap_total, d_flags, d_long, d_count, d_out, d_stats, lane_max, h->stream);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, tm.end());
  std::vector<uint32_t> slots(out_total);
  uint32_t n_long = 0;
  if (out_total) HIPCHK(h, hipMemcpyAsync(slots.data(), d_out, out_total * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(out, d_stats, n * sizeof(wfm_leftalign_t), hipMemcpyDeviceToHost, h->stream));
  if (tm.on) HIPCHK(h, hipMemcpyAsync(&n_long, d_count, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // the problems' runs end to end (a problem used at most n_runs + n_gaps of its slots)
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) {
    if (out[i].runs_out > probs[i].n_runs + probs[i].n_gaps) { h->err = "wfm_left_align_runs: a problem's runs outgrew their slots"; return WFM_E_HIP; }
    total += out[i].runs_out;
  }
  uint32_t* packed = (uint32_t*)malloc(std::max<size_t>(total, 1) * 4);
  if (!packed) { h->err = "out of host memory (left-align)"; return WFM_E_NOMEM; }
  uint64_t pos = 0;
  int spans = 0;
  uint64_t moved = 0, bases = 0;
  for (size_t i = 0; i < n; ++i) {
    if (out[i].runs_out) memcpy(packed + pos, slots.data() + probs[i].out_off, (size_t)out[i].runs_out * 4);
    res[i].ops_off = pos; res[i].n_runs = out[i].runs_out;
    pos += out[i].runs_out;
    spans += (out[i].flags & WFM_LA_SPANS) != 0;
    moved += out[i].moved; bases += out[i].bases_moved;
  }
  *runs_out = packed;
  if (n_runs_out_total) *n_runs_out_total = (size_t)total;
  float ms = 0;
  if (tm.event_ms(&ms))
    fprintf(stderr, "[wfm] left-align: %zu problems, %zu runs, %llu gaps (%u to the wave kernel), %llu moved by %llu bases in %.3f ms\n", n, nr,
            (unsigned long long)gap_total, n_long, (unsigned long long)moved, (unsigned long long)bases, ms);
  return spans;
}

namespace {
// the problems as wfa_cs.hip, wfa_variants.hip and wfa_maf.hip see them; the run ranges are validated here, before anything is launched.  The
// run records lie in problem order whatever order the runs come in, `slack` slots behind each problem's (wfa_maf.hip: one, for its totals)
int cs_problems(wfm_handle_t* h, const wfm_seqset_t* s, const wfm_result_t* res, size_t n_runs_total, unsigned slack, std::vector<CsProb>& probs, uint64_t* rec_total) {
  const size_t n = s->meta.size();
  probs.resize(n);
  for (size_t i = 0; i < n; ++i) {
    CsProb& c = probs[i];
    memset(&c, 0, sizeof(c));
    fill_prob(c, s->meta[i], res[i], true);
    if (c.skip) continue;
    if (!runs_inside(res[i].ops_off, res[i].n_runs, n_runs_total)) return runs_leave(h, i);
    c.run_off = res[i].ops_off; c.n_runs = res[i].n_runs;
    c.rec_off = *rec_total;
    *rec_total += (uint64_t)c.n_runs + slack;
  }
  return WFM_OK;
}
}  // namespace

// ---- the cs difference string of every problem's runs (wfmash_hip.h; the kernels: wfa_cs.hip) ----
int wfm_cs_strings(wfm_handle_t* h, const wfm_seqset_t* s, const wfm_result_t* res, const uint32_t* runs, size_t n_runs_total, int form, char** out,
                   size_t* out_bytes, wfm_cs_t* per) {
  if (!h || !s || !out || !out_bytes || (n_runs_total && !runs)) return WFM_E_ARG;
  *out = nullptr;
  *out_bytes = 0;
  PassTimer tm(h);
  if (form != WFM_CS_SHORT && form != WFM_CS_LONG) { h->err = "wfm_cs_strings: form " + std::to_string(form) + " is neither WFM_CS_SHORT nor WFM_CS_LONG"; return WFM_E_ARG; }
  const size_t n = s->meta.size();
  if (n == 0) return WFM_OK;
  if (!res || !per) return WFM_E_ARG;
  if (n > (size_t)INT32_MAX || n_runs_total > ((size_t)1 << 31)) { h->err = "wfm_cs_strings: too many problems or runs for one call"; return WFM_E_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<CsProb> probs;
  uint64_t rec_total = 0;
  if (int rc = cs_problems(h, s, res, n_runs_total, 0, probs, &rec_total)) return rc;
  // one block: [records] 16 bytes per run, [offsets] n + 1 and [totals] n of 8 bytes, [problems], [runs], [flags]
  const size_t nr = n_runs_total;
  uint4* d_recs;
  unsigned long long *d_goff, *d_tot;
  CsProb* d_probs;
  uint32_t *d_runs, *d_flags;
  std::vector<unsigned long long> goff(n + 1);
  std::vector<uint32_t> flags(n);
  int spans = 0;
  // chunks of problems whose strings fit the output block (a problem larger than that is a chunk of its own)
  const EmitSpec sp{"wfm_cs_strings", "cs", "cs", "cs output", h->scratch, h->outblk, (unsigned long long)std::max(1, env_num("WFM_CS_OUT_MB", 256)) << 20};
  const EmitStream streams[] = {{goff, 1, WFM_CS_SLICE, plain_alloc, (void**)out, out_bytes}};
  EmitStats st;
  const int rc = emit_lists(
      h, tm, sp, n, streams,
      [&](Carver& cv) { cv.piece(&d_recs, (size_t)rec_total); cv.piece(&d_goff, n + 1); cv.piece(&d_tot, n); cv.piece(&d_probs, n); cv.piece(&d_runs, nr); cv.piece(&d_flags, n); },
      [&](auto down) {
        if (nr) HIPCHK(h, hipMemcpyAsync(d_runs, runs, nr * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_probs, probs.data(), n * sizeof(CsProb), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, tm.timed([&] { launch_cs_index(d_runs, d_probs, (int)n, form, d_recs, d_tot, d_flags, h->stream); }));
        down(goff.data() + 1, d_tot, n * 8); down(flags.data(), d_flags, n * 4);
        return WFM_OK;
      },
      [&]() {  // the problems' totals, once: the host takes their prefix sum
        goff[0] = 0;
        for (size_t i = 0; i < n; ++i) {
          per[i].flags = flags[i]; per[i].n_runs = probs[i].n_runs;
          per[i].off = goff[i]; per[i].len = goff[i + 1];
          goff[i + 1] += goff[i];
          spans += (flags[i] & WFM_CS_SPANS) != 0;
        }
        if (goff[n]) HIPCHK(h, hipMemcpyAsync(d_goff, goff.data(), (n + 1) * 8, hipMemcpyHostToDevice, h->stream));
        return spans;
      },
      [&](size_t ka, size_t kb, uint8_t* const* d) {
        return hip_rc(h, sp.fn, tm.timed([&] { launch_cs_write(s->d_seq, d_probs, d_recs, d_goff, (uint32_t)ka, (uint32_t)kb, goff[kb] - goff[ka], form, d[0], h->stream); }));
      },
      &st);
  if (tm.on && st.chunks)
    fprintf(stderr, "[wfm] cs (%s): %zu problems, %zu runs, %llu bytes in %zu chunks, index %.3f ms, write %.3f ms (device events), the call %.3f ms (host clock)\n",
            form == WFM_CS_LONG ? "long" : "short", n, (size_t)rec_total, goff[n], st.chunks, st.ms_index, st.ms_write, tm.host_ms());
  return rc;
}

void wfm_free_cs(char* p) { free(p); }

// ---- the variants of every problem's runs (wfmash_hip.h; the kernels: wfa_variants.hip) ----
int wfm_call_variants(wfm_handle_t* h, const wfm_seqset_t* s, const wfm_result_t* res, const uint32_t* runs, size_t n_runs_total, wfm_variant_t** vars,
                      size_t* n_vars, char** alleles, size_t* allele_bytes, wfm_varcall_t* per) {
  if (!h || !s || !vars || !n_vars || !alleles || !allele_bytes || (n_runs_total && !runs)) return WFM_E_ARG;
  *vars = nullptr; *alleles = nullptr;
  *n_vars = 0; *allele_bytes = 0;
  PassTimer tm(h);
  const size_t n = s->meta.size();
  if (n == 0) return WFM_OK;
  if (!res || !per) return WFM_E_ARG;
  if (n > (size_t)INT32_MAX || n_runs_total > ((size_t)1 << 31)) { h->err = "wfm_call_variants: too many problems or runs for one call"; return WFM_E_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<CsProb> probs;
  uint64_t rec_total = 0;
  if (int rc = cs_problems(h, s, res, n_runs_total, 0, probs, &rec_total)) return rc;
  // one block: [run records] 16 bytes per run, [offsets of the alleles] and [of the records] n + 1 each, [totals of both] n each of 8 bytes,
  // [problems], [runs], [record prefixes] one word per run, [flags], [end gaps]
  const size_t nr = n_runs_total;
  uint4* d_recs;
  unsigned long long *d_goff, *d_voff, *d_totb, *d_totr;
  CsProb* d_probs;
  uint32_t *d_runs, *d_rpre, *d_flags, *d_ends;
  std::vector<unsigned long long> goff(n + 1), voff(n + 1);
  std::vector<uint32_t> flags(n), ends(n);
  int spans = 0;
  // chunks of problems whose records and alleles fit the output block (a problem larger than that is a chunk of its own); the block: the
  // chunk's records, then its alleles in whole slices
  const EmitSpec sp{"wfm_call_variants", "variants", "variants", "variants output", h->scratch, h->outblk, (unsigned long long)std::max(1, env_num("WFM_VAR_OUT_MB", 256)) << 20};
  const EmitStream streams[] = {{voff, sizeof(wfm_variant_t), 1, plain_alloc, (void**)vars, n_vars}, {goff, 1, WFM_VAR_SLICE, plain_alloc, (void**)alleles, allele_bytes}};
  EmitStats st;
  const int rc = emit_lists(
      h, tm, sp, n, streams,
      [&](Carver& cv) {
        cv.piece(&d_recs, (size_t)rec_total); cv.piece(&d_goff, n + 1); cv.piece(&d_voff, n + 1); cv.piece(&d_totb, n); cv.piece(&d_totr, n);
        cv.piece(&d_probs, n); cv.piece(&d_runs, nr); cv.piece(&d_rpre, (size_t)rec_total); cv.piece(&d_flags, n); cv.piece(&d_ends, n);
      },
      [&](auto down) {
        if (nr) HIPCHK(h, hipMemcpyAsync(d_runs, runs, nr * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_probs, probs.data(), n * sizeof(CsProb), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, tm.timed([&] { launch_var_index(d_runs, d_probs, (int)n, d_recs, d_rpre, d_totb, d_totr, d_ends, d_flags, h->stream); }));
        down(goff.data() + 1, d_totb, n * 8); down(voff.data() + 1, d_totr, n * 8); down(flags.data(), d_flags, n * 4); down(ends.data(), d_ends, n * 4);
        return WFM_OK;
      },
      [&]() {  // the problems' totals, once: the host takes the two prefix sums
        goff[0] = 0; voff[0] = 0;
        for (size_t i = 0; i < n; ++i) {
          per[i].flags = flags[i]; per[i].n_runs = probs[i].n_runs;
          per[i].first = voff[i]; per[i].count = voff[i + 1];
          per[i].end_gaps = ends[i]; per[i].pad_ = 0;
          goff[i + 1] += goff[i]; voff[i + 1] += voff[i];
          spans += (flags[i] & WFM_VAR_SPANS) != 0;
        }
        if (goff[n]) {  // (a record has allele bytes: no bytes, no records)
          HIPCHK(h, hipMemcpyAsync(d_goff, goff.data(), (n + 1) * 8, hipMemcpyHostToDevice, h->stream));
          HIPCHK(h, hipMemcpyAsync(d_voff, voff.data(), (n + 1) * 8, hipMemcpyHostToDevice, h->stream));
        }
        return spans;
      },
      [&](size_t ka, size_t kb, uint8_t* const* d) {
        return hip_rc(h, sp.fn, tm.timed([&] {
          launch_var_write(s->d_seq, d_probs, d_recs, d_rpre, d_goff, d_voff, (uint32_t)ka, (uint32_t)kb, goff[kb] - goff[ka], d[1], d[0], h->stream);
        }));
      },
      &st);
  if (tm.on && st.chunks)
    fprintf(stderr, "[wfm] variants: %zu problems, %zu runs, %llu records, %llu allele bytes in %zu chunks, index %.3f ms, write %.3f ms (device events), the call %.3f ms (host clock)\n",
            n, (size_t)rec_total, voff[n], goff[n], st.chunks, st.ms_index, st.ms_write, tm.host_ms());
  return rc;
}

void wfm_free_variants(wfm_variant_t* vars, char* alleles) { free(vars); free(alleles); }

// ---- the two gapped rows of every problem's runs, in the blocks of a pairwise MAF (wfmash_hip.h; the kernels: wfa_maf.hip) ----
namespace {
// The caller's row buffer (released with free, as wfm_free_maf does).  From 8 MiB on it begins on a 2 MiB boundary, is a whole number of such
// pieces and is advised to huge pages: the rows are written once by memcpy, read once and freed, and a buffer of tens of MB on 4 KiB pages
// pays for every page on each of the three (profiles/maf.md section 3: 7 ms a call against 2 for 42 MB)
char* maf_rows_alloc(size_t bytes) {
  constexpr size_t HUGE = (size_t)2 << 20;
  if (bytes >= 4 * HUGE) {
    const size_t whole = (bytes + HUGE - 1) / HUGE * HUGE;
    if (void* p = aligned_alloc(HUGE, whole)) {
      (void)madvise(p, whole, MADV_HUGEPAGE);
      return (char*)p;
    }
  }
  return (char*)malloc(bytes);
}
}  // namespace

int wfm_maf_rows(wfm_handle_t* h, const wfm_seqset_t* s, const wfm_result_t* res, const uint32_t* runs, size_t n_runs_total, uint32_t split,
                 wfm_maf_block_t** blocks, size_t* n_blocks, char** rows, size_t* bytes, wfm_mafcall_t* per) {
  if (!h || !s || !blocks || !n_blocks || !rows || !bytes || (n_runs_total && !runs)) return WFM_E_ARG;
  *blocks = nullptr; *rows = nullptr;
  *n_blocks = 0; *bytes = 0;
  PassTimer tm(h);
  const size_t n = s->meta.size();
  if (n == 0) return WFM_OK;
  if (!res || !per) return WFM_E_ARG;
  if (n > (size_t)INT32_MAX || n_runs_total > ((size_t)1 << 31)) { h->err = "wfm_maf_rows: too many problems or runs for one call"; return WFM_E_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<CsProb> probs;
  uint64_t rec_total = 0;
  if (int rc = cs_problems(h, s, res, n_runs_total, 1, probs, &rec_total)) return rc;
  size_t run_total = 0;
  for (const CsProb& c : probs) run_total += c.n_runs;
  // one block: [run records] 16 and [prefixes] 8 bytes per slot, [offsets of the rows] and [of the blocks] n + 1 each, [blocks] and
  // [columns] n each of 8 bytes, [problems], [runs], [flags]
  const size_t nr = n_runs_total;
  uint4* d_recs;
  uint2* d_pre;
  unsigned long long *d_goff, *d_boff, *d_nblk, *d_ncols;
  CsProb* d_probs;
  uint32_t *d_runs, *d_flags;
  std::vector<unsigned long long> goff(n + 1), boff(n + 1);
  std::vector<uint32_t> flags(n);
  int spans = 0;
  // chunks of whole problems whose blocks and rows fit the output block (a problem larger than that is a chunk of its own); the block: the
  // chunk's block table (to a multiple of 16 bytes), then its rows in whole slices
  const EmitSpec sp{"wfm_maf_rows", "maf", "maf", "maf output", h->scratch, h->outblk, cap_units("WFM_MAF_OUT_MB", 1, 1)};
  const EmitStream streams[] = {{boff, sizeof(wfm_maf_block_t), 16, plain_alloc, (void**)blocks, n_blocks}, {goff, 1, WFM_MAF_SLICE, maf_rows_alloc, (void**)rows, bytes}};
  EmitStats st;
  const int rc = emit_lists(
      h, tm, sp, n, streams,
      [&](Carver& cv) {
        cv.piece(&d_recs, (size_t)rec_total); cv.piece(&d_pre, (size_t)rec_total); cv.piece(&d_goff, n + 1); cv.piece(&d_boff, n + 1);
        cv.piece(&d_nblk, n); cv.piece(&d_ncols, n); cv.piece(&d_probs, n); cv.piece(&d_runs, nr); cv.piece(&d_flags, n);
      },
      [&](auto down) {
        if (nr) HIPCHK(h, hipMemcpyAsync(d_runs, runs, nr * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_probs, probs.data(), n * sizeof(CsProb), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, tm.timed([&] { launch_maf_index(d_runs, d_probs, (int)n, split, d_recs, d_pre, d_nblk, d_ncols, d_flags, h->stream); }));
        down(goff.data() + 1, d_ncols, n * 8); down(boff.data() + 1, d_nblk, n * 8); down(flags.data(), d_flags, n * 4);
        return WFM_OK;
      },
      [&]() {  // the problems' blocks and columns, once: the host takes the two prefix sums
        goff[0] = 0; boff[0] = 0;
        for (size_t i = 0; i < n; ++i) {
          per[i].flags = flags[i]; per[i].n_runs = probs[i].n_runs;
          per[i].first = boff[i]; per[i].count = boff[i + 1];
          goff[i + 1] = goff[i] + 2 * goff[i + 1];  // (two rows a column)
          boff[i + 1] += boff[i];
          spans += (flags[i] & WFM_MAF_SPANS) != 0;
        }
        if (boff[n]) {  // (a block has columns: no blocks, no bytes)
          HIPCHK(h, hipMemcpyAsync(d_goff, goff.data(), (n + 1) * 8, hipMemcpyHostToDevice, h->stream));
          HIPCHK(h, hipMemcpyAsync(d_boff, boff.data(), (n + 1) * 8, hipMemcpyHostToDevice, h->stream));
        }
        return spans;
      },
      [&](size_t ka, size_t kb, uint8_t* const* d) {
        const unsigned long long nb = boff[kb] - boff[ka];
        if (nb > 0xffffffffull) { h->err = "wfm_maf_rows: too many blocks in one chunk"; return (int)WFM_E_ARG; }
        return hip_rc(h, sp.fn, tm.timed([&] {
          launch_maf_write(s->d_seq, d_probs, d_recs, d_pre, d_nblk, d_goff, d_boff, (uint32_t)ka, (uint32_t)kb, goff[kb] - goff[ka], d[0], (uint32_t)nb, d[1], h->stream);
        }));
      },
      &st);
  if (tm.on && st.chunks)
    fprintf(stderr, "[wfm] maf (split %u): %zu problems, %zu runs, %llu blocks, %llu bytes in %zu chunks, index %.3f ms, blocks + write %.3f ms (device events), the call %.3f ms (host clock)\n",
            split, n, run_total, boff[n], goff[n], st.chunks, st.ms_index, st.ms_write, tm.host_ms());
  return rc;
}

void wfm_free_maf(wfm_maf_block_t* blocks, char* rows) { free(blocks); free(rows); }

// ---- per-base depth of the target from the runs of many records (wfmash_hip.h; the kernels: wfa_coverage.hip) ----
struct wfm_coverage {
  int device = 0;
  uint64_t n_bases = 0, ntiles = 0;
  int32_t* d = nullptr;                      // the difference array: ntiles whole tiles, zero behind word n_bases
  uint64_t* aux = nullptr;                   // one block for the four below
  uint32_t* tile_cnt = nullptr;              // ntiles
  unsigned long long* tile_off = nullptr;    // ntiles + 1
  unsigned long long* tile_sums = nullptr;   // one per WFM_COV_SCAN_BLOCK tiles, + 1
  unsigned long long* cells = nullptr;       // the depth carried from chunk to chunk, then the three totals
  DevBuf<uint64_t> work;                     // a call's problems and runs, or a chunk's entries, intervals and block sums
};

extern "C++" {  // (a template among them)
namespace {
static_assert(sizeof(wfm_cov_prob_t) == 24 && sizeof(CovProb) == 24 && sizeof(wfm_cov_entry_t) == 16 && sizeof(wfm_cov_interval_t) == 16, "wfmash_hip.h states these sizes");

int cov_usable(wfm_handle_t* h, const wfm_coverage_t* cov) { return DeviceGuard::usable(h, cov->device, "the coverage object"); }

// every tile's offset in the compact list, on the device (cov->tile_off) and here
int cov_tile_offsets(wfm_handle_t* h, wfm_coverage_t* cov, std::vector<unsigned long long>& off) {
  launch_cov_tile_offsets(cov->d, cov->ntiles, cov->tile_cnt, cov->tile_sums, cov->tile_off, h->stream);
  HIPCHK(h, hipGetLastError());
  off.resize((size_t)cov->ntiles + 1);
  HIPCHK(h, hipMemcpyAsync(off.data(), cov->tile_off, off.size() * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return WFM_OK;
}

// The compact list in chunks of whole tiles that hold at most WFM_COV_OUT_MB MiB of entries: each chunk's entries are written to the head
// of cov->work, which holds words_per_entry 8-byte words for every entry of the chunk and room for its block sums, and handed to
// f(d_entries, first entry, entries, last chunk) -> WFM_*.
template <class F>
int cov_chunks(wfm_handle_t* h, wfm_coverage_t* cov, const std::vector<unsigned long long>& off, size_t words_per_entry, F f) {
  const unsigned long long total = off.back();
  const unsigned long long cap = cap_units("WFM_COV_OUT_MB", 16, WFM_COV_TILE);
  for (size_t ta = 0, tb; ta < (size_t)cov->ntiles; ta = tb) {
    tb = chunk_end(ta, off, cap);
    const unsigned long long m = off[tb] - off[ta];
    if (m == 0) continue;
    if (cov->work.ensure((size_t)m * words_per_entry + (size_t)m / WFM_COV_SCAN_BLOCK + 8)) { h->err = "out of device memory (coverage list)"; return WFM_E_NOMEM; }
    launch_cov_write(cov->d, cov->tile_off, ta, tb, off[ta], cov->work.p, h->stream);
    HIPCHK(h, hipGetLastError());
    const int rc = f((const uint8_t*)cov->work.p, off[ta], m, off[tb] == total);
    if (rc != WFM_OK) return rc;
  }
  return WFM_OK;
}
}  // namespace
}  // extern "C++"

int wfm_coverage_create(wfm_handle_t* h, uint64_t n_bases, wfm_coverage_t** cov) {
  if (!h || !cov) return WFM_E_ARG;
  *cov = nullptr;
  const double gib = env_decimal("WFM_COV_GB", 32.0), need = ((double)n_bases + 1.0) * 4.0 / 1073741824.0;
  if (n_bases >= ((uint64_t)1 << 40) || need > gib) {
    char msg[200];
    snprintf(msg, sizeof msg, "wfm_coverage_create: the difference array of %llu target bases needs %.3f GiB, more than WFM_COV_GB = %.3f",
             (unsigned long long)n_bases, need, gib);
    h->err = msg;
    return WFM_E_ARG;
  }
  HIPCHK(h, hipSetDevice(h->device));
  std::unique_ptr<wfm_coverage> c(new wfm_coverage());
  c->device = h->device;
  c->n_bases = n_bases;
  c->ntiles = (n_bases + 1 + WFM_COV_TILE - 1) / WFM_COV_TILE;
  const size_t nsums = (size_t)(c->ntiles + WFM_COV_SCAN_BLOCK - 1) / WFM_COV_SCAN_BLOCK + 1;
  const size_t w_cnt = ((size_t)c->ntiles * 4 + 7) / 8, w_off = (size_t)c->ntiles + 1;
  if (wfm_dmalloc((void**)&c->d, (size_t)c->ntiles * WFM_COV_TILE * 4) != hipSuccess ||
      wfm_dmalloc((void**)&c->aux, (w_cnt + w_off + nsums + 4) * 8) != hipSuccess) {
    (void)hipGetLastError();
    if (c->d) wfm_dfree(c->d);
    h->err = "out of device memory (coverage)";
    return WFM_E_NOMEM;
  }
  c->tile_cnt = (uint32_t*)c->aux;
  c->tile_off = (unsigned long long*)(c->aux + w_cnt);
  c->tile_sums = c->tile_off + w_off;
  c->cells = c->tile_sums + nsums;
  hipError_t e = hipMemsetAsync(c->d, 0, (size_t)c->ntiles * WFM_COV_TILE * 4, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) { wfm_dfree(c->d); wfm_dfree(c->aux); h->err = std::string("wfm_coverage_create: ") + hipGetErrorString(e); return WFM_E_HIP; }
  *cov = c.release();
  return WFM_OK;
}

void wfm_coverage_free(wfm_coverage_t* cov) {
  if (!cov) return;
  DeviceGuard on(cov->device);
  cov->work.release();
  if (cov->d) wfm_dfree(cov->d);
  if (cov->aux) wfm_dfree(cov->aux);
  delete cov;
}

int wfm_coverage_add(wfm_handle_t* h, wfm_coverage_t* cov, const wfm_cov_prob_t* probs, size_t n, const uint32_t* runs, size_t n_runs_total,
                     uint32_t* flags_out) {
  if (!cov) return WFM_E_ARG;
  CovProb* d_probs;
  uint32_t *d_runs, *d_flags;
  Carver cv{cov->work, "coverage add"};
  const int rc = add_preface(h, cov, cov->device, "the coverage object", "wfm_coverage_add", cv, probs, n, runs, n_runs_total, flags_out, &d_probs, &d_runs,
                             [&] { cv.piece(&d_flags, n); return WFM_OK; });
  if (rc || !d_probs) return rc;
  launch_cov_add(d_runs, d_probs, (int)n, cov->d, cov->n_bases, d_flags, h->stream);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(flags_out, d_flags, n * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return count_flagged(flags_out, n, WFM_COV_SPANS);
}

int wfm_coverage_export(wfm_handle_t* h, wfm_coverage_t* cov, wfm_cov_entry_t** entries, size_t* n) {
  if (!h || !cov || !entries || !n) return WFM_E_ARG;
  *entries = nullptr; *n = 0;
  if (int rc = cov_usable(h, cov)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  PassTimer tm(h);
  std::vector<unsigned long long> off;
  if (int rc = cov_tile_offsets(h, cov, off)) return rc;
  const double ms_off = tm.lap();
  const unsigned long long total = off.back();
  if (total == 0) return WFM_OK;
  char* host = (char*)malloc((size_t)total * sizeof(wfm_cov_entry_t));
  if (!host) { h->err = "out of host memory (coverage list)"; return WFM_E_NOMEM; }
  const bool pinned = pin_pieces(h);
  const int rc = cov_chunks(h, cov, off, 2, [&](const uint8_t* d_ent, unsigned long long first, unsigned long long m, bool) {
    const hipError_t e = copy_down(h, pinned, host + first * sizeof(wfm_cov_entry_t), d_ent, (size_t)m * sizeof(wfm_cov_entry_t));  // (the block is the next chunk's)
    if (e != hipSuccess) { h->err = std::string("wfm_coverage_export: ") + hipGetErrorString(e); return (int)WFM_E_HIP; }
    return (int)WFM_OK;
  });
  if (rc != WFM_OK) { free(host); return rc; }
  *entries = (wfm_cov_entry_t*)host; *n = (size_t)total;
  if (tm.on)
    fprintf(stderr, "[wfm] coverage export: %llu bases, %llu non-zero words, count + offsets %.3f ms, write + copy down %.3f ms (host clock, each ends in a synchronise)\n",
            (unsigned long long)cov->n_bases, total, ms_off, tm.lap());
  return WFM_OK;
}

int wfm_coverage_import(wfm_handle_t* h, wfm_coverage_t* cov, const wfm_cov_entry_t* entries, size_t n) {
  if (!h || !cov || (n && !entries)) return WFM_E_ARG;
  if (n == 0) return WFM_OK;
  if (int rc = cov_usable(h, cov)) return rc;
  for (size_t i = 0; i < n; ++i)
    if (entries[i].pos > cov->n_bases) { h->err = "entry " + std::to_string(i) + ": its position lies beyond the object's bases"; return WFM_E_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  constexpr size_t PIECE = (size_t)4 << 20;  // entries: 64 MiB a piece
  if (cov->work.ensure(std::min(n, PIECE) * 2)) { h->err = "out of device memory (coverage import)"; return WFM_E_NOMEM; }
  for (size_t at = 0; at < n; at += PIECE) {
    const size_t m = std::min(PIECE, n - at);
    HIPCHK(h, hipMemcpyAsync(cov->work.p, entries + at, m * sizeof(wfm_cov_entry_t), hipMemcpyHostToDevice, h->stream));
    launch_cov_import(cov->work.p, m, cov->d, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));  // (the block is the next piece's)
  }
  return WFM_OK;
}

int wfm_coverage_intervals(wfm_handle_t* h, wfm_coverage_t* cov, wfm_cov_interval_t** iv, size_t* n, uint64_t totals[3]) {
  if (!h || !cov || !iv || !n) return WFM_E_ARG;
  *iv = nullptr; *n = 0;
  if (totals) totals[0] = totals[1] = totals[2] = 0;
  if (int rc = cov_usable(h, cov)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  PassTimer tm(h);
  std::vector<unsigned long long> off;
  if (int rc = cov_tile_offsets(h, cov, off)) return rc;
  const double ms_off = tm.lap();
  const unsigned long long total = off.back();
  // (slot 0 is kept for the interval that begins at 0 where the first non-zero word lies further on)
  wfm_cov_interval_t* host = (wfm_cov_interval_t*)malloc(((size_t)total + 1) * sizeof(wfm_cov_interval_t));
  if (!host) { h->err = "out of host memory (coverage intervals)"; return WFM_E_NOMEM; }
  host[0].start = 0; host[0].depth = 0; host[0].pad_ = 0;
  hipError_t e0 = hipMemsetAsync(cov->cells, 0, 4 * 8, h->stream);
  if (e0 != hipSuccess) { free(host); h->err = std::string("wfm_coverage_intervals: ") + hipGetErrorString(e0); return WFM_E_HIP; }
  const bool pinned = pin_pieces(h);
  unsigned long long prev_pos = 0;
  size_t chunks = 0;
  int rc = cov_chunks(h, cov, off, 4, [&](const uint8_t* d_ent, unsigned long long first, unsigned long long m, bool last) {
    uint8_t* d_iv = (uint8_t*)(cov->work.p + 2 * (size_t)m);
    unsigned long long* d_sums = (unsigned long long*)(cov->work.p + 4 * (size_t)m);
    launch_cov_intervals(d_ent, m, d_sums, cov->cells, prev_pos, cov->n_bases, last ? 1 : 0, d_iv, cov->cells + 1, h->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = copy_down(h, pinned, (char*)(host + 1 + first), d_iv, (size_t)m * sizeof(wfm_cov_interval_t));
    if (e != hipSuccess) { h->err = std::string("wfm_coverage_intervals: ") + hipGetErrorString(e); return (int)WFM_E_HIP; }
    prev_pos = host[first + m].start;
    ++chunks;
    return (int)WFM_OK;
  });
  unsigned long long tot[3] = {0, 0, 0};
  if (rc == WFM_OK) {
    hipError_t e = hipMemcpyAsync(tot, cov->cells + 1, sizeof tot, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { h->err = std::string("wfm_coverage_intervals: ") + hipGetErrorString(e); rc = WFM_E_HIP; }
  }
  if (rc != WFM_OK) { free(host); return rc; }
  // the word at n_bases starts no interval; the interval from 0 is there already where word 0 is non-zero
  size_t count = (size_t)total;
  if (count && host[count].start >= cov->n_bases) --count;
  const bool lead = count == 0 || host[1].start != 0;
  if (!lead) memmove(host, host + 1, count * sizeof(wfm_cov_interval_t));
  *iv = host; *n = count + (lead ? 1 : 0);
  if (totals) { totals[0] = tot[0]; totals[1] = tot[1]; totals[2] = tot[2]; }
  if (tm.on)
    fprintf(stderr, "[wfm] coverage intervals: %llu bases, %llu non-zero words in %zu chunks, %zu intervals, count + offsets %.3f ms, write + scan + copy down %.3f ms (host clock, each ends in a synchronise)\n",
            (unsigned long long)cov->n_bases, total, chunks, *n, ms_off, tm.lap());
  return WFM_OK;
}

void wfm_coverage_free_list(void* p) { free(p); }

// ---- target intervals lifted through the runs of many records (wfmash_hip.h; the kernels: wfa_lift.hip) ----
struct wfm_liftset {
  int device = 0;
  uint64_t n = 0, n_bases = 0;
  uint64_t* iv = nullptr;               // one block: n intervals {start, end}, then pm (n), then the blocks' maxima
  unsigned long long* pm = nullptr;
  mutable DevBuf<uint64_t> work;        // a call's prefix words, problems, windows, offsets and runs
  mutable DevBuf<uint64_t> out;         // a chunk's lifts
};

static_assert(sizeof(wfm_lift_iv_t) == 16 && sizeof(wfm_lift_t) == 32 && sizeof(wfm_liftcall_t) == 24 && sizeof(LiftProb) == 32 && sizeof(LiftWin) == 32,
              "wfmash_hip.h and wfa_device.h state these sizes");

int wfm_liftset_create(wfm_handle_t* h, const wfm_lift_iv_t* iv, size_t n, uint64_t n_bases, wfm_liftset_t** out) {
  if (!h || !out || (n && !iv)) return WFM_E_ARG;
  *out = nullptr;
  if (n >= ((size_t)1 << 32)) { h->err = "wfm_liftset_create: too many intervals for one set"; return WFM_E_ARG; }
  for (size_t i = 0; i < n; ++i) {
    if (!(iv[i].start < iv[i].end && iv[i].end <= n_bases)) {
      h->err = "wfm_liftset_create: interval " + std::to_string(i) + " is empty or ends beyond the " + std::to_string(n_bases) + " target bases";
      return WFM_E_ARG;
    }
    if (i && (iv[i].start < iv[i - 1].start || (iv[i].start == iv[i - 1].start && iv[i].end < iv[i - 1].end))) {
      h->err = "wfm_liftset_create: interval " + std::to_string(i) + " lies before its predecessor: the intervals must be sorted by (start, end)";
      return WFM_E_ARG;
    }
  }
  HIPCHK(h, hipSetDevice(h->device));
  std::unique_ptr<wfm_liftset> s(new wfm_liftset());
  s->device = h->device;
  s->n = n;
  s->n_bases = n_bases;
  if (n) {
    const size_t nb = (n + WFM_LIFT_SCAN_BLOCK - 1) / WFM_LIFT_SCAN_BLOCK;
    if (wfm_dmalloc((void**)&s->iv, (n * 3 + nb + 2) * 8) != hipSuccess) { (void)hipGetLastError(); h->err = "out of device memory (liftset)"; return WFM_E_NOMEM; }
    s->pm = (unsigned long long*)(s->iv + n * 2);
    hipError_t e = hipMemcpyAsync(s->iv, iv, n * sizeof(wfm_lift_iv_t), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) { launch_lift_pm(s->iv, n, s->pm + n, s->pm, h->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { wfm_dfree(s->iv); h->err = std::string("wfm_liftset_create: ") + hipGetErrorString(e); return WFM_E_HIP; }
  }
  *out = s.release();
  return WFM_OK;
}

void wfm_liftset_free(wfm_liftset_t* s) {
  if (!s) return;
  DeviceGuard on(s->device);
  s->work.release();
  s->out.release();
  if (s->iv) wfm_dfree(s->iv);
  delete s;
}

int wfm_lift_runs(wfm_handle_t* h, const wfm_liftset_t* s, const wfm_cov_prob_t* probs, size_t n, const uint32_t* runs, size_t n_runs_total,
                  wfm_lift_t** lifts, size_t* n_lifts, wfm_liftcall_t* per) {
  if (!h || !s || !lifts || !n_lifts || (n && (!probs || !per)) || (n_runs_total && !runs)) return WFM_E_ARG;
  *lifts = nullptr; *n_lifts = 0;
  if (n == 0) return WFM_OK;
  if (n > (size_t)INT32_MAX || n_runs_total > ((size_t)1 << 31)) { h->err = "wfm_lift_runs: too many problems or runs for one call"; return WFM_E_ARG; }
  if (int rc = DeviceGuard::usable(h, s->device, "the liftset")) return rc;
  if (int rc = all_runs_inside(h, probs, n, n_runs_total)) return rc;
  std::vector<LiftProb> lp(n);
  uint64_t n_pre = 0;
  for (size_t i = 0; i < n; ++i) {
    lp[i] = LiftProb{probs[i].base, probs[i].runs_off, n_pre, probs[i].n_runs, 0u};
    n_pre += (uint64_t)probs[i].n_runs + 1;
  }
  HIPCHK(h, hipSetDevice(h->device));
  PassTimer tm(h);
  // (the prefix words come first: they are read 16 bytes at a time)
  uint4* d_pre;
  LiftProb* d_probs;
  LiftWin* d_win;
  unsigned long long* d_off;
  uint32_t* d_runs;
  std::vector<LiftWin> win(n);
  std::vector<unsigned long long> off(n + 1);
  double ms_index = 0;
  // chunks of whole problems that hold at most WFM_LIFT_OUT_MB MiB of lifts; a single problem may exceed that alone
  const EmitSpec sp{"wfm_lift_runs", "lift", "lifts", "lifts", s->work, s->out, cap_units("WFM_LIFT_OUT_MB", sizeof(wfm_lift_t), 1) * sizeof(wfm_lift_t)};
  const EmitStream streams[] = {{off, sizeof(wfm_lift_t), 1, plain_alloc, (void**)lifts, n_lifts}};
  EmitStats st;
  const int rc = emit_lists(
      h, tm, sp, n, streams,
      [&](Carver& cv) { cv.piece(&d_pre, (size_t)n_pre); cv.piece(&d_probs, n); cv.piece(&d_win, n); cv.piece(&d_off, n + 1); cv.piece(&d_runs, n_runs_total); },
      [&](auto down) {
        HIPCHK(h, hipMemcpyAsync(d_probs, lp.data(), n * sizeof(LiftProb), hipMemcpyHostToDevice, h->stream));
        if (n_runs_total) HIPCHK(h, hipMemcpyAsync(d_runs, runs, n_runs_total * 4, hipMemcpyHostToDevice, h->stream));
        launch_lift_index(d_runs, d_probs, (int)n, s->iv, s->pm, s->n, s->n_bases, d_pre, d_win, d_off, h->stream);
        HIPCHK(h, hipGetLastError());
        down(win.data(), d_win, n * sizeof(LiftWin)); down(off.data(), d_off, (n + 1) * 8);
        return WFM_OK;
      },
      [&]() {  // (the offsets are the device's)
        ms_index = tm.lap();
        for (size_t i = 0; i < n; ++i) per[i] = wfm_liftcall_t{win[i].flags, probs[i].n_runs, off[i], win[i].count};
        return WFM_OK;
      },
      [&](size_t ka, size_t kb, uint8_t* const* d) {
        launch_lift_write(d_runs, d_probs, s->iv, d_pre, d_win, d_off, (uint32_t)ka, (uint32_t)kb, d[0], h->stream);
        return hip_rc(h, sp.fn, hipGetLastError());
      },
      &st);
  if (tm.on && st.chunks)
    fprintf(stderr, "[wfm] lift: %zu problems, %zu runs, %llu intervals, %llu lifts in %zu chunks, upload + index + count %.3f ms, write + copy down %.3f ms (host clock, each ends in a synchronise)\n",
            n, n_runs_total, (unsigned long long)s->n, off[n], st.chunks, ms_index, tm.lap());
  return rc;
}

void wfm_free_lifts(wfm_lift_t* p) { free(p); }

// ---- the blocks and gaps of a chain from every problem's runs (wfmash_hip.h; the kernels: wfa_chain.hip) ----
static_assert(sizeof(wfm_chain_prob_t) == 16 && sizeof(wfm_chain_block_t) == 16 && sizeof(wfm_chaincall_t) == 48 && sizeof(ChainProb) == 24 && sizeof(ChainWin) == 40,
              "wfmash_hip.h and wfa_device.h state these sizes");

int wfm_chain_runs(wfm_handle_t* h, const wfm_chain_prob_t* probs, size_t n, const uint32_t* runs, size_t n_runs_total, wfm_chain_block_t** blocks,
                   size_t* n_blocks, wfm_chaincall_t* per) {
  if (!h || !blocks || !n_blocks || (n && (!probs || !per)) || (n_runs_total && !runs)) return WFM_E_ARG;
  *blocks = nullptr; *n_blocks = 0;
  if (n == 0) return WFM_OK;
  if (n > (size_t)INT32_MAX || n_runs_total > ((size_t)1 << 31)) { h->err = "wfm_chain_runs: too many problems or runs for one call"; return WFM_E_ARG; }
  if (int rc = all_runs_inside(h, probs, n, n_runs_total)) return rc;
  std::vector<ChainProb> cp(n);
  uint64_t n_pre = 0;
  for (size_t i = 0; i < n; ++i) {
    if (probs[i].flags & ~(WFM_CHAIN_SWAP | WFM_CHAIN_REVERSE)) {
      h->err = "problem " + std::to_string(i) + ": flags " + std::to_string(probs[i].flags) + " hold a bit that is neither WFM_CHAIN_SWAP nor WFM_CHAIN_REVERSE";
      return WFM_E_ARG;
    }
    cp[i] = ChainProb{probs[i].runs_off, n_pre, probs[i].n_runs, probs[i].flags};
    n_pre += (uint64_t)probs[i].n_runs + 1;
  }
  HIPCHK(h, hipSetDevice(h->device));
  PassTimer tm(h);
  // (the prefix words come first: they are read 16 bytes at a time)
  uint4* d_pre;
  ChainProb* d_probs;
  ChainWin* d_win;
  unsigned long long* d_off;
  uint32_t* d_runs;
  std::vector<ChainWin> win(n);
  std::vector<unsigned long long> off(n + 1);
  // chunks of whole problems that hold at most WFM_CHAIN_OUT_MB MiB of blocks; a single problem may exceed that alone
  const EmitSpec sp{"wfm_chain_runs", "chain", "chain", "chain output", h->scratch, h->outblk, cap_units("WFM_CHAIN_OUT_MB", sizeof(wfm_chain_block_t), 1) * sizeof(wfm_chain_block_t)};
  const EmitStream streams[] = {{off, sizeof(wfm_chain_block_t), 1, plain_alloc, (void**)blocks, n_blocks}};
  EmitStats st;
  const int rc = emit_lists(
      h, tm, sp, n, streams,
      [&](Carver& cv) { cv.piece(&d_pre, (size_t)n_pre); cv.piece(&d_probs, n); cv.piece(&d_win, n); cv.piece(&d_off, n + 1); cv.piece(&d_runs, n_runs_total); },
      [&](auto down) {
        HIPCHK(h, hipMemcpyAsync(d_probs, cp.data(), n * sizeof(ChainProb), hipMemcpyHostToDevice, h->stream));
        if (n_runs_total) HIPCHK(h, hipMemcpyAsync(d_runs, runs, n_runs_total * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, tm.timed([&] { launch_chain_index(d_runs, d_probs, (int)n, d_pre, d_win, d_off, h->stream); }));
        down(win.data(), d_win, n * sizeof(ChainWin)); down(off.data(), d_off, (n + 1) * 8);
        return WFM_OK;
      },
      [&]() {  // (the offsets are the device's)
        for (size_t i = 0; i < n; ++i) {
          const ChainWin& w = win[i];
          per[i] = wfm_chaincall_t{w.flags, probs[i].n_runs, off[i], w.count, w.lead_dt, w.lead_dq, w.trail_dt, w.trail_dq, w.eq, w.x};
        }
        return WFM_OK;
      },
      [&](size_t ka, size_t kb, uint8_t* const* d) {
        return hip_rc(h, sp.fn, tm.timed([&] { launch_chain_write(d_runs, d_probs, d_pre, d_win, d_off, (uint32_t)ka, (uint32_t)kb, d[0], h->stream); }));
      },
      &st);
  if (tm.on && st.chunks)
    fprintf(stderr, "[wfm] chain: %zu problems, %zu runs, %llu blocks in %zu chunks, index %.3f ms, write %.3f ms (device events), the call %.3f ms (host clock)\n",
            n, n_runs_total, off[n], st.chunks, st.ms_index, st.ms_write, tm.host_ms());
  return rc;
}

void wfm_free_chain(wfm_chain_block_t* p) { free(p); }

// ---- presence of target intervals per group of records (wfmash_hip.h; the kernels and the sort: wfa_pav.hip) ----
struct wfm_pav {
  int device = 0;
  uint64_t n_bases = 0;
  uint32_t n_groups = 0;
  unsigned long long* list = nullptr;    // one block: the start keys [0, cap), then the end keys [cap, 2 cap)
  size_t cap = 0, n = 0, n_union = 0;    // segments the block holds; segments in it; the first n_union of them are the last union's
  bool clean = false;                    // the list is a union and C its prefix
  DevBuf<uint64_t> c;                    // C: n_union + 1
  DevBuf<uint64_t> work;                 // a call's problems, runs, flags, counts and offsets; the sorted copy and the block words; a chunk of rows
  DevBuf<uint64_t> tmp;                  // the sort's own
  uint64_t added = 0, unions = 0;
  bool eq_only = false;                  // the = union of a sites object: a segment is a stretch of = runs, the limit WFM_SITES_MB
  unsigned long long* ks() const { return list; }
  unsigned long long* ke() const { return list + cap; }
};

extern "C++" {
namespace {
static_assert(sizeof(wfm_pav_prob_t) == 24 && sizeof(PavProb) == 24 && sizeof(wfm_pav_seg_t) == 16, "wfmash_hip.h states these sizes");
constexpr unsigned PAV_SHIFT = 40;
constexpr size_t PAV_MAX_SEGS = (size_t)1 << 31;

int pav_usable(wfm_handle_t* h, const wfm_pav_t* pav) { return DeviceGuard::usable(h, pav->device, "the pav object"); }

// room for `need` segments; what the list holds moves with it.  The block that is outgrown goes to the block cache, not to the driver.
int pav_reserve(wfm_handle_t* h, wfm_pav_t* pav, size_t need) {
  if (need <= pav->cap) return WFM_OK;
  if (need > PAV_MAX_SEGS) { h->err = "wfm_pav: more than 2^31 segments in one object; lower WFM_PAV_MB so that the union is taken sooner"; return WFM_E_NOMEM; }
  const size_t cap = std::max<size_t>(need + need / 2, 4096);
  unsigned long long* blk = nullptr;
  if (wfm_dmalloc((void**)&blk, cap * 16) != hipSuccess) { (void)hipGetLastError(); h->err = "out of device memory (pav segments)"; return WFM_E_NOMEM; }
  if (pav->n) {
    hipError_t e = hipMemcpyAsync(blk, pav->ks(), pav->n * 8, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(blk + cap, pav->ke(), pav->n * 8, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { wfm_dfree(blk); h->err = std::string("wfm_pav: ") + hipGetErrorString(e); return WFM_E_HIP; }
  }
  if (pav->list) wfm_dfree(pav->list);
  pav->list = blk;
  pav->cap = cap;
  return WFM_OK;
}

// the union where the raw part of the list has outgrown WFM_PAV_MB MiB (the = union of a sites object: WFM_SITES_MB)
int pav_maybe_union(wfm_handle_t* h, wfm_pav_t* pav) {
  const double limit = std::max(0.0, env_decimal(pav->eq_only ? "WFM_SITES_MB" : "WFM_PAV_MB", 256.0)) * 1048576.0;
  if (pav->n > pav->n_union && (double)(pav->n - pav->n_union) * 16.0 > limit) return wfm_pav_union(h, pav);
  return WFM_OK;
}
}  // namespace
}  // extern "C++"

int wfm_pav_create(wfm_handle_t* h, uint64_t n_bases, uint32_t n_groups, wfm_pav_t** pav) {
  if (!h || !pav) return WFM_E_ARG;
  *pav = nullptr;
  if (n_bases >= ((uint64_t)1 << PAV_SHIFT) || n_groups >= (1u << 24)) {
    h->err = "wfm_pav_create: " + std::to_string(n_bases) + " target bases and " + std::to_string(n_groups) +
             " groups do not fit a segment's key, group << 40 | start: fewer than 2^40 bases and 2^24 groups";
    return WFM_E_ARG;
  }
  HIPCHK(h, hipSetDevice(h->device));
  std::unique_ptr<wfm_pav> p(new wfm_pav());
  p->device = h->device;
  p->n_bases = n_bases;
  p->n_groups = n_groups;
  p->clean = true;  // (the empty union)
  *pav = p.release();
  return WFM_OK;
}

void wfm_pav_free(wfm_pav_t* pav) {
  if (!pav) return;
  DeviceGuard on(pav->device);
  pav->c.release();
  pav->work.release();
  pav->tmp.release();
  if (pav->list) wfm_dfree(pav->list);
  delete pav;
}

int wfm_pav_add(wfm_handle_t* h, wfm_pav_t* pav, const wfm_pav_prob_t* probs, size_t n, const uint32_t* runs, size_t n_runs_total, uint32_t* flags_out) {
  if (!pav) return WFM_E_ARG;
  PassTimer tm(h);
  PavProb* d_probs;
  uint32_t *d_runs, *d_flags;
  unsigned long long *d_cnt, *d_off;
  Carver cv{pav->work, "pav add"};
  const int rc0 = add_preface(h, pav, pav->device, "the pav object", "wfm_pav_add", cv, probs, n, runs, n_runs_total, flags_out, &d_probs, &d_runs,
                              [&] { cv.piece(&d_flags, n); cv.piece(&d_cnt, n); cv.piece(&d_off, n + 1); return WFM_OK; });
  if (rc0 || !d_probs) return rc0;
  launch_pav_count(d_runs, d_probs, (int)n, pav->n_bases, pav->n_groups, d_flags, d_cnt, d_off, pav->eq_only, h->stream);
  HIPCHK(h, hipGetLastError());
  unsigned long long total = 0;
  HIPCHK(h, hipMemcpyAsync(flags_out, d_flags, n * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(&total, d_off + n, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const int spans = count_flagged(flags_out, n, WFM_PAV_SPANS);
  if (total) {
    if (int rc = pav_reserve(h, pav, pav->n + (size_t)total)) return rc;
    launch_pav_write(d_runs, d_probs, (int)n, d_flags, d_off, pav->ks() + pav->n, pav->ke() + pav->n, pav->eq_only, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    pav->n += (size_t)total;
    pav->added += total;
    pav->clean = false;
  }
  if (tm.on)
    fprintf(stderr, "[wfm] pav add: %zu problems, %zu runs, %llu segments, %d flagged, %.3f ms (host clock, ends in a synchronise); the list holds %zu\n",
            n, n_runs_total, total, spans, tm.host_ms(), pav->n);
  if (int rc = pav_maybe_union(h, pav)) return rc;
  return spans;
}

int wfm_pav_union(wfm_handle_t* h, wfm_pav_t* pav) {
  if (!h || !pav) return WFM_E_ARG;
  if (int rc = pav_usable(h, pav)) return rc;
  if (pav->clean) return WFM_OK;  // (nothing was added since the last one)
  HIPCHK(h, hipSetDevice(h->device));
  PassTimer tm(h);
  const size_t n = pav->n, nb = (n + WFM_PAV_SCAN_BLOCK - 1) / WFM_PAV_SCAN_BLOCK;
  // the sorted copy: start keys, end keys, then the blocks' words
  unsigned long long *ks2, *ke2, *aux;
  Carver cv{pav->work, "pav union"};
  cv.piece(&ks2, n); cv.piece(&ke2, n); cv.piece(&aux, nb + 1);
  if (int rc = cv.commit(h)) return rc;
  unsigned end_bit = PAV_SHIFT;
  while (end_bit < 64 && ((uint64_t)pav->n_groups >> (end_bit - PAV_SHIFT)) != 0) ++end_bit;  // (keys are below n_groups << 40)
  // (a union has no more intervals than the list has segments: the block holds it)
  unsigned long long m = 0;
  if (int rc = interval_union(h, pav->tmp, "out of device memory (pav sort)", pav->ks(), pav->ke(), ks2, ke2, n, end_bit, aux, pav->ks(), pav->ke(), &m,
                              [] { return (int)WFM_OK; }))
    return rc;
  if (m > n) { h->err = "wfm_pav_union: the union has more intervals than the list had segments"; return WFM_E_HIP; }
  if (pav->c.ensure((size_t)m + 2)) { h->err = "out of device memory (pav prefix)"; return WFM_E_NOMEM; }
  launch_pav_prefix(pav->ks(), pav->ke(), m, aux, (unsigned long long*)pav->c.p, h->stream);
  HIPCHK(h, hipGetLastError());
  if (m == 0) HIPCHK(h, hipMemsetAsync(pav->c.p, 0, 8, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  pav->n = pav->n_union = (size_t)m;
  pav->clean = true;
  pav->unions += 1;
  if (tm.on)
    fprintf(stderr, "[wfm] pav union: %zu segments to %llu intervals in %.3f ms (host clock, ends in a synchronise); device bytes: the list's block %zu, the sorted copy and block words %zu, the sort's own %zu, the prefix %zu\n",
            n, m, tm.host_ms(), pav->cap * 16, pav->work.cap * 8, pav->tmp.cap * 8,
            pav->c.cap * 8);
  return WFM_OK;
}

int wfm_pav_export(wfm_handle_t* h, wfm_pav_t* pav, wfm_pav_seg_t** segs, size_t* n) {
  if (!h || !pav || !segs || !n) return WFM_E_ARG;
  *segs = nullptr; *n = 0;
  if (int rc = wfm_pav_union(h, pav)) return rc;
  const size_t m = pav->n;
  if (m == 0) return WFM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<unsigned long long> keys(2 * m);
  const bool pinned = pin_pieces(h);
  hipError_t e = copy_down(h, pinned, (char*)keys.data(), (const uint8_t*)pav->ks(), m * 8);
  if (e == hipSuccess) e = copy_down(h, pinned, (char*)(keys.data() + m), (const uint8_t*)pav->ke(), m * 8);
  if (e != hipSuccess) { h->err = std::string("wfm_pav_export: ") + hipGetErrorString(e); return WFM_E_HIP; }
  // a union interval of 2^32 bases or more comes as abutting pieces
  const uint64_t mask = ((uint64_t)1 << PAV_SHIFT) - 1, piece = 0x80000000ull;
  size_t total = 0;
  for (size_t i = 0; i < m; ++i) { const uint64_t len = keys[m + i] - keys[i]; total += len > 0xffffffffull ? (size_t)((len + piece - 1) / piece) : 1; }
  wfm_pav_seg_t* out = (wfm_pav_seg_t*)malloc(total * sizeof(wfm_pav_seg_t));
  if (!out) { h->err = "out of host memory (pav list)"; return WFM_E_NOMEM; }
  size_t at = 0;
  for (size_t i = 0; i < m; ++i) {
    uint64_t s = keys[i] & mask, len = keys[m + i] - keys[i];
    const uint32_t g = (uint32_t)(keys[i] >> PAV_SHIFT);
    while (len > 0xffffffffull) { out[at++] = wfm_pav_seg_t{s, (uint32_t)piece, g}; s += piece; len -= piece; }
    out[at++] = wfm_pav_seg_t{s, (uint32_t)len, g};
  }
  *segs = out; *n = at;
  return WFM_OK;
}

int wfm_pav_import(wfm_handle_t* h, wfm_pav_t* pav, const wfm_pav_seg_t* segs, size_t n) {
  if (!h || !pav || (n && !segs)) return WFM_E_ARG;
  if (n == 0) return WFM_OK;
  if (int rc = pav_usable(h, pav)) return rc;
  std::vector<unsigned long long> keys(2 * n);
  for (size_t i = 0; i < n; ++i) {
    if (segs[i].length == 0 || segs[i].start > pav->n_bases || segs[i].length > pav->n_bases - segs[i].start || segs[i].group >= pav->n_groups) {
      h->err = "wfm_pav_import: segment " + std::to_string(i) + " is empty, leaves the " + std::to_string(pav->n_bases) + " target bases or names a group that is not below " +
               std::to_string(pav->n_groups);
      return WFM_E_ARG;
    }
    keys[i] = ((uint64_t)segs[i].group << PAV_SHIFT) | segs[i].start;
    keys[n + i] = keys[i] + segs[i].length;
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = pav_reserve(h, pav, pav->n + n)) return rc;
  HIPCHK(h, hipMemcpyAsync(pav->ks() + pav->n, keys.data(), n * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(pav->ke() + pav->n, keys.data() + n, n * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  pav->n += n;
  pav->added += n;
  pav->clean = false;
  return pav_maybe_union(h, pav);
}

int wfm_pav_matrix(wfm_handle_t* h, wfm_pav_t* pav, const wfm_lift_iv_t* iv, size_t n_iv, uint32_t* out) {
  if (!h || !pav || (n_iv && (!iv || (pav->n_groups && !out)))) return WFM_E_ARG;
  for (size_t j = 0; j < n_iv; ++j)
    if (!(iv[j].start <= iv[j].end && iv[j].end <= pav->n_bases && iv[j].end - iv[j].start <= 0xffffffffull)) {
      h->err = "wfm_pav_matrix: interval " + std::to_string(j) + " is reversed, ends beyond the " + std::to_string(pav->n_bases) + " target bases or is 2^32 bases long or longer";
      return WFM_E_ARG;
    }
  if (int rc = wfm_pav_union(h, pav)) return rc;
  if (n_iv == 0 || pav->n_groups == 0) return WFM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  PassTimer tm(h);
  const size_t G = pav->n_groups;
  // chunks of whole rows that hold at most WFM_PAV_OUT_MB MiB of the matrix
  const size_t cap = (size_t)cap_units("WFM_PAV_OUT_MB", G * 4, 1);
  wfm_lift_iv_t* d_iv;
  uint32_t* d_out;
  Carver cv{pav->work, "pav matrix"};
  cv.piece(&d_iv, n_iv); cv.piece(&d_out, std::min(n_iv, cap) * G);
  if (int rc = cv.commit(h)) return rc;
  HIPCHK(h, hipMemcpyAsync(d_iv, iv, n_iv * sizeof(wfm_lift_iv_t), hipMemcpyHostToDevice, h->stream));
  const bool pinned = pin_pieces(h);
  size_t chunks = 0;
  for (size_t ra = 0, rb; ra < n_iv; ra = rb, ++chunks) {
    rb = chunk_end(ra, n_iv, cap, [](size_t a, size_t b) { return (unsigned long long)(b - a); });
    launch_pav_matrix(pav->ks(), pav->ke(), (const unsigned long long*)pav->c.p, pav->n, d_iv, ra, rb, pav->n_groups, d_out, h->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = copy_down(h, pinned, (char*)(out + ra * G), (const uint8_t*)d_out, (rb - ra) * G * 4);  // (the block is the next chunk's)
    if (e != hipSuccess) { h->err = std::string("wfm_pav_matrix: ") + hipGetErrorString(e); return WFM_E_HIP; }
  }
  if (tm.on)
    fprintf(stderr, "[wfm] pav matrix: %zu intervals x %zu groups over %zu union intervals in %zu chunks, %.3f ms (host clock, ends in a synchronise)\n", n_iv, G,
            pav->n, chunks, tm.host_ms());
  return WFM_OK;
}

int wfm_pav_counts(const wfm_pav_t* pav, uint64_t out[3]) {
  if (!pav || !out) return WFM_E_ARG;
  out[0] = pav->added; out[1] = pav->n_union; out[2] = pav->unions;
  return WFM_OK;
}

void wfm_pav_free_list(void* p) { free(p); }

// ---- the variants of many records joined into sites and genotypes (wfmash_hip.h; the kernels and the sorts: wfa_sites.hip) ----
struct wfm_sites {
  int device = 0;
  uint64_t n_bases = 0;
  uint32_t n_groups = 0;
  wfm_pav_t* eq = nullptr;        // the = union, a pav object in its eq_only mode
  SiteVar* vars = nullptr;        // the raw variants; off: into alle
  size_t vcap = 0, n = 0;
  uint8_t* alle = nullptr;        // their folded allele bytes
  size_t acap = 0, bytes = 0;
  std::vector<uint64_t> tasks;    // record << 32 | piece for every WFM_SITES_TASK bytes of a pair longer than WFM_SITES_SLICE
  DevBuf<uint64_t> work;          // the table call's keys, permutations, flags and rows; a chunk of cells
  DevBuf<uint64_t> tmp;           // the sorts' own
  uint64_t added = 0, last_sites = 0, last_collisions = 0;
};

extern "C++" {
namespace {
static_assert(sizeof(wfm_site_var_t) == 32 && sizeof(SiteVar) == 32 && sizeof(wfm_site_t) == 32 && sizeof(SiteRow) == 32, "wfmash_hip.h states these sizes");
constexpr size_t SITES_MAX_VARS = ((size_t)1 << 31) - 1;

int sites_usable(wfm_handle_t* h, const wfm_sites_t* s) { return DeviceGuard::usable(h, s->device, "the sites object"); }

int sites_refuse(wfm_handle_t* h, size_t i, const std::string& why) {
  h->err = "wfm_sites_add_variants: variant " + std::to_string(i) + " " + why + "; nothing was added";
  return WFM_E_ARG;
}
}  // namespace
}  // extern "C++"

int wfm_sites_create(wfm_handle_t* h, uint64_t n_bases, uint32_t n_groups, wfm_sites_t** s) {
  if (!h || !s) return WFM_E_ARG;
  *s = nullptr;
  wfm_pav_t* eq = nullptr;
  if (int rc = wfm_pav_create(h, n_bases, n_groups, &eq)) {
    if (rc == WFM_E_ARG && !h->err.empty()) h->err = "wfm_sites_create: " + h->err;
    return rc;
  }
  eq->eq_only = true;
  std::unique_ptr<wfm_sites> p(new wfm_sites());
  p->device = h->device;
  p->n_bases = n_bases;
  p->n_groups = n_groups;
  p->eq = eq;
  *s = p.release();
  return WFM_OK;
}

void wfm_sites_free(wfm_sites_t* s) {
  if (!s) return;
  wfm_pav_free(s->eq);
  DeviceGuard on(s->device);
  s->work.release();
  s->tmp.release();
  if (s->vars) wfm_dfree(s->vars);
  if (s->alle) wfm_dfree(s->alle);
  delete s;
}

int wfm_sites_add_variants(wfm_handle_t* h, wfm_sites_t* s, const wfm_site_var_t* vars, size_t n, const char* alleles, size_t bytes) {
  if (!h || !s || (n && !vars) || (bytes && !alleles)) return WFM_E_ARG;
  if (n == 0) return WFM_OK;
  if (int rc = sites_usable(h, s)) return rc;
  if (n > SITES_MAX_VARS - s->n) { h->err = "wfm_sites_add_variants: more than 2^31 - 1 variants in one object; nothing was added"; return WFM_E_ARG; }
  // everything is looked at before anything is added
  std::vector<SiteVar> mine(n);
  std::vector<uint64_t> tasks;
  for (size_t i = 0; i < n; ++i) {
    const wfm_site_var_t& v = vars[i];
    if (v.kind > WFM_VAR_DEL) return sites_refuse(h, i, "has kind " + std::to_string(v.kind) + ", not SNV, INS or DEL");
    const bool fits = v.kind == WFM_VAR_SNV ? (v.ref_len == 1 && v.alt_len == 1)
                      : v.kind == WFM_VAR_INS ? (v.ref_len == 1 && v.alt_len >= 2)
                                              : (v.ref_len >= 2 && v.alt_len == 1);
    if (!fits) return sites_refuse(h, i, "has lengths " + std::to_string(v.ref_len) + " / " + std::to_string(v.alt_len) + " that do not fit its kind (SNV 1/1, INS 1/L+1, DEL L+1/1)");
    if (v.pos > s->n_bases || v.ref_len > s->n_bases - v.pos) return sites_refuse(h, i, "ends beyond the " + std::to_string(s->n_bases) + " target bases");
    if (v.group >= s->n_groups) return sites_refuse(h, i, "names group " + std::to_string(v.group) + ", not below " + std::to_string(s->n_groups));
    const uint64_t len = (uint64_t)v.ref_len + v.alt_len;
    if (v.off > bytes || len > bytes - v.off) return sites_refuse(h, i, "has alleles outside the " + std::to_string(bytes) + " allele bytes");
    mine[i] = SiteVar{v.pos, v.kind, v.group, v.ref_len, v.alt_len, v.off + s->bytes};
    if (len > WFM_SITES_SLICE)
      for (uint64_t piece = 0; piece * WFM_SITES_TASK < len; ++piece) tasks.push_back((uint64_t)(s->n + i) << 32 | piece);
  }
  HIPCHK(h, hipSetDevice(h->device));
  PassTimer tm(h);
  if (int rc = grow_block(h, &s->vars, &s->vcap, s->n, s->n + n, "sites variants")) return rc;
  if (int rc = grow_block(h, &s->alle, &s->acap, s->bytes, s->bytes + bytes, "sites alleles")) return rc;
  HIPCHK(h, hipMemcpyAsync(s->vars + s->n, mine.data(), n * sizeof(SiteVar), hipMemcpyHostToDevice, h->stream));
  if (bytes) {
    HIPCHK(h, hipMemcpyAsync(s->alle + s->bytes, alleles, bytes, hipMemcpyHostToDevice, h->stream));
    launch_sites_fold(s->alle + s->bytes, bytes, h->stream);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  s->tasks.insert(s->tasks.end(), tasks.begin(), tasks.end());
  s->n += n;
  s->bytes += bytes;
  s->added += n;
  if (tm.on)
    fprintf(stderr, "[wfm] sites add: %zu variants, %zu allele bytes, %zu long-allele tasks, %.3f ms (host clock, ends in a synchronise); the object holds %zu\n", n, bytes,
            tasks.size(), tm.host_ms(), s->n);
  return WFM_OK;
}

int wfm_sites_add_ref(wfm_handle_t* h, wfm_sites_t* s, const wfm_pav_prob_t* probs, size_t n, const uint32_t* runs, size_t n_runs_total, uint32_t* flags_out) {
  if (!h || !s) return WFM_E_ARG;
  if (int rc = sites_usable(h, s)) return rc;
  return wfm_pav_add(h, s->eq, probs, n, runs, n_runs_total, flags_out);
}

int wfm_sites_table(wfm_handle_t* h, wfm_sites_t* s, wfm_site_t** sites, size_t* n_sites, char** alleles, size_t* bytes, char** gt) {
  if (!h || !s || !sites || !n_sites || !alleles || !bytes || !gt) return WFM_E_ARG;
  *sites = nullptr; *n_sites = 0; *alleles = nullptr; *bytes = 0; *gt = nullptr;
  if (int rc = sites_usable(h, s)) return rc;
  s->last_sites = s->last_collisions = 0;
  if (s->n == 0) return WFM_OK;
  if (int rc = wfm_pav_union(h, s->eq)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  PassTimer tm(h);
  const uint32_t n = (uint32_t)s->n;
  const size_t G = s->n_groups, sb = (n + WFM_PAV_SCAN_BLOCK - 1) / WFM_PAV_SCAN_BLOCK, n_tasks = s->tasks.size();
  const int hb = env_num("WFM_SITES_HASH_BITS", 64);
  const unsigned hash_bits = (unsigned)std::min(64, std::max(0, hb));
  unsigned k1_bits = 2, g_bits = 0;
  while (k1_bits < 64 && ((s->n_bases << 2 | 3) >> k1_bits) != 0) ++k1_bits;   // (k1 <= n_bases << 2 | 3)
  while (g_bits < 32 && ((uint64_t)(G - 1) >> g_bits) != 0) ++g_bits;          // (k3 < n_groups, and n_groups >= 1: a variant names a group)
  // chunks of whole rows that hold at most WFM_SITES_OUT_MB MiB of the table, and no more cells than one launch takes
  const size_t cap = (size_t)std::min<unsigned long long>(cap_units("WFM_SITES_OUT_MB", G, 1), std::max<unsigned long long>(1, ((unsigned long long)1 << 30) / G));
  SitesWork w{};
  uint64_t* d_tasks;
  SiteRow* d_rows;
  uint8_t* d_gt;
  Carver cv{s->work, "sites table"};
  cv.piece(&w.k1, n); cv.piece(&w.k2, n); cv.piece(&w.kg, n); cv.piece(&w.ks, n);
  cv.piece(&w.k3, n); cv.piece(&w.sk3, n); cv.piece(&w.pa, n); cv.piece(&w.pb, n);
  cv.piece(&w.first, (size_t)n + 1); cv.piece(&w.gfirst, (size_t)n + 1);
  cv.piece(&w.flag, n); cv.piece(&d_tasks, n_tasks); cv.piece(&w.aux, sb + 2);
  if (int rc = cv.commit(h)) return rc;
  w.tasks = (const unsigned long long*)d_tasks;
  if (n_tasks) HIPCHK(h, hipMemcpyAsync(d_tasks, s->tasks.data(), n_tasks * 8, hipMemcpyHostToDevice, h->stream));
  launch_sites_keys(s->vars, s->alle, n, w, n_tasks, hash_bits, h->stream);
  HIPCHK(h, hipGetLastError());
  // the sorts, least significant word first; cur: the permutation so far, oth: the other block.  Each asks for its own room first
  uint32_t *cur = w.pa, *oth = w.pb;
  auto sort64 = [&](const unsigned long long* keys, unsigned bits) -> int {
    size_t tb = 0;
    launch_sites_gather64(keys, cur, n, w.kg, h->stream);
    HIPCHK(h, sites_sort64(nullptr, &tb, w.kg, w.ks, cur, oth, n, bits, h->stream));
    if (s->tmp.ensure(tb / 8 + 2)) { h->err = "out of device memory (sites sort)"; return WFM_E_NOMEM; }
    HIPCHK(h, sites_sort64(s->tmp.p, &tb, w.kg, w.ks, cur, oth, n, bits, h->stream));
    std::swap(cur, oth);
    return WFM_OK;
  };
  if (g_bits) {
    size_t tb = 0;
    HIPCHK(h, sites_sort32(nullptr, &tb, w.k3, w.sk3, cur, oth, n, g_bits, h->stream));
    if (s->tmp.ensure(tb / 8 + 2)) { h->err = "out of device memory (sites sort)"; return WFM_E_NOMEM; }
    HIPCHK(h, sites_sort32(s->tmp.p, &tb, w.k3, w.sk3, cur, oth, n, g_bits, h->stream));
    std::swap(cur, oth);
  }
  if (hash_bits)
    if (int rc = sort64(w.k2, hash_bits)) return rc;
  if (int rc = sort64(w.k1, k1_bits)) return rc;
  launch_sites_gather64(w.k2, cur, n, w.kg, h->stream);   // (w.ks: the sorted k1; w.kg: the sorted k2)
  launch_sites_gather32(w.k3, cur, n, w.sk3, h->stream);
  launch_sites_heads(s->vars, s->alle, n, w, cur, oth, n_tasks, h->stream);
  HIPCHK(h, hipGetLastError());
  unsigned long long tot[2] = {0, 0};
  HIPCHK(h, hipMemcpyAsync(tot, w.aux + sb, 16, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const size_t S = (size_t)(tot[0] & 0xffffffffull);
  s->last_collisions = tot[1];
  if (tot[1]) {
    h->err = "wfm_sites_table: " + std::to_string(tot[1]) + " neighbours of the sorted list have equal keys (pos, kind, a " + std::to_string(hash_bits) +
             "-bit hash of the alleles) and different alleles: a hash collision; nothing was written";
    return WFM_E_INTERNAL;
  }
  if (S == 0 || S > n) { h->err = "wfm_sites_table: the heads do not add up"; return WFM_E_INTERNAL; }
  const double t_join = tm.lap();
  // the rows' block lies where the keys of the sorts lay (k1, k2: 16 n bytes and S <= n rows of 32 need k1 .. ks, which are read no more)
  d_rows = (SiteRow*)w.k1;
  // a chunk of cells: behind everything, in the handle's output block
  if (h->outblk.ensure(Carver::words64(std::min(S, cap) * G) + 8)) { h->err = "out of device memory (sites cells)"; return WFM_E_NOMEM; }
  d_gt = (uint8_t*)h->outblk.p;
  launch_sites_rows(s->vars, cur, w.first, w.gfirst, (uint32_t)S, d_rows, h->stream);
  HIPCHK(h, hipGetLastError());
  const bool pinned = pin_pieces(h);
  std::unique_ptr<wfm_site_t, void (*)(void*)> rows((wfm_site_t*)malloc(S * sizeof(wfm_site_t)), free);
  std::unique_ptr<char, void (*)(void*)> cells((char*)malloc(std::max<size_t>(S * G, 1)), free);
  std::vector<char> folded(s->bytes);
  if (!rows || !cells) { h->err = "out of host memory (sites table)"; return WFM_E_NOMEM; }
  hipError_t e = copy_down(h, pinned, (char*)rows.get(), (const uint8_t*)d_rows, S * sizeof(wfm_site_t));
  if (e == hipSuccess) e = copy_down(h, pinned, folded.data(), s->alle, s->bytes);
  if (e != hipSuccess) { h->err = std::string("wfm_sites_table: ") + hipGetErrorString(e); return WFM_E_HIP; }
  size_t chunks = 0;
  for (size_t ra = 0, rb; ra < S && G; ra = rb, ++chunks) {
    rb = chunk_end(ra, S, cap, [](size_t a, size_t b) { return (unsigned long long)(b - a); });
    launch_sites_gt(d_rows, w.first, w.sk3, s->eq->ks(), s->eq->ke(), (const unsigned long long*)s->eq->c.p, s->eq->n, ra, rb, s->n_groups, d_gt, h->stream);
    e = hipGetLastError();
    if (e == hipSuccess) e = copy_down(h, pinned, cells.get() + ra * G, d_gt, (rb - ra) * G);  // (the block is the next chunk's)
    if (e != hipSuccess) { h->err = std::string("wfm_sites_table: ") + hipGetErrorString(e); return WFM_E_HIP; }
  }
  // one representative's bytes per site, in site order
  size_t ab = 0;
  for (size_t i = 0; i < S; ++i) ab += (size_t)rows.get()[i].ref_len + rows.get()[i].alt_len;
  char* out_alle = (char*)malloc(std::max<size_t>(ab, 1));
  if (!out_alle) { h->err = "out of host memory (sites alleles)"; return WFM_E_NOMEM; }
  size_t at = 0;
  for (size_t i = 0; i < S; ++i) {
    wfm_site_t& r = rows.get()[i];
    const size_t len = (size_t)r.ref_len + r.alt_len;
    memcpy(out_alle + at, folded.data() + r.off, len);
    r.off = at;
    at += len;
  }
  s->last_sites = S;
  *sites = rows.release(); *n_sites = S; *alleles = out_alle; *bytes = ab; *gt = cells.release();
  if (tm.on)
    fprintf(stderr, "[wfm] sites table: %u variants (%zu long-allele tasks) to %zu sites in %.3f ms (keys, %u + %u + %u sorted bits, heads), %zu x %zu cells over %zu = intervals in %zu chunks, rows and bytes in %.3f ms (host clock)\n",
            n, n_tasks, S, t_join, g_bits, hash_bits, k1_bits, S, G, s->eq->n, chunks, tm.lap());
  return WFM_OK;
}

int wfm_sites_export(wfm_handle_t* h, wfm_sites_t* s, wfm_site_var_t** vars, size_t* n, char** alleles, size_t* bytes, wfm_pav_seg_t** segs, size_t* n_segs) {
  if (!h || !s || !vars || !n || !alleles || !bytes || !segs || !n_segs) return WFM_E_ARG;
  *vars = nullptr; *n = 0; *alleles = nullptr; *bytes = 0; *segs = nullptr; *n_segs = 0;
  if (int rc = sites_usable(h, s)) return rc;
  if (int rc = wfm_pav_export(h, s->eq, segs, n_segs)) return rc;
  if (s->n == 0) return WFM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  wfm_site_var_t* v = (wfm_site_var_t*)malloc(s->n * sizeof(wfm_site_var_t));
  char* a = (char*)malloc(std::max<size_t>(s->bytes, 1));
  const bool pinned = pin_pieces(h);
  hipError_t e = hipSuccess;
  if (v && a) e = copy_down(h, pinned, (char*)v, (const uint8_t*)s->vars, s->n * sizeof(wfm_site_var_t));
  if (v && a && e == hipSuccess) e = copy_down(h, pinned, a, s->alle, s->bytes);
  if (!v || !a || e != hipSuccess) {
    free(v); free(a); wfm_pav_free_list(*segs);
    *segs = nullptr; *n_segs = 0;
    if (e != hipSuccess) { h->err = std::string("wfm_sites_export: ") + hipGetErrorString(e); return WFM_E_HIP; }
    h->err = "out of host memory (sites list)";
    return WFM_E_NOMEM;
  }
  *vars = v; *n = s->n; *alleles = a; *bytes = s->bytes;
  return WFM_OK;
}

int wfm_sites_import(wfm_handle_t* h, wfm_sites_t* s, const wfm_site_var_t* vars, size_t n, const char* alleles, size_t bytes, const wfm_pav_seg_t* segs,
                     size_t n_segs) {
  if (!h || !s) return WFM_E_ARG;
  if (int rc = wfm_sites_add_variants(h, s, vars, n, alleles, bytes)) return rc;
  return wfm_pav_import(h, s->eq, segs, n_segs);
}

int wfm_sites_counts(const wfm_sites_t* s, uint64_t out[4]) {
  if (!s || !out) return WFM_E_ARG;
  out[0] = s->added; out[1] = s->last_sites; out[2] = s->eq->n_union; out[3] = s->last_collisions;
  return WFM_OK;
}

void wfm_sites_free_list(void* p) { free(p); }

// ---- a net across records: which record owns each target base (wfmash_hip.h; the kernels and the sorts: wfa_net.hip) ----
struct wfm_net {
  int device = 0;
  uint64_t n_bases = 0;
  NetBlock* blocks = nullptr;     // the raw blocks
  size_t bcap = 0, n = 0;
  NetRec* recs = nullptr;         // the record entries
  size_t rcap = 0, r = 0;
  std::vector<uint64_t> orders;   // the entries' orders once more, on the host: what import looks a block's record up in
  DevBuf<uint64_t> work;          // an add call's problems, runs, flags, words and offsets; the table's block ends, coordinates and ranks
  DevBuf<uint64_t> rw;            // the table's record keys, ranks, priorities and rows
  DevBuf<uint64_t> tree;          // the table's tree
  DevBuf<uint64_t> pc;            // the table's pieces, their keys and permutations
  DevBuf<uint64_t> tmp;           // the sorts' own
  uint64_t last_m = 0, last_pieces = 0, last_lost = 0;
};

extern "C++" {
namespace {
static_assert(sizeof(wfm_net_prob_t) == 32 && sizeof(NetProb) == 32 && sizeof(wfm_net_block_t) == 24 && sizeof(NetBlock) == 24 &&
              sizeof(wfm_net_rec_t) == 16 && sizeof(NetRec) == 16 && sizeof(wfm_netcall_t) == 48 && sizeof(NetPer) == 48, "wfmash_hip.h states these sizes");
constexpr size_t NET_MAX = ((size_t)1 << 31) - 1;  // blocks, and records: a winner is priority << 32 | block index

int net_usable(wfm_handle_t* h, const wfm_net_t* net) { return DeviceGuard::usable(h, net->device, "the net object"); }
unsigned bits_of(uint64_t v) { unsigned b = 0; while (b < 64 && (v >> b) != 0) ++b; return b; }
}  // namespace
}  // extern "C++"

int wfm_net_create(wfm_handle_t* h, uint64_t n_bases, wfm_net_t** net) {
  if (!h || !net) return WFM_E_ARG;
  *net = nullptr;
  if (n_bases >= ((uint64_t)1 << 40)) {
    h->err = "wfm_net_create: " + std::to_string(n_bases) + " target bases: fewer than 2^40, as wfm_pav_create";
    return WFM_E_ARG;
  }
  HIPCHK(h, hipSetDevice(h->device));
  std::unique_ptr<wfm_net> p(new wfm_net());
  p->device = h->device;
  p->n_bases = n_bases;
  *net = p.release();
  return WFM_OK;
}

void wfm_net_free(wfm_net_t* net) {
  if (!net) return;
  DeviceGuard on(net->device);
  net->work.release(); net->rw.release(); net->tree.release(); net->pc.release(); net->tmp.release();
  if (net->blocks) wfm_dfree(net->blocks);
  if (net->recs) wfm_dfree(net->recs);
  delete net;
}

int wfm_net_add(wfm_handle_t* h, wfm_net_t* net, const wfm_net_prob_t* probs, size_t n, const uint32_t* runs, size_t n_runs_total, uint32_t* flags_out) {
  if (!net) return WFM_E_ARG;
  PassTimer tm(h);
  NetProb* d_probs;
  uint32_t *d_runs, *d_flags, *d_score;
  unsigned long long *d_word, *d_off;
  Carver cv{net->work, "net add"};
  const int rc0 = add_preface(h, net, net->device, "the net object", "wfm_net_add", cv, probs, n, runs, n_runs_total, flags_out, &d_probs, &d_runs,
                              [&] { cv.piece(&d_flags, n); cv.piece(&d_score, n); cv.piece(&d_word, n); cv.piece(&d_off, n + 1); return WFM_OK; });
  if (rc0 || !d_probs) return rc0;
  launch_net_count(d_runs, d_probs, (int)n, net->n_bases, d_flags, d_word, d_off, d_score, h->stream);
  HIPCHK(h, hipGetLastError());
  unsigned long long total = 0;
  HIPCHK(h, hipMemcpyAsync(flags_out, d_flags, n * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(&total, d_off + n, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const int spans = count_flagged(flags_out, n, WFM_NET_SPANS);
  const size_t add_r = (size_t)(total >> 32), add_b = (size_t)(total & 0xffffffffull);
  if (add_r != n - (size_t)spans) { h->err = "wfm_net_add: the records do not add up"; return WFM_E_INTERNAL; }
  if (add_r) {
    if (add_b > NET_MAX - net->n || add_r > NET_MAX - net->r) { h->err = "wfm_net_add: more than 2^31 - 1 blocks or records in one object; nothing was added"; return WFM_E_ARG; }
    if (int rc = grow_block(h, &net->blocks, &net->bcap, net->n, net->n + add_b, "net blocks")) return rc;
    if (int rc = grow_block(h, &net->recs, &net->rcap, net->r, net->r + add_r, "net records")) return rc;
    launch_net_write(d_runs, d_probs, (int)n, d_flags, d_off, d_score, net->blocks + net->n, net->recs + net->r, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    net->n += add_b;
    net->r += add_r;
    for (size_t i = 0; i < n; ++i)
      if (!(flags_out[i] & WFM_NET_SPANS)) net->orders.push_back(probs[i].order);
  }
  if (tm.on)
    fprintf(stderr, "[wfm] net add: %zu problems, %zu runs, %zu blocks, %d flagged, %.3f ms (host clock, ends in a synchronise); the object holds %zu blocks of %zu records\n",
            n, n_runs_total, add_b, spans, tm.host_ms(), net->n, net->r);
  return spans;
}

int wfm_net_table(wfm_handle_t* h, wfm_net_t* net, wfm_net_piece_t** pieces, size_t* n_pieces, wfm_netcall_t** per, size_t* n_records) {
  if (!h || !net || !pieces || !n_pieces || !per || !n_records) return WFM_E_ARG;
  *pieces = nullptr; *n_pieces = 0; *per = nullptr; *n_records = 0;
  if (int rc = net_usable(h, net)) return rc;
  net->last_m = net->last_pieces = net->last_lost = 0;
  if (net->r == 0) return WFM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  PassTimer tm(h);
  auto lap = [&]() -> double {  // (WFM_DEBUG alone pays for the waits)
    if (!tm.on) return 0.0;
    (void)hipStreamSynchronize(h->stream);
    return tm.lap();
  };
  const size_t N = net->n, R = net->r, sb = (2 * N + WFM_NET_SCAN_BLOCK - 1) / WFM_NET_SCAN_BLOCK;
  NetWork w{};
  w.blocks = net->blocks; w.n = N; w.recs = net->recs; w.r = (uint32_t)R;
  NetPer* d_per;
  {
    Carver cv{net->rw, "net table: records"};
    cv.piece(&w.ro, R); cv.piece(&w.so, R); cv.piece(&w.k2, R); cv.piece(&w.k2s, R); cv.piece(&w.aligned, R); cv.piece(&w.won, R);
    cv.piece(&d_per, R); cv.piece(&w.ri, R); cv.piece(&w.sp, R); cv.piece(&w.p2, R); cv.piece(&w.prio, R); cv.piece(&w.sscore, R); cv.piece(&w.bad, 2);
    if (int rc = cv.commit(h)) return rc;
  }
  {
    Carver cv{net->work, "net table: blocks"};
    cv.piece(&w.e, 2 * N); cv.piece(&w.e2, 2 * N); cv.piece(&w.aux, sb + 2); cv.piece(&w.brank, N);
    if (int rc = cv.commit(h)) return rc;
  }
  auto room = [&](size_t bytes) -> int {
    if (net->tmp.ensure(bytes / 8 + 2)) { h->err = "out of device memory (net sort)"; return WFM_E_NOMEM; }
    return WFM_OK;
  };
  // the records: ranked by order, then by (score descending, order ascending) into the priorities R .. 1
  HIPCHK(h, hipMemsetAsync(w.aligned, 0, R * 8, h->stream));
  HIPCHK(h, hipMemsetAsync(w.won, 0, R * 8, h->stream));
  HIPCHK(h, hipMemsetAsync(w.bad, 0, 8, h->stream));
  launch_net_rec_keys(w, h->stream);
  size_t tb = 0;
  HIPCHK(h, sites_sort64(nullptr, &tb, w.ro, w.so, w.ri, w.sp, (uint32_t)R, 64, h->stream));
  if (int rc = room(tb)) return rc;
  HIPCHK(h, sites_sort64(net->tmp.p, &tb, w.ro, w.so, w.ri, w.sp, (uint32_t)R, 64, h->stream));
  launch_net_rec_rank(w, h->stream);
  HIPCHK(h, sites_sort64(nullptr, &tb, w.k2, w.k2s, w.ri, w.p2, (uint32_t)R, 64, h->stream));
  if (int rc = room(tb)) return rc;
  HIPCHK(h, sites_sort64(net->tmp.p, &tb, w.k2, w.k2s, w.ri, w.p2, (uint32_t)R, 64, h->stream));
  launch_net_prio(w, h->stream);
  HIPCHK(h, hipGetLastError());
  // the block ends, sorted, to the distinct coordinates
  unsigned long long distinct = 0;
  uint32_t bad[2] = {0, 0};
  if (N) {
    launch_net_ends(w, h->stream);
    const unsigned end_bit = std::max(1u, bits_of(net->n_bases));  // (an end is n_bases at most)
    HIPCHK(h, net_sort_keys(nullptr, &tb, w.e, w.e2, 2 * N, end_bit, h->stream));
    if (int rc = room(tb)) return rc;
    HIPCHK(h, net_sort_keys(net->tmp.p, &tb, w.e, w.e2, 2 * N, end_bit, h->stream));
    launch_net_distinct(w, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(&distinct, w.aux + sb, 8, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipMemcpyAsync(bad, w.bad, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (bad[0]) { h->err = "wfm_net_table: two records have the same order; nothing was written"; return WFM_E_ARG; }
  if (N && (distinct < 2 || distinct > 2 * N)) { h->err = "wfm_net_table: the coordinates do not add up"; return WFM_E_INTERNAL; }
  const double t_sort = lap();
  const size_t M = N ? (size_t)distinct - 1 : 0;
  w.m = M;
  size_t P = 0;
  double t_fill = 0, t_push = 0, t_compact = 0;
  if (M) {
    if (net->tree.ensure(2 * M + 2)) { h->err = "out of device memory (net table: tree)"; return WFM_E_NOMEM; }
    w.tree = (unsigned long long*)net->tree.p;
    HIPCHK(h, hipMemsetAsync(w.tree, 0, 2 * M * 8, h->stream));
    launch_net_fill(w, h->stream);
    HIPCHK(h, hipGetLastError());
    t_fill = lap();
    launch_net_push(w, h->stream);
    HIPCHK(h, hipGetLastError());
    t_push = lap();
    launch_net_heads_count(w, h->stream);
    HIPCHK(h, hipGetLastError());
    unsigned long long heads = 0;
    const size_t mb = (M + WFM_NET_SCAN_BLOCK - 1) / WFM_NET_SCAN_BLOCK;
    HIPCHK(h, hipMemcpyAsync(&heads, w.aux + mb, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(bad, w.bad, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (bad[1]) { h->err = "wfm_net_table: a block names a record that is not in the object"; return WFM_E_INTERNAL; }
    if (heads == 0 || heads > M) { h->err = "wfm_net_table: the heads do not add up"; return WFM_E_INTERNAL; }
    P = (size_t)heads;
    w.p = P;
    Carver cv{net->pc, "net table: pieces"};
    cv.piece(&w.ps, P); cv.piece(&w.pe, P); cv.piece(&w.pw, P); cv.piece(&w.key, P); cv.piece(&w.val, P); cv.piece(&w.sk, P); cv.piece(&w.sv, P);
    if (int rc = cv.commit(h)) return rc;
    launch_net_heads_write(w, h->stream);
    launch_net_piece_keys(w, h->stream);
    HIPCHK(h, hipGetLastError());
    // the pieces arrive in t order: a stable sort by the rank of their record leaves them sorted by (order, t)
    const unsigned kb = bits_of(R - 1);
    if (kb) {
      HIPCHK(h, sites_sort32(nullptr, &tb, w.key, w.sk, w.val, w.sv, (uint32_t)P, kb, h->stream));
      if (int rc = room(tb)) return rc;
      HIPCHK(h, sites_sort32(net->tmp.p, &tb, w.key, w.sk, w.val, w.sv, (uint32_t)P, kb, h->stream));
    } else {
      w.sk = w.key; w.sv = w.val;
    }
    t_compact = lap();
  }
  launch_net_per(w, d_per, h->stream);
  HIPCHK(h, hipGetLastError());
  // the way down: the rows, then the pieces in chunks of at most WFM_NET_OUT_MB MiB through the handle's output block
  const size_t cap = (size_t)cap_units("WFM_NET_OUT_MB", sizeof(wfm_net_piece_t), 1);
  std::unique_ptr<wfm_netcall_t, void (*)(void*)> rows((wfm_netcall_t*)malloc(R * sizeof(wfm_netcall_t)), free);
  std::unique_ptr<char, void (*)(void*)> out((char*)malloc(std::max<size_t>(P, 1) * sizeof(wfm_net_piece_t)), free);
  if (!rows || !out) { h->err = "out of host memory (net table)"; return WFM_E_NOMEM; }
  const bool pinned = pin_pieces(h);
  hipError_t e = copy_down(h, pinned, (char*)rows.get(), (const uint8_t*)d_per, R * sizeof(wfm_netcall_t));
  if (e != hipSuccess) { h->err = std::string("wfm_net_table: ") + hipGetErrorString(e); return WFM_E_HIP; }
  size_t chunks = 0;
  if (P) {
    if (h->outblk.ensure(Carver::words64(std::min(P, cap) * sizeof(wfm_net_piece_t)) + 8)) { h->err = "out of device memory (net pieces)"; return WFM_E_NOMEM; }
    NetBlock* d_out = (NetBlock*)h->outblk.p;
    for (size_t a = 0, b; a < P; a = b, ++chunks) {
      b = chunk_end(a, P, cap, [](size_t x, size_t y) { return (unsigned long long)(y - x); });
      launch_net_pieces(w, a, b, d_out, h->stream);
      e = hipGetLastError();
      if (e == hipSuccess) e = copy_down(h, pinned, out.get() + a * sizeof(wfm_net_piece_t), (const uint8_t*)d_out, (b - a) * sizeof(wfm_net_piece_t));  // (the block is the next chunk's)
      if (e != hipSuccess) { h->err = std::string("wfm_net_table: ") + hipGetErrorString(e); return WFM_E_HIP; }
    }
  }
  uint64_t lost = 0;
  for (size_t i = 0; i < R; ++i) lost += rows.get()[i].count == 0;
  net->last_m = M; net->last_pieces = P; net->last_lost = lost;
  *n_pieces = P; *n_records = R;
  *per = rows.release();
  if (P) *pieces = (wfm_net_piece_t*)out.release();
  if (tm.on)
    fprintf(stderr, "[wfm] net table: %zu blocks of %zu records, %zu elementary intervals, %zu pieces, %llu records won nothing; sorts %.3f ms, tree fill %.3f ms, push-down %.3f ms, compaction and piece sort %.3f ms, rows and %zu chunks down %.3f ms, the call %.3f ms (host clock)\n",
            N, R, M, P, (unsigned long long)lost, t_sort, t_fill, t_push, t_compact, chunks, tm.lap(), tm.host_ms());
  return WFM_OK;
}

int wfm_net_export(wfm_handle_t* h, wfm_net_t* net, wfm_net_block_t** blocks, size_t* n_blocks, wfm_net_rec_t** recs, size_t* n_recs) {
  if (!h || !net || !blocks || !n_blocks || !recs || !n_recs) return WFM_E_ARG;
  *blocks = nullptr; *n_blocks = 0; *recs = nullptr; *n_recs = 0;
  if (int rc = net_usable(h, net)) return rc;
  if (net->r == 0) return WFM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  wfm_net_block_t* b = (wfm_net_block_t*)malloc(std::max<size_t>(net->n, 1) * sizeof(wfm_net_block_t));
  wfm_net_rec_t* r = (wfm_net_rec_t*)malloc(net->r * sizeof(wfm_net_rec_t));
  const bool pinned = pin_pieces(h);
  hipError_t e = hipSuccess;
  if (b && r) e = copy_down(h, pinned, (char*)b, (const uint8_t*)net->blocks, net->n * sizeof(wfm_net_block_t));
  if (b && r && e == hipSuccess) e = copy_down(h, pinned, (char*)r, (const uint8_t*)net->recs, net->r * sizeof(wfm_net_rec_t));
  if (!b || !r || e != hipSuccess) {
    free(b); free(r);
    if (e != hipSuccess) { h->err = std::string("wfm_net_export: ") + hipGetErrorString(e); return WFM_E_HIP; }
    h->err = "out of host memory (net list)";
    return WFM_E_NOMEM;
  }
  if (net->n) { *blocks = b; *n_blocks = net->n; } else free(b);
  *recs = r; *n_recs = net->r;
  return WFM_OK;
}

int wfm_net_import(wfm_handle_t* h, wfm_net_t* net, const wfm_net_block_t* blocks, size_t n_blocks, const wfm_net_rec_t* recs, size_t n_recs) {
  if (!h || !net || (n_blocks && !blocks) || (n_recs && !recs)) return WFM_E_ARG;
  if (n_blocks == 0 && n_recs == 0) return WFM_OK;
  if (int rc = net_usable(h, net)) return rc;
  if (n_blocks > NET_MAX - net->n || n_recs > NET_MAX - net->r) { h->err = "wfm_net_import: more than 2^31 - 1 blocks or records in one object; nothing was added"; return WFM_E_ARG; }
  // everything is looked at before anything is added
  std::vector<uint64_t> known(net->orders);
  known.reserve(known.size() + n_recs);
  for (size_t i = 0; i < n_recs; ++i) known.push_back(recs[i].order);
  std::sort(known.begin(), known.end());
  for (size_t i = 0; i < n_blocks; ++i) {
    const wfm_net_block_t& b = blocks[i];
    if (b.size == 0 || b.t > net->n_bases || b.size > net->n_bases - b.t || (uint64_t)b.q + b.size > 0xffffffffull) {
      h->err = "wfm_net_import: block " + std::to_string(i) + " is empty, leaves the " + std::to_string(net->n_bases) + " target bases or ends beyond 2^32 query bases; nothing was added";
      return WFM_E_ARG;
    }
    if (!std::binary_search(known.begin(), known.end(), b.order)) {
      h->err = "wfm_net_import: block " + std::to_string(i) + " names the record of order " + std::to_string(b.order) + ", which is neither given nor in the object; nothing was added";
      return WFM_E_ARG;
    }
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = grow_block(h, &net->blocks, &net->bcap, net->n, net->n + n_blocks, "net blocks")) return rc;
  if (int rc = grow_block(h, &net->recs, &net->rcap, net->r, net->r + n_recs, "net records")) return rc;
  std::vector<NetRec> mine(n_recs);
  for (size_t i = 0; i < n_recs; ++i) mine[i] = NetRec{recs[i].order, recs[i].score, 0u};
  if (n_blocks) HIPCHK(h, hipMemcpyAsync(net->blocks + net->n, blocks, n_blocks * sizeof(NetBlock), hipMemcpyHostToDevice, h->stream));
  if (n_recs) HIPCHK(h, hipMemcpyAsync(net->recs + net->r, mine.data(), n_recs * sizeof(NetRec), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  net->n += n_blocks;
  net->r += n_recs;
  for (size_t i = 0; i < n_recs; ++i) net->orders.push_back(recs[i].order);
  return WFM_OK;
}

int wfm_net_counts(const wfm_net_t* net, uint64_t out[6]) {
  if (!net || !out) return WFM_E_ARG;
  out[0] = net->r; out[1] = net->n; out[2] = net->last_m; out[3] = net->last_pieces; out[4] = net->last_lost; out[5] = 0;
  return WFM_OK;
}

void wfm_net_free_list(void* p) { free(p); }

// ---- transitive lifts: intervals closed over all records, both ways (wfmash_hip.h; the kernels: wfa_trans.hip, the union: wfa_pav.hip) ----
struct wfm_trans {
  int device = 0;
  uint64_t n_bases = 0;
  uint4* pre = nullptr;                 // the records' prefix words, n_runs + 1 each
  size_t pcap = 0, np = 0;
  TransArc* arcs = nullptr;             // two per record, as they came
  size_t acap = 0, na = 0;
  std::vector<wfm_trans_rec_t> recs;    // the records once more, on the host: what export gives (pre_off: in pre)
  bool indexed = false;
  DevBuf<uint64_t> index;               // the arcs sorted by source start (4 words each), then pm and the blocks' maxima
  DevBuf<unsigned long long> acc, snap, prev;  // a closure's list as it grows, the list a round projects, the list of the round before (ks, then ke)
  DevBuf<uint64_t> tmp;                 // the sorts' own
  uint64_t last_rounds = 0, last_ivs = 0, last_pairs = 0;
  const TransArc* sorted() const { return (const TransArc*)index.p; }
  const unsigned long long* pm() const { return (const unsigned long long*)(index.p + 4 * na); }
};

extern "C++" {
namespace {
static_assert(sizeof(wfm_trans_prob_t) == 32 && sizeof(wfm_trans_rec_t) == 32 && sizeof(wfm_trans_word_t) == 16 && sizeof(wfm_trans_iv_t) == 24 &&
              sizeof(wfm_trans_seed_t) == 24, "wfmash_hip.h states these sizes");
constexpr unsigned TRANS_SHIFT = 40;
constexpr size_t TRANS_MAX = ((size_t)1 << 31) - 1;  // intervals of a list (one workgroup each), and arcs

int trans_usable(wfm_handle_t* h, const wfm_trans_t* obj) { return DeviceGuard::usable(h, obj->device, "the trans object"); }

// room for add_words more prefix words and add_recs more records, under WFM_TRANS_GB; nothing is changed where it fails
int trans_reserve(wfm_handle_t* h, wfm_trans_t* obj, const char* who, size_t add_words, size_t add_recs) {
  if (add_recs > (TRANS_MAX - obj->na) / 2) { h->err = std::string(who) + ": more than 2^31 - 1 arcs in one object; nothing was added"; return WFM_E_ARG; }
  // (an arc is kept twice, as it came and sorted, with 8 bytes of running maximum)
  const double gib = env_decimal("WFM_TRANS_GB", 32.0);
  const double need = ((double)(obj->np + add_words) * 16.0 + (double)(obj->na + 2 * add_recs) * 72.0) / 1073741824.0;
  if (need > gib) {
    char msg[240];
    snprintf(msg, sizeof msg, "%s: the transitive pass would keep %.3f GiB of prefix words and arcs on the device, more than WFM_TRANS_GB = %.3f; nothing was added",
             who, need, gib);
    h->err = msg;
    return WFM_E_NOMEM;
  }
  if (int rc = grow_block(h, &obj->pre, &obj->pcap, obj->np, obj->np + add_words, "transitive prefix words")) return rc;
  return grow_block(h, &obj->arcs, &obj->acap, obj->na, obj->na + 2 * add_recs, "transitive arcs");
}

// the two arcs of a record whose words begin at `at` of the object's block
void trans_arcs_of(const wfm_trans_rec_t& r, uint64_t at, uint32_t pspan, uint32_t tspan, TransArc out[2]) {
  const uint64_t rev = (r.flags & WFM_TRANS_REVERSE) ? TRANS_ARC_REVERSE : 0;
  out[0] = TransArc{r.t, r.q, at | rev, pspan, r.n_runs};
  out[1] = TransArc{r.q, r.t, at | rev | TRANS_ARC_BACK, tspan, r.n_runs};
}

// the arcs sorted by source start and pm, where something was added since they were made
int trans_index(wfm_handle_t* h, wfm_trans_t* obj) {
  if (obj->indexed) return WFM_OK;
  const size_t n = obj->na, nb = (n + WFM_TRANS_SCAN_BLOCK - 1) / WFM_TRANS_SCAN_BLOCK;
  if (n) {
    unsigned long long *key, *idx, *key2, *idx2;
    Carver cv{h->scratch, "transitive index"};
    cv.piece(&key, n); cv.piece(&idx, n); cv.piece(&key2, n); cv.piece(&idx2, n);
    if (int rc = cv.commit(h)) return rc;
    if (obj->index.ensure(5 * n + nb + 2)) { h->err = "out of device memory (transitive index)"; return WFM_E_NOMEM; }
    launch_trans_keys(obj->arcs, n, key, idx, h->stream);
    HIPCHK(h, hipGetLastError());
    const unsigned end_bit = std::max(1u, bits_of(obj->n_bases));  // (a source start is at most n_bases)
    size_t tmp_bytes = 0;
    HIPCHK(h, pav_sort(nullptr, &tmp_bytes, key, key2, idx, idx2, n, end_bit, h->stream));
    if (obj->tmp.ensure(tmp_bytes / 8 + 2)) { h->err = "out of device memory (transitive sort)"; return WFM_E_NOMEM; }
    HIPCHK(h, pav_sort(obj->tmp.p, &tmp_bytes, key, key2, idx, idx2, n, end_bit, h->stream));
    unsigned long long* pm = (unsigned long long*)(obj->index.p + 4 * n);
    launch_trans_index(obj->arcs, idx2, n, (TransArc*)obj->index.p, pm + n, pm, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  obj->indexed = true;
  return WFM_OK;
}

// acc = the union of acc's m intervals and the c pairs that launch(raw ks tail, raw ke tail) writes; *m = its intervals
template <class Launch>
int trans_union(wfm_handle_t* h, wfm_trans_t* obj, size_t* m, size_t c, unsigned end_bit, Launch launch) {
  const size_t n = *m + c, nb = (n + WFM_PAV_SCAN_BLOCK - 1) / WFM_PAV_SCAN_BLOCK;
  if (n > TRANS_MAX) { h->err = "wfm_trans_closure: more than 2^31 - 1 intervals in one round; lower WFM_TRANS_OUT_MB or take fewer seeds a call"; return WFM_E_ARG; }
  unsigned long long *rks, *rke, *sks, *ske, *aux;
  Carver cv{h->outblk, "transitive union"};
  cv.piece(&rks, n); cv.piece(&rke, n); cv.piece(&sks, n); cv.piece(&ske, n); cv.piece(&aux, nb + 1);
  if (int rc = cv.commit(h)) return rc;
  HIPCHK(h, hipMemcpyAsync(rks, obj->acc.p, *m * 8, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(rke, obj->acc.p + *m, *m * 8, hipMemcpyDeviceToDevice, h->stream));
  launch(rks + *m, rke + *m);
  HIPCHK(h, hipGetLastError());
  // (the end keys follow the start keys at the union's own length, which is known only behind the compaction: compact to the raw copy, then move)
  unsigned long long u = 0;
  const int rc = interval_union(h, obj->tmp, "out of device memory (transitive sort)", rks, rke, sks, ske, n, end_bit, aux, rks, rke, &u, [&] {
    // (acc's intervals are in the raw copy: the block may be replaced.  A union has no more intervals than the list has segments)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (obj->acc.ensure(2 * n)) { h->err = "out of device memory (transitive list)"; return (int)WFM_E_NOMEM; }
    return (int)WFM_OK;
  });
  if (rc != WFM_OK) return rc;
  if (u == 0 || u > n) { h->err = "wfm_trans_closure: the union does not add up"; return WFM_E_INTERNAL; }
  HIPCHK(h, hipMemcpyAsync(obj->acc.p, rks, (size_t)u * 8, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(obj->acc.p + u, rke, (size_t)u * 8, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *m = (size_t)u;
  return WFM_OK;
}

// the bases the m intervals of acc cover
int trans_bases(wfm_handle_t* h, wfm_trans_t* obj, size_t m, unsigned long long* bases) {
  const size_t nb = (m + WFM_PAV_SCAN_BLOCK - 1) / WFM_PAV_SCAN_BLOCK;
  unsigned long long *C, *aux;
  Carver cv{h->outblk, "transitive prefix"};
  cv.piece(&C, m + 1); cv.piece(&aux, nb + 1);
  if (int rc = cv.commit(h)) return rc;
  launch_pav_prefix(obj->acc.p, obj->acc.p + m, m, aux, C, h->stream);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(bases, C + m, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return WFM_OK;
}
}  // namespace
}  // extern "C++"

int wfm_trans_create(wfm_handle_t* h, uint64_t n_bases, wfm_trans_t** obj) {
  if (!h || !obj) return WFM_E_ARG;
  *obj = nullptr;
  if (n_bases >= ((uint64_t)1 << TRANS_SHIFT)) {
    h->err = "wfm_trans_create: a world of " + std::to_string(n_bases) + " bases: fewer than 2^40, as wfm_pav_create";
    return WFM_E_ARG;
  }
  HIPCHK(h, hipSetDevice(h->device));
  std::unique_ptr<wfm_trans> p(new wfm_trans());
  p->device = h->device;
  p->n_bases = n_bases;
  *obj = p.release();
  return WFM_OK;
}

void wfm_trans_free(wfm_trans_t* obj) {
  if (!obj) return;
  DeviceGuard on(obj->device);
  obj->index.release(); obj->acc.release(); obj->snap.release(); obj->prev.release(); obj->tmp.release();
  if (obj->pre) wfm_dfree(obj->pre);
  if (obj->arcs) wfm_dfree(obj->arcs);
  delete obj;
}

int wfm_trans_add(wfm_handle_t* h, wfm_trans_t* obj, const wfm_trans_prob_t* probs, size_t n, const uint32_t* runs, size_t n_runs_total, uint32_t* flags_out) {
  if (!h || !obj) return WFM_E_ARG;
  PassTimer tm(h);
  TransProb* d_probs;
  TransSpan* d_span;
  unsigned long long* d_at;
  uint32_t* d_runs;
  Carver cv{h->scratch, "transitive add"};
  const int rc0 = add_preface(h, obj, obj->device, "the trans object", "wfm_trans_add", cv, probs, n, runs, n_runs_total, flags_out, &d_probs, &d_runs, [&] {
    for (size_t i = 0; i < n; ++i)
      if (probs[i].flags & ~WFM_TRANS_REVERSE) {
        h->err = "problem " + std::to_string(i) + ": flags " + std::to_string(probs[i].flags) + " hold a bit that is not WFM_TRANS_REVERSE";
        return (int)WFM_E_ARG;
      }
    cv.piece(&d_span, n); cv.piece(&d_at, n);
    return (int)WFM_OK;
  });
  if (rc0 || !d_probs) return rc0;
  launch_trans_span(d_runs, d_probs, (int)n, obj->n_bases, d_span, h->stream);
  HIPCHK(h, hipGetLastError());
  std::vector<TransSpan> span(n);
  HIPCHK(h, hipMemcpyAsync(span.data(), d_span, n * sizeof(TransSpan), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // what is kept, and where: nothing is written before this is settled
  std::vector<unsigned long long> at(n, ~0ull);
  std::vector<TransArc> arcs;
  std::vector<wfm_trans_rec_t> recs;
  size_t words = 0;
  int spans = 0;
  for (size_t i = 0; i < n; ++i) {
    flags_out[i] = span[i].flags;
    if (span[i].flags & WFM_TRANS_SPANS) { ++spans; continue; }
    at[i] = obj->np + words;
    recs.push_back(wfm_trans_rec_t{probs[i].t, probs[i].q, at[i], probs[i].n_runs, probs[i].flags});
    TransArc two[2];
    trans_arcs_of(recs.back(), at[i], span[i].pspan, span[i].tspan, two);
    arcs.push_back(two[0]); arcs.push_back(two[1]);
    words += (size_t)probs[i].n_runs + 1;
  }
  if (!recs.empty()) {
    if (int rc = trans_reserve(h, obj, "wfm_trans_add", words, recs.size())) return rc;
    HIPCHK(h, hipMemcpyAsync(d_at, at.data(), n * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(obj->arcs + obj->na, arcs.data(), arcs.size() * sizeof(TransArc), hipMemcpyHostToDevice, h->stream));
    launch_trans_pre(d_runs, d_probs, (int)n, d_at, obj->pre, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    obj->np += words;
    obj->na += arcs.size();
    obj->recs.insert(obj->recs.end(), recs.begin(), recs.end());
    obj->indexed = false;
  }
  if (tm.on)
    fprintf(stderr, "[wfm] transitive add: %zu problems, %zu runs, %d flagged, %.3f ms (host clock, ends in a synchronise); the object holds %zu words of %zu records\n",
            n, n_runs_total, spans, tm.host_ms(), obj->np, obj->recs.size());
  return spans;
}

int wfm_trans_closure(wfm_handle_t* h, wfm_trans_t* obj, const wfm_lift_iv_t* seeds, size_t n_seeds, uint32_t depth, wfm_trans_iv_t** ivs, size_t* n_ivs,
                      wfm_trans_seed_t* per_seed) {
  if (!h || !obj || !ivs || !n_ivs || (n_seeds && !seeds)) return WFM_E_ARG;
  *ivs = nullptr; *n_ivs = 0;
  if (int rc = trans_usable(h, obj)) return rc;
  if (n_seeds >= ((size_t)1 << 24)) { h->err = "wfm_trans_closure: " + std::to_string(n_seeds) + " seeds in one call: fewer than 2^24 (a key is seed << 40 | position)"; return WFM_E_ARG; }
  for (size_t i = 0; i < n_seeds; ++i)
    if (!(seeds[i].start < seeds[i].end && seeds[i].end <= obj->n_bases)) {
      h->err = "wfm_trans_closure: seed " + std::to_string(i) + " is empty or ends beyond the " + std::to_string(obj->n_bases) + " bases of the world";
      return WFM_E_ARG;
    }
  obj->last_rounds = obj->last_ivs = obj->last_pairs = 0;
  if (n_seeds == 0) return WFM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  PassTimer tm(h);
  if (int rc = trans_index(h, obj)) return rc;
  const double ms_index = tm.lap();
  // R_0: one interval per seed, in key order as they are
  size_t m = n_seeds, m_snap = 0, m_prev = 0;
  {
    std::vector<unsigned long long> keys(2 * m);
    for (size_t i = 0; i < m; ++i) { keys[i] = ((uint64_t)i << TRANS_SHIFT) | seeds[i].start; keys[m + i] = ((uint64_t)i << TRANS_SHIFT) | seeds[i].end; }
    if (obj->acc.ensure(2 * m)) { h->err = "out of device memory (transitive list)"; return WFM_E_NOMEM; }
    HIPCHK(h, hipMemcpyAsync(obj->acc.p, keys.data(), 2 * m * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  const unsigned end_bit = std::min(64u, TRANS_SHIFT + std::max(1u, bits_of(n_seeds)));
  const unsigned long long cap = cap_units("WFM_TRANS_OUT_MB", 16, 1);
  unsigned long long bases = 0, pairs = 0;
  if (int rc = trans_bases(h, obj, m, &bases)) return rc;
  uint64_t rounds = 0;
  size_t chunks = 0;
  std::vector<unsigned long long> off;
  while (obj->na && (depth == 0 || rounds < depth)) {
    // the list this round projects, and the one of the round before
    std::swap(obj->prev, obj->snap);
    m_prev = m_snap;
    if (obj->snap.ensure(2 * m)) { h->err = "out of device memory (transitive list)"; return WFM_E_NOMEM; }
    HIPCHK(h, hipMemcpyAsync(obj->snap.p, obj->acc.p, 2 * m * 8, hipMemcpyDeviceToDevice, h->stream));
    m_snap = m;
    const unsigned long long *ks = obj->snap.p, *ke = obj->snap.p + m_snap;
    ulonglong2* d_win;
    unsigned long long *d_cnt, *d_off;
    Carver cv{h->scratch, "transitive round"};
    cv.piece(&d_win, m_snap); cv.piece(&d_cnt, m_snap); cv.piece(&d_off, m_snap + 1);
    if (int rc = cv.commit(h)) return rc;
    launch_trans_count(ks, ke, m_snap, obj->prev.p, obj->prev.p + m_prev, m_prev, obj->sorted(), obj->pm(), obj->na, d_win, d_cnt, d_off, h->stream);
    HIPCHK(h, hipGetLastError());
    off.resize(m_snap + 1);
    HIPCHK(h, hipMemcpyAsync(off.data(), d_off, (m_snap + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ++rounds;
    pairs += off[m_snap];
    // chunks of whole intervals that hold at most WFM_TRANS_OUT_MB MiB of pairs; a single interval may exceed that alone
    for (size_t ka = 0, kb; ka < m_snap; ka = kb) {
      kb = chunk_end(ka, off, cap);
      const size_t c = (size_t)(off[kb] - off[ka]);
      if (c == 0) continue;
      const int rc = trans_union(h, obj, &m, c, end_bit, [&](unsigned long long* oks, unsigned long long* oke) {
        launch_trans_write(ks, ke, d_win, d_off, ka, kb, obj->sorted(), obj->pre, oks, oke, h->stream);
      });
      if (rc != WFM_OK) return rc;
      ++chunks;
    }
    unsigned long long now = 0;
    if (int rc = trans_bases(h, obj, m, &now)) return rc;
    const bool fixed = now == bases;  // (R_k is inside R_k+1: the same bases, the same set)
    bases = now;
    if (fixed) break;
  }
  // the list, sorted by (seed, start) as the keys are
  std::vector<unsigned long long> keys(2 * m);
  const bool pinned = pin_pieces(h);
  hipError_t e = copy_down(h, pinned, (char*)keys.data(), (const uint8_t*)obj->acc.p, 2 * m * 8);
  if (e != hipSuccess) { h->err = std::string("wfm_trans_closure: ") + hipGetErrorString(e); return WFM_E_HIP; }
  wfm_trans_iv_t* out = (wfm_trans_iv_t*)malloc(m * sizeof(wfm_trans_iv_t));
  if (!out) { h->err = "out of host memory (transitive intervals)"; return WFM_E_NOMEM; }
  const uint64_t mask = ((uint64_t)1 << TRANS_SHIFT) - 1;
  if (per_seed) memset(per_seed, 0, n_seeds * sizeof(wfm_trans_seed_t));
  for (size_t i = 0; i < m; ++i) {
    const uint32_t s = (uint32_t)(keys[i] >> TRANS_SHIFT);
    out[i] = wfm_trans_iv_t{keys[i] & mask, keys[m + i] & mask, s, 0u};
    if (per_seed) {
      if (per_seed[s].count++ == 0) per_seed[s].first = i;
      per_seed[s].bases += out[i].end - out[i].start;
    }
  }
  *ivs = out; *n_ivs = m;
  obj->last_rounds = rounds; obj->last_ivs = m; obj->last_pairs = pairs;
  if (tm.on)
    fprintf(stderr, "[wfm] transitive closure: %zu seeds over %zu arcs, depth %u: %llu rounds, %llu pairs in %zu chunks, %zu intervals over %llu bases; index %.3f ms, rounds and copy down %.3f ms (host clock)\n",
            n_seeds, obj->na, depth, (unsigned long long)rounds, pairs, chunks, m, bases, ms_index, tm.lap());
  return WFM_OK;
}

int wfm_trans_export(wfm_handle_t* h, wfm_trans_t* obj, wfm_trans_rec_t** recs, size_t* n_recs, wfm_trans_word_t** words, size_t* n_words) {
  if (!h || !obj || !recs || !n_recs || !words || !n_words) return WFM_E_ARG;
  *recs = nullptr; *n_recs = 0; *words = nullptr; *n_words = 0;
  if (int rc = trans_usable(h, obj)) return rc;
  if (obj->recs.empty()) return WFM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  wfm_trans_rec_t* r = (wfm_trans_rec_t*)malloc(obj->recs.size() * sizeof(wfm_trans_rec_t));
  wfm_trans_word_t* w = (wfm_trans_word_t*)malloc(obj->np * sizeof(wfm_trans_word_t));
  hipError_t e = hipSuccess;
  if (r && w) e = copy_down(h, pin_pieces(h), (char*)w, (const uint8_t*)obj->pre, obj->np * sizeof(wfm_trans_word_t));
  if (!r || !w || e != hipSuccess) {
    free(r); free(w);
    if (e != hipSuccess) { h->err = std::string("wfm_trans_export: ") + hipGetErrorString(e); return WFM_E_HIP; }
    h->err = "out of host memory (transitive list)";
    return WFM_E_NOMEM;
  }
  memcpy(r, obj->recs.data(), obj->recs.size() * sizeof(wfm_trans_rec_t));
  *recs = r; *n_recs = obj->recs.size();
  *words = w; *n_words = obj->np;
  return WFM_OK;
}

int wfm_trans_import(wfm_handle_t* h, wfm_trans_t* obj, const wfm_trans_rec_t* recs, size_t n_recs, const wfm_trans_word_t* words, size_t n_words) {
  if (!h || !obj || (n_recs && !recs) || (n_words && !words)) return WFM_E_ARG;
  if (n_recs == 0) return WFM_OK;
  if (int rc = trans_usable(h, obj)) return rc;
  // everything is looked at before anything is added
  auto refuse = [&](size_t i, const char* why) {
    h->err = "wfm_trans_import: record " + std::to_string(i) + " " + why + "; nothing was added";
    return (int)WFM_E_ARG;
  };
  std::vector<TransArc> arcs(2 * n_recs);
  std::vector<wfm_trans_rec_t> mine(recs, recs + n_recs);
  for (size_t i = 0; i < n_recs; ++i) {
    const wfm_trans_rec_t& r = recs[i];
    if (r.flags & ~WFM_TRANS_REVERSE) return refuse(i, "holds a flag bit that is not WFM_TRANS_REVERSE");
    if (r.n_runs == 0 || r.pre_off > n_words || (uint64_t)r.n_runs + 1 > n_words - r.pre_off) return refuse(i, "has no runs, or its prefix words leave the list");
    const wfm_trans_word_t* w = words + r.pre_off;
    if (w[0].p | w[0].t | w[0].eq | w[0].x) return refuse(i, "does not begin at zero");
    for (uint32_t k = 0; k < r.n_runs; ++k) {
      const wfm_trans_word_t &a = w[k], &b = w[k + 1];
      if (b.p < a.p || b.t < a.t || b.eq < a.eq || b.x < a.x) return refuse(i, "has a prefix that falls");
      const uint32_t dp = b.p - a.p, dt = b.t - a.t, de = b.eq - a.eq, dx = b.x - a.x, len = std::max(dp, dt);
      const bool run = len && (dp == 0 || dp == len) && (dt == 0 || dt == len) && ((dp == len && dt == len) ? (de + dx == len && (de == 0 || dx == 0)) : (de == 0 && dx == 0));
      if (!run) return refuse(i, "has a step between two prefix words that is no run of =, X, I or D");
    }
    const uint32_t P = w[r.n_runs].p, T = w[r.n_runs].t;
    if (r.t > obj->n_bases || P > obj->n_bases - r.t || r.q > obj->n_bases || T > obj->n_bases - r.q) return refuse(i, "leaves the world");
    mine[i].pre_off = obj->np + r.pre_off;
    trans_arcs_of(mine[i], mine[i].pre_off, P, T, &arcs[2 * i]);
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = trans_reserve(h, obj, "wfm_trans_import", n_words, n_recs)) return rc;
  HIPCHK(h, hipMemcpyAsync(obj->pre + obj->np, words, n_words * sizeof(wfm_trans_word_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(obj->arcs + obj->na, arcs.data(), arcs.size() * sizeof(TransArc), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  obj->np += n_words;
  obj->na += arcs.size();
  obj->recs.insert(obj->recs.end(), mine.begin(), mine.end());
  obj->indexed = false;
  return WFM_OK;
}

int wfm_trans_counts(const wfm_trans_t* obj, uint64_t out[6]) {
  if (!obj || !out) return WFM_E_ARG;
  out[0] = obj->recs.size(); out[1] = obj->np; out[2] = obj->na; out[3] = obj->last_rounds; out[4] = obj->last_ivs; out[5] = obj->last_pairs;
  return WFM_OK;
}

void wfm_trans_free_list(void* p) { free(p); }

// ---- every score proved optimal by a banded DP (wfmash_hip.h; the band: wfa_optband.h; the kernel: wfa_optcheck.hip) ----
int wfm_check_optimal(wfm_handle_t* h, const wfm_penalties_t* pen, const wfm_seqset_t* s, const wfm_result_t* res, uint64_t max_cells,
                      wfm_optcheck_t* out) {
  if (!h || !s || !out || !res || !pen) return WFM_E_ARG;
  const int pmax = 32767;
  if (pen->x <= 0 || pen->e1 <= 0 || pen->e2 <= 0 || pen->o1 < 0 || pen->o2 < 0 || pen->x > pmax || pen->o1 > pmax || pen->e1 > pmax ||
      pen->o2 > pmax || pen->e2 > pmax) { h->err = "wfm_check_optimal: unsupported penalties"; return WFM_E_UNSUPPORTED; }
  const size_t n = s->meta.size();
  if (n == 0) return 0;
  if (n > (size_t)INT32_MAX) { h->err = "wfm_check_optimal: too many problems for one call"; return WFM_E_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  const OptPen op{pen->x, pen->o1, pen->e1, pen->o2, pen->e2};
  // the plan: every checked problem's band, the form it runs in, and per form the problems largest first
  struct Item { uint64_t cells; uint32_t prob; };
  std::vector<Item> forms[4];
  std::vector<OptProb> probs(n);
  for (size_t i = 0; i < n; ++i) {
    const ProbMeta& m = s->meta[i];
    wfm_optcheck_t& o = out[i];
    o.flags = 0; o.dp_score = -1; o.band_lo = 0; o.band_hi = -1; o.cells = 0;
    if (res[i].status != 0 || res[i].score < 0 || res[i].score >= (1 << 29)) { o.flags = WFM_OPT_NOT_CHECKED; continue; }
    const OptBand b = opt_band(op, m.plen, m.tlen, m.pbf, m.pef, m.tbf, m.tef, res[i].score);  // (0 unless the mode is ENDSFREE: layout_seqset)
    o.band_lo = (int32_t)b.lo; o.band_hi = (int32_t)b.hi;
    if (max_cells && b.cells > max_cells) { o.flags = WFM_OPT_SKIPPED; continue; }
    o.cells = b.cells;
    OptProb& c = probs[i];
    fill_seq(c, m);
    c.row_off = 0;
    c.pbf = std::min(std::max(m.pbf, 0), m.plen); c.pef = std::min(std::max(m.pef, 0), m.plen);
    c.tbf = std::min(std::max(m.tbf, 0), m.tlen); c.tef = std::min(std::max(m.tef, 0), m.tlen);
    c.band_lo = o.band_lo; c.band_hi = o.band_hi;
    const int64_t W = b.hi - b.lo + 1;
    forms[W <= WFM_OPT_BAND_C1 ? 0 : W <= WFM_OPT_BAND_C4 ? 1 : W <= WFM_OPT_REG_MAX ? 2 : 3].push_back(Item{b.cells, (uint32_t)i});
  }
  PassTimer tm(h);
  uint64_t cells_total = 0;
  size_t launches = 0;
  std::vector<OptProb> chunk;
  std::vector<int32_t> dp;
  const size_t rows_cap = ((size_t)WFM_OPT_ROWS_MB << 20) / sizeof(int32_t);
  for (int form = 0; form < 4; ++form) {
    std::vector<Item>& v = forms[form];
    std::stable_sort(v.begin(), v.end(), [](const Item& a, const Item& b) { return a.cells > b.cells; });
    for (size_t i0 = 0; i0 < v.size();) {
      // a chunk: all of a register form at once; of the memory form as many as the row budget holds (one at least)
      chunk.clear();
      size_t row_elems = 0, i1 = i0;
      for (; i1 < v.size(); ++i1) {
        OptProb c = probs[v[i1].prob];
        if (form == 3) {
          const size_t W = (size_t)((int64_t)c.band_hi - c.band_lo + 1);
          const size_t need = 3 * ((W + WFM_OPT_REG_MAX - 1) / WFM_OPT_REG_MAX * WFM_OPT_REG_MAX + 1);
          if (!chunk.empty() && row_elems + need > rows_cap) break;
          c.row_off = (int64_t)row_elems;
          row_elems += need;
        }
        chunk.push_back(c);
      }
      const size_t m = chunk.size();
      OptProb* d_probs;
      int32_t* d_out;
      Carver cv{h->scratch, "optimality check"};
      cv.piece(&d_probs, m); cv.piece(&d_out, m);
      if (int rc = cv.commit(h)) return rc;
      if (row_elems && h->optrows.ensure(row_elems)) { h->err = "out of device memory (optimality check: rows of a wide band)"; return WFM_E_NOMEM; }
      HIPCHK(h, hipMemcpyAsync(d_probs, chunk.data(), m * sizeof(OptProb), hipMemcpyHostToDevice, h->stream));
      launch_optcheck(s->d_seq, d_probs, (int)m, form, h->optrows.p, d_out, DevPen{pen->x, pen->o1, pen->e1, pen->o2, pen->e2}, h->stream);
      HIPCHK(h, hipGetLastError());
      dp.resize(m);
      HIPCHK(h, hipMemcpyAsync(dp.data(), d_out, m * 4, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));  // (the chunk's host vectors and the row block are free for the next one)
      for (size_t q = 0; q < m; ++q) out[v[i0 + q].prob].dp_score = dp[q];
      ++launches;
      i0 = i1;
    }
  }
  int flagged = 0;
  for (size_t i = 0; i < n; ++i) {
    wfm_optcheck_t& o = out[i];
    if (o.flags) continue;
    cells_total += o.cells;
    if (o.dp_score < 0 || o.dp_score > res[i].score) o.flags = WFM_OPT_UNREACHED;
    else if (o.dp_score < res[i].score) o.flags = WFM_OPT_CHEAPER;
    flagged += o.flags != 0;
  }
  if (tm.on)
    fprintf(stderr, "[wfm] optimality check: %zu problems (%zu / %zu / %zu in registers, %zu from memory), %zu launches, %llu cells in %.3f ms\n", n,
            forms[0].size(), forms[1].size(), forms[2].size(), forms[3].size(), launches, (unsigned long long)cells_total, tm.host_ms());
  return flagged;
}

}  // extern "C"
