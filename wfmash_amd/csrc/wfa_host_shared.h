// wfa_host_shared.h -- what the translation units behind the C ABI share (wfa_host.hip: the align driver, the handles and the sequence
// uploads; wfa_passes.hip: the record passes).  Internal: nothing under include/ names it.
#ifndef WFM_WFA_HOST_SHARED_H_
#define WFM_WFA_HOST_SHARED_H_
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/wfmash_hip.h"
#include "wfa_device.h"
#include "dev_cache.h"

#define HIPCHK(h, call)                                                                 \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) {                                                             \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                     \
      return WFM_E_HIP;                                                                 \
    }                                                                                   \
  } while (0)

namespace wfm {

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  // The blocks come from, and go back to, the per-device block cache (dev_cache.h), never straight to the driver: memory a
  // process has freed is wiped before it is handed out again, and an allocation that lands on it waits for that -- 40 ms per GB
  // as a rule, 1.3 - 1.8 s at worst (profiles/r4_map_host.md).  An arena that is outgrown waits in the cache (its size class
  // serves the next handle, or the next batch's sequences); at most as much again as the final arena is held that way.
  int ensure(size_t n) {
    if (n <= cap) return 0;
    const size_t old_cap = cap;
    if (p) wfm_dfree(p);  // (waits for the device, as hipFree did)
    p = nullptr; cap = 0;
    // (an arena that has to grow doubles at least: every regrowth is a fresh allocation, 30 - 70 ms per GB on this driver, and a
    // divergent batch -- C1 -- used to walk its ring arena up in five steps of 3.5 .. 12 GB)
    // ... but never by more than 8 GB beyond what is asked for: the arenas live under per-handle budgets of up to 32 GB, and a ring arena near
    // its budget that doubled held 64 GB + the outgrown 32 in the cache, outside every budget's accounting)
    size_t want = std::max(n + n / 8 + 64, std::min(old_cap * 2, n + ((size_t)8 << 30) / sizeof(T)));
    const auto t0 = std::chrono::steady_clock::now();
    if (wfm_dmalloc((void**)&p, want * sizeof(T)) != hipSuccess) {  // (the cache has given everything back and tried again by then)
      (void)hipGetLastError();  // the failure must not surface after a later launch
      if (wfm_dmalloc((void**)&p, n * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return -1; }
      want = n;
    }
    cap = want;
    if (want * sizeof(T) >= ((size_t)256 << 20) && getenv("WFM_DEBUG"))
      fprintf(stderr, "[wfm] device block of %.2f GB took %.1f ms\n", (double)(want * sizeof(T)) / 1073741824.0,
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return 0;
  }
  void release() { if (p) wfm_dfree(p); p = nullptr; cap = 0; }
};

struct ProbMeta {
  int64_t p_fwd, t_fwd, p_rev, t_rev;  // offsets into device sequence buffer
  int32_t plen, tlen;
  int32_t mode, pbf, pef, tbf, tef;
  int32_t hint;     // the caller's guess of an upper bound of the score (0: none)
  int64_t rle_off;  // start of this problem's RLE slot range (a score-only problem has none: its range is empty)
  int32_t flags;    // WFM_MODE_SCORE_ONLY / WFM_MODE_SCORE_LIMIT as the problem came with them (mode holds the bits under WFM_MODE_MASK)
  int32_t limit;    // WFM_MODE_SCORE_LIMIT: the hard limit of the score (0: none); hint is 0 then
  bool score_only() const { return (flags & WFM_MODE_SCORE_ONLY) != 0; }
};

// a switch of the environment as a number (unset: dflt); WFM_DEBUG's level (0: unset).  Read once per call, into Knobs / TileCfg / BaseCfg
inline int env_num(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
inline int env_debug() { return getenv("WFM_DEBUG") ? std::max(1, env_num("WFM_DEBUG", 0)) : 0; }

inline int validate_pen(const wfm_penalties_t* pen, int* scope) {
  if (!pen) return WFM_E_ARG;
  if (pen->x <= 0 || pen->e1 <= 0 || pen->e2 <= 0 || pen->o1 < 0 || pen->o2 < 0) return WFM_E_UNSUPPORTED;
  const int sc = std::max(pen->x, std::max(pen->o1 + pen->e1, pen->o2 + pen->e2)) + 1;
  // (two rows of a ring are always in the making: the step kernel clears the row-maximum slot of row s + 2 while rows back to
  // s - scope + 1 are still read, so a ring of R rows serves scopes up to R - 2)
  if (sc > RING_BIG - 2) return WFM_E_UNSUPPORTED;  // o2 + e2 (or o1 + e1, or x) beyond 125: deeper rings than the kernels are built with
  *scope = sc;
  return WFM_OK;
}

}  // namespace wfm

struct wfm_seqset {
  uint8_t* d_seq = nullptr;
  uint32_t* d_pk = nullptr;          // 2-bit mirror of d_seq (wfa_tile2.hip), PK_PAD_WORDS behind it
  std::vector<int32_t> acgt;         // per problem: nonzero = both sequences are pure upper-case ACGT
  size_t bytes = 0;
  std::vector<wfm::ProbMeta> meta;
  int64_t rle_total = 0;
  uint64_t seq_bases = 0;
};

struct wfm_handle {
  int device = 0;
  std::vector<std::pair<double, double>> busy_abs;  // merged intervals during which a kernel of the last align call ran, ms after the device's origin
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
  std::vector<hipEvent_t> tile_ev;  // start/stop pairs for the tile blocks of one chunk
  std::vector<wfm_handle*> peers;   // further contexts for the other parts of a batch (created on first use)
  bool is_peer = false;             // a part's context: it shares its owner's budget and is not counted as a handle of the device
  hipEvent_t ev_base = nullptr;     // time origin of the call (shared by the two halves)
  hipEvent_t call_base = nullptr;   // the origin this call measures against
  std::vector<std::pair<float, float>> tile_iv;  // (start, end) of every tile kernel launch of the call, ms after call_base
  std::vector<std::pair<float, float>> bp_iv, base_iv;  // the same for the step kernel and the base kernel
  std::string err;
  std::string name;
  std::vector<uint32_t> prob_flags;  // WFM_PF_* of every problem of the last align call (wfm_get_problem_flags)
  int other_calls = 0;         // wfm_set_concurrent_calls: align calls the caller keeps in flight on this device beside this handle's
  size_t mem_budget = 0;       // arena budget in force for the call at hand
  size_t mem_budget_full = 0;  // the handle's whole budget (40 % of free HBM at creation, or WFM_MEM_BUDGET_MB)
  wfm_stats_t stats{};
  uint64_t tile_ctr[WFM_TILE_COUNTERS] = {};  // which paths the tile phase took in the last align call (wfm_get_tile_counters)
  wfm::DevBuf<int32_t> ring;      // breakpoint rings
  wfm::DevBuf<int32_t> base32;    // base: pre + rings
  wfm::DevBuf<uint8_t> base8;     // base: bt
  wfm::DevBuf<uint32_t> rle, rle_out;
  wfm::DevBuf<wfm::BpJob> bpjobs;
  wfm::DevBuf<wfm::TileJob> tilejobs;
  wfm::DevBuf<wfm::TileTask> tiletasks;
  wfm::DevBuf<int32_t> tilemak;
  wfm::DevBuf<int32_t> p2rows, p2max, p2bmax;  // phase 2 from rows computed ahead (P2Job)
  wfm::DevBuf<wfm::P2Job> p2jobs;
  wfm::DevBuf<wfm::RingWidenJob> widenjobs;
  wfm::DevBuf<wfm::KeepTask> keeptasks;        // parent reuse: the keeps behind a chunk of tile blocks, the restores at a look of the host and what they found
  wfm::DevBuf<wfm::RestoreTask> restoretasks;
  wfm::DevBuf<int32_t> restoreres;
  wfm::DevBuf<wfm::SeqRev> revjobs;
  wfm::DevBuf<wfm::BoundJob> bndjobs;   // roots whose score is bounded from above before their wavefronts run (wfa_bound_kernel)
  wfm::DevBuf<int32_t> bndres;
  uint8_t* stage = nullptr;  // pinned staging buffer of wfm_upload_sequences (grow-only)
  size_t stage_cap = 0;
  wfm::DevBuf<wfm::BpResult> bpres;
  wfm::DevBuf<wfm::BaseJob> bsjobs;
  wfm::DevBuf<wfm::BaseResult> bsres;
  wfm::DevBuf<wfm::Base2TJob> b2tjobs;     // base jobs on tiles (wfa_base2t_kernel)
  wfm::DevBuf<wfm::Base2TTask> b2ttasks;
  wfm::DevBuf<unsigned long long> b2tkeys;
  wfm::DevBuf<int32_t> b2toffs, b2tactive;
  wfm::DevBuf<int64_t> i64a, i64b, i64c;
  wfm::DevBuf<int32_t> i32a;
  wfm::DevBuf<int32_t> seqflags;  // wfm_upload_sequences: per problem, nonzero = pure ACGT
  wfm::DevBuf<wfm::SeqRev> flagjobs;
  wfm::DevBuf<wfm::SeqGatherTask> gathertasks;  // wfm_upload_sequence_refs
  uint8_t* cspin[2] = {nullptr, nullptr};  // the two pinned pieces a chunk's bytes reach the caller's buffer through (PIN_PIECE each)
  wfm::DevBuf<uint64_t> scratch;          // the record passes (wfa_passes.hip): everything a call has on the device, carved out of one block;
  wfm::DevBuf<uint64_t> outblk;           // the output block of one chunk (cs, variants).  A pass waits for the stream before it returns: one of each serves all
  wfm::DevBuf<int32_t> optrows;           // wfm_check_optimal: the rows of the bands too wide for registers
  wfm::DevBuf<unsigned long long> total;
  void* attachment = nullptr;  // owned by another translation unit (map_kernels.hip: the pinned staging ring)
  void (*attachment_free)(void*) = nullptr;
};
#endif
