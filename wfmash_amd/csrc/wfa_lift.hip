// wfa_lift.hip -- the kernels behind wfm_liftset_* and wfm_lift_runs (include/wfmash_hip.h): where intervals of the target lie in the query,
// through the runs of many records.  The pattern is the target, the text the query as aligned.  Nothing but runs is read: no sequence bytes.
//
//   launch_runmax            (wfa_scan.h) the running maximum of `end` over the sorted intervals, pm[i] = max(end[0 .. i]), per block of
//                            WFM_LIFT_SCAN_BLOCK intervals.
//   lift_index_kernel        one workgroup per problem.  wfa_scan.h's run_span takes the pattern and text spans (the problem is refused
//                            when the pattern span leaves [0, n_bases], a span does not fit 32 bits or a run is empty) BEFORE anything is
//                            written; the second pass goes in rounds of 256 runs with a carry and stores per run the four exclusive prefixes
//                            {pattern, text, = columns, X columns} as ONE 16-byte word, and the four totals behind the last run.  Then the
//                            candidate window [lo, hi) of the problem's span [a, b): lo = the first i with pm[i] > a, hi = the first i with
//                            start[i] >= b, two binary searches, and the count of the intervals in it with end > a.
//   scan_sums_kernel         (wfa_scan.h) ONE workgroup: the counts to their exclusive prefixes over the problems.
//   lift_write_kernel        one workgroup per problem of a chunk: the same enumeration in rounds of 256 intervals, every overlapping interval
//                            placed by a block scan (no atomics: two calls give the same bytes), ONE lane per pair resolving its endpoints in
//                            four binary searches over the prefix words (lift_resolve), 32 bytes a lift in two 16-byte stores.
// Offsets inside a problem are 32-bit, global positions 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wfmash_hip.h"
#include "wfa_device.h"
#include "wfa_scan.h"

namespace wfm {
namespace {

constexpr int LIFT_THREADS = 256;
constexpr int LIFT_WAVES = LIFT_THREADS / 64;
static_assert(WFM_LIFT_SCAN_BLOCK == LIFT_THREADS * 4, "a scan block is four intervals per lane");

__global__ __launch_bounds__(LIFT_THREADS) void lift_index_kernel(const uint32_t* __restrict__ runs, const LiftProb* __restrict__ probs,
                                                                  const ulonglong2* __restrict__ iv, const unsigned long long* __restrict__ pm,
                                                                  unsigned long long n_iv, unsigned long long n_bases, uint4* __restrict__ pre,
                                                                  LiftWin* __restrict__ win) {
  const LiftProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x;
  __shared__ unsigned long long wtot[LIFT_WAVES];
  __shared__ uint32_t s_bad;
  __shared__ unsigned long long s_lo, s_hi;
  const uint32_t* my = runs + pr.runs_off;
  const uint32_t n = pr.n_runs;
  // the spans first: nothing is written for a problem that is refused
  unsigned long long span, tspan;
  const bool empty_run = run_span<LIFT_WAVES, true>(my, n, wtot, &s_bad, &span, &tspan);
  const bool spans = empty_run || n == 0 || pr.base > n_bases || span > n_bases - pr.base || span > 0xffffffffull || tspan > 0xffffffffull;
  if (spans) {
    if (tid == 0) { LiftWin w; w.lo = 0; w.hi = 0; w.count = 0; w.flags = WFM_LIFT_SPANS; w.plen = 0; win[blockIdx.x] = w; }
    return;
  }
  uint4* mypre = pre + pr.pre_off;
  unsigned long long cp = 0, ct = 0, ce = 0, cx = 0;
  for (uint32_t base = 0; base < n; base += LIFT_THREADS) {
    const uint32_t r = base + (uint32_t)tid;
    const bool valid = r < n;
    const uint32_t run = valid ? my[r] : 0u;
    const uint32_t len = WFM_RUN_LEN(run), op = WFM_RUN_OP(run);
    unsigned long long tp, tt, te, tx;
    const unsigned long long pp = cp + block_excl<LIFT_WAVES>((valid && op != OP_I) ? len : 0u, wtot, &tp);
    const unsigned long long pt = ct + block_excl<LIFT_WAVES>((valid && op != OP_D) ? len : 0u, wtot, &tt);
    const unsigned long long pe = ce + block_excl<LIFT_WAVES>((valid && op == OP_M) ? len : 0u, wtot, &te);
    const unsigned long long px = cx + block_excl<LIFT_WAVES>((valid && op == OP_X) ? len : 0u, wtot, &tx);
    cp += tp; ct += tt; ce += te; cx += tx;
    if (valid) mypre[r] = make_uint4((uint32_t)pp, (uint32_t)pt, (uint32_t)pe, (uint32_t)px);
  }
  if (tid == 0) mypre[n] = make_uint4((uint32_t)cp, (uint32_t)ct, (uint32_t)ce, (uint32_t)cx);
  // the candidate window and the number of intervals in it that reach beyond a
  const unsigned long long a = pr.base, b = pr.base + span;
  if (tid == 0) {
    s_lo = span ? first_true(n_iv, [&](unsigned long long i) { return pm[i] > a; }) : 0ull;
    s_hi = span ? first_true(n_iv, [&](unsigned long long i) { return iv[i].x >= b; }) : 0ull;
  }
  __syncthreads();
  const unsigned long long lo = s_lo, hi = s_hi > s_lo ? s_hi : s_lo;
  unsigned long long c = 0;
  for (unsigned long long i = lo + (unsigned long long)tid; i < hi; i += LIFT_THREADS) c += iv[i].y > a;
  unsigned long long all;
  (void)block_excl<LIFT_WAVES>(c, wtot, &all);
  if (tid == 0) { LiftWin w; w.lo = lo; w.hi = hi; w.count = all; w.flags = 0; w.plen = (uint32_t)span; win[blockIdx.x] = w; }
}

// One pair.  P: the problem's n + 1 prefix words {pattern, text, = columns, X columns} (the totals last); [c0, c1), c0 < c1 <= the pattern
// span: the interval clipped to it.  Four binary searches, no walk: a pattern offset finds its run by the LAST prefix at or before it (an I
// run shares its prefix with the run behind it, so the last match is the non-I run; a final I run's prefix is the span itself, beyond every
// offset asked for), which gives the ordinal of the nearest aligned column inward; the ordinal finds its run the same way among the
// aligned-column prefixes (a gap run shares its ordinal with the run behind it; final gap runs hold the total, beyond every ordinal asked for).
__device__ __forceinline__ void lift_resolve(const uint4* __restrict__ P, const uint32_t* __restrict__ my, uint32_t n, uint32_t c0, uint32_t c1, uint32_t* o) {
  const uint32_t r0 = last_le(0u, n, [&](uint32_t r) { return P[r].x <= c0; });
  const uint32_t r1 = last_le(0u, n, [&](uint32_t r) { return P[r].x <= c1 - 1u; });
  const uint4 w0 = P[r0], w1 = P[r1];
  const uint32_t ord0 = w0.z + w0.w + (WFM_RUN_OP(my[r0]) <= OP_X ? c0 - w0.x : 0u);  // the first aligned column at or behind c0
  const uint32_t ord1 = w1.z + w1.w + (WFM_RUN_OP(my[r1]) <= OP_X ? c1 - w1.x : 0u);  // one past the last aligned column before c1
  if (ord0 >= ord1) {  // nothing aligned in [c0, c1): r0 is a D run, the text stands where that run found it
    o[0] = c0; o[1] = c0; o[2] = w0.y; o[3] = w0.y; o[4] = 0u; o[5] = 0u;
    return;
  }
  const uint32_t ra = last_le(0u, n, [&](uint32_t r) { return P[r].z + P[r].w <= ord0; });
  const uint32_t rb = last_le(0u, n, [&](uint32_t r) { return P[r].z + P[r].w <= ord1 - 1u; });
  const uint4 wa = P[ra], wb = P[rb];
  const uint32_t ka = ord0 - (wa.z + wa.w), kb = ord1 - (wb.z + wb.w);  // columns of the run before the first lifted one / up to the last
  const bool xa = WFM_RUN_OP(my[ra]) == OP_X, xb = WFM_RUN_OP(my[rb]) == OP_X;
  o[0] = wa.x + ka; o[1] = wb.x + kb;
  o[2] = wa.y + ka; o[3] = wb.y + kb;
  o[4] = (wb.z + (xb ? 0u : kb)) - (wa.z + (xa ? 0u : ka));
  o[5] = (wb.w + (xb ? kb : 0u)) - (wa.w + (xa ? ka : 0u));
}

// the problems from ka on, one per workgroup; out[0] is lift number off[ka] of the whole call
__global__ __launch_bounds__(LIFT_THREADS) void lift_write_kernel(const uint32_t* __restrict__ runs, const LiftProb* __restrict__ probs,
                                                                  const ulonglong2* __restrict__ iv, const uint4* __restrict__ pre,
                                                                  const LiftWin* __restrict__ win, const unsigned long long* __restrict__ off,
                                                                  uint32_t ka, uint4* __restrict__ out) {
  __shared__ unsigned long long wtot[LIFT_WAVES];
  const uint32_t k = ka + blockIdx.x;
  const LiftWin w = win[k];
  if (w.count == 0) return;  // (the whole workgroup)
  const LiftProb pr = probs[k];
  const uint4* P = pre + pr.pre_off;
  const uint32_t* my = runs + pr.runs_off;
  const unsigned long long a = pr.base, b = pr.base + w.plen;
  unsigned long long at = off[k] - off[ka];
  for (unsigned long long base = w.lo; base < w.hi; base += LIFT_THREADS) {
    const unsigned long long i = base + threadIdx.x;
    ulonglong2 v = make_ulonglong2(0ull, 0ull);
    if (i < w.hi) v = iv[i];
    const bool take = i < w.hi && v.y > a;
    unsigned long long all;
    const unsigned long long slot = at + block_excl<LIFT_WAVES>(take ? 1u : 0u, wtot, &all);
    at += all;
    if (!take) continue;
    const uint32_t c0 = (uint32_t)((v.x > a ? v.x : a) - a), c1 = (uint32_t)((v.y < b ? v.y : b) - a);
    uint32_t o[6];
    lift_resolve(P, my, pr.n_runs, c0, c1, o);
    out[2 * slot] = make_uint4(k, (uint32_t)i, o[0], o[1]);
    out[2 * slot + 1] = make_uint4(o[2], o[3], o[4], o[5]);
  }
}

}  // namespace

void launch_lift_pm(const void* iv, unsigned long long n, unsigned long long* maxs, unsigned long long* pm, hipStream_t st) {
  if (n == 0) return;
  launch_runmax<LIFT_WAVES>(LoadEnd{(const ulonglong2*)iv}, n, maxs, pm, st);  // pm[i] = max(end[0 .. i])
}

void launch_lift_index(const uint32_t* runs, const LiftProb* probs, int nprob, const void* iv, const unsigned long long* pm, unsigned long long n_iv,
                       unsigned long long n_bases, void* pre, LiftWin* win, unsigned long long* off, hipStream_t st) {
  if (nprob <= 0) return;
  hipLaunchKernelGGL(lift_index_kernel, dim3((unsigned)nprob), dim3(LIFT_THREADS), 0, st, runs, probs, (const ulonglong2*)iv, pm, n_iv, n_bases, (uint4*)pre, win);
  // off[i] = the lifts of the problems before i, off[nprob] = all of them
  hipLaunchKernelGGL((scan_sums_kernel<LIFT_WAVES, false, LoadWinCount>), dim3(1), dim3(LIFT_THREADS), 0, st, LoadWinCount{win}, (unsigned long long)nprob, off,
                     (unsigned long long*)nullptr);
}

void launch_lift_write(const uint32_t* runs, const LiftProb* probs, const void* iv, const void* pre, const LiftWin* win, const unsigned long long* off,
                       uint32_t ka, uint32_t kb, void* out, hipStream_t st) {
  if (kb <= ka) return;
  hipLaunchKernelGGL(lift_write_kernel, dim3(kb - ka), dim3(LIFT_THREADS), 0, st, runs, probs, (const ulonglong2*)iv, (const uint4*)pre, win, off, ka, (uint4*)out);
}

}  // namespace wfm
