// wfa_trans.hip -- the kernels behind wfm_trans_* (include/wfmash_hip.h): intervals of one coordinate space mapped through the runs of many
// records, in both directions, round after round.  Nothing but prefix words is read: no sequence bytes, and after wfm_trans_add no runs.
//
//   trans_span_kernel     one workgroup per problem.  wfa_scan.h's run_span takes the pattern and text spans; the problem is refused (an empty
//                         run, no runs, a span that does not fit 32 bits or leaves the world) and NOTHING is written but its flags and spans.
//   trans_pre_kernel      one workgroup per problem that was kept: rounds of 256 runs with four carries, per run the exclusive prefixes
//                         {pattern, text, = columns, X columns} as ONE 16-byte word in the object's block, the four totals behind the last run
//                         (lift_index_kernel's second pass).  The runs are not kept: a run's op follows from two neighbouring words.
//   trans_key_kernel      the arcs' source starts and 0, 1, 2 ... for rocprim::radix_sort_pairs (wfa_pav.hip's pav_sort);
//   trans_gather_kernel   the arcs in sorted order, 32 bytes each; launch_runmax (wfa_scan.h) gives pm[i] = max(source end[0 .. i]).
//   trans_count_kernel    one workgroup per interval [a, b) of the current list.  An interval that the list before had already is skipped (one
//                         binary search: its hulls are in the list).  Else lo = the first arc with pm > a, hi = the first arc with start >= b,
//                         and the number of arcs in [lo, hi) with end > a, in rounds of 256.
//   scan_sums_kernel      (wfa_scan.h) ONE workgroup: the counts to their exclusive prefixes over the intervals.
//   trans_write_kernel    one workgroup per interval of a chunk: the same enumeration, every pair placed by a block scan (no atomics: two
//                         calls give the same bytes), ONE lane per (interval, arc) pair resolving the hull in four binary searches over the
//                         record's prefix words (trans_resolve): O(log n_runs) a pair, never a walk.  It writes seed << 40 | lo and
//                         seed << 40 | hi; a pair whose hull is empty writes the interval itself, which the list holds already, so it adds nothing.
// The union of the list with a chunk's pairs is wfa_pav.hip's: pav_sort, launch_pav_runmax, launch_pav_compact, launch_pav_prefix, on the
// keys seed << 40 | position as they are on group << 40 | position.  No workgroup ever waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wfmash_hip.h"
#include "wfa_device.h"
#include "wfa_scan.h"

namespace wfm {
namespace {

constexpr int TRANS_THREADS = 256;
constexpr int TRANS_WAVES = TRANS_THREADS / 64;
constexpr unsigned long long TRANS_POS = ((unsigned long long)1 << 40) - 1;
static_assert(WFM_TRANS_SCAN_BLOCK == TRANS_THREADS * 4, "a scan block is four arcs per lane");
static_assert(sizeof(TransArc) == 32 && sizeof(TransProb) == 32 && sizeof(TransSpan) == 16, "wfa_device.h states these sizes");

struct LoadArcEnd {
  const TransArc* p;
  __device__ __forceinline__ unsigned long long operator()(unsigned long long i) const { return p[i].s + p[i].slen; }
};

__global__ __launch_bounds__(TRANS_THREADS) void trans_span_kernel(const uint32_t* __restrict__ runs, const TransProb* __restrict__ probs,
                                                                   unsigned long long n_bases, TransSpan* __restrict__ out) {
  const TransProb pr = probs[blockIdx.x];
  __shared__ unsigned long long wtot[TRANS_WAVES];
  __shared__ uint32_t s_bad;
  unsigned long long span, tspan;
  const bool empty_run = run_span<TRANS_WAVES, true>(runs + pr.runs_off, pr.n_runs, wtot, &s_bad, &span, &tspan);
  const bool spans = empty_run || pr.n_runs == 0 || span > 0xffffffffull || tspan > 0xffffffffull || pr.t > n_bases || span > n_bases - pr.t ||
                     pr.q > n_bases || tspan > n_bases - pr.q;
  if (threadIdx.x == 0) {
    TransSpan s;
    s.flags = spans ? WFM_TRANS_SPANS : 0u; s.pspan = spans ? 0u : (uint32_t)span; s.tspan = spans ? 0u : (uint32_t)tspan; s.pad_ = 0;
    out[blockIdx.x] = s;
  }
}

// pre_off[k]: where problem k's n_runs + 1 words begin in pre, or ~0 for a problem that was refused
__global__ __launch_bounds__(TRANS_THREADS) void trans_pre_kernel(const uint32_t* __restrict__ runs, const TransProb* __restrict__ probs,
                                                                  const unsigned long long* __restrict__ pre_off, uint4* __restrict__ pre) {
  const unsigned long long at = pre_off[blockIdx.x];
  if (at == ~0ull) return;  // (the whole workgroup)
  const TransProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x;
  __shared__ unsigned long long wtot[TRANS_WAVES];
  const uint32_t* my = runs + pr.runs_off;
  const uint32_t n = pr.n_runs;
  uint4* mypre = pre + at;
  unsigned long long cp = 0, ct = 0, ce = 0, cx = 0;
  for (uint32_t base = 0; base < n; base += TRANS_THREADS) {
    const uint32_t r = base + (uint32_t)tid;
    const bool valid = r < n;
    const uint32_t run = valid ? my[r] : 0u;
    const uint32_t len = WFM_RUN_LEN(run), op = WFM_RUN_OP(run);
    unsigned long long tp, tt, te, tx;
    const unsigned long long pp = cp + block_excl<TRANS_WAVES>((valid && op != OP_I) ? len : 0u, wtot, &tp);
    const unsigned long long pt = ct + block_excl<TRANS_WAVES>((valid && op != OP_D) ? len : 0u, wtot, &tt);
    const unsigned long long pe = ce + block_excl<TRANS_WAVES>((valid && op == OP_M) ? len : 0u, wtot, &te);
    const unsigned long long px = cx + block_excl<TRANS_WAVES>((valid && op == OP_X) ? len : 0u, wtot, &tx);
    cp += tp; ct += tt; ce += te; cx += tx;
    if (valid) mypre[r] = make_uint4((uint32_t)pp, (uint32_t)pt, (uint32_t)pe, (uint32_t)px);
  }
  if (tid == 0) mypre[n] = make_uint4((uint32_t)cp, (uint32_t)ct, (uint32_t)ce, (uint32_t)cx);
}

__global__ __launch_bounds__(TRANS_THREADS) void trans_key_kernel(const TransArc* __restrict__ arcs, unsigned long long n,
                                                                  unsigned long long* __restrict__ key, unsigned long long* __restrict__ idx) {
  const unsigned long long i = (unsigned long long)blockIdx.x * TRANS_THREADS + threadIdx.x;
  if (i < n) { key[i] = arcs[i].s; idx[i] = i; }
}

__global__ __launch_bounds__(TRANS_THREADS) void trans_gather_kernel(const TransArc* __restrict__ arcs, const unsigned long long* __restrict__ idx,
                                                                     unsigned long long n, TransArc* __restrict__ sorted) {
  const unsigned long long i = (unsigned long long)blockIdx.x * TRANS_THREADS + threadIdx.x;
  if (i < n) sorted[i] = arcs[idx[i]];  // (idx is a permutation of [0, n): the sort's values)
}

__global__ __launch_bounds__(TRANS_THREADS) void trans_count_kernel(const unsigned long long* __restrict__ ks, const unsigned long long* __restrict__ ke,
                                                                    const unsigned long long* __restrict__ pks, const unsigned long long* __restrict__ pke,
                                                                    unsigned long long m_prev, const TransArc* __restrict__ arcs,
                                                                    const unsigned long long* __restrict__ pm, unsigned long long n_arcs,
                                                                    ulonglong2* __restrict__ win, unsigned long long* __restrict__ cnt) {
  __shared__ unsigned long long wtot[TRANS_WAVES];
  __shared__ unsigned long long s_lo, s_hi;
  const unsigned long long key_a = ks[blockIdx.x], key_b = ke[blockIdx.x];
  const unsigned long long a = key_a & TRANS_POS, b = key_b & TRANS_POS;
  if (threadIdx.x == 0) {
    // an interval the list before held as it is has been projected: its hulls are in the list
    const unsigned long long at = first_true(m_prev, [&](unsigned long long i) { return pks[i] >= key_a; });
    const bool old = at < m_prev && pks[at] == key_a && pke[at] == key_b;
    s_lo = old ? 0ull : first_true(n_arcs, [&](unsigned long long i) { return pm[i] > a; });
    s_hi = old ? 0ull : first_true(n_arcs, [&](unsigned long long i) { return arcs[i].s >= b; });
  }
  __syncthreads();
  const unsigned long long lo = s_lo, hi = s_hi > s_lo ? s_hi : s_lo;
  unsigned long long c = 0;
  for (unsigned long long i = lo + threadIdx.x; i < hi; i += TRANS_THREADS) c += arcs[i].s + arcs[i].slen > a;
  unsigned long long all;
  (void)block_excl<TRANS_WAVES>(c, wtot, &all);
  if (threadIdx.x == 0) { win[blockIdx.x] = make_ulonglong2(lo, hi); cnt[blockIdx.x] = all; }
}

// One pair.  P: the record's n + 1 prefix words {pattern, text, = columns, X columns} (the totals last); text: the source axis is the text
// (a back arc), else the pattern; [c0, c1), c0 < c1 <= the source span, offsets on that axis.  A source offset finds its run by the LAST
// prefix at or before it: a run that does not advance the axis (I on the pattern, D on the text) shares its prefix with the run behind it,
// so the last match is the run that holds the base; final runs of that kind hold the span itself, beyond every offset asked for.  That gives
// the ordinal of the nearest aligned column inward; the ordinal finds its run the same way among the aligned-column prefixes.  A run is
// aligned where the ordinal grows over it.  false: no aligned source base in [c0, c1).  d0, d1: the other axis' offsets opposite the first
// aligned base and one past the one opposite the last.
__device__ __forceinline__ bool trans_resolve(const uint4* __restrict__ P, uint32_t n, bool text, uint32_t c0, uint32_t c1, uint32_t* d0, uint32_t* d1) {
  auto src = [&](const uint4& w) { return text ? w.y : w.x; };
  auto dst = [&](const uint4& w) { return text ? w.x : w.y; };
  auto ord = [&](const uint4& w) { return w.z + w.w; };
  const uint32_t r0 = last_le(0u, n, [&](uint32_t r) { return src(P[r]) <= c0; });
  const uint32_t r1 = last_le(0u, n, [&](uint32_t r) { return src(P[r]) <= c1 - 1u; });
  const uint4 w0 = P[r0], w1 = P[r1];
  const uint32_t ord0 = ord(w0) + (ord(P[r0 + 1]) > ord(w0) ? c0 - src(w0) : 0u);  // the first aligned column at or behind c0
  const uint32_t ord1 = ord(w1) + (ord(P[r1 + 1]) > ord(w1) ? c1 - src(w1) : 0u);  // one past the last aligned column before c1
  if (ord0 >= ord1) return false;
  const uint32_t ra = last_le(0u, n, [&](uint32_t r) { return ord(P[r]) <= ord0; });
  const uint32_t rb = last_le(0u, n, [&](uint32_t r) { return ord(P[r]) <= ord1 - 1u; });
  const uint4 wa = P[ra], wb = P[rb];
  *d0 = dst(wa) + (ord0 - ord(wa));
  *d1 = dst(wb) + (ord1 - ord(wb));
  return true;
}

// the intervals from ka on, one per workgroup; oks[0] / oke[0] is pair number off[ka] of the round
__global__ __launch_bounds__(TRANS_THREADS) void trans_write_kernel(const unsigned long long* __restrict__ ks, const unsigned long long* __restrict__ ke,
                                                                    const ulonglong2* __restrict__ win, const unsigned long long* __restrict__ off,
                                                                    unsigned long long ka, const TransArc* __restrict__ arcs,
                                                                    const uint4* __restrict__ pre, unsigned long long* __restrict__ oks,
                                                                    unsigned long long* __restrict__ oke) {
  __shared__ unsigned long long wtot[TRANS_WAVES];
  const unsigned long long k = ka + blockIdx.x;
  if (off[k + 1] == off[k]) return;  // (the whole workgroup)
  const ulonglong2 w = win[k];
  const unsigned long long key_a = ks[k], key_b = ke[k];
  const unsigned long long seed = key_a & ~TRANS_POS, a = key_a & TRANS_POS, b = key_b & TRANS_POS;
  unsigned long long at = off[k] - off[ka];
  for (unsigned long long base = w.x; base < w.y; base += TRANS_THREADS) {
    const unsigned long long i = base + threadIdx.x;
    TransArc arc;
    arc.s = 0; arc.d = 0; arc.pre = 0; arc.slen = 0; arc.n_runs = 0;
    if (i < w.y) arc = arcs[i];
    const unsigned long long e = arc.s + arc.slen;
    const bool take = i < w.y && e > a;  // (trans_count_kernel counted the same arcs: slot < off[k + 1] - off[ka])
    unsigned long long all;
    const unsigned long long slot = at + block_excl<TRANS_WAVES>(take ? 1u : 0u, wtot, &all);
    at += all;
    if (!take) continue;
    unsigned long long lo = a, hi = b;  // an empty hull: the interval itself, which the list holds
    const unsigned long long s0 = arc.s > a ? arc.s : a, s1 = e < b ? e : b;
    if (s0 < s1 && arc.n_runs) {
      const uint4* P = pre + (arc.pre & TRANS_ARC_PRE);
      const bool back = (arc.pre & TRANS_ARC_BACK) != 0, rev = (arc.pre & TRANS_ARC_REVERSE) != 0;
      const uint4 tot = P[arc.n_runs];
      uint32_t c0 = (uint32_t)(s0 - arc.s), c1 = (uint32_t)(s1 - arc.s), d0 = 0, d1 = 0;
      // a back arc's source is the forward query window: text index i is its base slen - 1 - i where the record is reversed
      if (back && rev) { const uint32_t u = arc.slen - c1; c1 = arc.slen - c0; c0 = u; }
      if (trans_resolve(P, arc.n_runs, back, c0, c1, &d0, &d1)) {
        if (!back && rev) { const uint32_t u = tot.y - d1; d1 = tot.y - d0; d0 = u; }
        lo = arc.d + d0; hi = arc.d + d1;
      }
    }
    oks[slot] = seed | lo; oke[slot] = seed | hi;
  }
}

unsigned trans_blocks(unsigned long long n, unsigned long long per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

void launch_trans_span(const uint32_t* runs, const TransProb* probs, int nprob, unsigned long long n_bases, TransSpan* out, hipStream_t st) {
  if (nprob <= 0) return;
  hipLaunchKernelGGL(trans_span_kernel, dim3((unsigned)nprob), dim3(TRANS_THREADS), 0, st, runs, probs, n_bases, out);
}

void launch_trans_pre(const uint32_t* runs, const TransProb* probs, int nprob, const unsigned long long* pre_off, void* pre, hipStream_t st) {
  if (nprob <= 0) return;
  hipLaunchKernelGGL(trans_pre_kernel, dim3((unsigned)nprob), dim3(TRANS_THREADS), 0, st, runs, probs, pre_off, (uint4*)pre);
}

void launch_trans_keys(const TransArc* arcs, unsigned long long n, unsigned long long* key, unsigned long long* idx, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(trans_key_kernel, dim3(trans_blocks(n, TRANS_THREADS)), dim3(TRANS_THREADS), 0, st, arcs, n, key, idx);
}

void launch_trans_index(const TransArc* arcs, const unsigned long long* idx, unsigned long long n, TransArc* sorted, unsigned long long* maxs,
                        unsigned long long* pm, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(trans_gather_kernel, dim3(trans_blocks(n, TRANS_THREADS)), dim3(TRANS_THREADS), 0, st, arcs, idx, n, sorted);
  launch_runmax<TRANS_WAVES>(LoadArcEnd{sorted}, n, maxs, pm, st);  // pm[i] = max(source end[0 .. i])
}

void launch_trans_count(const unsigned long long* ks, const unsigned long long* ke, unsigned long long m, const unsigned long long* pks,
                        const unsigned long long* pke, unsigned long long m_prev, const TransArc* arcs, const unsigned long long* pm,
                        unsigned long long n_arcs, void* win, unsigned long long* cnt, unsigned long long* off, hipStream_t st) {
  if (m == 0) return;
  hipLaunchKernelGGL(trans_count_kernel, dim3((unsigned)m), dim3(TRANS_THREADS), 0, st, ks, ke, pks, pke, m_prev, arcs, pm, n_arcs, (ulonglong2*)win, cnt);
  // off[i] = the pairs of the intervals before i, off[m] = all of them
  hipLaunchKernelGGL((scan_sums_kernel<TRANS_WAVES, false, LoadWord>), dim3(1), dim3(TRANS_THREADS), 0, st, LoadWord{cnt}, m, off, (unsigned long long*)nullptr);
}

void launch_trans_write(const unsigned long long* ks, const unsigned long long* ke, const void* win, const unsigned long long* off,
                        unsigned long long ka, unsigned long long kb, const TransArc* arcs, const void* pre, unsigned long long* oks,
                        unsigned long long* oke, hipStream_t st) {
  if (kb <= ka) return;
  hipLaunchKernelGGL(trans_write_kernel, dim3((unsigned)(kb - ka)), dim3(TRANS_THREADS), 0, st, ks, ke, (const ulonglong2*)win, off, ka, arcs, (const uint4*)pre, oks, oke);
}

}  // namespace wfm
