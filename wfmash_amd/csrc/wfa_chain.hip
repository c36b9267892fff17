// wfa_chain.hip -- the kernels behind wfm_chain_runs (include/wfmash_hip.h): the runs of many records compacted into the blocks and gaps of a
// UCSC chain.  The pattern is the target, the text the query as aligned.  Nothing but runs is read: no sequence bytes.
//
//   chain_index_kernel     one workgroup per problem.  wfa_scan.h's run_span takes the pattern and text spans (the problem is refused when a
//                          span does not fit 32 bits, a run is empty or there are no runs) BEFORE anything is written; the second pass goes in
//                          rounds of 256 runs with a carry, stores per run the four exclusive prefixes {pattern, text, = columns, X columns} as
//                          ONE 16-byte word (lift_index_kernel's) and the four totals behind the last run, and counts the HEADS: an aligned run
//                          whose predecessor is not aligned, or the first run if it is aligned.  Two binary searches by one lane then give the
//                          bases before the first block and behind the last one.
//   scan_sums_kernel       (wfa_scan.h) ONE workgroup: the counts to their exclusive prefixes over the problems.
//   chain_write_kernel     one workgroup per problem of a chunk, rounds of 256 runs: head number k by a block scan of the head flags plus the
//                          carry (no atomics: two calls give the same bytes), ONE lane per head.  With A = the aligned columns before a run
//                          and G = the gap bases before it (both from its prefix word, both ascending), the first gap run g behind head r is
//                          the LAST index with G == G[r], the next head the LAST index with A == A[g], the gap run behind the block before
//                          the FIRST index with A == A[r]: binary searches over the n + 1 words, never a walk.  size and eq are prefix
//                          differences between r and g, (dt, dq) between g and the next head -- or, under WFM_CHAIN_REVERSE, where block k
//                          goes to slot n - 1 - k, between the gap run behind the block before and r.  16 bytes a block in one store.
// Offsets inside a problem are 32-bit (the spans fit), sums of two of them 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wfmash_hip.h"
#include "wfa_device.h"
#include "wfa_scan.h"

namespace wfm {
namespace {

constexpr int CHAIN_THREADS = 256;
constexpr int CHAIN_WAVES = CHAIN_THREADS / 64;

struct LoadChainCount { const ChainWin* p; __device__ __forceinline__ unsigned long long operator()(unsigned long long i) const { return p[i].count; } };

// the aligned columns and the gap bases before the run a prefix word belongs to
__device__ __forceinline__ unsigned long long chain_aligned(const uint4 w) { return (unsigned long long)w.z + w.w; }
__device__ __forceinline__ unsigned long long chain_gaps(const uint4 w) { return (unsigned long long)w.x + w.y - 2ull * chain_aligned(w); }

__global__ __launch_bounds__(CHAIN_THREADS) void chain_index_kernel(const uint32_t* __restrict__ runs, const ChainProb* __restrict__ probs,
                                                                    uint4* __restrict__ pre, ChainWin* __restrict__ win) {
  const ChainProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x;
  __shared__ unsigned long long wtot[CHAIN_WAVES];
  __shared__ uint32_t s_bad;
  const uint32_t* my = runs + pr.runs_off;
  const uint32_t n = pr.n_runs;
  // the spans first: nothing is written for a problem that is refused
  unsigned long long span, tspan;
  const bool empty_run = run_span<CHAIN_WAVES, true>(my, n, wtot, &s_bad, &span, &tspan);
  if (empty_run || n == 0 || span > 0xffffffffull || tspan > 0xffffffffull) {
    if (tid == 0) { ChainWin w; w.count = 0; w.flags = WFM_CHAIN_SPANS; w.lead_dt = w.lead_dq = w.trail_dt = w.trail_dq = w.eq = w.x = 0; w.pad_ = 0; win[blockIdx.x] = w; }
    return;
  }
  uint4* mypre = pre + pr.pre_off;
  unsigned long long cp = 0, ct = 0, ce = 0, cx = 0, heads = 0;
  for (uint32_t base = 0; base < n; base += CHAIN_THREADS) {
    const uint32_t r = base + (uint32_t)tid;
    const bool valid = r < n;
    const uint32_t run = valid ? my[r] : 0u;
    const uint32_t len = WFM_RUN_LEN(run), op = WFM_RUN_OP(run);
    unsigned long long tp, tt, te, tx;
    const unsigned long long pp = cp + block_excl<CHAIN_WAVES>((valid && op != OP_I) ? len : 0u, wtot, &tp);
    const unsigned long long pt = ct + block_excl<CHAIN_WAVES>((valid && op != OP_D) ? len : 0u, wtot, &tt);
    const unsigned long long pe = ce + block_excl<CHAIN_WAVES>((valid && op == OP_M) ? len : 0u, wtot, &te);
    const unsigned long long px = cx + block_excl<CHAIN_WAVES>((valid && op == OP_X) ? len : 0u, wtot, &tx);
    cp += tp; ct += tt; ce += te; cx += tx;
    if (valid) mypre[r] = make_uint4((uint32_t)pp, (uint32_t)pt, (uint32_t)pe, (uint32_t)px);
    heads += valid && op <= OP_X && (r == 0 || WFM_RUN_OP(my[r - 1]) > OP_X);
  }
  unsigned long long count;
  (void)block_excl<CHAIN_WAVES>(heads, wtot, &count);
  if (tid != 0) return;
  mypre[n] = make_uint4((uint32_t)cp, (uint32_t)ct, (uint32_t)ce, (uint32_t)cx);
  // (block_excl's barriers lie behind every lane's stores to mypre[0 .. n): this lane may read them)
  const unsigned long long all = ce + cx;
  uint32_t ldt = (uint32_t)(cp - all), ldq = (uint32_t)(ct - all), rdt = 0, rdq = 0;  // gap runs only: everything leads
  if (all) {
    // the first head is the last run with no aligned column before it; the first run behind the last block the first with all of them
    const uint32_t h0 = last_le(0u, n + 1u, [&](uint32_t r) { return chain_aligned(mypre[r]) == 0; });
    const uint32_t g1 = (uint32_t)first_true(n, [&](unsigned long long r) { return chain_aligned(mypre[r]) >= all; });
    const uint4 w0 = mypre[h0];
    ldt = w0.x; ldq = w0.y;  // (nothing aligned before h0: its prefixes are D and I bases alone)
    const uint4 w1 = g1 < n ? mypre[g1] : make_uint4((uint32_t)cp, (uint32_t)ct, 0u, 0u);
    rdt = (uint32_t)cp - w1.x; rdq = (uint32_t)ct - w1.y;
  }
  ChainWin w;
  w.count = count; w.flags = 0; w.eq = (uint32_t)ce; w.x = (uint32_t)cx; w.pad_ = 0;
  const bool rev = pr.flags & WFM_CHAIN_REVERSE, swp = pr.flags & WFM_CHAIN_SWAP;
  const uint32_t a_dt = rev ? rdt : ldt, a_dq = rev ? rdq : ldq, b_dt = rev ? ldt : rdt, b_dq = rev ? ldq : rdq;
  w.lead_dt = swp ? a_dq : a_dt; w.lead_dq = swp ? a_dt : a_dq;
  w.trail_dt = swp ? b_dq : b_dt; w.trail_dq = swp ? b_dt : b_dq;
  win[blockIdx.x] = w;
}

// the problems from ka on, one per workgroup; out[0] is block number off[ka] of the whole call
__global__ __launch_bounds__(CHAIN_THREADS) void chain_write_kernel(const uint32_t* __restrict__ runs, const ChainProb* __restrict__ probs,
                                                                    const uint4* __restrict__ pre, const ChainWin* __restrict__ win,
                                                                    const unsigned long long* __restrict__ off, uint32_t ka, uint4* __restrict__ out) {
  __shared__ unsigned long long wtot[CHAIN_WAVES];
  const uint32_t k = ka + blockIdx.x;
  const unsigned long long count = win[k].count;
  if (count == 0) return;  // (the whole workgroup)
  const ChainProb pr = probs[k];
  const uint4* P = pre + pr.pre_off;
  const uint32_t* my = runs + pr.runs_off;
  const uint32_t n = pr.n_runs;
  const bool rev = pr.flags & WFM_CHAIN_REVERSE, swp = pr.flags & WFM_CHAIN_SWAP;
  uint4* mine = out + (off[k] - off[ka]);
  unsigned long long carry = 0;
  for (uint32_t base = 0; base < n; base += CHAIN_THREADS) {
    const uint32_t r = base + (uint32_t)threadIdx.x;
    const bool head = r < n && WFM_RUN_OP(my[r]) <= OP_X && (r == 0 || WFM_RUN_OP(my[r - 1]) > OP_X);
    unsigned long long all;
    const unsigned long long b = carry + block_excl<CHAIN_WAVES>(head ? 1u : 0u, wtot, &all);
    carry += all;
    if (!head) continue;
    const uint4 wr = P[r];
    const unsigned long long gr = chain_gaps(wr);
    const uint32_t g = last_le(r, n + 1u, [&](uint32_t i) { return chain_gaps(P[i]) <= gr; });  // (r < g <= n: run r is aligned)
    const uint4 wg = P[g];
    uint32_t dt = 0, dq = 0;
    if (!rev) {
      const unsigned long long ag = chain_aligned(wg);
      const uint32_t h2 = last_le(g, n + 1u, [&](uint32_t i) { return chain_aligned(P[i]) <= ag; });
      if (h2 < n) { const uint4 wh = P[h2]; dt = wh.x - wg.x; dq = wh.y - wg.y; }  // (h2 == n: gap runs to the end, the trail)
    } else if (b) {
      const unsigned long long ar = chain_aligned(wr);
      const uint32_t gp = (uint32_t)first_true(r, [&](unsigned long long i) { return chain_aligned(P[i]) >= ar; });  // (0 < gp < r: a block lies before)
      const uint4 wp = P[gp];
      dt = wr.x - wp.x; dq = wr.y - wp.y;
    }
    // (b < count: chain_index_kernel counted the same heads)
    const unsigned long long slot = rev ? count - 1 - b : b;
    mine[slot] = make_uint4((uint32_t)(chain_aligned(wg) - chain_aligned(wr)), swp ? dq : dt, swp ? dt : dq, wg.z - wr.z);
  }
}

}  // namespace

void launch_chain_index(const uint32_t* runs, const ChainProb* probs, int nprob, void* pre, ChainWin* win, unsigned long long* off, hipStream_t st) {
  if (nprob <= 0) return;
  hipLaunchKernelGGL(chain_index_kernel, dim3((unsigned)nprob), dim3(CHAIN_THREADS), 0, st, runs, probs, (uint4*)pre, win);
  // off[i] = the blocks of the problems before i, off[nprob] = all of them
  hipLaunchKernelGGL((scan_sums_kernel<CHAIN_WAVES, false, LoadChainCount>), dim3(1), dim3(CHAIN_THREADS), 0, st, LoadChainCount{win}, (unsigned long long)nprob, off,
                     (unsigned long long*)nullptr);
}

void launch_chain_write(const uint32_t* runs, const ChainProb* probs, const void* pre, const ChainWin* win, const unsigned long long* off, uint32_t ka,
                        uint32_t kb, void* out, hipStream_t st) {
  if (kb <= ka) return;
  hipLaunchKernelGGL(chain_write_kernel, dim3(kb - ka), dim3(CHAIN_THREADS), 0, st, runs, probs, (const uint4*)pre, win, off, ka, (uint4*)out);
}

}  // namespace wfm
