// wfa_net.hip -- the kernels behind wfm_net_* (include/wfmash_hip.h): the blocks of many records, and which record owns each base of the
// target.  Nothing but runs is read, and never a dense array: memory follows the N blocks, not the target's length.
//
//   net_count_kernel      one workgroup per problem.  wfa_scan.h's run_span takes the pattern and text spans; the problem is refused (an
//                         empty run, no runs, a span that leaves [0, n_bases] or does not fit 32 bits) BEFORE anything is written; then the
//                         number of maximal stretches of =/X runs (the blocks it will write) and its = columns (WFM_NET_SCORE_EQ's score).
//   scan_sums_kernel      (wfa_scan.h) ONE workgroup: the words (record << 32 | blocks) to their exclusive prefixes over the problems.
//   net_write_kernel      one workgroup per problem, rounds of 256 runs with carries (pav_write_kernel's shape): the pattern and text
//                         advances and the slot by block_excl, the start of the stretch a run lies in by a running maximum over the heads'
//                         (pattern << 32 | text) + 1 (both ascend from head to head).  The LAST run of a stretch writes the block.
// The table, with N blocks, R records, M elementary intervals, P pieces:
//   net_ends_kernel       e[2 i] = t, e[2 i + 1] = t + size; sorted by rocprim::radix_sort_keys (net_sort_keys).
//   net_flag_sum_kernel / net_distinct_kernel   the distinct coordinates x[0 .. M], compacted by a prefix of the flags (the blocks' sums
//                         by scan_sums_kernel; the apply step is the consumer's).
//   net_rec_keys_kernel, net_rec_rank_kernel, net_prio_kernel   the records sorted by order (equal neighbours are counted: the call
//                         refuses them) and, by ~score << 32 | rank, into a dense priority R .. 1.
//   net_fill_kernel       one lane per block: the rank of its record by a binary search over the sorted orders; [lo, hi) by two in x; then
//                         the canonical nodes of [lo, hi) in the implicit tree (node 1 the root, leaf k at M + k, any M), at most
//                         2 log2 M of them, each an atomicMax of priority << 32 | block index.  An integer maximum does not depend on who
//                         comes first; the loop's length depends on M alone, never on how many blocks pile on a base.  bases_aligned is
//                         an integer atomicAdd per block (sites_longhash_kernel's precedent: order-free).
//   net_push_kernel       level by level, root first: node i takes the maximum of itself and node i >> 1.  A gather; no atomics.
//   net_heads_*           leaf k heads a piece iff its winner w is non-zero and differs from leaf k - 1's, ends one iff w is non-zero and
//                         differs from leaf k + 1's; heads and tails alternate, so the j-th head and the j-th tail are one piece.
//   net_piece_keys_kernel the rank of a piece's record (the stable sort's key: the pieces arrive in t order) and bases_won (integer add).
//   net_pieces_kernel     a gather: {order, t, q = the block's q + (t - the block's t), size} at the sorted places.
//   net_per_kernel        one lane per record: its first piece and the next record's by two binary searches over the sorted ranks.
// No workgroup ever waits for another; no kernel uses scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include <rocprim/rocprim.hpp>

#include "../../include/wfmash_hip.h"
#include "wfa_device.h"
#include "wfa_scan.h"

namespace wfm {
namespace {

constexpr int NET_THREADS = 256;
constexpr int NET_WAVES = NET_THREADS / 64;
static_assert(WFM_NET_SCAN_BLOCK == NET_THREADS * 4, "a scan block is four elements per lane");

__device__ __forceinline__ bool net_in(uint32_t op) { return op <= OP_X; }

__global__ __launch_bounds__(NET_THREADS) void net_count_kernel(const uint32_t* __restrict__ runs, const NetProb* __restrict__ probs,
                                                                unsigned long long n_bases, uint32_t* __restrict__ flags,
                                                                unsigned long long* __restrict__ word, uint32_t* __restrict__ score) {
  const NetProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x;
  __shared__ unsigned long long wtot[NET_WAVES];
  __shared__ uint32_t s_bad;
  const uint32_t* my = runs + pr.runs_off;
  const uint32_t n = pr.n_runs;
  // the spans first: a problem that is refused writes nothing
  unsigned long long span, tspan;
  const bool empty_run = run_span<NET_WAVES, true>(my, n, wtot, &s_bad, &span, &tspan);
  const bool spans = empty_run || n == 0 || pr.base > n_bases || span > n_bases - pr.base || span > 0xffffffffull || tspan > 0xffffffffull;
  if (spans) {
    if (tid == 0) { flags[blockIdx.x] = WFM_NET_SPANS; word[blockIdx.x] = 0; score[blockIdx.x] = 0; }
    return;
  }
  unsigned long long c = 0, eq = 0;
  for (uint32_t r = (uint32_t)tid; r < n; r += NET_THREADS) {
    const uint32_t run = my[r];
    c += net_in(WFM_RUN_OP(run)) && (r + 1 == n || !net_in(WFM_RUN_OP(my[r + 1])));
    if (WFM_RUN_OP(run) == OP_M) eq += WFM_RUN_LEN(run);
  }
  unsigned long long all, all_eq;
  (void)block_excl<NET_WAVES>(c, wtot, &all);
  (void)block_excl<NET_WAVES>(eq, wtot, &all_eq);
  if (tid == 0) {
    flags[blockIdx.x] = 0;
    word[blockIdx.x] = (1ull << 32) | all;  // (all <= n_runs <= 2^31)
    score[blockIdx.x] = pr.score == WFM_NET_SCORE_EQ ? (uint32_t)all_eq : pr.score;  // (all_eq <= span < 2^32)
  }
}

__global__ __launch_bounds__(NET_THREADS) void net_write_kernel(const uint32_t* __restrict__ runs, const NetProb* __restrict__ probs,
                                                                const uint32_t* __restrict__ flags, const unsigned long long* __restrict__ off,
                                                                const uint32_t* __restrict__ score, NetBlock* __restrict__ blocks,
                                                                NetRec* __restrict__ recs) {
  if (flags[blockIdx.x]) return;  // (the whole workgroup)
  const NetProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x;
  __shared__ unsigned long long wtot[NET_WAVES];
  __shared__ unsigned long long wmax[NET_WAVES];
  const uint32_t* my = runs + pr.runs_off;
  const uint32_t n = pr.n_runs;
  const unsigned long long o = off[blockIdx.x];
  if (tid == 0) recs[o >> 32] = NetRec{pr.order, score[blockIdx.x], 0u};
  unsigned long long carry_p = 0, carry_q = 0, carry_s = o & 0xffffffffull, carry_h = 0;
  for (uint32_t base = 0; base < n; base += NET_THREADS) {
    const uint32_t r = base + (uint32_t)tid;
    const bool valid = r < n;
    const uint32_t run = valid ? my[r] : 0u;
    const uint32_t len = WFM_RUN_LEN(run), op = WFM_RUN_OP(run);
    const bool aligned = valid && net_in(op);
    const bool head = aligned && (r == 0 || !net_in(WFM_RUN_OP(my[r - 1])));
    const bool tail = aligned && (r + 1 == n || !net_in(WFM_RUN_OP(my[r + 1])));
    unsigned long long tp, tq, ts, th;
    const unsigned long long pp = carry_p + block_excl<NET_WAVES>((valid && op != OP_I) ? len : 0u, wtot, &tp);  // (from the problem's base)
    const unsigned long long qq = carry_q + block_excl<NET_WAVES>((valid && op != OP_D) ? len : 0u, wtot, &tq);
    const unsigned long long slot = carry_s + block_excl<NET_WAVES>(tail ? 1u : 0u, wtot, &ts);
    // where the stretch this run lies in begins, on both sides, + 1: from head to head both ascend, so the latest head is the largest.
    // (a head's pp is below the span, so below 2^32 - 1: the word does not wrap)
    unsigned long long h1 = block_incl_max<NET_WAVES>(head ? ((pp << 32) | qq) + 1 : 0ull, wmax, &th);
    if (carry_h > h1) h1 = carry_h;
    carry_p += tp; carry_q += tq; carry_s += ts;
    if (th > carry_h) carry_h = th;
    // (slot is below the next problem's: net_count_kernel counted the same tails)
    if (tail) {
      const unsigned long long hp = (h1 - 1) >> 32, hq = (h1 - 1) & 0xffffffffull;
      blocks[slot] = NetBlock{pr.order, pr.base + hp, (uint32_t)hq, (uint32_t)(pp + len - hp)};
    }
  }
}

__global__ __launch_bounds__(NET_THREADS) void net_ends_kernel(const NetBlock* __restrict__ blocks, unsigned long long n, unsigned long long* __restrict__ e) {
  const unsigned long long i = (unsigned long long)blockIdx.x * NET_THREADS + threadIdx.x;
  if (i >= n) return;
  const NetBlock b = blocks[i];
  e[2 * i] = b.t;
  e[2 * i + 1] = b.t + b.size;
}

// what the two compactions count per element.  DISTINCT: sorted value i differs from i - 1.  Else: leaf i heads a piece
template <bool DISTINCT>
__device__ __forceinline__ unsigned long long net_term(const unsigned long long* __restrict__ a, unsigned long long i) {
  if (DISTINCT) return (i == 0 || a[i] != a[i - 1]) ? 1ull : 0ull;
  return (a[i] != 0 && (i == 0 || a[i] != a[i - 1])) ? 1ull : 0ull;
}

template <bool DISTINCT>
__global__ __launch_bounds__(NET_THREADS) void net_flag_sum_kernel(const unsigned long long* __restrict__ a, unsigned long long n,
                                                                   unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long wtot[NET_WAVES];
  const unsigned long long at = (unsigned long long)blockIdx.x * WFM_NET_SCAN_BLOCK + (unsigned long long)threadIdx.x * 4u;
  unsigned long long v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (at + k < n) v += net_term<DISTINCT>(a, at + k);
  unsigned long long all;
  (void)block_excl<NET_WAVES>(v, wtot, &all);
  if (threadIdx.x == 0) sums[blockIdx.x] = all;
}

__global__ __launch_bounds__(NET_THREADS) void net_distinct_kernel(const unsigned long long* __restrict__ a, unsigned long long n,
                                                                   const unsigned long long* __restrict__ sums, unsigned long long* __restrict__ x) {
  __shared__ unsigned long long wtot[NET_WAVES];
  const unsigned long long at = (unsigned long long)blockIdx.x * WFM_NET_SCAN_BLOCK + (unsigned long long)threadIdx.x * 4u;
  unsigned long long f[4], v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { f[k] = at + k < n ? net_term<true>(a, at + k) : 0ull; v += f[k]; }
  unsigned long long all;
  unsigned long long rank = sums[blockIdx.x] + block_excl<NET_WAVES>(v, wtot, &all);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (f[k]) x[rank] = a[at + k];  // (rank is below the total, which is n at most: x has n words)
    rank += f[k];
  }
}

// leaves: the tree from node m on.  The j-th head writes the piece's start and winner, the j-th tail its end
__global__ __launch_bounds__(NET_THREADS) void net_heads_kernel(const unsigned long long* __restrict__ leaves, const unsigned long long* __restrict__ x,
                                                                unsigned long long m, const unsigned long long* __restrict__ sums,
                                                                unsigned long long* __restrict__ ps, unsigned long long* __restrict__ pe,
                                                                unsigned long long* __restrict__ pw) {
  __shared__ unsigned long long wtot[NET_WAVES];
  const unsigned long long at = (unsigned long long)blockIdx.x * WFM_NET_SCAN_BLOCK + (unsigned long long)threadIdx.x * 4u;
  unsigned long long f[4], v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { f[k] = at + k < m ? net_term<false>(leaves, at + k) : 0ull; v += f[k]; }
  unsigned long long all;
  unsigned long long rank = sums[blockIdx.x] + block_excl<NET_WAVES>(v, wtot, &all);  // the heads before this lane's first leaf
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long i = at + k;
    if (i >= m) break;
    const unsigned long long w = leaves[i];
    if (f[k]) { ps[rank] = x[i]; pw[rank] = w; }
    rank += f[k];
    // (a leaf with a winner lies behind a head, so rank >= 1 here; rank <= the total the caller made room for)
    if (w != 0 && (i + 1 == m || leaves[i + 1] != w)) pe[rank - 1] = x[i + 1];
  }
}

__global__ __launch_bounds__(NET_THREADS) void net_rec_keys_kernel(const NetRec* __restrict__ recs, uint32_t r, unsigned long long* __restrict__ ro,
                                                                   uint32_t* __restrict__ ri) {
  const uint32_t i = blockIdx.x * NET_THREADS + threadIdx.x;
  if (i >= r) return;
  ro[i] = recs[i].order;
  ri[i] = i;
}

__global__ __launch_bounds__(NET_THREADS) void net_rec_rank_kernel(const NetRec* __restrict__ recs, uint32_t r, const unsigned long long* __restrict__ so,
                                                                   const uint32_t* __restrict__ sp, unsigned long long* __restrict__ k2,
                                                                   uint32_t* __restrict__ sscore, uint32_t* __restrict__ bad) {
  const uint32_t j = blockIdx.x * NET_THREADS + threadIdx.x;
  if (j >= r) return;
  const uint32_t s = recs[sp[j]].score;
  sscore[j] = s;
  k2[j] = ((unsigned long long)(~s) << 32) | j;  // ascending: the greatest score first, then the smallest order
  if (j && so[j] == so[j - 1]) atomicMax(&bad[0], 1u);
}

__global__ __launch_bounds__(NET_THREADS) void net_prio_kernel(const uint32_t* __restrict__ p2, uint32_t r, uint32_t* __restrict__ prio) {
  const uint32_t i = blockIdx.x * NET_THREADS + threadIdx.x;
  if (i < r) prio[p2[i]] = r - i;  // (p2 is a permutation: every rank is written once)
}

__global__ __launch_bounds__(NET_THREADS) void net_fill_kernel(const NetBlock* __restrict__ blocks, unsigned long long n,
                                                               const unsigned long long* __restrict__ so, uint32_t r, const uint32_t* __restrict__ prio,
                                                               const unsigned long long* __restrict__ x, unsigned long long m,
                                                               unsigned long long* __restrict__ tree, uint32_t* __restrict__ brank,
                                                               unsigned long long* __restrict__ aligned, uint32_t* __restrict__ bad) {
  const unsigned long long i = (unsigned long long)blockIdx.x * NET_THREADS + threadIdx.x;
  if (i >= n) return;
  const NetBlock b = blocks[i];
  const unsigned long long rk = first_true(r, [&](unsigned long long u) { return so[u] >= b.order; });
  if (rk >= r || so[rk] != b.order) { brank[i] = 0; atomicMax(&bad[1], 1u); return; }  // (import looks for this on the host)
  brank[i] = (uint32_t)rk;
  atomicAdd(&aligned[rk], (unsigned long long)b.size);
  // x holds both ends of every block: the searches find them.  lo < hi <= m as size >= 1
  unsigned long long lo = first_true(m + 1, [&](unsigned long long u) { return x[u] >= b.t; });
  unsigned long long hi = first_true(m + 1, [&](unsigned long long u) { return x[u] >= b.t + b.size; });
  if (hi > m) hi = m;
  const unsigned long long v = ((unsigned long long)prio[rk] << 32) | i;
  for (lo += m, hi += m; lo < hi; lo >>= 1, hi >>= 1) {  // (nodes 1 .. 2 m - 1)
    if (lo & 1) atomicMax(&tree[lo++], v);
    if (hi & 1) atomicMax(&tree[--hi], v);
  }
}

// the nodes [a, b) of one level: their parents are final
__global__ __launch_bounds__(NET_THREADS) void net_push_kernel(unsigned long long* __restrict__ tree, unsigned long long a, unsigned long long b) {
  const unsigned long long i = a + (unsigned long long)blockIdx.x * NET_THREADS + threadIdx.x;
  if (i >= b) return;
  const unsigned long long up = tree[i >> 1];
  if (up > tree[i]) tree[i] = up;
}

__global__ __launch_bounds__(NET_THREADS) void net_piece_keys_kernel(const unsigned long long* __restrict__ ps, const unsigned long long* __restrict__ pe,
                                                                     const unsigned long long* __restrict__ pw, unsigned long long p,
                                                                     const uint32_t* __restrict__ brank, uint32_t* __restrict__ key, uint32_t* __restrict__ val,
                                                                     unsigned long long* __restrict__ won) {
  const unsigned long long j = (unsigned long long)blockIdx.x * NET_THREADS + threadIdx.x;
  if (j >= p) return;
  const uint32_t rk = brank[pw[j] & 0xffffffffull];
  key[j] = rk;
  val[j] = (uint32_t)j;
  atomicAdd(&won[rk], pe[j] - ps[j]);
}

__global__ __launch_bounds__(NET_THREADS) void net_pieces_kernel(const NetBlock* __restrict__ blocks, const unsigned long long* __restrict__ ps,
                                                                 const unsigned long long* __restrict__ pe, const unsigned long long* __restrict__ pw,
                                                                 const uint32_t* __restrict__ sv, unsigned long long a, unsigned long long b,
                                                                 NetBlock* __restrict__ out) {
  const unsigned long long s = a + (unsigned long long)blockIdx.x * NET_THREADS + threadIdx.x;
  if (s >= b) return;
  const uint32_t j = sv[s];
  const NetBlock blk = blocks[pw[j] & 0xffffffffull];
  const unsigned long long t = ps[j];
  out[s - a] = NetBlock{blk.order, t, blk.q + (uint32_t)(t - blk.t), (uint32_t)(pe[j] - t)};  // (inside the block: below its q + size)
}

__global__ __launch_bounds__(NET_THREADS) void net_per_kernel(const unsigned long long* __restrict__ so, const uint32_t* __restrict__ sscore, uint32_t r,
                                                              const uint32_t* __restrict__ sk, unsigned long long p,
                                                              const unsigned long long* __restrict__ won, const unsigned long long* __restrict__ aligned,
                                                              NetPer* __restrict__ per) {
  const uint32_t j = blockIdx.x * NET_THREADS + threadIdx.x;
  if (j >= r) return;
  const unsigned long long first = first_true(p, [&](unsigned long long u) { return sk[u] >= j; });
  const unsigned long long next = first_true(p, [&](unsigned long long u) { return sk[u] > j; });
  per[j] = NetPer{so[j], sscore[j], 0u, first, next - first, won[j], aligned[j]};
}

unsigned net_blocks_of(unsigned long long n, unsigned long long per) { return (unsigned)((n + per - 1) / per); }

// ONE workgroup: words[0 .. n) to their exclusive prefixes in out (which may be words), out[n] = the total
void net_scan_words(const unsigned long long* words, unsigned long long n, unsigned long long* out, hipStream_t st) {
  hipLaunchKernelGGL((scan_sums_kernel<NET_WAVES, false, LoadWord>), dim3(1), dim3(NET_THREADS), 0, st, LoadWord{words}, n, out, (unsigned long long*)nullptr);
}

}  // namespace

void launch_net_count(const uint32_t* runs, const NetProb* probs, int nprob, unsigned long long n_bases, uint32_t* flags, unsigned long long* word,
                      unsigned long long* off, uint32_t* score, hipStream_t st) {
  if (nprob <= 0) return;
  hipLaunchKernelGGL(net_count_kernel, dim3((unsigned)nprob), dim3(NET_THREADS), 0, st, runs, probs, n_bases, flags, word, score);
  net_scan_words(word, (unsigned long long)nprob, off, st);
}

void launch_net_write(const uint32_t* runs, const NetProb* probs, int nprob, const uint32_t* flags, const unsigned long long* off, const uint32_t* score,
                      NetBlock* blocks, NetRec* recs, hipStream_t st) {
  if (nprob <= 0) return;
  hipLaunchKernelGGL(net_write_kernel, dim3((unsigned)nprob), dim3(NET_THREADS), 0, st, runs, probs, flags, off, score, blocks, recs);
}

void launch_net_ends(const NetWork& w, hipStream_t st) {
  if (w.n == 0) return;
  hipLaunchKernelGGL(net_ends_kernel, dim3(net_blocks_of(w.n, NET_THREADS)), dim3(NET_THREADS), 0, st, w.blocks, w.n, w.e);
}

hipError_t net_sort_keys(void* tmp, size_t* tmp_bytes, const unsigned long long* k, unsigned long long* k2, unsigned long long n, unsigned end_bit, hipStream_t st) {
  return rocprim::radix_sort_keys(tmp, *tmp_bytes, k, k2, (size_t)n, 0u, end_bit, st);
}

void launch_net_distinct(const NetWork& w, hipStream_t st) {
  const unsigned long long n2 = 2 * w.n;
  if (n2 == 0) return;
  const unsigned nb = net_blocks_of(n2, WFM_NET_SCAN_BLOCK);
  hipLaunchKernelGGL(net_flag_sum_kernel<true>, dim3(nb), dim3(NET_THREADS), 0, st, (const unsigned long long*)w.e2, n2, w.aux);
  net_scan_words(w.aux, (unsigned long long)nb, w.aux, st);
  hipLaunchKernelGGL(net_distinct_kernel, dim3(nb), dim3(NET_THREADS), 0, st, (const unsigned long long*)w.e2, n2, (const unsigned long long*)w.aux, w.e);
}

void launch_net_rec_keys(const NetWork& w, hipStream_t st) {
  if (w.r == 0) return;
  hipLaunchKernelGGL(net_rec_keys_kernel, dim3(net_blocks_of(w.r, NET_THREADS)), dim3(NET_THREADS), 0, st, w.recs, w.r, w.ro, w.ri);
}

void launch_net_rec_rank(const NetWork& w, hipStream_t st) {
  if (w.r == 0) return;
  hipLaunchKernelGGL(net_rec_rank_kernel, dim3(net_blocks_of(w.r, NET_THREADS)), dim3(NET_THREADS), 0, st, w.recs, w.r, (const unsigned long long*)w.so,
                     (const uint32_t*)w.sp, w.k2, w.sscore, w.bad);
}

void launch_net_prio(const NetWork& w, hipStream_t st) {
  if (w.r == 0) return;
  hipLaunchKernelGGL(net_prio_kernel, dim3(net_blocks_of(w.r, NET_THREADS)), dim3(NET_THREADS), 0, st, (const uint32_t*)w.p2, w.r, w.prio);
}

void launch_net_fill(const NetWork& w, hipStream_t st) {
  if (w.n == 0 || w.m == 0) return;
  hipLaunchKernelGGL(net_fill_kernel, dim3(net_blocks_of(w.n, NET_THREADS)), dim3(NET_THREADS), 0, st, w.blocks, w.n, (const unsigned long long*)w.so, w.r,
                     (const uint32_t*)w.prio, (const unsigned long long*)w.e, w.m, w.tree, w.brank, w.aligned, w.bad);
}

void launch_net_push(const NetWork& w, hipStream_t st) {
  const unsigned long long end = 2 * w.m;
  for (unsigned long long a = 2; a < end; a <<= 1) {
    const unsigned long long b = a * 2 < end ? a * 2 : end;
    hipLaunchKernelGGL(net_push_kernel, dim3(net_blocks_of(b - a, NET_THREADS)), dim3(NET_THREADS), 0, st, w.tree, a, b);
  }
}

void launch_net_heads_count(const NetWork& w, hipStream_t st) {
  if (w.m == 0) return;
  const unsigned nb = net_blocks_of(w.m, WFM_NET_SCAN_BLOCK);
  hipLaunchKernelGGL(net_flag_sum_kernel<false>, dim3(nb), dim3(NET_THREADS), 0, st, (const unsigned long long*)(w.tree + w.m), w.m, w.aux);
  net_scan_words(w.aux, (unsigned long long)nb, w.aux, st);
}

void launch_net_heads_write(const NetWork& w, hipStream_t st) {
  if (w.m == 0 || w.p == 0) return;
  const unsigned nb = net_blocks_of(w.m, WFM_NET_SCAN_BLOCK);
  hipLaunchKernelGGL(net_heads_kernel, dim3(nb), dim3(NET_THREADS), 0, st, (const unsigned long long*)(w.tree + w.m), (const unsigned long long*)w.e, w.m,
                     (const unsigned long long*)w.aux, w.ps, w.pe, w.pw);
}

void launch_net_piece_keys(const NetWork& w, hipStream_t st) {
  if (w.p == 0) return;
  hipLaunchKernelGGL(net_piece_keys_kernel, dim3(net_blocks_of(w.p, NET_THREADS)), dim3(NET_THREADS), 0, st, (const unsigned long long*)w.ps,
                     (const unsigned long long*)w.pe, (const unsigned long long*)w.pw, w.p, (const uint32_t*)w.brank, w.key, w.val, w.won);
}

void launch_net_pieces(const NetWork& w, unsigned long long a, unsigned long long b, NetBlock* out, hipStream_t st) {
  if (b <= a) return;
  hipLaunchKernelGGL(net_pieces_kernel, dim3(net_blocks_of(b - a, NET_THREADS)), dim3(NET_THREADS), 0, st, w.blocks, (const unsigned long long*)w.ps,
                     (const unsigned long long*)w.pe, (const unsigned long long*)w.pw, (const uint32_t*)w.sv, a, b, out);
}

void launch_net_per(const NetWork& w, NetPer* per, hipStream_t st) {
  if (w.r == 0) return;
  hipLaunchKernelGGL(net_per_kernel, dim3(net_blocks_of(w.r, NET_THREADS)), dim3(NET_THREADS), 0, st, (const unsigned long long*)w.so, (const uint32_t*)w.sscore,
                     w.r, (const uint32_t*)w.sk, w.p, (const unsigned long long*)w.won, (const unsigned long long*)w.aligned, per);
}

}  // namespace wfm
