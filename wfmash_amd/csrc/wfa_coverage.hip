// wfa_coverage.hip -- the kernels behind wfm_coverage_* (include/wfmash_hip.h): per-base depth of the target from the runs of many records,
// kept as a DIFFERENCE array of int32 words over the concatenation of the target sequences.  Nothing but runs is read: no sequence bytes.
//
//   cov_add_kernel        one workgroup per problem.  wfa_scan.h's run_span takes the pattern span (the problem is refused when it leaves
//                         [0, n_bases] or holds an empty run) BEFORE any word is touched; the second pass goes in rounds of 256 runs with a
//                         carry (var_index_kernel's shape, wfa_scan.h's block_excl for the pattern advance) and emits +1 where an aligned
//                         segment (=/X runs with no I or D between them) begins and -1 where it ends: two integer atomics per segment.
//   cov_count_kernel      one workgroup per tile of WFM_COV_TILE words: how many are non-zero, read in 16-byte loads.
//   cov_sum_kernel        the two scans (tile counts; the deltas of a compact list) in the reduce / scan-of-sums / apply form, as separate
//                         launches: per block of WFM_COV_SCAN_BLOCK elements its sum; ONE workgroup turns the sums into exclusive prefixes
//                         (wfa_scan.h's scan_sums_kernel); the apply step is the consumer's.  No workgroup ever waits for another.
//   cov_offsets_kernel    apply for the tile counts: every tile's offset in the compact list.
//   cov_write_kernel      one workgroup per tile: the non-zero words as {pos, delta} in ascending pos, 16 bytes a store.
//   cov_import_kernel     one lane per entry of such a list: atomicAdd into another array (the merge of two devices' objects).
//   cov_intervals_kernel  apply for the deltas: entry i starts the interval of depth = inclusive prefix of delta; the interval that ENDS at
//                         entry i (from the entry before it, with the depth before it) goes into the totals {covered bases, sum of depth, max
//                         depth}, reduced per workgroup and added with integer atomics.  Dense depths never exist.
// Integer atomics only: they commute, so any order of adds gives the same array, and two calls give the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wfmash_hip.h"
#include "wfa_device.h"
#include "wfa_scan.h"

namespace wfm {
namespace {

constexpr int COV_THREADS = 256;
constexpr int COV_WAVES = COV_THREADS / 64;
static_assert(WFM_COV_TILE == COV_THREADS * 16, "a tile is four 16-byte loads per lane");
static_assert(WFM_COV_SCAN_BLOCK == COV_THREADS * 4, "a scan block is four elements per lane");

__global__ __launch_bounds__(COV_THREADS) void cov_add_kernel(const uint32_t* __restrict__ runs, const CovProb* __restrict__ probs,
                                                              int32_t* __restrict__ d, unsigned long long n_bases, uint32_t* __restrict__ flags) {
  const CovProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x;
  __shared__ unsigned long long wtot[COV_WAVES];
  __shared__ uint32_t s_bad;
  const uint32_t* my = runs + pr.runs_off;
  const uint32_t n = pr.n_runs;
  // the span first: nothing is written for a problem that would leave the array
  unsigned long long span;
  const bool empty_run = run_span<COV_WAVES, false>(my, n, wtot, &s_bad, &span, nullptr);
  const bool spans = empty_run || pr.base > n_bases || span > n_bases - pr.base;
  if (tid == 0) flags[blockIdx.x] = spans ? WFM_COV_SPANS : 0u;
  if (spans) return;
  unsigned long long carry = 0;
  for (uint32_t base = 0; base < n; base += COV_THREADS) {
    const uint32_t r = base + (uint32_t)tid;
    const bool valid = r < n;
    const uint32_t run = valid ? my[r] : 0u;
    const uint32_t len = WFM_RUN_LEN(run), op = WFM_RUN_OP(run);
    unsigned long long tp;
    const unsigned long long pp = pr.base + carry + block_excl<COV_WAVES>((valid && op != OP_I) ? len : 0u, wtot, &tp);
    carry += tp;
    if (!valid || op > OP_X) continue;
    // (pp + len <= pr.base + span <= n_bases, the array's last word)
    if (r == 0 || WFM_RUN_OP(my[r - 1]) > OP_X) atomicAdd(d + pp, 1);
    if (r + 1 == n || WFM_RUN_OP(my[r + 1]) > OP_X) atomicAdd(d + pp + len, -1);
  }
}

__device__ __forceinline__ uint32_t nonzero4(const uint4 v) { return (v.x != 0) + (v.y != 0) + (v.z != 0) + (v.w != 0); }

// d holds a whole number of tiles (the words behind n_bases are zero)
__global__ __launch_bounds__(COV_THREADS) void cov_count_kernel(const uint4* __restrict__ d, uint32_t* __restrict__ tile_cnt) {
  __shared__ unsigned long long wtot[COV_WAVES];
  const uint4* t = d + (size_t)blockIdx.x * (WFM_COV_TILE / 4);
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) c += nonzero4(t[k * COV_THREADS + threadIdx.x]);
  unsigned long long all;
  (void)block_excl<COV_WAVES>(c, wtot, &all);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (uint32_t)all;
}

// sums[b] = the sum of block b's elements: the tile counts, or (ENTRIES) the deltas of a compact list, sign-extended (sums wrap as two's complement)
template <bool ENTRIES>
__global__ __launch_bounds__(COV_THREADS) void cov_sum_kernel(const void* __restrict__ in, unsigned long long n, unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long wtot[COV_WAVES];
  const unsigned long long at = (unsigned long long)blockIdx.x * WFM_COV_SCAN_BLOCK + (unsigned long long)threadIdx.x * 4u;
  unsigned long long v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (at + k < n) v += ENTRIES ? (unsigned long long)(long long)(int32_t)((const uint4*)in)[at + k].z : (unsigned long long)((const uint32_t*)in)[at + k];
  unsigned long long all;
  (void)block_excl<COV_WAVES>(v, wtot, &all);
  if (threadIdx.x == 0) sums[blockIdx.x] = all;
}

// tile_off[t] = the number of non-zero words in the tiles before t; tile_off[ntiles] = all of them (by the block that holds the last tile)
__global__ __launch_bounds__(COV_THREADS) void cov_offsets_kernel(const uint32_t* __restrict__ tile_cnt, unsigned long long ntiles,
                                                                  const unsigned long long* __restrict__ sums, unsigned long long* __restrict__ tile_off) {
  __shared__ unsigned long long wtot[COV_WAVES];
  const unsigned long long at = (unsigned long long)blockIdx.x * WFM_COV_SCAN_BLOCK + (unsigned long long)threadIdx.x * 4u;
  uint32_t c[4];
  unsigned long long v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { c[k] = at + k < ntiles ? tile_cnt[at + k] : 0u; v += c[k]; }
  unsigned long long all;
  unsigned long long run = sums[blockIdx.x] + block_excl<COV_WAVES>(v, wtot, &all);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (at + k < ntiles) tile_off[at + k] = run;
    run += c[k];
    if (at + k + 1 == ntiles) tile_off[ntiles] = run;
  }
}

// the tiles from tile_a on, one per workgroup; out[0] is the entry number out_base of the whole list
__global__ __launch_bounds__(COV_THREADS) void cov_write_kernel(const uint4* __restrict__ d, const unsigned long long* __restrict__ tile_off,
                                                                unsigned long long tile_a, unsigned long long out_base, uint4* __restrict__ out) {
  __shared__ unsigned long long wtot[COV_WAVES];
  const unsigned long long tile = tile_a + blockIdx.x;
  if (tile_off[tile + 1] == tile_off[tile]) return;  // (the whole workgroup: an empty tile)
  const uint4* t = d + tile * (WFM_COV_TILE / 4);
  unsigned long long at = tile_off[tile] - out_base;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t q = (uint32_t)k * COV_THREADS + threadIdx.x;
    const uint4 v = t[q];
    unsigned long long all;
    unsigned long long o = at + block_excl<COV_WAVES>(nonzero4(v), wtot, &all);
    at += all;
    const unsigned long long pos = tile * WFM_COV_TILE + (unsigned long long)q * 4u;
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (w[j]) { out[o++] = make_uint4((uint32_t)(pos + j), (uint32_t)((pos + j) >> 32), w[j], 0u); }
  }
}

// (the host has checked every pos against n_bases)
__global__ __launch_bounds__(COV_THREADS) void cov_import_kernel(const uint4* __restrict__ ent, unsigned long long n, int32_t* __restrict__ d) {
  const unsigned long long i = (unsigned long long)blockIdx.x * COV_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint4 e = ent[i];
  atomicAdd(d + (((unsigned long long)e.y << 32) | e.x), (int32_t)e.z);
}

__device__ __forceinline__ unsigned long long pos_of(const uint4 e) { return ((unsigned long long)e.y << 32) | e.x; }

// ent: m entries of the list, in order; sums: the exclusive prefixes of the blocks' delta sums (the depth before the block); prev_pos: the
// pos of the entry before ent[0] (0 when there is none: the depth there is 0 as well); last: ent[m - 1] is the whole list's last entry
__global__ __launch_bounds__(COV_THREADS) void cov_intervals_kernel(const uint4* __restrict__ ent, unsigned long long m,
                                                                    const unsigned long long* __restrict__ sums, unsigned long long prev_pos,
                                                                    unsigned long long n_bases, int last, uint4* __restrict__ iv,
                                                                    unsigned long long* __restrict__ totals) {
  __shared__ unsigned long long wtot[COV_WAVES];
  const unsigned long long at = (unsigned long long)blockIdx.x * WFM_COV_SCAN_BLOCK + (unsigned long long)threadIdx.x * 4u;
  uint4 e[4];
  unsigned long long v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    e[k] = at + k < m ? ent[at + k] : make_uint4(0, 0, 0, 0);
    v += (unsigned long long)(long long)(int32_t)e[k].z;
  }
  unsigned long long all;
  long long depth = (long long)(sums[blockIdx.x] + block_excl<COV_WAVES>(v, wtot, &all));  // before entry `at`
  unsigned long long before = at == 0 ? prev_pos : (at - 1 < m ? pos_of(ent[at - 1]) : 0ull);
  unsigned long long covered = 0, sum = 0, top = 0;
  auto interval = [&](unsigned long long a, unsigned long long b, long long dep) {
    if (b <= a || dep <= 0) return;
    covered += b - a; sum += (b - a) * (unsigned long long)dep;
    if ((unsigned long long)dep > top) top = (unsigned long long)dep;
  };
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (at + k >= m) break;
    const unsigned long long pos = pos_of(e[k]);
    interval(before, pos, depth);
    depth += (long long)(int32_t)e[k].z;
    iv[at + k] = make_uint4(e[k].x, e[k].y, (uint32_t)depth, 0u);
    if (last && at + k + 1 == m) interval(pos, n_bases, depth);
    before = pos;
  }
  unsigned long long c_all, s_all;
  (void)block_excl<COV_WAVES>(covered, wtot, &c_all);
  (void)block_excl<COV_WAVES>(sum, wtot, &s_all);
  // the maximum over the workgroup: through the waves' words
  for (int dlt = 32; dlt > 0; dlt >>= 1) {
    const unsigned long long u = ((unsigned long long)__shfl_down((unsigned)(top >> 32), dlt, 64) << 32) | __shfl_down((unsigned)top, dlt, 64);
    if (u > top) top = u;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = top;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < COV_WAVES; ++w) if (wtot[w] > top) top = wtot[w];
    if (c_all) atomicAdd(totals + 0, c_all);
    if (s_all) atomicAdd(totals + 1, s_all);
    if (top) atomicMax(totals + 2, top);
  }
}

unsigned blocks_of(unsigned long long n, unsigned long long per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

void launch_cov_add(const uint32_t* runs, const CovProb* probs, int nprob, int32_t* d, unsigned long long n_bases, uint32_t* flags, hipStream_t st) {
  if (nprob <= 0) return;
  hipLaunchKernelGGL(cov_add_kernel, dim3((unsigned)nprob), dim3(COV_THREADS), 0, st, runs, probs, d, n_bases, flags);
}

void launch_cov_tile_offsets(const int32_t* d, unsigned long long ntiles, uint32_t* tile_cnt, unsigned long long* sums, unsigned long long* tile_off,
                             hipStream_t st) {
  const unsigned nb = blocks_of(ntiles, WFM_COV_SCAN_BLOCK);
  hipLaunchKernelGGL(cov_count_kernel, dim3((unsigned)ntiles), dim3(COV_THREADS), 0, st, (const uint4*)d, tile_cnt);
  hipLaunchKernelGGL(cov_sum_kernel<false>, dim3(nb), dim3(COV_THREADS), 0, st, (const void*)tile_cnt, ntiles, sums);
  hipLaunchKernelGGL((scan_sums_kernel<COV_WAVES, false, LoadWord>), dim3(1), dim3(COV_THREADS), 0, st, LoadWord{sums}, (unsigned long long)nb, sums,
                     (unsigned long long*)nullptr);
  hipLaunchKernelGGL(cov_offsets_kernel, dim3(nb), dim3(COV_THREADS), 0, st, (const uint32_t*)tile_cnt, ntiles, (const unsigned long long*)sums, tile_off);
}

void launch_cov_write(const int32_t* d, const unsigned long long* tile_off, unsigned long long tile_a, unsigned long long tile_b,
                      unsigned long long out_base, void* out, hipStream_t st) {
  if (tile_b <= tile_a) return;
  hipLaunchKernelGGL(cov_write_kernel, dim3((unsigned)(tile_b - tile_a)), dim3(COV_THREADS), 0, st, (const uint4*)d, tile_off, tile_a, out_base, (uint4*)out);
}

void launch_cov_import(const void* ent, unsigned long long n, int32_t* d, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(cov_import_kernel, dim3(blocks_of(n, COV_THREADS)), dim3(COV_THREADS), 0, st, (const uint4*)ent, n, d);
}

void launch_cov_intervals(const void* ent, unsigned long long m, unsigned long long* sums, unsigned long long* carry, unsigned long long prev_pos,
                          unsigned long long n_bases, int last, void* iv, unsigned long long* totals, hipStream_t st) {
  if (m == 0) return;
  const unsigned nb = blocks_of(m, WFM_COV_SCAN_BLOCK);
  hipLaunchKernelGGL(cov_sum_kernel<true>, dim3(nb), dim3(COV_THREADS), 0, st, ent, m, sums);
  // (the prefixes begin at *carry, the depth behind the chunks before, and *carry is brought up to date)
  hipLaunchKernelGGL((scan_sums_kernel<COV_WAVES, true, LoadWord>), dim3(1), dim3(COV_THREADS), 0, st, LoadWord{sums}, (unsigned long long)nb, sums, carry);
  hipLaunchKernelGGL(cov_intervals_kernel, dim3(nb), dim3(COV_THREADS), 0, st, (const uint4*)ent, m, (const unsigned long long*)sums, prev_pos, n_bases, last,
                     (uint4*)iv, totals);
}

}  // namespace wfm
