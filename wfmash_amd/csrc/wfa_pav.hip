// wfa_pav.hip -- the kernels behind wfm_pav_* (include/wfmash_hip.h): which groups of records cover which bases of the target, kept as a
// list of aligned SEGMENTS per group and never as a dense array.  Nothing but runs is read: no sequence bytes.  A segment is two 64-bit keys,
// ks = group << 40 | start and ke = group << 40 | end, in two arrays: what the sort and the binary searches take as they are.
//
//   pav_count_kernel      one workgroup per problem.  A first pass over the runs takes the pattern span and refuses the problem (an empty run,
//                         a span that leaves [0, n_bases] or does not fit 32 bits, a group that is not below n_groups) BEFORE anything is
//                         written; then the number of maximal stretches of =/X runs: the segments the problem will write.
//   pav_offsets_kernel    ONE workgroup: the counts to their exclusive prefixes over the problems (rounds of 256 with a carry).
//   pav_write_kernel      one workgroup per problem, rounds of 256 runs with three carries (cov_add_kernel's shape): the pattern advance and
//                         the slot by wfa_scan.h's block_excl, the start of the stretch a run lies in by a running maximum over the heads'
//                         positions (they ascend, so the maximum is the latest head, also across a round boundary).  The LAST run of a
//                         stretch writes the whole segment.  Slots come from scans, not atomics: two calls give the same list.
//   pav_block_max_kernel /  the inclusive running maximum of ke over the sorted list, in place, in the reduce / scan-of-maxima / apply form of
//   pav_scan_max_kernel /   wfa_lift.hip as three launches: per block of WFM_PAV_SCAN_BLOCK segments its maximum; ONE workgroup turns the
//   pav_apply_max_kernel    maxima into the maximum before each block; the apply step scans its block again.  A later group's keys are larger
//                           than every key of an earlier one, so the plain prefix maximum is a per-group one.
//   pav_block_sum_kernel /  the two sums (the head flags of the union; the lengths of its intervals) in the same form: per block its sum, ONE
//   pav_scan_sums_kernel    workgroup for the exclusive prefixes of the sums, the apply step the consumer's:
//   pav_compact_kernel      segment i heads a union interval iff i == 0 or ks[i] > rm[i - 1] (abutting segments merge); the head writes the
//                           interval's start key at its rank, the interval's last member (i + 1 == n or i + 1 a head) the end key rm[i].
//   pav_prefix_kernel       C[i] = the bases of the union intervals before i, C[m] = all of them, 64 bits.
//   pav_matrix_kernel       one thread per (interval, group) cell: two binary searches over the union's keys and three words of C and the
//                           keys; O(log m) a cell, never a walk.
// No workgroup ever waits for another.  The sort is rocprim::radix_sort_pairs (pav_sort), as map_finish.hip's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include <rocprim/rocprim.hpp>

#include "../../include/wfmash_hip.h"
#include "wfa_device.h"
#include "wfa_scan.h"

namespace wfm {
namespace {

constexpr int PAV_THREADS = 256;
constexpr int PAV_WAVES = PAV_THREADS / 64;
constexpr unsigned PAV_SHIFT = 40;
static_assert(WFM_PAV_SCAN_BLOCK == PAV_THREADS * 4, "a scan block is four segments per lane");

// inclusive running maximum of v over the workgroup's threads (in thread order) and the maximum of all; wmax: PAV_WAVES words of LDS
__device__ __forceinline__ unsigned long long pav_incl_max(unsigned long long v, unsigned long long* wmax, unsigned long long* all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long u = scan_shfl_up64(incl, d);
    if (lane >= d && u > incl) incl = u;
  }
  __syncthreads();  // (the words may still be read from the scan before)
  if (lane == 63) wmax[wave] = incl;
  __syncthreads();
  unsigned long long top = 0;
#pragma unroll
  for (int w = 0; w < PAV_WAVES; ++w) {
    if (w < wave && wmax[w] > incl) incl = wmax[w];
    if (wmax[w] > top) top = wmax[w];
  }
  *all = top;
  return incl;
}

__global__ __launch_bounds__(PAV_THREADS) void pav_count_kernel(const uint32_t* __restrict__ runs, const PavProb* __restrict__ probs,
                                                                unsigned long long n_bases, uint32_t n_groups, uint32_t* __restrict__ flags,
                                                                unsigned long long* __restrict__ cnt) {
  const PavProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x;
  __shared__ unsigned long long wtot[PAV_WAVES];
  __shared__ uint32_t s_bad;
  if (tid == 0) s_bad = 0;
  const uint32_t* my = runs + pr.runs_off;
  const uint32_t n = pr.n_runs;
  // the span first: a problem that is refused writes nothing
  unsigned long long mine = 0;
  bool bad = false;
  for (uint32_t r = (uint32_t)tid; r < n; r += PAV_THREADS) {
    const uint32_t run = my[r];
    if (WFM_RUN_LEN(run) == 0) bad = true;
    if (WFM_RUN_OP(run) != OP_I) mine += WFM_RUN_LEN(run);
  }
  unsigned long long span;
  (void)block_excl<PAV_WAVES>(mine, wtot, &span);
  if (bad) s_bad = 1;  // (every writer stores the same value)
  __syncthreads();
  const bool spans = s_bad || pr.group >= n_groups || pr.base > n_bases || span > n_bases - pr.base || span > 0xffffffffull;
  if (spans) {
    if (tid == 0) { flags[blockIdx.x] = WFM_PAV_SPANS; cnt[blockIdx.x] = 0; }
    return;
  }
  unsigned long long c = 0;
  for (uint32_t r = (uint32_t)tid; r < n; r += PAV_THREADS)
    c += WFM_RUN_OP(my[r]) <= OP_X && (r + 1 == n || WFM_RUN_OP(my[r + 1]) > OP_X);
  unsigned long long all;
  (void)block_excl<PAV_WAVES>(c, wtot, &all);
  if (tid == 0) { flags[blockIdx.x] = 0; cnt[blockIdx.x] = all; }
}

// ONE workgroup: off[i] = the segments of the problems before i, off[n] = all of them
__global__ __launch_bounds__(PAV_THREADS) void pav_offsets_kernel(const unsigned long long* __restrict__ cnt, unsigned long long n,
                                                                  unsigned long long* __restrict__ off) {
  __shared__ unsigned long long wtot[PAV_WAVES];
  unsigned long long run = 0;
  for (unsigned long long base = 0; base < n; base += PAV_THREADS) {
    const unsigned long long i = base + threadIdx.x;
    const unsigned long long v = i < n ? cnt[i] : 0ull;
    unsigned long long all;
    const unsigned long long ex = block_excl<PAV_WAVES>(v, wtot, &all);
    if (i < n) off[i] = run + ex;
    run += all;
  }
  if (threadIdx.x == 0) off[n] = run;
}

__global__ __launch_bounds__(PAV_THREADS) void pav_write_kernel(const uint32_t* __restrict__ runs, const PavProb* __restrict__ probs,
                                                                const uint32_t* __restrict__ flags, const unsigned long long* __restrict__ off,
                                                                unsigned long long* __restrict__ ks, unsigned long long* __restrict__ ke) {
  if (flags[blockIdx.x]) return;  // (the whole workgroup)
  const PavProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x;
  __shared__ unsigned long long wtot[PAV_WAVES];
  __shared__ unsigned long long wmax[PAV_WAVES];
  const uint32_t* my = runs + pr.runs_off;
  const uint32_t n = pr.n_runs;
  const unsigned long long g = (unsigned long long)pr.group << PAV_SHIFT;
  unsigned long long carry_p = 0, carry_s = off[blockIdx.x], carry_h = 0;
  for (uint32_t base = 0; base < n; base += PAV_THREADS) {
    const uint32_t r = base + (uint32_t)tid;
    const bool valid = r < n;
    const uint32_t run = valid ? my[r] : 0u;
    const uint32_t len = WFM_RUN_LEN(run), op = WFM_RUN_OP(run);
    const bool aligned = valid && op <= OP_X;
    const bool head = aligned && (r == 0 || WFM_RUN_OP(my[r - 1]) > OP_X);
    const bool tail = aligned && (r + 1 == n || WFM_RUN_OP(my[r + 1]) > OP_X);
    unsigned long long tp, ts, th;
    const unsigned long long pp = pr.base + carry_p + block_excl<PAV_WAVES>((valid && op != OP_I) ? len : 0u, wtot, &tp);
    const unsigned long long slot = carry_s + block_excl<PAV_WAVES>(tail ? 1u : 0u, wtot, &ts);
    // the start of the stretch this run lies in, + 1: the heads' positions ascend, so the latest head is the largest
    unsigned long long h1 = pav_incl_max(head ? pp + 1 : 0ull, wmax, &th);
    if (carry_h > h1) h1 = carry_h;
    carry_p += tp; carry_s += ts;
    if (th > carry_h) carry_h = th;
    // (slot < off[blockIdx.x + 1]: pav_count_kernel counted the same tails; pp + len <= base + span <= n_bases < 2^40)
    if (tail) { ks[slot] = g | (h1 - 1); ke[slot] = g | (pp + len); }
  }
}

// maxs[b] = the largest end key of block b
__global__ __launch_bounds__(PAV_THREADS) void pav_block_max_kernel(const unsigned long long* __restrict__ ke, unsigned long long n,
                                                                    unsigned long long* __restrict__ maxs) {
  __shared__ unsigned long long wmax[PAV_WAVES];
  const unsigned long long at = (unsigned long long)blockIdx.x * WFM_PAV_SCAN_BLOCK + (unsigned long long)threadIdx.x * 4u;
  unsigned long long v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (at + k < n && ke[at + k] > v) v = ke[at + k];
  unsigned long long all;
  (void)pav_incl_max(v, wmax, &all);
  if (threadIdx.x == 0) maxs[blockIdx.x] = all;
}

// ONE workgroup: maxs[0 .. nb) to the maximum of the blocks BEFORE each (0 before the first: every end key is 1 at least)
__global__ __launch_bounds__(PAV_THREADS) void pav_scan_max_kernel(unsigned long long* __restrict__ maxs, unsigned long long nb) {
  __shared__ unsigned long long wmax[PAV_WAVES];
  __shared__ unsigned long long prev[PAV_THREADS];
  unsigned long long run = 0;
  for (unsigned long long base = 0; base < nb; base += PAV_THREADS) {
    const unsigned long long i = base + threadIdx.x;
    const unsigned long long v = i < nb ? maxs[i] : 0ull;
    unsigned long long all;
    const unsigned long long incl = pav_incl_max(v, wmax, &all);
    __syncthreads();  // (prev may still be read from the round before)
    prev[threadIdx.x] = incl;
    __syncthreads();
    const unsigned long long before = threadIdx.x ? prev[threadIdx.x - 1] : 0ull;
    if (i < nb) maxs[i] = run > before ? run : before;
    if (all > run) run = all;
  }
}

// apply, in place: ke[i] = max(the maximum before the block, the end keys of the block up to i)
__global__ __launch_bounds__(PAV_THREADS) void pav_apply_max_kernel(unsigned long long* __restrict__ ke, unsigned long long n,
                                                                    const unsigned long long* __restrict__ maxs) {
  __shared__ unsigned long long wmax[PAV_WAVES];
  __shared__ unsigned long long prev[PAV_THREADS];
  const unsigned long long at = (unsigned long long)blockIdx.x * WFM_PAV_SCAN_BLOCK + (unsigned long long)threadIdx.x * 4u;
  unsigned long long e[4], v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { e[k] = at + k < n ? ke[at + k] : 0ull; if (e[k] > v) v = e[k]; }
  unsigned long long all;
  const unsigned long long incl = pav_incl_max(v, wmax, &all);
  prev[threadIdx.x] = incl;
  __syncthreads();
  unsigned long long run = maxs[blockIdx.x];
  if (threadIdx.x && prev[threadIdx.x - 1] > run) run = prev[threadIdx.x - 1];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (e[k] > run) run = e[k];
    if (at + k < n) ke[at + k] = run;  // (a lane writes the words it read alone)
  }
}

// what the two sums add up per element: a = ks, b = rm (HEADS: 1 where segment i heads a union interval) or a = uks, b = uke (the length)
template <bool HEADS>
__device__ __forceinline__ unsigned long long pav_term(const unsigned long long* __restrict__ a, const unsigned long long* __restrict__ b, unsigned long long i) {
  if (HEADS) return (i == 0 || a[i] > b[i - 1]) ? 1ull : 0ull;
  return b[i] - a[i];
}

template <bool HEADS>
__global__ __launch_bounds__(PAV_THREADS) void pav_block_sum_kernel(const unsigned long long* __restrict__ a, const unsigned long long* __restrict__ b,
                                                                    unsigned long long n, unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long wtot[PAV_WAVES];
  const unsigned long long at = (unsigned long long)blockIdx.x * WFM_PAV_SCAN_BLOCK + (unsigned long long)threadIdx.x * 4u;
  unsigned long long v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (at + k < n) v += pav_term<HEADS>(a, b, at + k);
  unsigned long long all;
  (void)block_excl<PAV_WAVES>(v, wtot, &all);
  if (threadIdx.x == 0) sums[blockIdx.x] = all;
}

// ONE workgroup: sums[0 .. nb) to their exclusive prefixes, sums[nb] = the total
__global__ __launch_bounds__(PAV_THREADS) void pav_scan_sums_kernel(unsigned long long* __restrict__ sums, unsigned long long nb) {
  __shared__ unsigned long long wtot[PAV_WAVES];
  unsigned long long run = 0;
  for (unsigned long long base = 0; base < nb; base += PAV_THREADS) {
    const unsigned long long i = base + threadIdx.x;
    const unsigned long long v = i < nb ? sums[i] : 0ull;
    unsigned long long all;
    const unsigned long long ex = block_excl<PAV_WAVES>(v, wtot, &all);
    if (i < nb) sums[i] = run + ex;
    run += all;
  }
  if (threadIdx.x == 0) sums[nb] = run;
}

__global__ __launch_bounds__(PAV_THREADS) void pav_compact_kernel(const unsigned long long* __restrict__ ks, const unsigned long long* __restrict__ rm,
                                                                  unsigned long long n, const unsigned long long* __restrict__ sums,
                                                                  unsigned long long* __restrict__ uks, unsigned long long* __restrict__ uke) {
  __shared__ unsigned long long wtot[PAV_WAVES];
  const unsigned long long at = (unsigned long long)blockIdx.x * WFM_PAV_SCAN_BLOCK + (unsigned long long)threadIdx.x * 4u;
  unsigned long long f[4], v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { f[k] = at + k < n ? pav_term<true>(ks, rm, at + k) : 0ull; v += f[k]; }
  unsigned long long all;
  unsigned long long rank = sums[blockIdx.x] + block_excl<PAV_WAVES>(v, wtot, &all);  // the heads before this lane's first segment
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long i = at + k;
    if (i >= n) break;
    if (f[k]) uks[rank] = ks[i];
    rank += f[k];
    // (segment 0 is a head, so rank >= 1 here; rank <= the total the caller made room for)
    if (i + 1 == n || ks[i + 1] > rm[i]) uke[rank - 1] = rm[i];
  }
}

__global__ __launch_bounds__(PAV_THREADS) void pav_prefix_kernel(const unsigned long long* __restrict__ uks, const unsigned long long* __restrict__ uke,
                                                                 unsigned long long m, const unsigned long long* __restrict__ sums,
                                                                 unsigned long long* __restrict__ C) {
  __shared__ unsigned long long wtot[PAV_WAVES];
  const unsigned long long at = (unsigned long long)blockIdx.x * WFM_PAV_SCAN_BLOCK + (unsigned long long)threadIdx.x * 4u;
  unsigned long long l[4], v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { l[k] = at + k < m ? pav_term<false>(uks, uke, at + k) : 0ull; v += l[k]; }
  unsigned long long all;
  unsigned long long run = sums[blockIdx.x] + block_excl<PAV_WAVES>(v, wtot, &all);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long i = at + k;
    if (i >= m) break;
    C[i] = run;
    run += l[k];
    if (i + 1 == m) C[m] = run;
  }
}

// the first i in [0, n) with gt(i), or n; gt is false on a prefix of the range and true behind it
template <class Gt>
__device__ __forceinline__ unsigned long long pav_first_true(unsigned long long n, Gt gt) {
  unsigned long long lo = 0, hi = n;
  while (lo < hi) {
    const unsigned long long mid = lo + (hi - lo) / 2;
    if (gt(mid)) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(PAV_THREADS) void pav_matrix_kernel(const unsigned long long* __restrict__ uks, const unsigned long long* __restrict__ uke,
                                                                 const unsigned long long* __restrict__ C, unsigned long long m,
                                                                 const ulonglong2* __restrict__ iv, unsigned long long ra, unsigned long long cells,
                                                                 uint32_t n_groups, uint32_t* __restrict__ out) {
  const unsigned long long cell = (unsigned long long)blockIdx.x * PAV_THREADS + threadIdx.x;
  if (cell >= cells) return;
  const unsigned long long j = ra + cell / n_groups, g = (cell % n_groups) << PAV_SHIFT;
  const ulonglong2 v = iv[j];
  const unsigned long long a = g | v.x, b = g | v.y;
  const unsigned long long lo = pav_first_true(m, [&](unsigned long long u) { return uke[u] > a; });
  const unsigned long long hi = pav_first_true(m, [&](unsigned long long u) { return uks[u] >= b; });
  unsigned long long c = 0;
  if (hi > lo) {  // (then intervals lo .. hi - 1 are this group's: end key > a and start key < b)
    c = C[hi] - C[lo];
    const unsigned long long s = uks[lo], e = uke[hi - 1];
    if (s < a) c -= a - s;
    if (e > b) c -= e - b;
  }
  out[cell] = (uint32_t)c;  // (at most the interval's length, which the caller has checked to fit)
}

unsigned blocks_of(unsigned long long n, unsigned long long per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

void launch_pav_count(const uint32_t* runs, const PavProb* probs, int nprob, unsigned long long n_bases, uint32_t n_groups, uint32_t* flags,
                      unsigned long long* cnt, unsigned long long* off, hipStream_t st) {
  if (nprob <= 0) return;
  hipLaunchKernelGGL(pav_count_kernel, dim3((unsigned)nprob), dim3(PAV_THREADS), 0, st, runs, probs, n_bases, n_groups, flags, cnt);
  hipLaunchKernelGGL(pav_offsets_kernel, dim3(1), dim3(PAV_THREADS), 0, st, (const unsigned long long*)cnt, (unsigned long long)nprob, off);
}

void launch_pav_write(const uint32_t* runs, const PavProb* probs, int nprob, const uint32_t* flags, const unsigned long long* off,
                      unsigned long long* ks, unsigned long long* ke, hipStream_t st) {
  if (nprob <= 0) return;
  hipLaunchKernelGGL(pav_write_kernel, dim3((unsigned)nprob), dim3(PAV_THREADS), 0, st, runs, probs, flags, off, ks, ke);
}

hipError_t pav_sort(void* tmp, size_t* tmp_bytes, const unsigned long long* ks, unsigned long long* ks2, const unsigned long long* ke,
                    unsigned long long* ke2, unsigned long long n, unsigned end_bit, hipStream_t st) {
  return rocprim::radix_sort_pairs(tmp, *tmp_bytes, ks, ks2, ke, ke2, (size_t)n, 0u, end_bit, st);
}

void launch_pav_runmax(unsigned long long* ke, unsigned long long n, unsigned long long* aux, hipStream_t st) {
  if (n == 0) return;
  const unsigned nb = blocks_of(n, WFM_PAV_SCAN_BLOCK);
  hipLaunchKernelGGL(pav_block_max_kernel, dim3(nb), dim3(PAV_THREADS), 0, st, (const unsigned long long*)ke, n, aux);
  hipLaunchKernelGGL(pav_scan_max_kernel, dim3(1), dim3(PAV_THREADS), 0, st, aux, (unsigned long long)nb);
  hipLaunchKernelGGL(pav_apply_max_kernel, dim3(nb), dim3(PAV_THREADS), 0, st, ke, n, (const unsigned long long*)aux);
}

void launch_pav_compact(const unsigned long long* ks, const unsigned long long* rm, unsigned long long n, unsigned long long* aux,
                        unsigned long long* uks, unsigned long long* uke, hipStream_t st) {
  if (n == 0) return;
  const unsigned nb = blocks_of(n, WFM_PAV_SCAN_BLOCK);
  hipLaunchKernelGGL(pav_block_sum_kernel<true>, dim3(nb), dim3(PAV_THREADS), 0, st, ks, rm, n, aux);
  hipLaunchKernelGGL(pav_scan_sums_kernel, dim3(1), dim3(PAV_THREADS), 0, st, aux, (unsigned long long)nb);
  hipLaunchKernelGGL(pav_compact_kernel, dim3(nb), dim3(PAV_THREADS), 0, st, ks, rm, n, (const unsigned long long*)aux, uks, uke);
}

void launch_pav_prefix(const unsigned long long* uks, const unsigned long long* uke, unsigned long long m, unsigned long long* aux,
                       unsigned long long* C, hipStream_t st) {
  if (m == 0) return;
  const unsigned nb = blocks_of(m, WFM_PAV_SCAN_BLOCK);
  hipLaunchKernelGGL(pav_block_sum_kernel<false>, dim3(nb), dim3(PAV_THREADS), 0, st, uks, uke, m, aux);
  hipLaunchKernelGGL(pav_scan_sums_kernel, dim3(1), dim3(PAV_THREADS), 0, st, aux, (unsigned long long)nb);
  hipLaunchKernelGGL(pav_prefix_kernel, dim3(nb), dim3(PAV_THREADS), 0, st, uks, uke, m, (const unsigned long long*)aux, C);
}

void launch_pav_matrix(const unsigned long long* uks, const unsigned long long* uke, const unsigned long long* C, unsigned long long m, const void* iv,
                       unsigned long long ra, unsigned long long rb, uint32_t n_groups, uint32_t* out, hipStream_t st) {
  if (rb <= ra || n_groups == 0) return;
  const unsigned long long cells = (rb - ra) * n_groups;
  hipLaunchKernelGGL(pav_matrix_kernel, dim3(blocks_of(cells, PAV_THREADS)), dim3(PAV_THREADS), 0, st, uks, uke, C, m, (const ulonglong2*)iv, ra, cells,
                     n_groups, out);
}

}  // namespace wfm
