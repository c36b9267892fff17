// wfa_scan.h -- what the kernels of the record passes share (wfa_cs.hip, wfa_variants.hip, wfa_coverage.hip, wfa_lift.hip, wfa_chain.hip, wfa_pav.hip, wfa_maf.hip):
// the exclusive prefix and the inclusive running maximum over a workgroup, the two binary searches, the first pass over a problem's runs,
// and the device-wide scans in the reduce / one-workgroup scan / apply form as templates (the scan of the blocks' sums; the running maximum
// in three launches).  A workgroup is WAVES x 64 threads; a scan block is four elements per lane.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wfmash_hip.h"
#include "wfa_device.h"

namespace wfm {

__device__ __forceinline__ unsigned long long scan_shfl_up64(unsigned long long v, int d) {
  const unsigned lo = __shfl_up((unsigned)v, d, 64), hi = __shfl_up((unsigned)(v >> 32), d, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// exclusive prefix of v over the workgroup's WAVES x 64 threads (in thread order) and the total; wtot: WAVES words of LDS.  Two barriers.
template <int WAVES>
__device__ __forceinline__ unsigned long long block_excl(unsigned long long v, unsigned long long* wtot, unsigned long long* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long u = scan_shfl_up64(incl, d);
    if (lane >= d) incl += u;
  }
  __syncthreads();  // (the words may still be read from the scan before)
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  unsigned long long before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) { if (w < wave) before += wtot[w]; all += wtot[w]; }
  *total = all;
  return before + incl - v;
}

// inclusive running maximum of v over the workgroup's WAVES x 64 threads (in thread order) and the maximum of all; wmax: WAVES words of
// LDS.  Two barriers.
template <int WAVES>
__device__ __forceinline__ unsigned long long block_incl_max(unsigned long long v, unsigned long long* wmax, unsigned long long* all) {
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
  for (int w = 0; w < WAVES; ++w) {
    if (w < wave && wmax[w] > incl) incl = wmax[w];
    if (wmax[w] > top) top = wmax[w];
  }
  *all = top;
  return incl;
}

// the last i in [lo, hi) with le(i), where le(lo) holds and le is true on a prefix of the range
template <class Le>
__device__ __forceinline__ uint32_t last_le(uint32_t lo, uint32_t hi, Le le) {
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (le(mid)) lo = mid; else hi = mid;
  }
  return lo;
}

// the first i in [0, n) with gt(i), or n; gt is false on a prefix of the range and true behind it
template <class Gt>
__device__ __forceinline__ unsigned long long first_true(unsigned long long n, Gt gt) {
  unsigned long long lo = 0, hi = n;
  while (lo < hi) {
    const unsigned long long mid = lo + (hi - lo) / 2;
    if (gt(mid)) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// The first pass over a problem's n runs, by the whole workgroup, BEFORE anything is written for the problem: *span = the bases of the
// pattern the runs cover, *tspan (TEXT) those of the text; returns "some run is empty".  The caller refuses the problem on that and on
// what it asks of the spans.  wtot: WAVES words of LDS; s_bad: one.
template <int WAVES, bool TEXT>
__device__ __forceinline__ bool run_span(const uint32_t* __restrict__ my, uint32_t n, unsigned long long* wtot, uint32_t* s_bad,
                                         unsigned long long* span, unsigned long long* tspan) {
  if (threadIdx.x == 0) *s_bad = 0;
  unsigned long long mine_p = 0, mine_t = 0;
  bool bad = false;
  for (uint32_t r = threadIdx.x; r < n; r += WAVES * 64) {
    const uint32_t run = my[r];
    if (WFM_RUN_LEN(run) == 0) bad = true;
    if (WFM_RUN_OP(run) != OP_I) mine_p += WFM_RUN_LEN(run);
    if (TEXT && WFM_RUN_OP(run) != OP_D) mine_t += WFM_RUN_LEN(run);
  }
  (void)block_excl<WAVES>(mine_p, wtot, span);
  if (TEXT) (void)block_excl<WAVES>(mine_t, wtot, tspan);
  if (bad) *s_bad = 1;  // (every writer stores the same value; the zero was stored before block_excl's barriers)
  __syncthreads();
  return *s_bad != 0;
}

// how an element of a scan is loaded: a 64-bit word of an array, the end of an interval {start, end}, the count of a LiftWin
struct LoadWord { const unsigned long long* p; __device__ __forceinline__ unsigned long long operator()(unsigned long long i) const { return p[i]; } };
struct LoadEnd { const ulonglong2* p; __device__ __forceinline__ unsigned long long operator()(unsigned long long i) const { return p[i].y; } };
struct LoadWinCount { const LiftWin* p; __device__ __forceinline__ unsigned long long operator()(unsigned long long i) const { return p[i].count; } };

// ONE workgroup: out[i] = the sum of the n elements before i (rounds of WAVES x 64 with a carry), out[n] = the total.  out may be the array
// the elements are loaded from.  CARRY: the prefixes begin at *carry, and *carry = the total too.
template <int WAVES, bool CARRY, class Load>
__global__ __launch_bounds__(WAVES * 64) void scan_sums_kernel(Load in, unsigned long long n, unsigned long long* out, unsigned long long* carry) {
  __shared__ unsigned long long wtot[WAVES];
  unsigned long long run = 0;
  if (CARRY) {
    run = *carry;
    __syncthreads();  // (thread 0 writes *carry at the end)
  }
  for (unsigned long long base = 0; base < n; base += WAVES * 64) {
    const unsigned long long i = base + threadIdx.x;
    const unsigned long long v = i < n ? in(i) : 0ull;
    unsigned long long all;
    const unsigned long long ex = block_excl<WAVES>(v, wtot, &all);
    if (i < n) out[i] = run + ex;
    run += all;
  }
  if (threadIdx.x == 0) { out[n] = run; if (CARRY) *carry = run; }
}

// The inclusive running maximum of n keys, out[i] = max(key(0) .. key(i)), in three launches: per scan block its maximum; ONE workgroup
// turns the maxima into the maximum BEFORE each block (0 before the first: every key is 1 at least); the apply step scans its block again.
// No workgroup ever waits for another.  out may be the array the keys are loaded from (a lane writes the words it read alone).
template <int WAVES, class Key>
__global__ __launch_bounds__(WAVES * 64) void runmax_block_kernel(Key key, unsigned long long n, unsigned long long* __restrict__ maxs) {
  __shared__ unsigned long long wmax[WAVES];
  const unsigned long long at = (unsigned long long)blockIdx.x * (WAVES * 256) + (unsigned long long)threadIdx.x * 4u;
  unsigned long long v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (at + k < n && key(at + k) > v) v = key(at + k);
  unsigned long long all;
  (void)block_incl_max<WAVES>(v, wmax, &all);
  if (threadIdx.x == 0) maxs[blockIdx.x] = all;
}

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void runmax_scan_kernel(unsigned long long* __restrict__ maxs, unsigned long long nb) {
  __shared__ unsigned long long wmax[WAVES];
  __shared__ unsigned long long prev[WAVES * 64];
  unsigned long long run = 0;
  for (unsigned long long base = 0; base < nb; base += WAVES * 64) {
    const unsigned long long i = base + threadIdx.x;
    const unsigned long long v = i < nb ? maxs[i] : 0ull;
    unsigned long long all;
    const unsigned long long incl = block_incl_max<WAVES>(v, wmax, &all);
    __syncthreads();  // (prev may still be read from the round before)
    prev[threadIdx.x] = incl;
    __syncthreads();
    const unsigned long long before = threadIdx.x ? prev[threadIdx.x - 1] : 0ull;
    if (i < nb) maxs[i] = run > before ? run : before;
    if (all > run) run = all;
  }
}

template <int WAVES, class Key>
__global__ __launch_bounds__(WAVES * 64) void runmax_apply_kernel(Key key, unsigned long long n, const unsigned long long* __restrict__ maxs,
                                                                  unsigned long long* out) {
  __shared__ unsigned long long wmax[WAVES];
  __shared__ unsigned long long prev[WAVES * 64];
  const unsigned long long at = (unsigned long long)blockIdx.x * (WAVES * 256) + (unsigned long long)threadIdx.x * 4u;
  unsigned long long e[4], v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { e[k] = at + k < n ? key(at + k) : 0ull; if (e[k] > v) v = e[k]; }
  unsigned long long all;
  const unsigned long long incl = block_incl_max<WAVES>(v, wmax, &all);
  prev[threadIdx.x] = incl;
  __syncthreads();
  unsigned long long run = maxs[blockIdx.x];
  if (threadIdx.x && prev[threadIdx.x - 1] > run) run = prev[threadIdx.x - 1];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (e[k] > run) run = e[k];
    if (at + k < n) out[at + k] = run;
  }
}

// maxs: n / (WAVES x 256) rounded up
template <int WAVES, class Key>
void launch_runmax(Key key, unsigned long long n, unsigned long long* maxs, unsigned long long* out, hipStream_t st) {
  if (n == 0) return;
  const unsigned nb = (unsigned)((n + WAVES * 256 - 1) / (WAVES * 256));
  hipLaunchKernelGGL((runmax_block_kernel<WAVES, Key>), dim3(nb), dim3(WAVES * 64), 0, st, key, n, maxs);
  hipLaunchKernelGGL((runmax_scan_kernel<WAVES>), dim3(1), dim3(WAVES * 64), 0, st, maxs, (unsigned long long)nb);
  hipLaunchKernelGGL((runmax_apply_kernel<WAVES, Key>), dim3(nb), dim3(WAVES * 64), 0, st, key, n, (const unsigned long long*)maxs, out);
}

}  // namespace wfm
