// wfa_scan.h -- what the kernels that index a problem's runs and deal output bytes to lanes share (wfa_cs.hip, wfa_variants.hip): the
// exclusive prefix over a workgroup and the binary search for the last element at or before a key.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

// the last i in [lo, hi) with le(i), where le(lo) holds and le is true on a prefix of the range
template <class Le>
__device__ __forceinline__ uint32_t last_le(uint32_t lo, uint32_t hi, Le le) {
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (le(mid)) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace wfm
