// wfa_pav.hip -- the kernels behind wfm_pav_* (include/wfmash_hip.h): which groups of records cover which bases of the target, kept as a
// list of aligned SEGMENTS per group and never as a dense array.  Nothing but runs is read: no sequence bytes.  A segment is two 64-bit keys,
// ks = group << 40 | start and ke = group << 40 | end, in two arrays: what the sort and the binary searches take as they are.
//
//   pav_count_kernel      one workgroup per problem.  wfa_scan.h's run_span takes the pattern span; the problem is refused (an empty run,
//                         a span that leaves [0, n_bases] or does not fit 32 bits, a group that is not below n_groups) BEFORE anything is
//                         written; then the number of maximal stretches of =/X runs: the segments the problem will write.  (EQ: of = runs
//                         alone, which is what wfm_sites_add_ref keeps; the write kernel likewise.)
//   scan_sums_kernel      (wfa_scan.h) ONE workgroup: the counts to their exclusive prefixes over the problems; the blocks' sums likewise.
//   pav_write_kernel      one workgroup per problem, rounds of 256 runs with three carries (cov_add_kernel's shape): the pattern advance and
//                         the slot by wfa_scan.h's block_excl, the start of the stretch a run lies in by a running maximum over the heads'
//                         positions (they ascend, so the maximum is the latest head, also across a round boundary).  The LAST run of a
//                         stretch writes the whole segment.  Slots come from scans, not atomics: two calls give the same list.
//   launch_runmax           (wfa_scan.h) the inclusive running maximum of ke over the sorted list, in place, per block of WFM_PAV_SCAN_BLOCK
//                           segments.  A later group's keys are larger than every key of an earlier one, so the plain prefix maximum is a
//                           per-group one.
//   pav_block_sum_kernel    the two sums (the head flags of the union; the lengths of its intervals) in the same form: per block its sum, ONE
//                           workgroup for the exclusive prefixes of the sums (scan_sums_kernel), the apply step the consumer's:
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

// what a segment is made of: =/X runs (wfm_pav_add) or, EQ, = runs alone (wfm_sites_add_ref)
template <bool EQ>
__device__ __forceinline__ bool pav_in(uint32_t op) { return EQ ? op == OP_M : op <= OP_X; }

template <bool EQ>
__global__ __launch_bounds__(PAV_THREADS) void pav_count_kernel(const uint32_t* __restrict__ runs, const PavProb* __restrict__ probs,
                                                                unsigned long long n_bases, uint32_t n_groups, uint32_t* __restrict__ flags,
                                                                unsigned long long* __restrict__ cnt) {
  const PavProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x;
  __shared__ unsigned long long wtot[PAV_WAVES];
  __shared__ uint32_t s_bad;
  const uint32_t* my = runs + pr.runs_off;
  const uint32_t n = pr.n_runs;
  // the span first: a problem that is refused writes nothing
  unsigned long long span;
  const bool empty_run = run_span<PAV_WAVES, false>(my, n, wtot, &s_bad, &span, nullptr);
  const bool spans = empty_run || pr.group >= n_groups || pr.base > n_bases || span > n_bases - pr.base || span > 0xffffffffull;
  if (spans) {
    if (tid == 0) { flags[blockIdx.x] = WFM_PAV_SPANS; cnt[blockIdx.x] = 0; }
    return;
  }
  unsigned long long c = 0;
  for (uint32_t r = (uint32_t)tid; r < n; r += PAV_THREADS)
    c += pav_in<EQ>(WFM_RUN_OP(my[r])) && (r + 1 == n || !pav_in<EQ>(WFM_RUN_OP(my[r + 1])));
  unsigned long long all;
  (void)block_excl<PAV_WAVES>(c, wtot, &all);
  if (tid == 0) { flags[blockIdx.x] = 0; cnt[blockIdx.x] = all; }
}

template <bool EQ>
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
    const bool aligned = valid && pav_in<EQ>(op);
    const bool head = aligned && (r == 0 || !pav_in<EQ>(WFM_RUN_OP(my[r - 1])));
    const bool tail = aligned && (r + 1 == n || !pav_in<EQ>(WFM_RUN_OP(my[r + 1])));
    unsigned long long tp, ts, th;
    const unsigned long long pp = pr.base + carry_p + block_excl<PAV_WAVES>((valid && op != OP_I) ? len : 0u, wtot, &tp);
    const unsigned long long slot = carry_s + block_excl<PAV_WAVES>(tail ? 1u : 0u, wtot, &ts);
    // the start of the stretch this run lies in, + 1: the heads' positions ascend, so the latest head is the largest
    unsigned long long h1 = block_incl_max<PAV_WAVES>(head ? pp + 1 : 0ull, wmax, &th);
    if (carry_h > h1) h1 = carry_h;
    carry_p += tp; carry_s += ts;
    if (th > carry_h) carry_h = th;
    // (slot < off[blockIdx.x + 1]: pav_count_kernel counted the same tails; pp + len <= base + span <= n_bases < 2^40)
    if (tail) { ks[slot] = g | (h1 - 1); ke[slot] = g | (pp + len); }
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

__global__ __launch_bounds__(PAV_THREADS) void pav_matrix_kernel(const unsigned long long* __restrict__ uks, const unsigned long long* __restrict__ uke,
                                                                 const unsigned long long* __restrict__ C, unsigned long long m,
                                                                 const ulonglong2* __restrict__ iv, unsigned long long ra, unsigned long long cells,
                                                                 uint32_t n_groups, uint32_t* __restrict__ out) {
  const unsigned long long cell = (unsigned long long)blockIdx.x * PAV_THREADS + threadIdx.x;
  if (cell >= cells) return;
  const unsigned long long j = ra + cell / n_groups, g = (cell % n_groups) << PAV_SHIFT;
  const ulonglong2 v = iv[j];
  const unsigned long long a = g | v.x, b = g | v.y;
  const unsigned long long lo = first_true(m, [&](unsigned long long u) { return uke[u] > a; });
  const unsigned long long hi = first_true(m, [&](unsigned long long u) { return uks[u] >= b; });
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

// ONE workgroup: words[0 .. n) to their exclusive prefixes in out (which may be words), out[n] = the total
void scan_words(const unsigned long long* words, unsigned long long n, unsigned long long* out, hipStream_t st) {
  hipLaunchKernelGGL((scan_sums_kernel<PAV_WAVES, false, LoadWord>), dim3(1), dim3(PAV_THREADS), 0, st, LoadWord{words}, n, out, (unsigned long long*)nullptr);
}

}  // namespace

void launch_pav_count(const uint32_t* runs, const PavProb* probs, int nprob, unsigned long long n_bases, uint32_t n_groups, uint32_t* flags,
                      unsigned long long* cnt, unsigned long long* off, bool eq_only, hipStream_t st) {
  if (nprob <= 0) return;
  if (eq_only) hipLaunchKernelGGL(pav_count_kernel<true>, dim3((unsigned)nprob), dim3(PAV_THREADS), 0, st, runs, probs, n_bases, n_groups, flags, cnt);
  else hipLaunchKernelGGL(pav_count_kernel<false>, dim3((unsigned)nprob), dim3(PAV_THREADS), 0, st, runs, probs, n_bases, n_groups, flags, cnt);
  scan_words(cnt, (unsigned long long)nprob, off, st);  // off[i] = the segments of the problems before i, off[nprob] = all of them
}

void launch_pav_write(const uint32_t* runs, const PavProb* probs, int nprob, const uint32_t* flags, const unsigned long long* off,
                      unsigned long long* ks, unsigned long long* ke, bool eq_only, hipStream_t st) {
  if (nprob <= 0) return;
  if (eq_only) hipLaunchKernelGGL(pav_write_kernel<true>, dim3((unsigned)nprob), dim3(PAV_THREADS), 0, st, runs, probs, flags, off, ks, ke);
  else hipLaunchKernelGGL(pav_write_kernel<false>, dim3((unsigned)nprob), dim3(PAV_THREADS), 0, st, runs, probs, flags, off, ks, ke);
}

hipError_t pav_sort(void* tmp, size_t* tmp_bytes, const unsigned long long* ks, unsigned long long* ks2, const unsigned long long* ke,
                    unsigned long long* ke2, unsigned long long n, unsigned end_bit, hipStream_t st) {
  return rocprim::radix_sort_pairs(tmp, *tmp_bytes, ks, ks2, ke, ke2, (size_t)n, 0u, end_bit, st);
}

void launch_pav_runmax(unsigned long long* ke, unsigned long long n, unsigned long long* aux, hipStream_t st) {
  if (n == 0) return;
  launch_runmax<PAV_WAVES>(LoadWord{ke}, n, aux, ke, st);  // in place
}

void launch_pav_compact(const unsigned long long* ks, const unsigned long long* rm, unsigned long long n, unsigned long long* aux,
                        unsigned long long* uks, unsigned long long* uke, hipStream_t st) {
  if (n == 0) return;
  const unsigned nb = blocks_of(n, WFM_PAV_SCAN_BLOCK);
  hipLaunchKernelGGL(pav_block_sum_kernel<true>, dim3(nb), dim3(PAV_THREADS), 0, st, ks, rm, n, aux);
  scan_words(aux, (unsigned long long)nb, aux, st);
  hipLaunchKernelGGL(pav_compact_kernel, dim3(nb), dim3(PAV_THREADS), 0, st, ks, rm, n, (const unsigned long long*)aux, uks, uke);
}

void launch_pav_prefix(const unsigned long long* uks, const unsigned long long* uke, unsigned long long m, unsigned long long* aux,
                       unsigned long long* C, hipStream_t st) {
  if (m == 0) return;
  const unsigned nb = blocks_of(m, WFM_PAV_SCAN_BLOCK);
  hipLaunchKernelGGL(pav_block_sum_kernel<false>, dim3(nb), dim3(PAV_THREADS), 0, st, uks, uke, m, aux);
  scan_words(aux, (unsigned long long)nb, aux, st);
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
