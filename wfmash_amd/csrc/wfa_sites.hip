// wfa_sites.hip -- the kernels behind wfm_sites_* (include/wfmash_hip.h): the variants of many records joined into distinct sites, and the
// sites x groups table of '0' / '1' / '.'.  Everything here runs at the table call but the fold, which runs once per add.
//
//   sites_fold_kernel     the allele bytes of an add to upper case, one byte a lane.
//   sites_key_kernel      one lane per variant: k1 = pos << 2 | kind, k3 = group, the identity permutation, and, where REF + ALT fit
//                         WFM_SITES_SLICE bytes (the common case), their hash; 0 for a longer pair.
//   sites_longhash_kernel one workgroup per WFM_SITES_TASK bytes of a long pair, one slice of WFM_SITES_SLICE bytes a lane whatever the
//                         pair's length.  The hash is a polynomial modulo 2^64, sum of (byte[j] + 1) * P^j: a slice's partial times
//                         P^(its first index) is its share, and the shares ADD UP exactly, in any order -- the one atomic of this file,
//                         an integer add per task, cannot make two calls differ.
//   sites_mix_kernel      the two lengths into the sum, a bijective mix, the cut to WFM_SITES_HASH_BITS bits.
//   sort                  three stable rocprim::radix_sort_pairs, group, hash, k1: least significant word first, each over the bits its
//                         keys can have, a permutation as the value (sites_gather*_kernel fetches the next pass's keys through it).
//   sites_head_kernel     sorted record i heads a site iff i == 0, or (k1, k2) differ from i - 1's, or the lengths or the BYTES differ:
//                         a short pair is compared by the lane, a long one is left to
//   sites_longcmp_kernel  one workgroup per task again, against the sorted neighbour before the record (sites_inv_kernel has the record's
//                         place).  Equal keys with different bytes is a COLLISION: the record heads a site of its own and is counted;
//                         the host fails the call if the count is not 0.
//   sites_sum_kernel      per block of WFM_PAV_SCAN_BLOCK records the heads (low half) and the heads of a (site, group) pair (high half)
//                         in one word, the collisions beside; scan_sums_kernel (wfa_scan.h) turns the blocks' sums into prefixes;
//   sites_compact_kernel  first[s] = the site's first record, gfirst[s] = the pairs before it: first[s + 1] - first[s] records sorted by
//                         group, gfirst[s + 1] - gfirst[s] distinct groups among them, with no walk.
//   sites_row_kernel      one lane per site: the representative's fields.
//   sites_gt_kernel       one lane per cell.  Carried: a binary search for g among the site's records.  Else the reference: wfa_pav.hip's
//                         two binary searches in the = union and its prefix C; '0' iff the covered bases of [pos, pos + ref_len) are
//                         ref_len.  O(log n) a cell, no atomics.
// No workgroup ever waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include <rocprim/rocprim.hpp>

#include "../../include/wfmash_hip.h"
#include "wfa_device.h"
#include "wfa_scan.h"

namespace wfm {
namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_WAVES = ST_THREADS / 64;
constexpr unsigned ST_SHIFT = 40;
constexpr unsigned long long ST_P = 0x9E3779B97F4A7C15ull;  // (odd: a unit modulo 2^64)
static_assert(WFM_SITES_TASK == ST_THREADS * WFM_SITES_SLICE, "a task is one slice per lane");
static_assert(WFM_PAV_SCAN_BLOCK == ST_THREADS * 4, "a scan block is four records per lane");

__device__ __forceinline__ unsigned long long st_pow(unsigned long long e) {
  unsigned long long r = 1, b = ST_P;
  for (; e; e >>= 1, b *= b)
    if (e & 1) r *= b;
  return r;
}

// sum of (b[t] + 1) * P^t over t < len, len <= WFM_SITES_SLICE
__device__ __forceinline__ unsigned long long st_slice(const uint8_t* __restrict__ b, uint32_t len) {
  unsigned long long h = 0;
  for (uint32_t t = len; t-- > 0;) h = h * ST_P + (unsigned long long)b[t] + 1ull;
  return h;
}

__device__ __forceinline__ unsigned long long st_mix(unsigned long long x) {  // (splitmix64's finisher: a bijection)
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__global__ __launch_bounds__(ST_THREADS) void sites_fold_kernel(uint8_t* __restrict__ alle, unsigned long long bytes) {
  const unsigned long long i = (unsigned long long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (i >= bytes) return;
  const uint8_t c = alle[i];
  if (c >= 'a' && c <= 'z') alle[i] = (uint8_t)(c - 32);
}

__global__ __launch_bounds__(ST_THREADS) void sites_key_kernel(const SiteVar* __restrict__ vars, const uint8_t* __restrict__ alle, uint32_t n,
                                                               unsigned long long* __restrict__ k1, unsigned long long* __restrict__ k2,
                                                               uint32_t* __restrict__ k3, uint32_t* __restrict__ perm) {
  const uint32_t i = blockIdx.x * ST_THREADS + threadIdx.x;
  if (i >= n) return;
  const SiteVar v = vars[i];
  const unsigned long long len = (unsigned long long)v.ref_len + v.alt_len;
  k1[i] = v.pos << 2 | v.kind;
  k2[i] = len <= WFM_SITES_SLICE ? st_slice(alle + v.off, (uint32_t)len) : 0ull;
  k3[i] = v.group;
  perm[i] = i;
}

__global__ __launch_bounds__(ST_THREADS) void sites_longhash_kernel(const SiteVar* __restrict__ vars, const uint8_t* __restrict__ alle,
                                                                    const unsigned long long* __restrict__ tasks, unsigned long long* __restrict__ k2) {
  __shared__ unsigned long long wtot[ST_WAVES];
  const unsigned long long task = tasks[blockIdx.x];
  const uint32_t rec = (uint32_t)(task >> 32);
  const SiteVar v = vars[rec];
  const unsigned long long len = (unsigned long long)v.ref_len + v.alt_len;
  const unsigned long long j0 = (task & 0xffffffffull) * WFM_SITES_TASK + (unsigned long long)threadIdx.x * WFM_SITES_SLICE;
  unsigned long long share = 0;
  if (j0 < len) {
    const uint32_t l = len - j0 < WFM_SITES_SLICE ? (uint32_t)(len - j0) : (uint32_t)WFM_SITES_SLICE;
    share = st_slice(alle + v.off + j0, l) * st_pow(j0);
  }
  unsigned long long all;
  (void)block_excl<ST_WAVES>(share, wtot, &all);
  if (threadIdx.x == 0) atomicAdd(&k2[rec], all);
}

__global__ __launch_bounds__(ST_THREADS) void sites_mix_kernel(const SiteVar* __restrict__ vars, uint32_t n, unsigned long long mask,
                                                               unsigned long long* __restrict__ k2) {
  const uint32_t i = blockIdx.x * ST_THREADS + threadIdx.x;
  if (i >= n) return;
  k2[i] = st_mix(k2[i] + ((unsigned long long)vars[i].ref_len << 32 | vars[i].alt_len) * 0xD6E8FEB86659FD93ull) & mask;
}

template <class T>
__global__ __launch_bounds__(ST_THREADS) void sites_gather_kernel(const T* __restrict__ in, const uint32_t* __restrict__ perm, uint32_t n, T* __restrict__ out) {
  const uint32_t i = blockIdx.x * ST_THREADS + threadIdx.x;
  if (i < n) out[i] = in[perm[i]];
}

__global__ __launch_bounds__(ST_THREADS) void sites_inv_kernel(const uint32_t* __restrict__ perm, uint32_t n, uint32_t* __restrict__ inv) {
  const uint32_t i = blockIdx.x * ST_THREADS + threadIdx.x;
  if (i < n) inv[perm[i]] = i;
}

__global__ __launch_bounds__(ST_THREADS) void sites_head_kernel(const SiteVar* __restrict__ vars, const uint8_t* __restrict__ alle, uint32_t n,
                                                                const unsigned long long* __restrict__ sk1, const unsigned long long* __restrict__ sk2,
                                                                const uint32_t* __restrict__ perm, uint8_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * ST_THREADS + threadIdx.x;
  if (i >= n) return;
  uint8_t f = 1;
  if (i > 0 && sk1[i] == sk1[i - 1] && sk2[i] == sk2[i - 1]) {
    const SiteVar a = vars[perm[i]], b = vars[perm[i - 1]];
    const unsigned long long len = (unsigned long long)a.ref_len + a.alt_len;
    if (a.ref_len != b.ref_len || a.alt_len != b.alt_len) f = 3;
    else if (len > WFM_SITES_SLICE) f = 2;
    else {
      const uint8_t *pa = alle + a.off, *pb = alle + b.off;
      bool differ = false;
      for (uint32_t t = 0; t < (uint32_t)len; ++t) differ |= pa[t] != pb[t];
      f = differ ? 3 : 0;
    }
  }
  flag[i] = f;
}

__global__ __launch_bounds__(ST_THREADS) void sites_longcmp_kernel(const SiteVar* __restrict__ vars, const uint8_t* __restrict__ alle,
                                                                   const unsigned long long* __restrict__ tasks, const uint32_t* __restrict__ perm,
                                                                   const uint32_t* __restrict__ inv, uint8_t* flag) {
  const unsigned long long task = tasks[blockIdx.x];
  const uint32_t rec = (uint32_t)(task >> 32);
  const uint32_t i = inv[rec];
  // (2: sites_head_kernel found the keys and the lengths equal to i - 1's, so i >= 1; 3: another task of this record found a difference)
  if (flag[i] < 2) return;  // (the whole workgroup)
  const SiteVar a = vars[rec], b = vars[perm[i - 1]];
  const unsigned long long len = (unsigned long long)a.ref_len + a.alt_len;
  const unsigned long long j0 = (task & 0xffffffffull) * WFM_SITES_TASK + (unsigned long long)threadIdx.x * WFM_SITES_SLICE;
  int differ = 0;
  if (j0 < len) {
    const uint32_t l = len - j0 < WFM_SITES_SLICE ? (uint32_t)(len - j0) : (uint32_t)WFM_SITES_SLICE;
    const uint8_t *pa = alle + a.off + j0, *pb = alle + b.off + j0;
    for (uint32_t t = 0; t < l; ++t) differ |= pa[t] != pb[t];
  }
  if (__syncthreads_or(differ) && threadIdx.x == 0) flag[i] = 3;  // (every writer stores the same value)
}

// what the scan adds up per sorted record: 1 where it heads a site, 1 << 32 where it heads a (site, group) pair
__device__ __forceinline__ unsigned long long st_term(const uint8_t* __restrict__ flag, const uint32_t* __restrict__ sk3, uint32_t i) {
  const bool head = (flag[i] & 1) != 0;
  const bool ghead = head || (i > 0 && sk3[i] != sk3[i - 1]);
  return (head ? 1ull : 0ull) | (ghead ? 1ull << 32 : 0ull);
}

__global__ __launch_bounds__(ST_THREADS) void sites_sum_kernel(const uint8_t* __restrict__ flag, const uint32_t* __restrict__ sk3, uint32_t n,
                                                               unsigned long long* __restrict__ sums, unsigned long long* __restrict__ coll) {
  __shared__ unsigned long long wtot[ST_WAVES];
  const unsigned long long at = (unsigned long long)blockIdx.x * WFM_PAV_SCAN_BLOCK + (unsigned long long)threadIdx.x * 4u;
  unsigned long long v = 0, c = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (at + k < n) { v += st_term(flag, sk3, (uint32_t)(at + k)); c += flag[at + k] == 3; }
  unsigned long long all, call;
  (void)block_excl<ST_WAVES>(v, wtot, &all);
  (void)block_excl<ST_WAVES>(c, wtot, &call);
  if (threadIdx.x == 0) {
    sums[blockIdx.x] = all;
    if (call) atomicAdd(coll, call);  // (an integer sum: the same whatever the order)
  }
}

__global__ __launch_bounds__(ST_THREADS) void sites_compact_kernel(const uint8_t* __restrict__ flag, const uint32_t* __restrict__ sk3, uint32_t n,
                                                                   const unsigned long long* __restrict__ sums, uint32_t* __restrict__ first,
                                                                   uint32_t* __restrict__ gfirst) {
  __shared__ unsigned long long wtot[ST_WAVES];
  const unsigned long long at = (unsigned long long)blockIdx.x * WFM_PAV_SCAN_BLOCK + (unsigned long long)threadIdx.x * 4u;
  unsigned long long f[4], v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { f[k] = at + k < n ? st_term(flag, sk3, (uint32_t)(at + k)) : 0ull; v += f[k]; }
  unsigned long long all;
  unsigned long long run = sums[blockIdx.x] + block_excl<ST_WAVES>(v, wtot, &all);  // (n < 2^31: neither half carries into the other)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long i = at + k;
    if (i >= n) break;
    // (the heads before i are fewer than the sites, and the caller has made room for n + 1 of each)
    if (f[k] & 1) { first[(uint32_t)run] = (uint32_t)i; gfirst[(uint32_t)run] = (uint32_t)(run >> 32); }
    run += f[k];
    if (i + 1 == n) { first[(uint32_t)run] = n; gfirst[(uint32_t)run] = (uint32_t)(run >> 32); }
  }
}

__global__ __launch_bounds__(ST_THREADS) void sites_row_kernel(const SiteVar* __restrict__ vars, const uint32_t* __restrict__ perm,
                                                               const uint32_t* __restrict__ first, const uint32_t* __restrict__ gfirst, uint32_t n_sites,
                                                               SiteRow* __restrict__ rows) {
  const uint32_t s = blockIdx.x * ST_THREADS + threadIdx.x;
  if (s >= n_sites) return;
  const SiteVar v = vars[perm[first[s]]];
  rows[s] = SiteRow{v.pos, v.kind, gfirst[s + 1] - gfirst[s], v.ref_len, v.alt_len, v.off};
}

__global__ __launch_bounds__(ST_THREADS) void sites_gt_kernel(const SiteRow* __restrict__ rows, const uint32_t* __restrict__ first,
                                                              const uint32_t* __restrict__ sk3, const unsigned long long* __restrict__ uks,
                                                              const unsigned long long* __restrict__ uke, const unsigned long long* __restrict__ C,
                                                              unsigned long long m, unsigned long long ra, unsigned long long cells, uint32_t n_groups,
                                                              uint8_t* __restrict__ out) {
  const unsigned long long cell = (unsigned long long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (cell >= cells) return;
  const unsigned long long s = ra + cell / n_groups;
  const uint32_t g = (uint32_t)(cell % n_groups);
  // carried: the first of the site's records whose group is g or larger
  const uint32_t f0 = first[s], f1 = first[s + 1];
  const unsigned long long at = f0 + first_true(f1 - f0, [&](unsigned long long u) { return sk3[f0 + u] >= g; });
  uint8_t c = '1';
  if (at >= f1 || sk3[at] != g) {
    const SiteRow r = rows[s];
    const unsigned long long gk = (unsigned long long)g << ST_SHIFT, a = gk | r.pos, b = gk | (r.pos + r.ref_len);
    const unsigned long long lo = first_true(m, [&](unsigned long long u) { return uke[u] > a; });
    const unsigned long long hi = first_true(m, [&](unsigned long long u) { return uks[u] >= b; });
    unsigned long long cov = 0;
    if (hi > lo) {  // (then intervals lo .. hi - 1 are this group's: end key > a and start key < b)
      cov = C[hi] - C[lo];
      const unsigned long long st = uks[lo], en = uke[hi - 1];
      if (st < a) cov -= a - st;
      if (en > b) cov -= en - b;
    }
    c = cov == r.ref_len ? '0' : '.';
  }
  out[cell] = c;
}

unsigned st_blocks(unsigned long long n, unsigned long long per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

void launch_sites_fold(uint8_t* alle, unsigned long long bytes, hipStream_t st) {
  if (bytes == 0) return;
  hipLaunchKernelGGL(sites_fold_kernel, dim3(st_blocks(bytes, ST_THREADS)), dim3(ST_THREADS), 0, st, alle, bytes);
}

void launch_sites_keys(const SiteVar* vars, const uint8_t* alle, uint32_t n, const SitesWork& w, unsigned long long n_tasks, unsigned hash_bits, hipStream_t st) {
  if (n == 0) return;
  const unsigned nb = st_blocks(n, ST_THREADS);
  hipLaunchKernelGGL(sites_key_kernel, dim3(nb), dim3(ST_THREADS), 0, st, vars, alle, n, w.k1, w.k2, w.k3, w.pa);
  if (n_tasks) hipLaunchKernelGGL(sites_longhash_kernel, dim3((unsigned)n_tasks), dim3(ST_THREADS), 0, st, vars, alle, w.tasks, w.k2);
  const unsigned long long mask = hash_bits >= 64 ? ~0ull : ((1ull << hash_bits) - 1);
  hipLaunchKernelGGL(sites_mix_kernel, dim3(nb), dim3(ST_THREADS), 0, st, vars, n, mask, w.k2);
}

void launch_sites_gather64(const unsigned long long* in, const uint32_t* perm, uint32_t n, unsigned long long* out, hipStream_t st) {
  if (n) hipLaunchKernelGGL(sites_gather_kernel<unsigned long long>, dim3(st_blocks(n, ST_THREADS)), dim3(ST_THREADS), 0, st, in, perm, n, out);
}

void launch_sites_gather32(const uint32_t* in, const uint32_t* perm, uint32_t n, uint32_t* out, hipStream_t st) {
  if (n) hipLaunchKernelGGL(sites_gather_kernel<uint32_t>, dim3(st_blocks(n, ST_THREADS)), dim3(ST_THREADS), 0, st, in, perm, n, out);
}

hipError_t sites_sort64(void* tmp, size_t* tmp_bytes, const unsigned long long* k, unsigned long long* k2, const uint32_t* v, uint32_t* v2, uint32_t n,
                        unsigned end_bit, hipStream_t st) {
  return rocprim::radix_sort_pairs(tmp, *tmp_bytes, k, k2, v, v2, (size_t)n, 0u, end_bit, st);
}

hipError_t sites_sort32(void* tmp, size_t* tmp_bytes, const uint32_t* k, uint32_t* k2, const uint32_t* v, uint32_t* v2, uint32_t n, unsigned end_bit,
                        hipStream_t st) {
  return rocprim::radix_sort_pairs(tmp, *tmp_bytes, k, k2, v, v2, (size_t)n, 0u, end_bit, st);
}

void launch_sites_heads(const SiteVar* vars, const uint8_t* alle, uint32_t n, const SitesWork& w, const uint32_t* perm, uint32_t* inv,
                        unsigned long long n_tasks, hipStream_t st) {
  if (n == 0) return;
  const unsigned nb = st_blocks(n, ST_THREADS), sb = st_blocks(n, WFM_PAV_SCAN_BLOCK);
  hipLaunchKernelGGL(sites_head_kernel, dim3(nb), dim3(ST_THREADS), 0, st, vars, alle, n, (const unsigned long long*)w.ks, (const unsigned long long*)w.kg, perm, w.flag);
  if (n_tasks) {
    hipLaunchKernelGGL(sites_inv_kernel, dim3(nb), dim3(ST_THREADS), 0, st, perm, n, inv);
    hipLaunchKernelGGL(sites_longcmp_kernel, dim3((unsigned)n_tasks), dim3(ST_THREADS), 0, st, vars, alle, w.tasks, perm, (const uint32_t*)inv, w.flag);
  }
  (void)hipMemsetAsync(w.aux + sb + 1, 0, 8, st);
  hipLaunchKernelGGL(sites_sum_kernel, dim3(sb), dim3(ST_THREADS), 0, st, (const uint8_t*)w.flag, (const uint32_t*)w.sk3, n, w.aux, w.aux + sb + 1);
  hipLaunchKernelGGL((scan_sums_kernel<ST_WAVES, false, LoadWord>), dim3(1), dim3(ST_THREADS), 0, st, LoadWord{w.aux}, (unsigned long long)sb, w.aux,
                     (unsigned long long*)nullptr);
  hipLaunchKernelGGL(sites_compact_kernel, dim3(sb), dim3(ST_THREADS), 0, st, (const uint8_t*)w.flag, (const uint32_t*)w.sk3, n,
                     (const unsigned long long*)w.aux, w.first, w.gfirst);
}

void launch_sites_rows(const SiteVar* vars, const uint32_t* perm, const uint32_t* first, const uint32_t* gfirst, uint32_t n_sites, SiteRow* rows, hipStream_t st) {
  if (n_sites) hipLaunchKernelGGL(sites_row_kernel, dim3(st_blocks(n_sites, ST_THREADS)), dim3(ST_THREADS), 0, st, vars, perm, first, gfirst, n_sites, rows);
}

void launch_sites_gt(const SiteRow* rows, const uint32_t* first, const uint32_t* sk3, const unsigned long long* uks, const unsigned long long* uke,
                     const unsigned long long* C, unsigned long long m, unsigned long long ra, unsigned long long rb, uint32_t n_groups, uint8_t* out,
                     hipStream_t st) {
  if (rb <= ra || n_groups == 0) return;
  const unsigned long long cells = (rb - ra) * n_groups;
  hipLaunchKernelGGL(sites_gt_kernel, dim3(st_blocks(cells, ST_THREADS)), dim3(ST_THREADS), 0, st, rows, first, sk3, uks, uke, C, m, ra, cells, n_groups, out);
}

}  // namespace wfm
