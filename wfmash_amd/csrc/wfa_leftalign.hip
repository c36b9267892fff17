// wfa_leftalign.hip -- wfm_left_align_runs: every interior gap of a CIGAR moved to the leftmost placement a rotation of its bases
// allows (include/wfmash_hip.h states the rule).  Nothing is shared with the aligners' cell step or walk back, and only the seqset's
// forward BYTE copies are read (never the 2-bit mirror: a problem with an N has no usable one, and a gap's two windows are L bytes apart
// at unrelated alignments, so the packed form would need a funnel shift per word for no fewer loads).  Four launches per call:
//
//   la_index_kernel     one workgroup per problem.  Rounds of 256 runs with a carry: the exclusive prefix of every run's pattern and
//                       text advance (kept in registers: only a gap's own start is needed later), the structural test (a run of length 0, two neighbours with one op, totals other than
//                       plen x tlen: WFM_LA_SPANS) and the compact list of the problem's interior gaps, one record each: where its
//                       sequence lies, its first index g, its length L and the run it is.
//   la_rot_lane_kernel  one LANE per gap: rot = the number of k >= 1, consecutive from 1, with S[g - k] == S[g + L - k].  8 bytes per
//                       step from two unaligned 8-byte loads; the step that would reach before the sequence's begin takes its bytes
//                       one by one from clamped indices and masks the ones that do not exist.  Most gaps end in the first step.  A gap
//                       still equal after LA_LANE_MAX bases is appended to a second list (the call's only atomic).
//   la_rot_wave_kernel  one WAVE per gap of the second list: 64 lanes x 16 bytes per step, the first differing lane found by ballot.
//                       The waves of a fixed grid take the list's entries in turn, so the host never reads the list's length.
//   la_shift_kernel     one workgroup per problem.  d by a scan over the RUNS: with x = the shift of the gap before (0 behind an X run
//                       or the begin), an M run of e bases maps x to e + x, a gap maps x to min(rot, x - [the M run before it follows
//                       a gap of the same op]), an X run and the first run start over.  These are maps x -> min(a, b + x); they
//                       compose to (min(a2, b2 + a1), b2 + b1), so a round of 256 runs is one scan and the value that leaves it is
//                       the next round's x.  Then the rewrite: an M run loses what the gap behind it takes and gains what the gap
//                       before it gave, a gap stays, and a gap whose successor is no M run leaves its d bases as a new M run; the
//                       runs that remain are numbered through by a second scan and written to the problem's slots of the output.
//                       A problem that is not to be touched (score-only, status != 0, WFM_LA_SPANS) has its runs copied.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/wfmash_hip.h"
#include "wfa_device.h"

namespace wfm {
namespace {

constexpr int LA_THREADS = 256;
constexpr int LA_WAVES = LA_THREADS / 64;
constexpr long long LA_INF = 1ll << 40;  // "no bound": beyond every sum of run lengths (a problem spells at most 2^29 bases)

__device__ __forceinline__ long long la_shfl_up64(long long v, int d) {
  const unsigned lo = __shfl_up((unsigned)v, d, 64), hi = __shfl_up((unsigned)((unsigned long long)v >> 32), d, 64);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ unsigned long long la_shfl_down64(unsigned long long v, int d) {
  const unsigned lo = __shfl_down((unsigned)v, d, 64), hi = __shfl_down((unsigned)(v >> 32), d, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// exclusive prefix of v over the workgroup's threads (in thread order) and the total; wtot: LA_WAVES words of LDS.  Two barriers.
__device__ __forceinline__ uint32_t la_block_excl(uint32_t v, uint32_t* wtot, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(incl, d, 64);
    if (lane >= d) incl += u;
  }
  __syncthreads();  // (the words may still be read from the round before)
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < LA_WAVES; ++w) { if (w < wave) before += wtot[w]; all += wtot[w]; }
  *total = all;
  return before + incl - v;
}

__global__ __launch_bounds__(LA_THREADS) void la_index_kernel(const uint32_t* __restrict__ runs, const LaProb* __restrict__ probs,
                                                             uint32_t* __restrict__ rot, LaGap* __restrict__ gaps,
                                                             uint32_t* __restrict__ flags) {
  const LaProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x;
  if (pr.skip) {
    if (tid == 0) flags[blockIdx.x] = WFM_LA_NOT_DONE;
    return;
  }
  __shared__ uint32_t wtot[LA_WAVES];
  __shared__ uint32_t s_bad;
  if (tid == 0) s_bad = 0;
  const uint32_t* my = runs + pr.run_off;
  const uint32_t n = pr.n_runs;
  unsigned long long carry_p = 0, carry_t = 0;
  uint32_t carry_g = 0;
  bool bad = false;
  for (uint32_t base = 0; base < n; base += LA_THREADS) {
    const uint32_t r = base + (uint32_t)tid;
    const bool valid = r < n;
    const uint32_t run = valid ? my[r] : 0u;
    const uint32_t len = WFM_RUN_LEN(run), op = WFM_RUN_OP(run);
    const uint32_t ap = (valid && op != OP_I) ? len : 0u, at = (valid && op != OP_D) ? len : 0u;
    const bool gap = valid && op >= OP_I && r > 0 && r + 1 < n;
    if (valid && (len == 0 || (r > 0 && WFM_RUN_OP(my[r - 1]) == op))) bad = true;
    // (one round spells at most 256 x 2^30 bases: the round's sums are taken in 64 bits by halves of 2^15)
    uint32_t tp_lo, tp_hi, tt_lo, tt_hi, tg;
    const uint32_t ep_lo = la_block_excl(ap & 0x7fffu, wtot, &tp_lo), ep_hi = la_block_excl(ap >> 15, wtot, &tp_hi);
    const uint32_t et_lo = la_block_excl(at & 0x7fffu, wtot, &tt_lo), et_hi = la_block_excl(at >> 15, wtot, &tt_hi);
    const uint32_t eg = la_block_excl(gap ? 1u : 0u, wtot, &tg);
    const unsigned long long pp = carry_p + (((unsigned long long)ep_hi << 15) + ep_lo), tt = carry_t + (((unsigned long long)et_hi << 15) + et_lo);
    if (valid) {
      // (a problem whose totals pass its sequences' lengths is flagged below and its gaps are never read: the low word is all g is for)
      rot[pr.run_off + r] = 0;
      if (gap && carry_g + eg < pr.n_gaps) {
        LaGap g;
        g.s_off = op == OP_D ? pr.p_off : pr.t_off;
        g.g = (uint32_t)(op == OP_D ? pp : tt);
        g.len = len;
        g.prob = blockIdx.x;
        g.run = r;
        gaps[pr.gap_off + carry_g + eg] = g;
      }
    }
    carry_p += ((unsigned long long)tp_hi << 15) + tp_lo;
    carry_t += ((unsigned long long)tt_hi << 15) + tt_lo;
    carry_g += tg;
  }
  if (bad) s_bad = 1;  // (every writer stores the same value)
  __syncthreads();
  if (tid == 0) {
    // carry_g != n_gaps: the host counted other gaps than the device sees, which no input can cause; the problem is then left alone
    const bool spans = s_bad || carry_p != (unsigned long long)pr.plen || carry_t != (unsigned long long)pr.tlen || carry_g != pr.n_gaps;
    flags[blockIdx.x] = spans ? WFM_LA_SPANS : 0u;
  }
}

// how many of the cnt top bytes of a and b agree, counted from the top (byte 7) down; cnt in 1 .. 8, the bytes below them are ignored
__device__ __forceinline__ int la_equal_from_top8(unsigned long long a, unsigned long long b, int cnt) {
  unsigned long long x = a ^ b;
  if (cnt < 8) x |= 1ull << (8 * (8 - cnt) - 1);  // a difference in the first byte that does not count
  return x ? (__clzll((long long)x) >> 3) : 8;
}
// 8 bytes S[e - 8 .. e) with every index clamped to >= 0 (the bytes before the begin repeat S[0] and are masked by the caller)
__device__ __forceinline__ unsigned long long la_load8_clamped(const uint8_t* S, long long e) {
  unsigned long long v = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const long long i = e - 8 + q;
    v |= (unsigned long long)S[i > 0 ? i : 0] << (8 * q);
  }
  return v;
}
__device__ __forceinline__ unsigned long long la_load8(const uint8_t* p) {
  unsigned long long v;
  __builtin_memcpy(&v, p, 8);
  return v;
}

__global__ __launch_bounds__(LA_THREADS) void la_rot_lane_kernel(const uint8_t* __restrict__ seq, const LaGap* __restrict__ gaps, uint32_t ngaps,
                                                                const LaProb* __restrict__ probs, const uint32_t* __restrict__ flags,
                                                                uint32_t* __restrict__ rot, uint32_t* __restrict__ long_list,
                                                                uint32_t* __restrict__ long_count, uint32_t lane_max, uint32_t nprob) {
  const uint32_t gi = blockIdx.x * LA_THREADS + threadIdx.x;
  if (gi >= ngaps) return;
  const LaGap g = gaps[gi];
  // a record that was never written (the list is filled with ones before the call) or whose problem is left alone names no bases
  if (g.prob >= nprob || flags[g.prob]) return;
  const uint8_t* S = seq + g.s_off;
  const long long L = g.len;
  long long e = g.g;  // S[e - 1] is the next base to compare with S[e - 1 + L]
  uint32_t k = 0;
  bool more = e > 0;
  while (more && k < lane_max) {
    int cnt, eq;
    if (e >= 8) {
      cnt = 8;
      eq = la_equal_from_top8(la_load8(S + e - 8), la_load8(S + e - 8 + L), 8);
    } else {
      cnt = (int)e;
      eq = la_equal_from_top8(la_load8_clamped(S, e), la_load8_clamped(S + L, e), cnt);
    }
    k += (uint32_t)eq;
    e -= eq;
    more = eq == cnt && e > 0;
  }
  rot[probs[g.prob].run_off + g.run] = k;
  if (more) long_list[atomicAdd(long_count, 1u)] = gi;  // still equal after lane_max bases and not at the begin: the wave kernel goes on
}

__global__ __launch_bounds__(LA_THREADS) void la_rot_wave_kernel(const uint8_t* __restrict__ seq, const LaGap* __restrict__ gaps,
                                                                const LaProb* __restrict__ probs, uint32_t* __restrict__ rot,
                                                                const uint32_t* __restrict__ long_list, const uint32_t* __restrict__ long_count) {
  const int lane = threadIdx.x & 63;
  const uint32_t nwaves = gridDim.x * LA_WAVES, count = *long_count;
  for (uint32_t q = blockIdx.x * LA_WAVES + (threadIdx.x >> 6); q < count; q += nwaves) {
    const LaGap g = gaps[long_list[q]];
    const uint8_t* S = seq + g.s_off;
    const long long L = g.len;
    const uint64_t at = probs[g.prob].run_off + g.run;
    uint32_t k = rot[at];  // what the lane kernel found
    long long e = (long long)g.g - k;
    for (;;) {
      // lane l: the 16 bytes below e - 16 l, their agreeing bytes counted from the top
      const long long hi = e - 16 * lane;
      int eq = 0;
      if (hi >= 16) {
        const int e1 = la_equal_from_top8(la_load8(S + hi - 8), la_load8(S + hi - 8 + L), 8);
        eq = e1 < 8 ? e1 : 8 + la_equal_from_top8(la_load8(S + hi - 16), la_load8(S + hi - 16 + L), 8);
      } else if (hi > 0) {
        const int c1 = hi >= 8 ? 8 : (int)hi;
        const int e1 = la_equal_from_top8(la_load8_clamped(S, hi), la_load8_clamped(S + L, hi), c1);
        eq = e1;
        if (e1 == 8 && hi > 8) eq = 8 + la_equal_from_top8(la_load8_clamped(S, hi - 8), la_load8_clamped(S + L, hi - 8), (int)(hi - 8));
      }
      const unsigned long long stop = __ballot(eq < 16);  // (a lane at or before the begin stops the count as well)
      if (stop == 0) { k += 1024; e -= 1024; continue; }
      const int f = __ffsll((long long)stop) - 1;
      k += 16u * (uint32_t)f + (uint32_t)__shfl(eq, f, 64);
      break;
    }
    if (lane == 0) rot[at] = k;
  }
}

__global__ __launch_bounds__(LA_THREADS) void la_shift_kernel(const uint32_t* __restrict__ runs, const LaProb* __restrict__ probs,
                                                             const uint32_t* __restrict__ flags, const uint32_t* __restrict__ rot,
                                                             uint32_t* __restrict__ dval, uint32_t* __restrict__ out,
                                                             wfm_leftalign_t* __restrict__ stats) {
  const LaProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* my = runs + pr.run_off;
  const uint32_t n = pr.n_runs;
  uint32_t* o = out + pr.out_off;
  const uint32_t fl = flags[blockIdx.x];
  if (fl) {  // left exactly as it came
    for (uint32_t r = (uint32_t)tid; r < n; r += LA_THREADS) o[r] = my[r];
    if (tid == 0) {
      wfm_leftalign_t s;
      memset(&s, 0, sizeof(s));
      s.flags = fl; s.runs_out = n;
      stats[blockIdx.x] = s;
    }
    return;
  }
  __shared__ long long s_a[LA_WAVES], s_b[LA_WAVES];
  __shared__ uint32_t wtot[LA_WAVES];
  __shared__ uint32_t s_moved[LA_WAVES], s_longest[LA_WAVES];
  __shared__ unsigned long long s_bases[LA_WAVES];
  uint32_t* d = dval + pr.run_off;
  const uint32_t* rt = rot + pr.run_off;
  // ---- d: the scan of the maps x -> min(a, b + x) over the runs ----
  long long x_in = 0;
  uint32_t moved = 0, longest = 0;
  unsigned long long bases = 0;
  for (uint32_t base = 0; base < n; base += LA_THREADS) {
    const uint32_t r = base + (uint32_t)tid;
    long long a = LA_INF, b = 0;  // (a thread past the last run: the identity)
    bool gap = false;
    if (r < n) {
      const uint32_t run = my[r], len = WFM_RUN_LEN(run), op = WFM_RUN_OP(run);
      if (r == 0) { a = op == OP_M ? (long long)len - 1 : 0; b = LA_INF; }  // the first run stays the first: one base of it is kept
      else if (op == OP_X) { a = 0; b = LA_INF; }
      else if (op == OP_M) { a = LA_INF; b = len; }
      else if (r + 1 == n) { a = 0; b = LA_INF; }  // the last run is not touched
      else {
        gap = true;
        // two gaps of one op never merge: one base of the M run between them is kept
        const bool same = r >= 2 && WFM_RUN_OP(my[r - 1]) == OP_M && WFM_RUN_OP(my[r - 2]) == op;
        a = rt[r]; b = same ? -1 : 0;
      }
    }
    // inclusive scan of the composition (later after earlier): within a wave by shuffles, across the waves through LDS
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) {
      const long long a1 = la_shfl_up64(a, dd), b1 = la_shfl_up64(b, dd);
      if (lane >= dd) { a = min(a, b + a1); b = min(b + b1, LA_INF); }
    }
    __syncthreads();
    if (lane == 63) { s_a[wave] = a; s_b[wave] = b; }
    __syncthreads();
    long long x = x_in, x_round = x_in;
#pragma unroll
    for (int w = 0; w < LA_WAVES; ++w) {
      if (w < wave) x = min(s_a[w], s_b[w] + x);
      x_round = min(s_a[w], s_b[w] + x_round);
    }
    const long long v = min(a, b + x);
    if (r < n) {
      const uint32_t dv = gap ? (uint32_t)v : 0u;
      d[r] = dv;
      if (dv) { ++moved; bases += dv; longest = max(longest, dv); }
    }
    x_in = x_round;
  }
  // (the counts: wave sums by shuffles, the four waves' by thread 0 below)
#pragma unroll
  for (int dd = 32; dd > 0; dd >>= 1) {
    moved += __shfl_down(moved, dd, 64);
    longest = max(longest, (uint32_t)__shfl_down(longest, dd, 64));
    bases += la_shfl_down64(bases, dd);
  }
  if (lane == 0) { s_moved[wave] = moved; s_longest[wave] = longest; s_bases[wave] = bases; }
  __syncthreads();  // (d[] of every run is written and visible to the workgroup)
  // ---- the rewrite ----
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n; base += LA_THREADS) {
    const uint32_t r = base + (uint32_t)tid;
    uint32_t first = 0, second = 0;  // the runs this run leaves (0: none)
    if (r < n) {
      const uint32_t run = my[r], len = WFM_RUN_LEN(run), op = WFM_RUN_OP(run);
      const uint32_t d_before = r > 0 ? d[r - 1] : 0u, d_behind = r + 1 < n ? d[r + 1] : 0u;
      if (op == OP_M) {
        const uint32_t nl = len + d_before - d_behind;
        first = nl ? (nl << 2) | OP_M : 0u;
      } else {
        first = run;
        if (op >= OP_I && r + 1 < n && WFM_RUN_OP(my[r + 1]) != OP_M) {
          const uint32_t nl = d[r] - d_behind;  // (the gap behind can take at most what this one gave)
          second = nl ? (nl << 2) | OP_M : 0u;
        }
      }
    }
    uint32_t total;
    const uint32_t at = carry + la_block_excl((first ? 1u : 0u) + (second ? 1u : 0u), wtot, &total);
    if (first) o[at] = first;
    if (second) o[at + (first ? 1u : 0u)] = second;
    carry += total;
  }
  if (tid == 0) {
    wfm_leftalign_t s;
    memset(&s, 0, sizeof(s));
    s.gaps = pr.n_gaps;
    s.runs_out = carry;
    for (int w = 0; w < LA_WAVES; ++w) { s.moved += s_moved[w]; s.bases_moved += s_bases[w]; s.longest = max(s.longest, s_longest[w]); }
    stats[blockIdx.x] = s;
  }
}

}  // namespace

void launch_left_align(const uint8_t* seq, const uint32_t* runs, const LaProb* probs, int nprob, uint32_t* rot,
                       uint32_t* dval, LaGap* gaps, uint64_t ngaps, uint32_t* flags, uint32_t* long_list, uint32_t* long_count, uint32_t* out,
                       void* stats, uint32_t lane_max, hipStream_t st) {
  if (nprob <= 0) return;
  hipLaunchKernelGGL(la_index_kernel, dim3((unsigned)nprob), dim3(LA_THREADS), 0, st, runs, probs, rot, gaps, flags);
  if (ngaps > 0) {
    const unsigned blocks = (unsigned)((ngaps + LA_THREADS - 1) / LA_THREADS);
    hipLaunchKernelGGL(la_rot_lane_kernel, dim3(blocks), dim3(LA_THREADS), 0, st, seq, gaps, (uint32_t)ngaps, probs, flags, rot, long_list, long_count, lane_max, (uint32_t)nprob);
    // (a wave per long gap, in turn: 1024 workgroups hold every wave slot of the device several times over)
    const unsigned wblocks = (unsigned)std::min<uint64_t>((ngaps + LA_WAVES - 1) / LA_WAVES, 1024);
    hipLaunchKernelGGL(la_rot_wave_kernel, dim3(wblocks), dim3(LA_THREADS), 0, st, seq, gaps, probs, rot, long_list, long_count);
  }
  hipLaunchKernelGGL(la_shift_kernel, dim3((unsigned)nprob), dim3(LA_THREADS), 0, st, runs, probs, flags, rot, dval, out, (wfm_leftalign_t*)stats);
}

}  // namespace wfm
