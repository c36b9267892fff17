// wfa_check.hip -- wfm_check_runs: every CIGAR run held against the bases it covers (include/wfmash_hip.h).
//
// The check shares nothing with the aligners: it reads the seqset's forward BYTE copies (never the 2-bit mirror), has no cell
// step and no walk back.  Three launches per call:
//
//   check_scan_kernel     one workgroup per problem.  Rounds of 256 runs with a carry: the exclusive prefix of the (op, pattern,
//                         text) advance of every run goes to three arrays, and the same pass gives the price, the counts and the
//                         structural flags (BAD_RUN, SPANS, COUNTS, SCORE).  cmp_ops[problem] = the ops to compare, 0 where the
//                         runs spell more bases than a sequence has: such a problem is never compared.
//   check_compare_kernel  one workgroup per slice of WFM_CHECK_SLICE ops of one problem.  The slice finds its first run by binary
//                         search in the op prefix and takes its runs 256 at a time: every M / X run, cut to the slice, is so many
//                         units of 16 bases; the units of the 256 runs are numbered through (a block scan) and dealt to the lanes,
//                         so a long run is read by consecutive lanes, 16 consecutive bytes each, and short runs take a lane each.
//                         A unit is two unaligned 16-byte loads (pattern and text start at unrelated alignments), one XOR, one
//                         exact per-byte "differs" mask and one mask for the run's edge.  Only the last 15 bytes of a sequence
//                         are read byte by byte: no load ever leaves [0, plen) / [0, tlen).
//                         An offending base goes into a 64-bit atomic minimum per problem on (pattern index << 32) | run: pattern
//                         indices rise strictly over M / X bases, so the minimum is the same whatever order the tasks finish in.
//   check_finish_kernel   one thread per problem: the minimum back into bad_p / bad_t / bad_run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/wfmash_hip.h"
#include "wfa_device.h"

namespace wfm {
namespace {

constexpr int CK_THREADS = 256;
constexpr unsigned long long CK_NONE = ~0ull;

__device__ __forceinline__ unsigned long long shfl_up64(unsigned long long v, int d) {
  const unsigned lo = __shfl_up((unsigned)v, d, 64), hi = __shfl_up((unsigned)(v >> 32), d, 64);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(CK_THREADS) void check_scan_kernel(const uint32_t* __restrict__ runs, const CheckProb* __restrict__ probs,
                                                               uint32_t* __restrict__ ops_pre, uint32_t* __restrict__ p_pre,
                                                               uint32_t* __restrict__ t_pre, wfm_check_t* __restrict__ out,
                                                               unsigned long long* __restrict__ keys, uint32_t* __restrict__ cmp_ops, DevPen pen) {
  const CheckProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) { keys[blockIdx.x] = CK_NONE; cmp_ops[blockIdx.x] = 0; }
  if (pr.skip) {
    if (tid == 0) {
      wfm_check_t o;
      memset(&o, 0, sizeof(o));
      o.flags = WFM_CK_NOT_CHECKED; o.bad_p = -1; o.bad_t = -1;
      out[blockIdx.x] = o;
    }
    return;
  }
  __shared__ unsigned long long wtot[3][CK_THREADS / 64];
  __shared__ unsigned long long s_price;
  __shared__ unsigned int s_cnt[6], s_first_bad;
  if (tid == 0) { s_price = 0; s_first_bad = 0xffffffffu; }
  if (tid < 6) s_cnt[tid] = 0;
  const uint32_t* my = runs + pr.run_off;
  const uint32_t n = pr.n_runs;
  unsigned long long carry_o = 0, carry_p = 0, carry_t = 0;
  unsigned long long price = 0;
  uint32_t cnt[6] = {0, 0, 0, 0, 0, 0};  // matches, mismatches, ins_runs, ins_bases, del_runs, del_bases
  uint32_t first_bad = 0xffffffffu;
  for (uint32_t base = 0; base < n; base += CK_THREADS) {
    const uint32_t r = base + (uint32_t)tid;
    const bool valid = r < n;
    const uint32_t run = valid ? my[r] : 0u;
    const uint32_t len = WFM_RUN_LEN(run), op = WFM_RUN_OP(run);
    unsigned long long ao = len, ap = (op != OP_I) ? len : 0u, at = (op != OP_D) ? len : 0u;
    if (valid) {
      if ((len == 0 || (r > 0 && WFM_RUN_OP(my[r - 1]) == op)) && r < first_bad) first_bad = r;
      if (op == OP_M) cnt[0] += len;
      else if (op == OP_X) { cnt[1] += len; price += (unsigned long long)pen.x * len; }
      else {
        if (op == OP_I) { cnt[2] += len ? 1u : 0u; cnt[3] += len; } else { cnt[4] += len ? 1u : 0u; cnt[5] += len; }
        // the free part of the problem's first and last run (ENDSFREE; the allowances are 0 otherwise): the gap price is monotone,
        // so taking off all that is allowed is the cheapest reading
        long long L = len;
        if (r == 0) L -= min(L, (long long)(op == OP_D ? pr.pbf : pr.tbf));
        if (r == n - 1) L -= min(L, (long long)(op == OP_D ? pr.pef : pr.tef));
        if (L > 0) price += (unsigned long long)min((long long)pen.o1 + (long long)pen.e1 * L, (long long)pen.o2 + (long long)pen.e2 * L);
      }
    }
    // inclusive scan of the three advances over the round: within a wave by shuffles, across the four waves through LDS
    unsigned long long io = ao, ip = ap, it = at;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long uo = shfl_up64(io, d), up = shfl_up64(ip, d), ut = shfl_up64(it, d);
      if (lane >= d) { io += uo; ip += up; it += ut; }
    }
    if (lane == 63) { wtot[0][wave] = io; wtot[1][wave] = ip; wtot[2][wave] = it; }
    __syncthreads();
    unsigned long long bo = carry_o, bp = carry_p, bt = carry_t, to = 0, tp = 0, tt = 0;
#pragma unroll
    for (int w = 0; w < CK_THREADS / 64; ++w) {
      if (w < wave) { bo += wtot[0][w]; bp += wtot[1][w]; bt += wtot[2][w]; }
      to += wtot[0][w]; tp += wtot[1][w]; tt += wtot[2][w];
    }
    if (valid) {
      // (a problem whose totals pass its sequences' lengths is never compared: the low words are all its prefix is read for)
      ops_pre[pr.run_off + r] = (uint32_t)(bo + io - ao);
      p_pre[pr.run_off + r] = (uint32_t)(bp + ip - ap);
      t_pre[pr.run_off + r] = (uint32_t)(bt + it - at);
    }
    carry_o += to; carry_p += tp; carry_t += tt;
    __syncthreads();
  }
  __syncthreads();  // (the accumulators' zeroes, for a problem without runs)
  if (price) atomicAdd(&s_price, price);
#pragma unroll
  for (int q = 0; q < 6; ++q) if (cnt[q]) atomicAdd(&s_cnt[q], cnt[q]);
  if (first_bad != 0xffffffffu) atomicMin(&s_first_bad, first_bad);
  __syncthreads();
  if (tid == 0) {
    wfm_check_t o;
    memset(&o, 0, sizeof(o));
    const unsigned long long total = s_price;
    o.score = total > 0x7fffffffull ? 0x7fffffff : (int32_t)total;
    o.bad_p = -1; o.bad_t = -1;
    o.n_runs = n;
    o.matches = s_cnt[0]; o.mismatches = s_cnt[1]; o.ins_runs = s_cnt[2]; o.ins_bases = s_cnt[3]; o.del_runs = s_cnt[4]; o.del_bases = s_cnt[5];
    uint32_t f = 0;
    if (s_first_bad != 0xffffffffu) { f |= WFM_CK_BAD_RUN; o.bad_run = s_first_bad; }
    if (carry_p != (unsigned long long)pr.plen || carry_t != (unsigned long long)pr.tlen) f |= WFM_CK_SPANS;
    if (carry_o != (unsigned long long)pr.res_ops_len) f |= WFM_CK_COUNTS;
    if (pr.res_score >= 0 && total != (unsigned long long)pr.res_score) f |= WFM_CK_SCORE;
    o.flags = f;
    out[blockIdx.x] = o;
    // bases are compared only where the runs stay inside both sequences (then carry_o <= plen + tlen <= 2^29)
    if (carry_p <= (unsigned long long)pr.plen && carry_t <= (unsigned long long)pr.tlen) cmp_ops[blockIdx.x] = (uint32_t)carry_o;
  }
}

// bit 7 of every byte of x that is not zero (exact per byte: 0x7f + 0x7f does not carry into the next byte)
__device__ __forceinline__ unsigned long long nonzero_bytes(unsigned long long x) {
  const unsigned long long L = 0x7f7f7f7f7f7f7f7full;
  return (((x & L) + L) | x) & ~L;
}
// bit 7 of the bytes [0, cnt) of a 64-bit word, cnt in 0 .. 8
__device__ __forceinline__ unsigned long long first_bytes(int cnt) {
  const unsigned long long H = 0x8080808080808080ull;
  return cnt >= 8 ? H : (cnt <= 0 ? 0ull : H & ((1ull << (8 * cnt)) - 1ull));
}
// up to 15 bytes, one at a time: the tail of a sequence, where a 16-byte load would leave it
__device__ __forceinline__ void load_tail(const uint8_t* p, int cnt, unsigned long long* w0, unsigned long long* w1) {
  unsigned long long a = 0, b = 0;
  for (int q = 0; q < cnt && q < 8; ++q) a |= (unsigned long long)p[q] << (8 * q);
  for (int q = 8; q < cnt; ++q) b |= (unsigned long long)p[q] << (8 * (q - 8));
  *w0 = a; *w1 = b;
}

__global__ __launch_bounds__(CK_THREADS) void check_compare_kernel(const uint8_t* __restrict__ seq, const uint32_t* __restrict__ runs,
                                                                  const CheckProb* __restrict__ probs, const CheckTask* __restrict__ tasks,
                                                                  const uint32_t* __restrict__ ops_pre, const uint32_t* __restrict__ p_pre,
                                                                  const uint32_t* __restrict__ t_pre, const uint32_t* __restrict__ cmp_ops,
                                                                  wfm_check_t* __restrict__ out, unsigned long long* __restrict__ keys) {
  const CheckTask task = tasks[blockIdx.x];
  const uint32_t total = cmp_ops[task.prob];
  const uint32_t s0 = (uint32_t)task.slice * (uint32_t)WFM_CHECK_SLICE;
  if (s0 >= total) return;
  const uint32_t s1 = min(s0 + (uint32_t)WFM_CHECK_SLICE, total);
  const CheckProb pr = probs[task.prob];
  const uint32_t n = pr.n_runs;
  const uint32_t* my = runs + pr.run_off;
  const uint32_t* opre = ops_pre + pr.run_off;
  const uint32_t* ppre = p_pre + pr.run_off;
  const uint32_t* tpre = t_pre + pr.run_off;
  const uint8_t* P = seq + pr.p_off;
  const uint8_t* T = seq + pr.t_off;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the slice's first run: the last one that begins at or before s0 (total > s0 >= 0, so there is one)
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (opre[mid] <= s0) lo = mid; else hi = mid;
  }
  __shared__ uint32_t s_incl[CK_THREADS], s_p[CK_THREADS], s_t[CK_THREADS], s_len[CK_THREADS];  // s_len: (bases << 1) | (op == X)
  __shared__ uint32_t s_wtot[CK_THREADS / 64];
  for (uint32_t base = lo; base < n; base += CK_THREADS) {
    const uint32_t r = base + (uint32_t)tid;
    uint32_t units = 0, ps = 0, ts = 0, cl = 0;
    if (r < n) {
      const uint32_t o = opre[r];
      if (o < s1) {
        const uint32_t run = my[r], len = WFM_RUN_LEN(run), op = WFM_RUN_OP(run);
        const uint32_t a = max(o, s0), b = min(o + len, s1);
        if (op <= OP_X && b > a) {
          units = (b - a + 15u) >> 4;
          ps = ppre[r] + (a - o); ts = tpre[r] + (a - o);
          cl = ((b - a) << 1) | op;
        }
      }
    }
    uint32_t incl = units;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t u = __shfl_up(incl, d, 64);
      if (lane >= d) incl += u;
    }
    if (lane == 63) s_wtot[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < CK_THREADS / 64; ++w) { if (w < wave) before += s_wtot[w]; all += s_wtot[w]; }
    s_incl[tid] = incl + before; s_p[tid] = ps; s_t[tid] = ts; s_len[tid] = cl;
    __syncthreads();
    for (uint32_t u = (uint32_t)tid; u < all; u += CK_THREADS) {
      // the run of unit u: the first j with s_incl[j] > u
      int j = 0;
#pragma unroll
      for (int step = CK_THREADS / 2; step > 0; step >>= 1)
        if (s_incl[j + step - 1] <= u) j += step;
      const uint32_t cl_j = s_len[j], blen = cl_j >> 1;
      const uint32_t nun = (blen + 15u) >> 4;
      const uint32_t k = u - (s_incl[j] - nun);
      const uint32_t off = k << 4;
      const int cnt = (int)min(16u, blen - off);
      const uint32_t p = s_p[j] + off, t = s_t[j] + off;
      unsigned long long a0, a1, b0, b1;
      if (p + 16u <= (uint32_t)pr.plen && t + 16u <= (uint32_t)pr.tlen) {
        uint4 va, vb;
        __builtin_memcpy(&va, P + p, 16);
        __builtin_memcpy(&vb, T + t, 16);
        a0 = ((unsigned long long)va.y << 32) | va.x; a1 = ((unsigned long long)va.w << 32) | va.z;
        b0 = ((unsigned long long)vb.y << 32) | vb.x; b1 = ((unsigned long long)vb.w << 32) | vb.z;
      } else {  // (cnt <= 15 here: 16 bases of a run lie inside both sequences)
        load_tail(P + p, cnt, &a0, &a1);
        load_tail(T + t, cnt, &b0, &b1);
      }
      const unsigned long long H = 0x8080808080808080ull;
      unsigned long long d0 = nonzero_bytes(a0 ^ b0), d1 = nonzero_bytes(a1 ^ b1);
      const bool is_x = (cl_j & 1u) != 0;
      if (is_x) { d0 = ~d0 & H; d1 = ~d1 & H; }  // an X run offends where the bytes are EQUAL
      d0 &= first_bytes(cnt); d1 &= first_bytes(cnt - 8);
      if (d0 | d1) {
        const uint32_t idx = d0 ? (uint32_t)(__ffsll((long long)d0) - 1) >> 3 : 8u + ((uint32_t)(__ffsll((long long)d1) - 1) >> 3);
        atomicMin(&keys[task.prob], ((unsigned long long)(p + idx) << 32) | (unsigned long long)(base + (uint32_t)j));
        atomicOr(&out[task.prob].flags, is_x ? WFM_CK_X_EQUAL : WFM_CK_M_DIFFERS);
      }
    }
    if (base + CK_THREADS >= n || opre[base + CK_THREADS] >= s1) break;  // (the same for every thread)
    __syncthreads();
  }
}

__global__ __launch_bounds__(CK_THREADS) void check_finish_kernel(const CheckProb* __restrict__ probs, const uint32_t* __restrict__ p_pre,
                                                                 const uint32_t* __restrict__ t_pre, const unsigned long long* __restrict__ keys,
                                                                 wfm_check_t* __restrict__ out, int nprob) {
  const int i = blockIdx.x * CK_THREADS + threadIdx.x;
  if (i >= nprob) return;
  const unsigned long long key = keys[i];
  if (key == CK_NONE) return;
  const uint32_t p = (uint32_t)(key >> 32), run = (uint32_t)key;
  const uint64_t at = probs[i].run_off + run;
  out[i].bad_p = (int32_t)p;
  out[i].bad_t = (int32_t)(t_pre[at] + (p - p_pre[at]));
  out[i].bad_run = run;
}

}  // namespace

void launch_check(const uint8_t* seq, const uint32_t* runs, const CheckProb* probs, int nprob, const CheckTask* tasks, int64_t ntasks,
                  uint32_t* ops_pre, uint32_t* p_pre, uint32_t* t_pre, uint32_t* cmp_ops, unsigned long long* keys, void* out, DevPen pen,
                  hipStream_t st) {
  if (nprob <= 0) return;
  wfm_check_t* o = (wfm_check_t*)out;
  hipLaunchKernelGGL(check_scan_kernel, dim3((unsigned)nprob), dim3(CK_THREADS), 0, st, runs, probs, ops_pre, p_pre, t_pre, o, keys, cmp_ops, pen);
  if (ntasks > 0)
    hipLaunchKernelGGL(check_compare_kernel, dim3((unsigned)ntasks), dim3(CK_THREADS), 0, st, seq, runs, probs, tasks, ops_pre, p_pre, t_pre, cmp_ops, o, keys);
  hipLaunchKernelGGL(check_finish_kernel, dim3((unsigned)((nprob + CK_THREADS - 1) / CK_THREADS)), dim3(CK_THREADS), 0, st, probs, p_pre, t_pre, keys, o, nprob);
}

}  // namespace wfm
