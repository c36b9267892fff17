// wfa_cs.hip -- wfm_cs_strings: minimap2's cs difference string of every problem's runs, spelled on the device (include/wfmash_hip.h
// states the grammar).  Nothing is shared with the aligners, and only the seqset's forward BYTE copies are read (never the 2-bit mirror: the
// string carries the bytes themselves, an N included).  The string is spelled from the runs, never from a comparison.  Two kernels:
//
//   cs_index_kernel   one workgroup per problem.  Rounds of 256 runs with a carry: the exclusive prefix of every run's pattern advance, text
//                     advance and output bytes (M: 1 + digits(L) short, 1 + L long; X: 3 L; I, D: 1 + L), the structural test (a run of
//                     length 0, two neighbours with one op, totals other than plen x tlen: WFM_CS_SPANS) and one record per run: where its
//                     bases begin in the pattern and the text, where its bytes begin in the problem's string, and the run itself.  The
//                     problem's total goes to the host, which sizes the output and takes the prefix sum over the problems.
//   cs_write_kernel   one workgroup per WFM_CS_SLICE output bytes of a chunk of problems; every lane owns output BYTES.  The workgroup
//                     finds the problem and the run its slice begins in by binary search (over the problems' offsets, then over that
//                     problem's run records), and walks on from there: CS_STAGE run records at a time are staged in LDS, the bytes they
//                     cover are dealt to the lanes one each, and a lane finds its run by a binary search of the staged offsets and
//                     derives its byte from (run, offset within the run).  A long run is as many lanes' work as it has bytes.  The slice
//                     is assembled in LDS and leaves in 16-byte stores, contiguous over the workgroup.
// No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wfmash_hip.h"
#include "wfa_device.h"
#include "wfa_scan.h"

namespace wfm {
namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_WAVES = CS_THREADS / 64;
constexpr int CS_WRITE_THREADS = 1024;  // cs_write_kernel: a slice is 16 rounds of one byte per lane (with 256 lanes a short-form call of few slices waited on 64)
constexpr int CS_STAGE = 1024;  // run records staged at a time: 16 KB of LDS beside the slice's 16 KB

__device__ __forceinline__ uint32_t cs_digits(uint32_t v) {  // v < 2^30: at most 10
  return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
         (v >= 1000000000u);
}
__device__ __forceinline__ uint32_t cs_pow10(uint32_t e) {  // e in 0 .. 9
  uint32_t v = 1;
  for (uint32_t i = 0; i < e; ++i) v *= 10u;
  return v;
}
__device__ __forceinline__ uint8_t cs_lc(uint8_t c) { return (c >= 'A' && c <= 'Z') ? (uint8_t)(c + 32) : c; }

// the bytes a run spells
__device__ __forceinline__ unsigned long long cs_run_bytes(uint32_t op, uint32_t len, int form) {
  if (op == OP_M) return form == WFM_CS_LONG ? 1ull + len : 1ull + cs_digits(len);
  if (op == OP_X) return 3ull * len;
  return 1ull + len;
}

__global__ __launch_bounds__(CS_THREADS) void cs_index_kernel(const uint32_t* __restrict__ runs, const CsProb* __restrict__ probs, int form,
                                                             uint4* __restrict__ recs, unsigned long long* __restrict__ totals,
                                                             uint32_t* __restrict__ flags) {
  const CsProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x;
  if (pr.skip) {
    if (tid == 0) { flags[blockIdx.x] = WFM_CS_NOT_DONE; totals[blockIdx.x] = 0; }
    return;
  }
  __shared__ unsigned long long wtot[CS_WAVES];
  __shared__ uint32_t s_bad;
  if (tid == 0) s_bad = 0;
  const uint32_t* my = runs + pr.run_off;
  uint4* rec = recs + pr.rec_off;
  const uint32_t n = pr.n_runs;
  unsigned long long carry_p = 0, carry_t = 0, carry_o = 0;
  bool bad = false;
  for (uint32_t base = 0; base < n; base += CS_THREADS) {
    const uint32_t r = base + (uint32_t)tid;
    const bool valid = r < n;
    const uint32_t run = valid ? my[r] : 0u;
    const uint32_t len = WFM_RUN_LEN(run), op = WFM_RUN_OP(run);
    const unsigned long long ap = (valid && op != OP_I) ? len : 0u, at = (valid && op != OP_D) ? len : 0u;
    const unsigned long long ao = valid ? cs_run_bytes(op, len, form) : 0ull;
    if (valid && (len == 0 || (r > 0 && WFM_RUN_OP(my[r - 1]) == op))) bad = true;
    unsigned long long tp, tt, to;
    const unsigned long long pp = carry_p + block_excl<CS_WAVES>(ap, wtot, &tp);
    const unsigned long long tx = carry_t + block_excl<CS_WAVES>(at, wtot, &tt);
    const unsigned long long oo = carry_o + block_excl<CS_WAVES>(ao, wtot, &to);
    // (a problem whose totals pass its sequences' lengths, or 32 bits, is flagged below and its records are never read)
    if (valid) rec[r] = make_uint4((uint32_t)pp, (uint32_t)tx, (uint32_t)oo, run);
    carry_p += tp; carry_t += tt; carry_o += to;
  }
  if (bad) s_bad = 1;  // (every writer stores the same value)
  __syncthreads();
  if (tid == 0) {
    const bool spans = s_bad || carry_p != (unsigned long long)pr.plen || carry_t != (unsigned long long)pr.tlen || carry_o >= (1ull << 32);
    flags[blockIdx.x] = spans ? WFM_CS_SPANS : 0u;
    totals[blockIdx.x] = spans ? 0ull : carry_o;
  }
}

// the byte at offset `off` of the string of `run`, whose bases begin at P and T
__device__ __forceinline__ uint8_t cs_byte(uint32_t run, uint32_t off, const uint8_t* __restrict__ P, const uint8_t* __restrict__ T, int form) {
  const uint32_t len = WFM_RUN_LEN(run), op = WFM_RUN_OP(run);
  if (op == OP_X) {
    const uint32_t j = off / 3u, m = off - 3u * j;
    return m == 0 ? (uint8_t)'*' : cs_lc(m == 1 ? P[j] : T[j]);
  }
  if (op == OP_M) {
    if (form == WFM_CS_LONG) return off == 0 ? (uint8_t)'=' : P[off - 1];
    if (off == 0) return (uint8_t)':';
    return (uint8_t)('0' + (len / cs_pow10(cs_digits(len) - off)) % 10u);
  }
  if (off == 0) return op == OP_I ? (uint8_t)'+' : (uint8_t)'-';
  return cs_lc(op == OP_I ? T[off - 1] : P[off - 1]);
}

// goff: the offsets of the call's problems in *out, n + 1 of them; the chunk is the problems [ka, kb), whose strings are the bytes
// [goff[ka], goff[ka] + chunk_bytes) of *out and the bytes [0, chunk_bytes) of `out` here
__global__ __launch_bounds__(CS_WRITE_THREADS) void cs_write_kernel(const uint8_t* __restrict__ seq, const CsProb* __restrict__ probs,
                                                             const uint4* __restrict__ recs, const unsigned long long* __restrict__ goff,
                                                             uint32_t ka, uint32_t kb, unsigned long long chunk_bytes, int form,
                                                             uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t s_out[WFM_CS_SLICE];
  __shared__ uint4 s_rec[CS_STAGE];
  const int tid = threadIdx.x;
  const unsigned long long s0 = (unsigned long long)blockIdx.x * WFM_CS_SLICE;
  if (s0 >= chunk_bytes) return;
  const unsigned long long chunk_base = goff[ka];
  const unsigned long long s1 = s0 + WFM_CS_SLICE < chunk_bytes ? s0 + WFM_CS_SLICE : chunk_bytes;
  unsigned long long g = chunk_base + s0;
  const unsigned long long gend = chunk_base + s1;
  // the problem the slice begins in: the last k in [ka, kb) with goff[k] <= g (goff[kb] >= gend > g, so its own end lies behind g)
  uint32_t k = last_le(ka, kb, [&](uint32_t i) { return goff[i] <= g; });  // goff[ka] <= g < goff[kb]
  while (g < gend) {  // (uniform over the workgroup)
    const unsigned long long pb = goff[k], pe = goff[k + 1];
    if (pe <= g) { ++k; continue; }  // a problem without a string
    const CsProb pr = probs[k];
    const uint4* R = recs + pr.rec_off;
    const uint32_t n = pr.n_runs, rel = (uint32_t)(g - pb);
    // the run the byte g lies in: the last r with R[r].z <= rel.  Only where the slice begins inside a problem: behind that the walk
    // arrives at every run's first byte
    const uint32_t r0 = rel ? last_le(0u, n, [&](uint32_t i) { return R[i].z <= rel; }) : 0u;
    const uint32_t cnt = n - r0 < (uint32_t)CS_STAGE ? n - r0 : (uint32_t)CS_STAGE;
    __syncthreads();  // (the records of the round before are no longer read)
    for (uint32_t i = (uint32_t)tid; i < cnt; i += CS_WRITE_THREADS) s_rec[i] = R[r0 + i];
    const unsigned long long staged_end = pb + (r0 + cnt < n ? (unsigned long long)R[r0 + cnt].z : pe - pb);
    const unsigned long long seg_end = staged_end < gend ? staged_end : gend;
    __syncthreads();
    const uint8_t* P = seq + pr.p_off;
    const uint8_t* T = seq + pr.t_off;
    for (unsigned long long q = g + (unsigned long long)tid; q < seg_end; q += CS_WRITE_THREADS) {
      const uint32_t rq = (uint32_t)(q - pb);
      const uint4 rc = s_rec[last_le(0u, cnt, [&](uint32_t i) { return s_rec[i].z <= rq; })];  // s_rec[0].z <= rq (< the offset behind the staged runs)
      s_out[(uint32_t)(q - chunk_base - s0)] = cs_byte(rc.w, rq - rc.z, P + rc.x, T + rc.y, form);
    }
    g = seg_end;
  }
  __syncthreads();
  // (the output block is a whole number of slices long: the last vector of the chunk's last slice may carry bytes nobody reads)
  const uint32_t nbytes = (uint32_t)(s1 - s0);
  for (uint32_t i = (uint32_t)tid * 16u; i < nbytes; i += CS_WRITE_THREADS * 16u)
    *reinterpret_cast<uint4*>(out + s0 + i) = *reinterpret_cast<const uint4*>(s_out + i);
}

}  // namespace

void launch_cs_index(const uint32_t* runs, const CsProb* probs, int nprob, int form, void* recs, unsigned long long* totals, uint32_t* flags,
                     hipStream_t st) {
  if (nprob <= 0) return;
  hipLaunchKernelGGL(cs_index_kernel, dim3((unsigned)nprob), dim3(CS_THREADS), 0, st, runs, probs, form, (uint4*)recs, totals, flags);
}

void launch_cs_write(const uint8_t* seq, const CsProb* probs, const void* recs, const unsigned long long* goff, uint32_t ka, uint32_t kb,
                     unsigned long long chunk_bytes, int form, uint8_t* out, hipStream_t st) {
  if (chunk_bytes == 0) return;
  const unsigned blocks = (unsigned)((chunk_bytes + WFM_CS_SLICE - 1) / WFM_CS_SLICE);
  hipLaunchKernelGGL(cs_write_kernel, dim3(blocks), dim3(CS_WRITE_THREADS), 0, st, seq, probs, (const uint4*)recs, goff, ka, kb, chunk_bytes, form, out);
}

}  // namespace wfm
