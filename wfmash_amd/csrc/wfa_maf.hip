// wfa_maf.hip -- wfm_maf_rows: the two gapped rows of every problem's runs, cut into the blocks of a pairwise MAF file, spelled on the device
// (include/wfmash_hip.h states the rule).  Nothing is shared with the aligners, and only the seqset's forward BYTE copies are read.  The
// rows are spelled from the runs, never from a comparison.  Three kernels:
//
//   maf_index_kernel   one workgroup per problem, two passes in rounds of 256 runs with a carry.  Pass 1: the exclusive prefixes of every
//                      run's pattern advance, text advance, aligned columns and = columns, the structural test of cs_index_kernel (a run
//                      of length 0, two neighbours with one op, totals other than plen x tlen: WFM_MAF_SPANS, taken before pass 2), the
//                      totals in one slot behind the last run.  Pass 2: a gap run finds the head of its stretch and the run behind it by
//                      two binary searches over the aligned-column prefix (wfa_chain.hip's: the stretch is where that prefix stands
//                      still), takes the stretch's gap bases from the two prefix words and decides "break" against split -- never a walk;
//                      the exclusive prefix of the WRITTEN columns (a break run writes none) completes the run's 16-byte record
//                      {p, t, column offset in the problem, run}; a block's head is a kept run whose predecessor is a break (or none),
//                      counted by a block scan.  The problem's blocks and columns go to the host, which sizes the output.
//   maf_blocks_kernel  one workgroup per problem of a chunk: block number k = block_excl of the head flags plus the carry (no atomics:
//                      two calls give the same bytes), ONE lane per head.  The block ends at the next break, which is the LAST slot whose
//                      count of dropped columns (all columns - written columns, both read off the prefixes) equals the head's: a binary
//                      search; psize, tsize, cols, eq and x are prefix differences.  40 bytes a block.
//   maf_write_kernel   one workgroup per WFM_MAF_SLICE output bytes of a chunk; every lane owns output BYTES.  The workgroup finds the
//                      block its slice begins in by binary search over the blocks' offsets, the row from byte - off >= cols, the run by
//                      binary search over the problem's run records on the written-column prefix, and walks on through rows and blocks:
//                      MAF_STAGE run records at a time are staged in LDS and stay there while the rows that follow lie inside them (row T
//                      behind row P, a run of small blocks), the bytes are dealt to the lanes one each, a lane finds its run by a binary
//                      search of the staged offsets and its byte is P[p + k], T[t + k] or '-'.  The slice is assembled in LDS and leaves
//                      in 16-byte stores, contiguous over the workgroup.
// No atomics, no scratch.  Offsets inside a problem are 32-bit (plen + tlen < 2^32), sums of them 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wfmash_hip.h"
#include "wfa_device.h"
#include "wfa_scan.h"

namespace wfm {
namespace {

constexpr int MAF_THREADS = 256;
constexpr int MAF_WAVES = MAF_THREADS / 64;
constexpr int MAF_WRITE_THREADS = 1024;  // cs_write_kernel's measured shape: a slice is 16 rounds of one byte per lane
constexpr int MAF_STAGE = 1024;          // run records staged at a time: 16 KB of LDS beside the slice's 16 KB

struct MafBlock { unsigned long long off; uint32_t problem, p, t, psize, tsize, cols, eq, x; };
static_assert(sizeof(MafBlock) == sizeof(wfm_maf_block_t) && sizeof(MafBlock) == 40, "MafBlock restates wfm_maf_block_t");

// the gap bases before the run of slot i: pattern + text advance - twice the aligned columns
__device__ __forceinline__ unsigned long long maf_gaps(const uint4* rec, const uint2* pre, uint32_t i) {
  const uint2 pt = *reinterpret_cast<const uint2*>(rec + i);  // (x and y alone: another lane may be storing z)
  return (unsigned long long)pt.x + pt.y - 2ull * pre[i].x;
}
// the columns before the run of slot i that are NOT written: all columns (pattern + text advance - aligned) - the written ones
__device__ __forceinline__ unsigned long long maf_dropped(const uint4* rec, const uint2* pre, uint32_t i) {
  const uint4 w = rec[i];
  return (unsigned long long)w.x + w.y - pre[i].x - w.z;
}

__global__ __launch_bounds__(MAF_THREADS) void maf_index_kernel(const uint32_t* __restrict__ runs, const CsProb* __restrict__ probs, uint32_t split,
                                                                uint4* recs, uint2* pres, unsigned long long* __restrict__ nblk,
                                                                unsigned long long* __restrict__ ncols, uint32_t* __restrict__ flags) {
  const CsProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x;
  if (pr.skip) {
    if (tid == 0) { flags[blockIdx.x] = WFM_MAF_NOT_DONE; nblk[blockIdx.x] = 0; ncols[blockIdx.x] = 0; }
    return;
  }
  __shared__ unsigned long long wtot[MAF_WAVES];
  __shared__ uint32_t s_bad;
  __shared__ uint8_t s_brk[MAF_THREADS];
  if (tid == 0) s_bad = 0;
  __syncthreads();
  const uint32_t* my = runs + pr.run_off;
  uint4* rec = recs + pr.rec_off;
  uint2* pre = pres + pr.rec_off;
  const uint32_t n = pr.n_runs;
  // pass 1: the four prefixes and the structural test
  unsigned long long cp = 0, ct = 0, ca = 0, ce = 0;
  bool bad = false;
  for (uint32_t base = 0; base < n; base += MAF_THREADS) {
    const uint32_t r = base + (uint32_t)tid;
    const bool valid = r < n;
    const uint32_t run = valid ? my[r] : 0u;
    const uint32_t len = WFM_RUN_LEN(run), op = WFM_RUN_OP(run);
    if (valid && (len == 0 || (r > 0 && WFM_RUN_OP(my[r - 1]) == op))) bad = true;
    unsigned long long tp, tt, ta, te;
    const unsigned long long pp = cp + block_excl<MAF_WAVES>((valid && op != OP_I) ? len : 0u, wtot, &tp);
    const unsigned long long pt = ct + block_excl<MAF_WAVES>((valid && op != OP_D) ? len : 0u, wtot, &tt);
    const unsigned long long pa = ca + block_excl<MAF_WAVES>((valid && op <= OP_X) ? len : 0u, wtot, &ta);
    const unsigned long long pe = ce + block_excl<MAF_WAVES>((valid && op == OP_M) ? len : 0u, wtot, &te);
    // (a problem whose totals pass its sequences' lengths, or 32 bits, is flagged below and its records are never read)
    if (valid) { rec[r] = make_uint4((uint32_t)pp, (uint32_t)pt, 0u, run); pre[r] = make_uint2((uint32_t)pa, (uint32_t)pe); }
    cp += tp; ct += tt; ca += ta; ce += te;
  }
  if (bad) s_bad = 1;  // (every writer stores the same value)
  if (tid == 0) { rec[n] = make_uint4((uint32_t)cp, (uint32_t)ct, 0u, 0u); pre[n] = make_uint2((uint32_t)ca, (uint32_t)ce); }
  __syncthreads();  // (s_bad, and every lane's records: pass 2 reads other lanes')
  if (s_bad || cp != (unsigned long long)pr.plen || ct != (unsigned long long)pr.tlen) {  // (the whole workgroup)
    if (tid == 0) { flags[blockIdx.x] = WFM_MAF_SPANS; nblk[blockIdx.x] = 0; ncols[blockIdx.x] = 0; }
    return;
  }
  // pass 2: breaks, the written-column prefix, the heads of the blocks
  unsigned long long cc = 0, heads = 0;
  uint32_t prev_brk = 1;  // "the run before the first is a break": a kept first run is a head
  for (uint32_t base = 0; base < n; base += MAF_THREADS) {
    const uint32_t r = base + (uint32_t)tid;
    const bool valid = r < n;
    const uint32_t run = valid ? my[r] : 0u;
    const uint32_t len = WFM_RUN_LEN(run), op = WFM_RUN_OP(run);
    bool brk = false;
    if (valid && split && op >= OP_I) {
      // the stretch of gap runs r lies in is where the aligned-column prefix stands still: its head is the FIRST slot with that value,
      // the run behind it (or the totals' slot) the LAST
      const uint32_t a = pre[r].x;
      const uint32_t head = (uint32_t)first_true(r, [&](unsigned long long i) { return pre[i].x >= a; });
      const uint32_t behind = last_le(r, n + 1u, [&](uint32_t i) { return pre[i].x <= a; });
      brk = maf_gaps(rec, pre, behind) - maf_gaps(rec, pre, head) >= (unsigned long long)split;
    }
    s_brk[tid] = brk ? 1 : 0;
    __syncthreads();
    const uint32_t before = tid ? s_brk[tid - 1] : prev_brk;
    prev_brk = s_brk[MAF_THREADS - 1];  // (lanes behind n store 0; no round follows them)
    unsigned long long tc, th;
    const unsigned long long col = cc + block_excl<MAF_WAVES>((valid && !brk) ? len : 0u, wtot, &tc);
    (void)block_excl<MAF_WAVES>((valid && !brk && before) ? 1u : 0u, wtot, &th);  // (its barriers lie between the reads of s_brk and the next round's stores)
    if (valid) reinterpret_cast<uint32_t*>(rec + r)[2] = (uint32_t)col;
    cc += tc; heads += th;
  }
  if (tid == 0) {
    reinterpret_cast<uint32_t*>(rec + n)[2] = (uint32_t)cc;
    flags[blockIdx.x] = 0u; nblk[blockIdx.x] = heads; ncols[blockIdx.x] = cc;
  }
}

// the problems from ka on, one per workgroup; out[0] is block number boff[ka] of the whole call
__global__ __launch_bounds__(MAF_THREADS) void maf_blocks_kernel(const CsProb* __restrict__ probs, const uint4* __restrict__ recs,
                                                                 const uint2* __restrict__ pres, const unsigned long long* __restrict__ nblk,
                                                                 const unsigned long long* __restrict__ goff,
                                                                 const unsigned long long* __restrict__ boff, uint32_t ka, MafBlock* __restrict__ out) {
  __shared__ unsigned long long wtot[MAF_WAVES];
  const uint32_t k = ka + blockIdx.x;
  if (nblk[k] == 0) return;  // (the whole workgroup)
  const CsProb pr = probs[k];
  const uint4* rec = recs + pr.rec_off;
  const uint2* pre = pres + pr.rec_off;
  const uint32_t n = pr.n_runs;
  MafBlock* mine = out + (boff[k] - boff[ka]);
  const unsigned long long row0 = goff[k];
  unsigned long long carry = 0;
  for (uint32_t base = 0; base < n; base += MAF_THREADS) {
    const uint32_t r = base + (uint32_t)threadIdx.x;
    bool head = false;
    uint4 wr = make_uint4(0u, 0u, 0u, 0u);
    if (r < n) {
      // (no run is empty here: a run that writes no column is a break)
      wr = rec[r];
      head = rec[r + 1].z != wr.z && (r == 0 || rec[r - 1].z == wr.z);
    }
    unsigned long long all;
    const unsigned long long b = carry + block_excl<MAF_WAVES>(head ? 1u : 0u, wtot, &all);
    carry += all;
    if (!head) continue;
    // the block ends at the next break e (or the totals' slot): the slots r .. e have the same count of dropped columns, e + 1 has more
    const unsigned long long dr = maf_dropped(rec, pre, r);
    const uint32_t e = last_le(r, n + 1u, [&](uint32_t i) { return maf_dropped(rec, pre, i) <= dr; });  // (r < e <= n: run r is kept)
    const uint4 we = rec[e];
    const uint2 ar = pre[r], ae = pre[e];
    MafBlock blk;
    blk.off = row0 + 2ull * wr.z;
    blk.problem = k; blk.p = wr.x; blk.t = wr.y;
    blk.psize = we.x - wr.x; blk.tsize = we.y - wr.y; blk.cols = we.z - wr.z;
    blk.eq = ae.y - ar.y; blk.x = (ae.x - ar.x) - blk.eq;
    mine[b] = blk;  // (b < nblk[k]: maf_index_kernel counted the same heads)
  }
}

// blk: the chunk's nb blocks, whose rows are the bytes [blk[0].off, blk[0].off + chunk_bytes) of the call's rows and the bytes
// [0, chunk_bytes) of `out` here; goff: the offsets of the call's problems in the call's rows
__global__ __launch_bounds__(MAF_WRITE_THREADS) void maf_write_kernel(const uint8_t* __restrict__ seq, const CsProb* __restrict__ probs,
                                                                      const uint4* __restrict__ recs, const MafBlock* __restrict__ blk, uint32_t nb,
                                                                      const unsigned long long* __restrict__ goff, unsigned long long chunk_bytes,
                                                                      uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t s_out[WFM_MAF_SLICE];
  __shared__ uint4 s_rec[MAF_STAGE];
  const int tid = threadIdx.x;
  const unsigned long long s0 = (unsigned long long)blockIdx.x * WFM_MAF_SLICE;
  if (s0 >= chunk_bytes) return;
  const unsigned long long chunk_base = blk[0].off;
  const unsigned long long s1 = s0 + WFM_MAF_SLICE < chunk_bytes ? s0 + WFM_MAF_SLICE : chunk_bytes;
  unsigned long long g = chunk_base + s0;
  const unsigned long long gend = chunk_base + s1;
  // the block the slice begins in: the last b with blk[b].off <= g (the blocks tile the chunk's bytes: every byte lies in one)
  uint32_t b = last_le(0u, nb, [&](uint32_t i) { return blk[i].off <= g; });
  // what is staged: records of problem st_k that cover the written columns [st_lo, st_hi) of it
  uint32_t st_k = 0xffffffffu, st_lo = 0, st_hi = 0, cnt = 0;
  while (g < gend) {  // (uniform over the workgroup)
    const MafBlock B = blk[b];
    const unsigned long long rel = g - B.off;
    if (rel >= 2ull * B.cols) { ++b; continue; }  // (b + 1 < nb: g < gend lies in a block)
    const uint32_t row = rel >= B.cols ? 1u : 0u;
    const uint32_t c = (uint32_t)rel - row * B.cols;
    const CsProb pr = probs[B.problem];
    const uint32_t bc0 = (uint32_t)((B.off - goff[B.problem]) >> 1);  // the block's first column in the problem: every block before it spent 2 bytes a column
    const uint32_t q0 = bc0 + c;
    unsigned long long seg = (unsigned long long)(B.cols - c);  // to the end of the row
    if (gend - g < seg) seg = gend - g;
    if (!(B.problem == st_k && q0 >= st_lo && q0 < st_hi)) {
      const uint4* R = recs + pr.rec_off;
      const uint32_t n = pr.n_runs;
      // the run column q0 lies in: the last r with R[r].z <= q0 (R[0].z = 0; the next slot's z lies behind q0, so the run is kept)
      const uint32_t r0 = last_le(0u, n, [&](uint32_t i) { return R[i].z <= q0; });
      cnt = n - r0 < (uint32_t)MAF_STAGE ? n - r0 : (uint32_t)MAF_STAGE;
      __syncthreads();  // (the records staged before are no longer read)
      for (uint32_t i = (uint32_t)tid; i < cnt; i += MAF_WRITE_THREADS) s_rec[i] = R[r0 + i];
      st_k = B.problem; st_lo = R[r0].z; st_hi = R[r0 + cnt].z;  // (slot n holds the problem's columns; st_hi > q0)
      __syncthreads();
    }
    if ((unsigned long long)(st_hi - q0) < seg) seg = st_hi - q0;
    const uint8_t* P = seq + pr.p_off;
    const uint8_t* T = seq + pr.t_off;
    const uint32_t at = (uint32_t)(g - chunk_base - s0);
    for (uint32_t j = (uint32_t)tid; j < (uint32_t)seg; j += MAF_WRITE_THREADS) {
      const uint32_t q = q0 + j;
      // (s_rec[0].z <= q < st_hi: the last record with z <= q writes columns, a break's z is its successor's)
      const uint4 rc = s_rec[last_le(0u, cnt, [&](uint32_t i) { return s_rec[i].z <= q; })];
      const uint32_t op = WFM_RUN_OP(rc.w), kk = q - rc.z;
      s_out[at + j] = row == 0 ? (op == OP_I ? (uint8_t)'-' : P[rc.x + kk]) : (op == OP_D ? (uint8_t)'-' : T[rc.y + kk]);
    }
    g += seg;
  }
  __syncthreads();
  // (the output block is a whole number of slices long: the last vector of the chunk's last slice may carry bytes nobody reads)
  const uint32_t nbytes = (uint32_t)(s1 - s0);
  for (uint32_t i = (uint32_t)tid * 16u; i < nbytes; i += MAF_WRITE_THREADS * 16u)
    *reinterpret_cast<uint4*>(out + s0 + i) = *reinterpret_cast<const uint4*>(s_out + i);
}

}  // namespace

void launch_maf_index(const uint32_t* runs, const CsProb* probs, int nprob, uint32_t split, void* recs, void* pre, unsigned long long* nblk,
                      unsigned long long* ncols, uint32_t* flags, hipStream_t st) {
  if (nprob <= 0) return;
  hipLaunchKernelGGL(maf_index_kernel, dim3((unsigned)nprob), dim3(MAF_THREADS), 0, st, runs, probs, split, (uint4*)recs, (uint2*)pre, nblk, ncols, flags);
}

void launch_maf_write(const uint8_t* seq, const CsProb* probs, const void* recs, const void* pre, const unsigned long long* nblk,
                      const unsigned long long* goff, const unsigned long long* boff, uint32_t ka, uint32_t kb, unsigned long long chunk_bytes,
                      void* blocks, uint32_t n_blocks, uint8_t* out, hipStream_t st) {
  if (kb <= ka || chunk_bytes == 0 || n_blocks == 0) return;
  hipLaunchKernelGGL(maf_blocks_kernel, dim3(kb - ka), dim3(MAF_THREADS), 0, st, probs, (const uint4*)recs, (const uint2*)pre, nblk, goff, boff, ka,
                     (MafBlock*)blocks);
  const unsigned slices = (unsigned)((chunk_bytes + WFM_MAF_SLICE - 1) / WFM_MAF_SLICE);
  hipLaunchKernelGGL(maf_write_kernel, dim3(slices), dim3(MAF_WRITE_THREADS), 0, st, seq, probs, (const uint4*)recs, (const MafBlock*)blocks, n_blocks, goff,
                     chunk_bytes, out);
}

}  // namespace wfm
