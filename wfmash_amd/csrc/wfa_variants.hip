// wfa_variants.hip -- wfm_call_variants: the substitutions, insertions and deletions of every problem's runs as VCF-style records, called on
// the device (include/wfmash_hip.h states the grammar).  Only the seqset's forward BYTE copies are read, and the records are called from
// the runs, never from a comparison.  The shape is wfa_cs.hip's (the scan and the searches are wfa_scan.h's).  Two kernels:
//
//   var_index_kernel  one workgroup per problem.  Rounds of 256 runs with a carry: the exclusive prefix of every run's pattern advance, text
//                     advance, records (X: L; a called gap: 1) and allele bytes (X: 2 L; a called gap: L + 2), the structural test of
//                     cs_index_kernel (WFM_VAR_SPANS) and one record per run: where its bases begin in the pattern and the text, where its
//                     allele bytes begin in the problem's, the run itself, and -- in a second table -- the index of its first record in the
//                     problem's.  A gap is called unless it is the problem's first or last run or no pattern base lies before it; those are
//                     counted.  The problem's totals go to the host, which takes the prefix sums over the problems.
//   var_write_kernel  one workgroup per WFM_VAR_SLICE allele bytes of a chunk of problems; every lane owns allele BYTES.  The workgroup
//                     finds the problem and the run its slice begins in by binary search and walks on from there, VAR_STAGE run records
//                     at a time staged in LDS; a lane finds its run among them and derives its byte from (run, offset within the run).  The
//                     lane that owns a record's first allele byte also writes the record (32 bytes, two 16-byte stores), the MASKED bit
//                     included: so a 70 kb deletion is 70 k lanes' work, and a record may lie in one slice and its last bytes two slices on.
//                     The slice is assembled in LDS and leaves in 16-byte stores.
// No atomics: two calls give the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wfmash_hip.h"
#include "wfa_device.h"
#include "wfa_scan.h"

namespace wfm {
namespace {

constexpr int VAR_THREADS = 256;
constexpr int VAR_WAVES = VAR_THREADS / 64;
constexpr int VAR_WRITE_THREADS = 1024;  // a slice is 16 rounds of one byte per lane, as in cs_write_kernel
constexpr int VAR_STAGE = 1024;          // run records staged at a time: 16 KB + 4 KB of LDS beside the slice's 16 KB (36 KB of a CU's 160 KB: two workgroups' 32 waves fill the CU first)

__global__ __launch_bounds__(VAR_THREADS) void var_index_kernel(const uint32_t* __restrict__ runs, const CsProb* __restrict__ probs,
                                                                uint4* __restrict__ recs, uint32_t* __restrict__ rpre,
                                                                unsigned long long* __restrict__ tot_bytes, unsigned long long* __restrict__ tot_recs,
                                                                uint32_t* __restrict__ end_gaps, uint32_t* __restrict__ flags) {
  const CsProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x;
  if (pr.skip) {
    if (tid == 0) { flags[blockIdx.x] = WFM_VAR_NOT_DONE; tot_bytes[blockIdx.x] = 0; tot_recs[blockIdx.x] = 0; end_gaps[blockIdx.x] = 0; }
    return;
  }
  __shared__ unsigned long long wtot[VAR_WAVES];
  __shared__ uint32_t s_bad;
  if (tid == 0) s_bad = 0;
  const uint32_t* my = runs + pr.run_off;
  uint4* rec = recs + pr.rec_off;
  uint32_t* rp = rpre + pr.rec_off;
  const uint32_t n = pr.n_runs;
  unsigned long long carry_p = 0, carry_t = 0, carry_r = 0, carry_o = 0, ends = 0;
  bool bad = false;
  for (uint32_t base = 0; base < n; base += VAR_THREADS) {
    const uint32_t r = base + (uint32_t)tid;
    const bool valid = r < n;
    const uint32_t run = valid ? my[r] : 0u;
    const uint32_t len = WFM_RUN_LEN(run), op = WFM_RUN_OP(run);
    const unsigned long long ap = (valid && op != OP_I) ? len : 0u, at = (valid && op != OP_D) ? len : 0u;
    if (valid && (len == 0 || (r > 0 && WFM_RUN_OP(my[r - 1]) == op))) bad = true;
    unsigned long long tp, tt, tr, to;
    const unsigned long long pp = carry_p + block_excl<VAR_WAVES>(ap, wtot, &tp);
    const unsigned long long tx = carry_t + block_excl<VAR_WAVES>(at, wtot, &tt);
    // a gap is called where it is interior and has its anchor, the pattern base before it
    const bool gap = valid && (op == OP_I || op == OP_D);
    const bool called = gap && r > 0 && r + 1 < n && pp > 0;
    if (gap && !called) ++ends;
    const unsigned long long ar = !valid ? 0ull : op == OP_X ? (unsigned long long)len : called ? 1ull : 0ull;
    const unsigned long long ao = !valid ? 0ull : op == OP_X ? 2ull * len : called ? 2ull + len : 0ull;
    const unsigned long long rr = carry_r + block_excl<VAR_WAVES>(ar, wtot, &tr);
    const unsigned long long oo = carry_o + block_excl<VAR_WAVES>(ao, wtot, &to);
    // (a problem whose totals pass its sequences' lengths, or 32 bits, is flagged below and its records are never read)
    if (valid) { rec[r] = make_uint4((uint32_t)pp, (uint32_t)tx, (uint32_t)oo, run); rp[r] = (uint32_t)rr; }
    carry_p += tp; carry_t += tt; carry_r += tr; carry_o += to;
  }
  unsigned long long all_ends;
  (void)block_excl<VAR_WAVES>(ends, wtot, &all_ends);
  if (bad) s_bad = 1;  // (every writer stores the same value)
  __syncthreads();
  if (tid == 0) {
    const bool spans = s_bad || carry_p != (unsigned long long)pr.plen || carry_t != (unsigned long long)pr.tlen || carry_o >= (1ull << 32);
    flags[blockIdx.x] = spans ? WFM_VAR_SPANS : 0u;
    tot_bytes[blockIdx.x] = spans ? 0ull : carry_o;
    tot_recs[blockIdx.x] = spans ? 0ull : carry_r;
    end_gaps[blockIdx.x] = spans ? 0u : (uint32_t)all_ends;
  }
}

__device__ __forceinline__ bool var_acgt(uint8_t c) {
  const uint8_t u = c & 0xdfu;  // (clears the bit that tells 'a' from 'A': u == 'A' exactly for those two bytes)
  return u == 'A' || u == 'C' || u == 'G' || u == 'T';
}

__device__ __forceinline__ void var_store(uint4* __restrict__ v, uint32_t problem, uint32_t kind, uint32_t p, uint32_t t, uint32_t ref_len,
                                          uint32_t alt_len, unsigned long long off) {
  v[0] = make_uint4(problem, kind, p, t);
  v[1] = make_uint4(ref_len, alt_len, (uint32_t)off, (uint32_t)(off >> 32));
}

// goff / voff: the offsets of the call's problems in *alleles and in *vars, n + 1 of each; the chunk is the problems [ka, kb), whose allele
// bytes are [goff[ka], goff[ka] + chunk_bytes) of *alleles and the bytes [0, chunk_bytes) of `out` here, and whose records are
// [voff[ka], voff[kb]) of *vars and begin at vars[0] here (two uint4 each)
__global__ __launch_bounds__(VAR_WRITE_THREADS) void var_write_kernel(const uint8_t* __restrict__ seq, const CsProb* __restrict__ probs,
                                                                      const uint4* __restrict__ recs, const uint32_t* __restrict__ rpre,
                                                                      const unsigned long long* __restrict__ goff,
                                                                      const unsigned long long* __restrict__ voff, uint32_t ka, uint32_t kb,
                                                                      unsigned long long chunk_bytes, uint8_t* __restrict__ out,
                                                                      uint4* __restrict__ vars) {
  __shared__ __attribute__((aligned(16))) uint8_t s_out[WFM_VAR_SLICE];
  __shared__ uint4 s_rec[VAR_STAGE];
  __shared__ uint32_t s_rpre[VAR_STAGE];
  const int tid = threadIdx.x;
  const unsigned long long s0 = (unsigned long long)blockIdx.x * WFM_VAR_SLICE;
  if (s0 >= chunk_bytes) return;
  const unsigned long long chunk_base = goff[ka], chunk_vars = voff[ka];
  const unsigned long long s1 = s0 + WFM_VAR_SLICE < chunk_bytes ? s0 + WFM_VAR_SLICE : chunk_bytes;
  unsigned long long g = chunk_base + s0;
  const unsigned long long gend = chunk_base + s1;
  // the problem the slice begins in: the last k in [ka, kb) with goff[k] <= g (goff[kb] >= gend > g, so its own end lies behind g)
  uint32_t k = last_le(ka, kb, [&](uint32_t i) { return goff[i] <= g; });
  while (g < gend) {  // (uniform over the workgroup)
    const unsigned long long pb = goff[k], pe = goff[k + 1];
    if (pe <= g) { ++k; continue; }  // a problem without alleles
    const CsProb pr = probs[k];
    const uint4* R = recs + pr.rec_off;
    const uint32_t* RP = rpre + pr.rec_off;
    const uint32_t n = pr.n_runs, rel = (uint32_t)(g - pb);
    // the run the byte g lies in: the last r with R[r].z <= rel.  Runs without bytes (M, uncalled gaps) share their offset with the run
    // behind them, so the last one at an offset is the one that owns it, and pe > g says some run does: the walk always advances.
    // Behind the slice's first problem the walk arrives at a problem's first byte, and the search (a chain of dependent loads per
    // problem) is spared where staging from run 0 is known to reach a run with bytes
    const bool from_first = rel == 0 && (n <= (uint32_t)VAR_STAGE || R[VAR_STAGE].z > 0);
    const uint32_t r0 = from_first ? 0u : last_le(0u, n, [&](uint32_t i) { return R[i].z <= rel; });
    const uint32_t cnt = n - r0 < (uint32_t)VAR_STAGE ? n - r0 : (uint32_t)VAR_STAGE;
    __syncthreads();  // (the records of the round before are no longer read)
    for (uint32_t i = (uint32_t)tid; i < cnt; i += VAR_WRITE_THREADS) { s_rec[i] = R[r0 + i]; s_rpre[i] = RP[r0 + i]; }
    const unsigned long long staged_end = pb + (r0 + cnt < n ? (unsigned long long)R[r0 + cnt].z : pe - pb);
    const unsigned long long seg_end = staged_end < gend ? staged_end : gend;
    __syncthreads();
    const uint8_t* P = seq + pr.p_off;
    const uint8_t* T = seq + pr.t_off;
    uint4* V = vars + 2 * (voff[k] - chunk_vars);
    for (unsigned long long q = g + (unsigned long long)tid; q < seg_end; q += VAR_WRITE_THREADS) {
      const uint32_t rq = (uint32_t)(q - pb);
      const uint32_t at = last_le(0u, cnt, [&](uint32_t i) { return s_rec[i].z <= rq; });  // s_rec[0].z <= rq (< the offset behind the staged runs)
      const uint4 rc = s_rec[at];
      const uint32_t len = WFM_RUN_LEN(rc.w), op = WFM_RUN_OP(rc.w), o = rq - rc.z;
      uint8_t byte;
      if (op == OP_X) {
        const uint32_t j = o >> 1;
        const uint8_t ref = P[rc.x + j], alt = T[rc.y + j];
        byte = (o & 1u) ? alt : ref;
        if (!(o & 1u))
          var_store(V + 2ull * (s_rpre[at] + j), k, WFM_VAR_SNV | ((var_acgt(ref) && var_acgt(alt)) ? 0u : WFM_VAR_MASKED), rc.x + j, rc.y + j, 1u, 1u, q);
      } else if (op == OP_I) {  // REF = the anchor, ALT = the anchor + the L text bytes (a called gap has rc.x >= 1)
        byte = o < 2u ? P[rc.x - 1u] : T[rc.y + o - 2u];
        if (o == 0) var_store(V + 2ull * s_rpre[at], k, WFM_VAR_INS, rc.x - 1u, rc.y, 1u, len + 1u, q);
      } else {                  // OP_D (an M run has no bytes): REF = the anchor + the L pattern bytes, ALT = the anchor
        byte = o <= len ? P[rc.x - 1u + o] : P[rc.x - 1u];
        if (o == 0) var_store(V + 2ull * s_rpre[at], k, WFM_VAR_DEL, rc.x - 1u, rc.y, len + 1u, 1u, q);
      }
      s_out[(uint32_t)(q - chunk_base - s0)] = byte;
    }
    g = seg_end;
  }
  __syncthreads();
  // (the allele block is a whole number of slices long: the last vector of the chunk's last slice may carry bytes nobody reads)
  const uint32_t nbytes = (uint32_t)(s1 - s0);
  for (uint32_t i = (uint32_t)tid * 16u; i < nbytes; i += VAR_WRITE_THREADS * 16u)
    *reinterpret_cast<uint4*>(out + s0 + i) = *reinterpret_cast<const uint4*>(s_out + i);
}

}  // namespace

void launch_var_index(const uint32_t* runs, const CsProb* probs, int nprob, void* recs, uint32_t* rpre, unsigned long long* tot_bytes,
                      unsigned long long* tot_recs, uint32_t* end_gaps, uint32_t* flags, hipStream_t st) {
  if (nprob <= 0) return;
  hipLaunchKernelGGL(var_index_kernel, dim3((unsigned)nprob), dim3(VAR_THREADS), 0, st, runs, probs, (uint4*)recs, rpre, tot_bytes, tot_recs, end_gaps, flags);
}

void launch_var_write(const uint8_t* seq, const CsProb* probs, const void* recs, const uint32_t* rpre, const unsigned long long* goff,
                      const unsigned long long* voff, uint32_t ka, uint32_t kb, unsigned long long chunk_bytes, uint8_t* out, void* vars,
                      hipStream_t st) {
  if (chunk_bytes == 0) return;
  const unsigned blocks = (unsigned)((chunk_bytes + WFM_VAR_SLICE - 1) / WFM_VAR_SLICE);
  hipLaunchKernelGGL(var_write_kernel, dim3(blocks), dim3(VAR_WRITE_THREADS), 0, st, seq, probs, (const uint4*)recs, rpre, goff, voff, ka, kb, chunk_bytes, out,
                     (uint4*)vars);
}

}  // namespace wfm
