// wfa_optcheck.hip -- wfm_check_optimal: the optimal gap-affine-2-piece price of every problem of a seqset by a textbook minimising
// DP over cells (i = pattern index, j = text index), restricted to a band of diagonals k = j - i (include/wfmash_hip.h; the band:
// wfa_optband.h).
//
// Like wfa_check.hip it shares nothing with the aligners: no wavefront offsets, no cell step, no walk back.  It reads the seqset's
// forward BYTE copies (never the 2-bit mirror) and compares bytes as bytes.
//
// One workgroup per problem, rows i = 0 .. plen in sequence.  A tile is THREADS x C consecutive diagonals, thread t owns C of them.
// In diagonal coordinates
//   the diagonal move (i-1, j-1) -> (i, j) stays on the thread's own diagonal,
//   the vertical gap F (from (i-1, j)) comes from diagonal k + 1 of the previous row: the thread's next slot, or the first slot of
//     thread t + 1 (through LDS; through the row block in the memory form),
//   the horizontal gap E (from (i, j-1)) is the one dependency inside a row.  With H' = min(diagonal move, F1, F2, start value):
//     E1[j] = min over j' < j of H'[j'] + o1 + e1 (j - j')  =  e1 rel(j) + min over j' < j of (H'[j'] + o1 - e1 rel(j')),
//     rel = the slot's index in the tile (so the linear term stays small); piece 2 likewise.  Opening a gap from a cell that was
//     itself reached by that gap is dominated, so H' is enough.  Two exclusive prefix minima per row: inside the thread, across
//     the wave by DPP, across the waves through LDS, across tiles by a carry that moves by e x tile per tile.
// Rows of a band of up to WFM_OPT_REG_MAX diagonals stay in registers: 256 threads x 1 diagonal (WFM_OPT_BAND_C1), 256 x 4
// (WFM_OPT_BAND_C4), 512 x 8 (WFM_OPT_REG_MAX).  A wider band keeps H, F1, F2 of its row in a block of the device heap (L2 resident:
// 12 bytes per diagonal) and walks it in tiles of WFM_OPT_REG_MAX diagonals, 1024 threads x 4.  Values saturate at 2^29 ("no path");
// penalties are at most 32767, so nothing leaves 32 bits.  Two barriers per row and tile: one for the waves' minima, one before the
// row is read as the previous one.
// No byte outside [0, plen) / [0, tlen) is read; the row block is indexed inside [0, 3 (tiles x tile + 1)).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wfmash_hip.h"
#include "wfa_device.h"

namespace wfm {
namespace {

constexpr int OC_THREADS = 256;        // workgroup of the two narrow register forms (1 and 4 diagonals per thread)
constexpr int OC_THREADS_WIDE = 512;   // ... of the widest register form (8 per thread)
constexpr int OC_THREADS_MEM = 1024;   // ... of the memory form (4 per thread, tiles of WFM_OPT_REG_MAX diagonals)
constexpr int OC_INF = 1 << 29;

__device__ __forceinline__ int sat(int v) { return min(v, OC_INF); }
// the text byte under column j (byte j - 1), from an index clamped into the text: a column without a byte (j < 1: no diagonal move ends
// there; j > tlen: outside the matrix) gets some byte of the text that nothing uses.  Unconditional on purpose: a branch around the load
// would make every byte of a thread's slots wait for the one before.  tlen > 0 (the same for every thread).
__device__ __forceinline__ int text_byte(const uint8_t* T, int tlen, int j) { return (int)T[min(max(j - 1, 0), tlen - 1)]; }

// inclusive prefix minimum over the wave's 64 lanes, by DPP: Hillis-Steele inside each row of 16 lanes (a lane without a source keeps
// "no path"), then lane 15 of rows 0 and 2 into rows 1 and 3, then lane 31 into rows 2 and 3
__device__ __forceinline__ int wave_prefix_min(int x) {
  x = min(x, __builtin_amdgcn_update_dpp(OC_INF, x, 0x111, 0xf, 0xf, false));  // row_shr:1
  x = min(x, __builtin_amdgcn_update_dpp(OC_INF, x, 0x112, 0xf, 0xf, false));  // row_shr:2
  x = min(x, __builtin_amdgcn_update_dpp(OC_INF, x, 0x114, 0xf, 0xf, false));  // row_shr:4
  x = min(x, __builtin_amdgcn_update_dpp(OC_INF, x, 0x118, 0xf, 0xf, false));  // row_shr:8
  x = min(x, __builtin_amdgcn_update_dpp(OC_INF, x, 0x142, 0xa, 0xf, false));  // row_bcast:15
  x = min(x, __builtin_amdgcn_update_dpp(OC_INF, x, 0x143, 0xc, 0xf, false));  // row_bcast:31
  return x;
}
// the value of the lane before (lane 0: "no path")
__device__ __forceinline__ int from_lane_before(int x) { return __builtin_amdgcn_update_dpp(OC_INF, x, 0x138, 0xf, 0xf, false); }  // wave_shr:1

template <int C, bool MEM, int THREADS>
__global__ __launch_bounds__(THREADS) void optcheck_kernel(const uint8_t* __restrict__ seq, const OptProb* __restrict__ probs,
                                                              int32_t* __restrict__ rows, int32_t* __restrict__ out, DevPen pen) {
  constexpr int TILE = THREADS * C;
  constexpr int WAVES = THREADS / 64;
  const OptProb pr = probs[blockIdx.x];
  const uint8_t* P = seq + pr.p_off;
  const uint8_t* T = seq + pr.t_off;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int plen = pr.plen, tlen = pr.tlen;
  const int W = pr.band_hi - pr.band_lo + 1;
  const int ntiles = MEM ? (W + TILE - 1) / TILE : 1;
  const int Wp = ntiles * TILE + 1;  // (memory form) slots of one of the three row arrays: one beyond the last tile, never written
  int32_t* rH = MEM ? rows + pr.row_off : nullptr;
  int32_t* rF1 = MEM ? rH + Wp : nullptr;
  int32_t* rF2 = MEM ? rF1 + Wp : nullptr;
  __shared__ int s_nb[3][THREADS];      // register form: H, F1, F2 of every thread's first diagonal, previous row
  __shared__ int s_wt[2][2][WAVES];     // [parity][piece][wave]: the waves' minima of a tile
  __shared__ int s_best[WAVES];
  int H[C], F1[C], F2[C], tb[C];
#pragma unroll
  for (int c = 0; c < C; ++c) { H[c] = F1[c] = F2[c] = OC_INF; tb[c] = 0; }
  if (MEM) {
    for (int q = tid; q < 3 * Wp; q += THREADS) rH[q] = OC_INF;
  } else {
    s_nb[0][tid] = s_nb[1][tid] = s_nb[2][tid] = OC_INF;
    // the text bytes under the thread's diagonals in row 0 (slot c: column j = k + c, byte j - 1); they slide by one per row
    const int j0 = pr.band_lo + tid * C;
    if (tlen > 0) {
#pragma unroll
      for (int c = 0; c < C; ++c) tb[c] = text_byte(T, tlen, j0 + c);
    }
  }
  __syncthreads();
  const int oe1 = pen.o1 + pen.e1, oe2 = pen.o2 + pen.e2;
  int best = OC_INF;
  int par = 0;
  int pb = 0, pb_next = plen > 0 ? (int)P[0] : 0;  // the pattern byte of the row (the same for every thread), fetched a row ahead
  for (int i = 0; i <= plen; ++i) {
    pb = pb_next;                              // row i compares P[i - 1] (row 0 compares nothing)
    if (i < plen) pb_next = (int)P[i];
    int carry1 = OC_INF, carry2 = OC_INF;      // the row's prefix minima up to the tile, relative to the tile's first slot
    for (int t = 0; t < ntiles; ++t) {
      const int d0 = t * TILE + tid * C;       // the thread's first slot in the band
      const int j0 = i + pr.band_lo + d0;      // ... and its column in this row
      int nH, nF1, nF2;                        // previous row, diagonal one above the thread's last
      if (MEM) {
#pragma unroll
        for (int c = 0; c < C; ++c) { H[c] = rH[d0 + c]; F1[c] = rF1[d0 + c]; F2[c] = rF2[d0 + c]; }
        if (tlen > 0) {
#pragma unroll
          for (int c = 0; c < C; ++c) tb[c] = text_byte(T, tlen, j0 + c);
        }
        nH = rH[d0 + C]; nF1 = rF1[d0 + C]; nF2 = rF2[d0 + C];
      } else {
        const bool has = tid + 1 < THREADS;
        nH = has ? s_nb[0][tid + 1] : OC_INF; nF1 = has ? s_nb[1][tid + 1] : OC_INF; nF2 = has ? s_nb[2][tid + 1] : OC_INF;
      }
      int run1 = OC_INF, run2 = OC_INF;        // min of H' + o - e rel over the thread's earlier slots
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int j = j0 + c, rel = tid * C + c;
        const bool inmat = j >= 0 && j <= tlen && d0 + c < W;
        const int hn = c + 1 < C ? H[c + 1] : nH, f1n = c + 1 < C ? F1[c + 1] : nF1, f2n = c + 1 < C ? F2[c + 1] : nF2;
        int f1 = sat(min(hn + oe1, f1n + pen.e1));
        int f2 = sat(min(hn + oe2, f2n + pen.e2));
        const int hd = (i > 0 && j > 0) ? H[c] + (pb == tb[c] ? 0 : pen.x) : OC_INF;
        const int sv = ((i == 0 && j <= pr.tbf) || (j == 0 && i <= pr.pbf)) ? 0 : OC_INF;
        int hp = sat(min(min(hd, sv), min(f1, f2)));
        if (!inmat) { hp = OC_INF; f1 = OC_INF; f2 = OC_INF; }
        const int hl = min(hp, sat(min(run1 + pen.e1 * rel, run2 + pen.e2 * rel)));
        run1 = min(run1, hp + pen.o1 - pen.e1 * rel);
        run2 = min(run2, hp + pen.o2 - pen.e2 * rel);
        H[c] = hl; F1[c] = f1; F2[c] = f2;
      }
      // the wave's exclusive prefix minima of the threads' minima, and its total
      const int in1 = wave_prefix_min(run1), in2 = wave_prefix_min(run2);
      const int ex1 = from_lane_before(in1), ex2 = from_lane_before(in2);
      if (lane == 63) { s_wt[par][0][wave] = in1; s_wt[par][1][wave] = in2; }
      __syncthreads();
      int c1 = min(carry1, ex1), c2 = min(carry2, ex2), all1 = carry1, all2 = carry2;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) {
        const int w1 = s_wt[par][0][w], w2 = s_wt[par][1][w];
        if (w < wave) { c1 = min(c1, w1); c2 = min(c2, w2); }
        all1 = min(all1, w1); all2 = min(all2, w2);
      }
      par ^= 1;  // (the next tile's minima go to the other half: a slow thread may still be reading this one)
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int j = j0 + c, rel = tid * C + c;
        const bool inmat = j >= 0 && j <= tlen && d0 + c < W;
        const int h = inmat ? min(H[c], sat(min(c1 + pen.e1 * rel, c2 + pen.e2 * rel))) : OC_INF;
        H[c] = h;
        const bool at_end = (j == tlen && i >= plen - pr.pef) || (i == plen && j >= tlen - pr.tef);
        best = min(best, (inmat && at_end) ? h : OC_INF);
      }
      if (MEM) {
#pragma unroll
        for (int c = 0; c < C; ++c) { rH[d0 + c] = H[c]; rF1[d0 + c] = F1[c]; rF2[d0 + c] = F2[c]; }
        carry1 = sat(all1 + pen.e1 * TILE); carry2 = sat(all2 + pen.e2 * TILE);
      } else {
        s_nb[0][tid] = H[0]; s_nb[1][tid] = F1[0]; s_nb[2][tid] = F2[0];
        // slide the text bytes: slot c of the next row stands on column j0 + c + 1
#pragma unroll
        for (int c = 0; c + 1 < C; ++c) tb[c] = tb[c + 1];
        if (tlen > 0) tb[C - 1] = text_byte(T, tlen, j0 + C);
      }
    }
    __syncthreads();  // the row is whole (LDS, or the row block) before anyone reads it as the previous one
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) best = min(best, __shfl_down(best, d, 64));
  if (lane == 0) s_best[wave] = best;
  __syncthreads();
  if (tid == 0) {
    int b = s_best[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) b = min(b, s_best[w]);
    out[blockIdx.x] = b >= OC_INF ? -1 : b;
  }
}

}  // namespace

void launch_optcheck(const uint8_t* seq, const OptProb* probs, int nprob, int form, int32_t* rows, int32_t* out, DevPen pen, hipStream_t st) {
  if (nprob <= 0) return;
  // (measured on 64 problems each: the widest register form runs 1.4 x faster with 512 threads x 8 diagonals than with 256 x 16, the memory
  // form 1.7 x faster with 1024 x 4 -- more waves per SIMD to hide the barriers and the row block's loads behind; profiles/verify_optimal.md)
  static_assert(WFM_OPT_BAND_C1 == OC_THREADS && WFM_OPT_BAND_C4 == 4 * OC_THREADS && WFM_OPT_REG_MAX == 8 * OC_THREADS_WIDE &&
                WFM_OPT_REG_MAX == 4 * OC_THREADS_MEM, "the widths of the header are the kernel's");
  const dim3 g((unsigned)nprob);
  if (form == 0) hipLaunchKernelGGL((optcheck_kernel<1, false, OC_THREADS>), g, dim3(OC_THREADS), 0, st, seq, probs, rows, out, pen);
  else if (form == 1) hipLaunchKernelGGL((optcheck_kernel<4, false, OC_THREADS>), g, dim3(OC_THREADS), 0, st, seq, probs, rows, out, pen);
  else if (form == 2) hipLaunchKernelGGL((optcheck_kernel<8, false, OC_THREADS_WIDE>), g, dim3(OC_THREADS_WIDE), 0, st, seq, probs, rows, out, pen);
  else hipLaunchKernelGGL((optcheck_kernel<4, true, OC_THREADS_MEM>), g, dim3(OC_THREADS_MEM), 0, st, seq, probs, rows, out, pen);
}

}  // namespace wfm
