// wfa_base.h -- what every base-job kernel does the same way, whatever it keeps its rows in (r32:: / r128::wfa_base_kernel on a
// global-memory ring, wfa_base2_kernel on registers, wfa_base2t_kernel on tiles with wfa_base2t_finish_kernel behind it): the
// range of row 0 and of the rows after it, the result of a trivial job, the run-length writer and the walk back through pre / bt.
// ONE definition: every tie the walk resolves decides CIGAR bytes.  Device code only; included at wfm scope by wfa_kernels.hip
// (before its two inclusions of wfa_generic_inc.h) and by wfa_tile2.hip.
#ifndef WFM_WFA_BASE_H_
#define WFM_WFA_BASE_H_

#include "wfa_device.h"

namespace wfm {

__device__ __forceinline__ int rdlane(int v, int src) { return __builtin_amdgcn_readlane(v, src); }

// The rows of a base job.  Row 0: the diagonals the begin-free lengths allow (ends-free), or diagonal 0 alone.  Row s as the ring
// kernel keeps it -- the union of its sources' ranges, the I / D sources reaching one diagonal further -- in closed form for the
// default penalties: row s - 1 is among the sources (e2 = 1) and holds every older row, so a row is its predecessor and one
// diagonal more on either side, clipped to the problem and to the job's columns [klo, khi].  Empty: lo > hi.
struct BaseRows { int lo0, hi0, klo, khi; };
__device__ __forceinline__ BaseRows base_rows(const BaseJob& J) {
  const int kmin = J.kmin, kmax = J.kmin + J.width - 1;
  BaseRows R;
  if (J.endsfree) { R.lo0 = max(-J.pbf, kmin); R.hi0 = min(J.tbf, kmax); }
  else { R.lo0 = 0; R.hi0 = 0; }
  R.klo = max(-J.pl, kmin); R.khi = min(J.tl, kmax);
  return R;
}
__device__ __forceinline__ void base_row(const BaseRows& R, int s, int& lo, int& hi) { lo = max(R.lo0 - s, R.klo); hi = min(R.hi0 + s, R.khi); }

// trivial: all-D or all-I (wavefront_bialign_alignment trivial cases).  One thread calls it.
__device__ __forceinline__ BaseResult base_trivial_result(const BaseJob& J, uint32_t* __restrict__ rle) {
  BaseResult r; r.status = 0; r.cells = 0; r.nruns = 0; r.score = 0; r.pad_ = 0;
  const int len = J.type == 1 ? J.pl : J.tl;
  if (len > 0 && !J.score_only) { rle[J.rle_end - 1] = ((uint32_t)len << 2) | (uint32_t)(J.type == 1 ? OP_D : OP_I); r.nruns = 1; }
  return r;
}

struct RleWriter {
  uint32_t* base;  // entries are written at base[-1], base[-2], ...
  int n;
  int cur_op;
  uint32_t cur_len;
  bool writes;  // several lanes may keep the same writer in step; one of them stores
  __device__ void push(int op, int len) {
    if (len <= 0) return;
    if (op == cur_op) { cur_len += (uint32_t)len; return; }
    flush();
    cur_op = op; cur_len = (uint32_t)len;
  }
  __device__ void flush() {
    if (cur_len) { ++n; if (writes) base[-n] = (cur_len << 2) | (uint32_t)cur_op; }
    cur_len = 0; cur_op = -1;
  }
};

// wavefront_backtrace_affine over the rows a forward pass has left (pre: the offset of every M cell before its extension, bt: its decision byte; both
// addressed [score][diagonal] with the job's width): one wave, every lane with the same state, lane 0 writes.  The walk starts in the job's end
// component (M for ends-free) at score s on diagonal k_from with offset off_from.  Returns the number of runs written below rle[J.rle_end].
// Inside a gap the walk visits one cell per base and each visit is a dependent load of a decision byte; a patch begins with the ~1 kb end gap
// of its record, so those walks were most of the ring kernel's time.  The cells of a gap lie on a known line -- (score - j e, diagonal +- j) --
// so the 64 lanes read the next 64 decision bytes at once and the walk jumps to the first one that does not say "extension".
__device__ __forceinline__ int base_walk(const BaseJob& J, const DevPen pn, const int32_t* __restrict__ pre_base, const uint8_t* __restrict__ bt_base,
                                         uint32_t* __restrict__ rle, int s, int k_from, int off_from, int lane) {
  const int pl = J.pl, tl = J.tl;
  const int64_t width = J.width;
  RleWriter w; w.base = rle + J.rle_end; w.n = 0; w.cur_op = -1; w.cur_len = 0; w.writes = lane == 0;
  int comp = J.endsfree ? C_M : J.comp_end;
  int k = k_from;
  int off = off_from;
  int sc = s;
  int h = off, v = off - k;
  if (comp == C_M) {
    if (v < pl) w.push(OP_D, pl - v);
    if (h < tl) w.push(OP_I, tl - h);
  }
  while (v > 0 && h > 0 && sc > 0) {
    if (comp != C_M) {
      // a run of gap cells: j-th cell of the line, with the loop's own conditions
      const bool ins = comp == C_I1 || comp == C_I2;
      const int e = (comp == C_I1 || comp == C_D1) ? pn.e1 : pn.e2, o = (comp == C_I1 || comp == C_D1) ? pn.o1 : pn.o2;
      const unsigned mask = comp == C_I1 ? BT_I1_EXT : (comp == C_I2 ? BT_I2_EXT : (comp == C_D1 ? BT_D1_EXT : BT_D2_EXT));
      const int scj = sc - lane * e, kj = ins ? k - lane : k + lane;
      const bool alive = scj > 0 && (ins ? h - lane > 0 : v - lane > 0);
      const unsigned bj = alive ? bt_base[(int64_t)scj * width + kj] : 0u;
      const unsigned long long stop = __ballot(!(alive && (bj & mask)));
      const int j0 = stop ? (int)__builtin_ctzll(stop) : 64;  // cells 0 .. j0-1 continue the gap
      if (j0 > 0) {
        w.push(ins ? OP_I : OP_D, j0);
        sc -= j0 * e;
        if (ins) { k -= j0; off -= j0; } else k += j0;
        v = off - k; h = off;
      }
      if (j0 < 64) {
        if (!(v > 0 && h > 0 && sc > 0)) break;   // the walk ends inside the gap
        sc -= o + e; comp = C_M;                  // the cell that opened the gap
        w.push(ins ? OP_I : OP_D, 1);
        if (ins) { --k; --off; } else ++k;
        v = off - k; h = off;
      }
      continue;
    }
    // (round 6) A run of mismatches stays on its diagonal, x scores apart -- and between unrelated sequences (the patches that pass every
    // score budget) that is what a path is made of: thousands of cells, each a dependent load.  The 64 lanes read the decision byte and the
    // offset of the next 64 cells of that line at once; the walk goes through them from registers for as long as each one's source is the
    // mismatch.  (Measured: it is NOT what C2's 9.3 ms launches of the ring kernel are made of -- nor are the ring loads or the extension's
    // round trips to L2, both tried in LDS / batched four diagonals at a time and taken out again: ~4000 score steps at 2.3 us, ~250
    // instructions per wave and step over rows of 3.4 k diagonals.  DESIGN.md section 8.)
    const int scj = sc - lane * pn.x;
    const unsigned bj = scj > 0 ? (unsigned)bt_base[(int64_t)scj * width + k] : 0u;
    const int pj = scj > 0 ? pre_base[(int64_t)scj * width + k] : 0;
    bool stop = false;
    for (int j = 0; j < 64; ++j) {
      const unsigned b = (unsigned)rdlane((int)bj, j);
      const int pre = rdlane(pj, j);
      w.push(OP_M, off - pre);
      off = pre; v = off - k; h = off;
      if (v <= 0 || h <= 0) { stop = true; break; }
      const unsigned src = b & 7u;
      if (src == C_M) {
        sc -= pn.x; comp = C_M; w.push(OP_X, 1); --off;
        v = off - k; h = off;
        if (!(v > 0 && h > 0 && sc > 0)) break;  // (the walk's own condition: it ends here)
        continue;                                // the next cell of the line: lane j + 1 holds it
      }
      if (src == C_I1) { if (b & BT_I1_EXT) { sc -= pn.e1; comp = C_I1; } else { sc -= pn.o1 + pn.e1; comp = C_M; } w.push(OP_I, 1); --k; --off; }
      else if (src == C_I2) { if (b & BT_I2_EXT) { sc -= pn.e2; comp = C_I2; } else { sc -= pn.o2 + pn.e2; comp = C_M; } w.push(OP_I, 1); --k; --off; }
      else if (src == C_D1) { if (b & BT_D1_EXT) { sc -= pn.e1; comp = C_D1; } else { sc -= pn.o1 + pn.e1; comp = C_M; } w.push(OP_D, 1); ++k; }
      else { if (b & BT_D2_EXT) { sc -= pn.e2; comp = C_D2; } else { sc -= pn.o2 + pn.e2; comp = C_M; } w.push(OP_D, 1); ++k; }
      v = off - k; h = off;
      break;  // the path leaves the line
    }
    if (stop) break;
  }
  if (comp == C_M && v > 0 && h > 0) { const int nm = min(v, h); w.push(OP_M, nm); v -= nm; h -= nm; }
  if (v > 0) w.push(OP_D, v);
  if (h > 0) w.push(OP_I, h);
  w.flush();
  return w.n;
}

}  // namespace wfm
#endif
