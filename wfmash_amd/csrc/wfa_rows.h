// wfa_rows.h -- the diagonals a row of a BiWFA job holds, the diagonals a tile block covers and how that range is cut into tiles:
// ONE definition for the tile kernels (wfa_kernels.hip, wfa_tile2.hip), the host driver (wfa_host.hip) and its planners
// (wfa_plan.h).  No HIP header: plain C++ under g++, __host__ __device__ under hipcc.  If the host and a kernel disagreed on any
// of this a job would get too few tiles, or a single tile narrower than the range the kernel derives: wrong output, no error.
#ifndef WFM_WFA_ROWS_H_
#define WFM_WFA_ROWS_H_

#include <stdint.h>

// (forced inline on the device, as the kernels' own copies of these functions were: their code must not change with where they are defined)
#if defined(__HIPCC__)
#define WFM_ROWS_FN __host__ __device__ __forceinline__
#else
#define WFM_ROWS_FN inline
#endif

namespace wfm {

constexpr int SUB_NONE = 1 << 29;  // "no upper bound of the score is known" (BpJob::sub, TileJob::sub, P2Job::sub, Node::sub)

WFM_ROWS_FN int rows_min(int a, int b) { return a < b ? a : b; }
WFM_ROWS_FN int rows_max(int a, int b) { return a > b ? a : b; }

// Row ranges in closed form.  Score s reaches the diagonals [-s, s] (every change of diagonal costs at least e2 = 1), clipped to
// the problem -- and, when an upper bound `sub` of the problem's score is known (a BiWFA child is handed its score by its
// parent; a root may come with a hint), only the diagonals from which the end diagonal kinv = tl - pl is still within
// reach: |k - kinv| <= sub - s.  A cell outside cannot lie on an alignment of score <= sub, and no cell inside depends on one
// outside (a predecessor is one diagonal away at most and at least e2 cheaper), so the cells inside keep their exact
// values and every breakpoint of score <= sub is found where the reference finds it: the phase-1 trigger (the running
// maxima of the antidiagonals) can only fire LATER without the cells outside, never after a pair of cells of a real
// overlap exists, and phase 2 tests the rows that triggered.  For a record with 1 kb end gaps this removes half the cells.
struct Rng { int pl, tl, kb_lo, kb_hi; };  // kb_lo = kinv - sub, kb_hi = kinv + sub
WFM_ROWS_FN Rng make_rng(int pl, int tl, int sub) { Rng r; r.pl = pl; r.tl = tl; r.kb_lo = (tl - pl) - sub; r.kb_hi = (tl - pl) + sub; return r; }
WFM_ROWS_FN int rng_lo(const Rng& r, int s) { return rows_max(rows_max(-r.pl, -s), r.kb_lo + s); }
WFM_ROWS_FN int rng_hi(const Rng& r, int s) { return rows_min(rows_min(r.tl, s), r.kb_hi - s); }
// The diagonals a tile pass over the scores (s_from, s_to] has to hold: every bound at its loosest score of the block -- and
// the score bound as it stood 25 scores BEFORE the block: the edge a score bound sets moves inwards, so the rows the block
// starts from are wider than its own, and the snapshot it leaves behind must hold every row of the last 26 scores whole --
// a short last block (one that stops at the meeting point after a few steps) hands rows older than its own first row to
// phase 2, which reads each row over its full range.  (Until round 3 the bound was taken at s_from: the cells of the older
// rows beyond it never reached the output ring, and phase 2 read whatever the ring held there.  With the slack the bounds
// used to carry -- 56 for a child, 200 for a caller's guess -- those cells could not complete an overlap within the bound
// and stale values of the same job never made one up; an exact bound on a small batch, where rings are reused across
// jobs, did: a false breakpoint one point under the optimum.)
constexpr int RNG_BACK = 25;
constexpr int SNAP_ROWS = RNG_BACK + 1;  // rows of a snapshot that phase 2 reads: scores sd - RNG_BACK .. sd (the default penalties' scope)
constexpr int KEEP_ROWS = SNAP_ROWS + 6;  // rows of a kept snapshot (parent reuse): M of scores s - RNG_BACK .. s, I1 / D1 of s and s - 1, I2 / D2 of s -- what a block loads
constexpr int P2_BACK = SNAP_ROWS + 1;   // the window of phase-2 rows begins this far before the earlier direction's score: the snapshot's rows and one of margin
WFM_ROWS_FN void rng_block(const Rng& r, int s_from, int s_to, int& L, int& R) {
  L = rows_max(rows_max(-r.pl, -s_to), r.kb_lo + s_from - RNG_BACK);
  R = rows_min(rows_min(r.tl, s_to), r.kb_hi - s_from + RNG_BACK);
}

// Does every diagonal of [k_first, k_last] lie inside its row at EVERY score of [s_first, s_last]?  The two end rows decide it.  A diagonal k is
// inside row s where -pl <= k <= tl (no matter of s), |k| <= s and s <= min(k - kb_lo, kb_hi - k): the triangle only ever lets a diagonal
// in as the score grows, the score bound's cone only ever lets it out, so the scores at which k is inside are one interval and k is inside
// at every score between two at which it is.  A row's range is an interval of diagonals as well, so the span is inside a row when its two
// end diagonals are.  Exact, not only sufficient: a span that fails at an end row is not inside at that row.  (No row of a negative score
// holds a cell -- rng_lo > rng_hi there -- and an empty span or an empty interval of scores is never "inside".)
WFM_ROWS_FN bool rng_interior(const Rng& r, int k_first, int k_last, int s_first, int s_last) {
  return k_first <= k_last && s_first <= s_last && k_first >= rows_max(rng_lo(r, s_first), rng_lo(r, s_last)) &&
         k_last <= rows_min(rng_hi(r, s_first), rng_hi(r, s_last));
}
// The two tests by which a wave of the packed tile kernel (wfa_tile2.hip: two diagonals a lane, WAVE_DIAGS a wave, the first of them kw) takes
// its lean snapshot paths, from wave-uniform values alone.  Load: every lane's pair is the tile's and inside every row the block starts from
// (M of scores s0 - RNG_BACK .. s0; the gap rows loaded are of s0 and s0 - 1).  Store: the block wrote a whole snapshot (Tn >= SNAP_ROWS steps),
// and the part of the wave that lies in the tile's core -- all of it, or what a halo leaves of the tile's first and last wave -- is made of whole
// lanes (a lane's pair is the core's or it is not: the part begins and ends an even number of diagonals from kw) and is inside every row of the
// snapshot.  The lanes of that part then store their pairs without a test; the others store nothing, as in the general form.
constexpr int WAVE_DIAGS = 128;
WFM_ROWS_FN bool tile_wave_lean_load(const Rng& r, int kw, int kmax, int s0) {
  return kw + WAVE_DIAGS - 1 <= kmax && s0 - RNG_BACK >= 0 && rng_interior(r, kw, kw + WAVE_DIAGS - 1, s0 - RNG_BACK, s0);
}
WFM_ROWS_FN bool tile_wave_lean_store(const Rng& r, int kw, int core_lo, int core_hi, int s_end, int Tn) {
  const int a = rows_max(kw, core_lo), b = rows_min(kw + WAVE_DIAGS - 1, core_hi);
  return Tn >= SNAP_ROWS && a <= b && ((a - kw) & 1) == 0 && ((b + 1 - kw) & 1) == 0 && s_end - RNG_BACK >= 0 &&
         rng_interior(r, a, b, s_end - RNG_BACK, s_end);
}

// a workgroup of a tile launch
struct TileTask {
  int32_t job, dir;
  int32_t core_lo, core_hi;            // in memory: (tile index, tile width); the kernels turn it into the inclusive
                                       // diagonal range owned by the tile for the block at hand
};
// A block's range [L, R] is cut into tiles of `core` diagonals from its own left end, so every tile but the last is full:
// tile idx owns [lo, hi] (lo > R: the block has no such tile), and the range needs tiles_for() of them.
WFM_ROWS_FN void tile_span(int L, int R, int idx, int core, int* lo, int* hi) {
  const int first = L + idx * core;
  *lo = first;
  *hi = rows_min(R, first + core - 1);
}
WFM_ROWS_FN int tiles_for(int L, int R, int core) { return R >= L ? (R - L + core) / core : 0; }

}  // namespace wfm
#endif
