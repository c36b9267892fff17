// wfa_plan.h -- the arithmetic of the BiWFA level driver (wfa_host.hip) that needs no device: how large a wavefront ring is, the
// geometry of a banded ring, which ring a job gets under the memory budget (plan_ring), and how a problem's runs become its op
// string (expand_runs).  Host only, no HIP; the CPU suite reaches it through wfmh_test_ring_plan / wfmh_test_expand_runs
// (tests/test_ring_plan_cpu.py).
#ifndef WFM_WFA_PLAN_H_
#define WFM_WFA_PLAN_H_
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <climits>
#include <vector>

#include "../../include/wfmash_hip.h"

namespace wfm {

constexpr int PLAN_SUB_NONE = 1 << 29;  // SUB_NONE of wfa_device.h (a HIP header): no upper bound of the score is known

// one job of the recursion: a sub-range of a problem between two breakpoints
struct Node {
  int32_t prob;
  int32_t pb, pl, tb, tl;
  int32_t cb, ce;
  int32_t score_rem;  // INT_MAX at the root
  int32_t smax;       // base jobs: score budget (0 = derive)
  int32_t endsfree;
  int32_t noband;     // bialign jobs: 1 = ran out of a narrow ring once, gets the full one now
  int32_t sub;        // bialign jobs: upper bound of the score (SUB_NONE: none); the wavefronts are cut to what can stay under it
  int32_t hinted;     // the bound is the caller's guess (a root): the job is run again without it if the guess was too small
  int32_t tries;      // base jobs: how many score budgets the job has overflowed so far
  int32_t band;       // bialign jobs that are run again: the band (scores a direction) of the attempt that failed, 0: it had a full ring.  Where the
                      // full ring does not fit the budget the next attempt's band grows from it (plan_ring below, called by plan_chunk)
  int32_t snap;       // bialign jobs: 1 + the index of the snapshot the job goes on from on its wider ring (GrownSnap), 0: it starts at score 0
};

// ---- the size of a ring: `w` columns of 2 directions x 5 components x RR rows of int32 ----
inline size_t ring_full_width(int pl, int tl) { return ((size_t)pl + tl + 9 + 3) & ~(size_t)3; }  // columns 4 .. pl+tl+4, 16-byte chunks
inline size_t ring_col_bytes(int RR) { return (size_t)2 * 5 * RR * 4; }                             // 1280 B at 32 rows
inline size_t ring_elems(size_t w, int RR, int rings = 1) { return w * 2 * 5 * RR * rings; }        // (tiled jobs have two: the snapshots)

// A ring for b scores a direction: it holds |k| <= b + 8, its left margin stays 4 columns.  `shift` columns are cut off on the
// left (whole 16-byte chunks; 0: a short pattern, the ring is cut on the right only), column = k + koff.
struct BandGeometry { int64_t shift; size_t width; int koff; };
inline BandGeometry band_geometry(int pl, int tl, int64_t b) {
  const int64_t shift = std::max<int64_t>(0, ((int64_t)pl - (b + 8)) & ~(int64_t)3);
  const int64_t right = std::min<int64_t>(tl, b + 8);  // largest diagonal kept
  return BandGeometry{shift, ((size_t)((int64_t)pl - shift + right + 9) + 3) & ~(size_t)3, (int)(pl + 4 - shift)};
}

// what plan_ring decides by, beside the node: TileCfg's enabled / min_len / min_score / chunk / T, the rows of the call's rings, the
// handle's budget (bytes), WFM_BAND_ROOT, and the state of the level (use_band, over_budget) and of the call (roots_off)
struct RingRules {
  bool tiles = true;
  int min_len = 128, min_score = 64, chunk = 2, T = 100;
  int RR = 32;
  size_t mem_budget = 0;
  int band_root = 4096;
  bool use_band = false, over_budget = false, roots_off = false;
};
struct RingPlan {
  bool fits = true;      // false: the job's score is beyond the budget (WFM_ST_OOM)
  size_t width = 0;      // columns
  int koff = 0, band = 0;  // band 0: the full ring
  bool tile_it = false;  // on the tile kernels (two rings), else the step kernel alone
  bool grown = false;    // a band the budget forced, not one the level chose
  size_t need = 0;       // elements
};

inline RingPlan plan_ring(const Node& nd, const RingRules& r) {
  RingPlan p;
  const size_t full_width = ring_full_width(nd.pl, nd.tl);
  p.width = full_width;
  p.koff = nd.pl + 4;
  p.tile_it = r.tiles && nd.pl + nd.tl >= r.min_len && (nd.score_rem == INT_MAX || nd.score_rem >= r.min_score);
  const bool tiles_take_it = p.tile_it;
  // (a root without a bound gets a guessed band only when the level would not fit otherwise: below the budget the
  // guess has nothing to win and a deep record -- 5 % divergence: 6 k scores per direction -- everything to lose)
  const bool known = nd.score_rem != INT_MAX || nd.sub != PLAN_SUB_NONE;
  if (r.use_band && (known || r.over_budget) && p.tile_it && !nd.noband && !(r.roots_off && nd.score_rem == INT_MAX)) {
    // scores one direction is allowed to reach
    // (a root under a bound of its score leaves the tile phase once a direction passes (bound + 128) / 2)
    int64_t dir_scores = nd.score_rem == INT_MAX ? (int64_t)r.band_root : (int64_t)nd.score_rem / 2 + 64;
    if (nd.score_rem == INT_MAX && nd.sub != PLAN_SUB_NONE) dir_scores = std::min<int64_t>(dir_scores, ((int64_t)nd.sub + 128) / 2 + 64);
    const int64_t b = dir_scores + (int64_t)r.chunk * r.T + 16;
    const BandGeometry g = band_geometry(nd.pl, nd.tl, b);
    if (g.shift > 0 && g.width * 2 <= full_width) { p.band = (int)b; p.width = g.width; p.koff = g.koff; }  // (a band has to halve the ring)
  }
  if (p.tile_it && ring_elems(p.width, r.RR, 2) * 4 > r.mem_budget) p.tile_it = false;  // two snapshot rings do not fit: step-by-step kernel
  p.need = ring_elems(p.width, r.RR, p.tile_it ? 2 : 1);
  // The ring does not fit the budget (the job's first attempt, without a band it could have had; or its full ring, after a band ran out
  // or a guess of its score failed): a ring for max(4 x the band it had, WFM_BAND_ROOT) scores a direction -- the cells of a job grow with the
  // square of the score it reaches, so all the attempts before the one that holds cost a fifteenth of it -- on the tile kernels where they
  // take the job and two such rings fit, on the step kernel alone otherwise; no wider than the budget holds.  (A child's first band is what its
  // known score asks for, as above.)  Once the band's ring would be as wide as the full one -- below the budget a band has to halve the ring
  // to be worth a second attempt, here the full ring is no alternative -- or the job has spent the widest band the budget holds, its score
  // is beyond the budget: WFM_ST_OOM.
  if (p.need * 4 > r.mem_budget) {
    const size_t col_bytes = ring_col_bytes(r.RR);
    const int64_t first = nd.score_rem == INT_MAX ? (int64_t)r.band_root : (int64_t)nd.score_rem / 2 + 64 + (int64_t)r.chunk * r.T + 16;
    int64_t nb = nd.band > 0 ? std::max<int64_t>(4 * (int64_t)nd.band, first) : first;
    BandGeometry g = band_geometry(nd.pl, nd.tl, nb);
    p.fits = g.width < full_width;
    if (p.fits && g.width * col_bytes > r.mem_budget) {
      nb = ((int64_t)(r.mem_budget / col_bytes) - 32) / 2;  // (a ring for b scores is at most 2 b + 32 columns wide)
      p.fits = nb > (int64_t)nd.band && nb >= 64;
      if (p.fits) { g = band_geometry(nd.pl, nd.tl, nb); p.fits = g.width < full_width && g.width * col_bytes <= r.mem_budget; }
    }
    if (!p.fits) return p;
    p.grown = true;
    p.band = (int)nb; p.width = g.width; p.koff = g.koff;
    p.tile_it = tiles_take_it && ring_elems(p.width, r.RR, 2) * 4 <= r.mem_budget;
    p.need = ring_elems(p.width, r.RR, p.tile_it ? 2 : 1);
  }
  return p;
}

// ---- a problem's runs ((len << 2) | op, ops M 0, X 1, I 2, D 3) into its op string ----
// Adjacent runs of one op are merged.  runs_out == nullptr: one byte per op into ops[0 .. ops_cap); else the merged runs are
// appended to *runs_out (taken back where the spans do not match) and ops_len counts the ops the runs spell.
enum { EXPAND_OK = 0, EXPAND_SPANS = 1, EXPAND_ARENA = 2, EXPAND_RUN_TOO_LONG = 3 };
struct Expanded {
  int32_t score = -1;
  uint32_t n_runs = 0, ops_len = 0;
  uint64_t pc = 0, tc = 0;  // pattern / text bases the runs span
};
inline int expand_runs(const uint32_t* e, int cnt, const wfm_penalties_t& pen, int plen, int tlen, char* ops, size_t ops_cap,
                       std::vector<uint32_t>* runs_out, Expanded* out) {
  static const char opc[4] = {'M', 'X', 'I', 'D'};
  const size_t runs_before = runs_out ? runs_out->size() : 0;
  int64_t score = 0;
  uint64_t pc = 0, tc = 0, both = 0;
  uint32_t nruns = 0;
  size_t pos = 0;
  int k = 0;
  while (k < cnt) {
    const int op = (int)(e[k] & 3u);
    uint64_t len = e[k] >> 2;
    int k2 = k + 1;
    while (k2 < cnt && (int)(e[k2] & 3u) == op) { len += e[k2] >> 2; ++k2; }
    if (runs_out) {
      if (len >= (1u << 30)) return EXPAND_RUN_TOO_LONG;
      runs_out->push_back((uint32_t)(len << 2) | (uint32_t)op);
    } else {
      if (pos + len > ops_cap) return EXPAND_ARENA;
      memset(ops + pos, opc[op], (size_t)len);
      pos += (size_t)len;
    }
    ++nruns;
    if (op == 1) { score += (int64_t)len * pen.x; pc += len; tc += len; both += len; }
    else if (op == 0) { pc += len; tc += len; both += len; }
    else {
      score += std::min<int64_t>(pen.o1 + (int64_t)len * pen.e1, pen.o2 + (int64_t)len * pen.e2);
      if (op == 2) tc += len; else pc += len;
    }
    k = k2;
  }
  out->pc = pc; out->tc = tc;
  if (pc != (uint64_t)plen || tc != (uint64_t)tlen) {
    if (runs_out) runs_out->resize(runs_before);
    return EXPAND_SPANS;
  }
  // ops spelled: every M / X op advances both sequences, I the text, D the pattern
  out->ops_len = runs_out ? (uint32_t)(pc + tc - both) : (uint32_t)pos;
  out->n_runs = nruns;
  out->score = (int32_t)score;
  return EXPAND_OK;
}

}  // namespace wfm
#endif
