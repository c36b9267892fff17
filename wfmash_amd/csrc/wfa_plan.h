// wfa_plan.h -- the arithmetic of the BiWFA level driver (wfa_host.hip) that needs no device: how large a wavefront ring is, the
// geometry of a banded ring, which ring a job gets under the memory budget (plan_ring), how a problem's runs become its op
// string (expand_runs); what a chunk of the tile phase and of phase 2 launches (plan_tile_chunk, plan_p2_chunk) and which kernel a
// base job goes to (base_kind, base_columns, plan_base_tiles).  Host only, no HIP, no getenv, no handle; the CPU suite reaches it
// through the wfmh_test_* hooks of host/capi_host.cpp (tests/test_ring_plan_cpu.py, tests/test_tile_plan_cpu.py).
#ifndef WFM_WFA_PLAN_H_
#define WFM_WFA_PLAN_H_
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <climits>
#include <vector>

#include "../../include/wfmash_hip.h"
#include "wfa_rows.h"

namespace wfm {

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
  int32_t keep;       // bialign jobs: 1 + the index of the kept rows of its parent that its outer direction resumes from (KeptRows), 0: both directions start at score 0
  int32_t keep_dir;   // the direction those rows are of: 0 forward (a first child), 1 reverse (a second child)
  int32_t limit;      // roots of a problem with a hard score limit (WFM_MODE_SCORE_LIMIT): the limit; 0: none.  sub <= limit then, and no attempt runs without it
  int32_t meet;       // bialign children: sf + sr of the planned end of phase 1 (planned_meet below), 0: none -- the job searches for its meeting point
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
  const bool known = nd.score_rem != INT_MAX || nd.sub != SUB_NONE;
  if (r.use_band && (known || r.over_budget) && p.tile_it && !nd.noband && !(r.roots_off && nd.score_rem == INT_MAX)) {
    // scores one direction is allowed to reach
    // (a root under a bound of its score leaves the tile phase once a direction passes (bound + 128) / 2)
    int64_t dir_scores = nd.score_rem == INT_MAX ? (int64_t)r.band_root : (int64_t)nd.score_rem / 2 + 64;
    if (nd.score_rem == INT_MAX && nd.sub != SUB_NONE) dir_scores = std::min<int64_t>(dir_scores, ((int64_t)nd.sub + 128) / 2 + 64);
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

// ---- cells of a job's rows ----
// sum over the scores a .. b of the cells of a row (rng_lo .. rng_hi): the row's edges are piecewise linear in the score (each a
// min / max of three lines), so between two consecutive kinks the count is an arithmetic series
inline int64_t cells_sum(int pl, int tl, int sub, int a, int b) {
  if (b < a) return 0;
  const Rng rg = make_rng(pl, tl, sub);
  const int64_t kinv = (int64_t)tl - pl, khi = kinv + sub, klo = kinv - sub;
  // scores at which two of the lines of an edge cross (the kink lies between the floor and the next integer)
  int64_t cand[16];
  int nc = 0;
  auto add = [&](int64_t x) { for (int64_t y : {x, x + 1}) if (y > a && y <= b) cand[nc++] = y; };
  add(tl); add(khi / 2 - (khi < 0 && (khi & 1) ? 1 : 0)); add(khi - tl);     // hi: s vs tl, s vs khi - s, tl vs khi - s
  add(pl); add((-klo) / 2 - (-klo < 0 && ((-klo) & 1) ? 1 : 0)); add(-klo - pl);  // lo: -s vs -pl, -s vs klo + s, -pl vs klo + s
  std::sort(cand, cand + nc);
  int64_t total = 0;
  int64_t u = a;
  auto cells = [&](int64_t s) { return (int64_t)rng_hi(rg, (int)s) - rng_lo(rg, (int)s) + 1; };
  auto seg = [&](int64_t x, int64_t y) {  // linear on [x, y]
    if (y < x) return;
    const int64_t cx = cells(x), cy = cells(y);
    if (cx <= 0 && cy <= 0) return;
    if (cx > 0 && cy > 0) { total += (cx + cy) * (y - x + 1) / 2; return; }
    if (y == x) { total += std::max<int64_t>(cx, 0); return; }
    // one end at or below zero: the slope is (cy - cx) / (y - x), an integer (each edge moves by whole diagonals per score)
    const int64_t slope = (cy - cx) / (y - x);
    if (cx > 0) {  // falls: positive up to x + (cx - 1) / -slope
      const int64_t last = x + (cx - 1) / (-slope);
      total += (cx + cells(last)) * (last - x + 1) / 2;
    } else {       // rises: positive from y - (cy - 1) / slope
      const int64_t first = y - (cy - 1) / slope;
      total += (cells(first) + cy) * (y - first + 1) / 2;
    }
  };
  for (int q = 0; q < nc; ++q) {
    if (cand[q] <= u) continue;
    seg(u, cand[q] - 1);
    u = cand[q];
  }
  seg(u, b);
  return total;
}

// ---- a chunk of the tile phase (run_tiled_phase): `chunk` blocks of T scores launched back to back ----
// what the planner needs of a job (TileJob's fields of the same names); jobs that are not active get no tile
struct TilePlanJob { int pl, tl, sub, s0, mode, fine_s, packed, active; };
struct TilePlanRules {
  int threads = 512, C = 2, T = 100, chunk = 2;
  int core = 0;            // diagonals of a tile with a halo: Wt - 2 T
  bool reg = true;         // register tiles (TileCfg::reg)
  bool fine = true;        // WFM_TILE_FINE: every block of a single-tile chunk gets the workgroup size its own widest range needs
  bool coarse_on = false;  // the packed kernel keeps one maximum per block below a job's fine_s
  bool planned = false;    // jobs with a planned end (TileJob::plan_sum) that carry fine_s = INT_MAX are among the phase's: a block of nothing but runs
                           // up to a meeting point goes to the instantiation without per-score maxima, so that such jobs alone never launch the other
};
struct TileChunkPlan {
  std::vector<int> threads_b, variants_b;  // per block of the chunk: workgroup size; instantiations of the packed kernel (1 without per-score maxima, 2 with)
  int core_c = 0;                          // diagonals a tile owns
  std::vector<TileTask> tasks, tasks_by;   // tasks: the packed jobs' tiles, then (once the plan is complete) the byte kernel's, which tasks_by collects
  size_t n_pk = 0;                         // tiles of packed jobs: tasks[0 .. n_pk)
};

// A job leaves the tile phase before a chunk (mode 3; it is run again): on a narrow ring (band > 0) when the chunk's last score
// no longer fits it -- and under a score bound that is a guess: the two directions meet near half the score, so a job still going
// well past half the bound has a score above it; or nothing is left within the bound.
inline bool tile_job_leaves(int pl, int tl, int sub, int s0, int band, int chunk, int T) {
  if (band > 0 && s0 + chunk * T + 2 > band) return true;
  if (sub == SUB_NONE) return false;
  int L, R;
  rng_block(make_rng(pl, tl, sub), s0, s0 + T, L, R);
  return 2 * s0 > sub + 128 || R < L;
}
// Under a hard limit of the score (Node::limit, sub <= limit) the same tests are verdicts: a job whose directions stand apart at s0 has a score
// above s0 (an alignment of at most s0 would have brought either direction to the far end alone) and above 2 s0 - the dearest gap opening (its
// two halves, the opening counted twice, would have met) -- at most 124, validate_pen -- and nothing of an alignment within the bound lies outside
// the rows the bound cuts.  So no block is planned whose first score passes the limit, and a job that leaves for one of these reasons is beyond
// its limit whatever ring it ran on (the band's own test above is no such verdict: the band of a root is a guess).
inline bool tile_job_beyond_limit(int pl, int tl, int sub, int limit, int s0, int T) {
  if (limit <= 0) return false;
  if (s0 >= limit) return true;
  int L, R;
  rng_block(make_rng(pl, tl, sub), s0, s0 + T, L, R);
  return 2 * s0 > sub + 128 || R < L;
}

// While the widest range of a chunk fits one tile, every job-direction is ONE tile without a halo, and the workgroups are only
// as large as that range needs: whole waves, C diagonals per lane
inline bool fits_one_tile(int widest, int threads, int C) { return widest <= threads * C; }
inline int one_tile_threads(int widest, int threads, int C) { return std::min(threads, std::max(64, ((widest + C - 1) / C + 63) / 64 * 64)); }

// the tiles of one direction of a job: packed jobs' (wfa_tile2_kernel) apart from the others' (an N, soft-masked bases: the byte
// kernel), which go behind them.  A task is (tile index, tile width): the kernel places it (tile_span)
// dirs: the directions of the job that run at all (bit 0 forward, bit 1 reverse; a job that waits for its parent's rows runs its inner one alone)
inline void append_tile_tasks(TileChunkPlan& p, int job, int dir, int ntiles, int core, bool packed, int dirs = 3) {
  if (!((dirs >> dir) & 1)) return;
  std::vector<TileTask>& to = packed ? p.tasks : p.tasks_by;
  for (int t = 0; t < ntiles; ++t) to.push_back(TileTask{(int32_t)job, dir, t, core});
}
inline void close_task_list(TileChunkPlan& p) {
  p.n_pk = p.tasks.size();
  p.tasks.insert(p.tasks.end(), p.tasks_by.begin(), p.tasks_by.end());
}

// dirs: per job the directions that get tiles (append_tile_tasks), nullptr: both of every job
inline void plan_tile_chunk(const TilePlanJob* jobs, size_t n, const TilePlanRules& r, TileChunkPlan& p, const uint8_t* dirs = nullptr) {
  const int chunk = r.chunk, T = r.T;
  auto block_range = [&](const TilePlanJob& j, int b, int& L, int& R) { rng_block(make_rng(j.pl, j.tl, j.sub), j.s0 + b * T, j.s0 + (b + 1) * T, L, R); };
  // as many tiles of `core` diagonals per job and direction as the last block of this chunk can need
  p.tasks.clear(); p.tasks_by.clear();
  p.core_c = r.core;
  p.threads_b.assign((size_t)chunk, r.threads);
  if (r.reg && r.C == 2) {
    std::vector<int> wb((size_t)chunk, 0);  // widest range per block
    for (size_t i = 0; i < n; ++i) {
      if (!jobs[i].active) continue;
      // a job may run the same block twice (the block in which its wavefronts met, up to the meeting point), and with a
      // score bound the ranges shrink again towards the end: block b of the chunk needs the widest range up to b
      int wmax = 0;
      for (int b = 0; b < chunk; ++b) {
        int L, R;
        block_range(jobs[i], b, L, R);
        wmax = std::max(wmax, R - L + 1);
        wb[(size_t)b] = std::max(wb[(size_t)b], wmax);
      }
    }
    if (fits_one_tile(wb[(size_t)chunk - 1], r.threads, r.C)) {
      for (int b = 0; b < chunk; ++b) {
        const int wdt = r.fine ? wb[(size_t)b] : wb[(size_t)chunk - 1];
        p.threads_b[(size_t)b] = r.fine ? one_tile_threads(wdt, r.threads, r.C) : std::min(r.threads, wdt <= 256 ? 128 : (wdt <= 512 ? 256 : r.threads));
      }
      p.core_c = p.threads_b[(size_t)chunk - 1] * r.C;
    }
  }
  for (size_t i = 0; i < n; ++i) {
    if (!jobs[i].active) continue;
    int ntiles = 0;  // of the widest block of the chunk
    for (int b = 0; b < chunk; ++b) {
      int L, R;
      block_range(jobs[i], b, L, R);
      ntiles = std::max(ntiles, tiles_for(L, R, p.core_c));
    }
    for (int d = 0; d < 2; ++d) append_tile_tasks(p, (int)i, d, ntiles, p.core_c, jobs[i].packed != 0, dirs ? dirs[i] : 3);
  }
  close_task_list(p);
  // which instantiations of the packed kernel a block of the chunk can have tiles for (wfa_tile2_kernel, FINE): the one without per-score
  // maxima always (the blocks before a job's meeting block and the run up to the meeting point); the one with them where a job that simply
  // moved on has reached its fine_s, and in the chunk's first block for the jobs the last chunk left in mode 5
  p.variants_b.assign((size_t)chunk, r.coarse_on ? 0 : 2);
  if (!r.coarse_on) return;
  for (size_t i = 0; i < n; ++i) {
    const TilePlanJob& j = jobs[i];
    if (!j.active || !(j.packed & 1)) continue;
    for (int b = 0; b < chunk; ++b) {
      const bool reaches = (int64_t)j.s0 + (int64_t)(b + 1) * T >= (int64_t)j.fine_s;
      if ((j.mode == 5 && b == 0) || (j.mode == 0 && reaches)) p.variants_b[(size_t)b] |= 2;
      // without maxima: a job that simply moved on and is still below its fine_s (it may also have met meanwhile: its run up to the meeting
      // point needs no maxima either -- and is taken by the FINE instantiation where that one is launched alone)
      if (j.mode == 0 && !reaches) p.variants_b[(size_t)b] |= 1;
    }
  }
  // (a job with a planned end in a chunk that launches both carries fine_s = INT_MAX: it never reaches it, and counts for the instantiation without maxima in every block)
  for (int b = 0; b < chunk; ++b) if (!p.variants_b[(size_t)b]) p.variants_b[(size_t)b] = r.planned ? 1 : 2;  // (only runs up to a meeting point: either would do)
}

// ---- a child's outer direction from its parent's kept rows ("parent reuse") ----
// A job's forward direction and its first child's start in the same cell, in the same component, over the same bases (and so do its reverse
// direction and its second child's): while no cell of the parent's rows has reached the child's box, the child's own rows ARE the parent's, cut to
// the child's ranges.  The parent keeps a compact copy of its input snapshot every `cadence` blocks (KEEP_ROWS rows a direction, each over its own
// range); the child runs its inner direction alone up to the score of the keep it picked, takes the kept rows for the other one, and goes on as
// any tiled job.
// blocks between two keeps: WFM_REUSE_EVERY rounded up to whole chunks -- a keep is taken where the host looks, and a child can only take one over there
inline int reuse_cadence(int every, int chunk) { return (std::max(1, every) + chunk - 1) / chunk * chunk; }
// the last score a child of score `score_rem` may resume at: its meeting block must not be the first one after the restore (that block's input
// holds the gap rows two deep and one deep, not the 26 a short run up to the meeting point hands on)
inline int reuse_resume_limit(int score_rem, int T, int fine_margin) {
  const int64_t x = (int64_t)score_rem / 2 - fine_margin;
  return x < 0 ? -1 : (int)(x / T * T - T);
}
// the newest of the kept scores the child may take (an index into kept_s), -1: none.  min_blocks (WFM_REUSE_MIN_BLOCKS, at least 1): a keep fewer
// blocks deep is not worth the restore -- a look of the host with a launch and a wait of its own, where the blocks it saves are a few tiles each
inline int reuse_pick_keep(const int32_t* kept_s, size_t n, int score_rem, int T, int fine_margin, int min_blocks = 1) {
  if (score_rem == INT_MAX) return -1;
  const int limit = reuse_resume_limit(score_rem, T, fine_margin);
  const int64_t least = (int64_t)std::max(1, min_blocks) * T;
  int best = -1;
  for (size_t i = 0; i < n; ++i)
    if (kept_s[i] >= least && kept_s[i] <= limit && (best < 0 || kept_s[i] > kept_s[(size_t)best])) best = (int)i;
  return best;
}
// every row of the keep at score s_k holds the child's whole range of that score
inline bool reuse_ranges_contained(int ppl, int ptl, int psub, int cpl, int ctl, int csub, int s_k) {
  const Rng P = make_rng(ppl, ptl, psub), Cc = make_rng(cpl, ctl, csub);
  for (int s = std::max(0, s_k - RNG_BACK); s <= s_k; ++s) {
    const int lo = rng_lo(Cc, s), hi = rng_hi(Cc, s);
    if (hi < lo) continue;
    if (lo < rng_lo(P, s) || hi > rng_hi(P, s)) return false;
  }
  return true;
}
// Whether a node may resume from the keep it carries: it knows its score (and the bound its parent handed it with it: a call whose children run
// without their parents' scores -- WFM_SUB_SLACK of 2^28 and more, the tests' unbounded configuration -- computes every row itself), runs on the tile kernels on a full ring that no budget shaped,
// and its parent's rows hold its own.  (ppl, ptl, psub: the parent's box and bound, as its rows were cut)
inline bool reuse_eligible(const Node& nd, const RingPlan& rp, int ppl, int ptl, int psub, int child_sub, int s_k, int T) {
  if (nd.keep <= 0 || nd.score_rem == INT_MAX || nd.sub == SUB_NONE || !rp.fits || !rp.tile_it || rp.band != 0 || rp.grown) return false;
  if (s_k < T || s_k % T != 0) return false;
  return reuse_ranges_contained(ppl, ptl, psub, nd.pl, nd.tl, child_sub, s_k);
}
// Whether a keep at score `es` can be the one a child resumes from.  The two directions of a job meet at the same score (a step apart), so
// its children have half its score each and resume near HALF the score s_meet its directions meet at: at most s_meet / 2 - fine_margin - T, at
// least a cadence and two blocks below that.  A child knows s_meet (half its score); a root's is read off its progress so far (reuse_meet_estimate),
// give or take a fifth.  Keeps outside [0.4 s_meet - 64 - (2 + cadence) T, 0.6 s_meet] are not written: the copy of a keep grows with its score,
// and all keeps up to the meeting point would be four times the bytes (a child whose keep is missing all the same starts at score 0, as ever).
inline bool reuse_keep_wanted(int es, int64_t s_meet, int cadence, int T) {
  if (s_meet <= 0) return false;
  return 100 * (int64_t)es >= 40 * s_meet - 100 * (64 + (int64_t)(2 + cadence) * T) && 100 * (int64_t)es <= 60 * s_meet;
}
// the score a job's directions will meet at, from where it stands: at s0 with the sum `mak` of its two directions' largest antidiagonals, which
// meet when that sum reaches A (a record with an end gap moves slowly at first: the estimate is high then); 0: nothing to go by yet
inline int64_t reuse_meet_estimate(int s0, int64_t mak, int64_t A) { return s0 <= 0 || mak <= 0 ? 0 : (int64_t)s0 * A / mak; }
// elements of one direction of a keep at score s: KEEP_ROWS rows over the widest of them
inline int reuse_keep_kmin(int pl, int s) { return std::max(-pl, -s); }
inline int reuse_keep_cols(int pl, int tl, int s) { return std::min(tl, s) - std::max(-pl, -s) + 1; }
inline size_t reuse_keep_elems(int pl, int tl, int s) { return (size_t)KEEP_ROWS * (size_t)reuse_keep_cols(pl, tl, s); }
// The cadence under the store's cap: what the keeping jobs would keep up to `upto` (the last score a child of theirs could resume at, where a
// bound of the score is known; a guess otherwise) has to fit cap_bytes -- the cadence doubles until it does; 0: not even one keep a job, no reuse
struct ReuseKeeper { int pl, tl, upto; };
inline int reuse_fit_cadence(const ReuseKeeper* jobs, size_t n, int cadence, int T, size_t cap_bytes) {
  int upto_max = 0;
  for (size_t i = 0; i < n; ++i) upto_max = std::max(upto_max, jobs[i].upto);
  for (; (int64_t)cadence * T <= upto_max; cadence *= 2) {
    size_t bytes = 0;
    for (size_t i = 0; i < n && bytes <= cap_bytes; ++i)
      for (int64_t s = (int64_t)cadence * T; s <= jobs[i].upto && bytes <= cap_bytes; s += (int64_t)cadence * T) bytes += 2 * 4 * reuse_keep_elems(jobs[i].pl, jobs[i].tl, (int)s);
    if (bytes <= cap_bytes) return cadence;
  }
  return 0;
}

// ---- the planned end of phase 1 of a job whose score is known ("the planned end") ----
// The reference's first loop (wavefront_bialign_find_breakpoint, oracle/wfa2p.c) walks a fixed track of states (sf, sr): (1, 0), (1, 1), (2, 1),
// (2, 2) ... -- the state with sf + sr = P is (ceil(P / 2), floor(P / 2)), the forward direction stepped last iff P is odd -- and leaves it at the
// trigger Y, where the two largest antidiagonals sum to pl + tl - 1.  The second loop goes on along the SAME track (test the direction stepped
// last against the other's newest `scope` rows, step the other), so "phase 2 from the state X" differs from "phase 2 from Y" only in the tests
// at the states between the two, and both give the same breakpoint, field for field, if all of those fail:
//  * X behind Y.  A test at (sf, sr) pairs row sf (or sr) with rows si <= sr (sf) of the other direction; a pair that hits in component c --
//    o0 + o1 >= tl on a diagonal -- is an alignment of score sf + si - gopen(c) of the job in the job's own terms (below).  None is cheaper than
//    the optimum S_own, so no test at a state with sf + sr < S_own hits; nor does the loop end there (it ends when sf + sr - (scope - 1) -
//    max(o1, o2) reaches the best score in hand, which starts above the job's bound).
//  * X before Y.  M[s][k] >= every gap component's [s][k] (a row's M is the maximum of its sources), so a hit in any component puts two M cells
//    with o0 + o1 >= tl on a diagonal, whose antidiagonals 2 o - k sum to at least pl + tl: the trigger has fired by then.  No test before Y hits.
// So every X with sf + sr <= S_own will do, and the largest leaves the fewest tests: the walk of phase 2 runs on to sf + sr = best + scope - 1 +
// max(o1, o2) (49 past S_own at the default penalties), inside the 2 * P2K = 64 tests of one round only if X is less than 15 short of S_own.
// S_own in terms of Node::score_rem, the score the PARENT's search credited the child with: a direction that starts in a gap component extends
// that gap without opening it (the row of score 0 is the component's), and a gap the breakpoint cut was opened on BOTH sides of the cut (hence
// the reference's "- gopen" in a gap breakpoint's score).  A first child (comp_end is the cut) was credited score_forward, its parent's forward
// direction's cost INCLUDING that opening; its own search starts the reverse direction inside the gap and never pays it: S_own = score_rem -
// gopen(comp_end).  A second child (comp_begin is the cut): S_own = score_rem - gopen(comp_begin).  The other end's component came down from an
// ancestor whose direction started in it at score 0: nothing to subtract.  (A child that is one gap from end to end has no pattern or no text
// and is a base job.)  D = that opening, 0 for a cut in M: exact, so the walk stays within one round.
// second: the job is the second child of its parent (its comp_begin is the cut, not its comp_end).  -> sf + sr of X; 0: no plan (no known score)
inline int planned_meet_sum(int score_rem, const wfm_penalties_t& pen, int comp_begin, int comp_end, bool second) {
  if (score_rem == INT_MAX || score_rem <= 0) return 0;
  const int cut = second ? comp_begin : comp_end;
  const int D = cut == 0 ? 0 : ((cut == 1 || cut == 3) ? pen.o1 : pen.o2);  // (wfa_device.h: C_M 0, C_I1 1, C_I2 2, C_D1 3, C_D2 4)
  return std::max(0, score_rem - D);
}
struct PlannedMeet { int sf, sr, last_fwd; };
inline PlannedMeet planned_meet_state(int sum) { return PlannedMeet{(sum + 1) / 2, sum / 2, sum & 1}; }
inline PlannedMeet planned_meet(int score_rem, const wfm_penalties_t& pen, int comp_begin, int comp_end, bool second) {
  return planned_meet_state(planned_meet_sum(score_rem, pen, comp_begin, comp_end, second));
}
// the block of T scores the planned end lies in begins at this score: the state (s0 + tf, s0 + tr) with tf in 1 .. T, tr in 0 .. T
inline int planned_meet_block(int sum, int T) { return ((sum + 1) / 2 - 1) / T * T; }
// Whether a node takes its planned end (the same shape of test as reuse_eligible): it knows its score and carries the bound that came with it
// (not so the children of a call in the unbounded WFM_SUB_SLACK configuration), and runs on the packed tile kernel on a ring no budget shaped --
// the full one, or the narrow one the level chose for its known score (band = score_rem / 2 + 64 + chunk * T + 16: every row up to the planned
// end, at most score_rem / 2, and the P2K rows behind it lie inside; a ring that GREW under the budget is a guess and stays on the search).
// s_keep: the score of the keep the job resumes from (0: none) -- the block of the planned end must not be the first one after the restore
// (reuse_resume_limit's rule: that block's input holds no gap rows 26 deep)
inline bool planned_meet_eligible(const Node& nd, const RingPlan& rp, bool packed, int s_keep, int T) {
  if (nd.meet <= 0 || nd.score_rem == INT_MAX || nd.sub == SUB_NONE || !rp.fits || !rp.tile_it || rp.grown || !packed) return false;
  if (planned_meet_state(nd.meet).sf < 1) return false;
  return s_keep <= 0 || planned_meet_block(nd.meet, T) >= s_keep + T;
}

// ---- a chunk of phase 2 from rows computed ahead (run_p2_phase): P2K more rows of both directions of every job ----
struct P2PlanJob { int pl, tl, sub, sf, sr, packed; };  // sf / sr: the scores the directions stand at (BpJob::resume_s / resume_sr)
struct P2Geometry {
  int koff2; size_t w2, nblk;   // the job's P2 rows: column = k + koff2, w2 columns, nblk blocks of 64 diagonals
  size_t p2_off, bm_off;        // element offsets of its rows and of its block maxima
};
struct P2ChunkPlan {
  std::vector<P2Geometry> geo;  // of the jobs the chunk takes: candidates i0 .. i0 + geo.size()
  size_t elems = 0, bm_elems = 0, maxw2 = 0;
  int threads_c = 0;
  TileChunkPlan tiles;          // (core_c, tasks, n_pk; jobs are numbered within the chunk)
};
// rows: P2K, rows_bm: P2ROWS (wfa_device.h); budget: bytes the rows of a chunk may take; core: Wt - 2 P2K
// exact: per candidate, nonzero where the job takes the exact walk (P2Job::exact) -- it reads no maxima, so none are laid out for it (bm_off 0);
// nullptr: every job searches
inline void plan_p2_chunk(const P2PlanJob* cand, size_t n_cand, size_t i0, int rows, int rows_bm, size_t budget, int threads, int core, P2ChunkPlan& p,
                          const char* exact = nullptr) {
  p.geo.clear(); p.elems = 0; p.bm_elems = 0; p.maxw2 = 0;
  p.tiles.tasks.clear(); p.tiles.tasks_by.clear();
  for (size_t i = i0; i < n_cand; ++i) {
    const P2PlanJob& j = cand[i];
    const int reach = std::max(j.sf, j.sr) + rows;
    int L, R;  // every diagonal a row of the window can hold: the snapshot's rows (26 back) and the rows computed ahead
    rng_block(make_rng(j.pl, j.tl, j.sub), std::max(0, std::min(j.sf, j.sr) - P2_BACK), reach, L, R);
    if (R < L) { L = 0; R = 0; }
    P2Geometry g;
    g.koff2 = ((-L + 4) + 3) & ~3;  // column of diagonal 0: a multiple of 4, >= 4 columns of margin
    g.w2 = ((size_t)(R + g.koff2 + 8) + 3) & ~(size_t)3;
    g.nblk = (g.w2 >> 6) + 1;
    const size_t need = g.w2 * 2 * 5 * rows, need_bm = (exact && exact[i]) ? 0 : g.nblk * 2 * rows_bm * 5;
    if (!p.geo.empty() && (p.elems + need + 2 * (p.bm_elems + need_bm)) * 4 > budget) break;
    p.maxw2 = std::max(p.maxw2, g.w2);
    g.p2_off = p.elems; g.bm_off = p.bm_elems;
    p.bm_elems += need_bm;
    p.elems += need;
    p.geo.push_back(g);
  }
  const size_t n = p.geo.size();
  auto dir_range = [&](const P2PlanJob& j, int d, int& L, int& R) { rng_block(make_rng(j.pl, j.tl, j.sub), d == 0 ? j.sf : j.sr, (d == 0 ? j.sf : j.sr) + rows, L, R); };
  // one tile without a halo per job-direction while the widest range of the chunk fits one
  p.threads_c = threads; p.tiles.core_c = core;
  int widest = 0;
  for (size_t q = 0; q < n; ++q)
    for (int d = 0; d < 2; ++d) {
      int L, R;
      dir_range(cand[i0 + q], d, L, R);
      widest = std::max(widest, R - L + 1);
    }
  if (fits_one_tile(widest, threads, 2)) {
    p.threads_c = one_tile_threads(widest, threads, 2);
    p.tiles.core_c = p.threads_c * 2;
  }
  for (size_t q = 0; q < n; ++q)
    for (int d = 0; d < 2; ++d) {
      int L, R;
      dir_range(cand[i0 + q], d, L, R);
      append_tile_tasks(p.tiles, (int)q, d, tiles_for(L, R, p.tiles.core_c), p.tiles.core_c, cand[i0 + q].packed != 0);
    }
  close_task_list(p.tiles);
}

// The workgroup of wfa_p2_exact_kernel for a chunk whose widest rows hold maxw2 columns: a thread takes four diagonals of a scan at a time, so
// this many threads pass the widest row in one stride; narrower chunks (the deep levels: thousands of jobs of a few hundred columns) get
// small workgroups, several of which share a compute unit
inline int p2_exact_threads(size_t maxw2) {
  const size_t t = ((maxw2 + 3) / 4 + 63) / 64 * 64;
  return (int)std::min<size_t>(1024, std::max<size_t>(128, t));
}

// ---- base jobs (run_base_jobs) ----
// The diagonals a base job's rows have to hold under its score budget: within `smax` of where an alignment may begin (diagonal 0 of an
// end-to-end job, [-pbf, tbf] of an ends-free one) -- and, when the alignment has to END in the far corner (no free ends there: leaves, and the
// head patches, whose free ends are at the beginning), within `smax` of the corner's diagonal tl - pl as well: every change of diagonal costs at least
// e2 = 1, so a cell further away lies on no alignment of score <= smax, no cell on such an alignment takes its value from one (the argument of the
// score bounds, section 5 of DESIGN.md), and a job that needs more than its budget is run again anyway.  A head patch begins with ALL its diagonals
// (its begin-free lengths are the eroded lengths: rows of 2 - 8 k diagonals for a budget of 256); with the corner's band its rows are 513 wide.
// pbf / pef / tbf / tef: the problem's free ends (ends-free jobs); corner_band: WFM_BASE_CORNER_BAND
inline void base_columns(const Node& nd, int pbf, int pef, int tbf, int tef, bool corner_band, int64_t* kmin_out, int64_t* kmax_out) {
  int64_t kmin = nd.endsfree ? std::max<int64_t>(-nd.pl, -(int64_t)pbf - nd.smax) : std::max<int64_t>(-nd.pl, -nd.smax);
  int64_t kmax = nd.endsfree ? std::min<int64_t>(nd.tl, (int64_t)tbf + nd.smax) : std::min<int64_t>(nd.tl, nd.smax);
  const bool end_fixed = !nd.endsfree || (pef == 0 && tef == 0);
  if (corner_band && end_fixed) {
    const int64_t k_end = (int64_t)nd.tl - nd.pl;
    const int64_t bmin = std::max(kmin, k_end - nd.smax), bmax = std::min(kmax, k_end + nd.smax);
    // the first row must keep a cell inside (a budget that cannot reach the corner at all leaves the columns as they were: the job overflows as before)
    const int64_t lo0 = nd.endsfree ? std::max<int64_t>(-(int64_t)pbf, bmin) : 0, hi0 = nd.endsfree ? std::min<int64_t>((int64_t)tbf, bmax) : 0;
    if (bmin <= bmax && lo0 <= hi0 && lo0 >= bmin && hi0 <= bmax) { kmin = bmin; kmax = bmax; }
  }
  *kmin_out = kmin; *kmax_out = kmax;
}

// Kinds of base jobs, each in launches of its own: 0 / 1 / 2 = the register kernel on packed sequences (wfa_base2_kernel: default
// penalties, pure ACGT, rows up to 128 / 512 / 2048 diagonals, sequences that fit its windows), 3 / 4 = the ring kernel with
// 256 / 1024 threads (other penalties, an N, wider rows: a patch eroded to its 4096-base limit starts 8 k diagonals wide),
// 5 = the register kernel's step on tiles (wfa_base2t_kernel): rows beyond 2048 diagonals of jobs the register kernel would take -- the third
// attempt of a patch, whose score passed 1020.
// (Sequences longer than the register kernel's LDS windows are fine: what lies beyond is read from the global mirror.  Jobs without
// any cell -- an empty pattern or text -- ride along with kind 1: they are one store each)
struct BaseRules {
  bool base_v2 = true;       // default penalties, and neither WFM_BASE_V2=0 nor WFM_TILE_V2=0
  bool base_tiles = true;    // WFM_BASE_TILES != 0
  bool force_tiles = false;  // WFM_BASE_TILES=2 (tests): every leaf and patch with rows beyond 128 diagonals
  bool few_jobs = false;     // fewer than 128 jobs in the call
  int wide_from = 2048;      // rows beyond this get 1024 threads of the ring kernel (512 when the launch is too small to fill the device anyway)
};
// width: the job's widest row (0 for the all-gap jobs); acgt: the problem's sequences are pure upper-case ACGT
inline int base_kind(int64_t width, int pl, int tl, int tries, bool acgt, const BaseRules& r) {
  if (r.base_v2 && (pl == 0 || tl == 0)) return 1;
  if (r.base_v2 && width <= 2048 && acgt)
    // (a handful of retries: more workgroups of fewer waves per job on the tiles of the register kernel, and ONE launch with the wider ones
    // instead of one per width class, each a few jobs and hundreds of score steps long)
    return width <= 128 ? 0 : (r.base_tiles && (r.force_tiles || (r.few_jobs && (tries > 0 || width > 640))) ? 5 : (width <= 640 ? 1 : 2));
  if (r.base_v2 && r.base_tiles && acgt) return 5;
  return width > r.wide_from ? 4 : 3;
}

// base jobs on tiles: blocks of T scores; a tile is a workgroup of `threads` with two diagonals per lane that owns `core` diagonals
// and computes T columns of halo on either side for itself
struct BaseTilePlan { int core = 0, nblocks = 0; std::vector<int> ntiles; };
inline BaseTilePlan plan_base_tiles(const int32_t* width, const int32_t* smax, size_t n, int T, int threads) {
  BaseTilePlan p;
  p.core = threads * 2 - 2 * T;
  p.ntiles.resize(n);
  int smax_all = 0;
  for (size_t q = 0; q < n; ++q) {
    p.ntiles[q] = (width[q] + p.core - 1) / p.core;
    smax_all = std::max(smax_all, smax[q]);
  }
  p.nblocks = (smax_all + T - 1) / T + 1;
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
