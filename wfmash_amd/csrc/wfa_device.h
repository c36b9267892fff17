// wfa_device.h -- job descriptors shared by the HIP kernels and the host driver.
#ifndef WFM_WFA_DEVICE_H_
#define WFM_WFA_DEVICE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wfa_rows.h"

namespace wfm {

constexpr int WF_NULL = -(1 << 30);
constexpr int RING = 32;  // rows kept per component; must be >= score scope.  The default penalties (scope 26) and everything
constexpr int RMASK = RING - 1;  // built for them (register tiles, phase 2 from rows computed ahead) use this depth
constexpr int RING_BIG = 128;  // the depth for other penalties whose scope passes 32 (o2 + e2 up to 125): step kernel + base kernel only

// wavefront components (same numbering as oracle/wfa2p.h)
enum { C_M = 0, C_I1 = 1, C_I2 = 2, C_D1 = 3, C_D2 = 4 };
// RLE op codes: entry = (len << 2) | op ; 0 = empty slot
enum { OP_M = 0, OP_X = 1, OP_I = 2, OP_D = 3 };
// backtrace decision byte: bits 0-2 = M source component, bits 3-6 = "came by extension"
enum { BT_I1_EXT = 8, BT_I2_EXT = 16, BT_D1_EXT = 32, BT_D2_EXT = 64 };

constexpr int WFM_DEV_UNREACHABLE = -300;
constexpr int WFM_DEV_OVERFLOW = -2;  // base job exceeded its score budget (smax)
constexpr int WFM_DEV_BAND = -4;      // bialign job ran out of its diagonal band (BpJob::band)
constexpr int WFM_DEV_P2_NOTHING = -6; // phase 2 ended without improving on the breakpoint it was handed (BpJob / P2Job::best0): that one stands
constexpr int WFM_DEV_LIMIT = -7;     // bialign job under a hard score limit (BpJob::limit): a direction stands at the limit and the directions have not met
constexpr int WFM_DEV_P2_MORE = -5;   // phase 2 did not end within the P2K rows computed ahead: the step kernel takes the job
constexpr int WFM_DEV_P2_EXACT_MISS = -8;  // the exact walk (P2Job::exact) found no pair of the job's own score within its reach: the ordinary walk takes the job from the same state

struct DevPen { int x, o1, e1, o2, e2; };

struct BpJob {
  int64_t p_fwd, t_fwd, p_rev, t_rev;  // byte offsets of the sub-range starts in the sequence buffer
  int64_t ring_off;                    // int32 element offset of this job's ring
  int32_t pl, tl;
  int32_t comp_begin, comp_end;
  int32_t width;                       // row stride = round4(pl + tl + 9)
  int32_t koff;                        // column = k + koff (multiple of 4; normally pl + 4)
  int32_t resume_s;                    // -1: start at score 0; >= 0: the forward direction resumes at this score
  int32_t fmax0, rmax0;                // running max antidiagonals at the resume point
  int32_t band;                        // > 0: the ring only holds diagonals |k| <= band + 8 (a job that is expected to end at a low
                                       // score gets a narrow ring); a direction that would pass score `band` ends the job with
                                       // WFM_DEV_BAND and the host runs it again on a full ring.  resume_s == -3: the tile phase
                                       // already ran out of the band
  // resume_sr >= 0: the snapshot is the exact meeting point found by the tile kernels -- forward at resume_s,
  // reverse at resume_sr (= resume_s or resume_s - 1), phase 1 is over; -1: both directions resume at resume_s
  int32_t resume_sr;
  int32_t last_fwd;                    // with resume_sr >= 0: 1 if the forward step was the last one taken
  int32_t sub;                         // upper bound of the job's score (SUB_NONE: none): rows only hold |k - (tl - pl)| <= sub - s
  int32_t best0;                       // > 0: phase 2 resumes with a breakpoint of this score in hand (found by earlier rounds of rows
                                       // computed ahead); only a better one is reported, else WFM_DEV_P2_NOTHING
  int32_t packed;                      // bit 0: both sequences are pure upper-case ACGT -- the tile kernel may read the 2-bit mirror (wfa_tile2.hip);
                                       // bit 1: near-identical sequences (score known to be under a sixteenth of the length): long runs go to the wave's tail at once
  int32_t limit;                       // > 0: the problem's hard score limit (WFM_MODE_SCORE_LIMIT; sub <= limit then).  Phase 1 of the step kernel ends with WFM_DEV_LIMIT
                                       // once the forward direction stands at it with the directions apart: a score within the limit would have brought it to the end
};
static_assert(sizeof(BpJob) == 104, "BpJob::limit fills the struct's tail padding: the job arrays keep their stride");

// ---- time-tiled phase 1 (wfa_tile_kernel) ----
// A block advances every active job by T scores.  A tile owns `core` diagonals of one
// direction of one job, loads core + 2T columns of the snapshot (scope M rows, e1 rows of
// I1/D1, e2 rows of I2/D2) into LDS, runs T steps there (trapezoid: the computed region
// shrinks by one column per side per step) and writes the last `scope` rows of all five
// components of its core back.  Row ranges are closed-form: score s covers
// diagonals [max(-pl,-s), min(tl,s)].
struct TileJob {
  int64_t p_fwd, t_fwd, p_rev, t_rev;
  int64_t ring_in, ring_out;           // int32 element offsets of the two snapshot rings
  int32_t pl, tl;
  int32_t comp_begin, comp_end;
  int32_t width, koff;
  int32_t s0;                          // snapshot score of ring_in
  int32_t active;                      // 0: the meeting point lies in the block after s0 (or the job is over): tiles exit
  int32_t fmax, rmax;                  // running maximum antidiagonals of the two directions up to s0
  int32_t nblocks;                     // tile blocks executed so far (incl. the one that found the meeting point)
  int32_t mode;                        // 0: full blocks; 1: next block stops exactly at the meeting point; 2: stopped there; 6: the block BEFORE s0 runs again (ring_prev, below);
                                       // 5: the block after s0 runs again with per-score maxima (it ran with one maximum for the whole block
                                       // and the wavefronts met inside it: fine_s below)
                                       // (a job with a planned end -- plan_sum below -- knows where mode 1 begins and never takes mode 5)
  int32_t tf, tr;                      // mode >= 1: steps of the forward / reverse direction inside the block after s0
  int32_t last_fwd;                    // mode >= 1: 1 if the forward check ended phase 1 (reverse is one step behind)
  int32_t packed;                      // as BpJob::packed (the job's tiles run wfa_tile2_kernel)
  // mode 4 (phase-2 rows, see P2Job): forward starts at score tf, reverse at tr (s0 is not used), every row goes to the
  // job's P2 rows instead of an output snapshot
  int64_t p2_off;
  int32_t w2, koff2;
  int32_t sub;                         // as BpJob::sub
  // Round 6: the per-score maximum antidiagonals (a six-step DPP reduction per wave and score, a seventh of the step's vector issue) are only
  // needed in the block in which the wavefronts meet.  A block that ends below score fine_s keeps ONE maximum per direction (monotone running
  // maxima: fm + rm >= A at the block's end <=> the directions met somewhere inside it); the advance kernel runs a block that met with a single
  // maximum again with per-score maxima (mode 5) -- a child's score is known, so its last blocks are fine from the start and nothing runs three times.
  int32_t fine_s;
  // Round 6: a block used to write the gap components' rows of its last 26 scores into its output snapshot -- 104 values per diagonal, 60 % of the
  // tile kernel's HBM traffic -- for ONE reader: the run up to the meeting point of the NEXT block, when that run is shorter than 26 scores and
  // its own output (which phase 2 reads 26 rows deep in all five components) needs rows from before its start.  With a third ring the input
  // of the block before (ring_prev) survives one block longer: blocks write the two rows (I1 / D1) and one row (I2 / D2) the next block loads,
  // and when a run up to the meeting point is short, the block before it runs once more WITH its gap rows (mode 6: from ring_prev into ring_out)
  // and the run starts from that.  ring_prev < 0: no third ring (the chunk did not fit one) -- every block writes the 26 rows as before.
  int64_t ring_prev;
  int32_t prev_ok;                     // ring_prev holds the snapshot of score s0 - T (false before the phase's second block)
  int32_t reran;                       // mode-6 runs so far (the host's cell count)
  // The planned end (wfa_plan.h, planned_meet): a job whose score is known need not search for its meeting point.  plan_sum > 0 is sf + sr of the
  // state of the reference's alternating track at which this job's phase 1 ends -- forward (plan_sum + 1) / 2, reverse plan_sum / 2, the forward
  // direction stepped last iff plan_sum is odd; no test of phase 2 before that state can hit, so phase 2 from there finds the reference's
  // breakpoint.  Such a job never reads its maxima score by score: it is never in mode 5, no block of it runs in full only to be run again.  In
  // a chunk that launches both instantiations its fine_s is INT_MAX: every block of it belongs to the one without per-score maxima, and it never
  // counts for the other.  In a chunk that keeps per-score maxima from the first block on (fine_s = 0 for all of its jobs: too many jobs, or
  // too few blocks, for the coarse path -- the flagship workload's deeper levels) its fine_s is 0 like its neighbours' and it rides in that
  // chunk's one launch per block, the instantiation WITH per-score maxima, whose maxima nobody reads for it.  Either way the advance kernel moves it
  // on block by block whatever the maxima say, and when the block behind s0 holds the planned end the job goes to mode 1 (mode 6 first where min(tf, tr) < 26 and
  // ring_prev holds the block before) with the planned tf / tr / last_fwd -- the host does the same at set-up for a planned end in the first
  // block.  The run up to a meeting point takes no maxima: fmax / rmax of such a job are those of s0, and nobody reads them behind an exact end.
  // 0: the job searches (roots, jobs without their bound, the byte kernel's, grown rings, WFM_TILE_PLANNED_END=0).
  int32_t plan_sum;
  // 1: where the run up to the planned end is shorter than the 26 rows phase 2 reads behind it, the block BEFORE it writes the gap rows of its last
  // 26 scores the first time it runs (the stores are mode 6's; the block is known one block ahead, tile_plan_short_next) and no block runs again;
  // 0: that block runs again for them, mode 6, as for a job that searches
  int32_t plan_deep;
};
static_assert(sizeof(TileJob) == 160, "TileJob::plan_sum and its padding behind reran: no field the tile kernels read has moved");
// A job with a planned end that stands at s0 in mode 0: if the block behind s0 holds the planned end, the job's next block is the run up to it
// (the advance kernel between two blocks, the host at set-up).  -> whether it does
__host__ __device__ inline bool tile_plan_enter(TileJob& J, int T) {
  if (J.plan_sum <= 0) return false;
  const int sf = (J.plan_sum + 1) / 2, sr = J.plan_sum / 2;
  if ((sf - 1) / T * T != J.s0) return false;
  J.tf = sf - J.s0; J.tr = sr - J.s0; J.last_fwd = J.plan_sum & 1;
  // (prev_ok: the block before s0 ran as a block of this job -- with plan_deep it wrote the rows a short run needs, tile_plan_short_next)
  J.mode = (J.ring_prev >= 0 && J.prev_ok && !J.plan_deep && (J.tf < J.tr ? J.tf : J.tr) < 26) ? 6 : 1;
  return true;
}
// the block behind s0 of a job in mode 0 is the one BEFORE a run up to the planned end of fewer than 26 steps: it writes its gap rows 26 deep
__host__ __device__ inline bool tile_plan_short_next(const TileJob& J, int T) {
  if (J.plan_sum <= 0 || !J.plan_deep || J.mode != 0) return false;
  const int sf = (J.plan_sum + 1) / 2, sr = J.plan_sum / 2, b0 = (sf - 1) / T * T;
  return b0 == J.s0 + T && sr - b0 < 26;
}

// ---- a child's outer direction from its parent's kept rows (wfa_plan.h, "parent reuse") ----
// A keep is one direction of a job's input snapshot at a block boundary s, compact: KEEP_ROWS rows of n columns (diagonals kmin .. kmin + n - 1),
// row r = keep_row(r): M of score s - r for r < SNAP_ROWS, then I1 of s, s - 1, D1 of s, s - 1, I2 of s, D2 of s; WF_NULL outside a row's own range.
struct KeepTask {
  int32_t* dst;                        // KEEP_ROWS x n
  int32_t job, dir;
  int32_t expect_s;                    // the job keeps only if it stands at this score, active, in mode 0 (it moved on as the host expected)
  int32_t kmin, n;
  int32_t pad_;
};
// The keep into the planes of direction `dir` of the job's ring_in (the job stands at s_k, the keep's score), over the job's own ranges only.
// out[2 * task] |= 1 if a cell written is within `slack` of the job's box (offset >= min(tl, pl + k) - slack: the parent may have run past a wall
// the child stops at); out[2 * task + 1] = the largest antidiagonal 2 h - k of the M cells written.
struct RestoreTask {
  const int32_t* src;
  int32_t job, dir;
  int32_t s_k, kmin, n;
  int32_t slack;
};
void launch_keep(const int32_t* ring, const TileJob* jobs, const KeepTask* tasks, int ntasks, int max_n, hipStream_t st);
void launch_restore(int32_t* ring, const TileJob* jobs, const RestoreTask* tasks, int32_t* out, int ntasks, int max_n, hipStream_t st);

// ---- phase 2 (overlap detection) without a step-by-step kernel ----
// wavefront_bialign_find_breakpoint's second loop alternates "test the newest row of one direction against the last
// `scope` rows of the other" and "advance the other direction by one row" until no better breakpoint is possible
// -- about 2 * scope rows past the meeting point.  The rows do not depend on the tests, so they are computed ahead:
// the tile kernel runs P2K more scores of both directions from the exact snapshot and keeps EVERY row (five components,
// [dir][comp][P2K][w2]); wfa_p2_blockmax_kernel takes the maxima of every row per component and per block of 64
// diagonals (a pair of rows can only meet where both are far along: the block maxima prune by POSITION, which the row
// maxima cannot -- a direction that has already crossed most of the text would otherwise let every diagonal of the other
// through); wfa_p2_overlap_kernel then walks the reference's loop, one workgroup per job, with nothing but
// the tests left in it (doing all tests of a job side by side was tried: without the best breakpoint so far to prune
// with, the tests after the first hit cost more than the whole sequential walk).  A job whose loop has not ended after
// 2 * P2K tests (WFM_DEV_P2_MORE) is finished by wfa_bp_kernel from the same snapshot.
// A job that stands at the end planned from its known score needs neither the maxima nor the pruning: only pairs of rows of exactly its own
// score can be the breakpoint, one row per component and test (P2Job::exact, wfa_p2_exact_kernel).  A chunk's jobs that search come first on
// the device, the maxima and the two kernels above are theirs alone; below the roots' level a chunk usually has none.
constexpr int P2K = 32;            // (48 until jobs could take further rounds: most walks end within 2 x 26 tests, and the rows of the
                                    // others are computed when they are asked for -- C3 109 -> 106 ms per step, C1 substitute 5.5 -> 5.4 s)
constexpr int P2ROWS = SNAP_ROWS + P2K;  // row maxima per direction: the snapshot's rows sd-25 .. sd, then sd+1 .. sd+P2K
constexpr int P2TESTS = 2 * P2K;
constexpr int P2ENT = RING * 5;    // (row of the other direction, component) slots of a test; scope <= RING rows are used
struct P2Job {
  int64_t ring_in;                     // the exact snapshot (rows <= sf / sr), int32 element offset of the job's ring
  int64_t p2_off;                      // int32 element offset of the job's P2 rows
  int32_t width, koff;                 // ring geometry
  int32_t w2, koff2;                   // P2 geometry: column = k + koff2
  int32_t pl, tl;
  int32_t sf, sr, last_fwd;            // state at the meeting point
  int32_t sub, best0;                  // as BpJob::sub, BpJob::best0
  int32_t nblk;                        // 64-diagonal blocks of a row: block of diagonal k = (k + koff2) >> 6
  // > 0: the job stands at the end planned from its known score, sf + sr = exact = that score (wfa_plan.h, planned_meet): no pair of rows is
  // cheaper, so the walk only looks at the pairs of exactly this score, at most one row per component and test, and ends at the first that
  // meets (wfa_p2_exact_kernel: no maxima, no bm_off).  0: the job searches (wfa_p2_blockmax_kernel, wfa_p2_overlap_kernel)
  int32_t exact;
  int64_t bm_off;                      // int32 element offset of the job's block maxima [dir][P2ROWS][comp][nblk]
};
static_assert(sizeof(P2Job) == 80, "P2Job is built by the host per launch: nothing else holds its layout");

struct BpResult {
  int32_t status;  // 0 breakpoint found; 1 end reached at score 0; <0 error
  int32_t score, score_fwd, score_rev, k_fwd, off_fwd, comp;
  int32_t steps;
  uint64_t cells;
  int32_t steps_p1;            // steps spent before the antidiagonals met
  uint32_t ticks_p1, ticks_p2; // wall_clock64 ticks (100 MHz) per phase
  int32_t pad_;
  uint32_t ticks_list, ticks_pick;  // wfa_p2_overlap_kernel: the block-listing and the pick stages (diagnostics)
  uint32_t work_items, pad2_;       // blocks listed over all rounds
};

struct BaseJob {
  int64_t p_off, t_off;  // byte offsets of the (forward) sub-range starts
  int64_t pre_off;       // int32 element offset: pre[(smax+1)][width]
  int64_t bt_off;        // byte offset: bt[(smax+1)][width]
  int64_t ring_off;      // int32 element offset: ring[5][RING][width]
  int64_t rle_end;       // exclusive end of this job's slot in the RLE buffer
  int32_t pl, tl;
  int32_t comp_begin, comp_end;
  int32_t endsfree, pbf, pef, tbf, tef;
  int32_t smax, kmin, width;
  int32_t type;          // 0 WFA; 1 all-D (tl == 0); 2 all-I (pl == 0)
  int32_t pad_;
  int32_t score_only;    // nonzero: the job ends behind its forward pass -- BaseResult::score is all it reports, no walk back, nothing written to the RLE slots
};
static_assert(sizeof(BaseJob) == 112, "BaseJob::score_only fills the struct's tail padding: the job arrays keep their stride");

struct BaseResult {
  int32_t status;  // 0 ok; WFM_DEV_OVERFLOW; <0 error
  int32_t score;
  int32_t nruns;
  int32_t pad_;
  uint64_t cells;
};

// ---- base jobs whose rows are wider than one workgroup's registers hold (wfa_base2t_kernel, round 6) ----
// A patch that overflowed its budget of 1020 ran on r32::wfa_base_kernel<1024> until round 6: one workgroup per job, 6 us per score step over rows of
// 3 k diagonals from a global-memory ring, a dozen jobs on a device of 256 CUs for 9 ms at the end of every batch.  Here the columns of such a job are
// cut into tiles as the tile phase of BiWFA cuts its rows: a launch is one BLOCK of T scores, every tile a workgroup that holds core + 2 T diagonals in
// the register kernel's delay lines (wfa_base2_kernel's step, its decisions, its rows of pre / bt -- written for the core only), T columns of halo on
// either side that it computes for itself and that go wrong one column per step from the outside, a snapshot of the last 26 rows between two blocks.
// A tiny kernel between two launches replays the end test over the tiles of a job (the first score at which a cell ends, the smallest such diagonal),
// and one wave per job walks back through pre / bt at the end (base_walk in wfa_base.h: every base kernel's walk).
struct Base2TJob {
  BaseJob b;                   // as for wfa_base2_kernel; b.ring_off: two snapshots of B2T_ROWS rows x width behind each other
  int64_t snap_in, snap_out;   // int32 element offsets of the snapshot the next block loads / writes
  int32_t ntiles, core;        // tiles of `core` diagonals from b.kmin on
  int32_t task0;               // the job's first entry in the task list (its tiles follow each other)
  int32_t s0;                  // score the next block starts from (0: row 0 is still to be made)
  int32_t done;                // 0 running, 1 an end was found (end_s / end_k / end_off), 2 the budget is spent
  int32_t end_s, end_k, end_off;
};
struct Base2TTask { int32_t job, tile; };
constexpr int B2T_ROWS = 32;   // rows of a snapshot: M of the last 26 scores, I1 / D1 of the last two, I2 / D2 of the last
constexpr int B2T_THREADS = 512;
void launch_base2t_block(const uint32_t* pk, int32_t* a32, uint8_t* a8, const Base2TJob* jobs, const Base2TTask* tasks, unsigned long long* tile_key,
                         int32_t* tile_off, int ntasks, int T, hipStream_t st);
void launch_base2t_advance(Base2TJob* jobs, const unsigned long long* tile_key, const int32_t* tile_off, int njobs, int T, int32_t* active_slot, hipStream_t st);
void launch_base2t_finish(const int32_t* a32, const uint8_t* a8, uint32_t* rle, const Base2TJob* jobs, BaseResult* res, int njobs, hipStream_t st);

// ---- an upper bound of a root's score before its wavefronts are computed (wfa_bound_kernel) ----
struct BoundJob { int64_t p_off, t_off; int32_t pl, tl; };
void launch_bound(const uint8_t* seq, const BoundJob* jobs, int32_t* out, int njobs, DevPen pen, hipStream_t st);

// reversed copies of the sequences of a BiWFA problem, made on the device (wfm_upload_sequences)
struct SeqRev { int64_t p_fwd, p_rev, t_fwd, t_rev; int32_t plen, tlen; };
void launch_reverse(uint8_t* seq, const SeqRev* jobs, int njobs, int pad, hipStream_t st);
// a window of a device-resident sequence copied into a seqset (wfm_upload_sequence_refs): len bytes from src to dst, read backwards
// (reverse) and / or with A<->T, C<->G swapped (complement), then pad zero bytes; any alignment of src and dst.  A task covers at
// most WFM_SEQ_GATHER_CHUNK bytes; the aligned 16-byte words of the source it reads reach at most 15 bytes beyond [src, src + len).
struct SeqGatherTask { const uint8_t* src; uint8_t* dst; int32_t len, pad; int32_t reverse, complement; };
void launch_seq_gather(const SeqGatherTask* tasks, int64_t ntasks, hipStream_t st);
// wfm_check_runs (wfa_check.hip): a problem's forward byte copies in the seqset, its runs, and what its result claims
struct CheckProb {
  int64_t p_off, t_off;                // byte offsets of the forward copies in the sequence buffer
  uint64_t run_off;                    // index of the problem's first run
  uint32_t n_runs;
  int32_t plen, tlen;
  int32_t pbf, pef, tbf, tef;          // ENDSFREE allowances (0 for the other modes)
  int32_t res_score;                   // < 0: the price is not compared
  uint32_t res_ops_len;
  int32_t skip;                        // nonzero: WFM_CK_NOT_CHECKED (score-only, or status != 0)
};
struct CheckTask { int32_t prob, slice; };  // ops [slice, slice + 1) * WFM_CHECK_SLICE of a problem
// scan, compare and finish on st.  ops_pre / p_pre / t_pre: one element per run of the call; cmp_ops / keys: one per problem; out: nprob wfm_check_t
void launch_check(const uint8_t* seq, const uint32_t* runs, const CheckProb* probs, int nprob, const CheckTask* tasks, int64_t ntasks,
                  uint32_t* ops_pre, uint32_t* p_pre, uint32_t* t_pre, uint32_t* cmp_ops, unsigned long long* keys, void* out, DevPen pen,
                  hipStream_t st);
// wfm_left_align_runs (wfa_leftalign.hip): a problem's forward byte copies, its runs, its slots in the output (n_runs + n_gaps of them)
// and in the list of interior gaps
struct LaProb {
  int64_t p_off, t_off;
  uint64_t run_off, out_off, gap_off;
  uint32_t n_runs, n_gaps;             // n_gaps: interior I / D runs (neither the first nor the last run)
  int32_t plen, tlen;
  int32_t skip, pad_;                  // nonzero: WFM_LA_NOT_DONE (score-only, or status != 0)
};
struct LaGap { int64_t s_off; uint32_t g, len, prob, run; };  // S = the sequence buffer at s_off; the gap covers S[g, g + len); run: its index in the problem
// index, rot (one lane per gap, then one wave per gap of the second list), shift + rewrite, on st.  rot / dval: one element per run of the call;
// flags: one per problem; gaps / long_list: ngaps; long_count: 1, zeroed by the caller; stats: nprob wfm_leftalign_t.  lane_max: the bases after
// which a gap leaves the lane kernel for the wave kernel
void launch_left_align(const uint8_t* seq, const uint32_t* runs, const LaProb* probs, int nprob, uint32_t* rot, uint32_t* dval, LaGap* gaps,
                       uint64_t ngaps, uint32_t* flags, uint32_t* long_list, uint32_t* long_count, uint32_t* out, void* stats, uint32_t lane_max,
                       hipStream_t st);
// wfm_cs_strings (wfa_cs.hip): a problem's forward byte copies, its runs and its slots in the table of run records (one uint4 per run:
// pattern index, text index, offset of the run's bytes in the problem's string, the run)
struct CsProb {
  int64_t p_off, t_off;
  uint64_t run_off, rec_off;
  uint32_t n_runs;
  int32_t plen, tlen;
  int32_t skip;                        // nonzero: WFM_CS_NOT_DONE (score-only, status != 0, no runs)
};
// recs: one uint4 per run of the problems that are not skipped; totals / flags: one per problem (a flagged problem's total is 0)
void launch_cs_index(const uint32_t* runs, const CsProb* probs, int nprob, int form, void* recs, unsigned long long* totals, uint32_t* flags,
                     hipStream_t st);
// the problems [ka, kb), whose strings are the chunk_bytes bytes behind goff[ka] (goff: the n + 1 offsets of the call's strings), into out,
// which holds chunk_bytes rounded up to a multiple of WFM_CS_SLICE
void launch_cs_write(const uint8_t* seq, const CsProb* probs, const void* recs, const unsigned long long* goff, uint32_t ka, uint32_t kb,
                     unsigned long long chunk_bytes, int form, uint8_t* out, hipStream_t st);
// wfm_maf_rows (wfa_maf.hip): the problems are CsProb as well, but a problem takes n_runs + 1 slots at rec_off (the last holds its totals).
// recs: one uint4 per slot (pattern index, text index, WRITTEN columns before the run, the run); pre: one uint2 per slot (aligned columns
// and = columns before the run); nblk / ncols / flags: one per problem (a flagged problem's are 0)
void launch_maf_index(const uint32_t* runs, const CsProb* probs, int nprob, uint32_t split, void* recs, void* pre, unsigned long long* nblk,
                      unsigned long long* ncols, uint32_t* flags, hipStream_t st);
// the problems [ka, kb): their n_blocks = boff[kb] - boff[ka] blocks into blocks (40 bytes each, wfm_maf_block_t) and the chunk_bytes bytes
// of their rows behind goff[ka] into out, which holds chunk_bytes rounded up to a multiple of WFM_MAF_SLICE and is 16-byte aligned (goff /
// boff: the n + 1 offsets of the call's rows and blocks)
void launch_maf_write(const uint8_t* seq, const CsProb* probs, const void* recs, const void* pre, const unsigned long long* nblk,
                      const unsigned long long* goff, const unsigned long long* boff, uint32_t ka, uint32_t kb, unsigned long long chunk_bytes,
                      void* blocks, uint32_t n_blocks, uint8_t* out, hipStream_t st);
// wfm_call_variants (wfa_variants.hip): the problems are CsProb as well.  recs: one uint4 per run of the problems that are not skipped
// (pattern index, text index, offset of the run's allele bytes in the problem's, the run), rpre: the index of the run's first record in
// the problem's; tot_bytes / tot_recs / end_gaps / flags: one per problem (a flagged problem's are 0)
void launch_var_index(const uint32_t* runs, const CsProb* probs, int nprob, void* recs, uint32_t* rpre, unsigned long long* tot_bytes,
                      unsigned long long* tot_recs, uint32_t* end_gaps, uint32_t* flags, hipStream_t st);
// the problems [ka, kb): their chunk_bytes allele bytes behind goff[ka] into out, which holds chunk_bytes rounded up to a multiple of
// WFM_VAR_SLICE, and their voff[kb] - voff[ka] records into vars, 32 bytes each (goff / voff: the n + 1 offsets of the call's problems)
void launch_var_write(const uint8_t* seq, const CsProb* probs, const void* recs, const uint32_t* rpre, const unsigned long long* goff,
                      const unsigned long long* voff, uint32_t ka, uint32_t kb, unsigned long long chunk_bytes, uint8_t* out, void* vars,
                      hipStream_t st);
// wfm_coverage_* (wfa_coverage.hip).  A problem is wfm_cov_prob_t as the caller wrote it; d: the difference array, a whole number of
// tiles of WFM_COV_TILE words of which the first n_bases + 1 are used
struct CovProb {
  uint64_t base, runs_off;
  uint32_t n_runs, pad_;
};
void launch_cov_add(const uint32_t* runs, const CovProb* probs, int nprob, int32_t* d, unsigned long long n_bases, uint32_t* flags, hipStream_t st);
// count, sum, scan of sums, apply: tile_cnt: ntiles; sums: ntiles / WFM_COV_SCAN_BLOCK rounded up, + 1; tile_off: ntiles + 1
void launch_cov_tile_offsets(const int32_t* d, unsigned long long ntiles, uint32_t* tile_cnt, unsigned long long* sums, unsigned long long* tile_off,
                             hipStream_t st);
// the non-zero words of the tiles [tile_a, tile_b) as 16-byte entries; out[0] is entry number out_base of the whole list
void launch_cov_write(const int32_t* d, const unsigned long long* tile_off, unsigned long long tile_a, unsigned long long tile_b,
                      unsigned long long out_base, void* out, hipStream_t st);
void launch_cov_import(const void* ent, unsigned long long n, int32_t* d, hipStream_t st);
// m entries of the list to m intervals (sum, scan of sums, apply).  sums: m / WFM_COV_SCAN_BLOCK rounded up, + 1; *carry: the depth behind
// the entries of the chunks before (0 at the first), brought up to date; prev_pos: the pos of the entry before ent[0]; last: this is the
// list's last chunk; totals: three words, zeroed before the first chunk
void launch_cov_intervals(const void* ent, unsigned long long m, unsigned long long* sums, unsigned long long* carry, unsigned long long prev_pos,
                          unsigned long long n_bases, int last, void* iv, unsigned long long* totals, hipStream_t st);
// wfm_liftset_* / wfm_lift_runs (wfa_lift.hip).  A problem is wfm_cov_prob_t with the place of its n_runs + 1 prefix words in `pre`; what
// lift_index_kernel leaves per problem: its window [lo, hi) of candidate intervals, how many of them overlap it, its flags, its pattern span
struct LiftProb {
  uint64_t base, runs_off, pre_off;
  uint32_t n_runs, pad_;
};
struct LiftWin {
  uint64_t lo, hi, count;
  uint32_t flags, plen;
};
// iv: n intervals {start, end}, 16 bytes each, sorted; maxs: n / WFM_LIFT_SCAN_BLOCK rounded up; pm: n
void launch_lift_pm(const void* iv, unsigned long long n, unsigned long long* maxs, unsigned long long* pm, hipStream_t st);
// pre: 16-byte words, the problems' n_runs + 1 each; win: nprob; off: nprob + 1
void launch_lift_index(const uint32_t* runs, const LiftProb* probs, int nprob, const void* iv, const unsigned long long* pm, unsigned long long n_iv,
                       unsigned long long n_bases, void* pre, LiftWin* win, unsigned long long* off, hipStream_t st);
// the lifts of the problems [ka, kb), 32 bytes each; out[0] is lift number off[ka] of the call
void launch_lift_write(const uint32_t* runs, const LiftProb* probs, const void* iv, const void* pre, const LiftWin* win, const unsigned long long* off,
                       uint32_t ka, uint32_t kb, void* out, hipStream_t st);
// wfm_chain_runs (wfa_chain.hip).  A problem is wfm_chain_prob_t with the place of its n_runs + 1 prefix words in `pre`; what
// chain_index_kernel leaves per problem: its blocks, its flags, the bases before the first and behind the last block (as the problem's flags
// order them) and its = and X columns
struct ChainProb {
  uint64_t runs_off, pre_off;
  uint32_t n_runs, flags;
};
struct ChainWin {
  uint64_t count;
  uint32_t flags, lead_dt, lead_dq, trail_dt, trail_dq, eq, x, pad_;
};
// pre: 16-byte words, the problems' n_runs + 1 each; win: nprob; off: nprob + 1
void launch_chain_index(const uint32_t* runs, const ChainProb* probs, int nprob, void* pre, ChainWin* win, unsigned long long* off, hipStream_t st);
// the blocks of the problems [ka, kb), 16 bytes each; out[0] is block number off[ka] of the call
void launch_chain_write(const uint32_t* runs, const ChainProb* probs, const void* pre, const ChainWin* win, const unsigned long long* off, uint32_t ka,
                        uint32_t kb, void* out, hipStream_t st);
// wfm_pav_* (wfa_pav.hip).  A problem is wfm_pav_prob_t as the caller wrote it.  A segment list is two arrays of keys, ks[i] = group << 40 |
// start and ke[i] = group << 40 | end
struct PavProb {
  uint64_t base, runs_off;
  uint32_t n_runs, group;
};
// flags: nprob; cnt: nprob, the segments each problem will write (0 where flagged); off: nprob + 1, their exclusive prefixes.  eq_only: a
// segment is a maximal stretch of = runs (wfm_sites_add_ref), not of =/X runs (wfm_pav_add); the same for launch_pav_write
void launch_pav_count(const uint32_t* runs, const PavProb* probs, int nprob, unsigned long long n_bases, uint32_t n_groups, uint32_t* flags,
                      unsigned long long* cnt, unsigned long long* off, bool eq_only, hipStream_t st);
// the segments of the problems, problem i's from slot off[i] of ks / ke on (the caller has made room for off[nprob] of them)
void launch_pav_write(const uint32_t* runs, const PavProb* probs, int nprob, const uint32_t* flags, const unsigned long long* off,
                      unsigned long long* ks, unsigned long long* ke, bool eq_only, hipStream_t st);
// rocprim::radix_sort_pairs of (ks, ke) by ks into (ks2, ke2), bits [0, end_bit); tmp == nullptr: *tmp_bytes = what it needs
hipError_t pav_sort(void* tmp, size_t* tmp_bytes, const unsigned long long* ks, unsigned long long* ks2, const unsigned long long* ke,
                    unsigned long long* ke2, unsigned long long n, unsigned end_bit, hipStream_t st);
// ke (sorted by ks) to its inclusive running maximum, in place; aux: n / WFM_PAV_SCAN_BLOCK rounded up, + 1
void launch_pav_runmax(unsigned long long* ke, unsigned long long n, unsigned long long* aux, hipStream_t st);
// the union of (ks, rm), rm the running maximum: its intervals to (uks, uke), their number to aux[number of blocks]
void launch_pav_compact(const unsigned long long* ks, const unsigned long long* rm, unsigned long long n, unsigned long long* aux,
                        unsigned long long* uks, unsigned long long* uke, hipStream_t st);
// C[i] = the bases of the union intervals before i, C[m] = all of them
void launch_pav_prefix(const unsigned long long* uks, const unsigned long long* uke, unsigned long long m, unsigned long long* aux,
                       unsigned long long* C, hipStream_t st);
// the cells of rows [ra, rb), out[(j - ra) * n_groups + g]; iv: {start, end}, 16 bytes an interval
void launch_pav_matrix(const unsigned long long* uks, const unsigned long long* uke, const unsigned long long* C, unsigned long long m, const void* iv,
                       unsigned long long ra, unsigned long long rb, uint32_t n_groups, uint32_t* out, hipStream_t st);
// wfm_sites_* (wfa_sites.hip).  A variant is wfm_site_var_t as the caller wrote it, its REF at alle[off .. off + ref_len), its ALT behind.
struct SiteVar {
  uint64_t pos;
  uint32_t kind, group;
  uint32_t ref_len, alt_len;
  uint64_t off;
};
struct SiteRow {  // wfm_site_t; off: still the representative's place in the object's allele block
  uint64_t pos;
  uint32_t kind, n_carrier_groups;
  uint32_t ref_len, alt_len;
  uint64_t off;
};
// what the table call has on the device; every array but tasks has n elements (first and gfirst n + 1)
struct SitesWork {
  unsigned long long *k1, *k2, *kg, *ks;  // pos << 2 | kind; the hash; a gathered key; a sorted key (in the end: the sorted k1, and kg the sorted k2)
  uint32_t *k3, *sk3, *pa, *pb;           // the group; the sorted group; two permutations
  uint32_t *first, *gfirst;               // per site its first sorted record and the distinct (site, group) pairs before it
  uint8_t* flag;                          // per sorted record: 0 not a head, 1 a head by its keys, 2 long alleles still equal, 3 a head by a collision
  const unsigned long long* tasks;        // record << 32 | piece, a piece = WFM_SITES_TASK bytes of a long allele pair
  unsigned long long* aux;                // the blocks' sums: n / WFM_PAV_SCAN_BLOCK rounded up, + 1; then one word: the collisions
};
// upper case in place
void launch_sites_fold(uint8_t* alle, unsigned long long bytes, hipStream_t st);
// k1, k2 (masked to hash_bits), k3 of every variant, and pa = 0, 1, 2, ...
void launch_sites_keys(const SiteVar* vars, const uint8_t* alle, uint32_t n, const SitesWork& w, unsigned long long n_tasks, unsigned hash_bits, hipStream_t st);
// out[i] = in[perm[i]]
void launch_sites_gather64(const unsigned long long* in, const uint32_t* perm, uint32_t n, unsigned long long* out, hipStream_t st);
void launch_sites_gather32(const uint32_t* in, const uint32_t* perm, uint32_t n, uint32_t* out, hipStream_t st);
// stable rocprim::radix_sort_pairs over bits [0, end_bit); tmp == nullptr: *tmp_bytes = what it needs
hipError_t sites_sort64(void* tmp, size_t* tmp_bytes, const unsigned long long* k, unsigned long long* k2, const uint32_t* v, uint32_t* v2, uint32_t n,
                        unsigned end_bit, hipStream_t st);
hipError_t sites_sort32(void* tmp, size_t* tmp_bytes, const uint32_t* k, uint32_t* k2, const uint32_t* v, uint32_t* v2, uint32_t n, unsigned end_bit,
                        hipStream_t st);
// the heads of the sorted list (keys w.ks, w.kg, w.sk3; permutation perm; inv: n words of room), compacted: w.first, w.gfirst; the sites'
// number in the low and the (site, group) pairs in the high half of w.aux[blocks], the collisions in w.aux[blocks + 1]
void launch_sites_heads(const SiteVar* vars, const uint8_t* alle, uint32_t n, const SitesWork& w, const uint32_t* perm, uint32_t* inv,
                        unsigned long long n_tasks, hipStream_t st);
void launch_sites_rows(const SiteVar* vars, const uint32_t* perm, const uint32_t* first, const uint32_t* gfirst, uint32_t n_sites, SiteRow* rows, hipStream_t st);
// the cells of rows [ra, rb), out[(s - ra) * n_groups + g] = '0' / '1' / '.'; (uks, uke, C, m): the = union as wfm_pav_union leaves it
void launch_sites_gt(const SiteRow* rows, const uint32_t* first, const uint32_t* sk3, const unsigned long long* uks, const unsigned long long* uke,
                     const unsigned long long* C, unsigned long long m, unsigned long long ra, unsigned long long rb, uint32_t n_groups, uint8_t* out,
                     hipStream_t st);
// wfm_net_* (wfa_net.hip).  A problem is wfm_net_prob_t as the caller wrote it, a block wfm_net_block_t, a record entry wfm_net_rec_t.
struct NetProb {
  uint64_t base, runs_off;
  uint32_t n_runs, score;
  uint64_t order;
};
struct NetBlock {
  uint64_t order, t;
  uint32_t q, size;
};
struct NetRec {
  uint64_t order;
  uint32_t score, zero;
};
struct NetPer {  // wfm_netcall_t
  uint64_t order;
  uint32_t score, zero;
  uint64_t first, count, won, aligned;
};
// flags: nprob; word: nprob, (1 << 32 where the problem is taken) | the blocks it will write; off: nprob + 1, their exclusive prefixes (the
// records before a problem in the high half, the blocks in the low one); score: nprob, the score each record competes with
void launch_net_count(const uint32_t* runs, const NetProb* probs, int nprob, unsigned long long n_bases, uint32_t* flags, unsigned long long* word,
                      unsigned long long* off, uint32_t* score, hipStream_t st);
// the record entry and the blocks of every problem taken, from slots off[i] >> 32 of recs and off[i] & 0xffffffff of blocks on
void launch_net_write(const uint32_t* runs, const NetProb* probs, int nprob, const uint32_t* flags, const unsigned long long* off, const uint32_t* score,
                      NetBlock* blocks, NetRec* recs, hipStream_t st);
// what the table call has on the device
struct NetWork {
  const NetBlock* blocks; unsigned long long n;  // the object's blocks
  const NetRec* recs; uint32_t r;                // and record entries
  unsigned long long *e, *e2;          // 2 n: the block ends, and sorted; e then holds x, the m + 1 distinct coordinates
  unsigned long long* aux;             // the blocks' sums of a scan: 2 n / WFM_NET_SCAN_BLOCK rounded up, + 2
  uint32_t* brank;                     // n: the rank in order of a block's record
  unsigned long long *ro, *so;         // r: the orders, and sorted
  uint32_t *ri, *sp;                   // r: 0, 1, 2, ...; the record at each rank
  unsigned long long *k2, *k2s;        // r: ~score << 32 | rank, and sorted
  uint32_t *p2, *prio, *sscore;        // r: the rank at each place of that sort; the priority (1 .. r) and the score by rank
  unsigned long long *aligned, *won;   // r: by rank
  uint32_t* bad;                       // 2 words: equal orders; blocks without a record
  unsigned long long* tree;            // 2 m: node 1 the root, the leaves from m on
  unsigned long long m;
  unsigned long long *ps, *pe, *pw;    // p: a piece's start, end and winner
  uint32_t *key, *val, *sk, *sv;       // p: the winner's rank and 0, 1, 2, ..., and sorted
  unsigned long long p;
};
void launch_net_ends(const NetWork& w, hipStream_t st);
hipError_t net_sort_keys(void* tmp, size_t* tmp_bytes, const unsigned long long* k, unsigned long long* k2, unsigned long long n, unsigned end_bit, hipStream_t st);
// the distinct values of the sorted e2 to e; their number to aux[number of scan blocks]
void launch_net_distinct(const NetWork& w, hipStream_t st);
// ro = the orders, ri = 0, 1, 2 ...
void launch_net_rec_keys(const NetWork& w, hipStream_t st);
// (so, sp) sorted by order: bad[0] where two neighbours are equal, k2 = ~score << 32 | rank, sscore
void launch_net_rec_rank(const NetWork& w, hipStream_t st);
// (k2s, p2) sorted: prio[p2[i]] = r - i
void launch_net_prio(const NetWork& w, hipStream_t st);
// one lane per block: brank, aligned, and the maxima into the tree's canonical nodes
void launch_net_fill(const NetWork& w, hipStream_t st);
// the maxima pushed down, one launch per level
void launch_net_push(const NetWork& w, hipStream_t st);
// the number of pieces to aux[number of scan blocks]; then, with room for them, their starts, ends and winners
void launch_net_heads_count(const NetWork& w, hipStream_t st);
void launch_net_heads_write(const NetWork& w, hipStream_t st);
// key = the winner's rank, val = 0, 1, 2 ..., won
void launch_net_piece_keys(const NetWork& w, hipStream_t st);
// the pieces at the sorted places [a, b), 24 bytes each
void launch_net_pieces(const NetWork& w, unsigned long long a, unsigned long long b, NetBlock* out, hipStream_t st);
void launch_net_per(const NetWork& w, NetPer* per, hipStream_t st);
// wfm_trans_* (wfa_trans.hip).  A problem is wfm_trans_prob_t as the caller wrote it; what trans_span_kernel leaves per problem: its flags
// and its two spans.  An arc is one direction of a record: its source [s, s + slen) and the start d of its destination in the world, where
// its record's n_runs + 1 prefix words begin in the object's block (the low 62 bits of pre), whether its source is the query window
// (TRANS_ARC_BACK) and whether the record's text is the reverse complement of that window (TRANS_ARC_REVERSE).
struct TransProb {
  uint64_t t, q, runs_off;
  uint32_t n_runs, flags;
};
struct TransSpan {
  uint32_t flags, pspan, tspan, pad_;
};
struct TransArc {
  uint64_t s, d, pre;
  uint32_t slen, n_runs;
};
constexpr uint64_t TRANS_ARC_BACK = (uint64_t)1 << 62, TRANS_ARC_REVERSE = (uint64_t)1 << 63, TRANS_ARC_PRE = TRANS_ARC_BACK - 1;
void launch_trans_span(const uint32_t* runs, const TransProb* probs, int nprob, unsigned long long n_bases, TransSpan* out, hipStream_t st);
// pre_off: nprob, where each problem's words begin in pre, ~0 for a problem that is not kept
void launch_trans_pre(const uint32_t* runs, const TransProb* probs, int nprob, const unsigned long long* pre_off, void* pre, hipStream_t st);
// key[i] = arc i's source start, idx[i] = i: what pav_sort takes
void launch_trans_keys(const TransArc* arcs, unsigned long long n, unsigned long long* key, unsigned long long* idx, hipStream_t st);
// sorted[i] = arcs[idx[i]]; pm[i] = the largest source end of sorted[0 .. i]; maxs: n / WFM_TRANS_SCAN_BLOCK rounded up
void launch_trans_index(const TransArc* arcs, const unsigned long long* idx, unsigned long long n, TransArc* sorted, unsigned long long* maxs,
                        unsigned long long* pm, hipStream_t st);
// (ks, ke): the m intervals of the list, keys seed << 40 | position; (pks, pke): the m_prev of the list before; arcs sorted, pm theirs.
// win: m windows {lo, hi}, 16 bytes each; cnt: m; off: m + 1, the counts' exclusive prefixes
void launch_trans_count(const unsigned long long* ks, const unsigned long long* ke, unsigned long long m, const unsigned long long* pks,
                        const unsigned long long* pke, unsigned long long m_prev, const TransArc* arcs, const unsigned long long* pm,
                        unsigned long long n_arcs, void* win, unsigned long long* cnt, unsigned long long* off, hipStream_t st);
// the pairs of the intervals [ka, kb) as keys; oks[0] / oke[0] is pair number off[ka] of the round
void launch_trans_write(const unsigned long long* ks, const unsigned long long* ke, const void* win, const unsigned long long* off,
                        unsigned long long ka, unsigned long long kb, const TransArc* arcs, const void* pre, unsigned long long* oks,
                        unsigned long long* oke, hipStream_t st);
// wfm_check_optimal (wfa_optcheck.hip): a problem's forward byte copies, its ends-free allowances (clamped; 0 for the other modes),
// its band of diagonals (wfa_optband.h) and, for the memory form, where its three row arrays begin in `rows` (32-bit elements)
struct OptProb {
  int64_t p_off, t_off, row_off;
  int32_t plen, tlen;
  int32_t pbf, pef, tbf, tef;
  int32_t band_lo, band_hi;
};
// one workgroup per problem; form 0 / 1 / 2: rows in registers, 1 / 4 / 8 diagonals per thread (bands up to WFM_OPT_BAND_C1 / _C4 /
// WFM_OPT_REG_MAX); form 3: rows in `rows`, 3 x (tiles x WFM_OPT_REG_MAX + 1) elements per problem.  out[i]: the banded optimum or -1
void launch_optcheck(const uint8_t* seq, const OptProb* probs, int nprob, int form, int32_t* rows, int32_t* out, DevPen pen, hipStream_t st);
// makeUpperCaseAndValidDNA in place on nbytes (rounded up to 16) from a 16-byte aligned device address (wfm_seqstore_add)
void launch_seq_normalize(uint8_t* seq, int64_t nbytes, hipStream_t st);
// the 2-bit mirror of the sequence buffer (word i = bytes 16 i .. 16 i + 15) and, per BiWFA problem, "pure ACGT" (flag stays nonzero)
void launch_seq_pack(const uint8_t* seq, uint32_t* pk, int64_t nwords, int64_t nbytes, const SeqRev* jobs, int njobs, int32_t* flag, hipStream_t st);
constexpr int64_t PK_PAD_WORDS = 2048 + 64;  // words of padding behind the mirror: a tile stages a whole window from any origin inside
// the tile kernel on packed sequences (wfa_tile2.hip): same contract as launch_tile_reg / launch_tile_p2
void launch_tile2(const uint32_t* pk, int32_t* ring, const TileJob* jobs, const TileTask* tasks, int32_t* mak, int ntasks, int threads, int T, int variants, hipStream_t st);
// LDS slots per score of the packed kernel's per-score maxima (its FAST + FINE phase-1 form), by workgroup size: (T + 1) * slots * 4 bytes of
// dynamic LDS beside ~17.5 KB of static, sized so that the workgroups a CU holds by registers still fit its 160 KB (8 of 128 threads, 4 of 256)
#ifndef WFM_TILE_SLOTS_WIDE
#define WFM_TILE_SLOTS_WIDE 16
#endif
constexpr int TILE_SLOTS_WAVE1 = 2, TILE_SLOTS_SMALL = 4, TILE_SLOTS_WIDE = WFM_TILE_SLOTS_WIDE;
constexpr int tile_fine_slots(int threads) { return threads <= 64 ? TILE_SLOTS_WAVE1 : (threads <= 128 ? TILE_SLOTS_SMALL : TILE_SLOTS_WIDE); }
bool tile2_coarse_maxima();  // wfa_tile2_kernel keeps one maximum per block below TileJob::fine_s (the FAST form; WFM_TILE_COARSE=0: per score always)
void launch_tile2_p2(const uint32_t* pk, int32_t* ring, const TileJob* jobs, const TileTask* tasks, int ntasks, int threads, int32_t* p2, hipStream_t st);
int selftest_dpp(int* host_out128, hipStream_t st);
// leaves and patches on registers and packed sequences (default penalties; rows of at most 2 * threads diagonals): launch_base's contract
void launch_base2(const uint32_t* pk, int32_t* a32, uint8_t* a8, uint32_t* rle, const BaseJob* jobs, BaseResult* res, int njobs, int threads, hipStream_t st);
void launch_bp(const uint8_t* seq, int32_t* ring, const BpJob* jobs, BpResult* res, int njobs, int threads,
               DevPen pen, int scope, int ring_rows, hipStream_t st);
void launch_tile_init(const uint8_t* seq, int32_t* ring, const TileJob* jobs, int32_t* mak0, int njobs, int ring_rows, hipStream_t st);
void launch_tile(const uint8_t* seq, int32_t* ring, const TileJob* jobs, const TileTask* tasks, int32_t* mak, int ntasks,
                 int threads, int T, int Wt, size_t lds_bytes, DevPen pen, int scope, int ring_rows, hipStream_t st);
void launch_tile_advance(TileJob* jobs, int32_t* mak, int njobs, int T, DevPen pen, int exact, int coarse, int launched, hipStream_t st);
void launch_tile_reg(const uint8_t* seq, int32_t* ring, const TileJob* jobs, const TileTask* tasks, int32_t* mak, int ntasks,
                     int threads, int T, int C, bool cut, hipStream_t st);  // cut: some job of the launch carries a score bound
// phase-2 rows of the jobs in mode 4 (T = P2K scores, two diagonals per thread), their per-row maxima into p2max
void launch_tile_p2(const uint8_t* seq, int32_t* ring, const TileJob* jobs, const TileTask* tasks, int ntasks, int threads,
                    int32_t* p2, bool cut, hipStream_t st);
// The state after 2 * P2K tests as a snapshot: the last RING rows of both directions, out of the P2 rows into the job's ring
// (jobs whose walk ran out of rows go another round from there)
void launch_p2_to_ring(int32_t* ring, const int32_t* p2, const P2Job* jobs, int njobs, hipStream_t st);
// A ring moved into another geometry (a job that ran out of its narrow ring goes on from its snapshot on a wider one): every row of
// both directions and all five components ([dir][comp][ring rows][width], column = k + koff) from src to dst, diagonals klo .. khi;
// every other column of dst is WF_NULL.  src and dst are the rings' first elements; they may lie in different device blocks.
struct RingWidenJob {
  const int32_t* src;
  int32_t* dst;
  int32_t src_w, src_koff;
  int32_t dst_w, dst_koff;             // dst_w: a multiple of 4
  int32_t klo, khi;
};
void launch_ring_widen(const RingWidenJob* jobs, int njobs, int max_dst_w, int ring_rows, hipStream_t st);
void launch_p2_blockmax(const int32_t* ring, const int32_t* p2, const P2Job* jobs, int32_t* bmax, int32_t* p2max, int njobs, hipStream_t st);
void launch_p2_overlap(const int32_t* ring, const int32_t* p2, const P2Job* jobs, const int32_t* p2max, const int32_t* bmax,
                       BpResult* res, int njobs, int threads, int max_nblk, DevPen pen, int scope, hipStream_t st);
// the walk of the jobs with P2Job::exact > 0, one workgroup of `threads` per job (no maxima)
void launch_p2_exact(const int32_t* ring, const int32_t* p2, const P2Job* jobs, BpResult* res, int njobs, int threads, DevPen pen, int scope, hipStream_t st);
void launch_base(const uint8_t* seq, int32_t* a32, uint8_t* a8, uint32_t* rle, const BaseJob* jobs, BaseResult* res,
                 int njobs, DevPen pen, bool wide, int ring_rows, hipStream_t st);  // wide: 1024 threads per job instead of 256
void launch_compact(const uint32_t* rle, const int64_t* off, const int64_t* cap, uint32_t* out, unsigned long long* total,
                    int64_t* out_start, int32_t* out_count, int nprob, hipStream_t st);

}  // namespace wfm
#endif
