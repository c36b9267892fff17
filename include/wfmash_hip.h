/*
 * include/wfmash_hip.h -- C ABI of libwfmash_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the wfmash hot path.  Every entry point below replaces
 * one seam of the reference (file:line relative to waveygang/wfmash):
 *
 *   align path
 *     wfm_align_batch   <- wfa::WFAlignerGapAffine2Pieces::alignEnd2End /
 *                          alignEndsFree + getAlignment as used at
 *                          src/common/wflign/src/wflign.cpp:136-148 (main BiWFA,
 *                          MemoryUltralow), :280-309 (head patch, MemoryMed),
 *                          :368-401 (tail patch) and
 *                          src/common/wflign/src/wflign_alignment.cpp:665-678
 *                          (wflign_edit_cigar_copy).  One call aligns a whole
 *                          batch of mapping records (the batch seam above
 *                          Aligner::processAlignment,
 *                          src/align/include/computeAlignments.hpp:661).
 *   map path
 *     wfm_hash_kmers        <- CommonFunc::getHash, src/map/include/commonFunc.hpp:173-182
 *                              (MurmurHash3_x64_128 seed 42, src/common/murmur3.h:226-302)
 *     wfm_sketch_fragments  <- CommonFunc::sketchSequence, commonFunc.hpp:218-323
 *                              via MappingCore::getSeedHits, mappingCore.hpp:62-76
 *     wfm_add_minmers[_multi] <- CommonFunc::addMinmers, commonFunc.hpp:440-708
 *     wfm_prefilter_kmers   <- (no counterpart: the device-side thinning of addMinmers' input stream)
 *     wfm_finish_records    <- the closing steps of addMinmers, commonFunc.hpp:660-706 (pieces of w windows, strand signs,
 *                              std::sort by (wpos, wpos_end) with the library's tie order, std::unique)
 *     wfm_index_build       <- Sketch::build (index stage), winSketch.hpp:266-429
 *     wfm_index_build_sequences <- Sketch::build as a whole, winSketch.hpp:175-457
 *     wfm_sketch_part / wfm_index_build_parts <- the same in two steps: buildHelper per sequence (winSketch.hpp:200-239) on
 *                              the device that holds the sequence, the index stage (:266-429) once on the union
 *     wfm_index_replicate   <- (the one Sketch all mapping threads share, computeMap.hpp:431-484: one copy per GPU)
 *     wfm_index_upload / wfm_index_download <- Sketch::readIndex / writeIndex (device side), winSketch.hpp:569-866
 *     wfm_map_l1            <- getSeedIntervalPoints + computeL1CandidateRegions, mappingCore.hpp:82-301
 *     wfm_map_l2            <- computeL2MappedRegions + SlideMapper + doL2Mapping,
 *                              mappingCore.hpp:307-442, slidingMap.hpp:28-212, computeMap.hpp:989-1061
 *     wfm_map_fragments     <- Map::mapSingleQueryFrag for a whole batch, computeMap.hpp:875-938
 *     wfm_minhash_sketch    <- StreamingMinHash over one sequence (ANI estimate), map_stats.hpp:569-616
 *     wfm_sketch_intersections <- the estimate's pairwise merge of pooled sketches, map_stats.hpp:719-731, all pairs at once
 *   (file-level drivers of both phases: include/wfmash_host.h)
 *
 * All pointers are HOST memory unless stated; the library owns every device
 * buffer.  No torch types.  A handle is bound to one GPU and is not
 * thread-safe; use one handle per host thread / per rank.
 * Every function returns 0 on success or a negative WFM_E_* code; there is no
 * CPU fallback: without a visible gfx950 device wfm_create fails.
 */
#ifndef WFMASH_HIP_H_
#define WFMASH_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WFM_OK              0
#define WFM_E_NODEVICE     (-1)
#define WFM_E_HIP          (-2)   /* a HIP runtime call failed; see wfm_last_error */
#define WFM_E_ARG          (-3)
#define WFM_E_NOMEM        (-4)
#define WFM_E_UNSUPPORTED  (-5)   /* e.g. penalties whose score scope exceeds the ring */
#define WFM_E_ARENA        (-6)   /* caller's ops arena too small */
#define WFM_E_INTERNAL     (-7)   /* the library's own invariant did not hold (wfm_sites_table: a hash collision); see wfm_last_error */

/* per-problem status (wfm_result_t.status); 0 mirrors WF_STATUS_ALG_COMPLETED
 * tested at wflign.cpp:150,307,399 */
#define WFM_ST_OK            0
#define WFM_ST_UNREACHABLE (-300)
/* The wavefronts of the problem do not fit the handle's memory budget.  For a BiWFA problem the limit is the alignment's SCORE, not the
 * record's length: where a ring over all diagonals does not fit, rings grow with the score a job reaches (about 2 x score columns of
 * 1280 bytes -- 5120 for penalties of a scope beyond 30 -- have to fit the budget). */
#define WFM_ST_OOM         (-200)
/* The optimal score is beyond the problem's score limit (WFM_MODE_SCORE_LIMIT below); mirrors WF_STATUS_MAX_STEPS_REACHED. */
#define WFM_ST_MAX_SCORE   (-100)

#define WFMASH_HIP_VERSION "wfmash-hip-0.3"   /* SAM @PG VN:, `wfmash-hip --version` */

typedef struct wfm_handle wfm_handle_t;

/* wflign_penalties_t (wflign_alignment.hpp:21) minus match (always 0) */
typedef struct { int32_t x, o1, e1, o2, e2; } wfm_penalties_t;

/* alignment mode = the WFAligner memory model / entry point the reference uses */
#define WFM_MODE_END2END_BIWFA 0   /* alignEnd2End, MemoryUltralow  (wflign.cpp:136-148) */
#define WFM_MODE_ENDSFREE      1   /* alignEndsFree, MemoryMed      (wflign.cpp:280-305,368-397) */
#define WFM_MODE_END2END_UNI   2   /* alignEnd2End, full backtrace (MemoryHigh)            */
/* Flags, OR-ed into `mode` with one of the three modes above (wfm_problem_t and wfm_problem_ref_t alike).
 *
 * WFM_MODE_SCORE_ONLY (WFAligner's AlignmentScope Score), with any of the three modes: the result carries status, score and
 * cells, ops_len = n_runs = 0, and nothing of the problem is written to the ops arena or to the runs.  score is the optimal
 * gap-affine-2p score -- end-to-end for modes 0 and 2, ends-free for mode 1 -- exactly what the full alignment of the same
 * problem reports; the device stops where it knows it: a BiWFA root at the score its directions meet at (no children, no
 * leaves), a base job behind its forward pass (no walk back).  wfm_align_arena_bytes counts 0 for such problems,
 * wfm_align_batch accepts ops_arena == NULL with arena_bytes == 0 when every problem is score-only, and score-only and full
 * problems may be mixed in one call through every entry point.  wfm_get_problem_flags reports the paths taken, as ever.
 *
 * WFM_MODE_SCORE_LIMIT (WFAligner::setMaxAlignmentSteps), END2END_BIWFA only: score_hint (> 0) is a hard limit instead of a
 * guess.  status is WFM_ST_OK with the exact result (the score, and the op string unless SCORE_ONLY) if and only if the optimal
 * score is <= score_hint; otherwise status is WFM_ST_MAX_SCORE, score is -1 and there are no ops -- a failed problem in the
 * call's return value like any other.  There is never a second run without the limit, no wavefront is computed beyond it
 * (tile blocks stop at the first block that begins at or past it, the step kernel at the first score past it, a short
 * problem's base job runs with the limit as its score budget), and it holds whatever the WFM_* environment switches say
 * about hints and bounds.  With another mode, or with score_hint <= 0, the upload fails with WFM_E_ARG.
 *
 * Every upload (wfm_upload_sequences, wfm_upload_sequence_refs and the calls built on them) checks `mode`: a mode other than
 * 0, 1, 2 under WFM_MODE_MASK or a bit outside the mask and the two flags is WFM_E_ARG with a message; the handle stays usable. */
#define WFM_MODE_MASK        0xff
#define WFM_MODE_SCORE_ONLY  0x100
#define WFM_MODE_SCORE_LIMIT 0x200

typedef struct {
  const char* pattern;  int32_t plen;     /* wfmash passes pattern = target */
  const char* text;     int32_t tlen;     /* wfmash passes text    = query  */
  int32_t mode;                           /* WFM_MODE_*, optionally | WFM_MODE_SCORE_ONLY | WFM_MODE_SCORE_LIMIT */
  int32_t pattern_begin_free, pattern_end_free;   /* ENDSFREE only */
  int32_t text_begin_free, text_end_free;
  int32_t score_hint;                     /* END2END_BIWFA only; 0 = none.  A guess of an upper bound of the alignment's
                                           * score (e.g. the cost of the end gaps the caller's padding implies plus a
                                           * divergence allowance).  The wavefronts are then only computed where an
                                           * alignment of at most that score can pass; a guess that turns out too small
                                           * costs a second run without it, never a different result.  With
                                           * WFM_MODE_SCORE_LIMIT: the hard limit of the score (see above). */
  int32_t pad_;
} wfm_problem_t;

typedef struct {
  int32_t  status;     /* WFM_ST_*                                             */
  int32_t  score;      /* gap-affine-2p penalty of the returned alignment; ENDSFREE: the ends-free score (the free
                        * parts of the op string's first and last gap cost nothing), what alignEndsFree reports      */
  uint64_t ops_off;    /* offset of this problem's op string in ops_arena (wfm_align_batch_rle: index of its first run) */
  uint32_t ops_len;    /* number of ops over {M,X,I,D}; I = text-only, D = pattern-only */
  uint32_t n_runs;     /* number of run-length encoded CIGAR runs             */
  uint64_t cells;      /* (score,diagonal) cells computed on the device        */
} wfm_result_t;

typedef struct {
  uint64_t cells;            /* cells computed in the last batch                  */
  uint64_t bytes_algorithmic;/* 48*cells + sum(plen+tlen)         */
  double   ms_kernels;       /* device time of all WFA kernels (hipEvent)         */
  double   ms_breakpoint;    /* device time of the BiWFA breakpoint kernels       */
  double   ms_base;          /* device time of the base / backtrace kernels       */
  double   ms_total;         /* host wall time of the whole call                  */
  uint32_t levels;           /* BiWFA recursion levels executed                   */
  uint32_t bp_jobs, base_jobs;
  uint32_t bp_launches, base_launches;
  uint64_t cells_bp;         /* cells computed by wfa_bp_kernel launches          */
  uint64_t cells_base;       /* cells computed by wfa_base_kernel launches        */
  uint64_t cells_tile;       /* part of cells_bp computed by wfa_tile_kernel      */
  double   ms_tile;          /* part of ms_breakpoint spent in wfa_tile_kernel    */
  uint32_t tile_launches, tile_tasks;
  double   ms_tile_busy;     /* time during which at least one tile kernel launch was running: equals ms_tile unless
                              * the two halves of a batch ran their tile kernels side by side on two streams */
  uint32_t streams;          /* parts of the batch that ran side by side, each on its own stream */
  uint32_t pad_;
  uint64_t cells_tile_unique;/* cells_tile without the block a job computes twice: the full block in which its wavefronts
                              * meet is thrown away and run again up to the meeting point only */
  double   ms_bp_busy;       /* as ms_tile_busy, for the wfa_bp_kernel launches (ms_breakpoint - ms_tile summed over streams) */
  double   ms_base_busy;     /* as ms_tile_busy, for the wfa_base_kernel launches */
  double   ms_any_busy;      /* time during which any of the three kernels was running */
  uint32_t p2_launches, p2_jobs; /* phase 2 from rows computed ahead (tile kernel + wfa_p2_* kernels): launch sets, jobs */
  uint32_t p2_more, p2_again; /* of those jobs, the ones wfa_bp_kernel had to finish step by step; further rounds of rows computed ahead (jobs x rounds) */
} wfm_stats_t;

int  wfm_device_count(void);   /* usable HIP devices of this node (0 without a GPU) */
int  wfm_create(int device, wfm_handle_t** out);
void wfm_destroy(wfm_handle_t* h);
const char* wfm_last_error(const wfm_handle_t* h);
int  wfm_device_name(const wfm_handle_t* h, char* buf, size_t buflen);

/* Upper bound of the ops_arena bytes wfm_align_batch needs for these problems
 * (sum of plen+tlen+1 over the problems that are not WFM_MODE_SCORE_ONLY). */
size_t wfm_align_arena_bytes(const wfm_problem_t* problems, size_t n);

/* Align n problems.  out[i].ops_off/ops_len locate the op string of problem i
 * inside ops_arena (not NUL-terminated).  Returns the number of problems whose
 * status != 0, or a negative WFM_E_* code if the call itself failed. */
int  wfm_align_batch(wfm_handle_t* h, const wfm_penalties_t* pen,
                     const wfm_problem_t* problems, size_t n,
                     wfm_result_t* out, char* ops_arena, size_t arena_bytes);

/* The same with run-length output, the form the align driver consumes: the reference's own pipeline compresses the op
 * string at once (compress_cigar, wflign.cpp:183-208) and works on runs from there on (erosion scan, merge, swizzle and
 * write_alignment_paf: wflign.cpp:174-231,241-454), so nothing on that path needs one byte per base; wfm_align_batch's
 * expanded form stays for getAlignment(char**, int*) (wflign_alignment.cpp:671-677).
 * *runs receives a buffer of 32-bit runs owned by the caller (release with wfm_free_runs), run = (length << 2) | op
 * with op 0 = M, 1 = X, 2 = I (text only), 3 = D (pattern only); adjacent runs of one problem never share an op.
 * out[i].ops_off = index of problem i's first run in *runs, out[i].n_runs their number, out[i].ops_len the number of
 * ops they spell.  Returns as wfm_align_batch. */
#define WFM_RUN_LEN(r) ((uint32_t)(r) >> 2)
#define WFM_RUN_OP(r)  ((uint32_t)(r) & 3u)
int  wfm_align_batch_rle(wfm_handle_t* h, const wfm_penalties_t* pen,
                         const wfm_problem_t* problems, size_t n,
                         wfm_result_t* out, uint32_t** runs, size_t* n_runs_total);
void wfm_free_runs(uint32_t* runs);

/* Upper bounds of the END2END scores of n problems without aligning them: the cost of one valid global alignment per
 * problem, found by a greedy walk on the device (one wave per problem: extend along the diagonal, at a difference try a
 * substitution and the indels up to 31 bases side by side; wfmash_amd/csrc/wfa_kernels.hip, wfa_bound_kernel).  out[i] >= the
 * optimal gap-affine-2p score of problem i, or -1 where the walk gave up (divergent sequences, structural differences,
 * sequences under 256 bases).  wfm_align_batch runs this itself for its long BiWFA problems and cuts their wavefronts to
 * what an alignment of at most that score can touch; the entry point exists for callers that want the bound and for tests. */
int  wfm_score_bounds(wfm_handle_t* h, const wfm_penalties_t* pen, const wfm_problem_t* problems, size_t n, int32_t* out);

/* Self-test of the cross-lane primitives the packed tile kernel leans on (DPP wave shifts, wfmash_amd/csrc/wfa_tile2.hip):
 * out128[lane] = the value 1000 + (lane - 1) taken from the previous lane (lane 0: the kernel's NULL, -2^30),
 * out128[64 + lane] = 1000 + (lane + 1) from the next lane (lane 63: NULL). */
int  wfm_selftest_dpp(wfm_handle_t* h, int32_t* out128);
/* Self-test of the device arenas' growth policy: capacities (in 4-byte elements) after a first request of n0 elements, after a request of one element
 * more than that capacity (must at least double it), and after a request that fits (must not allocate). */
int  wfm_selftest_arena_growth(wfm_handle_t* h, size_t n0, size_t* out3);

/* Same, but sequences are already resident in device memory (the timed region
 * of bench.py starts here): d_seqs is a device pointer, offsets index into it.
 * Sequences must be laid out by wfm_upload_sequences. */
typedef struct wfm_seqset wfm_seqset_t;
int  wfm_upload_sequences(wfm_handle_t* h, const wfm_problem_t* problems, size_t n, wfm_seqset_t** out);
void wfm_free_sequences(wfm_handle_t* h, wfm_seqset_t* s);
int  wfm_align_resident(wfm_handle_t* h, const wfm_penalties_t* pen, wfm_seqset_t* s,
                        wfm_result_t* out, char* ops_arena, size_t arena_bytes);
int  wfm_align_resident_rle(wfm_handle_t* h, const wfm_penalties_t* pen, wfm_seqset_t* s,
                            wfm_result_t* out, uint32_t** runs, size_t* n_runs_total);

/* ---- sequences resident on the device, problems by reference ----
 * A store holds whole sequences on one device, normalised as makeUpperCaseAndValidDNA leaves them (commonFunc.hpp:132-142: upper
 * case, anything but A C G T becomes N), one byte per base -- the form the align driver gives every window it fetches.  A problem
 * is then named as "bases [off, off + len) of sequence i, this strand" and the device cuts, reverse-complements and lays out the
 * windows itself; only sides given as host pointers cross PCIe.
 *
 * wfm_seqstore_create binds the store to h's DEVICE; every handle of that device may add to it and read from it, also at the same
 * time (an internal mutex guards the table).  wfm_seqstore_add uploads the raw bytes in chunks through pinned memory, normalises
 * them on the device and has finished there before it returns the sequence's id (>= 0) or a WFM_E_* code; a sequence lives in a
 * block of its own from the device heap, with 16 bytes and more of slack on either side, and never moves.  A store of another
 * device than h's: WFM_E_ARG; out of device memory: WFM_E_NOMEM, and the store stays usable.  wfm_seqstore_free releases the
 * blocks (no call that reads the store may be in flight). */
typedef struct wfm_seqstore wfm_seqstore_t;
int     wfm_seqstore_create(wfm_handle_t* h, wfm_seqstore_t** out);
void    wfm_seqstore_free(wfm_seqstore_t* s);
int32_t wfm_seqstore_add(wfm_handle_t* h, wfm_seqstore_t* s, const char* seq, int64_t len);
int     wfm_seqstore_info(const wfm_seqstore_t* s, int64_t* n_seqs, int64_t* bytes);  /* sequences held, bytes of their device blocks */

typedef struct {
  const char* pattern; const char* text;   /* host bytes for a side whose *_seq is -1, taken as they are (as wfm_problem_t) */
  int64_t pattern_off, text_off;           /* window start on the stored (forward) strand */
  int32_t pattern_seq, text_seq;           /* store id, or -1 = host pointer */
  int32_t plen, tlen;
  int32_t mode;
  int32_t pattern_revcomp, text_revcomp;   /* 1: the side is the reverse complement of the window (N stays N) */
  int32_t pattern_begin_free, pattern_end_free, text_begin_free, text_end_free;
  int32_t score_hint;
} wfm_problem_ref_t;                       /* 80 bytes */

/* Destination bytes one task of the gather kernel covers (seq_gather_kernel, wfmash_amd/csrc/wfa_kernels.hip): a window longer
 * than this is cut into several tasks, each a workgroup of its own. */
#define WFM_SEQ_GATHER_CHUNK 16384

/* wfm_upload_sequences for problems by reference: the seqset has exactly the layout wfm_upload_sequences gives the same problems
 * (forward copies, the reversed copies of the BiWFA problems, pads, 2-bit mirror, ACGT flags), so wfm_align_resident[_rle] and
 * everything behind them take it as they take any other.  store may be NULL when every side is a host pointer.  WFM_E_ARG (with a
 * message, the handle stays usable): an unknown id, a window that leaves its sequence, plen + tlen > 2^29, a null host pointer
 * for a -1 side of non-zero length, a store of another device. */
int wfm_upload_sequence_refs(wfm_handle_t* h, const wfm_seqstore_t* store, const wfm_problem_ref_t* refs, size_t n, wfm_seqset_t** out);
/* wfm_upload_sequence_refs + wfm_align_resident_rle + wfm_free_sequences */
int wfm_align_refs_rle(wfm_handle_t* h, const wfm_penalties_t* pen, const wfm_seqstore_t* store, const wfm_problem_ref_t* refs, size_t n,
                       wfm_result_t* out, uint32_t** runs, size_t* n_runs_total);
/* Diagnostic: the seqset's byte buffer (pads, forward and reversed copies) back on the host.  Writes min(cap, its size) bytes to
 * out (may be NULL); returns the buffer's size or a WFM_E_* code. */
int64_t wfm_download_sequences(wfm_handle_t* h, const wfm_seqset_t* s, uint8_t* out, int64_t cap);

/* ---- every run of a CIGAR held against the bases it covers ----
 * A self-check that is independent of the aligners: it reads the forward BYTE copies of the seqset (never the 2-bit mirror the
 * kernels extend on) and shares no code with the cell step or the walk back (wfmash_amd/csrc/wfa_check.hip).  s is any seqset,
 * res[i].ops_off / res[i].n_runs locate problem i's runs in `runs` in the format of wfm_align_batch_rle, out receives one
 * wfm_check_t per problem of s.  Bases are compared as bytes, as oracle/wfa2p.c compares them: N equals N, 'a' differs from 'A',
 * nothing is normalised.  The price: X costs x per base, a gap run of L bases min(o1 + e1 L, o2 + e2 L); in a WFM_MODE_ENDSFREE
 * problem the first run loses up to pattern_begin_free (D) or text_begin_free (I) bases before it is priced and the last run up
 * to pattern_end_free / text_end_free (a single run may use both allowances of its side) -- the score alignEndsFree reports.
 * bad_p / bad_t / bad_run name the offending base with the smallest pattern index, whatever order the device finds them in;
 * without one, bad_p = bad_t = -1 and bad_run is the first bad run (0: none).  No byte outside the problem's two sequences is
 * read: bases are compared only where the runs' totals do not exceed plen and tlen (WFM_CK_SPANS alone otherwise).
 * Returns the number of problems whose flags hold anything but WFM_CK_NOT_CHECKED, or a WFM_E_* code; a run range that leaves
 * runs[0 .. n_runs_total) is WFM_E_ARG.  Optimality is not checked here: wfm_check_optimal, below, proves it. */
#define WFM_CK_NOT_CHECKED  1u  /* no runs to check: a score-only problem, or status != 0 */
#define WFM_CK_BAD_RUN      2u  /* a run of length 0, or two adjacent runs with one op */
#define WFM_CK_SPANS        4u  /* the runs do not span exactly plen pattern and tlen text bases */
#define WFM_CK_M_DIFFERS    8u  /* an M run covers two different bytes */
#define WFM_CK_X_EQUAL     16u  /* an X run covers two equal bytes */
#define WFM_CK_SCORE       32u  /* the price of the runs is not res[i].score (compared only when res[i].score >= 0) */
#define WFM_CK_COUNTS      64u  /* ops_len of the result differs from what its n_runs runs spell (a wrong n_runs shows here too) */
typedef struct {
  uint32_t flags; int32_t score;        /* price of the runs under pen (ENDSFREE: ends-free price, above) */
  int32_t  bad_p, bad_t;                /* pattern / text index of the FIRST offending base (-1: none) */
  uint32_t bad_run, n_runs;             /* index of the run that holds it (or of the first bad run); runs read */
  uint32_t matches, mismatches, ins_runs, ins_bases, del_runs, del_bases;
} wfm_check_t;                          /* 48 bytes */
#define WFM_CHECK_SLICE 16384           /* ops one compare task covers, as WFM_SEQ_GATHER_CHUNK */
int wfm_check_runs(wfm_handle_t* h, const wfm_penalties_t* pen, const wfm_seqset_t* s,
                   const wfm_result_t* res, const uint32_t* runs, size_t n_runs_total, wfm_check_t* out);

/* ---- every interior gap moved to its leftmost placement ----
 * An indel inside a homopolymer or a tandem repeat has many placements of one score; the aligners leave it at the rightmost (they extend
 * matches before they open a gap).  This call moves every interior gap as far to the left as a rotation of its own bases allows -- the
 * convention of minimap2 and of VCF normalisation -- on the device (wfmash_amd/csrc/wfa_leftalign.hip; forward BYTE copies only, bytes compared
 * as bytes like wfm_check_runs: N equals N).  s, res and runs as for wfm_check_runs; the runs must be valid (M over equal bytes, X over
 * different ones, spanning plen x tlen).
 *
 * The rule.  The runs are taken from left to right and the output is built on the way.  An interior gap is an I or D run of L bases that is
 * neither the problem's first nor its last run (those are never touched); g = its first index in S, S = pattern for D, text for I.
 *   rot  = the number of k >= 1, counted consecutively from 1, with S[g - k] == S[g + L - k];
 *   room = 0 if the run now before the gap in the output is no M run, else that run's current length e (with what the gap before may have
 *          added to it) -- but e - 1 if that M run is the output's first run or the run before it is a gap of the same op: a gap never
 *          becomes the first run, and two gaps of one op never merge;
 *   d    = min(rot, room): the M run before the gap loses d bases (and goes at 0), the gap keeps its length, the d bases join the M run
 *          behind it or become a new M run where what follows is no M run.
 * So a problem's run count may shrink, or grow by at most one per gap.  The result is a valid CIGAR of the same bases with the same price
 * under any penalties and the same wfm_check_t counts; the first and last runs keep their ops; applying the call twice changes nothing.
 * Not normalised: end gaps, a gap behind an X run, gaps that would merge, co-optimal placements that differ by more than a rotation.
 *
 * *runs_out receives the new runs of all problems end to end (release with wfm_free_runs), adjacent runs never sharing an op,
 * *n_runs_out_total their number; res[i].ops_off and res[i].n_runs are rewritten to locate problem i in *runs_out, and score, ops_len and
 * cells are never touched.  out receives one wfm_leftalign_t per problem: gaps = its interior gaps, moved = those with d > 0, bases_moved
 * = the sum of d, longest = the largest d, runs_out = its runs now.  A problem flagged WFM_LA_NOT_DONE or WFM_LA_SPANS keeps its runs
 * verbatim.  Returns the number of problems flagged WFM_LA_SPANS, or a WFM_E_* code; a run range that leaves runs[0 .. n_runs_total) is
 * WFM_E_ARG (the handle stays usable).  (WFM_LA_LANE_MAX, read per call: the bases after which a gap's comparison leaves its single lane for
 * a whole wave, 256; a measuring switch.) */
typedef struct { uint32_t flags, gaps, moved, runs_out; uint64_t bases_moved; uint32_t longest, pad_; } wfm_leftalign_t;  /* 32 bytes */
#define WFM_LA_NOT_DONE 1u   /* status != 0, score-only, no runs */
#define WFM_LA_SPANS    2u   /* the runs do not span plen x tlen, or hold a bad run: left exactly as they came */
int wfm_left_align_runs(wfm_handle_t* h, const wfm_seqset_t* s, wfm_result_t* res /* n_runs, ops_off rewritten */,
                        const uint32_t* runs, size_t n_runs_total, uint32_t** runs_out, size_t* n_runs_out_total,
                        wfm_leftalign_t* out);   /* runs_out: wfm_free_runs */

/* ---- minimap2's cs difference string of every problem's runs ----
 * A CIGAR with = and X says where the bases differ; the cs string says which they are, so that substitutions, inserted and deleted bases
 * can be read off a line without either FASTA.  This call spells it on the device (wfmash_amd/csrc/wfa_cs.hip; forward BYTE copies only,
 * never the 2-bit mirror; nothing is shared with the aligners).  s, res and runs as for wfm_check_runs: res[i].ops_off may come in any order,
 * with unused words between the problems.
 *
 * The grammar.  Pattern = target = reference side P; text = query side T as aligned (already reverse-complemented for a '-' record).  The
 * problem's runs are spelled from left to right, p and t being the indices the run begins at:
 *   run                        WFM_CS_SHORT                              WFM_CS_LONG
 *   M of L bases               ':' + L in decimal                        '=' + the L pattern bytes as they are
 *   X of L bases               L times '*' + lc(P[p+j]) + lc(T[t+j])     the same
 *   I of L bases (text only)   '+' + lc of the L text bytes              the same
 *   D of L bases (pattern)     '-' + lc of the L pattern bytes           the same
 * lc maps 'A'..'Z' to 'a'..'z' and leaves every other byte alone (N becomes n).  The string is spelled from the runs and never from a
 * comparison: an X over two equal bytes is spelled "*aa", and an M over different bytes takes its bytes from the pattern in the long form.
 * Whether the runs fit the bases is wfm_check_runs' business.
 *
 * *out receives the strings of all problems end to end in problem order, not NUL-terminated, *out_bytes their total; the buffer is host
 * memory owned by the caller (release with wfm_free_cs).  per receives one wfm_cs_t per problem: off / len locate its string in *out, n_runs
 * is the number of runs it was spelled from.  A problem flagged WFM_CS_NOT_DONE or WFM_CS_SPANS has len 0 and nothing of it is spelled.
 * Returns the number of problems flagged WFM_CS_SPANS, or a WFM_E_* code; a run range that leaves runs[0 .. n_runs_total) and a form other
 * than the two are WFM_E_ARG with a message (*out is NULL, the handle stays usable).  No problems: WFM_OK, *out = NULL, *out_bytes = 0.
 * One workgroup writes WFM_CS_SLICE bytes of the output whatever runs or problems they belong to, and the problems are worked in chunks
 * whose device output block holds at most WFM_CS_OUT_MB MiB (environment, read per call, 256; a single problem may exceed it alone), each
 * copied to its place in *out: device memory stays bounded whatever a long-form batch spells. */
#define WFM_CS_SHORT 0
#define WFM_CS_LONG  1
#define WFM_CS_NOT_DONE 1u   /* status != 0, score-only, no runs: len = 0 */
#define WFM_CS_SPANS    2u   /* a run of length 0, two neighbours with one op, totals other than plen x tlen: len = 0, nothing spelled */
typedef struct { uint32_t flags, n_runs; uint64_t off, len; } wfm_cs_t;   /* 24 bytes; off/len locate the string in *out */
#define WFM_CS_SLICE 16384   /* output bytes one workgroup writes */
int  wfm_cs_strings(wfm_handle_t* h, const wfm_seqset_t* s, const wfm_result_t* res, const uint32_t* runs, size_t n_runs_total,
                    int form, char** out, size_t* out_bytes, wfm_cs_t* per);
void wfm_free_cs(char* p);

/* ---- the variants of every problem's runs ----
 * The list of differences itself: every substitution, insertion and deletion of a problem's runs as a record in VCF form, REF and ALT
 * alleles included, called on the device (wfmash_amd/csrc/wfa_variants.hip; forward BYTE copies only; nothing is shared with the aligners).
 * s, res and runs as for wfm_cs_strings: res[i].ops_off may come in any order, with unused words between the problems.
 *
 * The grammar.  Pattern = target = REF side P; text = query side T as aligned.  p and t are the indices a run begins at:
 *   run                        records                fields                                                         allele bytes
 *   M of L                     none                                                                                  0
 *   X of L                     L SNVs, j = 0..L-1     p = p+j, t = t+j, REF = P[p+j], ALT = T[t+j]; kind carries      2 each
 *                                                     WFM_VAR_MASKED when either byte is outside ACGTacgt
 *   I of L, called             1 INS                  p = p-1 (the anchor), t = t, REF = P[p-1], ALT = P[p-1] + T[t..t+L)   L + 2
 *   D of L, called             1 DEL                  p = p-1, t = t, REF = P[p-1..p+L), ALT = P[p-1]                  L + 2
 *   I or D, not called         none: counted in end_gaps                                                             0
 * A gap is called unless it is the problem's first or last run -- an alignment end, not a variant -- or no pattern base lies before it
 * (p = 0: it has no anchor, which happens only behind a first run that is an I).  Bytes are emitted as they are, with no case change.  Two
 * adjacent gaps (2I3D) and a gap behind an X run each keep the rule; they share an anchor, which is valid VCF.  The records are called
 * from the runs and never from a comparison, so their number and the allele bytes follow from the runs alone: a masked SNV is a flagged
 * record, not a missing one.  The defining property: applying a problem's records to P from the last to the first (SNV: P[p] = ALT; INS:
 * insert ALT[1:] behind P[p]; DEL: remove P[p+1 .. p+ref_len)) gives T for every valid CIGAR without end gaps.
 *
 * *vars receives the records of all problems -- problems in problem order, runs in run order, an X run's bases in base order -- and
 * *n_vars their number; *alleles the allele bytes in the same order, *allele_bytes their total: a record's REF is alleles[off .. off +
 * ref_len), its ALT the alt_len bytes behind.  Both are host memory owned by the caller (release with wfm_free_variants).  per receives
 * one wfm_varcall_t per problem: first / count locate its records in *vars, n_runs is the number of runs they were called from.  A
 * problem flagged WFM_VAR_NOT_DONE or WFM_VAR_SPANS has count 0 and nothing of it is called.  Returns the number of problems flagged
 * WFM_VAR_SPANS, or a WFM_E_* code; a run range that leaves runs[0 .. n_runs_total) is WFM_E_ARG with a message (the outputs are NULL,
 * the handle stays usable).  No problems: WFM_OK, NULL outputs and zero counts.
 * One workgroup writes WFM_VAR_SLICE allele bytes whatever runs or problems they belong to, and the problems are worked in chunks whose
 * device blocks, alleles and records together, hold at most WFM_VAR_OUT_MB MiB (environment, read per call, 256; a single problem may
 * exceed it alone).  No atomics: two calls give the same bytes. */
typedef struct { uint32_t problem, kind; uint32_t p, t; uint32_t ref_len, alt_len; uint64_t off; } wfm_variant_t;   /* 32 bytes */
typedef struct { uint32_t flags, n_runs; uint64_t first, count; uint32_t end_gaps, pad_; } wfm_varcall_t;        /* 32 bytes */
#define WFM_VAR_SNV 0u
#define WFM_VAR_INS 1u
#define WFM_VAR_DEL 2u
#define WFM_VAR_MASKED 256u      /* bit of kind: an SNV whose REF or ALT byte is not one of ACGTacgt */
#define WFM_VAR_NOT_DONE 1u      /* as WFM_CS_NOT_DONE */
#define WFM_VAR_SPANS    2u      /* as WFM_CS_SPANS: nothing of the problem is called */
#define WFM_VAR_SLICE 16384      /* allele bytes one workgroup writes */
int  wfm_call_variants(wfm_handle_t* h, const wfm_seqset_t* s, const wfm_result_t* res, const uint32_t* runs, size_t n_runs_total,
                       wfm_variant_t** vars, size_t* n_vars, char** alleles, size_t* allele_bytes, wfm_varcall_t* per);
void wfm_free_variants(wfm_variant_t* vars, char* alleles);

/* ---- per-base depth of the target from the runs of many records ----
 * What the calls above leave out: they take every problem alone.  A coverage object sums over all the problems added to it, call after
 * call: a zeroed DIFFERENCE array of int32 words, n_bases + 1 of them, over the concatenation of the target sequences, on the handle's
 * device (wfmash_amd/csrc/wfa_coverage.hip).  No sequence bytes are read: nothing goes up but runs.  depth(x) = the number of added
 * problems with an = or X base at x: D bases do not count, I runs advance nothing.
 *
 * wfm_coverage_create: 4 bytes per target base; refused with WFM_E_ARG and a message naming the GiB needed where that is more than
 * WFM_COV_GB GiB (environment, a decimal, read per call, 32).  The object is used with the handle it was made on and freed before it.
 * wfm_coverage_add: probs[i] = {base: the global index of the first pattern base, runs_off / n_runs: its runs in runs[0 .. n_runs_total)}.
 * An aligned segment -- =/X runs with no I or D between -- adds +1 at its first word and -1 behind its last: two integer atomics per
 * segment; abutting segments of two records cancel at the word they share.  A problem whose pattern span leaves [0, n_bases], or with
 * an empty run, adds NOTHING and is flagged WFM_COV_SPANS in flags_out[i] (the span is taken before any word is written).  Returns the
 * number of problems flagged, or WFM_E_*: a run range that leaves the run buffer is WFM_E_ARG with a message, nothing is added and the
 * handle stays usable.  No problems: WFM_OK.
 * wfm_coverage_export: the non-zero words as {pos, delta} in ascending pos, by a device compaction (count per tile of WFM_COV_TILE words,
 * prefix of the counts, write) brought down in chunks of at most WFM_COV_OUT_MB MiB (environment, a decimal, 256; one tile at least).
 * Host memory owned by the caller (wfm_coverage_free_list); NULL and 0 where every word is zero.
 * wfm_coverage_import: such a list added into this object (the merge of the objects of several devices); a pos beyond n_bases is
 * WFM_E_ARG and nothing is added.
 * wfm_coverage_intervals: the maximal intervals of constant depth: depth changes exactly at the non-zero words, so interval k starts at
 * the k-th of them with depth = the inclusive prefix sum of delta, taken on the device over the compact list (scans in the reduce /
 * scan-of-sums / apply form over blocks of WFM_COV_SCAN_BLOCK entries; dense depths are never made).  An interval ends where the next
 * starts, the last at n_bases; the first starts at 0 (depth 0 where word 0 is zero); an object with every word zero gives {0, 0} alone.
 * totals = {bases with depth >= 1, sum of depth over all bases, largest depth}, reduced on the device.  Release with
 * wfm_coverage_free_list.
 * Integer atomics only: any order of adds gives the same array, and two calls give the same bytes. */
typedef struct wfm_coverage wfm_coverage_t;
typedef struct { uint64_t base, runs_off; uint32_t n_runs, pad_; } wfm_cov_prob_t;      /* 24 bytes */
typedef struct { uint64_t pos; int32_t delta; uint32_t pad_; } wfm_cov_entry_t;         /* 16 bytes */
typedef struct { uint64_t start; uint32_t depth, pad_; } wfm_cov_interval_t;            /* 16 bytes */
#define WFM_COV_SPANS 2u          /* as WFM_VAR_SPANS: nothing of the problem is added */
#define WFM_COV_TILE 4096         /* words of the difference array one workgroup counts and writes */
#define WFM_COV_SCAN_BLOCK 1024   /* elements one workgroup takes in the two scans */
int  wfm_coverage_create(wfm_handle_t* h, uint64_t n_bases, wfm_coverage_t** cov);
void wfm_coverage_free(wfm_coverage_t* cov);
int  wfm_coverage_add(wfm_handle_t* h, wfm_coverage_t* cov, const wfm_cov_prob_t* probs, size_t n, const uint32_t* runs, size_t n_runs_total,
                      uint32_t* flags_out);
int  wfm_coverage_export(wfm_handle_t* h, wfm_coverage_t* cov, wfm_cov_entry_t** entries, size_t* n);
int  wfm_coverage_import(wfm_handle_t* h, wfm_coverage_t* cov, const wfm_cov_entry_t* entries, size_t n);
int  wfm_coverage_intervals(wfm_handle_t* h, wfm_coverage_t* cov, wfm_cov_interval_t** iv, size_t* n, uint64_t totals[3]);
void wfm_coverage_free_list(void* p);

/* ---- target intervals lifted through the runs of many records ----
 * "Where does this piece of the target lie in the query?"  A liftset is a sorted list of intervals over the concatenation of the target
 * sequences (the coordinate space of wfm_coverage_*), uploaded once per handle; wfm_lift_runs lifts them through every problem's runs on
 * the device (wfmash_amd/csrc/wfa_lift.hip).  The pattern is the target, the text the query as aligned; nothing goes up but runs.
 *
 * wfm_liftset_create: iv[0 .. n) half-open, sorted by (start, end), start < end <= n_bases; anything else is WFM_E_ARG with a message and
 * nothing is kept.  The device also makes pm[i] = max(end[0 .. i]) (a reduce / scan-of-sums / apply prefix over blocks of
 * WFM_LIFT_SCAN_BLOCK intervals with max in place of sum): the intervals that can overlap a span [a, b) are the indices in [lo, hi), lo = the
 * first i with pm[i] > a, hi = the first i with start[i] >= b -- two binary searches, however the intervals nest -- and inside that window
 * an interval overlaps iff end[i] > a.  n == 0 is legal: every later call returns no lifts.  The set is used with the handle it was made
 * on and freed before it.
 * wfm_lift_runs: probs as wfm_coverage_add takes them.  One wfm_lift_t for every (problem, interval) pair whose interval overlaps the
 * problem's pattern span [base, base + plen), problems in problem order, a problem's intervals in ascending index; per[i] = {flags, n_runs,
 * first, count} locates problem i's lifts.  A problem with an empty run, without runs, whose pattern span leaves [0, n_bases] or whose
 * pattern or text span does not fit 32 bits is flagged WFM_LIFT_SPANS and has count 0 (the spans are taken before anything is written).
 * Every field of a lift is an offset inside the problem, p* into the pattern, t* into the text.  With the interval clipped to the span,
 * c0 = max(start, base) - base, c1 = min(end, base + plen) - base, and a pattern base called ALIGNED where an = or X run covers it: p0 =
 * the first aligned pattern base >= c0, p1 = one past the last aligned pattern base < c1, t0 = the text base opposite p0, t1 = one past
 * the text base opposite p1 - 1.  So an endpoint in a D run snaps inward, an I run strictly between two lifted bases lies inside
 * [t0, t1), an I run directly before p0 or behind p1 - 1 outside it.  eq / x = the = / X columns in [p0, p1); inserted bases are
 * (t1 - t0) - (eq + x), deleted bases (p1 - p0) - (eq + x).  Where [c0, c1) holds no aligned base the pair is still there, with p0 = p1 =
 * c0, t0 = t1 = the text index reached at c0 and eq = x = 0: present in the target, absent from the query.
 * Per problem the runs are indexed once (four exclusive prefixes per run as one 16-byte word); every endpoint is resolved by binary
 * searches over them, O(log n_runs), never by a walk.  Lifts are placed by block scans, not atomics: two calls give the same bytes.  The
 * output comes down in chunks of whole problems holding at most WFM_LIFT_OUT_MB MiB of lifts (environment, a decimal, read per call,
 * 256; one problem at least).  Host memory owned by the caller (wfm_free_lifts); NULL and 0 without problems or pairs.  A run range that
 * leaves the run buffer is WFM_E_ARG with a message, the outputs are NULL and the handle stays usable.  Returns WFM_OK or WFM_E_*. */
typedef struct wfm_liftset wfm_liftset_t;
typedef struct { uint64_t start, end; } wfm_lift_iv_t;                              /* 16 bytes; global target coordinates, half-open */
typedef struct { uint32_t problem, interval, p0, p1, t0, t1, eq, x; } wfm_lift_t;   /* 32 bytes */
typedef struct { uint32_t flags, n_runs; uint64_t first, count; } wfm_liftcall_t;   /* 24 bytes */
#define WFM_LIFT_SPANS 2u          /* as WFM_COV_SPANS: nothing of the problem is lifted */
#define WFM_LIFT_SCAN_BLOCK 1024   /* intervals one workgroup takes in the running maximum */
int  wfm_liftset_create(wfm_handle_t* h, const wfm_lift_iv_t* iv, size_t n, uint64_t n_bases, wfm_liftset_t** out);
void wfm_liftset_free(wfm_liftset_t* s);
int  wfm_lift_runs(wfm_handle_t* h, const wfm_liftset_t* s, const wfm_cov_prob_t* probs, size_t n, const uint32_t* runs, size_t n_runs_total,
                   wfm_lift_t** lifts, size_t* n_lifts, wfm_liftcall_t* per);
void wfm_free_lifts(wfm_lift_t* p);

/* ---- the blocks and gaps of a UCSC chain from the runs of many records ----
 * A chain is a compaction of the runs: ungapped blocks and the pair of gap lengths between two of them.  wfm_chain_runs makes them on the
 * device (wfmash_amd/csrc/wfa_chain.hip).  The pattern is the target, the text the query as aligned; nothing goes up but runs.
 *
 * probs[i] = {runs_off, n_runs, flags}, runs as wfm_coverage_add takes them.  Block k of a problem is its k-th maximal stretch of =/X runs:
 * size = the stretch's columns, eq = the = columns among them, dt = the D bases and dq = the I bases between block k and block k + 1.  Any
 * number of I and D runs may lie between two blocks, in any order: 2I3D gives (3, 2), 10 000 alternating 1I1D give (10000, 10000).  The last
 * block of a problem has dt = dq = 0.  per[i] = {flags, n_runs, first, count, lead_dt, lead_dq, trail_dt, trail_dq, eq, x} locates problem
 * i's blocks, problems in problem order; lead_* and trail_* are the D and I bases before the first block and behind the last one (a chain
 * cannot spell them: the caller moves its start and end by them), eq and x the problem's totals.  A problem of gap runs only is legal:
 * count = 0, no flag, and in the plain output everything in lead_* and trail_* = 0.
 * With the plain output B[0 .. n), the gaps G[0 .. n - 1), lead L and trail R: WFM_CHAIN_REVERSE gives the blocks B[n - 1 - k], the gap
 * behind output block k is G[n - 2 - k], lead becomes R and trail becomes L (what a chain of the other strand lists); WFM_CHAIN_SWAP
 * exchanges the two members of every pair, lead and trail included (what chainSwap does to the two sides); both bits do both.  eq and x
 * do not change under either.  Any other flag bit is WFM_E_ARG with a message.
 * A problem with an empty run, without runs, or whose pattern or text span does not fit 32 bits is flagged WFM_CHAIN_SPANS and has count 0
 * and zeros elsewhere (the spans are taken before anything is written).
 * Per problem the runs are indexed once (four exclusive prefixes per run as one 16-byte word, as wfm_lift_runs); a block's head is an aligned
 * run whose predecessor is not aligned (or the first run); the end of its stretch and the next head are found by binary searches over the
 * prefix words, O(log n_runs), never by a walk.  Blocks are placed by block scans, not atomics: two calls give the same bytes.  The output
 * comes down in chunks of whole problems holding at most WFM_CHAIN_OUT_MB MiB of blocks (environment, a decimal, read per call, 256; one
 * problem at least).  Host memory owned by the caller (wfm_free_chain); NULL and 0 without problems or blocks.  A run range that leaves
 * the run buffer is WFM_E_ARG with a message, the outputs are NULL and the handle stays usable.  Returns WFM_OK or WFM_E_*. */
typedef struct { uint64_t runs_off; uint32_t n_runs, flags; } wfm_chain_prob_t;   /* 16 bytes */
#define WFM_CHAIN_SWAP    1u   /* dt and dq change places (lead and trail pairs too) */
#define WFM_CHAIN_REVERSE 2u   /* blocks from the last to the first; lead and trail change places */
typedef struct { uint32_t size, dt, dq, eq; } wfm_chain_block_t;                  /* 16 bytes */
typedef struct { uint32_t flags, n_runs; uint64_t first, count;
                 uint32_t lead_dt, lead_dq, trail_dt, trail_dq, eq, x; } wfm_chaincall_t;   /* 48 bytes */
#define WFM_CHAIN_SPANS 2u     /* as WFM_LIFT_SPANS: nothing of the problem is written */
int  wfm_chain_runs(wfm_handle_t* h, const wfm_chain_prob_t* probs, size_t n, const uint32_t* runs, size_t n_runs_total,
                    wfm_chain_block_t** blocks, size_t* n_blocks, wfm_chaincall_t* per);
void wfm_free_chain(wfm_chain_block_t* p);

/* ---- presence of target intervals per group of records ----
 * What wfm_coverage_* cannot say: WHICH records cover a base.  Every problem carries a group (a sample, a haplotype); a pav object keeps,
 * per group, the UNION of the = and X bases of the problems added to it, as a list of segments on the handle's device
 * (wfmash_amd/csrc/wfa_pav.hip) -- 16 bytes a segment whatever the target's length, never a dense array -- and answers for every
 * (interval, group) cell how many bases of the interval lie in that group's union.  D bases do not count, I runs advance nothing.
 *
 * wfm_pav_create: n_bases >= 2^40 or n_groups >= 2^24 is WFM_E_ARG with a message: a segment's sort key is group << 40 | start.  On the
 * device a segment is its two keys {group << 40 | start, group << 40 | end}, two 64-bit words; wfm_pav_seg_t is what export and import
 * speak.  The list grows through the device block cache.  The object is used with the handle it was made on and freed before it.
 * wfm_pav_add: probs[i] = {base, runs_off, n_runs, group}, runs as wfm_coverage_add takes them.  One segment per maximal stretch of =/X
 * runs (not per run) is appended.  A problem with an empty run, whose pattern span leaves [0, n_bases] or does not fit 32 bits, or whose
 * group is not below n_groups adds NOTHING and is flagged WFM_PAV_SPANS in flags_out[i] (taken before anything is written).  The slots are
 * placed by scans, not atomics: two calls give the same list.  Returns the number of problems flagged, or WFM_E_*.  Where the raw part
 * of the list then exceeds WFM_PAV_MB MiB (environment, a decimal, read per call, 256) the union is taken at once.
 * wfm_pav_union: the list sorted by key (rocprim::radix_sort_pairs), the inclusive running maximum of the end keys (later groups dominate
 * earlier ones, so a plain prefix maximum is a per-group one; reduce / scan-of-maxima / apply over blocks of WFM_PAV_SCAN_BLOCK segments,
 * three launches), segment i heading a union interval iff i == 0 or its start key > the running maximum before it (abutting segments
 * merge), the heads compacted by a prefix of the flags, a union interval's end the running maximum at its last member.  The disjoint
 * union REPLACES the list, and an exclusive prefix C of its lengths (64 bits) is kept beside it.  Running it twice changes nothing.
 * wfm_pav_export: the union, sorted by (group, start); a union interval of 2^32 bases or more comes as abutting pieces.  Host memory
 * owned by the caller (wfm_pav_free_list); NULL and 0 for an empty object.
 * wfm_pav_import: such a list (any list of segments with length >= 1 inside [0, n_bases] and group < n_groups; anything else is
 * WFM_E_ARG and nothing is added) appended as raw segments: the merge of the objects of several devices is a union of unions.
 * wfm_pav_matrix: iv[0 .. n_iv) half-open global intervals, start <= end <= n_bases and end - start < 2^32, else WFM_E_ARG; out:
 * n_iv * n_groups words, row-major.  One thread per cell, with a = group << 40 | start, b = group << 40 | end over the union's keys:
 * lo = the first u with end key > a, hi = the first u with start key >= b, 0 where hi <= lo, else C[hi] - C[lo] - max(0, a - start[lo])
 * - max(0, end[hi - 1] - b): two binary searches, never a walk.  Rows come down in chunks of at most WFM_PAV_OUT_MB MiB (environment, a
 * decimal, 256; one row at least).
 * wfm_pav_counts: out = {segments added (import included), union intervals after the last union, unions run}. */
typedef struct wfm_pav wfm_pav_t;
typedef struct { uint64_t base, runs_off; uint32_t n_runs, group; } wfm_pav_prob_t;   /* 24 bytes */
typedef struct { uint64_t start; uint32_t length, group; } wfm_pav_seg_t;             /* 16 bytes */
#define WFM_PAV_SPANS 2u          /* as WFM_COV_SPANS: nothing of the problem is added */
#define WFM_PAV_SCAN_BLOCK 1024   /* segments one workgroup takes in the scans of the union */
int  wfm_pav_create(wfm_handle_t* h, uint64_t n_bases, uint32_t n_groups, wfm_pav_t** pav);
void wfm_pav_free(wfm_pav_t* pav);
int  wfm_pav_add(wfm_handle_t* h, wfm_pav_t* pav, const wfm_pav_prob_t* probs, size_t n, const uint32_t* runs, size_t n_runs_total,
                 uint32_t* flags_out);
int  wfm_pav_union(wfm_handle_t* h, wfm_pav_t* pav);
int  wfm_pav_export(wfm_handle_t* h, wfm_pav_t* pav, wfm_pav_seg_t** segs, size_t* n);
int  wfm_pav_import(wfm_handle_t* h, wfm_pav_t* pav, const wfm_pav_seg_t* segs, size_t n);
int  wfm_pav_matrix(wfm_handle_t* h, wfm_pav_t* pav, const wfm_lift_iv_t* iv, size_t n_iv, uint32_t* out);
int  wfm_pav_counts(const wfm_pav_t* pav, uint64_t out[3]);
void wfm_pav_free_list(void* p);

/* ---- the variants of many records joined into sites, and a haploid genotype per (site, group) ----
 * wfm_call_variants names the differences of ONE record.  A sites object takes the variants of many records, each with a GLOBAL position
 * and the group of its record, and the = runs of the same records, and answers with the distinct sites and a table sites x groups.
 *
 * A VARIANT is {pos, kind, group, ref_len, alt_len, off}: what wfm_call_variants calls (WFM_VAR_SNV / _INS / _DEL, without the MASKED
 * bit: the caller leaves masked SNVs out), pos = the global position of its first REF base, REF = alleles[off .. off + ref_len), ALT the
 * alt_len bytes behind.  The allele bytes are folded to upper case on the device: a soft-masked record does not make a second site.
 * A SITE is a distinct (pos, kind, REF bytes, ALT bytes).  Sites are biallelic; nothing is joined into multi-allelic lines.
 * CELL (site, g), haploid:
 *   '1'  at least one variant of group g is exactly this site;
 *   '0'  otherwise, if the whole REF span [pos, pos + ref_len) lies inside the union of the = runs of group g's records -- = runs only,
 *        not =/X; abutting segments of several records merge, as in the pav union; another group's bases never count;
 *   '.'  otherwise: not aligned, under a D, under an X that spells another ALT, or only partly covered.
 * So a group with ANOTHER insertion at the same anchor, = on the anchor, is '0' on this line and '1' on its own (the convention of
 * bcftools norm -m-), and '1' wins over '0' where overlapping records of one group disagree.  The table is a set function of (variants,
 * = runs): the order of records, calls, objects and devices does not change a byte of it.
 *
 * wfm_sites_create: wfm_pav_create's limits and refusals (n_bases < 2^40, n_groups < 2^24).  The object is used with the handle it was
 *   made on and freed before it; it keeps its own device blocks.
 * wfm_sites_add_variants: appends.  WFM_E_ARG with a message, NOTHING added and the handle usable, for: a kind beyond SNV/INS/DEL;
 *   lengths that do not fit the kind (SNV 1/1, INS 1/L+1, DEL L+1/1, L >= 1); pos + ref_len > n_bases; group >= n_groups; an allele
 *   range that leaves alleles[0 .. bytes); more than 2^31 - 1 variants in the object.
 * wfm_sites_add_ref: wfm_pav_add's arguments, flags and return value; one segment per maximal stretch of = RUNS (an X ends a stretch)
 *   goes to a per-group union of its own.  Where the raw part of that list exceeds WFM_SITES_MB MiB (environment, 256) the union is
 *   taken at once.
 * wfm_sites_table: keys k1 = pos << 2 | kind, k2 = a 64-bit hash of the lengths and the folded bytes, k3 = group.  The hash is a
 *   polynomial modulo 2^64 whose per-slice partials add up exactly: alleles of up to WFM_SITES_SLICE bytes (REF + ALT) go one per lane,
 *   longer ones one slice per lane, WFM_SITES_TASK bytes per workgroup.  Three stable radix sorts (k3, k2, k1), each over the bits its
 *   keys can have.  Sorted record i heads a site iff i == 0, or (k1, k2) differ from i - 1's, or the lengths or BYTES differ (long
 *   alleles are compared by workgroups).  Equal keys with different bytes is a COLLISION: counted, and if there is one the call fails
 *   with WFM_E_INTERNAL and a message and returns nothing -- a site is never split or merged silently.  WFM_SITES_HASH_BITS (environment,
 *   per call, 64) cuts k2 to its low bits, for tests.  Returns the sites in ascending pos (the order among the sites of one pos is a
 *   function of the set), one representative's bytes per site (*alleles, off into it), and gt: n_sites * n_groups bytes, row-major.  Rows
 *   come down in chunks of at most WFM_SITES_OUT_MB MiB (environment, per call, 256; one row at least).  Host memory owned by the
 *   caller (wfm_sites_free_list each).  An empty object: WFM_OK, NULLs and 0.
 * wfm_sites_export / _import: the raw variants and their (folded) bytes as add_variants takes them, the = union as wfm_pav_seg_t; the
 *   merge of the objects of several devices is an import.
 * wfm_sites_counts: out = {variants added (import included), distinct sites of the last table, = union intervals after the last union,
 *   collisions of the last table}. */
typedef struct wfm_sites wfm_sites_t;
typedef struct { uint64_t pos; uint32_t kind, group; uint32_t ref_len, alt_len; uint64_t off; } wfm_site_var_t;             /* 32 bytes */
typedef struct { uint64_t pos; uint32_t kind, n_carrier_groups; uint32_t ref_len, alt_len; uint64_t off; } wfm_site_t;     /* 32 bytes */
#define WFM_SITES_SLICE 64       /* allele bytes one lane hashes or compares */
#define WFM_SITES_TASK 16384     /* allele bytes of a long allele pair one workgroup hashes or compares */
int  wfm_sites_create(wfm_handle_t* h, uint64_t n_bases, uint32_t n_groups, wfm_sites_t** s);
void wfm_sites_free(wfm_sites_t* s);
int  wfm_sites_add_variants(wfm_handle_t* h, wfm_sites_t* s, const wfm_site_var_t* vars, size_t n, const char* alleles, size_t bytes);
int  wfm_sites_add_ref(wfm_handle_t* h, wfm_sites_t* s, const wfm_pav_prob_t* probs, size_t n, const uint32_t* runs, size_t n_runs_total,
                       uint32_t* flags_out);
int  wfm_sites_table(wfm_handle_t* h, wfm_sites_t* s, wfm_site_t** sites, size_t* n_sites, char** alleles, size_t* bytes, char** gt);
int  wfm_sites_export(wfm_handle_t* h, wfm_sites_t* s, wfm_site_var_t** vars, size_t* n, char** alleles, size_t* bytes, wfm_pav_seg_t** segs,
                      size_t* n_segs);
int  wfm_sites_import(wfm_handle_t* h, wfm_sites_t* s, const wfm_site_var_t* vars, size_t n, const char* alleles, size_t bytes,
                      const wfm_pav_seg_t* segs, size_t n_segs);
int  wfm_sites_counts(const wfm_sites_t* s, uint64_t out[4]);
void wfm_sites_free_list(void* p);

/* ---- a net across records: which record owns each target base ----
 * wfm_chain_runs makes one chain per record, overlapping records included.  A net object takes the blocks of many records and answers with
 * the PIECES of them that are left when every target base is given to the best record over it (wfmash_amd/csrc/wfa_net.hip).
 *
 * BLOCKS AND RECORDS.  A record's blocks are those of wfm_chain_runs: its maximal stretches of =/X columns.  Block k has a global target
 * start t, a query offset q (the text bases between the first base the runs spell and the block, in the direction of the runs) and a size.
 * D bases belong to no block and are claimed by nobody; I runs advance only q.  Every record carries a score (32 bits) and an order (64
 * bits, unique in the object).  Record A BEATS record B iff score_A > score_B, or the scores are equal and order_A < order_B.
 * OWNER AND PIECES.  The owner of a target base is the best record with a block over it; a base under no block has no owner.  A piece is a
 * maximal stretch of consecutive bases with the same owner inside the same block of that owner (two blocks of one record never abut or
 * overlap, so "the same block" only matters for the definition): {order, t, q, size}, q = the block's q + (t - the block's t).  The NET is
 * the list of pieces sorted by (order, t); per record it also gives the number of pieces and the bases won.  The net is a set function of
 * (blocks, scores, orders): no order of calls, batches, threads or devices changes a byte of it.
 * Deliberately none of these: chainNet's minSpace, minFill and minScore thresholds; nesting levels or a .net file; joining of records into
 * one chain; single coverage on the query side.
 *
 * wfm_net_create: n_bases >= 2^40 is WFM_E_ARG with a message, as wfm_pav_create.  The object keeps its own device blocks (through the
 *   block cache), is used with the handle it was made on and freed before it.  Memory follows the blocks, never n_bases.
 * wfm_net_add: probs[i] = {base, runs_off, n_runs, score, order}, runs as wfm_coverage_add takes them.  score == WFM_NET_SCORE_EQ: the
 *   problem's = columns, counted on the device.  One record entry per problem and one block per maximal stretch of =/X runs are appended;
 *   a problem of gap runs only adds a record without blocks.  A problem with an empty run, without runs, or whose pattern or text span
 *   does not fit 32 bits or leaves [0, n_bases] adds NOTHING and is flagged WFM_NET_SPANS in flags_out[i] (taken before anything is
 *   written).  The slots are placed by scans, not atomics: two calls give the same list.  A run range that leaves the run buffer is
 *   WFM_E_ARG with a message, and the handle stays usable.  Returns the number of problems flagged, or WFM_E_*.
 * wfm_net_table: the net.  With N blocks: the 2 N block ends sorted (rocprim::radix_sort_keys) and compacted to the distinct coordinates
 *   x[0 .. M], M <= 2 N - 1 elementary intervals; the records ranked by order and, by a second sort, given a dense priority (score
 *   descending, order ascending); one lane per block finds its leaves [lo, hi) by two binary searches in x and takes a 64-bit integer
 *   maximum of priority << 32 | block index into the O(log M) canonical nodes of an implicit segment tree over the M leaves (the maximum
 *   of integers does not depend on the order of arrival); the maxima are pushed down level by level, one launch per level, a gather from
 *   the parent; leaf k heads a piece iff its winner is non-zero and differs from leaf k - 1's; heads and tails are compacted by prefixes
 *   of the flags; the pieces, which arrive in t order, are sorted stably by their record's rank in order.  Work is O((N + M) log M)
 *   whatever the number of blocks that pile on a base.  Pieces come down in chunks of at most WFM_NET_OUT_MB MiB (environment, a decimal,
 *   read per call, 256; one piece at least).  per[i] = {order, score as used, 0, first, count, bases_won, bases_aligned}, sorted by order,
 *   locates record i's pieces.  Two records with the same order: WFM_E_ARG with a message, nothing written.  An empty object: WFM_OK, NULLs
 *   and 0.  Host memory owned by the caller (wfm_net_free_list each).  The object is not changed: more may be added and the table taken again.
 * wfm_net_export / _import: the raw blocks and record entries, so that the objects of several handles merge.  Import looks at
 *   everything on the host before anything is added: size >= 1, the block inside [0, n_bases], q + size below 2^32, and every block's
 *   record among the records given or already in the object; anything else is WFM_E_ARG with a message and nothing is added.  (That the
 *   blocks of one record do not overlap is the caller's to keep: wfm_net_add's do not.)
 * wfm_net_counts: out = {records added, blocks added (import included), and of the last table: elementary intervals M, pieces, records
 *   that won nothing, 0}. */
typedef struct wfm_net wfm_net_t;
typedef struct { uint64_t base, runs_off; uint32_t n_runs, score; uint64_t order; } wfm_net_prob_t;   /* 32 bytes */
typedef struct { uint64_t order, t; uint32_t q, size; } wfm_net_block_t;                               /* 24 bytes: a block, and a piece */
typedef wfm_net_block_t wfm_net_piece_t;
typedef struct { uint64_t order; uint32_t score, zero; } wfm_net_rec_t;                                /* 16 bytes */
typedef struct { uint64_t order; uint32_t score, zero; uint64_t first, count, bases_won, bases_aligned; } wfm_netcall_t;   /* 48 bytes */
#define WFM_NET_SCORE_EQ 0xffffffffu   /* wfm_net_prob_t::score: take the problem's = columns */
#define WFM_NET_SPANS 2u               /* as WFM_PAV_SPANS: nothing of the problem is added */
#define WFM_NET_SCAN_BLOCK 1024        /* elements one workgroup takes in the scans of the table */
int  wfm_net_create(wfm_handle_t* h, uint64_t n_bases, wfm_net_t** net);
void wfm_net_free(wfm_net_t* net);
int  wfm_net_add(wfm_handle_t* h, wfm_net_t* net, const wfm_net_prob_t* probs, size_t n, const uint32_t* runs, size_t n_runs_total,
                 uint32_t* flags_out);
int  wfm_net_table(wfm_handle_t* h, wfm_net_t* net, wfm_net_piece_t** pieces, size_t* n_pieces, wfm_netcall_t** per, size_t* n_records);
int  wfm_net_export(wfm_handle_t* h, wfm_net_t* net, wfm_net_block_t** blocks, size_t* n_blocks, wfm_net_rec_t** recs, size_t* n_recs);
int  wfm_net_import(wfm_handle_t* h, wfm_net_t* net, const wfm_net_block_t* blocks, size_t n_blocks, const wfm_net_rec_t* recs, size_t n_recs);
int  wfm_net_counts(const wfm_net_t* net, uint64_t out[6]);
void wfm_net_free_list(void* p);

/* ---- transitive lifts: intervals closed over all records, in both directions ----
 * wfm_lift_runs says where a target interval lies in the query of ONE record.  A trans object keeps the records of a whole run on the
 * handle's device and answers, per seed interval, with everything the seed reaches through any chain of records, either way
 * (wfmash_amd/csrc/wfa_trans.hip).
 *
 * WORLD.  One coordinate space of n_bases < 2^40: the caller's to lay out (the driver puts the target sequences first, in index order,
 *   then the query sequences whose names no target has).
 * RECORD.  {t, q, flags, runs}: t = the world position of the first pattern base the runs spell, q = the world position of the first
 *   base of the FORWARD query window the runs spell.  WFM_TRANS_REVERSE: the text is the reverse complement of that window, text index i
 *   is world base q + T - 1 - i (T the text span); otherwise q + i.  P and T, the pattern and text spans, come from the runs.
 * ARCS.  Every record is TWO arcs: forward, source [t, t + P), destination the query window; back, source [q, q + T), destination the
 *   target.  A source base is ALIGNED where an = or X column holds it.
 * HULL.  hull(arc, [a, b)): [a, b) clipped to the arc's source span; where nothing is left or no aligned source base lies inside, the
 *   arc gives NOTHING (wfm_lift_runs reports an empty lift there).  Otherwise the first and the last aligned source base inside
 *   (endpoints in a gap run snap inward), the destination bases opposite them, and the half-open world interval from the smaller to the
 *   larger of the two, inclusive.  Gap runs strictly between two lifted columns are inside it; a gap run before the first or behind the
 *   last lifted column is not.  On the forward arc it is wfm_lift_runs' [t0, t1) moved to the world.
 * CLOSURE.  Per seed s: R_0 = {s}; R_(k+1) = R_k united with hull(arc, J) over all arcs and over the MAXIMAL intervals J of R_k
 *   (abutting and overlapping intervals are merged first, which makes the closure a set function of (records, seed): no order of records,
 *   calls, objects or devices changes a byte).  depth N >= 1 gives R_N; depth 0 walks until R_(k+1) = R_k (the covered bases are
 *   compared: R_k is inside R_(k+1)).  Seeds never merge with each other.  A maximal interval of R_k that R_(k-1) had as it is is not
 *   projected again: its hulls are in R_k.
 *
 * wfm_trans_create: n_bases >= 2^40 is WFM_E_ARG with a message.  The object is used with the handle it was made on and freed before it.
 * wfm_trans_add: probs[i] = {t, q, runs_off, n_runs, flags}, runs as wfm_coverage_add takes them, ONE call per batch.  A problem with an
 *   empty run, without runs, or whose pattern or text span does not fit 32 bits or leaves the world adds NOTHING and is flagged
 *   WFM_TRANS_SPANS in flags_out[i] (decided by a first kernel, before anything is written).  A run range that leaves the run buffer or a
 *   flag bit other than WFM_TRANS_REVERSE is WFM_E_ARG with a message, and the handle stays usable.  Kept per record: its n_runs + 1
 *   prefix words {pattern, text, = columns, X columns} (16 bytes a run, the totals behind the last; the runs themselves are not kept) and
 *   two 32-byte arc entries, in blocks of the object's own that grow by half through the device block cache.  Memory follows the records,
 *   never n_bases.  Where what the object keeps (the sorted copy of the arcs and its running maximum included) would exceed WFM_TRANS_GB
 *   GiB (environment, a decimal, read per call, 32) the call fails with WFM_E_NOMEM and a message that names the pass, and nothing is
 *   added.  Returns the number of problems flagged, or WFM_E_*.
 * wfm_trans_closure: seeds[i] = a half-open world interval, start < end <= n_bases, n_seeds < 2^24, depth >= 0; anything else is
 *   WFM_E_ARG with a message.  The index is made first where an add or import came since the last one: the arcs sorted by source start
 *   (rocprim::radix_sort_pairs over the bits n_bases has) and pm = the running maximum of their source ends.  One round: one workgroup
 *   per interval [a, b) of the list finds its arcs [lo, hi) (lo = the first with pm > a, hi = the first with start >= b) and counts those
 *   with end > a; the counts become offsets; the host walks the intervals in chunks of at most WFM_TRANS_OUT_MB MiB of pairs
 *   (environment, a decimal, read per call, 256; one interval at least); one lane per (interval, arc) pair resolves the hull in four
 *   binary searches over the record's prefix words and writes seed << 40 | lo and seed << 40 | hi (an empty hull writes its interval
 *   again, which adds nothing); the list and the chunk's pairs are united as wfm_pav_union unites segments (sort, running maximum, heads,
 *   compaction).  ivs: the result sorted by (seed, start), disjoint and not abutting per seed; per_seed[i] = {first, count, bases} locates
 *   seed i's.  Host memory owned by the caller (wfm_trans_free_list each; per_seed may be NULL).  The object is not changed: more may be
 *   added and the closure taken again.
 * wfm_trans_export / _import: the records {t, q, pre_off, n_runs, flags} and their prefix words (pre_off counts words from the first
 *   one exported), so that the objects of several handles merge; the two arcs of a record follow from its entry.  Import looks at
 *   everything on the host before anything is added: every record's words inside the list, the first one zero, every step one run of
 *   =, X, I or D of length >= 1, the spans inside the world, no unknown flag; anything else is WFM_E_ARG with a message.
 * wfm_trans_counts: out = {records kept, prefix words kept, arcs, and of the last closure: rounds run, intervals returned, pairs
 *   projected}. */
typedef struct wfm_trans wfm_trans_t;
typedef struct { uint64_t t, q, runs_off; uint32_t n_runs, flags; } wfm_trans_prob_t;   /* 32 bytes */
typedef struct { uint64_t t, q, pre_off; uint32_t n_runs, flags; } wfm_trans_rec_t;     /* 32 bytes */
typedef struct { uint32_t p, t, eq, x; } wfm_trans_word_t;                              /* 16 bytes: the exclusive prefixes of one run */
typedef struct { uint64_t start, end; uint32_t seed, pad_; } wfm_trans_iv_t;            /* 24 bytes */
typedef struct { uint64_t first, count, bases; } wfm_trans_seed_t;                      /* 24 bytes */
#define WFM_TRANS_REVERSE 1u        /* wfm_trans_prob_t::flags: the text is the reverse complement of the query window */
#define WFM_TRANS_SPANS 2u          /* as WFM_NET_SPANS: nothing of the problem is added */
#define WFM_TRANS_SCAN_BLOCK 1024   /* arcs one workgroup takes in the running maximum */
int  wfm_trans_create(wfm_handle_t* h, uint64_t n_bases, wfm_trans_t** obj);
void wfm_trans_free(wfm_trans_t* obj);
int  wfm_trans_add(wfm_handle_t* h, wfm_trans_t* obj, const wfm_trans_prob_t* probs, size_t n, const uint32_t* runs, size_t n_runs_total,
                   uint32_t* flags_out);
int  wfm_trans_closure(wfm_handle_t* h, wfm_trans_t* obj, const wfm_lift_iv_t* seeds, size_t n_seeds, uint32_t depth, wfm_trans_iv_t** ivs,
                       size_t* n_ivs, wfm_trans_seed_t* per_seed);
int  wfm_trans_export(wfm_handle_t* h, wfm_trans_t* obj, wfm_trans_rec_t** recs, size_t* n_recs, wfm_trans_word_t** words, size_t* n_words);
int  wfm_trans_import(wfm_handle_t* h, wfm_trans_t* obj, const wfm_trans_rec_t* recs, size_t n_recs, const wfm_trans_word_t* words, size_t n_words);
int  wfm_trans_counts(const wfm_trans_t* obj, uint64_t out[6]);
void wfm_trans_free_list(void* p);

/* ---- the aligned sequences themselves: the two gapped rows of every problem's runs, as pairwise MAF blocks ----
 * What `wgatools paf2maf` and its like make of a PAF on one CPU thread with both FASTAs open again.  This call spells the rows on the
 * device (wfmash_amd/csrc/wfa_maf.hip; forward BYTE copies only, shares nothing with the aligners).  Pattern = target side P, text =
 * query side T AS ALIGNED (for a `-` record T is the reverse complement of the query window: wfm_cs_strings' convention).  The runs are
 * read from left to right and every column of a run yields one byte in row P and one byte in row T:
 *
 *   run        row P             row T
 *   = of L     P[p .. p + L)     T[t .. t + L)
 *   X of L     P[p .. p + L)     T[t .. t + L)
 *   I of L     L x '-'           T[t .. t + L)
 *   D of L     P[p .. p + L)     L x '-'
 *
 * The bytes are emitted as the device holds them (what --cs=long prints behind `=`: upper-cased by the upload, non-ACGT as the upload left
 * it, no case change here).  The rows are spelled from the runs, never from a comparison: an = run over different bytes prints both bytes
 * as they are; whether the runs fit the bases is wfm_check_runs' business.
 *
 * Blocks and split.  A gap stretch is a maximal sequence of consecutive I / D runs.  With split = 0 a problem is ONE block of all its
 * runs.  With split = N >= 1 a gap stretch whose I bases + D bases >= N is a BREAK: none of its columns are written, it ends the block
 * before it and the next block begins behind it; a block is a maximal run sequence between breaks.  A break at the problem's first or
 * last run yields no block on that side; a problem that is only a break has count = 0 and no flag.  Where a problem begins and ends with
 * = / X (the align driver's do) every block begins and ends with an aligned column; through this call a block may have psize == 0 or
 * tsize == 0, which is legal and reported as it is.
 *
 * Per block {off, problem, p, t, psize, tsize, cols, eq, x}: p / t the indices in P and T where the block begins, psize / tsize the
 * non-gap bytes of each row, cols its columns, eq / x its = and X columns; row P is rows[off .. off + cols), row T is
 * rows[off + cols .. off + 2 cols).  The blocks are listed in problem order, left to right inside a problem; off is contiguous
 * (next.off = off + 2 cols) and *bytes = 2 x the sum of cols.  per[i] = {flags, n_runs, first, count}: the problem's blocks are
 * (*blocks)[first .. first + count).  s, res and runs exactly as for wfm_cs_strings (any order, unused words between the problems).
 * Returns the number of problems flagged WFM_MAF_SPANS, or a WFM_E_* code; a run range that leaves runs[0 .. n_runs_total) is WFM_E_ARG
 * with a message, the outputs NULL and the handle usable.  No problems, or no blocks: WFM_OK (or the count), NULL and 0.  Host memory
 * owned by the caller (wfm_free_maf).  One workgroup writes WFM_MAF_SLICE bytes of the rows whatever blocks or problems they belong to;
 * the problems are worked in chunks of whole problems whose block table and rows hold at most WFM_MAF_OUT_MB MiB on the device
 * (environment, a decimal read per call, 256; a single problem may exceed it alone).  No atomics: two calls give the same bytes. */
#define WFM_MAF_NOT_DONE 1u   /* status != 0, score-only, no runs: count = 0 */
#define WFM_MAF_SPANS    2u   /* as WFM_CS_SPANS: count = 0, nothing of the problem is spelled */
typedef struct { uint64_t off; uint32_t problem, p, t, psize, tsize, cols, eq, x; } wfm_maf_block_t;  /* 40 bytes */
typedef struct { uint32_t flags, n_runs; uint64_t first, count; } wfm_mafcall_t;                      /* 24 bytes */
#define WFM_MAF_SLICE 16384   /* output bytes one workgroup writes */
int  wfm_maf_rows(wfm_handle_t* h, const wfm_seqset_t* s, const wfm_result_t* res, const uint32_t* runs, size_t n_runs_total,
                  uint32_t split, wfm_maf_block_t** blocks, size_t* n_blocks, char** rows, size_t* bytes, wfm_mafcall_t* per);
void wfm_free_maf(wfm_maf_block_t* blocks, char* rows);

/* ---- every score proved optimal by a banded DP ----
 * What wfm_check_runs leaves out.  For every problem of the seqset s whose result claims a score S = res[i].score, a classical
 * minimising gap-affine-2-piece DP over cells (i = pattern index, j = text index) is run on the device, restricted to a band of
 * diagonals k = j - i; the kernel (wfmash_amd/csrc/wfa_optcheck.hip) shares no code with the aligners, reads the forward BYTE copies
 * only and compares bytes as bytes (N equals N, 'a' differs from 'A').  END2END_BIWFA and END2END_UNI run from (0, 0) to
 * (plen, tlen); ENDSFREE starts at price 0 on (0, j <= text_begin_free) or (i <= pattern_begin_free, 0) and ends at the minimum over
 * (plen, j >= tlen - text_end_free) and (i >= plen - pattern_end_free, tlen).  Score-only results are checked like any other.
 *
 * The band lemma.  g(L) = min(o1 + e1 L, o2 + e2 L) for L > 0, 0 otherwise; kf = tlen - plen; start diagonals [-pbf, tbf], end
 * diagonals [kf - tef, kf + pef] (free lengths clamped to their sequence; end-to-end: 0 and kf).  With hi0 = max(tbf, kf + pef) and
 * lo0 = min(-pbf, kf - tef): every diagonal in [lo0, hi0] is in the band; k > hi0 iff g(k - tbf) + g(k - kf - pef) <= S; k < lo0 iff
 * g(-pbf - k) + g(kf - tef - k) <= S.  (A path that reaches a diagonal above both its start and its end inserts at least k - ks bases
 * on the way out and deletes at least k - ke on the way back, in runs of their own; g is non-decreasing and subadditive, so the runs
 * of one kind cost at least g of their total.  Between start and end diagonals nothing can be excluded.)  Every alignment of price
 * <= S therefore lies inside the band, and the banded optimum dp tells the whole story: dp == S: S is optimal; dp < S: a cheaper
 * alignment exists (and dp is the true optimum); dp > S or no path inside the band: no alignment of price S exists.
 * band_lo / band_hi report the band, cut to the matrix [-plen, tlen].
 *
 * What is proved: that res[i].score is the optimal price of problem i's two byte strings under pen and its mode.  What is not: that
 * the CIGAR has that price or fits its bases (wfm_check_runs), that it is the reference's choice among co-optimal alignments, or
 * anything the host does to it afterwards.
 *
 * One workgroup per problem, so throughput rests on many problems per call (64 problems fill 64 of 256 CUs, and one huge problem
 * runs on one CU however empty the device is).  Rows of a band of up to WFM_OPT_BAND_C1 diagonals stay in registers with 1 diagonal
 * per thread (256 threads), up to WFM_OPT_BAND_C4 with 4 (256 threads), up to WFM_OPT_REG_MAX with 8 (512 threads); a wider band keeps
 * its rows in a block of the device heap, 12 bytes per diagonal, swept in tiles of WFM_OPT_REG_MAX diagonals by 1024 threads, and no
 * band is refused for its width.  The problems of a call are launched largest first; the memory-held rows of one launch take at most
 * WFM_OPT_ROWS_MB MiB (one problem alone may take more), and the problems run in chunks if they do not all fit.
 * Penalties: x, e1, e2 > 0 and o1, o2 >= 0, each at most 32767 (WFM_E_UNSUPPORTED otherwise); the aligners' scope limit does not apply.
 * A problem is WFM_OPT_NOT_CHECKED if its status != 0, its score < 0 or its score >= 2^29 (the DP's "no path").  max_cells caps the
 * cells of one problem's band (0: no cap): a problem beyond it is WFM_OPT_SKIPPED and nothing of it is computed.
 * Returns the number of problems flagged CHEAPER or UNREACHED, or a WFM_E_* code. */
#define WFM_OPT_NOT_CHECKED 1u  /* status != 0 or score < 0 */
#define WFM_OPT_SKIPPED     2u  /* the band holds more cells than max_cells: nothing was computed */
#define WFM_OPT_CHEAPER     4u  /* an alignment cheaper than res[i].score exists: the score is not optimal */
#define WFM_OPT_UNREACHED   8u  /* no alignment of price res[i].score exists */
typedef struct {
  uint32_t flags; int32_t dp_score;     /* the best price inside the band (-1: no path inside); the true optimum whenever <= the claim */
  int32_t  band_lo, band_hi;            /* the band of diagonals that was swept (0, -1 when nothing was) */
  uint64_t cells;                       /* DP cells computed (0 when skipped or not checked) */
} wfm_optcheck_t;                       /* 24 bytes */
#define WFM_OPT_BAND_C1   256           /* widest band with 1 diagonal per thread */
#define WFM_OPT_BAND_C4   1024          /* ... with 4 */
#define WFM_OPT_REG_MAX   4096          /* ... with 8 (512 threads): the widest band whose rows stay in registers; the memory form's tile */
#define WFM_OPT_ROWS_MB   256           /* device heap the memory-held rows of one launch may take */
int wfm_check_optimal(wfm_handle_t* h, const wfm_penalties_t* pen, const wfm_seqset_t* s,
                      const wfm_result_t* res, uint64_t max_cells /* per problem, 0 = no cap */, wfm_optcheck_t* out);

/* How many other align calls the caller keeps in flight on this handle's DEVICE while a call on this handle runs (the align
 * driver's workers, each on a handle of its own: wfmash_amd/host/aligner.cpp).  0, the default: none -- a batch is then cut
 * into up to three parts that run side by side on streams of their own, because the levels of a batch of near-identical
 * records are chains of short launches (a block of 100 scores takes its 0.13 ms however few workgroups it has) and the device
 * is only filled by several chains at once; with other calls beside it a batch of hundreds of hinted records stays one part
 * (three chains on a device are what its hardware queues run in parallel; gpurun_out/r5f_ab.log). */
void wfm_set_concurrent_calls(wfm_handle_t* h, int other_calls);

/* Which of the rarer paths the problems of the handle's LAST align call took, one word of WFM_PF_* bits per problem (a
 * diagnostic channel: the parity tests and bench.py draw their samples from it, so that the records whose root ran again,
 * whose patches went to a second or third score budget, or which ran on the byte kernels are all checked against the oracle
 * instead of the one in fifty a uniform sample holds).  out may be NULL; returns the number of problems of that call. */
#define WFM_PF_ROOT_AGAIN   1u   /* the root ran past its score hint / out of its narrow ring and was run again        */
#define WFM_PF_JOB_AGAIN    2u   /* a BiWFA child ran out of its narrow ring and was run again on a full one          */
#define WFM_PF_BASE_RETRY   4u   /* a leaf / ends-free patch overflowed its first score budget                        */
#define WFM_PF_BASE_RETRY2  8u   /* ... and its second (1020): the third attempt runs to the all-gap bound            */
#define WFM_PF_BYTE_KERNEL 16u   /* an N or a soft-masked base: the byte kernels instead of the 2-bit packed ones     */
#define WFM_PF_P2_ROUNDS   32u   /* an overlap walk went past the first round of rows computed ahead                  */
#define WFM_PF_RING_KERNEL 64u   /* a leaf / patch ran on the global-memory ring kernel (other penalties, an N; rows beyond 2048 diagonals until round 6) */
#define WFM_PF_BASE_TILES 128u   /* a patch with rows beyond 2048 diagonals ran as tiles of the register kernel (its third attempt)   */
#define WFM_PF_RING_GROWN 256u   /* the full ring of the root or of a child did not fit the budget: it ran on rings grown with its score   */
size_t wfm_get_problem_flags(const wfm_handle_t* h, uint32_t* out, size_t n);

/* Which paths the BiWFA tile phase took in the handle's LAST align call, summed over the call's parts and streams (a
 * diagnostic channel like the flags above: the block-boundary tests assert from it that the path they aim at ran).  Fills
 * out[0 .. min(n, WFM_TILE_COUNTERS)) in the order below; out may be NULL; returns WFM_TILE_COUNTERS. */
enum {
  WFM_TC_JOBS = 0,          /* jobs that entered the tile phase (a job that goes on from a snapshot on a wider ring enters again) */
  WFM_TC_EXACT_ENDS = 1,    /* jobs that left it stopped exactly at their meeting point                                          */
  WFM_TC_FINE_RERUNS = 2,   /* meeting blocks found with one maximum per block and run again with per-score maxima               */
  WFM_TC_GAP_RERUNS = 3,    /* blocks before a short run up to the meeting point run again for their gap rows                    */
  WFM_TC_RING3 = 4,         /* jobs that held a third ring                                                                       */
  WFM_TC_BLOCKS_COARSE = 5, /* blocks launched with the packed tile kernel's instantiation without per-score maxima              */
  WFM_TC_BLOCKS_FINE = 6,   /* blocks launched with the one that keeps them                                                      */
  WFM_TC_LEFT_BAND = 7,     /* jobs that left out of their band or out of their score bound                                      */
  WFM_TC_REUSE_RESUMED = 8,   /* jobs whose outer direction went on from rows their parent kept (parent reuse)                    */
  WFM_TC_REUSE_FALLBACKS = 9, /* jobs that came with such rows and gave them up: they ran (or were run again) from score 0           */
  WFM_TC_REUSE_KEEPS = 10,    /* snapshots of one direction written to the store of kept rows                                        */
  /* the fallbacks by cause (the two add up to WFM_TC_REUSE_FALLBACKS): */
  WFM_TC_REUSE_TOUCHED = 11,  /* the restore found a kept cell on the job's box or beyond it (v >= hmax_c(k) - WFM_REUSE_TOUCH_SLACK)    */
  WFM_TC_REUSE_FELL_OTHER = 12, /* any other cause: the maxima fired while one direction waited, the job met right behind the restore ... */
  WFM_TC_PLANNED_ENDS = 13,  /* jobs that ended phase 1 at the state planned from their known score, without a search (WFM_TILE_PLANNED_END)   */
  WFM_TC_P2_EXACT = 14,        /* jobs whose phase 2 took the exact walk: they stood at their own score, so only pairs of exactly that score were looked at (WFM_P2_EXACT) */
  WFM_TC_P2_EXACT_MISSES = 15, /* of those, the jobs that found no such pair within its reach and went through the ordinary walk from the same state                    */
  WFM_TILE_COUNTERS = 16
};
size_t wfm_get_tile_counters(const wfm_handle_t* h, uint64_t* out, size_t n);

/* Device blocks of both paths -- the map path's work buffers, the align path's arenas and a batch's sequence buffers, also
 * those of a handle that has been destroyed -- come from one heap per device and go back to it (wfmash_amd/csrc/dev_cache.h: an
 * address range reserved at the first wfm_create of the device, 1 GB chunks mapped behind what is there, WFM_POOL_GB -- 24 -- at once;
 * memory a process has never had costs ~30 ms per GB on this driver beyond its first ~30 GB, profiles/r6_vmm_fresh.md).  This hands
 * the free chunks at every heap's end (and the cached blocks under a megabyte) back to the driver and returns the bytes released. */
size_t wfm_trim_device_cache(void);

int  wfm_get_stats(const wfm_handle_t* h, wfm_stats_t* out);
/* The intervals during which a kernel of the handle's last align call was running, merged, as (start, end) pairs in ms on a
 * clock all handles of one device share: a caller that keeps several calls in flight on handles of their own (the align
 * driver does) merges them to get the time the device was really busy.  Returns their number (may exceed cap). */
size_t wfm_get_busy_intervals(const wfm_handle_t* h, double* start_end_ms, size_t cap);

/* ---- map path (see header comment for the reference functions) ---- */

/* Canonical k-mer hashes of every k-mer start 0..len-k of seq (upper-cased,
 * non-ACGT treated as N as makeUpperCaseAndValidDNA, commonFunc.hpp:132-142).
 * hash[i]   = min(getHash(fwd), getHash(revcomp)) ; strand[i] = +1 fwd < rev,
 * -1 rev < fwd, 0 palindromic or contains N (hash[i] undefined = UINT64_MAX). */
int  wfm_hash_kmers(wfm_handle_t* h, const char* seq, int64_t len, int k,
                    uint64_t* hash, int8_t* strand);

/* skch::MinmerInfo (base_types.hpp:28-35), 32 bytes */
typedef struct {
  uint64_t hash;
  int64_t  wpos;
  int64_t  wpos_end;
  int32_t  seqId;
  int16_t  strand;
  int16_t  pad_;
} wfm_minmer_t;

/* sketchSequence over n fragments of one buffer: fragment f = seq[frag_off[f] ..
 * frag_off[f]+frag_len[f]).  For each fragment the bottom-s distinct canonical
 * hashes ascending (commonFunc.hpp:218-323).  out holds n*s entries;
 * out_count[f] <= s. */
int  wfm_sketch_fragments(wfm_handle_t* h, const char* seq, int64_t seq_len,
                          const int64_t* frag_off, const int32_t* frag_len, size_t n,
                          int k, int s, int32_t seq_id,
                          wfm_minmer_t* out, int32_t* out_count);

/* skch::IntervalPoint (base_types.hpp:63-76), 24 bytes: endpoints of minmer intervals */
typedef struct {
  int64_t  pos;
  uint64_t hash;
  int32_t  seqId;
  int8_t   side;      /* OPEN = 1, CLOSE = -1 (base_types.hpp:123-127) */
  int8_t   pad_[3];
} wfm_interval_point_t;

/* Device-resident reference index: Sketch::build's index stage (winSketch.hpp:266-429).
 * `minmers` = the minmer intervals of all target sequences concatenated in seqId order (the
 * output of wfm_add_minmers per sequence).  max_kmer_freq as -F (parse_args.hpp:734-737;
 * <= 1: fraction of windows, > 1: absolute count; default 0.0002). */
typedef struct wfm_index wfm_index_t;
typedef struct {
  int64_t  n_windows;   /* minmer intervals given ("windows") */
  int64_t  n_kept;      /* size of minmerIndex after the frequency filter */
  int64_t  n_unique;    /* unique hashes in the position lookup */
  int64_t  n_points;    /* interval points */
  uint64_t threshold;   /* count_threshold actually used */
  int64_t  filtered;    /* intervals dropped by the frequency filter */
  int32_t  adjusted;    /* 1 if the over-filtering safety check raised the threshold (winSketch.hpp:326-349) */
  int32_t  pad_;
} wfm_index_info_t;
int  wfm_index_build(wfm_handle_t* h, const wfm_minmer_t* minmers, int64_t n, double max_kmer_freq, wfm_index_t** out);
void wfm_index_free(wfm_handle_t* h, wfm_index_t* ix);
int  wfm_index_info(const wfm_index_t* ix, wfm_index_info_t* out);
/* Copies the index back to the host (any pointer may be NULL): unique hashes ascending,
 * n_unique+1 offsets into points, the points, and minmerIndex. */
int  wfm_index_download(wfm_handle_t* h, const wfm_index_t* ix, uint64_t* uhash, int64_t* poff,
                        wfm_interval_point_t* points, wfm_minmer_t* minmers);

/* The index on another GPU of the same node (the index is replicated, read-only, on every device that maps:
 * computeMap.hpp:431-484 shares one Sketch between all worker threads).  Device-to-device copies of the four
 * arrays; *out belongs to dst (wfm_index_free(dst, *out)).  src == dst gives a second copy on the same device. */
int  wfm_index_replicate(wfm_handle_t* src, const wfm_index_t* ix, wfm_handle_t* dst, wfm_index_t** out);

/* The inverse of wfm_index_download: a device index from the structures of an index file (`-I`;
 * Sketch::readIndex, winSketch.hpp:834-866, host/index_file.cpp reads the file).  uhash ascending,
 * poff[n_unique + 1] offsets into points, minmers = minmerIndex sorted by (seqId, wpos). */
int  wfm_index_upload(wfm_handle_t* h, const uint64_t* uhash, const int64_t* poff, int64_t n_unique,
                      const wfm_interval_point_t* points, const wfm_minmer_t* minmers, int64_t n_kept,
                      wfm_index_t** out);

/* addMinmers (commonFunc.hpp:440-708): winnowed minmer intervals [wpos, wpos_end) of one target
 * sequence, sorted by (wpos, wpos_end), spans chunked to <= w.  This single-sequence form hashes on
 * the GPU and winnows on the calling host thread (the threads == 1 path; it is what the tests use
 * as the one-stream form).  The production path is wfm_add_minmers_multi / wfm_index_build_sequences:
 * hashing, thinning, winnowing (one wave per speculative chunk) and the closing sort all on the device.
 * Returns the number of intervals (which may exceed cap; only cap are written) or a negative WFM_E_* code. */
int64_t wfm_add_minmers(wfm_handle_t* h, const char* seq, int64_t len, int k, int w, int s, int32_t seq_id,
                        wfm_minmer_t* out, int64_t cap);

/* wfm_add_minmers for nseq sequences (the reference: one sequence per ThreadPool worker,
 * winSketch.hpp:200-239).  With threads > 1 every stage runs on the device: hashing, thinning of the
 * k-mer stream, winnowing (map_winnow.hip: one wave per speculative chunk, chunks of many sequences in
 * one launch) and the closing std::sort order (map_finish.hip); a sequence the device hands back (an N
 * among its first k-mers that the reference does not notice, a refill anomaly) is winnowed by the
 * `threads` host workers.  out receives the intervals of all sequences concatenated
 * in input order, counts[i] (optional) the number of sequence i.  Returns the total (may exceed
 * cap; only cap are written) or a WFM_E_* code. */
int64_t wfm_add_minmers_multi(wfm_handle_t* h, const char* const* seqs, const int64_t* lens, const int32_t* seq_ids,
                              int64_t nseq, int k, int w, int s, int threads, wfm_minmer_t* out, int64_t cap, int64_t* counts);

/* Sketch::build in one call (winSketch.hpp:175-457): wfm_add_minmers_multi followed by wfm_index_build, with the
 * minmer intervals going from the host workers straight to the device (no host array of all intervals).  The
 * index equals wfm_index_build(wfm_add_minmers_multi(...)).  *n_windows (optional) receives the number of
 * intervals; when it is 0 no index is made and *out stays NULL. */
int wfm_index_build_sequences(wfm_handle_t* h, const char* const* seqs, const int64_t* lens, const int32_t* seq_ids,
                              int64_t nseq, int k, int w, int s, int threads, double max_kmer_freq,
                              wfm_index_t** out, int64_t* n_windows);

/* Sketch::build split at its seam, for a target subset whose sequences are sketched on several GPUs of the node
 * (wfmh_map_multi): the records of a share of the sequences stay on the device that made them (a part), and the index
 * stage runs once on the union of all parts.
 *
 * wfm_sketch_part: wfm_add_minmers_multi's pipeline with the records left on h's device (one block of the device heap),
 * grouped by sequence in input order; a sequence shorter than k contributes 0 records.  The part outlives the call's
 * work buffers and may outlive h; release it with wfm_minmer_part_free. */
typedef struct wfm_minmer_part wfm_minmer_part_t;
int  wfm_sketch_part(wfm_handle_t* h, const char* const* seqs, const int64_t* lens, const int32_t* seq_ids, int64_t nseq,
                     int k, int w, int s, int threads, wfm_minmer_part_t** out);
/* *n_records (optional) = records of the part; counts (optional) receives min(cap, sequences) per-sequence counts.
 * Returns the number of sequences or a WFM_E_* code. */
int64_t wfm_minmer_part_info(const wfm_minmer_part_t* part, int64_t* n_records, int64_t* counts, int64_t cap);
/* The records on the host (up to cap of them), grouped by sequence in the part's order; h: any handle, it carries the
 * error message.  Returns the number of records (may exceed cap) or a WFM_E_* code. */
int64_t wfm_minmer_part_download(wfm_handle_t* h, const wfm_minmer_part_t* part, wfm_minmer_t* out, int64_t cap);
void wfm_minmer_part_free(wfm_minmer_part_t* part);

/* The index stage on the union of parts: order[i] names the i-th sequence of the union (the reference's minmerIndex
 * order: subset order), a sequence of a part at most once.  The index equals wfm_index_build_sequences on the sequences
 * in that order.  Parts on h's own device are read where they lie; a part on another device comes over through a pinned
 * host buffer (device-to-host on its device, host-to-device on h's stream, in chunks, the two overlapped -- no copy
 * between the two devices' heaps).  A segmented gather (WFM_GATHER_TILE destination records per workgroup) then lays
 * the sequences' records end to end; one part on h's device whose named records already lie end to end is read in
 * place instead.  *n_windows (optional) = records of the union; when it is 0 no index is made and *out stays NULL.
 * (WFM_INDEX_STAGE_ALL=1, read per call: parts on h's own device take the staging path as well -- a test switch for
 * nodes with one GPU; WFM_INDEX_STAGE_CHUNK: records per staged chunk, 1024 .. 2^18, the default.) */
typedef struct { int32_t part; int32_t seq; } wfm_part_seq_t;
#define WFM_GATHER_TILE 2048
int  wfm_index_build_parts(wfm_handle_t* h, const wfm_minmer_part_t* const* parts, int nparts, const wfm_part_seq_t* order,
                           int64_t norder, double max_kmer_freq, wfm_index_t** out, int64_t* n_windows);

/* The k-mers of a sequence that wfm_add_minmers_multi lets its host workers see: valid k-mers whose hash
 * is under the threshold that lets c_factor * s of a window's w-k+1 k-mers through, plus every valid k-mer of a window that may hold
 * fewer than s distinct such hashes (wfmash_amd/csrc/map_prefilter.hip states the rule and why winnowing
 * the kept k-mers alone reproduces addMinmers).  pos / hash / strand receive up to cap kept k-mers in
 * ascending position; returns their number (may exceed cap) or a WFM_E_* code. */
int64_t wfm_prefilter_kmers(wfm_handle_t* h, const char* seq, int64_t len, int k, int w, int s, double c_factor,
                            uint32_t* pos, uint64_t* hash, int8_t* strand, int64_t cap);

/* The closing steps of addMinmers (commonFunc.hpp:660-706) on the device, on raw interval records in the order the
 * winnower emitted them (what wfm_add_minmers[_multi] runs after its winnowing kernel; wfmash_amd/csrc/map_finish.hip): records
 * with wpos == wpos_end or a negative bound go, strand tallies become signs, records of more than w windows are cut into
 * pieces, everything is ordered by (wpos, wpos_end) -- records that tie in the order libstdc++'s std::sort leaves them --
 * and consecutive records with equal (wpos, hash) are reduced to the first.  Returns the number of records (may exceed
 * cap; only cap are written) or a WFM_E_* code; *levels (optional) = recursion depth the order took, *heap_ranges
 * (optional) = ranges that spent introsort's depth budget and were heap-sorted by the library on the host. */
int64_t wfm_finish_records(wfm_handle_t* h, const wfm_minmer_t* raw, int64_t n, int w, wfm_minmer_t* out, int64_t cap,
                           int32_t* levels, int32_t* heap_ranges);

/* MinHash of one whole sequence for the ANI estimate (estimate_identity_for_groups,
 * src/map/include/map_stats.hpp:325-822; StreamingMinHash, streamingMinHash.hpp:35-135): the
 * sketch_size smallest canonical k-mer hashes, duplicates included, ascending.  Returns how many
 * were written (< sketch_size for short or N-rich sequences) or a WFM_E_* code. */
int64_t wfm_minhash_sketch(wfm_handle_t* h, const char* seq, int64_t len, int k, int sketch_size, uint64_t* out);
/* Between wfm_map_sequence_cache(h, 1) and wfm_map_sequence_cache(h, 0) the normalised device copy of every sequence of a megabase and more that
 * wfm_minhash_sketch / wfm_sketch_fragments / wfm_hash_kmers upload stays on its device (WFM_NORM_CACHE_GB, 16, at most per process), and a later
 * call of those or of wfm_index_build_sequences with the same host pointer, length and first / last 32 bytes uses it instead of uploading and
 * normalising again -- the identity estimate and the index of one map call read the same chromosomes (mashmap's main.cpp:72-128 then
 * computeMap.hpp:405-484: two passes over the files there too).  The caller keeps the host memory alive and unchanged while the scope is open;
 * scopes nest, the last close releases the copies.  wfmh_map_paf opens one around its whole call. */
int wfm_map_sequence_cache(wfm_handle_t* h, int open);

/* The shared-hash counts of many sketches at once: the pairwise merge of the ANI estimate (map_stats.hpp:719-731) for every
 * (row, column) pair of a matrix, on the device (wfmash_amd/csrc/map_isect.hip).
 * shared[r * n_cols + c] = the multiset intersection size of sketches rows[r] and cols[c]:
 * the sum over values v of min(count of v in A, count of v in B).  This is exactly what the
 * two-pointer merge of map_stats.hpp:719-731 counts on two ascending sketches with duplicates.
 * Sketches are given CSR-style: sketch i is hashes[offsets[i] .. offsets[i+1]), ascending,
 * duplicates allowed, and may be empty (offsets has n_sketches + 1 entries).  rows and cols name sketches by index, in any order,
 * repeats allowed.  A column sketch of up to WFM_ISECT_LDS_MAX hashes is searched in LDS, a longer one in global memory; the counts
 * do not depend on which.  The matrix is computed in launches of at most 64 M cells (WFM_ISECT_CELLS, read per call: another bound,
 * a test switch), so device memory is the sketches plus one such block whatever n_rows x n_cols is; the call returns with the
 * counts on the host.
 * WFM_E_ARG, with a message, nothing written to shared and the handle usable afterwards: offsets[0] != 0 or offsets that decrease,
 * a sketch of more than 2^32 - 1 hashes, an index outside [0, n_sketches), a sketch that does not ascend (found by a device pass
 * over hashes before any intersection runs; the message names the first such sketch).  n_rows == 0 or n_cols == 0: WFM_OK,
 * nothing is written. */
#define WFM_ISECT_LDS_MAX 4096   /* longest column sketch held in LDS; longer ones take the global-memory form */
int wfm_sketch_intersections(wfm_handle_t* h, const uint64_t* hashes, const int64_t* offsets, int64_t n_sketches,
                             const int32_t* rows, int64_t n_rows, const int32_t* cols, int64_t n_cols,
                             uint32_t* shared /* n_rows * n_cols, row-major */);

/* L1 stage: getSeedIntervalPoints + computeL1CandidateRegions + doL1Mapping's group loop
 * (mappingCore.hpp:82-301, computeMap.hpp:945-984) for a batch of query fragments against a
 * device-resident index.  One candidate = skch::L1_candidateLocus_t (base_types.hpp:212-224)
 * plus the fragment it belongs to; candidates come out grouped by fragment, in the reference's
 * order within a fragment. */
typedef struct {
  int32_t  seqId;
  int32_t  frag;              /* index of the query fragment in this call */
  int64_t  rangeStartPos;
  int64_t  rangeEndPos;
  int32_t  intersectionSize;
  int32_t  pad_;
} wfm_l1_candidate_t;

typedef struct {
  int32_t  window_length;          /* Parameters::windowLength (= segment length; fragments are exactly this long) */
  int32_t  sketch_size;            /* Parameters::sketchSize */
  int32_t  min_hits_cached;        /* cached_minimum_hits (computeMap.hpp:155-160) */
  int32_t  cached_segment_length;  /* cached_segment_length */
  int32_t  skip_self, skip_prefix, lower_triangular;
  int32_t  stage1_topANI_filter, stage2_full_scan;
  int32_t  n_seq;                  /* number of sequences known to the SequenceIdManager */
  const int32_t* ref_group;        /* [n_seq] idManager.getRefGroup(seqId) */
  const int32_t* min_hits_by_qsketch; /* [sketch_size+1] Stat::estimateMinimumHitsRelaxed(q, k, ANI) for the non-cached length */
  const int32_t* sketch_cutoffs;   /* [n_cutoffs] Stat::sketch_cutoffs table (computeMap.hpp:182-186) */
  int32_t  n_cutoffs;
  int32_t  pad_;
} wfm_l1_params_t;

/* qsketch: nfrag x s minmers (layout of wfm_sketch_fragments), qcount[f] of them valid.
 * q_active[f] == 0 skips a fragment (kmerComplexity below the threshold, computeMap.hpp:951).
 * Returns the number of candidates (may exceed cap; only cap are written) or a WFM_E_* code. */
int64_t wfm_map_l1(wfm_handle_t* h, const wfm_index_t* ix, const wfm_minmer_t* qsketch, const int32_t* qcount,
                   const int32_t* q_seq_id, const int32_t* q_len, const uint8_t* q_active, int64_t nfrag, int s,
                   const wfm_l1_params_t* prm, wfm_l1_candidate_t* out, int64_t cap);

/* L2 stage: doL2Mapping + computeL2MappedRegions + SlideMapper (computeMap.hpp:989-1061,
 * mappingCore.hpp:307-442, slidingMap.hpp:28-212) for a batch of L1 candidates.
 * One mapping = skch::MappingResult (base_types.hpp:154-165), 28 bytes. */
typedef struct {
  uint32_t refSeqId;
  uint32_t refStartPos;
  uint32_t queryStartPos;      /* 0: relative to the fragment; the caller adds fragmentIndex * windowLength (computeMap.hpp:124-128) */
  uint32_t blockLength;
  uint32_t n_merged;
  uint32_t conservedSketches;
  uint16_t nucIdentity;        /* x 1e4 */
  uint8_t  flags;              /* bit 0: reverse strand, bit 1: discard, bit 2: overlapped */
  uint8_t  kmerComplexity;     /* x 100 */
} wfm_mapping_t;

typedef struct {
  int32_t  window_length;
  int32_t  sketch_size;            /* Parameters::sketchSize = S; tables below are (S+1) x (S+1), index Q.sketchSize * (S+1) + shared */
  int32_t  stage1_topANI_filter;
  int32_t  pad_;
  const uint8_t*  keep_table;      /* identity test of computeMap.hpp:1018-1024 */
  const uint16_t* ident_table;     /* MappingResult::setNucIdentity(1 - j2md(shared / Q.sketchSize)) */
  const double*   cutoff_j;        /* [S+1] Jaccard cutoff of computeMap.hpp:1001-1004 per Q.sketchSize */
} wfm_l2_params_t;

/* q_kmer_complexity[f]: MappingResult::setKmerComplexity(Q.kmerComplexity) already scaled.
 * Mappings come out grouped by fragment, sorted by (refSeqId, refStartPos) within a fragment
 * (computeMap.hpp:920-921); out_frag[i] is the fragment of out[i].  Returns the number of
 * mappings (may exceed cap; only cap are written) or a WFM_E_* code. */
int64_t wfm_map_l2(wfm_handle_t* h, const wfm_index_t* ix, const wfm_minmer_t* qsketch, const int32_t* qcount,
                   const int32_t* q_len, const uint8_t* q_kmer_complexity, int64_t nfrag, int s,
                   const wfm_l1_candidate_t* cands, int64_t ncand, const wfm_l2_params_t* prm,
                   wfm_mapping_t* out, int32_t* out_frag, int64_t cap);

/* The fused per-batch map path: Map::mapSingleQueryFrag (computeMap.hpp:875-938) for nfrag
 * fragments of window_length bases each, fragment f = seq[frag_off[f] .. +window_length) belonging
 * to query sequence frag_seq_id[f].  Sketches, interval points and candidates never leave the
 * device.  Output as wfm_map_l2. */
typedef struct {
  int32_t  kmer_size;
  float    kmer_complexity_threshold;   /* Parameters::kmerComplexityThreshold (computeMap.hpp:951) */
  wfm_l1_params_t l1;
  wfm_l2_params_t l2;
} wfm_map_params_t;
int64_t wfm_map_fragments(wfm_handle_t* h, const wfm_index_t* ix, const char* seq, int64_t seq_len,
                          const int64_t* frag_off, const int32_t* frag_seq_id, int64_t nfrag,
                          const wfm_map_params_t* prm, wfm_mapping_t* out, int32_t* out_frag, int64_t cap);
/* The same, and the first step of the query's post-processing with it: mergeMappingsInRange[WithChains]
 * (mappingFilter.hpp:402-421, :593-612) begins by sorting a query's mappings by (target, strand, query position, target position);
 * the mappings are still on the device when L2 ends, so the batch is sorted there.  frag_first[f] = the first fragment of fragment f's
 * query (the caller adds (f - frag_first[f]) * window_length to queryStartPos: the key is made of that sum).  out_perm[i] = index into
 * out[] of the i-th mapping in (query, target, strand, query position, target position) order; out_perm[0] = 0xffffffff when two
 * mappings of a query share a key (std::sort leaves ties in an order of its own: the caller sorts as before) or the order could not
 * be made.  out / out_frag stay in fragment order, the order the reference's representative ids count in. */
int64_t wfm_map_fragments_ordered(wfm_handle_t* h, const wfm_index_t* ix, const char* seq, int64_t seq_len,
                                  const int64_t* frag_off, const int32_t* frag_seq_id, int64_t nfrag,
                                  const wfm_map_params_t* prm, wfm_mapping_t* out, int32_t* out_frag, int64_t cap,
                                  const int32_t* frag_first, uint32_t* out_perm);

/* --streaming-minhash (CommonFunc::sketchSequenceStreaming, commonFunc.hpp:338-430, as Sketch::buildHelper calls it for every
 * target sequence, winSketch.hpp:467-497): the target sketch taken from a per-sequence bottom-s MinHash instead of winnowed
 * minmers.  Of sequence i, the min(s, k-mers) smallest canonical hashes, duplicates included, of the k-mers free of non-ACGT bases
 * whose two strands hash differently; each becomes one record {hash, wpos = the first position of that hash among those k-mers,
 * wpos_end = wpos + w, seq_ids[i] (NULL: i), strand +1}, and a sequence's records are ordered by wpos.  Hashing and selection run
 * on the device.  out receives the records grouped by sequence in input order, counts[i] (optional) the number of sequence i.
 * Returns the total (may exceed cap; only cap are written) or a WFM_E_* code. */
int64_t wfm_streaming_minmers(wfm_handle_t* h, const char* const* seqs, const int64_t* lens, const int32_t* seq_ids, int64_t nseq,
                              int k, int w, int s, wfm_minmer_t* out, int64_t cap, int64_t* counts);

/* Sketch::build with --streaming-minhash: wfm_streaming_minmers followed by the index stage (wfm_index_build), the records going to the
 * device directly.  *n_windows (optional) receives the number of records; when it is 0 no index is made and *out stays NULL. */
int wfm_index_build_streaming(wfm_handle_t* h, const char* const* seqs, const int64_t* lens, const int32_t* seq_ids, int64_t nseq,
                              int k, int w, int s, double max_kmer_freq, wfm_index_t** out, int64_t* n_windows);

#ifdef __cplusplus
}
#endif
#endif
