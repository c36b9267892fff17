/*
 * include/wfmash_host.h -- file-level seam of the align phase (C ABI).
 *
 * wfmh_align_paf replaces align::Aligner::compute()
 * (src/align/include/computeAlignments.hpp:185,318-455): it reads a mapping PAF
 * (the hand-off file between the reference's map and align phases, `-i file.paf`,
 * src/interface/parse_args.hpp:800-804), fetches the sequence windows, runs the
 * wflign pipeline (BiWFA + head/tail patches + swizzle) on the GPU and writes the
 * aligned PAF.  Defaults equal the reference's (parse_args.hpp:290-294,566-620).
 */
#ifndef WFMASH_HOST_H_
#define WFMASH_HOST_H_

#include <stdint.h>
#include "wfmash_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int32_t  mismatch, gap_open1, gap_ext1, gap_open2, gap_ext2;  /* --wfa-params, default 5,8,2,24,1 */
  float    min_identity;            /* 0 */
  uint64_t min_alignment_length;    /* 32 */
  float    min_block_identity;      /* 0.1 */
  uint64_t target_padding;          /* min(w,5000) = 1000 */
  uint64_t query_padding;           /* min(w,5000) = 1000 */
  uint64_t wflign_max_len_minor;    /* 128 * w = 128000 */
  int32_t  disable_chain_patching;  /* 0 */
  int32_t  sam_format;              /* -a: SAM instead of PAF (parse_args.hpp:128) */
  int32_t  emit_md_tag;             /* -d: MD:Z tag in SAM records (parse_args.hpp:129) */
  int32_t  no_seq_in_sam;           /* 0 */
  int32_t  threads;                 /* -t: host threads for fetching sequences and for the CIGAR / PAF work of a
                                       batch (the reference runs one Taskflow worker per record); 0 = all cores */
  int32_t  resident_sequences;      /* --resident-seqs: 1 = whole sequences stay on the device (one wfm_seqstore_t per device, filled on
                                       first use up to WFM_SEQSTORE_GB, 32) and the problems name their windows by reference; the host
                                       fetches a PAF record's bases only where the swizzle reads them.  0 (default): every window is
                                       fetched on the host and uploaded -- the gain is unmeasured (profiles/resident_sequences.md) */
} wfmh_align_params_t;

typedef struct {
  uint64_t records;      /* "total aligned records" */
  uint64_t aligned_bp;   /* "total aligned bp" (sum of query spans; computeAlignments.hpp:451-454) */
  uint64_t written;      /* PAF lines written */
  uint64_t skipped;      /* invalid rows */
  uint64_t cells;        /* wavefront cells computed on the GPU */
  double   ms_gpu;       /* time during which an align kernel was running (union over the streams and over the handles the
                            driver's workers use; the busiest device of a multi-GPU run) */
  double   ms_total;
  /* host stages, summed over the batches (batches of different workers overlap: the sums may exceed ms_total) */
  double   ms_rows;      /* parsing the mapping rows */
  double   ms_fetch;     /* fetching, normalising and strand-adjusting the sequence windows */
  double   ms_wflign;    /* the wflign pipeline of a batch: device calls (upload, alignment, patches) and the work on runs between them */
  double   ms_text;      /* collecting the records' text */
  uint64_t batches;
  /* the tile kernels' share (wfa_tile2_kernel / wfa_tile_reg_kernel, the dominant kernels of the path): cells the result needs
   * (the block a job computes twice counted once), launches, and the sum of the launches' durations -- launches of several
   * workers overlap, so the sum is an upper bound of the time the kernel had the device to itself */
  uint64_t cells_tile;
  uint64_t tile_launches;
  double   ms_tile;
  double   ms_tags;      /* WFM_RECORD_TAGS (a diagnostic channel of the parity tests and bench.py): writing the records' tags, summed over the batches */
  /* resident_sequences (both 0 without it) */
  uint64_t records_resident;  /* records whose two sides both came from the device's sequence store */
  uint64_t lazy_fetches;      /* of those, the ones whose bases the host fetched after all (a CIGAR that begins =,D or ends D,=) */
} wfmh_align_summary_t;

void wfmh_align_default_params(wfmh_align_params_t* p);

/* query_fasta may be NULL (= target_fasta, all-vs-all).  Returns 0 or WFM_E_*;
 * messages go to stderr and wfm_last_error(h). */
int wfmh_align_paf(wfm_handle_t* h, const char* target_fasta, const char* query_fasta,
                   const char* mapping_paf, const char* out_paf,
                   const wfmh_align_params_t* params, wfmh_align_summary_t* summary);

/* The same over n GPUs of one node (handles[i] from wfm_create(device_i)): batches of mapping records go to whichever
 * device is free (records are independent, computeAlignments.hpp:398-435; the split the reference's cluster script
 * makes ahead of time, scripts/split_approx_mappings_in_chunks.py:19-27,47, is made at run time), the output is
 * written in input order and does not depend on n.  Errors are reported on handles[0]. */
int wfmh_align_paf_multi(wfm_handle_t* const* handles, int n, const char* target_fasta, const char* query_fasta,
                         const char* mapping_paf, const char* out_paf,
                         const wfmh_align_params_t* params, wfmh_align_summary_t* summary);

/* ---- every aligned PAF line held against the bases it names (wfmash_amd/host/verify_paf.hpp) ----
 * A finished line is parsed on its own -- names, qs, qe, strand, ts, te as written, cg:Z: -- and becomes a problem by reference:
 * pattern = target [ts, te), text = query [qs, qe) (reverse-complemented for '-'), both normalised as every window the driver
 * fetches; the CIGAR becomes runs (= M, X X, I I, D D) and batches of lines go through wfm_upload_sequence_refs and
 * wfm_check_runs (wfmash_hip.h), by store id where the run keeps its sequences on the device (resident_sequences), by host
 * pointer otherwise.  A line without cg:Z: or with an op outside =XID (a plain M) is counted as unverifiable, not as failed.
 * What is checked: spans, run structure, every M and X base.  What is not: optimality (wfmh_set_verify_optimal, below).
 *
 * wfmh_set_verify(1): from now on every wfmh_align_paf[_multi] call of the process verifies each batch's finished lines -- what
 * the user gets after patching, erosion and swizzle -- before they are written; the output bytes do not change, a failure is
 * one line on stderr (query, target, coordinates, flag names, first offending position), SAM output is not verified.  Every
 * call of wfmh_set_verify zeroes the counts.  wfmh_verify_counts: out = {lines checked, failed, unverifiable, bases compared}
 * since then.  wfmh_verify_paf: the same check on an existing aligned PAF (this build's or the reference's), no mapping and no
 * alignment; query_fasta may be NULL (= target_fasta); out as above, for this call alone.  Returns 0 or WFM_E_*. */
void wfmh_set_verify(int on);
int  wfmh_verify_counts(uint64_t out[4]);
int  wfmh_verify_paf(wfm_handle_t* h, const char* target_fasta, const char* query_fasta, const char* aligned_paf, uint64_t out[4]);
/* Test hook (no GPU): a line as the verifier reads it -- "ok", qname, qs, qe, strand, tname, ts, te and the runs spelled back as
 * a CIGAR over =XID, separated by tabs; or "unverifiable" / "malformed" and the reason.  Release with wfmh_free. */
char* wfmh_test_verify_parse(const char* line);

/* ---- every score of the align driver proved optimal (wfm_check_optimal, wfmash_hip.h) ----
 * wfmh_set_verify_optimal(1, max_cells): from now on every device call of the align driver -- main BiWFA problems, head and tail
 * patches, late tails -- runs as upload, wfm_align_resident_rle, wfm_check_optimal, free instead of the one-call forms, and every
 * score it returns is held against a banded DP of the same two byte strings on the device.  The output bytes do not change.  A
 * failed problem is one line on stderr: "[wfmash::verify] NOT OPTIMAL" (a cheaper alignment exists) or "UNREACHED" (no alignment of
 * that price exists), the record's names and coordinates, which of its problems it is, the mode, the claimed and the DP score.
 * max_cells caps the DP cells of one problem (0: no cap); a problem beyond it is counted as skipped.  Every call zeroes the counts.
 * wfmh_verify_optimal_counts: out = {problems checked (the skipped among them), failed, skipped, DP cells computed} since then.
 * What is not proved: that the CIGAR is the reference's choice among co-optimal ones, or that the host's surgery on it (patching,
 * erosion, swizzle) is right -- wfmh_set_verify covers the latter.  Off by default; with the switch off nothing new runs. */
void wfmh_set_verify_optimal(int on, uint64_t max_cells);
int  wfmh_verify_optimal_counts(uint64_t out[4]);

/* ---- every interior gap of the records' final CIGARs at its leftmost placement (wfm_left_align_runs, wfmash_hip.h) ----
 * wfmh_set_left_align(1): from now on every batch of wfmh_align_paf[_multi] runs ONE more device call between the swizzle and the record
 * writers: the runs each record's line will spell (its final ops without the leading and trailing gaps the writers strip) against the
 * sub-windows they cover, by reference where the run keeps its sequences on the device.  Only cg:Z: changes in a PAF line, only CIGAR
 * and MD in a SAM record; wfmh_set_verify then checks the normalised lines.  A record whose runs do not span its windows is written as
 * it is and counted as left alone (the pipeline produces none).  Every call zeroes the counts.  wfmh_left_align_counts: out = {records
 * handed to the device, their interior gaps, gaps moved, records left alone} since then.  Off by default; with the switch off the
 * swizzle and the writers run back to back as ever, nothing new is called and the counts stay 0. */
void wfmh_set_left_align(int on);
int  wfmh_left_align_counts(uint64_t out[4]);

/* ---- minimap2's cs:Z: tag on every record written (wfm_cs_strings, wfmash_hip.h) ----
 * wfmh_set_cs(form), form 0 off, 1 short, 2 long: from now on every batch of wfmh_align_paf[_multi] runs ONE more device call between the
 * swizzle (and the left-align call, where that switch is on) and the record writers: the cs string of the runs each record's line will
 * spell against the sub-windows they cover, by reference where the run keeps its sequences on the device -- the host never needs a
 * record's bases for it.  With wfmh_set_left_align as well the windows are uploaded once for both calls and the string is that of the
 * normalised runs.  "\tcs:Z:" + the string becomes the last field of the PAF line or the SAM record; nothing else of the line changes.
 * A record whose runs do not span its windows is written without the field and counted (the pipeline produces none).  Every call
 * zeroes the counts.  wfmh_cs_counts: out = {records written with a string, bytes of those strings, records written without one, 0}
 * since then.  Off by default; with the switch off nothing new is called and the output bytes are what they always were. */
void wfmh_set_cs(int form);
int  wfmh_cs_counts(uint64_t out[4]);

/* ---- the variants of every record written, as a VCF (wfm_call_variants, wfmash_hip.h) ----
 * wfmh_set_variants(path): from now on every batch of wfmh_align_paf[_multi] runs ONE more device call between the swizzle (and the
 * left-align and cs calls, where those switches are on) and the record writers: the SNVs, insertions and deletions of the runs each
 * record's line will spell, alleles included, against the sub-windows they cover -- by reference where the run keeps its sequences on the
 * device, so the host never needs a record's bases.  The windows are uploaded once whichever of the three switches are on, and with
 * wfmh_set_left_align the variants are those of the normalised runs.  No output byte of the PAF or SAM changes.  The align phase writes
 * `path`: the header (##fileformat=VCFv4.2, ##source, one ##contig per sequence of the target index in index order, the ##INFO lines of
 * QNAME, QSTART, QEND and QSTRAND, #CHROM .. INFO: no sample columns), then the lines of every record written, in the order of the
 * records whatever the number of devices, within a record in ascending POS: POS = the record's target start + p + 1; ID, QUAL and
 * FILTER are '.'; alleles on the target's strand; [QSTART, QEND) = the 0-based forward-strand span of the query bases in ALT (one base
 * for an SNV, the inserted bases for an insertion, empty at the junction for a deletion).  The file is not sorted across records.  SNVs
 * with a base outside ACGT are left out and counted; a record whose runs do not span its windows has no lines and is counted as left
 * alone (the pipeline produces none).  NULL or "" switches it off.  Every call zeroes the counts.  wfmh_variants_counts: out = {records
 * called, variants written, SNVs masked, records left alone} since then.  Off by default; with the switch off nothing new is called
 * and no file is written. */
void wfmh_set_variants(const char* path_or_null);
int  wfmh_variants_counts(uint64_t out[4]);

/* ---- per-base depth of the target from the records written, as a bedGraph (wfm_coverage_*, wfmash_hip.h) ----
 * wfmh_set_coverage(path): from now on every batch of wfmh_align_paf[_multi] runs ONE more device call behind the record writers: the
 * runs of every record WRITTEN -- a record the filters drop adds nothing; with wfmh_set_left_align the normalised runs -- are added to a
 * depth object of the batch's handle (4 bytes per target base on each handle the run uses, made at the handle's first batch; refused
 * beyond WFM_COV_GB GiB, 32).  depth(c, x) = the number of written records whose line has an = or X base at x of target sequence c: D
 * bases do not count.  No output byte of the PAF or SAM changes.  After the last batch the objects are merged into one and the align
 * phase writes `path`: plain bedGraph without a track line, name<TAB>start<TAB>end<TAB>depth, the target's sequences in index order, per
 * sequence the maximal intervals of constant depth tiling [0, length) exactly, depth 0 included; a sequence without an alignment is one
 * line of depth 0.  The file does not depend on the number of devices, handles, threads or the order of the batches.  NULL or ""
 * switches it off.  Every call zeroes the counts.  wfmh_coverage_counts: out = {records added, target bases with depth >= 1, sum of
 * depth, intervals written} since then; the sum of depth is the total of the = and X run lengths of the lines written.  Off by
 * default; with the switch off nothing new is called and no file is written.
 * wfmh_coverage_paf: the same file for an existing aligned PAF (this build's, the reference's, minimap2 -c --eqx's); nothing else
 * runs.  A line without cg:Z: or with an op outside =XID, a malformed line, a line whose target the file does not have or whose tlen is
 * not the file's is skipped and counted; one line on stderr has the totals.  out = {lines added, lines skipped, covered bases, sum of
 * depth}.  Returns 0 or WFM_E_*. */
void wfmh_set_coverage(const char* path_or_null);
int  wfmh_coverage_counts(uint64_t out[4]);
int  wfmh_coverage_paf(wfm_handle_t* h, const char* target_fasta, const char* aligned_paf, const char* out_path, uint64_t out[4]);
/* Test hook (no GPU): the bedGraph of n_iv intervals of constant depth over the concatenation of n_seq sequences (starts ascending;
 * the first at 0, or depth 0 before it), exactly as the align phase writes it.  malloc'd, wfmh_free. */
char* wfmh_test_coverage_bedgraph(const char* const* names, const uint64_t* lengths, int n_seq, const uint64_t* starts, const uint32_t* depths,
                                  int64_t n_iv);

/* ---- target intervals lifted through the records written (wfm_liftset_*, wfm_lift_runs, wfmash_hip.h) ----
 * wfmh_set_lift(bed, out): from now on every batch of wfmh_align_paf[_multi] runs ONE more device call behind the record writers: the
 * intervals of the BED file `bed` -- positions on the target's sequences -- are lifted through the runs of every record WRITTEN (a
 * record the filters drop has no lines; with wfmh_set_left_align the normalised runs).  The BED is read once per run and uploaded once
 * per handle, at the handle's first batch; nothing else goes up but runs.  No output byte of the PAF or SAM changes.  The align phase
 * writes `out` through an ordered writer, in the order of the PAF's records and per record in ascending (start, end, input order) of the
 * intervals: the file does not depend on the number of devices, handles, threads or the order of the batches.
 * BED: tab-separated, three columns at least, column 4 the name ("." without one).  Skipped and counted: blank lines, lines that begin
 * with '#', `track` and `browser` lines, fewer than three columns, a start or end that is not a plain decimal, a sequence the target
 * does not have, start >= end, end beyond the sequence.
 * One line per (record, overlapping interval), 14 tab-separated columns, no header:
 *   qname qstart qend name strand tname tstart tend istart iend eq x ins del
 * [tstart, tend): the part actually lifted, on the target sequence; [istart, iend): the input interval; [qstart, qend): where it lies on
 * the query's forward strand; eq / x / ins / del: the = columns, X columns, inserted and deleted bases between the lifted ends.  An
 * interval that lies in a deletion has qstart == qend, tstart == tend and eq = x = 0: present in the target, absent from the query.
 * Either path NULL or "" switches it off.  Every call zeroes the counts.  wfmh_lift_counts: out = {records lifted, lines written, empty
 * lifts, BED lines skipped} since then.  Off by default; with the switch off nothing new is called and no file is written.
 * wfmh_lift_paf: the same file for an existing aligned PAF (this build's, the reference's, minimap2 -c --eqx's); nothing else runs.
 * Lines are read and skipped exactly as wfmh_coverage_paf does; one line on stderr has the totals.  out = the same four counts.
 * Returns 0 or WFM_E_*. */
void wfmh_set_lift(const char* bed_path_or_null, const char* out_path_or_null);
int  wfmh_lift_counts(uint64_t out[4]);
int  wfmh_lift_paf(wfm_handle_t* h, const char* target_fasta, const char* aligned_paf, const char* bed_path, const char* out_path, uint64_t out[4]);
/* ---- UCSC chain files from the records written (wfm_chain_runs, wfmash_hip.h) ----
 * wfmh_set_chain(path, swap): from now on every batch of wfmh_align_paf[_multi] runs ONE more device call behind the record writers: the
 * runs of every record WRITTEN, on the part of the ops its line spells (with wfmh_set_left_align the normalised runs), are compacted to
 * the blocks and gaps of a chain on the device; nothing goes up but runs.  No output byte of the PAF or SAM changes.  The align phase
 * writes `path` through an ordered writer, one chain per record in the order of the PAF's records, and the writer numbers the chains
 * 1, 2, 3 ... as it writes them: the file does not depend on the number of devices, handles, threads or the order of the batches.  A
 * record the filters drop has no chain; a record the device refuses has none, is counted and reported on stderr.
 * A chain: the header "chain score tName tSize + tStart tEnd qName qSize qStrand qStart qEnd id", space-separated; one line
 * "size<TAB>dt<TAB>dq" per block, the last block's `size` alone; one empty line.  The chain runs from the target to the query (what
 * liftOver, CrossMap and bcftools +liftover take to carry target positions to the query): [tStart, tEnd) is the target span the line's
 * runs spell, [qStart, qEnd) the query span on +, and on - [qSize - qEnd, qSize - qStart) of the PAF's forward coordinates: the chain
 * format counts a - side on the reverse strand.  score = the record's = columns: an integer that ranks longer and more identical chains
 * first, which is all liftOver uses it for; it is not blastz's score.
 * swap != 0 writes what chainSwap makes of that file, to lift the other way: the PAF query is the first side, always + with its forward
 * coordinates, the PAF target the second side with the record's strand, on - at [tSize - tEnd, tSize - tStart); every (dt, dq) changes
 * places and the blocks of a - record run from the last to the first (WFM_CHAIN_SWAP on every record, WFM_CHAIN_REVERSE on the - ones).
 * path NULL or "" switches it off.  Every call zeroes the counts.  wfmh_chain_counts: out = {chains written, blocks, records refused, 0}
 * since then.  Off by default; with the switch off nothing new is called and no file is written.
 * wfmh_chain_paf: the same file for an existing aligned PAF (this build's, the reference's, minimap2 -c --eqx's); nothing else runs.
 * Lines are read and skipped exactly as wfmh_coverage_paf does, the query's name and length are the line's; a cg:Z: that begins or ends
 * with I or D runs moves the chain's ends inward by them.  One line on stderr has the totals.  out = the same four counts.  Returns 0 or
 * WFM_E_*. */
void wfmh_set_chain(const char* path_or_null, int swap);
int  wfmh_chain_counts(uint64_t out[4]);
int  wfmh_chain_paf(wfm_handle_t* h, const char* target_fasta, const char* aligned_paf, const char* out_path, int swap, uint64_t out[4]);
/* ---- the aligned sequences of the records written, as pairwise MAF blocks (wfm_maf_rows, wfmash_hip.h) ----
 * wfmh_set_maf(path, split): from now on every batch of wfmh_align_paf[_multi] runs ONE more device call between the swizzle (and the
 * left-alignment, the cs strings and the variants, where they are on: the windows are uploaded once for all of them) and the record
 * writers: the two gapped rows of every record's runs, on the part of the ops its line spells (with wfmh_set_left_align the normalised
 * runs), are spelled on the device in blocks -- one per record with split = 0, cut at every gap stretch of split or more gap bases
 * otherwise (the stretch's columns are not written).  No output byte of the PAF or SAM changes.  The align phase writes `path` through an
 * ordered writer in the order of the PAF's records: the file does not depend on the number of devices, handles, threads or the order of
 * the batches.  A record the filters drop has no blocks; a record the device flags has none and is counted.
 * The file: "##maf version=1", then per block "a score=<eq>", "s <tname> <tstart> <psize> + <tlen> <row P>",
 * "s <qname> <qstart> <tsize> <+|-> <qlen> <row T>" and one empty line; single spaces, no column padding (readers split on whitespace).
 * score = the block's = columns (--chain's quantity, not a blastz score); tstart = the line's target start + p; qstart = the line's query
 * start + t on +, and qlen - the line's query end + t on -: MAF counts a - row on the reverse-complemented source, whose strand row T is.
 * path NULL or "" switches it off.  Every call zeroes the counts.  wfmh_maf_counts: out = {records written with blocks, blocks, columns,
 * records left without blocks} since then.  Off by default; with the switch off nothing new is called and no file is written.
 * wfmh_maf_paf: the same file for an existing aligned PAF; nothing else runs.  Lines are parsed as wfmh_verify_paf parses them and their
 * windows uploaded as it uploads them; a line without an =XID cg:Z:, a malformed one, one whose sequence its file does not have or has
 * with another length is skipped and counted.  As in wfmh_verify_paf, a line's target name is looked up in target_fasta and its query
 * name in query_fasta (target_fasta where that is NULL): with two files, a query that only the target file has counts as unknown.  A cg:Z: that begins or ends with I or D runs is spelled as it is (its first or last block then
 * begins or ends with gap columns).  One line on stderr has the totals.  out = the same four counts.  Returns 0 or WFM_E_*. */
void wfmh_set_maf(const char* path_or_null, uint32_t split);
int  wfmh_maf_counts(uint64_t out[4]);
int  wfmh_maf_paf(wfm_handle_t* h, const char* target_fasta, const char* query_fasta_or_null, const char* aligned_paf, const char* out_path, uint32_t split,
                  uint64_t out[4]);
/* Test hook (no GPU): the text side alone (chain_text.hpp).  spec: lines "R<TAB>qname<TAB>qsize<TAB>qs<TAB>qe<TAB>strand<TAB>tname<TAB>tsize
 * <TAB>ts<TAB>te<TAB>eq<TAB>lead_dt<TAB>lead_dq<TAB>trail_dt<TAB>trail_dq" (a record as its PAF line has it, and what wfm_chain_runs says of
 * its problem beside the blocks) each followed by its blocks "B<TAB>size<TAB>dt<TAB>dq" as the device gives them.  flags_out (or NULL):
 * per R line the flags its problem carries under `swap`.  Returns the chain file exactly as the align phase writes it, ids from 1; NULL
 * for a spec it cannot read.  malloc'd, wfmh_free. */
char* wfmh_test_chain_lines(const char* spec, int swap, uint32_t* flags_out);
/* ---- single-coverage chain files: a net across the records written (wfm_net_*, wfmash_hip.h) ----
 * wfmh_set_chain_net(path): from now on every batch of wfmh_align_paf[_multi] runs ONE more device call behind the record writers
 * (beside wfmh_set_chain's, with or without it): the runs of every record WRITTEN go to the net object of the batch's handle with
 * score = the record's = columns and order = batch number << 32 | the record's index among the batch's records packed.  No output byte
 * of the PAF, the SAM or the --chain file changes.  Once all batches are aligned the objects of the handles are merged into the first
 * (export, import), the net is taken once on the device, and `path` is written: in the order of the PAF's records, ids 1, 2, 3 ..., one
 * chain per record that won at least one target base, from the PIECES the net left it -- every target base lies under at most one chain,
 * the chain of the record with the most = columns over it (the earlier record where they are equal).  A chain: the header of
 * wfmh_set_chain's file with score = the score the record competed with, tStart = the first piece's start, tEnd = the last piece's end,
 * qStart and qEnd from the first and last pieces on the record's strand; one line "size<TAB>dt<TAB>dq" per piece with the distances to
 * the next piece on both sides, both of which may be non-zero, the last piece's `size` alone; one empty line.  A record that won nothing
 * has no chain and is counted.  The file does not depend on the number of devices, handles, threads or the order of the batches.  Not
 * here: chainNet's thresholds and levels, a .net file, joining records into one chain, single coverage on the query side (a swapped net).
 * path NULL or "" switches it off.  Every call zeroes the counts.  wfmh_chain_net_counts: out = {records added, chains written, pieces,
 * records that won nothing} since then.  Off by default; with the switch off nothing new is called and no file is written.
 * wfmh_chain_net_paf: the same file for an existing aligned PAF, lines read and skipped as wfmh_chain_paf does, order = the number of the
 * line among those taken; nothing else runs.  out = the same four counts.  Returns 0 or WFM_E_*. */
void wfmh_set_chain_net(const char* path_or_null);
int  wfmh_chain_net_counts(uint64_t out[4]);
int  wfmh_chain_net_paf(wfm_handle_t* h, const char* target_fasta, const char* aligned_paf, const char* out_path, uint64_t out[4]);
/* Test hook (no GPU): the text side alone (chain_text.hpp's net_body).  spec: lines "R<TAB>qname<TAB>qsize<TAB>qs<TAB>qe<TAB>strand<TAB>tname
 * <TAB>tsize<TAB>t_offset<TAB>score" (a record as its PAF line has it, where its target sequence begins in the concatenation, the score it
 * competed with) each followed by its pieces "P<TAB>t<TAB>q<TAB>size" as wfm_net_table gives them (t global).  Returns the file exactly as
 * the align phase writes it, ids from 1; NULL for a spec it cannot read.  malloc'd, wfmh_free. */
char* wfmh_test_chain_net_lines(const char* spec);
/* ---- transitive lifts: seed intervals closed over all records written, both ways (wfm_trans_*, wfmash_hip.h) ----
 * wfmh_set_transitive(bed, out, depth): from now on every batch of wfmh_align_paf[_multi] runs ONE more device call behind the record
 * writers: the runs of every record WRITTEN (with wfmh_set_left_align the normalised runs) go to the trans object of the batch's handle,
 * each with its two places in the WORLD: the target's sequences in index order, then the query's sequences whose names no target has, in
 * query index order.  No output byte of the PAF, the SAM or another side file changes.  Once all batches are aligned the objects of the
 * handles are merged into the first (export, import), the closure of the BED's intervals is taken once on the device at `depth` (0: to
 * the fixed point; the CLI's default is 2) and `out` is written, tab-separated: "seq start end name seed_seq seed_start seed_end", sorted
 * by (seed in input order, world start), an interval that crosses from one sequence into the next split there, the seed's own interval
 * among them.  The BED is read as wfmh_set_lift's, names looked up in the world.  The file does not depend on the number of devices,
 * handles, threads or the order of the batches.  Not here: a minimum length or identity of a hop, the depth or path of an interval, the
 * query strand of a result, gzip, more than 2^24 - 1 seeds.  bed or out NULL or "" switches it off.  Every call zeroes the counts.
 * wfmh_transitive_counts: out = {records added, lines written, rounds run, BED lines skipped} since then.  Off by default; with the
 * switch off nothing new is called and no file is written.
 * wfmh_transitive_paf: the same file for an existing aligned PAF, lines read and skipped as wfmh_coverage_paf does; a line whose query
 * neither FASTA has (or whose query window leaves its sequence) is skipped and counted, as wfmh_pav_paf does; nothing else runs.  out =
 * the same four counts.  Returns 0 or WFM_E_*. */
void wfmh_set_transitive(const char* bed_path_or_null, const char* out_path_or_null, uint32_t depth);
int  wfmh_transitive_counts(uint64_t out[4]);
int  wfmh_transitive_paf(wfm_handle_t* h, const char* target_fasta, const char* query_fasta_or_null, const char* aligned_paf, const char* bed_path,
                         const char* out_path, uint32_t depth, uint64_t out[4]);
/* Test hook (no GPU): the text side alone (transitive_text.hpp).  The world of the n_t target and n_q query sequences, what the parser
 * makes of `bed` in it ("#skipped" and "#iv" lines as wfmh_test_lift_lines spells them, in input order), and per line "I<TAB>seed<TAB>a
 * <TAB>b" of spec (a world interval of that seed) the file's lines.  NULL for a spec it cannot read.  malloc'd, wfmh_free. */
char* wfmh_test_transitive_lines(const char* const* tnames, const uint64_t* tlengths, int n_t, const char* const* qnames, const uint64_t* qlengths,
                                 int n_q, const char* bed, const char* spec);

/* ---- presence of target intervals per group of query sequences (wfm_pav_*, wfmash_hip.h) ----
 * wfmh_set_pav(bed, window, out): from now on every batch of wfmh_align_paf[_multi] runs ONE more device call behind the record writers:
 * the runs of every record WRITTEN (with wfmh_set_left_align the normalised runs) go into the handle's presence object under the column
 * of the query sequence's group.  Once the workers are done the objects of the handles are merged (export, import: a union of unions),
 * the table is taken once on the device and `out` is written: pav(j, g) = the bases of interval j under an = or X base of at least one
 * record written whose query belongs to group g.  D bases do not count.  No output byte of the PAF or SAM changes, and the file does not
 * depend on the number of devices, handles, threads or the order of the batches.
 * Groups: a query name's key is the part before its LAST '#', else the whole name; the columns are the distinct keys of ALL sequences of
 * the query FASTA, sorted bytewise; a group without a written record is a column of zeros.  The target's own group is a column like the
 * others: where the mapper skips self or same-group mappings it is 0.
 * Intervals: `bed` (read and skipped as wfmh_set_lift reads it, sorted by (global start, end, input order)), or window > 0: windows of
 * that many bases tiling every target sequence in index order, the last one shorter, named ".".  Exactly one of the two; anything else,
 * or no `out`, switches it off.
 * File: "#tname tstart tend name len" and the group keys, tab-separated, then one row per interval; cells are covered bases.
 * Every call zeroes the counts.  wfmh_pav_counts: out = {records added, rows written, union intervals, BED lines skipped} since then.
 * wfmh_pav_paf: the same file for an existing aligned PAF; query_fasta NULL or "": the target's sequences are the queries too.  Lines
 * are read and skipped exactly as wfmh_coverage_paf does; a line whose query is not in the query FASTA is skipped and counted; one line
 * on stderr has the totals.  out = the same four counts.  Returns 0 or WFM_E_*. */
void wfmh_set_pav(const char* bed_path_or_null, uint64_t window, const char* out_path_or_null);
int  wfmh_pav_counts(uint64_t out[4]);
int  wfmh_pav_paf(wfm_handle_t* h, const char* target_fasta, const char* query_fasta_or_null, const char* aligned_paf, const char* bed_path_or_null,
                  uint64_t window, const char* out_path, uint64_t out[4]);
/* ---- one sorted VCF of all records' variants with a haploid genotype per group of query sequences (wfm_sites_*, wfmash_hip.h) ----
 * wfmh_set_genotypes(path): from now on every batch of wfmh_align_paf[_multi] calls the variants of its records (as wfmh_set_variants does,
 * whether that switch is on or not: its file and counts do not change) and, behind the record writers, adds those of every record WRITTEN
 * -- masked SNVs left out, positions global, the group of the query sequence as wfmh_set_pav has it -- and the same records' runs to the
 * handle's sites object: two device calls per batch.  With wfmh_set_left_align they are the normalised runs' (give both: otherwise one
 * indel in a repeat can be two sites).  Once the workers are done the objects of the handles are merged (export, import), the table is
 * taken once on the device and `path` is written: --variants' header, AC and AN, FORMAT GT, the columns #CHROM .. INFO FORMAT and the
 * group keys, then one line per distinct site, "CHROM POS . REF ALT . . AC=a;AN=n GT" and one cell per group ('1' carried, '0' the REF
 * span under = bases of the group, '.' neither), sorted by (target sequence in index order, POS, REF bytes, ALT bytes).  The file is a set
 * function of the records written: it does not depend on the number of devices, handles, threads or the order of the batches.  NULL or ""
 * switches it off.  Every call zeroes the counts.
 * wfmh_genotypes_counts: out = {records added, sites written, variants merged away (variants added - sites), records left alone}. */
void wfmh_set_genotypes(const char* path_or_null);
int  wfmh_genotypes_counts(uint64_t out[4]);
/* Test hook (no GPU): the text side alone (genotype_text.hpp).  tnames / lengths: the n_t target sequences; keys: the n_groups columns;
 * sites: n_sites x {pos, ref_len, alt_len, off} as four uint64 each, pos global, in ascending pos; alleles: their bytes; gt: n_sites x
 * n_groups cells.  Returns the header and the lines in file order: malloc'd, wfmh_free. */
char* wfmh_test_genotype_text(const char* version, const char* const* tnames, const uint64_t* lengths, int n_t, const char* const* keys, int n_groups,
                              const uint64_t* sites, size_t n_sites, const char* alleles, const char* gt);

/* Test hook (no GPU): the text side alone (pav_text.hpp).  names: n_q query names; lengths: n_t target lengths; window: --pav-window's.
 * Returns "#key<TAB>name<TAB>key<TAB>column" per name, the header line, then one row per window with cell g = (row number + g): malloc'd,
 * wfmh_free. */
char* wfmh_test_pav_text(const char* const* names, int n_q, const char* const* tnames, const uint64_t* lengths, int n_t, uint64_t window);

/* Test hook (no GPU): the text side alone.  bed: the text of a BED file over n_seq target sequences; spec: lines "R<TAB>qname<TAB>qs
 * <TAB>qe<TAB>strand<TAB>tname<TAB>ts" (a record as its PAF line has it) and "L<TAB>record<TAB>interval<TAB>p0<TAB>p1<TAB>t0<TAB>t1<TAB>eq
 * <TAB>x" (a lift of record number `record` and interval number `interval` of the sorted list, as wfm_lift_runs gives it).  Returns
 * "#skipped<TAB>n", one "#iv<TAB>seq<TAB>start<TAB>end<TAB>name<TAB>input order<TAB>global start<TAB>global end" per interval kept, in
 * sorted order, then the L lines' lines of the lift file exactly as the align phase writes them; NULL for a spec it cannot read.
 * malloc'd, wfmh_free. */
char* wfmh_test_lift_lines(const char* const* names, const uint64_t* lengths, int n_seq, const char* bed, const char* spec);

/* Test hooks: the pure host-side CIGAR functions (erode / merge / swizzle / PAF writer /
 * parseMashmapRow) behind one string interface so the CPU test-suite can check them
 * without a GPU.  fn in {erode, merge, compress, swap_start, swap_end, head_erosion,
 * tail_erosion, paf, parse_row}.  The result is malloc'd; release with wfmh_free. */
char* wfmh_test_cigar(const char* fn, const char* a, const char* b, const char* query, const char* target,
                      long long i0, long long i1);
void  wfmh_free(char* p);
/* Test hook of the align driver's sub-window translation (resident_sequences): [a, b) of a side that is the window
 * [win_start, win_end) of a stored sequence -- reverse-complemented when rev -- as the forward window [*out_start, *out_end). */
void  wfmh_test_subwindow(int64_t win_start, int64_t win_end, int rev, int64_t a, int64_t b, int64_t* out_start, int64_t* out_end);
/* Test hooks of the tile phase's, phase 2's and the base jobs' planning (csrc/wfa_rows.h, csrc/wfa_plan.h; pure arithmetic, no GPU):
 * the layouts of their arguments are described at their definitions (host/capi_host.cpp) and wrapped by tests/test_tile_plan_cpu.py. */
int wfmh_test_rows(const int32_t* q, int64_t n, int64_t* out);
int wfmh_test_tile_plan(const int32_t* jobs, int64_t n, const int32_t* rules, int32_t* per_block, int32_t* tasks, int64_t tasks_cap, int64_t* scalars);
int wfmh_test_p2_plan(const int32_t* cand, int64_t n, int64_t i0, int rows, int rows_bm, unsigned long long budget, int threads, int core, int64_t* geo,
                      int32_t* tasks, int64_t tasks_cap, int64_t* scalars);
int wfmh_test_base_plan(int op, const int32_t* in, int64_t n, int32_t* out);
/* ... and of parent reuse (csrc/wfa_plan.h): which keep a child resumes from, whether it may, the cadence under the store's cap; the tile plan
 * with a direction mask per job (wrapped by tests/test_reuse_plan_cpu.py) */
int wfmh_test_reuse_plan(int op, const int64_t* in, int64_t n, int64_t* out);
int wfmh_test_planned_meet(const int64_t* in, int64_t n, int64_t* out);
int wfmh_test_tile_plan_dirs(const int32_t* jobs, int64_t n, const int32_t* rules, const uint8_t* dirs, int32_t* per_block, int32_t* tasks, int64_t tasks_cap,
                             int64_t* scalars);
/* ... and of the packed tile kernel's lean snapshot paths (csrc/wfa_rows.h): rng_interior against one query of (pl, tl, sub, first diagonal, last
 * diagonal, first score, last score) each, and the waves of one block of a job that pass the kernel's two wave tests (wrapped by
 * tests/test_tile_interior_cpu.py and tests/test_tile_lean_gpu.py) */
int wfmh_test_tile_interior(const int32_t* q, int64_t n, int32_t* out);
int wfmh_test_tile_lean_waves(const int32_t* in, int64_t* out);
/* ... and the band of wfm_check_optimal (csrc/wfa_optband.h; wrapped by tests/test_optcheck_cpu.py): in = {x, o1, e1, o2, e2, plen, tlen,
 * pbf, pef, tbf, tef, S}, out = {band_lo, band_hi, cells} */
int wfmh_test_opt_band(const int64_t* in, int64_t* out);
/* host winnowing stage of wfm_add_minmers on caller-supplied canonical k-mer hashes (CPU tests) */
int64_t wfmh_test_winnow(const char* seq, int64_t len, int k, int w, int s, int32_t seq_id,
                         const uint64_t* hash, const int8_t* strand, wfm_minmer_t* out, int64_t cap);

/* the same through speculative chunks of chunk_len k-mers (how wfm_add_minmers_multi spreads one
 * long sequence over its workers); *replays = chunks whose speculation failed and were replayed
 * from the previous chunk's state, -1 = the sequence fell back to one stream */
int64_t wfmh_test_winnow_chunked(const char* seq, int64_t len, int k, int w, int s, int32_t seq_id,
                                 const uint64_t* hash, const int8_t* strand, int64_t chunk_len,
                                 wfm_minmer_t* out, int64_t cap, int* replays);

/* the same on the thinned stream wfm_add_minmers_multi feeds its workers (wfm_prefilter_kmers,
 * wfmash_hip.h): the selection is restated on the host from its definition, with the hash threshold set to
 * let c_factor * s of a window's w-k+1 k-mers through, and only the kept k-mers are winnowed.  kept_pos (optional)
 * receives the kept k-mer starts, *n_kept their number. */
int64_t wfmh_test_winnow_thinned(const char* seq, int64_t len, int k, int w, int s, int32_t seq_id,
                                 const uint64_t* hash, const int8_t* strand, double c_factor, int64_t chunk_len,
                                 wfm_minmer_t* out, int64_t cap, uint32_t* kept_pos, int64_t cap_kept,
                                 int64_t* n_kept, int* replays);

/* the closing sort of a sequence's records by (wpos, wpos_end) (commonFunc.hpp:696): threads == 1 is std::sort,
 * threads > 1 the same introsort with its halves on several threads -- same result, ties included */
void wfmh_test_sort_records(wfm_minmer_t* recs, int64_t n, int threads);
/* CPU test hooks of the 2-bit packed extension (wfmash_amd/csrc/wfa_pack.h): the run of agreeing bases from (v, h) of two sequences that begin at
 * byte start_p / start_t of their buffers, computed on the packed mirror the way the tile kernel stages it; whether a buffer is pure upper-case ACGT */
int wfmh_test_packed_lce(const uint8_t* buf_p, int64_t n_p, int64_t start_p, const uint8_t* buf_t, int64_t n_t, int64_t start_t, int v, int h, int maxn);
int wfmh_test_is_acgt(const uint8_t* seq, int64_t n);

/* The winnowing kernel's control flow and capacities (wfmash_amd/csrc/map_winnow_core.h: one speculative chunk of the
 * thinned stream per wave, boundary states compared, interval starts resolved) run on the host over plain arrays, then
 * the closing steps.  Returns the number of records, or -1 when the device would hand the sequence back to the host's
 * winnower (*why: the wn::F_* bits of map_winnow_core.h; bit 31: an N among the first k-mers the reference does not notice).
 * chunk_len < 0: chunks of -chunk_len k-mers, and every second speculation counts as failed (the replay from the
 * predecessor's state). */
int64_t wfmh_test_winnow_model(const char* seq, int64_t len, int k, int w, int s, int32_t seq_id, const uint64_t* hash,
                               const int8_t* strand, double c_factor, int64_t chunk_len, wfm_minmer_t* out, int64_t cap,
                               uint32_t* why);

/* The arrangement wfm_finish_records computes on the device -- the partitions of std::sort's introsort loop as lists,
 * swaps and a cut, then a stable sort (wfmash_amd/csrc/map_finish.hip) -- computed on the host, in place; key = (wpos, wpos_end). */
void wfmh_test_sortlike_model(wfm_minmer_t* recs, int64_t n);

/* The closing steps of addMinmers on raw interval records by the host path (cut, strand signs, std::sort, std::unique):
 * what wfm_finish_records (wfmash_hip.h) is held against. */
int64_t wfmh_test_finish_records(const wfm_minmer_t* raw, int64_t n, int w, wfm_minmer_t* out, int64_t cap);

/* ---- map phase (skch::Map, src/map/include/computeMap.hpp) ---- */

/* skch::Parameters as set up by parse_args.hpp; wfmh_map_default_params fills the defaults
 * (file:line of each default in wfmash_amd/host/map_types.hpp). */
typedef struct {
  int32_t  kmer_size;                 /* -k 15 */
  int64_t  window_length;             /* -w / segment length, 1000 */
  int64_t  block_length;              /* -l 0 */
  int64_t  chain_gap;                 /* -c 2000 */
  uint64_t max_mapping_length;        /* -P 50000 */
  float    percentage_identity;       /* -p as a fraction; 0.70 unless estimated */
  int32_t  sketch_size;               /* -s; 0 = derive from identity (parse_args.hpp:642-644) */
  int32_t  filter_mode;               /* 1 map (default), 2 one-to-one, 3 none */
  uint32_t num_mappings_for_segment;  /* -n; UINT32_MAX = inf (default) */
  uint32_t num_mappings_for_scaffold; /* 1 */
  int32_t  drop_rand;                 /* 0 */
  int32_t  split;                     /* 1 */
  int32_t  merge_mappings;            /* 1 */
  int32_t  skip_self;                 /* 1 */
  int32_t  skip_prefix;               /* 1 */
  int32_t  lower_triangular;          /* 0 */
  char     prefix_delim;              /* '#' */
  int32_t  filter_length_mismatches;  /* 1 */
  uint64_t sparsity_hash_threshold;   /* UINT64_MAX */
  double   overlap_threshold;         /* 0.95 */
  double   scaffold_overlap_threshold;/* 0.5 */
  int64_t  scaffold_max_deviation;    /* 100000 */
  int64_t  scaffold_gap;              /* 100000 */
  int64_t  scaffold_min_length;       /* 10000 */
  int32_t  legacy_output;             /* 0 */
  int32_t  minimum_hits;              /* 3 */
  double   max_kmer_freq;             /* 0.0002 */
  int64_t  index_by_size;             /* -b; INT64_MAX */
  float    kmer_complexity_threshold; /* 0 */
  int32_t  stage1_topani_filter;      /* 1 */
  int32_t  stage2_full_scan;          /* 1 */
  float    ani_diff, ani_diff_conf;   /* 0.0, 0.999 */
  double   hg_numerator;              /* 1.0 */
  int32_t  threads;                   /* 1 */
  int32_t  auto_pct_identity;         /* 1: estimate the identity from the data, -p aniN[+-adj] (parse_args.hpp:341-395);
                                         0: use percentage_identity as given */
  int32_t  ani_percentile;            /* 50 */
  float    ani_adjustment;            /* -2.0 (percent) */
  /* sequence selection (parse_args.hpp:112-115); NULL = unset */
  const char* target_prefix;          /* -T: only targets whose name starts with this */
  const char* target_list;            /* -R: file with target names */
  const char* query_prefix;           /* -Q: comma-separated name prefixes */
  const char* query_list;             /* -A: file with query names (also how ranks shard the queries) */
  /* on-disk index (parse_args.hpp:745-758; format: wfmash_amd/host/index_file.hpp) */
  const char* index_file;             /* NULL = none */
  int32_t  write_index;               /* 1: -W, build the index of every target subset, write it and stop;
                                         0 with index_file set: -I, read the index instead of building it */
  int32_t  pad_;
  /* appended: nothing above moves */
  const char* scaffold_out;           /* --scaffold-out FILE: the scaffold chains the filter used as anchors (parse_args.hpp:105,464-465);
                                         NULL = none, and nothing of them is kept */
  int32_t  streaming_minhash;         /* --streaming-minhash (parse_args.hpp:137,177): 1 = target sketches from a per-sequence bottom-s
                                         MinHash (wfm_streaming_minmers) instead of winnowed minmers; 0 (default) = winnowing */
} wfmh_map_params_t;

void wfmh_map_default_params(wfmh_map_params_t* p);

typedef struct {
  uint64_t targets, queries, subsets;
  uint64_t target_bp, query_bp;
  uint64_t index_windows;   /* minmer intervals indexed (all subsets) */
  uint64_t fragments;       /* query fragments mapped (all subsets) */
  uint64_t l2_mappings;     /* MappingResults produced by the GPU stages */
  uint64_t written;         /* mapping PAF records written */
  float    percentage_identity;  /* the threshold used (estimated when auto_pct_identity) */
  int32_t  sketch_size;          /* the sketch size used */
  double   ms_index, ms_map, ms_filter, ms_total;
  double   ms_replicate;    /* copying the finished index to the other GPUs (wfmh_map_multi) */
  double   ms_identity;     /* the identity estimate (-p aniN: reading every sequence once + one MinHash per sequence on the device) */
  double   ms_wall;         /* the whole call: identity estimate, reading the sequences, index, mapping, post-processing, output */
  int32_t  index_parts;     /* the most handles that sketched one target subset (wfmh_map_multi deals a subset's sequences over its
                               handles): 1 = every subset on handles[0] alone, 0 = no subset was sketched (-I) */
  int32_t  pad_;
  double   ms_index_sketch; /* part of ms_index: the sketching of the subset's parts, the slowest part's wall time, summed over subsets
                               (0 where handles[0] built alone) */
  double   ms_index_merge;  /* part of ms_index: bringing the parts to handles[0]'s device and into subset order (staging + gather) */
} wfmh_map_summary_t;

/* The map phase on files: replaces skch::Map's constructor + mapQuery()
 * (src/map/include/computeMap.hpp:147-230, :329-872).  Reads the FASTA files (query_fasta NULL or
 * equal to target_fasta = all-vs-all), indexes the targets on the GPU, maps every query fragment
 * (sketch, L1, L2 on the GPU), post-processes per query on the host and writes the approximate
 * mapping PAF (the -m / -i hand-off file, parse_args.hpp:781-811).  Returns 0 or WFM_E_*. */
int wfmh_map(wfm_handle_t* h, const char* target_fasta, const char* query_fasta, const char* out_paf,
             const wfmh_map_params_t* params, wfmh_map_summary_t* summary);

/* The same over n GPUs of one node.  The sequences of a target subset are dealt over the handles (longest first onto the
 * least loaded, ties to the lower index), every handle sketches its share (wfm_sketch_part), the records meet on
 * handles[0]'s device where the index stage runs once on the union in subset order (wfm_index_build_parts), and the
 * finished index is copied to the other devices (wfm_index_replicate): the index, and with it every PAF byte and every
 * -W index file, is that of one handle.  --streaming-minhash records are made on the host and stay with handles[0], as does
 * everything with WFM_INDEX_SHARDED=0 (read per call; =1 takes the two-step path with a single handle too, which then reports
 * ms_index_sketch).  Batches of whole query sequences go to whichever device is free
 * (one task per query in the reference, computeMap.hpp:527-688), records are written in query order as with one GPU. */
int wfmh_map_multi(wfm_handle_t* const* handles, int n, const char* target_fasta, const char* query_fasta, const char* out_paf,
                   const wfmh_map_params_t* params, wfmh_map_summary_t* summary);

/* ---- the group-by-group ANI table the identity estimate is made from (wfmash_amd/host/ani_estimate.hpp) ----
 * estimate_identity_for_groups sketches every sequence on the device, pools the sketches per group and turns every (query group,
 * target group) pair's shared-hash count into an ANI (map_stats.hpp:325-822); the reference prints that table to stderr
 * (:746-752).  Here it is a file.  One row per ordered pair (query group q, target group t) with q != t, in ascending (q, t) group
 * ids: the two group prefixes, the sizes of the two pooled sketches, `shared` from one wfm_sketch_intersections call on
 * handles[0], jaccard = shared / the smaller size, ani = 1 - j2md((float)jaccard, 21) -- the estimate's arithmetic.  Pairs without
 * a shared hash or with an empty sketch are rows of zeros (the estimate drops them, the table shows them).  The text form: the line
 *   #query_group<TAB>target_group<TAB>query_hashes<TAB>target_hashes<TAB>shared<TAB>jaccard<TAB>ani
 * then one line per row, jaccard and ani as %.6f.
 *
 * wfmh_ani_matrix: the table of the sequences a map call with these files and params would take (-T, -Q, -R, -A, -Y apply), written
 * to out_tsv; sketching is spread over the handles as the estimate spreads it, the intersections run on handles[0]; no index, no
 * mapping.  query_fasta may be NULL (= target_fasta).  wfmh_ani_matrix_rows: the same rows as values instead of text (*rows is
 * released with wfmh_free_ani_rows).  wfmh_set_ani_matrix(path): the NEXT wfmh_map / wfmh_map_multi call of the process writes the
 * table to path before it maps -- from the very sketches its estimate uses, made also when auto_pct_identity is 0 -- and then goes
 * on as it would have: its PAF is byte for byte the one without the table.  The call takes the setting with it; NULL clears it.
 * Returns 0 or WFM_E_* (message in wfm_last_error(handles[0])). */
typedef struct {
  char*    query_group;
  char*    target_group;
  uint64_t query_hashes, target_hashes, shared;
  double   jaccard, ani;
} wfmh_ani_row_t;
int  wfmh_ani_matrix(wfm_handle_t* const* handles, int n, const char* target_fasta, const char* query_fasta,
                     const wfmh_map_params_t* params, const char* out_tsv);
int  wfmh_ani_matrix_rows(wfm_handle_t* const* handles, int n, const char* target_fasta, const char* query_fasta,
                          const wfmh_map_params_t* params, wfmh_ani_row_t** rows, int64_t* n_rows);
void wfmh_free_ani_rows(wfmh_ani_row_t* rows, int64_t n_rows);
void wfmh_set_ani_matrix(const char* out_tsv);
/* Test hook (no GPU needed): the table's text from n rows given as names, sketch sizes and counts; jaccard and ani are computed
 * as above.  malloc'd, wfmh_free. */
char* wfmh_test_ani_tsv(const char* const* query_groups, const char* const* target_groups, const uint64_t* query_hashes,
                        const uint64_t* target_hashes, const uint64_t* shared, int64_t n);

/* Test hook (no GPU needed): the deal of wfmh_map_multi's index build.  out_part[i] = the part (0 .. n_parts - 1) that item i of
 * lengths[0 .. n) goes to.  Returns 0 or WFM_E_ARG. */
int wfmh_test_deal(const int64_t* lengths, int64_t n, int n_parts, int32_t* out_part);

/* Test hook (no GPU needed): what the map driver decides without a device (wfmash_amd/host/map_plan.hpp), on in[0 .. n).
 * The caller sizes out for the op.  Returns 0 or WFM_E_ARG.
 *   0  layout_fragments: in = len, w, base, first_frag; out = nfrag, then the offsets
 *   1  target_subsets:   in = batch, then the targets' lengths; out = the number of subsets, then their sizes (the targets in order)
 *   2  plan_batch:       in = batch_bases, qi, then the queries' lengths (<= 0: missing or empty); out = next, in_place, n_bases,
 *                        the number of members, then the members
 *   3  in = n_handles, query_bp, nfrag, subset_size; out = batch_bases_for, mapping_cap, spare_hint, then the constants
 *                        kBatchBases, kCopyBases, kEarlyFilterFrags, kSpareMappings
 *   4  split_by_query:   in = nq, (first_frag, nfrag) per query, then mfrag per mapping; out = first_map[0 .. nq]
 *   5  query_results:    in = first_frag, w, m0, nq, threads, has_perm, n_maps, then mfrag, perm and queryStartPos per mapping;
 *                        out = orig's size, per result the mapping it was and its queryStartPos (nq each), then orig */
int wfmh_test_map_plan(int op, const int64_t* in, int64_t n, int64_t* out);

/* External seeds (-K, parse_args.hpp:78,771-773; skch::ExternalSeeder, src/map/include/externalSeeder.hpp) in place of the
 * MinHash mapper: the PAF records of another tool (seeds_paf; "-" or "/dev/stdin" = standard input) grouped by query, each query's
 * through the group plane sweep, sparsification and the scaffold filter, written as a mapping PAF (the -m / -i hand-off file) to
 * out_paf.  Host only, no device: the stages read nothing the identity estimate sets.  params->scaffold_out is honoured.
 * Summary: queries = seed groups, targets = target sequences, l2_mappings = seeds read, written = records written; ms_map = reading
 * the seeds, ms_filter = filters and output, ms_total = ms_wall = the whole call.  Returns 0 or WFM_E_* (message on stderr). */
int wfmh_seed_paf(const char* target_fasta, const char* query_fasta, const char* seeds_paf, const char* out_paf,
                  const wfmh_map_params_t* params, wfmh_map_summary_t* summary);

/* Test hook for the host-side post-processing of one query's mappings (CPU tests): runs
 * mappingBoundarySanityCheck + Map::filterSubsetMappings + reportReadMappings
 * (stage "subset"), or filterByGroup on the reference axis as the one-to-one pass does
 * (stage "onetoone"), on caller-supplied MappingResults and returns the mapping PAF text
 * (malloc'd; wfmh_free).  fasta: the file whose .fai (or the FASTA itself) defines the sequences. */
char* wfmh_test_filter(const char* stage, const wfm_mapping_t* maps, int64_t n, const char* fasta,
                       const char* query_name, const wfmh_map_params_t* prm);
/* The same for stage "subset" with the mappings given in chaining order, as the map driver builds them from the device's
 * permutation: orig[i] = the position maps[i] has in fragment order (filterSubsetMappings' presorted_orig). */
char* wfmh_test_filter_ordered(const char* stage, const wfm_mapping_t* maps, int64_t n, const uint32_t* orig, const char* fasta,
                               const char* query_name, const wfmh_map_params_t* prm);

/* Test hook for the FASTA reader that stands in for faigz/htslib (src/common/faigz.h:221-505;
 * random access through .fai, and .gzi for BGZF).  name == NULL: "indexed|in-memory" + one
 * "name\tlength" line per sequence in file order.  Otherwise bases [start, end_inclusive] of `name`
 * (faidx_reader_fetch_seq's convention); whole != 0 loads the sequence first, as the map driver does.
 * malloc'd, wfmh_free; "ERROR: ..." on failure. */
char* wfmh_test_fasta(const char* path, const char* name, int64_t start, int64_t end_inclusive, int whole);

/* The sequences a map call loaded stay in memory for the call that follows (the align phase fetches its windows from the
 * same files; the reference keeps its faidx readers open for the whole run, src/common/faigz.h:221-505).  They are let go
 * when the next map call hands in its own, or here.  (WFM_FASTA_KEEP=0: nothing is kept; WFM_FASTA_KEEP_GB: the most that is, 32.) */
void wfmh_release_sequences(void);

/* Test hook: the whole sequence `name` through the store the process shares per path (open_shared), which is then kept as a
 * map call keeps its stores: a second call on a file rewritten in between must see the new bytes.  malloc'd, wfmh_free. */
char* wfmh_test_fasta_shared(const char* path, const char* name);

/* Test hook for the on-disk index format (wfmash_amd/host/index_file.hpp; no GPU needed).  op "ids": the id
 * section alone (SequenceIdManager::exportIdMapping, sequenceIds.hpp:101-115) of fasta's sequences into out_path;
 * op "rewrite": every sub-index of in_path is read and written again into out_path.  0, or -1 (message on stderr). */
int wfmh_test_index_file(const char* op, const char* fasta, char prefix_delim, const char* in_path, const char* out_path);

#ifdef __cplusplus
}
#endif
#endif
