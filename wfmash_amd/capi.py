"""ctypes bindings of libwfmash_hip.so (the C ABI declared in include/wfmash_hip.h).

This is plumbing for tests and bench.py; the product is the shared library.
There is no CPU fallback: if the library is missing or no gfx950 device is
visible, loading / `Handle()` raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WFM_LIB_PATH") or os.path.join(_HERE, "libwfmash_hip.so")  # WFM_LIB_PATH: A/B runs of two builds

WFM_MODE_END2END_BIWFA = 0
WFM_MODE_ENDSFREE = 1
WFM_MODE_END2END_UNI = 2
# flags OR-ed into a problem's mode (include/wfmash_hip.h): the score alone; score_hint as a hard limit of the score (END2END_BIWFA)
WFM_MODE_MASK = 0xff
WFM_MODE_SCORE_ONLY = 0x100
WFM_MODE_SCORE_LIMIT = 0x200
WFM_ST_MAX_SCORE = -100  # the optimal score is beyond the problem's limit

DEFAULT_PEN = (5, 8, 2, 24, 1)  # parse_args.hpp:290-294
# wfm_get_problem_flags (include/wfmash_hip.h): which of the rarer paths a problem took
WFM_PF_ROOT_AGAIN, WFM_PF_JOB_AGAIN, WFM_PF_BASE_RETRY, WFM_PF_BASE_RETRY2, WFM_PF_BYTE_KERNEL, WFM_PF_P2_ROUNDS, WFM_PF_RING_KERNEL, WFM_PF_BASE_TILES = 1, 2, 4, 8, 16, 32, 64, 128
WFM_PF_RING_GROWN = 256
# wfm_get_tile_counters (include/wfmash_hip.h): the paths the BiWFA tile phase took in an align call, in the header's order
TILE_COUNTERS = ("jobs", "exact_ends", "fine_reruns", "gap_reruns", "ring3", "blocks_coarse", "blocks_fine", "left_band",
                 "reuse_resumed", "reuse_fallbacks", "reuse_keeps", "reuse_touched", "reuse_fell_other", "planned_ends",
                 "p2_exact", "p2_exact_misses")

EXPORTS = [
    "wfm_create", "wfm_destroy", "wfm_last_error", "wfm_device_name",
    "wfm_align_arena_bytes", "wfm_align_batch", "wfm_upload_sequences",
    "wfm_free_sequences", "wfm_align_resident", "wfm_get_stats",
    "wfm_hash_kmers", "wfm_sketch_fragments", "wfm_add_minmers",
    "wfm_index_build", "wfm_index_free", "wfm_index_info", "wfm_index_download",
    "wfm_map_l1", "wfm_map_l2", "wfm_map_fragments", "wfm_minhash_sketch", "wfm_add_minmers_multi",
    "wfm_prefilter_kmers", "wfm_index_build_sequences", "wfm_index_upload",
    "wfm_index_replicate", "wfm_device_count", "wfm_finish_records",
    "wfm_align_batch_rle", "wfm_align_resident_rle", "wfm_free_runs", "wfm_score_bounds", "wfm_get_busy_intervals", "wfm_trim_device_cache", "wfm_map_fragments_ordered", "wfm_map_sequence_cache", "wfm_selftest_dpp", "wfm_selftest_arena_growth", "wfm_set_concurrent_calls", "wfm_get_problem_flags",
    "wfm_get_tile_counters",
    "wfm_streaming_minmers", "wfm_index_build_streaming",
    "wfm_sketch_part", "wfm_minmer_part_info", "wfm_minmer_part_download", "wfm_minmer_part_free", "wfm_index_build_parts",
    "wfm_seqstore_create", "wfm_seqstore_free", "wfm_seqstore_add", "wfm_seqstore_info",
    "wfm_upload_sequence_refs", "wfm_align_refs_rle", "wfm_download_sequences",
    "wfm_check_runs", "wfm_check_optimal", "wfm_left_align_runs", "wfm_cs_strings", "wfm_free_cs",
    "wfm_call_variants", "wfm_free_variants", "wfm_maf_rows", "wfm_free_maf",
    "wfm_coverage_create", "wfm_coverage_free", "wfm_coverage_add", "wfm_coverage_export", "wfm_coverage_import", "wfm_coverage_intervals",
    "wfm_coverage_free_list",
    "wfm_liftset_create", "wfm_liftset_free", "wfm_lift_runs", "wfm_free_lifts",
    "wfm_chain_runs", "wfm_free_chain",
    "wfm_pav_create", "wfm_pav_free", "wfm_pav_add", "wfm_pav_union", "wfm_pav_export", "wfm_pav_import", "wfm_pav_matrix", "wfm_pav_counts",
    "wfm_pav_free_list",
    "wfm_sites_create", "wfm_sites_free", "wfm_sites_add_variants", "wfm_sites_add_ref", "wfm_sites_table", "wfm_sites_export", "wfm_sites_import",
    "wfm_sites_counts", "wfm_sites_free_list",
    "wfm_net_create", "wfm_net_free", "wfm_net_add", "wfm_net_table", "wfm_net_export", "wfm_net_import", "wfm_net_counts", "wfm_net_free_list",
    "wfm_trans_create", "wfm_trans_free", "wfm_trans_add", "wfm_trans_closure", "wfm_trans_export", "wfm_trans_import", "wfm_trans_counts",
    "wfm_trans_free_list",
    "wfm_sketch_intersections",
]
ISECT_LDS_MAX = 4096  # WFM_ISECT_LDS_MAX: the longest column sketch wfm_sketch_intersections searches in LDS
# wfm_check_runs (include/wfmash_hip.h): what a problem's runs were flagged for
WFM_CK_NOT_CHECKED, WFM_CK_BAD_RUN, WFM_CK_SPANS, WFM_CK_M_DIFFERS, WFM_CK_X_EQUAL, WFM_CK_SCORE, WFM_CK_COUNTS = 1, 2, 4, 8, 16, 32, 64
CK_NAMES = ("NOT_CHECKED", "BAD_RUN", "SPANS", "M_DIFFERS", "X_EQUAL", "SCORE", "COUNTS")
CHECK_SLICE = 16384  # WFM_CHECK_SLICE: ops one compare task covers
# wfm_left_align_runs (include/wfmash_hip.h): why a problem's runs were left as they came
WFM_LA_NOT_DONE, WFM_LA_SPANS = 1, 2
# wfm_cs_strings (include/wfmash_hip.h): the two forms, why a problem has no string, and the output bytes one workgroup writes
WFM_CS_SHORT, WFM_CS_LONG = 0, 1
WFM_CS_NOT_DONE, WFM_CS_SPANS = 1, 2
WFM_CS_SLICE = 16384
# wfm_maf_rows (include/wfmash_hip.h): why a problem has no blocks, and the output bytes one workgroup writes
WFM_MAF_NOT_DONE, WFM_MAF_SPANS = 1, 2
WFM_MAF_SLICE = 16384
# wfm_call_variants (include/wfmash_hip.h): a record's kind and its MASKED bit, why a problem has no records, the allele bytes one workgroup writes
WFM_VAR_SNV, WFM_VAR_INS, WFM_VAR_DEL = 0, 1, 2
WFM_VAR_MASKED = 256
WFM_VAR_NOT_DONE, WFM_VAR_SPANS = 1, 2
WFM_VAR_SLICE = 16384
# wfm_coverage_* (include/wfmash_hip.h): why a problem adds nothing, the words one workgroup counts and writes, the elements one workgroup scans
WFM_COV_SPANS = 2
WFM_COV_TILE = 4096
WFM_COV_SCAN_BLOCK = 1024
# wfm_liftset_* / wfm_lift_runs (include/wfmash_hip.h): why a problem has no lifts, the intervals one workgroup takes in the running maximum
WFM_LIFT_SPANS = 2
WFM_LIFT_SCAN_BLOCK = 1024
# wfm_chain_runs (include/wfmash_hip.h): a problem's two flags, and why a problem has no blocks
WFM_CHAIN_SWAP, WFM_CHAIN_REVERSE = 1, 2
WFM_CHAIN_SPANS = 2
# wfm_pav_* (include/wfmash_hip.h): why a problem added nothing, the segments one workgroup takes in the scans of the union
WFM_PAV_SPANS = 2
WFM_PAV_SCAN_BLOCK = 1024
# wfm_sites_* (include/wfmash_hip.h): the allele bytes one lane / one workgroup hashes or compares, the code of a hash collision
WFM_SITES_SLICE = 64
WFM_SITES_TASK = 16384
WFM_E_ARG, WFM_E_INTERNAL = -3, -7
# wfm_net_* (include/wfmash_hip.h): "take the = columns" as a problem's score, why a problem added nothing, the elements one workgroup scans
WFM_NET_SCORE_EQ = 0xffffffff
WFM_NET_SPANS = 2
WFM_NET_SCAN_BLOCK = 1024
# wfm_trans_* (include/wfmash_hip.h): a record's flag, why a problem added nothing, the arcs one workgroup takes in the running maximum
WFM_TRANS_REVERSE = 1
WFM_TRANS_SPANS = 2
WFM_TRANS_SCAN_BLOCK = 1024
WFM_E_NOMEM = -4
# wfm_check_optimal (include/wfmash_hip.h): what a problem's score was flagged for, and the band widths at which the kernel changes form
WFM_OPT_NOT_CHECKED, WFM_OPT_SKIPPED, WFM_OPT_CHEAPER, WFM_OPT_UNREACHED = 1, 2, 4, 8
OPT_NAMES = ("NOT_CHECKED", "SKIPPED", "CHEAPER", "UNREACHED")
OPT_BAND_C1, OPT_BAND_C4, OPT_REG_MAX = 256, 1024, 4096  # WFM_OPT_BAND_C1 / WFM_OPT_BAND_C4 / WFM_OPT_REG_MAX
OPT_ROWS_MB = 256  # WFM_OPT_ROWS_MB
SEQ_GATHER_CHUNK = 16384  # WFM_SEQ_GATHER_CHUNK (include/wfmash_hip.h): destination bytes per task of the gather kernel


class Penalties(C.Structure):
    _fields_ = [("x", C.c_int32), ("o1", C.c_int32), ("e1", C.c_int32),
                ("o2", C.c_int32), ("e2", C.c_int32)]


class Problem(C.Structure):
    _fields_ = [("pattern", C.c_char_p), ("plen", C.c_int32),
                ("text", C.c_char_p), ("tlen", C.c_int32),
                ("mode", C.c_int32),
                ("pattern_begin_free", C.c_int32), ("pattern_end_free", C.c_int32),
                ("text_begin_free", C.c_int32), ("text_end_free", C.c_int32),
                ("score_hint", C.c_int32), ("pad_", C.c_int32)]


class ProblemRef(C.Structure):
    """wfm_problem_ref_t: a problem whose sides are windows of sequences in a SeqStore (or host bytes where *_seq is -1)."""
    _fields_ = [("pattern", C.c_char_p), ("text", C.c_char_p),
                ("pattern_off", C.c_int64), ("text_off", C.c_int64),
                ("pattern_seq", C.c_int32), ("text_seq", C.c_int32),
                ("plen", C.c_int32), ("tlen", C.c_int32),
                ("mode", C.c_int32),
                ("pattern_revcomp", C.c_int32), ("text_revcomp", C.c_int32),
                ("pattern_begin_free", C.c_int32), ("pattern_end_free", C.c_int32),
                ("text_begin_free", C.c_int32), ("text_end_free", C.c_int32),
                ("score_hint", C.c_int32)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int32), ("score", C.c_int32),
                ("ops_off", C.c_uint64), ("ops_len", C.c_uint32),
                ("n_runs", C.c_uint32), ("cells", C.c_uint64)]


class Check(C.Structure):
    """wfm_check_t: what wfm_check_runs found in one problem's runs."""
    _fields_ = [("flags", C.c_uint32), ("score", C.c_int32), ("bad_p", C.c_int32), ("bad_t", C.c_int32),
                ("bad_run", C.c_uint32), ("n_runs", C.c_uint32),
                ("matches", C.c_uint32), ("mismatches", C.c_uint32), ("ins_runs", C.c_uint32), ("ins_bases", C.c_uint32),
                ("del_runs", C.c_uint32), ("del_bases", C.c_uint32)]


class LeftAlign(C.Structure):
    """wfm_leftalign_t: what wfm_left_align_runs did to one problem's runs."""
    _fields_ = [("flags", C.c_uint32), ("gaps", C.c_uint32), ("moved", C.c_uint32), ("runs_out", C.c_uint32),
                ("bases_moved", C.c_uint64), ("longest", C.c_uint32), ("pad_", C.c_uint32)]


class Cs(C.Structure):
    """wfm_cs_t: where wfm_cs_strings put one problem's cs string, and the runs it was spelled from."""
    _fields_ = [("flags", C.c_uint32), ("n_runs", C.c_uint32), ("off", C.c_uint64), ("len", C.c_uint64)]


class Variant(C.Structure):
    """wfm_variant_t: one record of wfm_call_variants; its REF is alleles[off : off + ref_len], its ALT the alt_len bytes behind."""
    _fields_ = [("problem", C.c_uint32), ("kind", C.c_uint32), ("p", C.c_uint32), ("t", C.c_uint32),
                ("ref_len", C.c_uint32), ("alt_len", C.c_uint32), ("off", C.c_uint64)]


VARIANT_DTYPE = np.dtype([("problem", "<u4"), ("kind", "<u4"), ("p", "<u4"), ("t", "<u4"), ("ref_len", "<u4"), ("alt_len", "<u4"), ("off", "<u8")])


class VarCall(C.Structure):
    """wfm_varcall_t: where wfm_call_variants put one problem's records, the runs they were called from and the gaps it did not call."""
    _fields_ = [("flags", C.c_uint32), ("n_runs", C.c_uint32), ("first", C.c_uint64), ("count", C.c_uint64),
                ("end_gaps", C.c_uint32), ("pad_", C.c_uint32)]


class MafBlock(C.Structure):
    """wfm_maf_block_t: one block of wfm_maf_rows; its row P is rows[off : off + cols], its row T the cols bytes behind."""
    _fields_ = [("off", C.c_uint64), ("problem", C.c_uint32), ("p", C.c_uint32), ("t", C.c_uint32), ("psize", C.c_uint32),
                ("tsize", C.c_uint32), ("cols", C.c_uint32), ("eq", C.c_uint32), ("x", C.c_uint32)]


MAF_BLOCK_DTYPE = np.dtype([("off", "<u8"), ("problem", "<u4"), ("p", "<u4"), ("t", "<u4"), ("psize", "<u4"), ("tsize", "<u4"),
                            ("cols", "<u4"), ("eq", "<u4"), ("x", "<u4")])


class MafCall(C.Structure):
    """wfm_mafcall_t: where wfm_maf_rows put one problem's blocks, and the runs they were spelled from."""
    _fields_ = [("flags", C.c_uint32), ("n_runs", C.c_uint32), ("first", C.c_uint64), ("count", C.c_uint64)]


class CovProb(C.Structure):
    """wfm_cov_prob_t: a problem of wfm_coverage_add: the global index of its first pattern base and its runs in the call's run buffer."""
    _fields_ = [("base", C.c_uint64), ("runs_off", C.c_uint64), ("n_runs", C.c_uint32), ("pad_", C.c_uint32)]


class CovEntry(C.Structure):
    """wfm_cov_entry_t: a non-zero word of a coverage object's difference array."""
    _fields_ = [("pos", C.c_uint64), ("delta", C.c_int32), ("pad_", C.c_uint32)]


class CovInterval(C.Structure):
    """wfm_cov_interval_t: an interval of constant depth; it ends where the next begins."""
    _fields_ = [("start", C.c_uint64), ("depth", C.c_uint32), ("pad_", C.c_uint32)]


COV_PROB_DTYPE = np.dtype([("base", "<u8"), ("runs_off", "<u8"), ("n_runs", "<u4"), ("pad_", "<u4")])
COV_ENTRY_DTYPE = np.dtype([("pos", "<u8"), ("delta", "<i4"), ("pad_", "<u4")])
COV_INTERVAL_DTYPE = np.dtype([("start", "<u8"), ("depth", "<u4"), ("pad_", "<u4")])


class Lift(C.Structure):
    """wfm_lift_t: one (problem, interval) pair of wfm_lift_runs; every field an offset inside the problem."""
    _fields_ = [("problem", C.c_uint32), ("interval", C.c_uint32), ("p0", C.c_uint32), ("p1", C.c_uint32), ("t0", C.c_uint32), ("t1", C.c_uint32),
                ("eq", C.c_uint32), ("x", C.c_uint32)]


class LiftCall(C.Structure):
    """wfm_liftcall_t: where a problem's lifts lie in the output of wfm_lift_runs."""
    _fields_ = [("flags", C.c_uint32), ("n_runs", C.c_uint32), ("first", C.c_uint64), ("count", C.c_uint64)]


LIFT_IV_DTYPE = np.dtype([("start", "<u8"), ("end", "<u8")])
LIFT_DTYPE = np.dtype([("problem", "<u4"), ("interval", "<u4"), ("p0", "<u4"), ("p1", "<u4"), ("t0", "<u4"), ("t1", "<u4"), ("eq", "<u4"), ("x", "<u4")])
LIFTCALL_DTYPE = np.dtype([("flags", "<u4"), ("n_runs", "<u4"), ("first", "<u8"), ("count", "<u8")])


# wfm_chain_prob_t, wfm_chain_block_t and wfm_chaincall_t of wfm_chain_runs
CHAIN_PROB_DTYPE = np.dtype([("runs_off", "<u8"), ("n_runs", "<u4"), ("flags", "<u4")])
CHAIN_BLOCK_DTYPE = np.dtype([("size", "<u4"), ("dt", "<u4"), ("dq", "<u4"), ("eq", "<u4")])
CHAINCALL_DTYPE = np.dtype([("flags", "<u4"), ("n_runs", "<u4"), ("first", "<u8"), ("count", "<u8"), ("lead_dt", "<u4"), ("lead_dq", "<u4"),
                            ("trail_dt", "<u4"), ("trail_dq", "<u4"), ("eq", "<u4"), ("x", "<u4")])


PAV_PROB_DTYPE = np.dtype([("base", "<u8"), ("runs_off", "<u8"), ("n_runs", "<u4"), ("group", "<u4")])
PAV_SEG_DTYPE = np.dtype([("start", "<u8"), ("length", "<u4"), ("group", "<u4")])
NET_PROB_DTYPE = np.dtype([("base", "<u8"), ("runs_off", "<u8"), ("n_runs", "<u4"), ("score", "<u4"), ("order", "<u8")])
NET_BLOCK_DTYPE = np.dtype([("order", "<u8"), ("t", "<u8"), ("q", "<u4"), ("size", "<u4")])   # wfm_net_block_t, and a piece
NET_REC_DTYPE = np.dtype([("order", "<u8"), ("score", "<u4"), ("zero", "<u4")])
TRANS_PROB_DTYPE = np.dtype([("t", "<u8"), ("q", "<u8"), ("runs_off", "<u8"), ("n_runs", "<u4"), ("flags", "<u4")])
TRANS_REC_DTYPE = np.dtype([("t", "<u8"), ("q", "<u8"), ("pre_off", "<u8"), ("n_runs", "<u4"), ("flags", "<u4")])
TRANS_WORD_DTYPE = np.dtype([("p", "<u4"), ("t", "<u4"), ("eq", "<u4"), ("x", "<u4")])
TRANS_IV_DTYPE = np.dtype([("start", "<u8"), ("end", "<u8"), ("seed", "<u4"), ("pad_", "<u4")])
TRANS_SEED_DTYPE = np.dtype([("first", "<u8"), ("count", "<u8"), ("bases", "<u8")])
NET_CALL_DTYPE = np.dtype([("order", "<u8"), ("score", "<u4"), ("zero", "<u4"), ("first", "<u8"), ("count", "<u8"), ("bases_won", "<u8"),
                           ("bases_aligned", "<u8")])
SITE_VAR_DTYPE = np.dtype([("pos", "<u8"), ("kind", "<u4"), ("group", "<u4"), ("ref_len", "<u4"), ("alt_len", "<u4"), ("off", "<u8")])
SITE_DTYPE = np.dtype([("pos", "<u8"), ("kind", "<u4"), ("n_carrier_groups", "<u4"), ("ref_len", "<u4"), ("alt_len", "<u4"), ("off", "<u8")])


class OptCheck(C.Structure):
    """wfm_optcheck_t: what wfm_check_optimal found for one problem's score."""
    _fields_ = [("flags", C.c_uint32), ("dp_score", C.c_int32), ("band_lo", C.c_int32), ("band_hi", C.c_int32), ("cells", C.c_uint64)]


class Stats(C.Structure):
    _fields_ = [("cells", C.c_uint64), ("bytes_algorithmic", C.c_uint64),
                ("ms_kernels", C.c_double), ("ms_breakpoint", C.c_double),
                ("ms_base", C.c_double), ("ms_total", C.c_double),
                ("levels", C.c_uint32), ("bp_jobs", C.c_uint32), ("base_jobs", C.c_uint32),
                ("bp_launches", C.c_uint32), ("base_launches", C.c_uint32),
                ("cells_bp", C.c_uint64), ("cells_base", C.c_uint64),
                ("cells_tile", C.c_uint64), ("ms_tile", C.c_double),
                ("tile_launches", C.c_uint32), ("tile_tasks", C.c_uint32),
                ("ms_tile_busy", C.c_double), ("streams", C.c_uint32), ("pad_", C.c_uint32),
                ("cells_tile_unique", C.c_uint64), ("ms_bp_busy", C.c_double), ("ms_base_busy", C.c_double),
                ("ms_any_busy", C.c_double), ("p2_launches", C.c_uint32), ("p2_jobs", C.c_uint32), ("p2_more", C.c_uint32),
                ("p2_again", C.c_uint32)]


class Minmer(C.Structure):
    _fields_ = [("hash", C.c_uint64), ("wpos", C.c_int64), ("wpos_end", C.c_int64),
                ("seqId", C.c_int32), ("strand", C.c_int16), ("pad_", C.c_int16)]


POINT_DTYPE = np.dtype([("pos", "<i8"), ("hash", "<u8"), ("seqId", "<i4"), ("side", "i1"), ("pad_", "V3")])


class IndexInfo(C.Structure):
    _fields_ = [("n_windows", C.c_int64), ("n_kept", C.c_int64), ("n_unique", C.c_int64), ("n_points", C.c_int64),
                ("threshold", C.c_uint64), ("filtered", C.c_int64), ("adjusted", C.c_int32), ("pad_", C.c_int32)]


MINMER_DTYPE = np.dtype([("hash", "<u8"), ("wpos", "<i8"), ("wpos_end", "<i8"),
                         ("seqId", "<i4"), ("strand", "<i2"), ("pad_", "<i2")])
L1_DTYPE = np.dtype([("seqId", "<i4"), ("frag", "<i4"), ("rangeStartPos", "<i8"), ("rangeEndPos", "<i8"),
                     ("intersectionSize", "<i4"), ("pad_", "<i4")])


class MapParams(C.Structure):
    pass  # fields set after L1Params / L2Params are defined


MAPPING_DTYPE = np.dtype([("refSeqId", "<u4"), ("refStartPos", "<u4"), ("queryStartPos", "<u4"), ("blockLength", "<u4"),
                          ("n_merged", "<u4"), ("conservedSketches", "<u4"), ("nucIdentity", "<u2"), ("flags", "u1"),
                          ("kmerComplexity", "u1")])


class L2Params(C.Structure):
    _fields_ = [("window_length", C.c_int32), ("sketch_size", C.c_int32), ("stage1_topANI_filter", C.c_int32), ("pad_", C.c_int32),
                ("keep_table", C.c_void_p), ("ident_table", C.c_void_p), ("cutoff_j", C.c_void_p)]


class L1Params(C.Structure):
    _fields_ = [("window_length", C.c_int32), ("sketch_size", C.c_int32), ("min_hits_cached", C.c_int32),
                ("cached_segment_length", C.c_int32), ("skip_self", C.c_int32), ("skip_prefix", C.c_int32),
                ("lower_triangular", C.c_int32), ("stage1_topANI_filter", C.c_int32), ("stage2_full_scan", C.c_int32),
                ("n_seq", C.c_int32), ("ref_group", C.c_void_p), ("min_hits_by_qsketch", C.c_void_p),
                ("sketch_cutoffs", C.c_void_p), ("n_cutoffs", C.c_int32), ("pad_", C.c_int32)]


MapParams._fields_ = [("kmer_size", C.c_int32), ("kmer_complexity_threshold", C.c_float), ("l1", L1Params), ("l2", L2Params)]

# The ctypes prototypes of the record passes and the device objects, name -> (restype, argtypes): every name of EXPORTS from wfm_check_runs
# to wfm_trans_free_list, declared here alone and applied by load()
_VP, _SZ, _INT, _U32, _U64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint64
_PVP, _PSZ, _PU64 = C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)
_FREE1 = (None, [_VP])
_FREE2 = (None, [_VP, _VP])
_ADD = (_INT, [_VP, _VP, _VP, _SZ, _VP, _SZ, _VP])          # handle, object, problems, n, runs, n_runs, flags out
_LIST1 = (_INT, [_VP, _VP, _PVP, _PSZ])                     # handle, object, a list out
_LIST2 = (_INT, [_VP, _VP, _PVP, _PSZ, _PVP, _PSZ])         # handle, object, two lists out
_IMPORT1 = (_INT, [_VP, _VP, _VP, _SZ])
_IMPORT2 = (_INT, [_VP, _VP, _VP, _SZ, _VP, _SZ])
_COUNTS = (_INT, [_VP, _PU64])
PROTOTYPES = {
    "wfm_check_runs": (_INT, [_VP, _VP, _VP, _VP, _VP, _SZ, _VP]),
    "wfm_check_optimal": (_INT, [_VP, _VP, _VP, _VP, _U64, _VP]),
    "wfm_left_align_runs": (_INT, [_VP, _VP, _VP, _VP, _SZ, C.POINTER(C.POINTER(C.c_uint32)), _PSZ, _VP]),
    "wfm_cs_strings": (_INT, [_VP, _VP, _VP, _VP, _SZ, _INT, _PVP, _PSZ, _VP]),
    "wfm_free_cs": _FREE1,
    "wfm_call_variants": (_INT, [_VP, _VP, _VP, _VP, _SZ, _PVP, _PSZ, _PVP, _PSZ, _VP]),
    "wfm_free_variants": _FREE2,
    "wfm_maf_rows": (_INT, [_VP, _VP, _VP, _VP, _SZ, _U32, _PVP, _PSZ, _PVP, _PSZ, _VP]),
    "wfm_free_maf": _FREE2,
    "wfm_coverage_create": (_INT, [_VP, _U64, _PVP]),
    "wfm_coverage_free": _FREE1,
    "wfm_coverage_add": _ADD,
    "wfm_coverage_export": _LIST1,
    "wfm_coverage_import": _IMPORT1,
    "wfm_coverage_intervals": (_INT, [_VP, _VP, _PVP, _PSZ, _PU64]),
    "wfm_coverage_free_list": _FREE1,
    "wfm_liftset_create": (_INT, [_VP, _VP, _SZ, _U64, _PVP]),
    "wfm_liftset_free": _FREE1,
    "wfm_lift_runs": (_INT, [_VP, _VP, _VP, _SZ, _VP, _SZ, _PVP, _PSZ, _VP]),
    "wfm_free_lifts": _FREE1,
    "wfm_chain_runs": (_INT, [_VP, _VP, _SZ, _VP, _SZ, _PVP, _PSZ, _VP]),
    "wfm_free_chain": _FREE1,
    "wfm_pav_create": (_INT, [_VP, _U64, _U32, _PVP]),
    "wfm_pav_free": _FREE1,
    "wfm_pav_add": _ADD,
    "wfm_pav_union": (_INT, [_VP, _VP]),
    "wfm_pav_export": _LIST1,
    "wfm_pav_import": _IMPORT1,
    "wfm_pav_matrix": (_INT, [_VP, _VP, _VP, _SZ, _VP]),
    "wfm_pav_counts": _COUNTS,
    "wfm_pav_free_list": _FREE1,
    "wfm_sites_create": (_INT, [_VP, _U64, _U32, _PVP]),
    "wfm_sites_free": _FREE1,
    "wfm_sites_add_variants": (_INT, [_VP, _VP, _VP, _SZ, C.c_char_p, _SZ]),
    "wfm_sites_add_ref": _ADD,
    "wfm_sites_table": (_INT, [_VP, _VP, _PVP, _PSZ, _PVP, _PSZ, _PVP]),
    "wfm_sites_export": (_INT, [_VP, _VP, _PVP, _PSZ, _PVP, _PSZ, _PVP, _PSZ]),
    "wfm_sites_import": (_INT, [_VP, _VP, _VP, _SZ, C.c_char_p, _SZ, _VP, _SZ]),
    "wfm_sites_counts": _COUNTS,
    "wfm_sites_free_list": _FREE1,
    "wfm_net_create": (_INT, [_VP, _U64, _PVP]),
    "wfm_net_free": _FREE1,
    "wfm_net_add": _ADD,
    "wfm_net_table": _LIST2,
    "wfm_net_export": _LIST2,
    "wfm_net_import": _IMPORT2,
    "wfm_net_counts": _COUNTS,
    "wfm_net_free_list": _FREE1,
    "wfm_trans_create": (_INT, [_VP, _U64, _PVP]),
    "wfm_trans_free": _FREE1,
    "wfm_trans_add": _ADD,
    "wfm_trans_closure": (_INT, [_VP, _VP, _VP, _SZ, _U32, _PVP, _PSZ, _VP]),
    "wfm_trans_export": _LIST2,
    "wfm_trans_import": _IMPORT2,
    "wfm_trans_counts": _COUNTS,
    "wfm_trans_free_list": _FREE1,
}

_LIB = None


def load():
    """Load libwfmash_hip.so; raises if it has not been built."""
    global _LIB, LIB_PATH
    if _LIB is not None:
        return _LIB
    # (WFM_LIB: another build of the same library, for A/B runs of two kernels inside one process launch -- scripts/c3_time.py)
    if os.environ.get("WFM_LIB"):
        LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), os.environ["WFM_LIB"]) if not os.path.isabs(os.environ["WFM_LIB"]) else os.environ["WFM_LIB"]
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.wfm_create.restype = C.c_int
    L.wfm_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.wfm_destroy.restype = None
    L.wfm_destroy.argtypes = [vp]
    L.wfm_last_error.restype = C.c_char_p
    L.wfm_last_error.argtypes = [vp]
    L.wfm_device_name.restype = C.c_int
    L.wfm_device_name.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.wfm_align_arena_bytes.restype = C.c_size_t
    L.wfm_align_arena_bytes.argtypes = [C.POINTER(Problem), C.c_size_t]
    L.wfm_align_batch.restype = C.c_int
    L.wfm_align_batch.argtypes = [vp, C.POINTER(Penalties), C.POINTER(Problem), C.c_size_t,
                                  C.POINTER(Result), vp, C.c_size_t]
    L.wfm_upload_sequences.restype = C.c_int
    L.wfm_upload_sequences.argtypes = [vp, C.POINTER(Problem), C.c_size_t, C.POINTER(vp)]
    L.wfm_free_sequences.restype = None
    L.wfm_free_sequences.argtypes = [vp, vp]
    L.wfm_align_resident.restype = C.c_int
    L.wfm_align_resident.argtypes = [vp, C.POINTER(Penalties), vp, C.POINTER(Result), vp, C.c_size_t]
    L.wfm_get_stats.restype = C.c_int
    L.wfm_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.wfm_hash_kmers.restype = C.c_int
    L.wfm_hash_kmers.argtypes = [vp, vp, C.c_int64, C.c_int, vp, vp]
    L.wfm_sketch_fragments.restype = C.c_int
    L.wfm_sketch_fragments.argtypes = [vp, vp, C.c_int64, vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_int32, vp, vp]
    for name in EXPORTS:  # every symbol include/wfmash_hip.h declares must be exported
        getattr(L, name)
    for name, (restype, argtypes) in PROTOTYPES.items():
        getattr(L, name).restype, getattr(L, name).argtypes = restype, argtypes
    _LIB = L
    return L


class WfmError(RuntimeError):
    pass


class AlignResult:
    __slots__ = ("status", "score", "ops", "n_runs", "cells")

    def __init__(self, status, score, ops, n_runs, cells):
        self.status, self.score, self.ops, self.n_runs, self.cells = status, score, ops, n_runs, cells


def _make_problems(items):
    """items: iterable of (pattern, text) or (pattern, text, mode, pbf, pef, tbf, tef[, score_hint])."""
    items = list(items)
    arr = (Problem * max(len(items), 1))()
    keep = []
    for i, it in enumerate(items):
        p, t = bytes(it[0]), bytes(it[1])
        keep.append((p, t))
        arr[i].pattern, arr[i].plen = p, len(p)
        arr[i].text, arr[i].tlen = t, len(t)
        if len(it) > 2:
            arr[i].mode = it[2]
            if len(it) > 3:
                (arr[i].pattern_begin_free, arr[i].pattern_end_free,
                 arr[i].text_begin_free, arr[i].text_end_free) = it[3:7]
                if len(it) > 7:
                    arr[i].score_hint = it[7]
        else:
            arr[i].mode = WFM_MODE_END2END_BIWFA
    return arr, keep, len(items)


def _result_array(results, n, copy=False):
    """The results of n problems as a ctypes array of Result.  results: such an array (returned as it is, or copied with copy=True: the
    call writes into it), or a list of (status, score, ops_off, ops_len, n_runs)."""
    if isinstance(results, C.Array) and not copy:
        return results
    arr = (Result * max(n, 1))()
    if isinstance(results, C.Array):
        C.memmove(arr, results, C.sizeof(Result) * n)
    else:
        assert len(results) == n, (len(results), n)
        for i, (status, score, ops_off, ops_len, n_runs) in enumerate(results):
            arr[i].status, arr[i].score, arr[i].ops_off, arr[i].ops_len, arr[i].n_runs = status, score, ops_off, ops_len, n_runs
    return arr


def _run_problems(problems, dtype):
    """A list of (base, runs_off, n_runs), (base, runs_off, n_runs, group) or (runs_off, n_runs, flags) as a numpy array of wfm_cov_prob_t /
    wfm_pav_prob_t / wfm_chain_prob_t, and its address (None for an empty list)."""
    probs = np.zeros(len(problems), dtype=dtype)
    for i, p in enumerate(problems):
        probs[i] = tuple(p) + (0,) * (len(dtype.names) - len(p))
    return probs, (probs.ctypes.data if len(probs) else None)


def _make_refs(refs):
    """refs: iterable of ProblemRef, or of dicts keyed by its field names.  A side is either a window of the store
    (pattern_seq / pattern_off / plen[/ pattern_revcomp], likewise text_*) or host bytes (pattern=b"...", text=b"..."; the
    length is taken from them).  mode defaults to END2END_BIWFA."""
    refs = list(refs)
    arr = (ProblemRef * max(len(refs), 1))()
    keep = []
    for i, r in enumerate(refs):
        if isinstance(r, ProblemRef):
            C.memmove(C.byref(arr[i]), C.byref(r), C.sizeof(ProblemRef))
            keep.append(r)
            continue
        a = arr[i]
        a.pattern_seq = a.text_seq = -1
        a.mode = WFM_MODE_END2END_BIWFA
        for k, v in r.items():
            if k in ("pattern", "text") and v is not None:
                v = bytes(v)
                keep.append(v)
                setattr(a, "plen" if k == "pattern" else "tlen", len(v))
            setattr(a, k, v)
    return arr, keep, len(refs)


class SeqSet:
    def __init__(self, handle, items, refs=False, store=None):
        """items: problems as for Handle.align or, with refs, problems by reference as for _make_refs (their windows from store)."""
        self._h = handle
        sp = C.c_void_p()
        if refs:
            self.problems, self._keep, self.n = _make_refs(items)
            f = handle._L.wfm_upload_sequence_refs
            f.restype = C.c_int
            f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(ProblemRef), C.c_size_t, C.POINTER(C.c_void_p)]
            rc = f(handle._p, store._p if store is not None else None, self.problems, self.n, C.byref(sp))
            if rc != 0:
                raise WfmError(f"wfm_upload_sequence_refs failed ({rc}): {handle.last_error()}")
            self.arena_bytes = sum(self.problems[i].plen + self.problems[i].tlen + 1 for i in range(self.n))
        else:
            self.problems, self._keep, self.n = _make_problems(items)
            rc = handle._L.wfm_upload_sequences(handle._p, self.problems, self.n, C.byref(sp))
            if rc != 0:
                raise WfmError(f"wfm_upload_sequences failed ({rc}): {handle.last_error()}")
            self.arena_bytes = handle._L.wfm_align_arena_bytes(self.problems, self.n)
        self._p = sp
        self.arena = np.zeros(self.arena_bytes + 8, dtype=np.uint8)
        self.results = (Result * max(self.n, 1))()

    def download(self):
        """wfm_download_sequences: the seqset's byte buffer (pads, forward and reversed copies) as bytes."""
        f = self._h._L.wfm_download_sequences
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        n = f(self._h._p, self._p, None, 0)
        if n < 0:
            raise WfmError(f"wfm_download_sequences failed ({n}): {self._h.last_error()}")
        out = np.zeros(max(n, 1), dtype=np.uint8)
        n2 = f(self._h._p, self._p, out.ctypes.data, n)
        if n2 != n:
            raise WfmError(f"wfm_download_sequences failed ({n2}): {self._h.last_error()}")
        return out[:n].tobytes()

    def free(self):
        if self._p:
            self._h._L.wfm_free_sequences(self._h._p, self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Index:
    def __init__(self, handle, ptr):
        self._h, self._p = handle, ptr

    def info(self):
        inf = IndexInfo()
        self._h._L.wfm_index_info(self._p, C.byref(inf))
        return inf

    def download(self):
        inf = self.info()
        uh = np.zeros(inf.n_unique, dtype=np.uint64)
        po = np.zeros(inf.n_unique + 1, dtype=np.int64)
        pts = np.zeros(inf.n_points, dtype=POINT_DTYPE)
        mm = np.zeros(inf.n_kept, dtype=MINMER_DTYPE)
        rc = self._h._L.wfm_index_download(self._h._p, self._p, uh.ctypes.data, po.ctypes.data, pts.ctypes.data, mm.ctypes.data)
        if rc != 0:
            raise WfmError(f"wfm_index_download failed ({rc})")
        return uh, po, pts, mm

    def free(self):
        if self._p:
            self._h._L.wfm_index_free(self._h._p, self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


GATHER_TILE = 2048  # WFM_GATHER_TILE (include/wfmash_hip.h): destination records per workgroup of wfm_index_build_parts' gather


class MinmerPart:
    """wfm_minmer_part_t: the records of some sequences, resident on the device of the handle that sketched them."""

    def __init__(self, handle, ptr):
        self._h, self._p = handle, ptr

    def info(self):
        """wfm_minmer_part_info: (number of records, per-sequence counts)."""
        f = self._h._L.wfm_minmer_part_info
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_int64]
        tot = C.c_int64(0)
        nseq = f(self._p, C.byref(tot), None, 0)
        if nseq < 0:
            raise WfmError(f"wfm_minmer_part_info failed ({nseq})")
        counts = np.zeros(max(nseq, 1), dtype=np.int64)
        f(self._p, None, counts.ctypes.data, nseq)
        return tot.value, counts[:nseq]

    def download(self):
        """wfm_minmer_part_download: one array of records per sequence, in the part's order."""
        tot, counts = self.info()
        out = np.zeros(max(tot, 1), dtype=MINMER_DTYPE)
        f = self._h._L.wfm_minmer_part_download
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        n = f(self._h._p, self._p, out.ctypes.data, tot)
        if n != tot:
            raise WfmError(f"wfm_minmer_part_download failed ({n}): {self._h.last_error()}")
        offs = np.concatenate([[0], np.cumsum(counts)])
        return [out[offs[i]:offs[i + 1]] for i in range(len(counts))]

    def free(self):
        if self._p:
            f = self._h._L.wfm_minmer_part_free
            f.restype = None
            f.argtypes = [C.c_void_p]
            f(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class SeqStore:
    """wfm_seqstore_t: whole sequences resident on a handle's device, normalised there (upper case, non-ACGT -> N)."""

    def __init__(self, handle):
        self._h = handle
        L = handle._L
        L.wfm_seqstore_create.restype = C.c_int
        L.wfm_seqstore_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.wfm_seqstore_free.restype = None
        L.wfm_seqstore_free.argtypes = [C.c_void_p]
        L.wfm_seqstore_add.restype = C.c_int32
        L.wfm_seqstore_add.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int64]
        L.wfm_seqstore_info.restype = C.c_int
        L.wfm_seqstore_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        p = C.c_void_p()
        rc = L.wfm_seqstore_create(handle._p, C.byref(p))
        if rc != 0:
            raise WfmError(f"wfm_seqstore_create failed ({rc}): {handle.last_error()}")
        self._p = p

    def add(self, seq: bytes, handle=None) -> int:
        """wfm_seqstore_add: the sequence's id.  handle: another handle of the store's device to add through."""
        h = handle or self._h
        seq = bytes(seq)
        i = h._L.wfm_seqstore_add(h._p, self._p, seq, len(seq))
        if i < 0:
            raise WfmError(f"wfm_seqstore_add failed ({i}): {h.last_error()}")
        return i

    def info(self):
        """wfm_seqstore_info: (sequences held, bytes of their device blocks)."""
        n, b = C.c_int64(0), C.c_int64(0)
        rc = self._h._L.wfm_seqstore_info(self._p, C.byref(n), C.byref(b))
        if rc != 0:
            raise WfmError(f"wfm_seqstore_info failed ({rc})")
        return n.value, b.value

    def free(self):
        if self._p:
            self._h._L.wfm_seqstore_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _DeviceObject:
    """What Coverage, LiftSet, Pav, Sites, Net and Transitive share: the handle, the library and the object's pointer; the calls named
    after _PREFIX (wfm_<prefix>_create / _free / _counts, and _free_list unless _FREE_LIST names another).  Close it before its handle."""
    _PREFIX = None
    _FREE_LIST = None
    _p = None

    def _create(self, handle, *args):
        self._h, self._L = handle, handle._L
        fn = f"wfm_{self._PREFIX}_create"
        p = C.c_void_p()
        rc = getattr(self._L, fn)(handle._p, *args, C.byref(p))
        if rc != 0:
            raise WfmError(f"{fn} failed ({rc}): {handle.last_error()}")
        self._p = p

    def close(self):
        if self._p:
            getattr(self._L, f"wfm_{self._PREFIX}_free")(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, fn, *args, counted=False):
        """fn(handle, object, *args); counted: a positive return value is a count, not an error."""
        rc = getattr(self._L, fn)(self._h._p, self._p, *args)
        if rc < 0 or (rc and not counted):
            raise WfmError(f"{fn} failed ({rc}): {self._h.last_error()}")
        return rc

    def _add(self, fn, problems, dtype, runs, spans):
        """An add that takes runs: the problems as `dtype`, the run words, the problems' flags back; the call returns how many hold `spans`."""
        probs, probs_p = _run_problems(problems, dtype)
        runs = np.ascontiguousarray(runs, dtype=np.uint32)
        flags = np.zeros(max(len(problems), 1), dtype=np.uint32)
        rc = self._call(fn, probs_p, len(probs), runs.ctypes.data if len(runs) else None, len(runs), flags.ctypes.data, counted=True)
        assert rc == int(np.count_nonzero(flags[:len(problems)] & spans))
        return flags[:len(problems)]

    def _take(self, ptr, nbytes):
        try:
            return C.string_at(ptr, nbytes) if nbytes else b""
        finally:
            getattr(self._L, self._FREE_LIST or f"wfm_{self._PREFIX}_free_list")(ptr)

    def _array(self, ptr, n, dtype):
        """a list the library allocated, as a numpy array; the list is freed"""
        return np.frombuffer(self._take(ptr, n.value * dtype.itemsize), dtype=dtype)

    def _counts(self, k):
        fn = f"wfm_{self._PREFIX}_counts"
        out = (C.c_uint64 * k)()
        rc = getattr(self._L, fn)(self._p, out)
        if rc != 0:
            raise WfmError(f"{fn} failed ({rc})")
        return tuple(int(v) for v in out)


def _interval_array(intervals):
    """[(start, end)] as an array of wfm_lift_iv_t, and its address (None for an empty list)"""
    iv = np.zeros(len(intervals), dtype=LIFT_IV_DTYPE)
    for i, (a, b) in enumerate(intervals):
        iv[i] = (a, b)
    return iv, (iv.ctypes.data if len(iv) else None)


def _take_lists(free, *lists):
    """The outputs of an emitting call, each (pointer, bytes), as bytes objects; then free(*pointers)."""
    try:
        return [C.string_at(p, nbytes) if nbytes else b"" for p, nbytes in lists]
    finally:
        free(*(p for p, _ in lists))


class Coverage(_DeviceObject):
    """wfm_coverage_t: per-base depth of n_bases target bases, summed on the device over every problem added (include/wfmash_hip.h).
    Close it before its handle."""
    _PREFIX = "coverage"

    def __init__(self, handle, n_bases):
        self.n_bases = int(n_bases)
        self._create(handle, self.n_bases)

    def add(self, problems, runs):
        """wfm_coverage_add.  problems: a list of (base, runs_off, n_runs); runs: the run words ((length << 2) | op).  Returns the
        problems' flags as a numpy array (WFM_COV_SPANS: nothing of the problem was added)."""
        return self._add("wfm_coverage_add", problems, COV_PROB_DTYPE, runs, WFM_COV_SPANS)

    def export(self):
        """wfm_coverage_export: the non-zero words of the difference array, ascending, as a numpy array with the fields of CovEntry."""
        ptr, n = C.c_void_p(), C.c_size_t(0)
        self._call("wfm_coverage_export", C.byref(ptr), C.byref(n))
        return self._array(ptr, n, COV_ENTRY_DTYPE)

    def import_entries(self, entries):
        """wfm_coverage_import: such a list (of another object, of another device) added into this one."""
        e = np.ascontiguousarray(entries, dtype=COV_ENTRY_DTYPE)
        self._call("wfm_coverage_import", e.ctypes.data if len(e) else None, len(e))

    def intervals(self):
        """wfm_coverage_intervals: (the maximal intervals of constant depth as a numpy array with the fields of CovInterval,
        (covered bases, sum of depth, max depth))."""
        ptr, n = C.c_void_p(), C.c_size_t(0)
        tot = (C.c_uint64 * 3)()
        self._call("wfm_coverage_intervals", C.byref(ptr), C.byref(n), tot)
        return self._array(ptr, n, COV_INTERVAL_DTYPE), tuple(int(v) for v in tot)


class LiftSet(_DeviceObject):
    """wfm_liftset_t: sorted intervals [(start, end)] over n_bases target bases, on the handle's device (include/wfmash_hip.h).  Close it
    before its handle."""
    _PREFIX = "liftset"
    _FREE_LIST = "wfm_free_lifts"

    def __init__(self, handle, intervals, n_bases):
        self.n_bases = int(n_bases)
        iv, iv_p = _interval_array(intervals)
        self.n = len(iv)
        self._create(handle, iv_p, len(iv), self.n_bases)

    def lift(self, problems, runs):
        """wfm_lift_runs.  problems: a list of (base, runs_off, n_runs); runs: the run words ((length << 2) | op).  Returns (the lifts as
        a numpy array with the fields of Lift, the problems' records as one with the fields of LiftCall)."""
        probs, probs_p = _run_problems(problems, COV_PROB_DTYPE)
        runs = np.ascontiguousarray(runs, dtype=np.uint32)
        per = np.zeros(max(len(problems), 1), dtype=LIFTCALL_DTYPE)
        ptr, n = C.c_void_p(), C.c_size_t(0)
        try:
            self._call("wfm_lift_runs", probs_p, len(probs), runs.ctypes.data if len(runs) else None, len(runs), C.byref(ptr), C.byref(n), per.ctypes.data)
        except WfmError:
            assert not ptr.value and n.value == 0
            raise
        return self._array(ptr, n, LIFT_DTYPE), per[:len(problems)]


class Pav(_DeviceObject):
    """wfm_pav_t: per group the union of the aligned bases of every problem added, as segments on the handle's device, over n_bases target
    bases and n_groups groups (include/wfmash_hip.h).  Close it before its handle."""
    _PREFIX = "pav"

    def __init__(self, handle, n_bases, n_groups):
        self.n_bases, self.n_groups = int(n_bases), int(n_groups)
        if not 0 <= self.n_groups < (1 << 32):
            raise WfmError(f"wfm_pav_create: {self.n_groups} groups do not fit 32 bits")
        self._create(handle, self.n_bases, self.n_groups)

    def add(self, problems, runs):
        """wfm_pav_add.  problems: a list of (base, runs_off, n_runs, group); runs: the run words ((length << 2) | op).  Returns the
        problems' flags as a numpy array (WFM_PAV_SPANS: nothing of the problem was added)."""
        return self._add("wfm_pav_add", problems, PAV_PROB_DTYPE, runs, WFM_PAV_SPANS)

    def union(self):
        """wfm_pav_union: the list becomes the disjoint union per group."""
        self._call("wfm_pav_union")

    def export(self):
        """wfm_pav_export: the union sorted by (group, start) as a numpy array with the fields {start, length, group}."""
        ptr, n = C.c_void_p(), C.c_size_t(0)
        self._call("wfm_pav_export", C.byref(ptr), C.byref(n))
        return self._array(ptr, n, PAV_SEG_DTYPE)

    def import_(self, segs):
        """wfm_pav_import: such a list (of another object, of another device) appended as raw segments."""
        e = np.ascontiguousarray(segs, dtype=PAV_SEG_DTYPE)
        self._call("wfm_pav_import", e.ctypes.data if len(e) else None, len(e))

    def matrix(self, intervals):
        """wfm_pav_matrix.  intervals: a list of (start, end), global and half-open.  Returns a numpy array [interval, group] of the
        covered bases."""
        iv, iv_p = _interval_array(intervals)
        out = np.zeros((len(iv), self.n_groups), dtype=np.uint32)
        self._call("wfm_pav_matrix", iv_p, len(iv), out.ctypes.data if out.size else None)
        return out

    def counts(self):
        """wfm_pav_counts: (segments added, union intervals after the last union, unions run)."""
        return self._counts(3)


class Sites(_DeviceObject):
    """wfm_sites_t: the variants of many records (global position, group, alleles) and the = runs of the same records, on the handle's device;
    .table() joins them into distinct sites and a sites x groups table of '0' / '1' / '.' (include/wfmash_hip.h).  Close it before its handle."""
    _PREFIX = "sites"

    def __init__(self, handle, n_bases, n_groups):
        self.n_bases, self.n_groups = int(n_bases), int(n_groups)
        if not 0 <= self.n_groups < (1 << 32):
            raise WfmError(f"wfm_sites_create: {self.n_groups} groups do not fit 32 bits")
        self._create(handle, self.n_bases, self.n_groups)

    @staticmethod
    def pack(variants):
        """[(pos, kind, group, ref bytes, alt bytes)] as (an array of wfm_site_var_t, the allele bytes)"""
        v = np.zeros(len(variants), dtype=SITE_VAR_DTYPE)
        parts, at = [], 0
        for i, (pos, kind, group, ref, alt) in enumerate(variants):
            v[i] = (pos, kind, group, len(ref), len(alt), at)
            parts += [ref, alt]
            at += len(ref) + len(alt)
        return v, b"".join(parts)

    def add_variants(self, variants, alleles=None):
        """wfm_sites_add_variants.  variants: a list of (pos, kind, group, ref bytes, alt bytes), or, with `alleles`, an array of
        wfm_site_var_t whose off point into those bytes."""
        v, a = self.pack(variants) if alleles is None else (np.ascontiguousarray(variants, dtype=SITE_VAR_DTYPE), bytes(alleles))
        self._call("wfm_sites_add_variants", v.ctypes.data if len(v) else None, len(v), a if a else None, len(a))

    def add_ref(self, problems, runs):
        """wfm_sites_add_ref: Pav.add's arguments and flags; the = runs alone make segments."""
        return self._add("wfm_sites_add_ref", problems, PAV_PROB_DTYPE, runs, WFM_PAV_SPANS)

    def table(self):
        """wfm_sites_table: (sites as an array of wfm_site_t in ascending pos, their allele bytes, gt as a uint8 array [site, group] of
        b'0' / b'1' / b'.')."""
        sp, ap, gp, n, nb = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_size_t(0)
        self._call("wfm_sites_table", C.byref(sp), C.byref(n), C.byref(ap), C.byref(nb), C.byref(gp))
        if n.value == 0:
            assert not sp.value and not ap.value and not gp.value and nb.value == 0
        sites = self._array(sp, n, SITE_DTYPE)
        alleles = self._take(ap, nb.value)
        gt = np.frombuffer(self._take(gp, n.value * self.n_groups), dtype=np.uint8).reshape(n.value, self.n_groups)
        return sites, alleles, gt

    def export(self):
        """wfm_sites_export: (the raw variants as an array of wfm_site_var_t, their folded allele bytes, the = union as Pav.export gives it)."""
        vp, ap, gp, n, nb, ns = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._call("wfm_sites_export", C.byref(vp), C.byref(n), C.byref(ap), C.byref(nb), C.byref(gp), C.byref(ns))
        return self._array(vp, n, SITE_VAR_DTYPE), self._take(ap, nb.value), self._array(gp, ns, PAV_SEG_DTYPE)

    def import_(self, variants, alleles, segs):
        """wfm_sites_import: what export returned (of another object, of another device), appended."""
        v = np.ascontiguousarray(variants, dtype=SITE_VAR_DTYPE)
        e = np.ascontiguousarray(segs, dtype=PAV_SEG_DTYPE)
        a = bytes(alleles)
        self._call("wfm_sites_import", v.ctypes.data if len(v) else None, len(v), a if a else None, len(a), e.ctypes.data if len(e) else None, len(e))

    def counts(self):
        """wfm_sites_counts: (variants added, distinct sites of the last table, = union intervals after the last union, collisions of the last table)."""
        return self._counts(4)


class Net(_DeviceObject):
    """wfm_net_t: the blocks of many records, each with a score and a unique order, on the handle's device; .table() gives every target
    base to the best record over it and returns the pieces that are left (include/wfmash_hip.h).  Close it before its handle."""
    _PREFIX = "net"

    def __init__(self, handle, n_bases):
        self.n_bases = int(n_bases)
        self._create(handle, self.n_bases)

    def add(self, problems, runs):
        """wfm_net_add.  problems: a list of (base, runs_off, n_runs, score, order), score WFM_NET_SCORE_EQ for the = columns; runs: the run
        words ((length << 2) | op).  Returns the problems' flags as a numpy array (WFM_NET_SPANS: nothing of the problem was added)."""
        return self._add("wfm_net_add", problems, NET_PROB_DTYPE, runs, WFM_NET_SPANS)

    def table(self):
        """wfm_net_table: (the pieces {order, t, q, size} sorted by (order, t), the records {order, score, zero, first, count, bases_won,
        bases_aligned} sorted by order), two numpy arrays."""
        pp, rp, n, nr = C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_size_t(0)
        self._call("wfm_net_table", C.byref(pp), C.byref(n), C.byref(rp), C.byref(nr))
        if n.value == 0:
            assert not pp.value
        if nr.value == 0:
            assert not rp.value and n.value == 0
        return self._array(pp, n, NET_BLOCK_DTYPE), self._array(rp, nr, NET_CALL_DTYPE)

    def export(self):
        """wfm_net_export: (the raw blocks as an array of wfm_net_block_t, the record entries as an array of wfm_net_rec_t)."""
        bp, rp, n, nr = C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_size_t(0)
        self._call("wfm_net_export", C.byref(bp), C.byref(n), C.byref(rp), C.byref(nr))
        return self._array(bp, n, NET_BLOCK_DTYPE), self._array(rp, nr, NET_REC_DTYPE)

    def import_(self, blocks, recs):
        """wfm_net_import: what export returned (of another object, of another device), appended."""
        b = np.ascontiguousarray(blocks, dtype=NET_BLOCK_DTYPE)
        r = np.ascontiguousarray(recs, dtype=NET_REC_DTYPE)
        self._call("wfm_net_import", b.ctypes.data if len(b) else None, len(b), r.ctypes.data if len(r) else None, len(r))

    def counts(self):
        """wfm_net_counts: (records, blocks, and of the last table: elementary intervals, pieces, records that won nothing)."""
        return self._counts(6)[:5]


class Transitive(_DeviceObject):
    """wfm_trans_t: the records of a run as arcs of one coordinate space, on the handle's device; .closure(seeds, depth) gives per seed
    interval everything it reaches through any chain of records, either way (include/wfmash_hip.h).  Close it before its handle."""
    _PREFIX = "trans"

    def __init__(self, handle, n_bases):
        self.n_bases = int(n_bases)
        self._create(handle, self.n_bases)

    def add(self, problems, runs):
        """wfm_trans_add.  problems: a list of (t, q, runs_off, n_runs, flags), flags WFM_TRANS_REVERSE or 0; runs: the run words
        ((length << 2) | op).  Returns the problems' flags as a numpy array (WFM_TRANS_SPANS: nothing of the problem was added)."""
        return self._add("wfm_trans_add", problems, TRANS_PROB_DTYPE, runs, WFM_TRANS_SPANS)

    def closure(self, seeds, depth=2):
        """wfm_trans_closure: seeds = [(start, end)] in world coordinates; depth 0 walks to the fixed point.  Returns (the intervals {start,
        end, seed} sorted by (seed, start), per seed {first, count, bases}), two numpy arrays."""
        iv, iv_p = _interval_array(seeds)
        per = np.zeros(max(len(seeds), 1), dtype=TRANS_SEED_DTYPE)
        pp, n = C.c_void_p(), C.c_size_t(0)
        self._call("wfm_trans_closure", iv_p, len(iv), int(depth), C.byref(pp), C.byref(n), per.ctypes.data)
        return self._array(pp, n, TRANS_IV_DTYPE), per[:len(seeds)]

    def export(self):
        """wfm_trans_export: (the records as an array of wfm_trans_rec_t, their prefix words as an array of wfm_trans_word_t)."""
        rp, wp, n, nw = C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_size_t(0)
        self._call("wfm_trans_export", C.byref(rp), C.byref(n), C.byref(wp), C.byref(nw))
        return self._array(rp, n, TRANS_REC_DTYPE), self._array(wp, nw, TRANS_WORD_DTYPE)

    def import_(self, recs, words):
        """wfm_trans_import: what export returned (of another object, of another device), appended."""
        r = np.ascontiguousarray(recs, dtype=TRANS_REC_DTYPE)
        w = np.ascontiguousarray(words, dtype=TRANS_WORD_DTYPE)
        self._call("wfm_trans_import", r.ctypes.data if len(r) else None, len(r), w.ctypes.data if len(w) else None, len(w))

    def counts(self):
        """wfm_trans_counts: (records, prefix words, arcs, and of the last closure: rounds run, intervals returned, pairs projected)."""
        return self._counts(6)


class Handle:
    """One handle per GPU (wfm_create)."""

    def __init__(self, device=0):
        self._L = load()
        p = C.c_void_p()
        rc = self._L.wfm_create(device, C.byref(p))
        if rc != 0:
            raise WfmError(f"wfm_create(device={device}) failed with {rc}: no usable gfx950 device "
                           "(there is no CPU fallback)")
        self._p = p

    def close(self):
        if self._p:
            self._L.wfm_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._L.wfm_last_error(self._p).decode()

    def device_name(self):
        buf = C.create_string_buffer(256)
        self._L.wfm_device_name(self._p, buf, 256)
        return buf.value.decode()

    def stats(self):
        st = Stats()
        self._L.wfm_get_stats(self._p, C.byref(st))
        return st

    def problem_flags(self, n):
        """wfm_get_problem_flags: WFM_PF_* bits of the problems of the handle's last align call."""
        f = self._L.wfm_get_problem_flags
        f.restype = C.c_size_t
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        out = np.zeros(max(n, 1), dtype=np.uint32)
        have = f(self._p, out.ctypes.data, n)
        return out[:min(n, have)]

    def tile_counters(self):
        """wfm_get_tile_counters: which paths the tile phase took in the handle's last align call, by the names of TILE_COUNTERS."""
        f = self._L.wfm_get_tile_counters
        f.restype = C.c_size_t
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        out = np.zeros(len(TILE_COUNTERS), dtype=np.uint64)
        have = f(self._p, out.ctypes.data, len(out))
        # (an older build of the library named by WFM_LIB_PATH or WFM_LIB -- A/B runs, scripts/driver_ab.py -- ends before the reuse counters, which
        # then read 0; the package's own library must know every counter)
        other_build = bool(os.environ.get("WFM_LIB_PATH") or os.environ.get("WFM_LIB"))
        assert have == len(TILE_COUNTERS) or (other_build and 8 <= have < len(TILE_COUNTERS)), have
        return {k: int(v) for k, v in zip(TILE_COUNTERS, out)}

    def upload(self, items):
        return SeqSet(self, items)

    def seqstore(self):
        """wfm_seqstore_create: a store of device-resident sequences on this handle's device."""
        return SeqStore(self)

    def upload_refs(self, store, refs):
        """wfm_upload_sequence_refs: a SeqSet from problems by reference (see _make_refs); store may be None when every side is host bytes."""
        return SeqSet(self, refs, refs=True, store=store)

    def align_refs(self, store, refs, pen=None):
        """wfm_align_refs_rle: problems by reference; returns the same [AlignResult] as align (the runs spelled out as an op string)."""
        arr, keep, n = _make_refs(refs)
        pn = Penalties(*(pen or DEFAULT_PEN))
        res = (Result * max(n, 1))()
        runs = C.POINTER(C.c_uint32)()
        total = C.c_size_t(0)
        f = self._L.wfm_align_refs_rle
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ProblemRef), C.c_size_t, C.c_void_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_size_t)]
        self._L.wfm_free_runs.restype = None
        self._L.wfm_free_runs.argtypes = [C.POINTER(C.c_uint32)]
        rc = f(self._p, C.byref(pn), store._p if store is not None else None, arr, n, res, C.byref(runs), C.byref(total))
        if rc < 0:
            raise WfmError(f"wfm_align_refs_rle failed ({rc}): {self.last_error()}")
        try:
            a = np.ctypeslib.as_array(runs, shape=(total.value,)).copy() if total.value else np.zeros(0, dtype=np.uint32)
        finally:
            self._L.wfm_free_runs(runs)
        opc = np.frombuffer(b"MXID", dtype=np.uint8)
        out = []
        for i in range(n):
            r = res[i]
            ops = None
            if r.status == 0:
                mine = a[r.ops_off:r.ops_off + r.n_runs]
                ops = np.repeat(opc[mine & 3], mine >> 2).tobytes() if r.n_runs else b""
            out.append(AlignResult(r.status, r.score, ops, r.n_runs, r.cells))
        return out

    def align_resident(self, seqset, pen=None, collect=True):
        pn = Penalties(*(pen or DEFAULT_PEN))
        rc = self._L.wfm_align_resident(self._p, C.byref(pn), seqset._p, seqset.results,
                                        seqset.arena.ctypes.data, seqset.arena_bytes)
        if rc < 0:
            raise WfmError(f"wfm_align_resident failed ({rc}): {self.last_error()}")
        if not collect:
            return rc
        return self._collect(seqset)

    @staticmethod
    def _collect(seqset):
        out = []
        a = seqset.arena
        for i in range(seqset.n):
            r = seqset.results[i]
            ops = a[r.ops_off:r.ops_off + r.ops_len].tobytes() if r.status == 0 else None
            out.append(AlignResult(r.status, r.score, ops, r.n_runs, r.cells))
        return out

    def align(self, items, pen=None):
        """items: list of (pattern, text[, mode, pbf, pef, tbf, tef]). Returns [AlignResult]."""
        probs, keep, n = _make_problems(items)
        pn = Penalties(*(pen or DEFAULT_PEN))
        nbytes = self._L.wfm_align_arena_bytes(probs, n)
        arena = np.zeros(nbytes + 8, dtype=np.uint8)
        res = (Result * max(n, 1))()
        rc = self._L.wfm_align_batch(self._p, C.byref(pn), probs, n, res, arena.ctypes.data, nbytes)
        if rc < 0:
            raise WfmError(f"wfm_align_batch failed ({rc}): {self.last_error()}")
        out = []
        for i in range(n):
            r = res[i]
            ops = arena[r.ops_off:r.ops_off + r.ops_len].tobytes() if r.status == 0 else None
            out.append(AlignResult(r.status, r.score, ops, r.n_runs, r.cells))
        return out

    def scores(self, items, pen=None, limit=None):
        """The optimal scores alone (WFM_MODE_SCORE_ONLY on every item): returns [(status, score)].  With `limit` the BiWFA items
        run under it as a hard limit (WFM_MODE_SCORE_LIMIT): status WFM_ST_MAX_SCORE and score -1 where the score is beyond it."""
        flagged = []
        for it in items:
            it = tuple(it)
            mode = it[2] if len(it) > 2 else WFM_MODE_END2END_BIWFA
            free = tuple(it[3:7]) if len(it) > 3 else (0, 0, 0, 0)
            hint = it[7] if len(it) > 7 else 0
            if limit is not None and (mode & WFM_MODE_MASK) == WFM_MODE_END2END_BIWFA:
                mode, hint = mode | WFM_MODE_SCORE_LIMIT, limit
            flagged.append((it[0], it[1], mode | WFM_MODE_SCORE_ONLY) + free + (hint,))
        probs, keep, n = _make_problems(flagged)
        pn = Penalties(*(pen or DEFAULT_PEN))
        res = (Result * max(n, 1))()
        f = self._L.wfm_align_batch
        rc = f(self._p, C.byref(pn), probs, n, res, None, 0)
        if rc < 0:
            raise WfmError(f"wfm_align_batch failed ({rc}): {self.last_error()}")
        return [(res[i].status, res[i].score) for i in range(n)]

    def score_bounds(self, items, pen=None):
        """wfm_score_bounds: per (pattern, text) an upper bound of the end-to-end score, or -1."""
        probs, keep, n = _make_problems(items)
        pn = Penalties(*(pen or DEFAULT_PEN))
        out = np.zeros(max(n, 1), dtype=np.int32)
        f = self._L.wfm_score_bounds
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        rc = f(self._p, C.byref(pn), probs, n, out.ctypes.data)
        if rc < 0:
            raise WfmError(f"wfm_score_bounds failed ({rc}): {self.last_error()}")
        return out[:n]

    def align_resident_rle(self, seqset, pen=None):
        """wfm_align_resident_rle: fills seqset.results (ops_off / n_runs index the runs) and returns (failed, runs as a uint32 array)."""
        pn = Penalties(*(pen or DEFAULT_PEN))
        runs = C.POINTER(C.c_uint32)()
        total = C.c_size_t(0)
        f = self._L.wfm_align_resident_rle
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_size_t)]
        self._L.wfm_free_runs.restype = None
        self._L.wfm_free_runs.argtypes = [C.POINTER(C.c_uint32)]
        rc = f(self._p, C.byref(pn), seqset._p, seqset.results, C.byref(runs), C.byref(total))
        if rc < 0:
            raise WfmError(f"wfm_align_resident_rle failed ({rc}): {self.last_error()}")
        try:
            arr = np.ctypeslib.as_array(runs, shape=(total.value,)).copy() if total.value else np.zeros(0, dtype=np.uint32)
        finally:
            self._L.wfm_free_runs(runs)
        return rc, arr

    def check_runs(self, seqset, results, runs, pen=None):
        """wfm_check_runs: every run held against the bases it covers.  results: a ctypes array of Result (seqset.results after an
        align call) or a list of (status, score, ops_off, ops_len, n_runs), one per problem of the seqset; runs: uint32 runs,
        (length << 2) | op.  Returns (flagged, [Check])."""
        n = seqset.n
        results = _result_array(results, n)
        runs = np.ascontiguousarray(runs, dtype=np.uint32)
        pn = Penalties(*(pen or DEFAULT_PEN))
        out = (Check * max(n, 1))()
        rc = self._L.wfm_check_runs(self._p, C.byref(pn), seqset._p, results, runs.ctypes.data if len(runs) else None, len(runs), out)
        if rc < 0:
            raise WfmError(f"wfm_check_runs failed ({rc}): {self.last_error()}")
        return rc, [out[i] for i in range(n)]

    def left_align(self, seqset, results, runs):
        """wfm_left_align_runs: every interior gap moved to its leftmost placement.  results and runs as for check_runs (a list of
        (status, score, ops_off, ops_len, n_runs) is copied; a ctypes array of Result is copied as well: the caller's stays as it is).
        Returns (results: a new ctypes array of Result whose ops_off / n_runs locate the problems in the new runs, runs: uint32 array,
        stats: [LeftAlign], one per problem)."""
        n = seqset.n
        arr = _result_array(results, n, copy=True)
        runs = np.ascontiguousarray(runs, dtype=np.uint32)
        out = (LeftAlign * max(n, 1))()
        new = C.POINTER(C.c_uint32)()
        total = C.c_size_t(0)
        self._L.wfm_free_runs.restype = None
        self._L.wfm_free_runs.argtypes = [C.POINTER(C.c_uint32)]
        rc = self._L.wfm_left_align_runs(self._p, seqset._p, arr, runs.ctypes.data if len(runs) else None, len(runs), C.byref(new), C.byref(total), out)
        if rc < 0:
            raise WfmError(f"wfm_left_align_runs failed ({rc}): {self.last_error()}")
        try:
            a = np.ctypeslib.as_array(new, shape=(total.value,)).copy() if total.value else np.zeros(0, dtype=np.uint32)
        finally:
            self._L.wfm_free_runs(new)
        return arr, a, [out[i] for i in range(n)]

    def cs_strings(self, seqset, results, runs, form):
        """wfm_cs_strings: minimap2's cs difference string of every problem's runs, spelled on the device.  results and runs as for
        check_runs; form: WFM_CS_SHORT or WFM_CS_LONG.  Returns (the strings as bytes, one per problem -- b"" for a flagged one --,
        [Cs], one per problem)."""
        n = seqset.n
        arr = _result_array(results, n, copy=True)
        runs = np.ascontiguousarray(runs, dtype=np.uint32)
        per = (Cs * max(n, 1))()
        text = C.c_void_p()
        total = C.c_size_t(0)
        rc = self._L.wfm_cs_strings(self._p, seqset._p, arr, runs.ctypes.data if len(runs) else None, len(runs), int(form), C.byref(text), C.byref(total), per)
        if rc < 0:
            raise WfmError(f"wfm_cs_strings failed ({rc}): {self.last_error()}")
        blob, = _take_lists(self._L.wfm_free_cs, (text, total.value))
        return [blob[per[i].off:per[i].off + per[i].len] for i in range(n)], [per[i] for i in range(n)]

    def call_variants(self, seqset, results, runs):
        """wfm_call_variants: the SNVs, insertions and deletions of every problem's runs, called on the device.  results and runs as for
        check_runs.  Returns (records: a numpy structured array with the fields of Variant, alleles: all allele bytes as bytes,
        [VarCall], one per problem)."""
        n = seqset.n
        arr = _result_array(results, n, copy=True)
        runs = np.ascontiguousarray(runs, dtype=np.uint32)
        per = (VarCall * max(n, 1))()
        recs, alleles = C.c_void_p(), C.c_void_p()
        n_recs, n_bytes = C.c_size_t(0), C.c_size_t(0)
        rc = self._L.wfm_call_variants(self._p, seqset._p, arr, runs.ctypes.data if len(runs) else None, len(runs), C.byref(recs), C.byref(n_recs),
                                       C.byref(alleles), C.byref(n_bytes), per)
        if rc < 0:
            raise WfmError(f"wfm_call_variants failed ({rc}): {self.last_error()}")
        raw, blob = _take_lists(self._L.wfm_free_variants, (recs, n_recs.value * C.sizeof(Variant)), (alleles, n_bytes.value))
        return np.frombuffer(raw, dtype=VARIANT_DTYPE), blob, [per[i] for i in range(n)]

    def maf_rows(self, seqset, results, runs, split=0):
        """wfm_maf_rows: the two gapped rows of every problem's runs in the blocks of a pairwise MAF, spelled on the device.  results and
        runs as for check_runs; split: 0, or the gap bases from which a gap stretch breaks a block.  Returns (blocks: a numpy structured
        array with the fields of MafBlock, rows: all row bytes as bytes, [MafCall], one per problem)."""
        n = seqset.n
        arr = _result_array(results, n, copy=True)
        runs = np.ascontiguousarray(runs, dtype=np.uint32)
        per = (MafCall * max(n, 1))()
        blocks, rows = C.c_void_p(), C.c_void_p()
        n_blocks, n_bytes = C.c_size_t(0), C.c_size_t(0)
        rc = self._L.wfm_maf_rows(self._p, seqset._p, arr, runs.ctypes.data if len(runs) else None, len(runs), int(split), C.byref(blocks), C.byref(n_blocks),
                                  C.byref(rows), C.byref(n_bytes), per)
        if rc < 0:
            assert not blocks.value and not rows.value and n_blocks.value == 0 and n_bytes.value == 0
            raise WfmError(f"wfm_maf_rows failed ({rc}): {self.last_error()}")
        raw, blob = _take_lists(self._L.wfm_free_maf, (blocks, n_blocks.value * C.sizeof(MafBlock)), (rows, n_bytes.value))
        return np.frombuffer(raw, dtype=MAF_BLOCK_DTYPE), blob, [per[i] for i in range(n)]

    def chain_runs(self, problems, runs):
        """wfm_chain_runs: the blocks and gaps of a UCSC chain from every problem's runs.  problems: a list of (runs_off, n_runs, flags),
        flags of WFM_CHAIN_SWAP and WFM_CHAIN_REVERSE; runs: the run words ((length << 2) | op).  Returns (the blocks as a numpy array with
        CHAIN_BLOCK_DTYPE, the problems' records as one with CHAINCALL_DTYPE)."""
        probs, probs_p = _run_problems(problems, CHAIN_PROB_DTYPE)
        runs = np.ascontiguousarray(runs, dtype=np.uint32)
        per = np.zeros(max(len(problems), 1), dtype=CHAINCALL_DTYPE)
        ptr, n = C.c_void_p(), C.c_size_t(0)
        rc = self._L.wfm_chain_runs(self._p, probs_p, len(probs), runs.ctypes.data if len(runs) else None, len(runs), C.byref(ptr), C.byref(n), per.ctypes.data)
        if rc != 0:
            assert not ptr.value and n.value == 0
            raise WfmError(f"wfm_chain_runs failed ({rc}): {self.last_error()}")
        raw, = _take_lists(self._L.wfm_free_chain, (ptr, n.value * CHAIN_BLOCK_DTYPE.itemsize))
        return np.frombuffer(raw, dtype=CHAIN_BLOCK_DTYPE), per[:len(problems)]

    def liftset(self, intervals, n_bases):
        """wfm_liftset_create: the sorted intervals [(start, end)] over n_bases target bases on this handle's device; .lift(problems, runs)
        lifts them through runs, .close() frees the set."""
        return LiftSet(self, intervals, n_bases)

    def pav(self, n_bases, n_groups):
        """wfm_pav_create: a presence object over n_bases target bases and n_groups groups on this handle's device; .add, .union, .export,
        .import_, .matrix, .counts, .close."""
        return Pav(self, n_bases, n_groups)

    def sites(self, n_bases, n_groups):
        """wfm_sites_create: a sites object over n_bases target bases and n_groups groups on this handle's device; .add_variants, .add_ref,
        .table, .export, .import_, .counts, .close."""
        return Sites(self, n_bases, n_groups)

    def net(self, n_bases):
        """A Net on this handle's device over n_bases target bases (wfm_net_create)."""
        return Net(self, n_bases)

    def transitive(self, n_bases):
        """A Transitive on this handle's device over a world of n_bases bases (wfm_trans_create)."""
        return Transitive(self, n_bases)

    def coverage(self, n_bases):
        """wfm_coverage_create: a depth object over n_bases target bases on this handle's device."""
        return Coverage(self, n_bases)

    def check_optimal(self, seqset, results, pen=None, max_cells=0):
        """wfm_check_optimal: every score held against a banded DP on the device.  results: a ctypes array of Result (seqset.results after
        an align call), or a list of (status, score) or plain scores, one per problem of the seqset.  Returns the list of OptCheck records
        (flags, dp_score, band_lo, band_hi, cells)."""
        n = seqset.n
        if not isinstance(results, C.Array):
            results = _result_array([(r if isinstance(r, tuple) else (0, r)) + (0, 0, 0) for r in results], n)
        pn = Penalties(*(pen or DEFAULT_PEN))
        out = (OptCheck * max(n, 1))()
        rc = self._L.wfm_check_optimal(self._p, C.byref(pn), seqset._p, results, int(max_cells), out)
        if rc < 0:
            raise WfmError(f"wfm_check_optimal failed ({rc}): {self.last_error()}")
        return [out[i] for i in range(n)]

    def align_rle(self, items, pen=None):
        """wfm_align_batch_rle: the same problems, run-length output.  AlignResult.ops is the list of (length, op) runs
        with op in b'MXID' (adjacent runs never share an op), .n_runs their number; `ops_len` travels as an extra
        attribute on the tuple: returns [(AlignResult, ops_len)]."""
        probs, keep, n = _make_problems(items)
        pn = Penalties(*(pen or DEFAULT_PEN))
        res = (Result * max(n, 1))()
        runs = C.POINTER(C.c_uint32)()
        total = C.c_size_t(0)
        f = self._L.wfm_align_batch_rle
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_size_t)]
        self._L.wfm_free_runs.restype = None
        self._L.wfm_free_runs.argtypes = [C.POINTER(C.c_uint32)]
        rc = f(self._p, C.byref(pn), probs, n, res, C.byref(runs), C.byref(total))
        if rc < 0:
            raise WfmError(f"wfm_align_batch_rle failed ({rc}): {self.last_error()}")
        try:
            arr = np.ctypeslib.as_array(runs, shape=(total.value,)).copy() if total.value else np.zeros(0, dtype=np.uint32)
        finally:
            self._L.wfm_free_runs(runs)
        out = []
        for i in range(n):
            r = res[i]
            ops = None
            if r.status == 0 and probs[i].mode & WFM_MODE_SCORE_ONLY:
                ops = b""  # (no runs were asked for)
            elif r.status == 0:
                mine = arr[r.ops_off:r.ops_off + r.n_runs]
                ops = [(int(x) >> 2, b"MXID"[int(x) & 3:(int(x) & 3) + 1]) for x in mine]
            out.append((AlignResult(r.status, r.score, ops, r.n_runs, r.cells), int(r.ops_len)))
        return out

    # ---- map path ----
    def hash_kmers(self, seq: bytes, k: int):
        n = max(len(seq) - k + 1, 0)
        hashes = np.zeros(n, dtype=np.uint64)
        strand = np.zeros(n, dtype=np.int8)
        buf = np.frombuffer(seq, dtype=np.uint8)
        rc = self._L.wfm_hash_kmers(self._p, buf.ctypes.data, len(seq), k, hashes.ctypes.data, strand.ctypes.data)
        if rc < 0:
            raise WfmError(f"wfm_hash_kmers failed ({rc}): {self.last_error()}")
        return hashes, strand

    def sketch_fragments(self, seq: bytes, frag_off, frag_len, k: int, s: int, seq_id: int = 0):
        frag_off = np.ascontiguousarray(frag_off, dtype=np.int64)
        frag_len = np.ascontiguousarray(frag_len, dtype=np.int32)
        n = len(frag_off)
        out = np.zeros(n * s, dtype=MINMER_DTYPE)
        cnt = np.zeros(n, dtype=np.int32)
        buf = np.frombuffer(seq, dtype=np.uint8)
        rc = self._L.wfm_sketch_fragments(self._p, buf.ctypes.data, len(seq), frag_off.ctypes.data,
                                          frag_len.ctypes.data, n, k, s, seq_id, out.ctypes.data, cnt.ctypes.data)
        if rc < 0:
            raise WfmError(f"wfm_sketch_fragments failed ({rc}): {self.last_error()}")
        return [out[i * s:i * s + cnt[i]] for i in range(n)]

    def index_build(self, minmers, max_kmer_freq=0.0002):
        """wfm_index_build: device-resident reference index from the concatenated minmer intervals."""
        m = np.ascontiguousarray(minmers, dtype=MINMER_DTYPE)
        L = self._L
        L.wfm_index_build.restype = C.c_int
        L.wfm_index_build.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.POINTER(C.c_void_p)]
        L.wfm_index_free.restype = None
        L.wfm_index_free.argtypes = [C.c_void_p, C.c_void_p]
        L.wfm_index_info.argtypes = [C.c_void_p, C.POINTER(IndexInfo)]
        L.wfm_index_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        ix = C.c_void_p()
        rc = L.wfm_index_build(self._p, m.ctypes.data, len(m), max_kmer_freq, C.byref(ix))
        if rc != 0:
            raise WfmError(f"wfm_index_build failed ({rc}): {self.last_error()}")
        return Index(self, ix)

    def index_build_sequences(self, seqs, k: int, w: int, s: int, seq_ids=None, threads: int = 1, max_kmer_freq=0.0002):
        """wfm_index_build_sequences: Sketch::build in one call; returns (Index or None, number of minmer intervals)."""
        n = len(seqs)
        ids = np.ascontiguousarray(seq_ids if seq_ids is not None else range(n), dtype=np.int32)
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in seqs]
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        lens = np.array([len(x) for x in seqs], dtype=np.int64)
        L = self._L
        L.wfm_index_free.restype = None
        L.wfm_index_free.argtypes = [C.c_void_p, C.c_void_p]
        L.wfm_index_info.argtypes = [C.c_void_p, C.POINTER(IndexInfo)]
        L.wfm_index_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        f = L.wfm_index_build_sequences
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                      C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        ix = C.c_void_p()
        nw = C.c_int64(0)
        rc = f(self._p, ptrs, lens.ctypes.data, ids.ctypes.data, n, k, w, s, threads, max_kmer_freq, C.byref(ix), C.byref(nw))
        if rc != 0:
            raise WfmError(f"wfm_index_build_sequences failed ({rc}): {self.last_error()}")
        return (Index(self, ix) if ix.value else None), nw.value

    def sketch_part(self, seqs, k: int, w: int, s: int, seq_ids=None, threads: int = 1):
        """wfm_sketch_part: the minmer intervals of the sequences, left on this handle's device; returns a MinmerPart."""
        n = len(seqs)
        ids = np.ascontiguousarray(seq_ids if seq_ids is not None else range(n), dtype=np.int32)
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in seqs]
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
        lens = np.array([len(x) for x in seqs], dtype=np.int64)
        f = self._L.wfm_sketch_part
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        part = C.c_void_p()
        rc = f(self._p, ptrs, lens.ctypes.data, ids.ctypes.data, n, k, w, s, threads, C.byref(part))
        if rc != 0:
            raise WfmError(f"wfm_sketch_part failed ({rc}): {self.last_error()}")
        return MinmerPart(self, part)

    def index_build_parts(self, parts, order, max_kmer_freq=0.0002):
        """wfm_index_build_parts: the index of the union of the parts (MinmerPart objects of any handle), order = one
        (part, sequence-in-part) pair per sequence of the union; returns (Index or None, number of minmer intervals)."""
        L = self._L
        L.wfm_index_free.restype = None
        L.wfm_index_free.argtypes = [C.c_void_p, C.c_void_p]
        L.wfm_index_info.argtypes = [C.c_void_p, C.POINTER(IndexInfo)]
        L.wfm_index_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        arr = (C.c_void_p * max(len(parts), 1))(*[p._p for p in parts])
        od = np.ascontiguousarray(order, dtype=np.int32).reshape(-1, 2)
        f = L.wfm_index_build_parts
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_double, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        ix = C.c_void_p()
        nw = C.c_int64(0)
        rc = f(self._p, arr, len(parts), od.ctypes.data, len(od), max_kmer_freq, C.byref(ix), C.byref(nw))
        if rc != 0:
            raise WfmError(f"wfm_index_build_parts failed ({rc}): {self.last_error()}")
        return (Index(self, ix) if ix.value else None), nw.value

    def map_l1(self, index, qsketch, qcount, q_seq_id, q_len, q_active, s, params, ref_group):
        """wfm_map_l1: L1 candidate regions of a batch of query fragments.  params: the dict of oracle/map_l1.py."""
        nfrag = len(qcount)
        q = np.ascontiguousarray(qsketch, dtype=MINMER_DTYPE)
        qc = np.ascontiguousarray(qcount, dtype=np.int32)
        qs = np.ascontiguousarray(q_seq_id, dtype=np.int32)
        ql = np.ascontiguousarray(q_len, dtype=np.int32)
        qa = np.ascontiguousarray(q_active, dtype=np.uint8)
        rg = np.ascontiguousarray(ref_group, dtype=np.int32)
        mh = np.ascontiguousarray(params["min_hits_by_qsketch"], dtype=np.int32)
        sc = np.ascontiguousarray(params["sketch_cutoffs"], dtype=np.int32)
        assert len(q) == nfrag * s and len(mh) == params["sketch_size"] + 1
        P = L1Params(params["window_length"], params["sketch_size"], params["min_hits_cached"], params["cached_segment_length"],
                     int(params["skip_self"]), int(params["skip_prefix"]), int(params["lower_triangular"]),
                     int(params["stage1_topani"]), int(params["stage2_full_scan"]), len(rg), rg.ctypes.data, mh.ctypes.data,
                     sc.ctypes.data, len(sc), 0)
        f = self._L.wfm_map_l1
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                      C.POINTER(L1Params), C.c_void_p, C.c_int64]
        cap = 1 << 16
        while True:
            out = np.zeros(cap, dtype=L1_DTYPE)
            n = f(self._p, index._p, q.ctypes.data, qc.ctypes.data, qs.ctypes.data, ql.ctypes.data, qa.ctypes.data, nfrag, s,
                  C.byref(P), out.ctypes.data, cap)
            if n < 0:
                raise WfmError(f"wfm_map_l1 failed ({n}): {self.last_error()}")
            if n <= cap:
                return out[:n]
            cap = int(n)

    def map_fragments(self, index, seq: bytes, frag_off, frag_seq_id, k, p1, p2, ref_group, kc_threshold=0.0):
        """wfm_map_fragments: sketch -> L1 -> L2 for fragments of p1["window_length"] bases of one buffer."""
        off = np.ascontiguousarray(frag_off, dtype=np.int64)
        sid = np.ascontiguousarray(frag_seq_id, dtype=np.int32)
        rg = np.ascontiguousarray(ref_group, dtype=np.int32)
        mh = np.ascontiguousarray(p1["min_hits_by_qsketch"], dtype=np.int32)
        sc = np.ascontiguousarray(p1["sketch_cutoffs"], dtype=np.int32)
        keep = np.ascontiguousarray(p2["keep_table"], dtype=np.uint8)
        ident = np.ascontiguousarray(p2["ident_table"], dtype=np.uint16)
        cut = np.ascontiguousarray(p2["cutoff_j"], dtype=np.float64)
        P = MapParams()
        P.kmer_size = k
        P.kmer_complexity_threshold = kc_threshold
        P.l1 = L1Params(p1["window_length"], p1["sketch_size"], p1["min_hits_cached"], p1["cached_segment_length"],
                        int(p1["skip_self"]), int(p1["skip_prefix"]), int(p1["lower_triangular"]), int(p1["stage1_topani"]),
                        int(p1["stage2_full_scan"]), len(rg), rg.ctypes.data, mh.ctypes.data, sc.ctypes.data, len(sc), 0)
        P.l2 = L2Params(p2["window_length"], p2["sketch_size"], int(p2["stage1_topani"]), 0, keep.ctypes.data, ident.ctypes.data,
                        cut.ctypes.data)
        buf = np.frombuffer(seq, dtype=np.uint8)
        f = self._L.wfm_map_fragments
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(MapParams),
                      C.c_void_p, C.c_void_p, C.c_int64]
        cap = 1 << 16
        while True:
            out = np.zeros(cap, dtype=MAPPING_DTYPE)
            frag = np.zeros(cap, dtype=np.int32)
            n = f(self._p, index._p, buf.ctypes.data, len(seq), off.ctypes.data, sid.ctypes.data, len(off), C.byref(P),
                  out.ctypes.data, frag.ctypes.data, cap)
            if n < 0:
                raise WfmError(f"wfm_map_fragments failed ({n}): {self.last_error()}")
            if n <= cap:
                return out[:n], frag[:n]
            cap = int(n)

    def minhash_sketch(self, seq: bytes, k: int = 21, sketch_size: int = 4096):
        """wfm_minhash_sketch: bottom-sketch_size canonical k-mer hashes (with multiplicity) of one sequence."""
        out = np.zeros(sketch_size, dtype=np.uint64)
        buf = np.frombuffer(seq, dtype=np.uint8)
        f = self._L.wfm_minhash_sketch
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]
        n = f(self._p, buf.ctypes.data, len(seq), k, sketch_size, out.ctypes.data)
        if n < 0:
            raise WfmError(f"wfm_minhash_sketch failed ({n}): {self.last_error()}")
        return out[:n]

    def sketch_intersections(self, sketches, rows=None, cols=None, offsets=None):
        """wfm_sketch_intersections: the multiset intersection sizes of sketches[rows[r]] and sketches[cols[c]] as a uint32 array
        [n_rows, n_cols].  sketches: a list of ascending uint64 arrays (duplicates allowed, empty allowed); rows / cols default to all
        of them.  offsets (a test's way to hand in a broken CSR) replaces the offsets the sketches' lengths give."""
        n = len(sketches)
        parts = [np.ascontiguousarray(s, dtype=np.uint64) for s in sketches]
        hashes = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)
        if offsets is None:
            offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts], dtype=np.int64)])
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        if len(offs) != n + 1:
            raise ValueError("one offset per sketch and one more")
        r = np.ascontiguousarray(np.arange(n) if rows is None else rows, dtype=np.int32)
        c = np.ascontiguousarray(np.arange(n) if cols is None else cols, dtype=np.int32)
        out = np.zeros((len(r), len(c)), dtype=np.uint32)
        f = self._L.wfm_sketch_intersections
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
        rc = f(self._p, hashes.ctypes.data, offs.ctypes.data, n, r.ctypes.data, len(r), c.ctypes.data, len(c), out.ctypes.data)
        if rc != 0:
            raise WfmError(f"wfm_sketch_intersections failed ({rc}): {self.last_error()}")
        return out

    def map_l2(self, index, qsketch, qcount, q_len, q_kc, s, cands, params):
        """wfm_map_l2: mappings (MAPPING_DTYPE) + fragment ids for a batch of L1 candidates.
        params: dict(window_length, sketch_size, stage1_topani, keep_table, ident_table, cutoff_j)."""
        nfrag = len(qcount)
        q = np.ascontiguousarray(qsketch, dtype=MINMER_DTYPE)
        qc = np.ascontiguousarray(qcount, dtype=np.int32)
        ql = np.ascontiguousarray(q_len, dtype=np.int32)
        kc = np.ascontiguousarray(q_kc, dtype=np.uint8)
        cd = np.ascontiguousarray(cands, dtype=L1_DTYPE)
        keep = np.ascontiguousarray(params["keep_table"], dtype=np.uint8)
        ident = np.ascontiguousarray(params["ident_table"], dtype=np.uint16)
        cut = np.ascontiguousarray(params["cutoff_j"], dtype=np.float64)
        S1 = params["sketch_size"] + 1
        assert keep.size == S1 * S1 and ident.size == S1 * S1 and cut.size == S1 and len(q) == nfrag * s
        P = L2Params(params["window_length"], params["sketch_size"], int(params["stage1_topani"]), 0, keep.ctypes.data,
                     ident.ctypes.data, cut.ctypes.data)
        f = self._L.wfm_map_l2
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                      C.c_int64, C.POINTER(L2Params), C.c_void_p, C.c_void_p, C.c_int64]
        cap = 1 << 16
        while True:
            out = np.zeros(cap, dtype=MAPPING_DTYPE)
            frag = np.zeros(cap, dtype=np.int32)
            n = f(self._p, index._p, q.ctypes.data, qc.ctypes.data, ql.ctypes.data, kc.ctypes.data, nfrag, s, cd.ctypes.data, len(cd),
                  C.byref(P), out.ctypes.data, frag.ctypes.data, cap)
            if n < 0:
                raise WfmError(f"wfm_map_l2 failed ({n}): {self.last_error()}")
            if n <= cap:
                return out[:n], frag[:n]
            cap = int(n)

    def add_minmers_multi(self, seqs, k: int, w: int, s: int, seq_ids=None, threads: int = 1, cap=None):
        """wfm_add_minmers_multi: minmer intervals of several sequences (GPU hashing, threaded host winnowing);
        returns one array per sequence."""
        n = len(seqs)
        ids = np.ascontiguousarray(seq_ids if seq_ids is not None else range(n), dtype=np.int32)
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in seqs]
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        lens = np.array([len(x) for x in seqs], dtype=np.int64)
        cap = int(cap) if cap else 4 * int(lens.sum()) + 64
        out = np.zeros(cap, dtype=MINMER_DTYPE)
        counts = np.zeros(n, dtype=np.int64)
        f = self._L.wfm_add_minmers_multi
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                      C.c_void_p]
        tot = f(self._p, ptrs, lens.ctypes.data, ids.ctypes.data, n, k, w, s, threads, out.ctypes.data, cap, counts.ctypes.data)
        if tot < 0:
            raise WfmError(f"wfm_add_minmers_multi failed ({tot}): {self.last_error()}")
        offs = np.concatenate([[0], np.cumsum(counts)])
        return [out[offs[i]:offs[i + 1]] for i in range(n)]

    def finish_records(self, raw, w: int):
        """wfm_finish_records: the closing steps of addMinmers on the device (map_finish.hip) on raw interval records;
        returns (records, recursion levels, ranges heap-sorted on the host)."""
        raw = np.ascontiguousarray(raw, dtype=MINMER_DTYPE)
        f = self._L.wfm_finish_records
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        cap = 4 * len(raw) + 64
        lv, hp = C.c_int32(0), C.c_int32(0)
        while True:
            out = np.zeros(cap, dtype=MINMER_DTYPE)
            n = f(self._p, raw.ctypes.data, len(raw), w, out.ctypes.data, cap, C.byref(lv), C.byref(hp))
            if n < 0:
                raise WfmError(f"wfm_finish_records failed ({n}): {self.last_error()}")
            if n <= cap:
                return out[:n], lv.value, hp.value
            cap = int(n)

    def prefilter_kmers(self, seq: bytes, k: int, w: int, s: int, c_factor: float = 4.0):
        """wfm_prefilter_kmers: the k-mers the host winnowing gets to see; returns (pos, hash, strand)."""
        cap = len(seq) + 1
        pos = np.zeros(cap, dtype=np.uint32)
        hsh = np.zeros(cap, dtype=np.uint64)
        st = np.zeros(cap, dtype=np.int8)
        buf = np.frombuffer(seq, dtype=np.uint8)
        f = self._L.wfm_prefilter_kmers
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        n = f(self._p, buf.ctypes.data, len(seq), k, w, s, c_factor, pos.ctypes.data, hsh.ctypes.data, st.ctypes.data, cap)
        if n < 0:
            raise WfmError(f"wfm_prefilter_kmers failed ({n}): {self.last_error()}")
        return pos[:n], hsh[:n], st[:n]

    def add_minmers(self, seq: bytes, k: int, w: int, s: int, seq_id: int = 0):
        """wfm_add_minmers: winnowed minmer intervals of one target sequence."""
        cap = 4 * len(seq) + 64
        out = np.zeros(cap, dtype=MINMER_DTYPE)
        buf = np.frombuffer(seq, dtype=np.uint8)
        self._L.wfm_add_minmers.restype = C.c_int64
        self._L.wfm_add_minmers.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int32, C.c_void_p, C.c_int64]
        n = self._L.wfm_add_minmers(self._p, buf.ctypes.data, len(seq), k, w, s, seq_id, out.ctypes.data, cap)
        if n < 0:
            raise WfmError(f"wfm_add_minmers failed ({n}): {self.last_error()}")
        return out[:n]


# ---------------------------------------------------------------------------
# host-side align driver (include/wfmash_host.h)
# ---------------------------------------------------------------------------
HOST_EXPORTS = ["wfmh_test_packed_lce", "wfmh_test_is_acgt", "wfmh_align_default_params", "wfmh_align_paf", "wfmh_test_cigar", "wfmh_free", "wfmh_test_winnow",
                "wfmh_map_default_params", "wfmh_test_filter", "wfmh_map", "wfmh_test_winnow_chunked", "wfmh_test_fasta", "wfmh_test_winnow_thinned", "wfmh_test_sort_records", "wfmh_test_index_file",
                "wfmh_map_multi", "wfmh_align_paf_multi", "wfmh_test_winnow_model", "wfmh_test_sortlike_model", "wfmh_test_finish_records",
                "wfmh_release_sequences", "wfmh_test_fasta_shared", "wfmh_seed_paf", "wfmh_test_deal", "wfmh_test_subwindow",
                "wfmh_test_rows", "wfmh_test_tile_plan", "wfmh_test_p2_plan", "wfmh_test_base_plan", "wfmh_test_map_plan", "wfmh_test_filter_ordered",
                "wfmh_test_reuse_plan", "wfmh_test_planned_meet", "wfmh_test_tile_plan_dirs", "wfmh_test_tile_interior", "wfmh_test_tile_lean_waves", "wfmh_set_verify", "wfmh_verify_counts", "wfmh_verify_paf", "wfmh_test_verify_parse",
                "wfmh_set_verify_optimal", "wfmh_verify_optimal_counts", "wfmh_test_opt_band", "wfmh_set_left_align", "wfmh_left_align_counts", "wfmh_set_cs", "wfmh_cs_counts", "wfmh_set_variants", "wfmh_variants_counts",
                "wfmh_set_coverage", "wfmh_coverage_counts", "wfmh_coverage_paf", "wfmh_test_coverage_bedgraph",
                "wfmh_set_lift", "wfmh_lift_counts", "wfmh_lift_paf", "wfmh_test_lift_lines",
                "wfmh_set_chain", "wfmh_chain_counts", "wfmh_chain_paf", "wfmh_test_chain_lines",
                "wfmh_set_maf", "wfmh_maf_counts", "wfmh_maf_paf",
                "wfmh_set_chain_net", "wfmh_chain_net_counts", "wfmh_chain_net_paf", "wfmh_test_chain_net_lines",
                "wfmh_set_transitive", "wfmh_transitive_counts", "wfmh_transitive_paf", "wfmh_test_transitive_lines",
                "wfmh_set_pav", "wfmh_pav_counts", "wfmh_pav_paf", "wfmh_test_pav_text",
                "wfmh_set_genotypes", "wfmh_genotypes_counts", "wfmh_test_genotype_text",
                "wfmh_ani_matrix", "wfmh_ani_matrix_rows", "wfmh_free_ani_rows", "wfmh_set_ani_matrix", "wfmh_test_ani_tsv"]


class MapSummary(C.Structure):
    _fields_ = [("targets", C.c_uint64), ("queries", C.c_uint64), ("subsets", C.c_uint64), ("target_bp", C.c_uint64),
                ("query_bp", C.c_uint64), ("index_windows", C.c_uint64), ("fragments", C.c_uint64), ("l2_mappings", C.c_uint64),
                ("written", C.c_uint64), ("percentage_identity", C.c_float), ("sketch_size", C.c_int32), ("ms_index", C.c_double), ("ms_map", C.c_double), ("ms_filter", C.c_double),
                ("ms_total", C.c_double), ("ms_replicate", C.c_double), ("ms_identity", C.c_double), ("ms_wall", C.c_double),
                ("index_parts", C.c_int32), ("pad_", C.c_int32), ("ms_index_sketch", C.c_double), ("ms_index_merge", C.c_double)]


def _handle_array(handles):
    arr = (C.c_void_p * len(handles))(*[h._p for h in handles])
    return arr


def map_paf_multi(handles, target_fasta: str, out_paf: str, query_fasta: str = None, params=None) -> "MapSummary":
    """wfmh_map_multi: the map phase over several GPUs of the node (index built once, copied to the others)."""
    L = load()
    L.wfmh_map_multi.restype = C.c_int
    L.wfmh_map_multi.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.POINTER(MapSummary)]
    s = MapSummary()
    rc = L.wfmh_map_multi(_handle_array(handles), len(handles), target_fasta.encode(), query_fasta.encode() if query_fasta else None,
                          out_paf.encode(), C.byref(params) if params is not None else None, C.byref(s))
    if rc != 0:
        raise WfmError(f"wfmh_map_multi failed ({rc}): {handles[0].last_error()}")
    return s


def seed_paf(target_fasta: str, seeds_paf: str, out_paf: str, query_fasta: str = None, params=None) -> "MapSummary":
    """wfmh_seed_paf: external seeds (-K) through the group sweep and the scaffold filter into a mapping PAF (host only, no GPU)."""
    L = load()
    L.wfmh_seed_paf.restype = C.c_int
    L.wfmh_seed_paf.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.POINTER(MapSummary)]
    s = MapSummary()
    rc = L.wfmh_seed_paf(target_fasta.encode(), query_fasta.encode() if query_fasta else None, seeds_paf.encode(), out_paf.encode(),
                         C.byref(params) if params is not None else None, C.byref(s))
    if rc != 0:
        raise WfmError(f"wfmh_seed_paf failed ({rc})")
    return s


def map_paf(handle, target_fasta: str, out_paf: str, query_fasta: str = None, params=None) -> "MapSummary":
    """wfmh_map: the map phase on files (FASTA -> approximate mapping PAF)."""
    L = load()
    L.wfmh_map.restype = C.c_int
    L.wfmh_map.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.POINTER(MapSummary)]
    s = MapSummary()
    rc = L.wfmh_map(handle._p, target_fasta.encode(), query_fasta.encode() if query_fasta else None, out_paf.encode(),
                    C.byref(params) if params is not None else None, C.byref(s))
    if rc != 0:
        raise WfmError(f"wfmh_map failed ({rc}): {handle.last_error()}")
    return s


class AniRowC(C.Structure):
    """wfmh_ani_row_t (include/wfmash_host.h)"""
    _fields_ = [("query_group", C.c_void_p), ("target_group", C.c_void_p), ("query_hashes", C.c_uint64), ("target_hashes", C.c_uint64),
                ("shared", C.c_uint64), ("jaccard", C.c_double), ("ani", C.c_double)]


def ani_matrix(handles_or_handle, target_fasta: str, query_fasta: str = None, params=None):
    """wfmh_ani_matrix_rows: the group-by-group ANI table the identity estimate is made from, one tuple (query_group, target_group,
    query_hashes, target_hashes, shared, jaccard, ani) per ordered pair of different groups, in ascending group ids."""
    L = load()
    handles = list(handles_or_handle) if isinstance(handles_or_handle, (list, tuple)) else [handles_or_handle]
    f = L.wfmh_ani_matrix_rows
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_void_p, C.POINTER(C.POINTER(AniRowC)), C.POINTER(C.c_int64)]
    L.wfmh_free_ani_rows.restype = None
    L.wfmh_free_ani_rows.argtypes = [C.POINTER(AniRowC), C.c_int64]
    rows, n = C.POINTER(AniRowC)(), C.c_int64(0)
    rc = f(_handle_array(handles), len(handles), os.fsencode(target_fasta), os.fsencode(query_fasta) if query_fasta else None,
           C.byref(params) if params is not None else None, C.byref(rows), C.byref(n))
    if rc != 0:
        raise WfmError(f"wfmh_ani_matrix_rows failed ({rc}): {handles[0].last_error()}")
    try:
        return [(C.string_at(r.query_group).decode(), C.string_at(r.target_group).decode(), int(r.query_hashes), int(r.target_hashes),
                 int(r.shared), float(r.jaccard), float(r.ani)) for r in (rows[i] for i in range(n.value))]
    finally:
        L.wfmh_free_ani_rows(rows, n)


def ani_matrix_tsv(handles_or_handle, target_fasta: str, out_tsv: str, query_fasta: str = None, params=None) -> None:
    """wfmh_ani_matrix: the same table written as TSV (what `wfmash-hip --ani-only --ani-matrix FILE` writes)."""
    L = load()
    handles = list(handles_or_handle) if isinstance(handles_or_handle, (list, tuple)) else [handles_or_handle]
    f = L.wfmh_ani_matrix
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_void_p, C.c_char_p]
    rc = f(_handle_array(handles), len(handles), os.fsencode(target_fasta), os.fsencode(query_fasta) if query_fasta else None,
           C.byref(params) if params is not None else None, os.fsencode(out_tsv))
    if rc != 0:
        raise WfmError(f"wfmh_ani_matrix failed ({rc}): {handles[0].last_error()}")


def set_ani_matrix(out_tsv) -> None:
    """wfmh_set_ani_matrix: the next map_paf / map_paf_multi call writes the ANI table to out_tsv before it maps (None clears)."""
    f = load().wfmh_set_ani_matrix
    f.restype = None
    f.argtypes = [C.c_char_p]
    f(os.fsencode(out_tsv) if out_tsv is not None else None)


def host_ani_tsv(rows) -> str:
    """wfmh_test_ani_tsv (no GPU): the table's text from (query_group, target_group, query_hashes, target_hashes, shared) tuples."""
    L = load()
    n = len(rows)
    enc = lambda x: x if isinstance(x, bytes) else x.encode()
    qn = (C.c_char_p * max(n, 1))(*[enc(r[0]) for r in rows])
    tn = (C.c_char_p * max(n, 1))(*[enc(r[1]) for r in rows])
    qh, th, sh = (np.array([r[j] for r in rows], dtype=np.uint64) for j in (2, 3, 4))
    f = L.wfmh_test_ani_tsv
    f.restype = C.c_void_p
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    L.wfmh_free.restype = None
    L.wfmh_free.argtypes = [C.c_void_p]
    p = f(qn, tn, qh.ctypes.data, th.ctypes.data, sh.ctypes.data, n)
    if not p:
        raise WfmError("wfmh_test_ani_tsv failed")
    s = C.string_at(p).decode()
    L.wfmh_free(p)
    return s


def host_deal(lengths, n_parts: int):
    """wfmh_test_deal: the part each of the sequences goes to when wfmh_map_multi deals a target subset over n_parts handles."""
    L = load()
    L.wfmh_test_deal.restype = C.c_int
    L.wfmh_test_deal.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    ln = np.ascontiguousarray(lengths, dtype=np.int64)
    out = np.zeros(max(len(ln), 1), dtype=np.int32)
    rc = L.wfmh_test_deal(ln.ctypes.data, len(ln), n_parts, out.ctypes.data)
    if rc != 0:
        raise WfmError(f"wfmh_test_deal failed ({rc})")
    return [int(x) for x in out[:len(ln)]]


def host_map_plan(op: int, values, out_size: int):
    """wfmh_test_map_plan: one function of the map driver's planner (host/map_plan.hpp) on a list of integers -> out_size integers."""
    L = load()
    L.wfmh_test_map_plan.restype = C.c_int
    L.wfmh_test_map_plan.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    v = np.ascontiguousarray(values, dtype=np.int64)
    out = np.full(max(out_size, 1), -(1 << 62), dtype=np.int64)
    rc = L.wfmh_test_map_plan(op, v.ctypes.data, len(v), out.ctypes.data)
    if rc != 0:
        raise WfmError(f"wfmh_test_map_plan failed ({rc})")
    return out[:out_size]


def host_fasta_shared(path: str, name: str) -> str:
    """wfmh_test_fasta_shared: a whole sequence through the per-path shared store, which is then kept as a map call keeps its stores."""
    L = load()
    L.wfmh_test_fasta_shared.restype = C.c_void_p
    L.wfmh_test_fasta_shared.argtypes = [C.c_char_p, C.c_char_p]
    L.wfmh_free.restype = None
    L.wfmh_free.argtypes = [C.c_void_p]
    p = L.wfmh_test_fasta_shared(path.encode(), name.encode())
    if not p:
        raise WfmError("wfmh_test_fasta_shared failed")
    s = C.string_at(p).decode()
    L.wfmh_free(p)
    if s.startswith("ERROR: "):
        raise WfmError(s)
    return s


def release_sequences() -> None:
    """wfmh_release_sequences: lets go of the sequences the last map call left loaded for the align phase."""
    L = load()
    L.wfmh_release_sequences.restype = None
    L.wfmh_release_sequences.argtypes = []
    L.wfmh_release_sequences()


class MapHostParams(C.Structure):
    """wfmh_map_params_t (include/wfmash_host.h)"""
    _fields_ = [("kmer_size", C.c_int32), ("window_length", C.c_int64), ("block_length", C.c_int64), ("chain_gap", C.c_int64),
                ("max_mapping_length", C.c_uint64), ("percentage_identity", C.c_float), ("sketch_size", C.c_int32),
                ("filter_mode", C.c_int32), ("num_mappings_for_segment", C.c_uint32), ("num_mappings_for_scaffold", C.c_uint32),
                ("drop_rand", C.c_int32), ("split", C.c_int32), ("merge_mappings", C.c_int32), ("skip_self", C.c_int32),
                ("skip_prefix", C.c_int32), ("lower_triangular", C.c_int32), ("prefix_delim", C.c_char),
                ("filter_length_mismatches", C.c_int32), ("sparsity_hash_threshold", C.c_uint64), ("overlap_threshold", C.c_double),
                ("scaffold_overlap_threshold", C.c_double), ("scaffold_max_deviation", C.c_int64), ("scaffold_gap", C.c_int64),
                ("scaffold_min_length", C.c_int64), ("legacy_output", C.c_int32), ("minimum_hits", C.c_int32),
                ("max_kmer_freq", C.c_double), ("index_by_size", C.c_int64), ("kmer_complexity_threshold", C.c_float),
                ("stage1_topani_filter", C.c_int32), ("stage2_full_scan", C.c_int32), ("ani_diff", C.c_float),
                ("ani_diff_conf", C.c_float), ("hg_numerator", C.c_double), ("threads", C.c_int32),
                ("auto_pct_identity", C.c_int32), ("ani_percentile", C.c_int32), ("ani_adjustment", C.c_float),
                ("target_prefix", C.c_char_p), ("target_list", C.c_char_p), ("query_prefix", C.c_char_p), ("query_list", C.c_char_p),
                ("index_file", C.c_char_p), ("write_index", C.c_int32), ("pad_", C.c_int32),
                ("scaffold_out", C.c_char_p), ("streaming_minhash", C.c_int32)]


def streaming_minmers(handle, seqs, k: int, w: int, s: int, seq_ids=None):
    """wfm_streaming_minmers: the --streaming-minhash target records (sketchSequenceStreaming) of several sequences, grouped by
    sequence in input order, each group ordered by wpos; one MINMER_DTYPE array."""
    L = load()
    n = len(seqs)
    ids = np.ascontiguousarray(seq_ids if seq_ids is not None else range(n), dtype=np.int32)
    bufs = [np.frombuffer(x, dtype=np.uint8) for x in seqs]
    ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    lens = np.array([len(x) for x in seqs], dtype=np.int64)
    counts = np.zeros(max(n, 1), dtype=np.int64)
    f = L.wfm_streaming_minmers
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    cap = n * s + 1
    out = np.zeros(cap, dtype=MINMER_DTYPE)
    tot = f(handle._p, ptrs, lens.ctypes.data, ids.ctypes.data, n, k, w, s, out.ctypes.data, cap, counts.ctypes.data)
    if tot < 0:
        raise WfmError(f"wfm_streaming_minmers failed ({tot}): {handle.last_error()}")
    assert tot <= cap, (tot, cap)
    return out[:tot]


def map_default_params(**over) -> MapHostParams:
    L = load()
    p = MapHostParams()
    L.wfmh_map_default_params.restype = None
    L.wfmh_map_default_params.argtypes = [C.POINTER(MapHostParams)]
    L.wfmh_map_default_params(C.byref(p))
    for k, v in over.items():
        if isinstance(v, str):
            v = v.encode()
        setattr(p, k, v)
    return p


def host_fasta(path: str, name: str = None, start: int = 0, end_inclusive: int = -1, whole: bool = False) -> str:
    """wfmh_test_fasta: the FASTA reader (random access through .fai/.gzi, or in-memory); no GPU needed.
    name None -> 'indexed|in-memory' and the name/length table."""
    L = load()
    L.wfmh_test_fasta.restype = C.c_void_p
    L.wfmh_test_fasta.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int]
    L.wfmh_free.restype = None
    L.wfmh_free.argtypes = [C.c_void_p]
    p = L.wfmh_test_fasta(path.encode(), name.encode() if name is not None else None, start, end_inclusive, int(whole))
    if not p:
        raise WfmError("wfmh_test_fasta failed")
    s = C.string_at(p).decode()
    L.wfmh_free(p)
    if s.startswith("ERROR: "):
        raise WfmError(s)
    return s


def host_filter(stage: str, mappings, fasta: str, query_name: str, params: MapHostParams) -> str:
    """wfmh_test_filter: the host-side post-processing on caller-supplied MappingResults (no GPU needed)."""
    L = load()
    m = np.ascontiguousarray(mappings, dtype=MAPPING_DTYPE)
    L.wfmh_test_filter.restype = C.c_void_p
    L.wfmh_test_filter.argtypes = [C.c_char_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_char_p, C.POINTER(MapHostParams)]
    L.wfmh_free.restype = None
    L.wfmh_free.argtypes = [C.c_void_p]
    p = L.wfmh_test_filter(stage.encode(), m.ctypes.data, len(m), fasta.encode(), query_name.encode(), C.byref(params))
    if not p:
        raise WfmError("wfmh_test_filter failed")
    s = C.string_at(p).decode()
    L.wfmh_free(p)
    if s.startswith("ERROR: "):
        raise WfmError(s)
    return s


def host_filter_ordered(stage: str, mappings, orig, fasta: str, query_name: str, params: MapHostParams) -> str:
    """wfmh_test_filter_ordered: host_filter on mappings given in chaining order; orig[i] = mapping i's position in fragment order."""
    L = load()
    m = np.ascontiguousarray(mappings, dtype=MAPPING_DTYPE)
    o = np.ascontiguousarray(orig, dtype=np.uint32)
    if len(o) != len(m):
        raise ValueError("one entry of orig per mapping")
    L.wfmh_test_filter_ordered.restype = C.c_void_p
    L.wfmh_test_filter_ordered.argtypes = [C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(MapHostParams)]
    L.wfmh_free.restype = None
    L.wfmh_free.argtypes = [C.c_void_p]
    p = L.wfmh_test_filter_ordered(stage.encode(), m.ctypes.data, len(m), o.ctypes.data, fasta.encode(), query_name.encode(), C.byref(params))
    if not p:
        raise WfmError("wfmh_test_filter_ordered failed")
    s = C.string_at(p).decode()
    L.wfmh_free(p)
    if s.startswith("ERROR: "):
        raise WfmError(s)
    return s


class AlignParams(C.Structure):
    _fields_ = [("mismatch", C.c_int32), ("gap_open1", C.c_int32), ("gap_ext1", C.c_int32),
                ("gap_open2", C.c_int32), ("gap_ext2", C.c_int32),
                ("min_identity", C.c_float), ("min_alignment_length", C.c_uint64),
                ("min_block_identity", C.c_float), ("target_padding", C.c_uint64),
                ("query_padding", C.c_uint64), ("wflign_max_len_minor", C.c_uint64),
                ("disable_chain_patching", C.c_int32), ("sam_format", C.c_int32),
                ("emit_md_tag", C.c_int32), ("no_seq_in_sam", C.c_int32), ("threads", C.c_int32), ("resident_sequences", C.c_int32)]


class AlignSummary(C.Structure):
    _fields_ = [("records", C.c_uint64), ("aligned_bp", C.c_uint64), ("written", C.c_uint64),
                ("skipped", C.c_uint64), ("cells", C.c_uint64), ("ms_gpu", C.c_double), ("ms_total", C.c_double),
                ("ms_rows", C.c_double), ("ms_fetch", C.c_double), ("ms_wflign", C.c_double), ("ms_text", C.c_double), ("batches", C.c_uint64),
                ("cells_tile", C.c_uint64), ("tile_launches", C.c_uint64), ("ms_tile", C.c_double), ("ms_tags", C.c_double),
                ("records_resident", C.c_uint64), ("lazy_fetches", C.c_uint64)]


def _host():
    L = load()
    if not getattr(L, "_host_bound", False):
        L.wfmh_align_default_params.restype = None
        L.wfmh_align_default_params.argtypes = [C.POINTER(AlignParams)]
        L.wfmh_align_paf.restype = C.c_int
        L.wfmh_align_paf.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                     C.POINTER(AlignParams), C.POINTER(AlignSummary)]
        L.wfmh_test_cigar.restype = C.c_void_p
        L.wfmh_test_cigar.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_longlong, C.c_longlong]
        L.wfmh_free.restype = None
        L.wfmh_free.argtypes = [C.c_void_p]
        L._host_bound = True
    return L


def host_cigar_fn(fn, a=b"", b=b"", query=b"", target=b"", i0=0, i1=0) -> str:
    """Pure host-side CIGAR helpers of wfmash_amd/host (no GPU needed)."""
    L = _host()
    enc = lambda x: x if isinstance(x, bytes) else x.encode()
    p = L.wfmh_test_cigar(enc(fn), enc(a), enc(b), enc(query), enc(target), i0, i1)
    s = C.string_at(p).decode()
    L.wfmh_free(p)
    return s


def set_verify(on: bool) -> None:
    """wfmh_set_verify: every later align_paf call of the process verifies its finished PAF lines on the device; zeroes the counts."""
    f = _host().wfmh_set_verify
    f.restype = None
    f.argtypes = [C.c_int]
    f(1 if on else 0)


def verify_counts():
    """wfmh_verify_counts: (lines checked, failed, unverifiable, bases compared) since wfmh_set_verify was last called."""
    f = _host().wfmh_verify_counts
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = f(out)
    if rc != 0:
        raise WfmError(f"wfmh_verify_counts failed ({rc})")
    return tuple(int(v) for v in out)


def set_left_align(on: bool) -> None:
    """wfmh_set_left_align: every later align_paf call of the process left-aligns its records' interior gaps on the device before they are
    written; zeroes the counts."""
    f = _host().wfmh_set_left_align
    f.restype = None
    f.argtypes = [C.c_int]
    f(1 if on else 0)


def left_align_counts():
    """wfmh_left_align_counts: (records, gaps, gaps moved, records left alone) since wfmh_set_left_align was last called."""
    f = _host().wfmh_left_align_counts
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = f(out)
    if rc != 0:
        raise WfmError(f"wfmh_left_align_counts failed ({rc})")
    return tuple(int(v) for v in out)


def set_cs(form: int) -> None:
    """wfmh_set_cs: every later align_paf call of the process appends minimap2's cs:Z: string, spelled on the device, to every record it
    writes (0: off, 1: short, 2: long); zeroes the counts."""
    f = _host().wfmh_set_cs
    f.restype = None
    f.argtypes = [C.c_int]
    f(int(form))


def cs_counts():
    """wfmh_cs_counts: (records written with a string, bytes of those strings, records written without one, 0) since wfmh_set_cs was
    last called."""
    f = _host().wfmh_cs_counts
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = f(out)
    if rc != 0:
        raise WfmError(f"wfmh_cs_counts failed ({rc})")
    return tuple(int(v) for v in out)


def set_variants(path) -> None:
    """wfmh_set_variants: every later align_paf call of the process writes the variants of the records it writes, called on the device, as a
    VCF to `path` (None: off); zeroes the counts."""
    f = _host().wfmh_set_variants
    f.restype = None
    f.argtypes = [C.c_char_p]
    f(os.fsencode(path) if path else None)


def variants_counts():
    """wfmh_variants_counts: (records called, variants written, SNVs masked, records left alone) since wfmh_set_variants was last called."""
    f = _host().wfmh_variants_counts
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = f(out)
    if rc != 0:
        raise WfmError(f"wfmh_variants_counts failed ({rc})")
    return tuple(int(v) for v in out)


def set_coverage(path) -> None:
    """wfmh_set_coverage: every later align_paf call of the process writes the per-base depth of the target, summed on the device over the
    records it writes, as a bedGraph to `path` (None: off); zeroes the counts."""
    f = _host().wfmh_set_coverage
    f.restype = None
    f.argtypes = [C.c_char_p]
    f(os.fsencode(path) if path else None)


def coverage_counts():
    """wfmh_coverage_counts: (records added, target bases with depth >= 1, sum of depth, intervals written) since wfmh_set_coverage."""
    f = _host().wfmh_coverage_counts
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = f(out)
    if rc != 0:
        raise WfmError(f"wfmh_coverage_counts failed ({rc})")
    return tuple(int(v) for v in out)


def coverage_paf(handle, target_fasta, aligned_paf, out_path):
    """wfmh_coverage_paf: the depth bedGraph of an existing aligned PAF; returns (lines added, lines skipped, covered bases, sum of depth)."""
    f = _host().wfmh_coverage_paf
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = f(handle._p, os.fsencode(target_fasta), os.fsencode(aligned_paf), os.fsencode(out_path), out)
    if rc != 0:
        raise WfmError(f"wfmh_coverage_paf failed ({rc}): {handle.last_error()}")
    return tuple(int(v) for v in out)


def host_coverage_bedgraph(names, lengths, intervals) -> str:
    """wfmh_test_coverage_bedgraph (no GPU): the bedGraph of `intervals` = [(start, depth)] over the concatenation of the sequences."""
    L = _host()
    f = L.wfmh_test_coverage_bedgraph
    f.restype = C.c_void_p
    f.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_int64]
    n, m = len(names), len(intervals)
    nm = (C.c_char_p * max(n, 1))(*[x.encode() if isinstance(x, str) else x for x in names])
    ln = (C.c_uint64 * max(n, 1))(*[int(x) for x in lengths])
    st = (C.c_uint64 * max(m, 1))(*[int(a) for a, _ in intervals])
    dp = (C.c_uint32 * max(m, 1))(*[int(d) for _, d in intervals])
    p = f(nm, ln, n, st, dp, m)
    s = C.string_at(p).decode()
    L.wfmh_free(p)
    return s


def set_lift(bed_path, out_path) -> None:
    """wfmh_set_lift: every later align_paf call of the process lifts the intervals of the BED file through the records it writes, on the
    device, and writes the lines to `out_path` (None: off); zeroes the counts."""
    f = _host().wfmh_set_lift
    f.restype = None
    f.argtypes = [C.c_char_p, C.c_char_p]
    f(os.fsencode(bed_path) if bed_path else None, os.fsencode(out_path) if out_path else None)


def lift_counts():
    """wfmh_lift_counts: (records lifted, lines written, empty lifts, BED lines skipped) since wfmh_set_lift."""
    f = _host().wfmh_lift_counts
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = f(out)
    if rc != 0:
        raise WfmError(f"wfmh_lift_counts failed ({rc})")
    return tuple(int(v) for v in out)


def lift_paf(handle, target_fasta, aligned_paf, bed_path, out_path):
    """wfmh_lift_paf: the lift file of an existing aligned PAF; returns (records lifted, lines written, empty lifts, BED lines skipped)."""
    f = _host().wfmh_lift_paf
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = f(handle._p, os.fsencode(target_fasta), os.fsencode(aligned_paf), os.fsencode(bed_path), os.fsencode(out_path), out)
    if rc != 0:
        raise WfmError(f"wfmh_lift_paf failed ({rc}): {handle.last_error()}")
    return tuple(int(v) for v in out)


def host_lift_lines(names, lengths, bed_text, spec) -> str:
    """wfmh_test_lift_lines (no GPU): what the BED parser keeps, and the lift file's lines of the lifts in `spec` (include/wfmash_host.h)."""
    L = _host()
    f = L.wfmh_test_lift_lines
    f.restype = C.c_void_p
    f.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_int, C.c_char_p, C.c_char_p]
    n = len(names)
    nm = (C.c_char_p * max(n, 1))(*[x.encode() if isinstance(x, str) else x for x in names])
    ln = (C.c_uint64 * max(n, 1))(*[int(x) for x in lengths])
    p = f(nm, ln, n, bed_text.encode(), spec.encode())
    if not p:
        raise WfmError("wfmh_test_lift_lines cannot read the spec")
    s = C.string_at(p).decode()
    L.wfmh_free(p)
    return s


def set_chain(path, swap=False) -> None:
    """wfmh_set_chain: every later align_paf call of the process writes the UCSC chain of every record it writes to `path` (None: off), its
    blocks and gaps made on the device; swap: the file from the query to the target, as chainSwap would make it; zeroes the counts."""
    f = _host().wfmh_set_chain
    f.restype = None
    f.argtypes = [C.c_char_p, C.c_int]
    f(os.fsencode(path) if path else None, 1 if swap else 0)


def chain_counts():
    """wfmh_chain_counts: (chains written, blocks, records refused, 0) since wfmh_set_chain."""
    f = _host().wfmh_chain_counts
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = f(out)
    if rc != 0:
        raise WfmError(f"wfmh_chain_counts failed ({rc})")
    return tuple(int(v) for v in out)


def chain_paf(handle, target_fasta, aligned_paf, out_path, swap=False, net_path=None):
    """wfmh_chain_paf: the chain file of an existing aligned PAF; returns (chains written, blocks, records refused, 0).  net_path: the
    single-coverage file of the same PAF too (wfmh_chain_net_paf); with out_path None that file alone, and its counts (records added,
    chains written, pieces, records that won nothing)."""
    out = (C.c_uint64 * 4)()
    net = (C.c_uint64 * 4)()
    if out_path is not None:
        f = _host().wfmh_chain_paf
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint64)]
        rc = f(handle._p, os.fsencode(target_fasta), os.fsencode(aligned_paf), os.fsencode(out_path), 1 if swap else 0, out)
        if rc != 0:
            raise WfmError(f"wfmh_chain_paf failed ({rc}): {handle.last_error()}")
    if net_path is not None:
        f = _host().wfmh_chain_net_paf
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64)]
        rc = f(handle._p, os.fsencode(target_fasta), os.fsencode(aligned_paf), os.fsencode(net_path), net)
        if rc != 0:
            raise WfmError(f"wfmh_chain_net_paf failed ({rc}): {handle.last_error()}")
    return tuple(int(v) for v in (out if out_path is not None else net))


def set_maf(path, split=0) -> None:
    """wfmh_set_maf: every later align_paf call of the process writes the aligned sequences of every record it writes as pairwise MAF
    blocks to `path` (None: off), the rows spelled on the device; split: 0, or the gap bases from which a gap stretch ends a block;
    zeroes the counts."""
    f = _host().wfmh_set_maf
    f.restype = None
    f.argtypes = [C.c_char_p, C.c_uint32]
    f(os.fsencode(path) if path else None, int(split))


def maf_counts():
    """wfmh_maf_counts: (records written with blocks, blocks, columns, records left without blocks) since wfmh_set_maf."""
    f = _host().wfmh_maf_counts
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = f(out)
    if rc != 0:
        raise WfmError(f"wfmh_maf_counts failed ({rc})")
    return tuple(int(v) for v in out)


def maf_paf(handle, target_fasta, aligned_paf, out_path, split=0, query_fasta=None):
    """wfmh_maf_paf: the MAF file of an existing aligned PAF; returns (records written with blocks, blocks, columns, records left without
    blocks)."""
    out = (C.c_uint64 * 4)()
    f = _host().wfmh_maf_paf
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint64)]
    rc = f(handle._p, os.fsencode(target_fasta), os.fsencode(query_fasta) if query_fasta else None, os.fsencode(aligned_paf), os.fsencode(out_path),
           int(split), out)
    if rc != 0:
        raise WfmError(f"wfmh_maf_paf failed ({rc}): {handle.last_error()}")
    return tuple(int(v) for v in out)


def set_chain_net(path) -> None:
    """wfmh_set_chain_net: every later align_paf call of the process adds the blocks of every record it writes to a net object on the
    device and, once all are aligned, writes the chain of the pieces the net left each record to `path` (None: off): every target base
    under at most one chain; zeroes the counts."""
    f = _host().wfmh_set_chain_net
    f.restype = None
    f.argtypes = [C.c_char_p]
    f(os.fsencode(path) if path else None)


def chain_net_counts():
    """wfmh_chain_net_counts: (records added, chains written, pieces, records that won nothing) since wfmh_set_chain_net."""
    f = _host().wfmh_chain_net_counts
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = f(out)
    if rc != 0:
        raise WfmError(f"wfmh_chain_net_counts failed ({rc})")
    return tuple(int(v) for v in out)


def set_transitive(bed_path, out_path, depth=2) -> None:
    """wfmh_set_transitive (include/wfmash_host.h): from now on every align_paf[_multi] adds the records it writes to a trans object per
    handle and, once all batches are aligned, writes the closure of the BED's intervals to out_path.  None for either switches it off."""
    L = _host()
    L.wfmh_set_transitive.restype = None
    L.wfmh_set_transitive.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32]
    L.wfmh_set_transitive(os.fsencode(bed_path) if bed_path else None, os.fsencode(out_path) if out_path else None, int(depth))


def transitive_counts():
    """wfmh_transitive_counts: (records added, lines written, rounds run, BED lines skipped) since set_transitive."""
    L = _host()
    L.wfmh_transitive_counts.restype = C.c_int
    L.wfmh_transitive_counts.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = L.wfmh_transitive_counts(out)
    if rc != 0:
        raise WfmError(f"wfmh_transitive_counts failed ({rc})")
    return tuple(int(v) for v in out)


def transitive_paf(handle, target_fasta, aligned_paf, bed_path, out_path, depth=2, query_fasta=None):
    """wfmh_transitive_paf: the --transitive file of an existing aligned PAF.  Returns (lines added, lines written, rounds run, BED lines
    skipped)."""
    L = _host()
    L.wfmh_transitive_paf.restype = C.c_int
    L.wfmh_transitive_paf.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = L.wfmh_transitive_paf(handle._p, os.fsencode(target_fasta), os.fsencode(query_fasta) if query_fasta else None, os.fsencode(aligned_paf),
                               os.fsencode(bed_path), os.fsencode(out_path), int(depth), out)
    if rc != 0:
        raise WfmError(f"wfmh_transitive_paf failed ({rc}): {handle.last_error()}")
    return tuple(int(v) for v in out)


def host_transitive_lines(tnames, tlengths, qnames, qlengths, bed_text, spec) -> str:
    """wfmh_test_transitive_lines (no GPU): what the BED parser keeps in the world of the two name lists, and the file's lines of the world
    intervals in `spec` (include/wfmash_host.h)."""
    L = _host()
    f = L.wfmh_test_transitive_lines
    f.restype = C.c_void_p
    f.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_int, C.c_char_p, C.c_char_p]
    tn = (C.c_char_p * max(len(tnames), 1))(*[n.encode() for n in tnames])
    tl = (C.c_uint64 * max(len(tlengths), 1))(*tlengths)
    qn = (C.c_char_p * max(len(qnames), 1))(*[n.encode() for n in qnames])
    ql = (C.c_uint64 * max(len(qlengths), 1))(*qlengths)
    p = f(tn, tl, len(tnames), qn, ql, len(qnames), bed_text.encode(), spec.encode())
    if not p:
        raise WfmError("wfmh_test_transitive_lines cannot read the spec")
    try:
        return C.string_at(p).decode()
    finally:
        L.wfmh_free.restype = None
        L.wfmh_free.argtypes = [C.c_void_p]
        L.wfmh_free(p)


def host_chain_net_lines(spec):
    """wfmh_test_chain_net_lines (no GPU): the --chain-net file of the records and pieces in `spec` (include/wfmash_host.h) as bytes."""
    L = _host()
    f = L.wfmh_test_chain_net_lines
    f.restype = C.c_void_p
    f.argtypes = [C.c_char_p]
    p = f(spec.encode())
    if not p:
        raise WfmError("wfmh_test_chain_net_lines cannot read the spec")
    s = C.string_at(p)
    L.wfmh_free(p)
    return s


def host_chain_lines(spec, swap=False):
    """wfmh_test_chain_lines (no GPU): the chain file of the records and blocks in `spec` (include/wfmash_host.h) as bytes, and the flags
    the records' problems carry under `swap`."""
    n_records = sum(1 for ln in spec.split("\n") if ln.startswith("R\t"))
    L = _host()
    f = L.wfmh_test_chain_lines
    f.restype = C.c_void_p
    f.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_uint32)]
    flags = (C.c_uint32 * max(n_records, 1))()
    p = f(spec.encode(), 1 if swap else 0, flags if n_records else None)
    if not p:
        raise WfmError("wfmh_test_chain_lines cannot read the spec")
    s = C.string_at(p)
    L.wfmh_free(p)
    return s, [int(v) for v in flags[:n_records]]


def set_pav(bed_path, window, out_path) -> None:
    """wfmh_set_pav: every later align_paf call of the process keeps per group of query sequences the union of the aligned target bases
    of the records it writes, on the device, and writes the table of the BED's intervals (or of windows of `window` bases) to `out_path`
    (None: off); zeroes the counts."""
    f = _host().wfmh_set_pav
    f.restype = None
    f.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p]
    f(os.fsencode(bed_path) if bed_path else None, int(window or 0), os.fsencode(out_path) if out_path else None)


def pav_counts():
    """wfmh_pav_counts: (records added, rows written, union intervals, BED lines skipped) since wfmh_set_pav."""
    f = _host().wfmh_pav_counts
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = f(out)
    if rc != 0:
        raise WfmError(f"wfmh_pav_counts failed ({rc})")
    return tuple(int(v) for v in out)


def pav_paf(handle, target_fasta, query_fasta, aligned_paf, bed_path, window, out_path):
    """wfmh_pav_paf: the table of an existing aligned PAF; returns (lines added, rows written, union intervals, BED lines skipped)."""
    f = _host().wfmh_pav_paf
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = f(handle._p, os.fsencode(target_fasta), os.fsencode(query_fasta) if query_fasta else None, os.fsencode(aligned_paf),
           os.fsencode(bed_path) if bed_path else None, int(window or 0), os.fsencode(out_path), out)
    if rc != 0:
        raise WfmError(f"wfmh_pav_paf failed ({rc}): {handle.last_error()}")
    return tuple(int(v) for v in out)


def host_pav_text(qnames, tnames, tlengths, window) -> str:
    """wfmh_test_pav_text (no GPU): the names' keys and columns, the header, the windows' rows (include/wfmash_host.h)."""
    L = _host()
    f = L.wfmh_test_pav_text
    f.restype = C.c_void_p
    f.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_int, C.c_uint64]
    nq, nt = len(qnames), len(tnames)
    qn = (C.c_char_p * max(nq, 1))(*[x.encode() if isinstance(x, str) else x for x in qnames])
    tn = (C.c_char_p * max(nt, 1))(*[x.encode() if isinstance(x, str) else x for x in tnames])
    ln = (C.c_uint64 * max(nt, 1))(*[int(x) for x in tlengths])
    p = f(qn, nq, tn, ln, nt, int(window))
    if not p:
        raise WfmError("wfmh_test_pav_text failed")
    s = C.string_at(p).decode()
    L.wfmh_free(p)
    return s


def set_genotypes(path) -> None:
    """wfmh_set_genotypes: every later align_paf call of the process joins the variants of the records it writes into one sorted VCF with a
    haploid GT column per group of query sequences, on the device, and writes it to `path` (None: off); zeroes the counts."""
    f = _host().wfmh_set_genotypes
    f.restype = None
    f.argtypes = [C.c_char_p]
    f(os.fsencode(path) if path else None)


def genotypes_counts():
    """wfmh_genotypes_counts: (records added, sites written, variants merged away, records left alone) since wfmh_set_genotypes."""
    f = _host().wfmh_genotypes_counts
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = f(out)
    if rc != 0:
        raise WfmError(f"wfmh_genotypes_counts failed ({rc})")
    return tuple(int(v) for v in out)


def host_genotype_text(version, tnames, tlengths, keys, sites, rows) -> str:
    """wfmh_test_genotype_text (no GPU): the header and the lines of --genotypes in file order.  sites: [(global pos, ref bytes, alt
    bytes)] in ascending pos; rows: per site a string of len(keys) cells (include/wfmash_host.h)."""
    L = _host()
    f = L.wfmh_test_genotype_text
    f.restype = C.c_void_p
    f.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_uint64), C.c_size_t,
                  C.c_char_p, C.c_char_p]
    nt, ng, ns = len(tnames), len(keys), len(sites)
    tn = (C.c_char_p * max(nt, 1))(*[x.encode() if isinstance(x, str) else x for x in tnames])
    ln = (C.c_uint64 * max(nt, 1))(*[int(x) for x in tlengths])
    kn = (C.c_char_p * max(ng, 1))(*[x.encode() if isinstance(x, str) else x for x in keys])
    flat, alleles = [], b""
    for pos, ref, alt in sites:
        flat += [int(pos), len(ref), len(alt), len(alleles)]
        alleles += ref + alt
    arr = (C.c_uint64 * max(len(flat), 1))(*flat)
    gt = "".join(rows).encode()
    assert len(gt) == ns * ng
    p = f(version.encode(), tn, ln, nt, kn, ng, arr, ns, alleles, gt)
    if not p:
        raise WfmError("wfmh_test_genotype_text failed")
    s = C.string_at(p).decode()
    L.wfmh_free(p)
    return s


def set_verify_optimal(on: bool, max_cells: int = 0) -> None:
    """wfmh_set_verify_optimal: every later device call of the align driver proves its scores optimal (wfm_check_optimal); max_cells caps
    one problem's DP cells (0: no cap); zeroes the counts."""
    f = _host().wfmh_set_verify_optimal
    f.restype = None
    f.argtypes = [C.c_int, C.c_uint64]
    f(1 if on else 0, int(max_cells))


def verify_optimal_counts():
    """wfmh_verify_optimal_counts: (problems checked, failed, skipped over the cell cap, DP cells) since wfmh_set_verify_optimal was last called."""
    f = _host().wfmh_verify_optimal_counts
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = f(out)
    if rc != 0:
        raise WfmError(f"wfmh_verify_optimal_counts failed ({rc})")
    return tuple(int(v) for v in out)


def host_opt_band(pen, plen, tlen, free, score):
    """wfmh_test_opt_band (no GPU): the band of wfm_check_optimal for a claimed score -> (band_lo, band_hi, cells)."""
    f = _host().wfmh_test_opt_band
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    a = (C.c_int64 * 12)(*(list(pen or DEFAULT_PEN) + [plen, tlen] + list(free) + [score]))
    out = (C.c_int64 * 3)()
    if f(a, out) != 0:
        raise WfmError("wfmh_test_opt_band: bad arguments")
    return int(out[0]), int(out[1]), int(out[2])


def verify_paf(handle, target_fasta, aligned_paf, query_fasta=None):
    """wfmh_verify_paf: an existing aligned PAF held against its bases; returns (checked, failed, unverifiable, bases compared)."""
    f = _host().wfmh_verify_paf
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 4)()
    rc = f(handle._p, os.fsencode(target_fasta), os.fsencode(query_fasta) if query_fasta else None, os.fsencode(aligned_paf), out)
    if rc != 0:
        raise WfmError(f"wfmh_verify_paf failed ({rc}): {handle.last_error()}")
    return tuple(int(v) for v in out)


def host_verify_parse(line) -> str:
    """wfmh_test_verify_parse (no GPU): a PAF line as the verifier reads it, fields separated by tabs."""
    L = _host()
    f = L.wfmh_test_verify_parse
    f.restype = C.c_void_p
    f.argtypes = [C.c_char_p]
    p = f(line if isinstance(line, bytes) else line.encode())
    s = C.string_at(p).decode()
    L.wfmh_free(p)
    return s


def host_subwindow(win_start, win_end, rev, a, b):
    """wfmh_test_subwindow: [a, b) of a side that is the (reverse-complemented when rev) window [win_start, win_end) of a stored
    sequence, as a forward window (start, end) of that sequence."""
    L = _host()
    f = L.wfmh_test_subwindow
    f.restype = None
    f.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    s, e = C.c_int64(0), C.c_int64(0)
    f(win_start, win_end, 1 if rev else 0, a, b, C.byref(s), C.byref(e))
    return s.value, e.value


def host_plan_batch_bytes(file_bytes, rows, row_bytes, row_bases_sum, batch_records, batch_bases, nworkers, ngpu=1, min_batches=1, level=True) -> int:
    """plan_batch_bytes (host/align_plan.hpp): bytes of the mapping file one batch may hold (2**64 - 1: no limit)."""
    L = _host()
    L.wfmh_test_plan_batch_bytes.restype = C.c_ulonglong
    L.wfmh_test_plan_batch_bytes.argtypes = [C.c_ulonglong] * 9 + [C.c_int]
    return int(L.wfmh_test_plan_batch_bytes(file_bytes, rows, row_bytes, row_bases_sum, batch_records, batch_bases, nworkers, ngpu, min_batches, 1 if level else 0))


def host_align_plan(op: int, values, out_size: int):
    """wfmh_test_align_plan: one function of the align driver's planner (host/align_plan.hpp) on a list of numbers -> out_size doubles.
    op 0 workers_per_gpu(threads, ngpu, override); 1 estimate_batches(file_bytes, rows, row_bytes, row_bases_sum, batch_records, batch_bases,
    batch_bytes) with -1 for "no limit", -1 back for "unknown"; 2 interval_union of (from, to) pairs -> count, total, the intervals;
    3 its twenty-bin histogram -> total, span, the bins."""
    L = _host()
    L.wfmh_test_align_plan.restype = C.c_int
    L.wfmh_test_align_plan.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double)]
    v = (C.c_double * max(1, len(values)))(*values)
    out = (C.c_double * out_size)()
    rc = L.wfmh_test_align_plan(op, v, len(values) // 2 if op >= 2 else len(values), out)
    if rc != 0:
        raise WfmError(f"wfmh_test_align_plan failed ({rc})")
    return list(out)


def host_patch_plan(cigar: str):
    """plan_patches (host/cigar_ops.hpp) of a main CIGAR: dict(head=(query_eroded, target_eroded, runs eroded),
    tail=(query_eroded, target_eroded, index of the first eroded run), head_wanted, tail_wanted, tail_independent)."""
    v = [int(x) for x in host_cigar_fn("patch_plan", cigar).split(",")]
    return dict(head=tuple(v[0:3]), tail=tuple(v[3:6]), head_wanted=bool(v[6]), tail_wanted=bool(v[7]), tail_independent=bool(v[8]))


SCORE_NONE, SUB_NONE = 2**31 - 1, 1 << 29  # Node::score_rem of a root; "no bound of the score" (csrc/wfa_device.h)


def ring_plan(pl, tl, mem_budget, score_rem=SCORE_NONE, sub=SUB_NONE, noband=0, band=0, tiles=True, min_len=128, min_score=64, chunk=2, T=100,
              RR=32, use_band=False, over_budget=False, roots_off=False, band_root=4096):
    """plan_ring of csrc/wfa_plan.h (no GPU): the ring a BiWFA job gets -- dict(width, koff, band, tile_it, grown, need), or None
    where the job's score is beyond the budget (WFM_ST_OOM)."""
    L = load()
    L.wfmh_test_ring_plan.restype = C.c_int
    L.wfmh_test_ring_plan.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_ulonglong, C.POINTER(C.c_int64)]
    node = (C.c_int32 * 6)(pl, tl, score_rem, sub, noband, band)
    rules = (C.c_int32 * 10)(int(tiles), min_len, min_score, chunk, T, RR, int(use_band), int(over_budget), int(roots_off), band_root)
    out = (C.c_int64 * 6)()
    rc = L.wfmh_test_ring_plan(node, rules, mem_budget, out)
    if rc != 0:
        assert rc == -200, rc
        return None
    return dict(width=out[0], koff=out[1], band=out[2], tile_it=bool(out[3]), grown=bool(out[4]), need=out[5])


def expand_runs(runs, plen, tlen, pen=DEFAULT_PEN, rle=False, ops_cap=None, before=()):
    """expand_runs of csrc/wfa_plan.h (no GPU): (code, score, n_runs, ops_len, output) for a problem's runs ((len << 2) | op); the
    output is the op bytes written, or with rle the run vector afterwards -- it held `before` when the call began."""
    L = load()
    L.wfmh_test_expand_runs.restype = C.c_int
    L.wfmh_test_expand_runs.argtypes = [C.POINTER(C.c_uint32), C.c_int, C.POINTER(Penalties), C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t,
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(C.c_int64)]
    e = (C.c_uint32 * max(1, len(runs)))(*runs)
    pn = Penalties(*pen)
    cap = sum(r >> 2 for r in runs) if ops_cap is None else ops_cap
    ops = C.create_string_buffer(cap + 1)
    vcap = len(before) + len(runs)
    vec = (C.c_uint32 * max(1, vcap))(*before)
    nvec = C.c_size_t(len(before))
    res = (C.c_int64 * 3)()
    rc = L.wfmh_test_expand_runs(e, len(runs), C.byref(pn), plen, tlen, 1 if rle else 0, ops, cap, vec, C.byref(nvec), vcap, res)
    out = list(vec[:nvec.value]) if rle else ops.raw[:res[2]]
    return rc, int(res[0]), int(res[1]), int(res[2]), out


def align_paf(handle, target_fasta, mapping_paf, out_paf, query_fasta=None, params=None):
    """wfmh_align_paf: the align phase on files (mapping PAF in, aligned PAF out)."""
    L = _host()
    prm = AlignParams()
    L.wfmh_align_default_params(C.byref(prm))
    for k, v in (params or {}).items():
        setattr(prm, k, v)
    summ = AlignSummary()
    rc = L.wfmh_align_paf(handle._p, target_fasta.encode(), query_fasta.encode() if query_fasta else None,
                          mapping_paf.encode(), out_paf.encode(), C.byref(prm), C.byref(summ))
    if rc != 0:
        raise WfmError(f"wfmh_align_paf failed ({rc}): {handle.last_error()}")
    return summ


def read_record_tags(path):
    """The align driver's diagnostic channel (WFM_RECORD_TAGS=<file>, host/aligner.cpp): {row of the mapping file: (tags, score, ok)}
    with tags = WFM_PF_* of the main alignment | of the head patch << 8 | of the tail patch << 16."""
    out = {}
    with open(path) as f:
        for line in f:
            a = line.split()
            if len(a) >= 4:
                out[int(a[0])] = (int(a[1]), int(a[2]), int(a[3]))
    return out


def stratified_rows(tags, n_rows, per_stratum=64, top_scores=32, uniform=64):
    """Rows of a mapping file to hold against the oracle, drawn where the align path has broken before rather than uniformly:
    every record (up to per_stratum each) whose root or a child ran again, whose patches went to a second / third budget or to the
    ring kernel, which ran on the byte kernels, whose overlap walk took several rounds; the top_scores highest scores; then every
    k-th row.  Returns (sorted rows, {stratum: count})."""
    strata = {
        "root_again": lambda t: t & WFM_PF_ROOT_AGAIN,
        "job_again": lambda t: t & WFM_PF_JOB_AGAIN,
        "patch_second_budget": lambda t: (t >> 8 | t >> 16) & WFM_PF_BASE_RETRY,
        "patch_third_budget": lambda t: (t >> 8 | t >> 16) & WFM_PF_BASE_RETRY2,
        "ring_kernel": lambda t: (t | t >> 8 | t >> 16) & WFM_PF_RING_KERNEL,
        "base_tiles": lambda t: (t >> 8 | t >> 16) & WFM_PF_BASE_TILES,
        "byte_kernel": lambda t: (t | t >> 8 | t >> 16) & WFM_PF_BYTE_KERNEL,
        "p2_rounds": lambda t: t & WFM_PF_P2_ROUNDS,
        "leaf_retry": lambda t: t & (WFM_PF_BASE_RETRY | WFM_PF_BASE_RETRY2),
    }
    rows, counts = set(), {}
    for name, pred in strata.items():
        hit = sorted(r for r, (t, _, ok) in tags.items() if pred(t))
        counts[name] = len(hit)
        step = max(1, len(hit) // per_stratum)
        rows.update(hit[::step][:per_stratum])
    by_score = sorted(tags, key=lambda r: -tags[r][1])[:top_scores]
    rows.update(by_score)
    counts["top_scores"] = len(by_score)
    if uniform and n_rows:
        rows.update(range(0, n_rows, max(1, n_rows // uniform)))
    counts["sampled"] = len(rows)
    return sorted(r for r in rows if r < n_rows), counts


def align_paf_multi(handles, target_fasta, mapping_paf, out_paf, query_fasta=None, params=None):
    """wfmh_align_paf_multi: the align phase over several GPUs of the node."""
    L = _host()
    L.wfmh_align_paf_multi.restype = C.c_int
    L.wfmh_align_paf_multi.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                       C.POINTER(AlignParams), C.POINTER(AlignSummary)]
    prm = AlignParams()
    L.wfmh_align_default_params(C.byref(prm))
    for k, v in (params or {}).items():
        setattr(prm, k, v)
    summ = AlignSummary()
    rc = L.wfmh_align_paf_multi(_handle_array(handles), len(handles), target_fasta.encode(), query_fasta.encode() if query_fasta else None,
                                mapping_paf.encode(), out_paf.encode(), C.byref(prm), C.byref(summ))
    if rc != 0:
        raise WfmError(f"wfmh_align_paf_multi failed ({rc}): {handles[0].last_error()}")
    return summ


def host_winnow(seq: bytes, k: int, w: int, s: int, seq_id: int, hashes, strands):
    """Host winnowing stage on caller-supplied canonical k-mer hashes (no GPU needed)."""
    L = load()
    L.wfmh_test_winnow.restype = C.c_int64
    L.wfmh_test_winnow.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    cap = 4 * len(seq) + 64
    out = np.zeros(cap, dtype=MINMER_DTYPE)
    hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
    strands = np.ascontiguousarray(strands, dtype=np.int8)
    n = L.wfmh_test_winnow(seq, len(seq), k, w, s, seq_id, hashes.ctypes.data, strands.ctypes.data, out.ctypes.data, cap)
    return out[:n]


def host_index_file(op: str, fasta: str, out_path: str, in_path: str = None, prefix_delim: str = "#"):
    """wfmh_test_index_file: 'ids' (id section of fasta's sequences) or 'rewrite' (read + write every sub-index)."""
    L = load()
    f = L.wfmh_test_index_file
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, C.c_char_p, C.c_char, C.c_char_p, C.c_char_p]
    rc = f(op.encode(), fasta.encode(), (prefix_delim or "\0").encode(), in_path.encode() if in_path else None, out_path.encode())
    if rc != 0:
        raise WfmError(f"wfmh_test_index_file({op}) failed")


def host_sort_records(recs, threads: int):
    """wfmh_test_sort_records: the closing (wpos, wpos_end) sort of a sequence's records; returns a sorted copy."""
    L = load()
    L.wfmh_test_sort_records.restype = None
    L.wfmh_test_sort_records.argtypes = [C.c_void_p, C.c_int64, C.c_int]
    a = np.array(recs, dtype=MINMER_DTYPE, copy=True)
    L.wfmh_test_sort_records(a.ctypes.data, len(a), threads)
    return a


def host_winnow_thinned(seq: bytes, k: int, w: int, s: int, seq_id: int, hashes, strands, c_factor: float = 4.0, chunk_len: int = 0):
    """The chunked host winnowing on the thinned stream (selection restated on the host); returns
    (minmers, kept positions, replays)."""
    L = load()
    f = L.wfmh_test_winnow_thinned
    f.restype = C.c_int64
    f.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_int64, C.c_void_p,
                  C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    cap = 4 * len(seq) + 64
    out = np.zeros(cap, dtype=MINMER_DTYPE)
    kept = np.zeros(len(seq) + 1, dtype=np.uint32)
    hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
    strands = np.ascontiguousarray(strands, dtype=np.int8)
    rep = C.c_int(0)
    nk = C.c_int64(0)
    n = f(seq, len(seq), k, w, s, seq_id, hashes.ctypes.data, strands.ctypes.data, c_factor, chunk_len, out.ctypes.data, cap,
          kept.ctypes.data, len(kept), C.byref(nk), C.byref(rep))
    return out[:n], kept[:nk.value], rep.value


def host_winnow_model(seq: bytes, k: int, w: int, s: int, seq_id: int, hashes, strands, c_factor: float = 3.0, chunk_len: int = 0):
    """The device winnower's control flow and capacities on the host (map_winnow.hip's model) over the thinned stream;
    returns (minmers or None when the device would hand the sequence back, why-bits)."""
    L = load()
    f = L.wfmh_test_winnow_model
    f.restype = C.c_int64
    f.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_int64, C.c_void_p,
                  C.c_int64, C.POINTER(C.c_uint32)]
    cap = 4 * len(seq) + 64
    out = np.zeros(cap, dtype=MINMER_DTYPE)
    hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
    strands = np.ascontiguousarray(strands, dtype=np.int8)
    why = C.c_uint32(0)
    n = f(seq, len(seq), k, w, s, seq_id, hashes.ctypes.data, strands.ctypes.data, c_factor, chunk_len, out.ctypes.data, cap, C.byref(why))
    return (None if n < 0 else out[:n]), why.value


def host_sortlike_model(recs):
    """map_finish.hip's data-parallel restatement of std::sort's arrangement, run on the host; returns the sorted copy."""
    L = load()
    f = L.wfmh_test_sortlike_model
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_int64]
    out = np.ascontiguousarray(recs, dtype=MINMER_DTYPE).copy()
    f(out.ctypes.data, len(out))
    return out


def host_finish_records(raw, w: int):
    """cut / strand sign / std::sort / de-duplication of raw interval records on the host (finish_records)."""
    L = load()
    f = L.wfmh_test_finish_records
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64]
    raw = np.ascontiguousarray(raw, dtype=MINMER_DTYPE)
    cap = 4 * len(raw) + 64
    while True:
        out = np.zeros(cap, dtype=MINMER_DTYPE)
        n = f(raw.ctypes.data, len(raw), w, out.ctypes.data, cap)
        if n <= cap:
            return out[:n]
        cap = n


def host_winnow_chunked(seq: bytes, k: int, w: int, s: int, seq_id: int, hashes, strands, chunk_len: int):
    """The speculative chunked form of the host winnowing (single thread); returns (minmers, replays).
    replays = chunks whose speculation failed and were replayed; -1 = fell back to one stream."""
    L = load()
    f = L.wfmh_test_winnow_chunked
    f.restype = C.c_int64
    f.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                  C.POINTER(C.c_int)]
    cap = 4 * len(seq) + 64
    out = np.zeros(cap, dtype=MINMER_DTYPE)
    hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
    strands = np.ascontiguousarray(strands, dtype=np.int8)
    rep = C.c_int(0)
    n = f(seq, len(seq), k, w, s, seq_id, hashes.ctypes.data, strands.ctypes.data, chunk_len, out.ctypes.data, cap, C.byref(rep))
    return out[:n], rep.value
