"""ctypes binding of librb_hip.so (the C ABI of include/rb_capi.h).

There is NO CPU fallback: if the HIP library is missing or cannot be loaded, importing this module
raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported from here.)
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "librb_hip.so")

RB_OK = 0
DBGBF, CBF, RPKBF, FPKBF = 0, 1, 2, 3
ADD_REVCOMP, ADD_COUNT_IF_PRESENT, ADD_STORE_READ_PAIRS, ADD_PAIRS_IF_PRESENT = 1, 2, 4, 8
OP_ADD, OP_ADD_IF_ABSENT, OP_ADD_COUNT_IF_PRESENT, OP_ADD_DBG_ONLY, OP_ADD_COUNT_ONLY, \
    OP_ADD_READ_PAIR, OP_ADD_FRAG_PAIR = range(7)
PROF_MAX = 32
SLOT_REC_KEYS, SLOT_REC_OCC, SLOT_PAIR_IDX, SLOT_DREQ_IDX, SLOT_DREQ_PROBE, SLOT_CREQ_IDX, SLOT_W_IDX, SLOT_W_VAL, \
    SLOT_CONF_EDGES, SLOT_CONF_RUNS, SLOT_CONF_OPS, SLOT_CW_IDX, SLOT_CW_VAL, SLOT_Q_BIDX, SLOT_Q_CIDX, SLOT_CACHE_UPD, SLOT_ORD_IDX = range(17)
MODE_ADD, MODE_COUNT_IF_PRESENT = 0, 2
STROBE_CANONICAL, STROBE_SLIDE = 1, 2
# rb_graph_screen_fragments: `what` and rb_screen_rec.flags, then the flags of a sequence that was not judged; chim_why; blunt_why
SCREEN_BRANCH_FREE, SCREEN_CHIMERA, SCREEN_BLUNT_END, SCREEN_BAD_LETTER, SCREEN_NO_KMER, SCREEN_OVER_BUDGET = 1, 2, 4, 8, 16, 32
CHIM_WHY_ENDS, CHIM_WHY_ASSEMBLED, CHIM_WHY_WIDE_GAP, CHIM_WHY_PATHS_MEET, CHIM_WHY_DISJOINT = range(5)
BLUNT_WHY_NO_ARM, BLUNT_WHY_LEFT_RANGE, BLUNT_WHY_RIGHT_RANGE, BLUNT_WHY_LEFT_FAILED, BLUNT_WHY_RIGHT_FAILED, BLUNT_WHY_LEFT_ARTIFACT, \
    BLUNT_WHY_RIGHT_ARTIFACT = range(7)
SCREEN_DEFAULT_VISITS = 65536
# rb_graph_represented: rb_repr_rec.flags bit 0 (its not-judged bits are SCREEN_BAD_LETTER / SCREEN_NO_KMER / SCREEN_OVER_BUDGET), why, path_form
REPR_REPRESENTED = 1
SCREEN_NOT_REACHED = 64         # rb_graph_represented_then_add: a sequence behind an over-budget stop (the next not-judged bit)
REPR_WHY_TRUE, REPR_WHY_NO_RUN, REPR_WHY_LEFT_LENGTH, REPR_WHY_LEFT_IDENTITY, REPR_WHY_WIDE_GAP, REPR_WHY_NO_PATH, REPR_WHY_PATH_LENGTH, \
    REPR_WHY_PATH_IDENTITY, REPR_WHY_RIGHT_LENGTH, REPR_WHY_RIGHT_IDENTITY = range(10)
REPR_PATH_NONE, REPR_PATH_LEFT, REPR_PATH_RIGHT, REPR_PATH_SPLICED = range(4)
# rb_graph_trim_rc_artifacts: mode; rb_trim_rec.flags (a sequence that is not judged carries SCREEN_BAD_LETTER / SCREEN_NO_KMER, or TRIM_NOT_JUDGED)
TRIM_HASHES, TRIM_EDGE, TRIM_LONG = range(3)
TRIM_FOUND, TRIM_TRIMMED, TRIM_NOT_JUDGED = 1, 2, 32
# rb_graph_correct_long: rb_long_rec.status, rb_long_rec.flags
LONG_NULL, LONG_UNCHANGED, LONG_CHANGED, LONG_NO_KMER = range(4)
LONG_OVERFLOW, LONG_TRIMMED_TO_NOTHING = 1, 2
# rb_graph_extend_loop: which; rb_extend_loop_rec.status, why, left_end / right_end; the record's fields (64 bytes; a numpy dtype is made of them)
EXTL_SE, EXTL_PE = 0, 1
EXTL_DONE, EXTL_ROOM, EXTL_NOT_JUDGED = range(3)
EXTL_WHY_NONE, EXTL_WHY_NO_KMER, EXTL_WHY_LETTER = range(3)
EXTL_END_NOT_RUN, EXTL_END_NOTHING, EXTL_END_USED_SHORT, EXTL_END_USED_PAIR, EXTL_END_ROOM = range(5)
EXTL_REC_FIELDS = [("status", "<i4"), ("why", "<i4"), ("left_ext", "<i4"), ("right_ext", "<i4"), ("out_len", "<i4"), ("left_end", "<i4"),
                   ("right_end", "<i4"), ("left_rounds", "<i4"), ("right_rounds", "<i4"), ("steps", "<i4"), ("floor_drops", "<i4"),
                   ("used_passed", "<i4"), ("left_floor", "<f4"), ("right_floor", "<f4"), ("pad", "<i4", (2,))]
EXTL_MAX_ROOM = 1 << 24
# rb_graph_naive_extend_fragments: rb_naive_frag_rec.status, why, left_end / right_end; the record's fields (64 bytes); the most k-mers + 2 room
# of a fragment whose terminator table stays in LDS (csrc/rb_naive_frag.hip NF_LDS_ENTRIES): beyond it the table is a row of device scratch
NFRAG_DONE, NFRAG_ROOM, NFRAG_NOT_JUDGED = range(3)
NFRAG_WHY_NONE, NFRAG_WHY_NO_KMER, NFRAG_WHY_LETTER = range(3)
NFRAG_END_NOT_RUN, NFRAG_END_NO_NEIGHBOUR, NFRAG_END_BACK_BRANCH, NFRAG_END_SEVERAL, NFRAG_END_MEMBER, NFRAG_END_ROOM = range(6)
NFRAG_REC_FIELDS = [("status", "<i4"), ("why", "<i4"), ("left_ext", "<i4"), ("right_ext", "<i4"), ("out_len", "<i4"), ("left_end", "<i4"),
                    ("right_end", "<i4"), ("left_hit", "<i4"), ("right_hit", "<i4"), ("pad", "<i4", (7,))]
NFRAG_MAX_ROOM = 1 << 24
NAIVE_FRAG_LDS_ENTRIES = 1024
# rb_graph_correct_pairs: rb_pairc_rec.status, end, flags; the record's fields (64 bytes; a numpy dtype is made of them)
PAIRC_UNCHANGED, PAIRC_CORRECTED, PAIRC_NOT_JUDGED = range(3)
PAIRC_END_ALL, PAIRC_END_NO_CHANGE, PAIRC_END_LOW, PAIRC_END_NO_KMER, PAIRC_END_LOST_KMERS = range(5)
PAIRC_LEFT, PAIRC_RIGHT, PAIRC_LEFT_OVERFLOW, PAIRC_RIGHT_OVERFLOW = 1, 2, 4, 8
# rb_long_prepare: rb_prep_rec.status, rb_prep_rec.flags; the record's fields (64 bytes; a numpy dtype is made of them)
PREP_SHORT, PREP_LOW_COMPLEXITY, PREP_SEGMENTS = range(3)
PREP_REVCOMP, PREP_HAS_POLYA, PREP_TAIL_FOUND, PREP_HEAD_FOUND, PREP_CUT_FIRED, PREP_ROUTE_WINDOWS, PREP_ROUTE_WINDOWED, PREP_ROUTE_WHOLE, \
    PREP_MAPPED_TWICE = 1, 2, 4, 8, 16, 32, 64, 128, 256
PREP_REC_FIELDS = [("status", "<i4"), ("flags", "<i4"), ("kept_begin", "<i4"), ("kept_end", "<i4"), ("tail_start", "<i4"), ("tail_end", "<i4"),
                   ("head_start", "<i4"), ("head_end", "<i4"), ("n_windows", "<i4"), ("n_low", "<i4"), ("offset", "<i4"), ("n_segments", "<i4"),
                   ("tail_searches", "<i4"), ("head_searches", "<i4"), ("reserved", "<i4", (2,))]
PREP_MAX_LC_WINDOW = 1024
# rb_subsample_reads: rb_subsample_params.mode; the record's status; the reference line that decided (R/util/SeqSubsampler.java); the record's
# eight ints in order (k-mer mode: nam_start is `start`, nam_end the missingChainLen the loop ended with)
SUB_STROBEMER, SUB_KMER = 0, 1
SUB_DROPPED, SUB_KEPT_SCAN, SUB_KEPT_TAIL, SUB_KEPT_START_FAILED, SUB_NOT_JUDGED = range(5)
SUB_LINE_SEEN_BEYOND_EDGE, SUB_LINE_MERGE_FAILED, SUB_LINE_UNSEEN_BEYOND_EDGE, SUB_LINE_GAP, SUB_LINE_TAIL, SUB_LINE_START_FAILED = \
    402, 408, 414, 421, 429, 456
SUB_LINE_KMER_START_FAILED, SUB_LINE_KMER_RANGE, SUB_LINE_KMER_CHAIN, SUB_LINE_KMER_NO_CHAIN = 153, 178, 191, 197
SUB_LINE_KMER_START_FAILED_C, SUB_LINE_KMER_RANGE_C, SUB_LINE_KMER_CHAIN_C, SUB_LINE_KMER_NO_CHAIN_C = 236, 263, 277, 283
SUB_REC_FIELDS = ("status", "line", "index", "nam_start", "nam_end", "elements", "unseen", "incremented")
SUB_LDS_ELEMS = 2048
PAIRC_REC_FIELDS = [("status", "<i4"), ("end", "<i4"), ("rounds_run", "<i4"), ("flags", "<i4"), ("left_len", "<i4"), ("right_len", "<i4"),
                    ("thr_first", "<u4"), ("thr_last", "<u4"), ("found_first", "<i4"), ("left_changed", "<i4"), ("right_changed", "<i4"),
                    ("gaps_replaced", "<i4"), ("gaps_trimmed", "<i4"), ("gaps_kept", "<i4"), ("mismatches", "<i4"), ("reserved", "<i4")]


class GraphParams(C.Structure):
    _fields_ = [("dbgbf_bits", C.c_int64), ("cbf_bytes", C.c_int64), ("pkbf_bits", C.c_int64),
                ("dbgbf_num_hash", C.c_int32), ("cbf_num_hash", C.c_int32), ("pkbf_num_hash", C.c_int32),
                ("k", C.c_int32), ("stranded", C.c_int32), ("use_read_paired_kmers", C.c_int32),
                ("device", C.c_int32), ("group_bits", C.c_int32), ("rng_seed", C.c_uint64),
                ("max_batch_kmers", C.c_int64)]


class AddStats(C.Structure):
    _fields_ = [("reads", C.c_int64), ("kmers", C.c_int64), ("pairs", C.c_int64),
                ("distinct", C.c_int64), ("conflict_ops", C.c_int64), ("sorted_kmers", C.c_int64)]


class SynthParams(C.Structure):
    _fields_ = [("n_pairs", C.c_int64), ("genome_bases", C.c_int64), ("read_len", C.c_int32),
                ("frag_mean", C.c_int32), ("frag_sd", C.c_int32), ("sub_rate", C.c_float),
                ("n_rate", C.c_float), ("expr_sigma", C.c_float), ("seed", C.c_uint64),
                ("tx_min", C.c_int32), ("tx_max", C.c_int32), ("pair_offset", C.c_int64), ("total_pairs", C.c_int64)]


COV_READS, COV_WINDOWS = 0, 1
COV_SE_FOUND, COV_PE_FOUND = 1, 2


class CovParams(C.Structure):
    _fields_ = [("segments", C.c_int32), ("window", C.c_int32), ("lookahead", C.c_int32),
                ("max_cov_gradient", C.c_float), ("cov_fpr", C.c_float), ("min_kmer_cov", C.c_float)]


class CovStats(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_solid", C.c_int32), ("n_complex", C.c_int32), ("flags", C.c_uint32),
                ("min", C.c_float), ("q1", C.c_float), ("median", C.c_float), ("q3", C.c_float), ("max", C.c_float),
                ("dropoff", C.c_float), ("se_threshold", C.c_float), ("pe_threshold", C.c_float)]


assert C.sizeof(CovParams) == 24 and C.sizeof(CovStats) == 48


class CorrParams(C.Structure):
    _fields_ = [("lookahead", C.c_int32), ("max_indel_size", C.c_int32), ("percent_identity", C.c_float), ("min_kmer_cov", C.c_float)]


assert C.sizeof(CorrParams) == 16


class PairCorrParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("lookahead", C.c_int32), ("max_indel_size", C.c_int32), ("max_cov_gradient", C.c_float),
                ("cov_fpr", C.c_float), ("min_cov_threshold", C.c_float), ("percent_identity", C.c_float), ("min_kmer_cov", C.c_float)]


class PairCorrRec(C.Structure):
    _fields_ = [(name, C.c_uint32 if t == "<u4" else C.c_int32) for name, t in PAIRC_REC_FIELDS]


assert C.sizeof(PairCorrParams) == 32 and C.sizeof(PairCorrRec) == 64


class LongParams(C.Structure):
    _fields_ = [("max_itr", C.c_int32), ("lookahead", C.c_int32), ("max_indel_size", C.c_int32), ("min_kmer_cov", C.c_int32),
                ("min_num_solid", C.c_int32), ("trim_low_cov_edges", C.c_int32), ("window_size", C.c_int32),
                ("max_cov_gradient", C.c_float), ("percent_identity", C.c_float)]


assert C.sizeof(LongParams) == 36


class PrepParams(C.Structure):
    _fields_ = [("min_len", C.c_int32), ("reverse_complement", C.c_int32), ("strand_specific", C.c_int32), ("polya", C.c_int32),
                ("seed_length", C.c_int32), ("max_gap", C.c_int32), ("window", C.c_int32), ("lc_window", C.c_int32),
                ("lc_min_length", C.c_int32), ("min_identity", C.c_float)]


assert C.sizeof(PrepParams) == 40


class SubsampleParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("k", C.c_int32), ("wmin", C.c_int32), ("wmax", C.c_int32), ("canonical", C.c_int32),
                ("max_multiplicity", C.c_int32), ("max_edge_clip", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(SubsampleParams) == 32


class Profile(C.Structure):
    _fields_ = [("n", C.c_int32), ("name", C.c_char_p * PROF_MAX), ("ms", C.c_double * PROF_MAX),
                ("launches", C.c_int64 * PROF_MAX)]


# every symbol include/rb_capi.h declares: (name, restype, argtypes)
_vp, _i64, _i32, _u64, _u32, _sz = C.c_void_p, C.c_int64, C.c_int, C.c_uint64, C.c_uint32, C.c_size_t
SYMBOLS = [
    ("rb_last_error", C.c_char_p, []),
    ("rb_version", _i32, []),
    ("rb_build_id", C.c_char_p, []),
    ("rb_graph_create", _i32, [C.POINTER(GraphParams), C.POINTER(_vp)]),
    ("rb_graph_destroy", _i32, [_vp]),
    ("rb_graph_clear", _i32, [_vp, C.c_uint]),
    ("rb_graph_set_read_paired_kmer_distance", _i32, [_vp, _i32]),
    ("rb_graph_set_frag_paired_kmer_distance", _i32, [_vp, _i32]),
    ("rb_graph_init_fragment_pairs", _i32, [_vp, _i64, _i32]),
    ("rb_graph_get_op_ordinal", _i32, [_vp, C.POINTER(_u64)]),
    ("rb_graph_set_op_ordinal", _i32, [_vp, _u64]),
    ("rb_batch_create_ascii", _i32, [_i32, _vp, _vp, _vp, _i64, _i32, C.POINTER(_vp)]),
    ("rb_batch_destroy", _i32, [_vp]),
    ("rb_batch_info", _i32, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    ("rb_batch_download_ascii", _i32, [_vp, _i64, _i64, _vp, _vp]),
    ("rb_batch_create_synthetic", _i32, [_i32, C.POINTER(SynthParams), C.POINTER(_vp)]),
    ("rb_graph_add_batch", _i32, [_vp, _vp, C.c_uint, C.POINTER(AddStats)]),
    ("rb_graph_add_batch_range", _i32, [_vp, _vp, _i64, _i64, C.c_uint, C.POINTER(AddStats)]),
    ("rb_graph_add_pairs", _i32, [_vp, _vp, _i64, _i64, _i32, C.c_uint, C.POINTER(AddStats)]),
    ("rb_graph_add_fragments", _i32, [_vp, _vp, _i64, _i64, _i32, C.POINTER(AddStats)]),
    ("rb_graph_add_reads", _i32, [_vp, _vp, _vp, _vp, _i64, _i32, C.c_uint, C.POINTER(AddStats)]),
    ("rb_graph_apply", _i32, [_vp, _i32, _vp, _sz]),
    ("rb_graph_contains", _i32, [_vp, _vp, _sz, _vp]),
    ("rb_graph_count", _i32, [_vp, _vp, _sz, _vp]),
    ("rb_filter_lookup", _i32, [_vp, _i32, _vp, _sz, _vp]),
    ("rb_filter_lookup_then_add", _i32, [_vp, _i32, _vp, _sz, _vp]),
    ("rb_filter_get_count", _i32, [_vp, _vp, _sz, _vp]),
    ("rb_graph_kmers", _i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    ("rb_graph_batch_counts", _i32, [_vp, _vp, _i64, _i64, _vp, _vp, _i32, _vp]),
    ("rb_graph_read_coverage", _i32, [_vp, _vp, _i64, _i64, _vp, _i64, C.POINTER(CovParams), _vp, _vp, _i32]),
    ("rb_graph_paired_kmer_segments", _i32, [_vp, _i32, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("rb_graph_correct_mismatches", _i32, [_vp, _vp, _vp, _i64, _vp, C.c_float, _vp, _vp, _vp, _vp]),
    ("rb_graph_correct_errors", _i32, [_vp, _vp, _vp, _i64, _vp, C.POINTER(CorrParams), _vp, _vp, _vp, _vp, _vp, _vp]),
    ("rb_graph_correct_pairs", _i32, [_vp, _vp, _vp, _vp, _vp, _i64, C.POINTER(PairCorrParams), _vp, _vp, _vp, _vp, _vp]),
    ("rb_graph_overlap_pairs", _i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, C.c_float, _vp, _vp, _vp]),
    ("rb_graph_extend_se", _i32, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    ("rb_graph_extend_pe", _i32, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    ("rb_graph_extend_loop", _i32, [_vp, _i32, _vp, _vp, _i64, _vp, C.c_float, _i32, _vp, _vp, _vp]),
    ("rb_graph_naive_extend_fragments", _i32, [_vp, _vp, _vp, _i64, _vp, C.c_float, _i32, _vp, _vp, _vp]),
    ("rb_graph_join_pairs", _i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, C.c_float, _i32, C.c_float, _vp, _vp, _vp]),
    ("rb_graph_connect_segments", _i32, [_vp, _vp, _vp, _vp, _i64, _i32, C.c_float, _vp, _vp, _vp, _vp]),
    ("rb_graph_screen_fragments", _i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i64, _vp]),
    ("rb_graph_represented", _i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, C.c_float, _i64, _vp]),
    ("rb_graph_represented_then_add", _i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, C.c_float, _i64, _vp, _vp, _vp, _vp]),
    ("rb_graph_trim_rc_artifacts", _i32, [_vp, _vp, _vp, _i64, _i32, _i32, C.c_float, _vp]),
    ("rb_graph_correct_long", _i32, [_vp, _vp, _vp, _i64, C.POINTER(LongParams), _vp, _vp, _vp]),
    ("rb_graph_neighbors", _i32, [_vp, _vp, _vp, _vp, _sz, _i32, _vp, _vp, _vp]),
    ("rb_graph_walk", _i32, [_vp, _vp, _vp, _sz, _i32, _i32, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("rb_graph_greedy_extend", _i32, [_vp, _vp, _vp, _sz, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    ("rb_graph_naive_extend", _i32, [_vp, _vp, _sz, _i32, _i32, _i32, _i32, C.c_float, _vp, _vp, _vp, _vp, _vp]),
    ("rb_filter_size", _i32, [_vp, _i32, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i32)]),
    ("rb_filter_popcount", _i32, [_vp, _i32, C.POINTER(_i64)]),
    ("rb_filter_fpr", _i32, [_vp, _i32, C.POINTER(C.c_float)]),
    ("rb_filter_fold", _i32, [_vp, _i32, C.POINTER(_u64)]),
    ("rb_filter_export", _i32, [_vp, _i32, _vp, _sz]),
    ("rb_filter_import", _i32, [_vp, _i32, _vp, _sz]),
    ("rb_expected_size", _i64, [_i64, C.c_float, _i32]),
    ("rb_graph_destroy_filter", _i32, [_vp, _i32]),
    ("rb_filter_increment_and_get", _i32, [_vp, _vp, _sz, _vp]),
    ("rb_cbf_to_bloom", _i32, [_vp, C.c_float, _vp, _i32]),
    ("rb_nthash_batch", _i32, [_vp, _i32, _i32, _i64, _i64, C.POINTER(_i64), _vp, _vp, _vp]),
    ("rb_minimizers", _i32, [_i32, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    ("rb_strobemers", _i32, [_i32, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    ("rb_randstrobes", _i32, [_i32, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    ("rb_strobe3", _i32, [_i32, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    ("rb_kmer_pair_hashes", _i32, [_i32, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    ("rb_minimizers_next", _i32, [_i32, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    ("rb_minimizer_set", _i32, [_i32, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    ("rb_long_prepare", _i32, [_i32, _vp, _vp, _i64, C.POINTER(PrepParams), _vp, _vp, _vp, _vp, C.POINTER(C.c_double)]),
    ("rb_subsample_reads", _i32, [_vp, C.POINTER(SubsampleParams), _vp, _vp, _i64, _vp, _vp, _vp]),
    ("rb_fastq_split", _i32, [_vp, _sz, _i32, _vp, _vp, _vp, _i64, C.POINTER(_i64)]),
    ("rb_gunzip", _i32, [_vp, _sz, _i32, _vp, _sz, C.POINTER(_sz)]),
    ("rb_batch_create_fastq", _i32, [_i32, _vp, _sz, _i32, _i32, _i32, C.POINTER(_vp), C.POINTER(_sz)]),
    ("rb_batch_create_fasta", _i32, [_i32, _vp, _sz, _i32, C.POINTER(_vp), C.POINTER(_sz), C.POINTER(_i32)]),
    ("rb_graph_add_fasta", _i32, [_vp, _vp, _sz, C.c_uint, C.POINTER(AddStats), C.POINTER(_i64)]),
    ("rb_graph_add_fastq", _i32, [_vp, _vp, _sz, _i32, C.c_uint, C.POINTER(AddStats), C.POINTER(_i64)]),
    ("rb_graph_add_fastq_file", _i32, [_vp, C.c_char_p, _i32, C.c_uint, C.POINTER(AddStats), C.POINTER(_i64)]),
    ("rb_graph_add_fasta_file", _i32, [_vp, C.c_char_p, C.c_uint, C.POINTER(AddStats), C.POINTER(_i64)]),
    ("rb_batch_create_nbits", _i32, [_i32, _vp, _sz, _i64, C.POINTER(_vp), C.POINTER(_sz)]),
    ("rb_nbits_encode", _i32, [_vp, _vp, _i64, _vp, _sz, C.POINTER(_sz)]),
    ("rb_host_alloc", _i32, [_sz, C.POINTER(_vp)]),
    ("rb_host_free", _i32, [_vp]),
    ("rb_batch_download_packed", _i32, [_vp, _i64, _i64, _vp, _vp, _vp, C.POINTER(_i64)]),
    ("rb_packed_stream_create", _i32, [_i32, _i64, _i64, C.POINTER(_vp)]),
    ("rb_packed_stream_begin", _i32, [_vp, _vp, _vp, _vp, _i64, _i64]),
    ("rb_packed_stream_finish", _i32, [_vp, C.POINTER(_vp)]),
    ("rb_packed_stream_destroy", _i32, [_vp]),
    ("rb_graph_add_packed", _i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, C.c_uint, C.POINTER(AddStats)]),
    ("rb_graph_prefetch_packed", _i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i64]),
    ("rb_graph_create_shard", _i32, [C.POINTER(GraphParams), _i32, _i32, C.POINTER(_vp)]),
    ("rb_shard_set_cache_replication", _i32, [_vp, _i32]),
    ("rb_shard_hash", _i32, [_vp, _vp, _i64, _i64, _i64, _i64, _u64, _u32, C.c_uint, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(AddStats)]),
    ("rb_shard_group", _i32, [_vp, _vp, _vp, _i64, _u64, _u32, C.c_uint, C.POINTER(_i64), C.POINTER(_i64)]),
    ("rb_shard_cache_apply", _i32, [_vp, _vp, _i64]),
    ("rb_shard_hash_begin", _i32, [_vp, _vp, _i64, _i64, _u64, _u32, C.c_uint]),
    ("rb_shard_hash_emit", _i32, [_vp]),
    ("rb_shard_hash_group", _i32, [_vp, _vp, _i64, _i64, _i64, _i64, _u64, _u32, C.c_uint, C.POINTER(_i64), C.POINTER(_i64),
                             C.POINTER(_i64), C.POINTER(AddStats)]),
    ("rb_shard_serve", _i32, [_vp, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
    ("rb_shard_resolve", _i32, [_vp, _i32, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(AddStats)]),
    ("rb_shard_order_serve", _i32, [_vp, _vp, _i64, _vp]),
    ("rb_shard_order_finish", _i32, [_vp, _i32, _vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(AddStats)]),
    ("rb_shard_apply_tagged", _i32, [_vp, _vp, _i64]),
    ("rb_shard_apply_writes", _i32, [_vp, _vp, _vp, _i64]),
    ("rb_shard_conflict_route", _i32, [_vp, _vp, _i64, _i64, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(AddStats)]),
    ("rb_shard_conflict_replay", _i32, [_vp, _vp, _i64, _vp, _i64, C.POINTER(_i64)]),
    ("rb_shard_take", _i32, [_vp, _i32, _vp, _i64]),
    ("rb_shard_slot", _i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(_i64)]),
    ("rb_shard_query_make", _i32, [_vp, _i32, _i32, _vp, _sz, C.POINTER(_i64), C.POINTER(_i64)]),
    ("rb_shard_query_serve", _i32, [_vp, _i32, _vp, _i64, _vp, _i64, _vp, _vp]),
    ("rb_shard_query_finish", _i32, [_vp, _i32, _vp, _vp, _vp, _vp]),
    ("rb_shard_trav_begin", _i32, [_vp, _i32, _vp, _vp, _sz, _i32, _i32, _i32, _i32, C.c_float, _vp, _vp, _i32]),
    ("rb_shard_trav_set_gate", _i32, [_vp, _vp]),
    ("rb_shard_trav_advance", _i32, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    ("rb_shard_trav_absorb", _i32, [_vp, _vp, _vp, _vp]),
    ("rb_shard_trav_end", _i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64)]),
    ("rb_shard_comm_unique_id", _i32, [_vp]),
    ("rb_shard_comm_create_rccl", _i32, [_vp, _i32, _i32, _i32, C.POINTER(_vp)]),
    ("rb_shard_comm_create_loopback", _i32, [_i32, C.POINTER(_vp)]),
    ("rb_shard_comm_destroy", _i32, [_vp]),
    ("rb_shard_comm_selftest", _i32, [_vp, _i32, _i32, _i64]),
    ("rb_shard_hash_begin_split", _i32, [_vp, _vp, _i64, _i64, _i64, _i64, C.c_uint64, C.c_uint32, C.c_uint]),
    ("rb_shard_pairs_flush_begin", _i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    ("rb_shard_pairs_flush_end", _i32, [_vp, _vp, C.POINTER(_i64)]),
    ("rb_shard_add_range", _i32, [_vp, _vp, _vp, _i64, _i64, C.c_uint, _i64, C.c_uint32, C.c_uint64, C.POINTER(AddStats)]),
    ("rb_shard_span", _i32, [_vp, _i32, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    ("rb_debug_probe_cbf", _i32, [_vp, _i32, C.POINTER(C.c_float)]),
    ("rb_debug_scan_u32", _i32, [_i32, _vp, _sz, _vp, _i32]),
    ("rb_debug_sort_pairs", _i32, [_i32, _vp, _vp, _i32, _sz, _i32, _i32, _i32, _i32]),
    ("rb_debug_group", _i32, [_i32, _vp, _vp, _sz, _i32, _i32, C.c_uint, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64,
                              _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("rb_debug_select", _i32, [_i32, _vp, _sz, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    ("rb_debug_cache_export", _i32, [_vp, _i32, _vp, _sz, C.POINTER(_u32), C.POINTER(_u32)]),
    ("rb_debug_prefilter", _i32, [_vp, _vp, _i64, _i64, _u64, _u32, _vp, _vp]),
    ("rb_graph_profile_enable", _i32, [_vp, _i32]),
    ("rb_graph_profile_get", _i32, [_vp, C.POINTER(Profile), _i32]),
]


class NativeError(RuntimeError):
    """Counterpart of the RuntimeException the reference's workers raise (R/RNABloom.java:903-905)."""

    def __init__(self, code, msg):
        super().__init__("librb_hip error %d: %s" % (code, msg))
        self.code = code


def load():
    # PyTorch (the multi-GPU driver's collectives) ships its own HIP / HSA runtime.  Two runtimes in one process
    # cannot both open the device: loading librb_hip.so (which binds to /opt/rocm's) and importing torch afterwards
    # ends in "no ROCm-capable device is detected" at the first HIP call.  So when torch is installed it is imported
    # first and librb_hip.so binds to the runtime that is already loaded.  (A process that never imports torch —
    # the reference's JVM through the JNI stub of INTEGRATION.md — can set RB_NO_TORCH_PRELOAD=1.)
    if not os.environ.get("RB_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(LIB_PATH):
        raise ImportError("HIP library %s not built — run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    return lib


lib = load()


def check(rc):
    if rc != RB_OK:
        raise NativeError(rc, (lib.rb_last_error() or b"").decode(errors="replace"))
