"""The rules of rb_graph_correct_pairs restated in Python from the reference's Java, line by line, over what the other rules files hold:

  GraphUtils.correctErrorsPE (R/util/GraphUtils.java:4051-4182): per round the two threshold searches over the mates' sorted counts
  (:4071-4126, test_read_coverage_rules.coverage_stats), the combining rule (:4129-4143, pair_threshold), the min_cov_threshold test (:4145)
  and correctErrorHelper on both mates (test_error_correction_rules.correct_errors);
  GraphUtils.correctErrorsSE (:3998-4049): one search (se_threshold), one run of the helper.

correct_pairs / correct_single return the record of include/rb_capi.h (rb_pairc_rec) as a dict and the final texts.  Hand-worked cases
run on the dictionary graph (k = 5); tests/test_gpu_pair_correction.py applies the same functions to the CPU oracle's filters."""
import os
import re

import numpy as np
import pytest

import test_error_correction_rules as E
from test_error_correction_rules import CORRECTED, REPLACED, TRIMMED, EGraph, correct_errors
from test_mismatch_rules import K, TRUE, sub
from test_read_coverage_rules import PE_FOUND, SE_FOUND, coverage_stats, java_round, pair_threshold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
UNCHANGED, CORRECTED_PAIR, NOT_JUDGED = 0, 1, 2
END_ALL, END_NO_CHANGE, END_LOW, END_NO_KMER, END_LOST_KMERS = range(5)
LEFT, RIGHT, LEFT_OVERFLOW, RIGHT_OVERFLOW = 1, 2, 4, 8
REC_FIELDS = ("status", "end", "rounds_run", "flags", "left_len", "right_len", "thr_first", "thr_last", "found_first", "left_changed", "right_changed",
              "gaps_replaced", "gaps_trimmed", "gaps_kept", "mismatches", "reserved")
DEFAULTS = dict(iterations=2, lookahead=5, max_indel=1, gradient=0.5, fpr=0.01, min_thr=2.0, pid=0.9, min_cov=1.0)


def bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


NONE = bits(-1.0)


def new_record(left, right):
    r = dict.fromkeys(REC_FIELDS, 0)
    r.update(status=UNCHANGED, end=END_ALL, thr_first=NONE, thr_last=NONE, left_len=len(left), right_len=len(right) if right is not None else 0)
    return r


def round_threshold(cl, cr, gradient, fpr):
    """:4071-4143 on the two count lists: (covThreshold or -1, found bits)"""
    l = coverage_stats(cl, 1, gradient, fpr, 1.0, mate_n=len(cr))
    r = coverage_stats(cr, 1, gradient, fpr, 1.0, mate_n=len(cl))
    return F32(pair_threshold(l, r)), (1 if l["flags"] & PE_FOUND else 0) | (2 if r["flags"] & PE_FOUND else 0)


def add_helper_result(rec, gaps, fixed):
    for g in gaps:
        rec["gaps_replaced" if g["outcome"] == REPLACED else "gaps_trimmed" if g["outcome"] == TRIMMED else "gaps_kept"] += 1
    rec["mismatches"] += fixed


def correct_pairs(left, right, k, params, G):
    """correctErrorsPE.  Returns (record, left text, right text); the texts of a pair that is not judged are the input."""
    p = dict(DEFAULTS, **params)
    left, right = bytes(left), bytes(right)
    rec = new_record(left, right)
    if p["iterations"] == 0:
        return rec, left, right
    if len(left) < k or len(right) < k:                      # covs[startIndex] throws (:4088)
        rec.update(status=NOT_JUDGED, end=END_NO_KMER)
        return rec, left, right
    cur = [left, right]
    for rnd in range(p["iterations"]):
        thr, found = round_threshold(G.counts(cur[0]), G.counts(cur[1]), p["gradient"], p["fpr"])
        if rnd == 0:
            rec.update(thr_first=bits(thr), found_first=found)
        rec["thr_last"] = bits(thr)
        if not thr >= F32(p["min_thr"]):                     # the round changes nothing, and neither does any later one
            rec["end"] = END_LOW
            break
        rec["rounds_run"] += 1
        changed = [False, False]
        for side in (0, 1):
            text, flags, gaps, fixed = helper(cur[side], k, thr, p, G)
            add_helper_result(rec, gaps, fixed)
            if flags & CORRECTED:                            # non-null (:4155, :4169)
                cur[side] = text
                changed[side] = True
                rec["left_changed" if side == 0 else "right_changed"] += 1
                rec["flags"] |= LEFT if side == 0 else RIGHT
        if not changed[0] and not changed[1]:
            rec["end"] = END_NO_CHANGE
            break
        if len(cur[0]) < k or len(cur[1]) < k:               # the next round would throw
            rec.update(status=NOT_JUDGED, end=END_LOST_KMERS, left_len=len(left), right_len=len(right))
            return rec, left, right
        rec["end"] = END_ALL
    rec.update(status=CORRECTED_PAIR if rec["flags"] & (LEFT | RIGHT) else UNCHANGED, left_len=len(cur[0]), right_len=len(cur[1]))
    return rec, cur[0], cur[1]


def helper(seq, k, thr, p, G):
    """correct_errors, and the number of replacements its mismatch pass made (correct_errors reports that only as a flag): (text, flags,
    gap records, replacements)"""
    seen = []
    keep = E.correct_mismatches

    def spy(*args):
        out = keep(*args)
        seen.append(int(out[1]))
        return out

    E.correct_mismatches = spy
    try:
        text, flags, gaps = correct_errors(seq, k, thr, p["lookahead"], p["max_indel"], p["pid"], p["min_cov"], G)
    finally:
        E.correct_mismatches = keep
    return text, flags, gaps, seen[0]


def correct_single(seq, k, params, G):
    """correctErrorsSE.  Returns (record, text): the text is the input where the reference returns null."""
    p = dict(DEFAULTS, **params)
    seq = bytes(seq)
    rec = new_record(seq, None)
    if p["iterations"] == 0:
        return rec, seq
    if len(seq) < k:                                         # kmers.isEmpty() (:4007)
        rec["end"] = END_NO_KMER
        return rec, seq
    st = coverage_stats(G.counts(seq), 1, p["gradient"], p["fpr"], 1.0)
    found = bool(st["flags"] & SE_FOUND)
    thr = F32(st["se_threshold"]) if found else F32(-1)
    rec.update(thr_first=bits(thr), thr_last=bits(thr), found_first=1 if found else 0)
    if not found:
        rec["end"] = END_LOW
        return rec, seq
    rec["rounds_run"] = 1
    text, flags, gaps, fixed = helper(seq, k, thr, p, G)
    add_helper_result(rec, gaps, fixed)
    if not flags & CORRECTED:
        rec["end"] = END_NO_CHANGE
        return rec, seq
    rec.update(status=CORRECTED_PAIR, end=END_ALL, flags=LEFT, left_changed=1, left_len=len(text))
    return rec, text


# ---- the threshold of a round, by hand ----
def test_nfp_comes_from_the_longer_mate():
    # left 10 counts, right 100: nFP = round(100 * 0.02) = 2, so the left walk starts at 9 - 2 = 7 and never sees the two 40s on top
    cl = [1, 1, 1, 10, 10, 10, 10, 10, 40, 40]
    cr = [10] * 100
    # left from covs[7] = 10: 10 * 0.5 = 5 >= 10 no ... >= 1 yes: found, 10.  right: all equal, 5 >= 10 never: not found, covs[0] = 10
    assert round_threshold(cl, cr, 0.5, 0.02) == (F32(10), 1)
    # with a mate of 10 nFP = round(0.2) = 0: the walk starts at the top, 40 * 0.5 = 20 >= 40 no, 20 >= 10 yes: found, 40
    assert round_threshold(cl, [10] * 10, 0.5, 0.02) == (F32(-1), 1)       # found left (40) but larger than the right's covs[0] = 10: none
    assert round_threshold(cl, [50] * 10, 0.5, 0.02) == (F32(40), 1)


def test_start_index_at_nfp_and_one_above():
    # fpr 0.5.  n = 5 both: nFP = round(2.5) = 3 (Math.round at one half goes up); startIndex = 4 > 3: lowered to 1
    assert java_round(F32(5) * F32(0.5)) == 3 and java_round(F32(3) * F32(0.5)) == 2 and java_round(F32(1) * F32(0.5)) == 1
    c5 = [1, 4, 9, 9, 9]
    # from covs[1] = 4: 2 >= 1: found, 4 on both sides
    assert round_threshold(c5, c5, 0.5, 0.5) == (F32(4), 3)
    # n = 4 both: nFP = round(2.0) = 2, startIndex = 3 > 2: lowered to 1.  n = 3: nFP = round(1.5) = 2 = startIndex: NOT lowered (:4085 is a strict >)
    assert round_threshold([1, 4, 9, 9], [1, 4, 9, 9], 0.5, 0.5) == (F32(4), 3)
    c3 = [1, 4, 9]
    assert round_threshold(c3, c3, 0.5, 0.5) == (F32(9), 3)                # from covs[2] = 9: 4.5 >= 4: found, 9
    # n = 1 with a mate of 1: nFP = round(0.5) = 1, startIndex 0: not lowered, no pair to test: not found
    assert round_threshold([7], [7], 0.5, 0.5) == (F32(-1), 0)


def test_every_branch_of_the_combining_rule():
    hi, lo = [2, 20, 20, 20], [1, 8, 8, 8]          # found 20; found 8
    flat9, flat30 = [9, 9, 9, 9], [30, 30, 30, 30]  # not found, covs[0] = 9 / 30
    assert round_threshold(hi, lo, 0.5, 0.0) == (F32(8), 3)                # both: the smaller
    assert round_threshold(lo, hi, 0.5, 0.0) == (F32(8), 3)
    assert round_threshold(hi, flat30, 0.5, 0.0) == (F32(20), 1)           # left only, 20 <= 30
    assert round_threshold(hi, flat9, 0.5, 0.0) == (F32(-1), 1)            # left only, but larger than the other's: none
    assert round_threshold(flat30, hi, 0.5, 0.0) == (F32(20), 2)           # right only
    assert round_threshold(flat9, hi, 0.5, 0.0) == (F32(-1), 2)
    assert round_threshold(flat9, flat30, 0.5, 0.0) == (F32(-1), 0)        # neither
    assert round_threshold([20, 20, 2], [20] * 3, 0.5, 0.0) == (F32(20), 1)    # equal counts across mates: <= holds


def test_gradient_one_equal_counts_and_short_lists():
    # the PE comparison is >=: with gradient 1 two equal counts are a drop; the SE comparison is strict and finds none
    assert round_threshold([6, 6, 6], [6, 6], 1.0, 0.0) == (F32(6), 3)
    assert coverage_stats([6, 6, 6], 1, 1.0, 0.0, 1.0)["flags"] & SE_FOUND == 0
    assert round_threshold([6], [6, 6], 1.0, 0.0) == (F32(6), 2)           # one k-mer: nothing to walk; right found 6 <= left's 6
    assert round_threshold([6], [6], 1.0, 0.0) == (F32(-1), 0)
    assert round_threshold([3, 6], [6], 0.5, 0.0) == (F32(6), 1)           # two k-mers: 6 * 0.5 = 3 >= 3
    assert round_threshold([4, 6], [6], 0.5, 0.0) == (F32(-1), 0)


# ---- whole pairs on the dictionary graph (k = 5, TRUE counted 10) ----
P5 = dict(lookahead=2, max_indel=1, pid=0.8, min_cov=1.0, fpr=0.0, gradient=0.5)
BAD = sub(TRUE, 12, "T")                              # windows 8 .. 12 count 0: an SNV gap that is kept, then the mismatch pass replaces the base


def test_iterations_zero_and_one_and_the_threshold_test():
    g = EGraph([(TRUE, 10)])
    rec, l, r = correct_pairs(BAD, TRUE, K, dict(P5, iterations=0), g)
    assert (l, r) == (BAD, TRUE) and (rec["status"], rec["end"], rec["rounds_run"], rec["thr_first"], rec["thr_last"]) == (UNCHANGED, END_ALL, 0, NONE, NONE)
    # one round: left found 10 (10 * 0.5 >= 0), right flat 10: threshold 10 >= 2; the left mate's base is replaced
    rec, l, r = correct_pairs(BAD, TRUE, K, dict(P5, iterations=1), g)
    assert (l, r) == (TRUE, TRUE)
    assert rec == dict(new_record(TRUE, TRUE), status=CORRECTED_PAIR, end=END_ALL, rounds_run=1, flags=LEFT, thr_first=bits(10), thr_last=bits(10),
                       found_first=1, left_changed=1, gaps_kept=1, mismatches=1)
    # two rounds: the second finds nothing below 10 on either mate and no drop: no threshold, END_LOW after one run
    rec, l, r = correct_pairs(BAD, TRUE, K, dict(P5, iterations=2), g)
    assert (l, r) == (TRUE, TRUE) and (rec["end"], rec["rounds_run"], rec["thr_first"], rec["thr_last"], rec["left_changed"]) == (END_LOW, 1, bits(10), NONE, 1)
    # min_cov_threshold exactly met runs; just above it does not
    assert correct_pairs(BAD, TRUE, K, dict(P5, iterations=1, min_thr=10.0), g)[0]["rounds_run"] == 1
    rec, l, r = correct_pairs(BAD, TRUE, K, dict(P5, iterations=3, min_thr=10.5), g)
    assert (l, r) == (BAD, TRUE) and (rec["status"], rec["end"], rec["rounds_run"], rec["thr_last"]) == (UNCHANGED, END_LOW, 0, bits(10))
    # both mates clean: no threshold at all
    rec, l, r = correct_pairs(TRUE, TRUE[3:], K, dict(P5, iterations=2), g)
    assert (rec["status"], rec["end"], rec["thr_first"], rec["found_first"]) == (UNCHANGED, END_LOW, NONE, 0)


def test_nothing_changes_ends_the_loop():
    g = EGraph([(TRUE, 10)])
    s = b"TT" + TRUE[:20]                                   # a left tip without variants: kept, nothing changes
    rec, l, r = correct_pairs(s, TRUE, K, dict(P5, iterations=4), g)
    assert (l, r) == (s, TRUE) and (rec["status"], rec["end"], rec["rounds_run"], rec["gaps_kept"], rec["flags"]) == (UNCHANGED, END_NO_CHANGE, 1, 1, 0)


def test_a_pair_that_changes_in_two_rounds():
    # the refillable bubble of test_error_correction_rules.test_snv_bubble: every window of left + G + right is known thinly (3).  Round 1:
    # counts 10 .. 3 0 0 0 3 .. 10, threshold 10; the SNV gap is replaced by the k + 2 thin k-mers and the mate grows by two letters.  Round 2 runs
    # on that text: its thin k-mers are below 10 again, a path gap now.
    cand = BAD[8:13] + b"G" + BAD[12:17]
    g = EGraph([(TRUE, 10)], extra={cand[i:i + K]: 3 for i in range(K + 2)})
    # on that text: its seven thin k-mers are below 10 again, a path gap now, and the true path between its anchors has five k-mers: 7 - 2 <= 5, so
    # with max_indel_size 2 it goes in and the mate is the true sequence; with 1 it is refused for length and the round changes nothing.
    grown = BAD[:13] + b"G" + BAD[12:]
    one, l1, _ = correct_pairs(BAD, TRUE, K, dict(P5, iterations=1, max_indel=2), g)
    assert l1 == grown and (one["gaps_replaced"], one["left_changed"], one["end"], one["left_len"]) == (1, 1, END_ALL, len(BAD) + 2)
    two, l2, r2 = correct_pairs(BAD, TRUE, K, dict(P5, iterations=2, max_indel=2), g)
    assert (l2, r2) == (TRUE, TRUE)
    assert two == dict(new_record(TRUE, TRUE), status=CORRECTED_PAIR, end=END_ALL, rounds_run=2, flags=LEFT, thr_first=bits(10), thr_last=bits(10),
                       found_first=1, left_changed=2, gaps_replaced=2)
    # a third round finds no threshold on the repaired pair
    three, l3, _ = correct_pairs(BAD, TRUE, K, dict(P5, iterations=3, max_indel=2), g)
    assert l3 == TRUE and (three["end"], three["rounds_run"], three["thr_last"], three["left_changed"]) == (END_LOW, 2, NONE, 2)
    kept, lk, _ = correct_pairs(BAD, TRUE, K, dict(P5, iterations=3, max_indel=1), g)
    assert lk == grown and (kept["end"], kept["rounds_run"], kept["left_changed"], kept["gaps_replaced"], kept["gaps_kept"]) == (END_NO_CHANGE, 2, 1, 1, 1)


def test_a_mate_without_a_kmer_is_not_judged():
    g = EGraph([(TRUE, 10)])
    for l, r in ((BAD, b"ACGA"), (b"", BAD), (b"ACG", b"AC")):
        rec, lo, ro = correct_pairs(l, r, K, dict(P5, iterations=2), g)
        assert (lo, ro) == (l, r) and (rec["status"], rec["end"], rec["rounds_run"], rec["left_len"], rec["right_len"]) == (NOT_JUDGED, END_NO_KMER, 0, len(l), len(r))
    assert correct_pairs(BAD, b"ACGA", K, dict(P5, iterations=0), g)[0]["status"] == UNCHANGED     # nothing runs: nothing throws
    assert correct_pairs(BAD, TRUE[:K], K, dict(P5, iterations=1), g)[0]["status"] != NOT_JUDGED   # one k-mer is a list


def test_single_form():
    g = EGraph([(TRUE, 10)])
    rec, s = correct_single(BAD, K, dict(P5, iterations=3), g)                # runs once whatever iterations > 0 is
    assert s == TRUE and rec == dict(new_record(TRUE, None), status=CORRECTED_PAIR, end=END_ALL, rounds_run=1, flags=LEFT, thr_first=bits(10),
                                     thr_last=bits(10), found_first=1, left_changed=1, gaps_kept=1, mismatches=1)
    assert correct_single(BAD, K, dict(P5, iterations=3, min_thr=1000.0), g)[1] == TRUE       # min_cov_threshold is not read
    rec, s = correct_single(TRUE, K, dict(P5, iterations=1), g)               # no drop: null
    assert s == TRUE and (rec["status"], rec["end"], rec["thr_first"], rec["found_first"]) == (UNCHANGED, END_LOW, NONE, 0)
    rec, s = correct_single(b"ACG", K, dict(P5, iterations=1), g)
    assert s == b"ACG" and (rec["status"], rec["end"]) == (UNCHANGED, END_NO_KMER)
    assert correct_single(BAD, K, dict(P5, iterations=0), g) == (new_record(BAD, None), BAD)
    # strict: 10 * 0.5 = 5 > 5 is false where the pair form's >= holds
    g5 = EGraph([(TRUE, 10)], extra={BAD[i:i + K]: 5 for i in range(8, 13)})
    assert correct_single(BAD, K, dict(P5, iterations=1), g5)[0]["found_first"] == 0
    assert correct_pairs(BAD, TRUE, K, dict(P5, iterations=1), g5)[0]["found_first"] == 1
    # the helper ran and returned null
    s = b"TT" + TRUE[:20]
    rec, out = correct_single(s, K, dict(P5, iterations=1), g)
    assert out == s and (rec["status"], rec["end"], rec["rounds_run"], rec["gaps_kept"]) == (UNCHANGED, END_NO_CHANGE, 1, 1)


# ---- the feature exists at every layer (these fail before it does) ----
def test_header_declares_the_entry_point():
    src = open(os.path.join(ROOT, "include", "rb_capi.h")).read()
    assert re.search(r"\bint rb_graph_correct_pairs\(rb_graph \*g, const char \*lseq, const int64_t \*loffsets, const char \*rseq, const int64_t \*roffsets, "
                     r"int64_t n,\s*const rb_pairc_params \*p, const int64_t \*lout_offsets, char \*lout, const int64_t \*rout_offsets, char \*rout,\s*"
                     r"rb_pairc_rec \*recs\);", src)
    assert "GraphUtils.java:4051-4182" in src and ":3998-4049" in src and "typedef struct rb_pairc_rec" in src


def test_library_exports_and_python_binds_it():
    import ctypes as C
    from rnabloom import _native as N
    assert hasattr(C.CDLL(N.LIB_PATH), "rb_graph_correct_pairs")
    assert "rb_graph_correct_pairs" in {s[0] for s in N.SYMBOLS}
    assert (N.PAIRC_UNCHANGED, N.PAIRC_CORRECTED, N.PAIRC_NOT_JUDGED) == (UNCHANGED, CORRECTED_PAIR, NOT_JUDGED)
    assert (N.PAIRC_END_ALL, N.PAIRC_END_NO_CHANGE, N.PAIRC_END_LOW, N.PAIRC_END_NO_KMER, N.PAIRC_END_LOST_KMERS) == tuple(range(5))
    assert (N.PAIRC_LEFT, N.PAIRC_RIGHT, N.PAIRC_LEFT_OVERFLOW, N.PAIRC_RIGHT_OVERFLOW) == (LEFT, RIGHT, LEFT_OVERFLOW, RIGHT_OVERFLOW)
    from rnabloom import graphutils
    from rnabloom.graph import BloomFilterDeBruijnGraph
    for name in ("correctPairsFlat", "correctPairs", "correctReads"):
        assert callable(getattr(BloomFilterDeBruijnGraph, name, None)), name
    for name in ("correctErrorsPE", "correctErrorsSE", "correctErrorsPEComposed"):
        assert callable(getattr(graphutils, name, None)), name


def test_the_record_is_64_bytes_in_field_order():
    import ctypes as C
    from rnabloom import _native as N
    from rnabloom.graph import BloomFilterDeBruijnGraph
    assert C.sizeof(N.PairCorrRec) == 64 and C.sizeof(N.PairCorrParams) == 32
    assert tuple(f[0] for f in N.PairCorrRec._fields_) == REC_FIELDS
    assert [getattr(N.PairCorrRec, f).offset for f in REC_FIELDS] == [4 * i for i in range(16)]
    dt = BloomFilterDeBruijnGraph.PAIRC_DTYPE
    assert dt.itemsize == 64 and dt.names == REC_FIELDS and [dt.fields[f][1] for f in REC_FIELDS] == [4 * i for i in range(16)]
    assert tuple(f[0] for f in N.PairCorrParams._fields_) == ("iterations", "lookahead", "max_indel_size", "max_cov_gradient", "cov_fpr",
                                                                "min_cov_threshold", "percent_identity", "min_kmer_cov")


def test_java_and_jni_sides_exist():
    java = open(os.path.join(ROOT, "java", "rnabloom", "graph", "NativeGraph.java")).read()
    assert re.search(r"public static native void correctPairs\(long h, ByteBuffer lseq, long\[\] loffsets, ByteBuffer rseq, long\[\] roffsets, int n,", java)
    jni = open(os.path.join(ROOT, "jni", "rb_jni.c")).read()
    assert "FN(correctPairs)" in jni and "rb_graph_correct_pairs(" in jni
    g = open(os.path.join(ROOT, "java", "rnabloom", "graph", "BloomFilterDeBruijnGraph.java")).read()
    assert "NativeGraph.correctPairs(handle" in g
    assert re.search(r"public boolean\[\] correctErrorsPE\(String\[\] lefts, String\[\] rights,", g) and re.search(r"public String\[\] correctErrorsSE\(String\[\] seqs,", g)
