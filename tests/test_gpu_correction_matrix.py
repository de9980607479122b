"""Mismatch and error correction beyond k = 47 and two hash functions: rb_graph_correct_mismatches (k_mismatch in csrc/rb_mismatch.hip) and
rb_graph_correct_errors (k_gap_scan, k_resolve_edge, k_resolve_snv, k_resolve_path, k_stitch, k_text_kmers in csrc/rb_correct.hip, and the walks
under them) on the worlds of tests/correction_worlds.py: k = 16 ... 256 on both sides of 64, 128 and 192 (a lane of k_mismatch owns a second,
third and fourth window, the median of its k - 1 and k codes crosses the register slots, rotations by 64 and more, the gate shuffle from lane
(k - 1) mod 64; k_resolve_snv's k + 2 windows take a second and third step), stranded and canonical, hash counts (1, 1), (3, 4), (2, 3), (3, 1),
(2, 2); gaps of more than 1024 bad k-mers, whose Levenshtein rows live in device scratch, in one call with gaps whose rows fit LDS; a sequence of
more than 4096 windows at k = 129.  Every expected value is the restatements' (tests/test_mismatch_rules.py, tests/test_error_correction_rules.py)
on the CPU oracle's filters; tests/test_correction_reach.py proves on the CPU that the worlds ask something.  Every comparison is exact — bytes,
integers, count rows as equal floats — through check() and compare() of the two device test files of the calls."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rnabloom.graph import _pack

import correction_worlds as CW
import test_gpu_error_correction as EC
import test_gpu_mismatch_correction as MM

IDS = [CW.case_id(c) for c in CW.CASES]


def release(w):
    if w.gg is not None:
        w.gg.destroy(); w.gg = None


@pytest.mark.parametrize("case", CW.CASES, ids=IDS)
def test_mismatch_correction(case):
    w, sets, (changed, reverse_only) = CW.mismatch_case(case)
    mincov = case[3]
    print("mismatch %s mincov=%g: %d of %d planted sequences change, %d by the reverse scan only" % (
        CW.case_id(case), mincov, changed, len(w.planted) + len(w.rev_only), reverse_only))
    w.device()                                                     # (compares dbgbf and cbf with the oracle's, byte for byte)
    try:
        fixed = 0
        for name, seqs in sets.items():
            fixed += sum(n for _, n, _ in MM.check(w, seqs, CW.T, mincov, (name, "fixed")))
        assert fixed >= changed
        everything = sum(sets.values(), [])
        MM.check(w, everything, CW.per_sequence_thresholds(len(everything)), mincov, "per-sequence thresholds")
    finally:
        release(w)


def test_mismatch_long_row_past_a_slot_boundary():
    w, seqs, want = CW.long_row_case()
    assert len(seqs[0]) - w.k + 1 > CW.MM_LDS_ROW and want[0][1] >= 2
    w.device()
    try:
        got = MM.check(w, seqs, CW.T, CW.LONG_ROW_CASE[3], "long row")
        assert [n for _, n, _ in got] == [n for _, n, _ in want]
    finally:
        release(w)


@pytest.mark.parametrize("case", CW.CASES, ids=IDS)
def test_error_correction(case):
    w, seqs, want = CW.errors_case(case)
    mincov, max_indel = case[4:]
    print("errors %s mincov=%g max_indel=%d: %s" % (CW.case_id(case), mincov, max_indel, sorted(EC.outcome_counts(want).items())))
    g = w.device()                                                 # (compares dbgbf and cbf with the oracle's, byte for byte)
    try:
        EC.compare(g, seqs, want, CW.T, mincov, max_indel, "all")
        some, thr, want2 = CW.errors_second_call(case)
        EC.compare(g, some, want2, thr, mincov, max_indel, "lookahead 3", lookahead=3, pid=0.97)
    finally:
        release(w)


@pytest.mark.parametrize("long_case", CW.LONG_GAP_CASES, ids=["k%d" % c[0] for c in CW.LONG_GAP_CASES])
def test_long_gaps_next_to_short_ones(long_case, monkeypatch):
    w, long_q, seqs, want, at = CW.long_gap_case(long_case)
    max_indel = long_case[3]
    for key, i in at.items():                                      # the gap the query was made for, with its row past LDS
        assert [(r["kind"], r["outcome"]) for r in want[i][2] if r["run"] + w.k - 1 > CW.LEV_LDS] == [key]
    g = w.device()
    try:
        whole = EC.compare(g, seqs, want, CW.T, 1.0, max_indel, "long gaps")
        monkeypatch.setenv("RB_QUERY_PIECE", "1")                  # a sequence to a piece: the long gap alone in its chunk, its row at offset 0
        seq, off = _pack(seqs)
        pieces = g.correctErrorsFlat(seq, off, CW.T, EC.LOOKAHEAD, max_indel, EC.PID, 1.0, gaps=True)
        assert EC.same(pieces, whole)
    finally:
        release(w)
