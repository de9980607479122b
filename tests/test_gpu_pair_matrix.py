"""The fragment-building calls beyond k = 25 and two hash functions: rb_graph_overlap_pairs (csrc/rb_overlap.hip), rb_graph_extend_se and
rb_graph_extend_pe (csrc/rb_extend.hip over csrc/rb_extend_step.hpp) and rb_graph_join_pairs (csrc/rb_join.hip, which calls the same step at
forks) on the worlds of tests/pair_worlds.py: k = 16 ... 256 on both sides of 64, 128 and 192, and 255 beside 256; stranded and canonical; hash
counts (1, 1, 1), (3, 4, 3), (2, 2, 3), (3, 1, 2) and (2, 2, 2).  What only runs there: the second and later rounds of the overlap's spanning
loop and of its singleton search (a first bad spanning k-mer at index 64 and at the last index, a singleton that is the 65th window asked),
isRepeat's signed-byte counter at 141 and 142 shared letters, ex_one's packing of the last k-mer up to lane 63 and into a partial byte, the
step's rotations by 0, 63, 64, 65 and more than 128, pair counting and next_equals with a seed longer than the walk rows, join's text and code
rows sized from k, and the generic lookup loops under k_join and the PE instantiation of k_extend.  Every expected value is the restatements'
(tests/test_overlap_rules.py, tests/test_extend_step_rules.py, tests/test_extend_pe_rules.py, tests/test_join_rules.py) on the CPU oracle's
filters; tests/test_pair_reach.py proves on the CPU that the worlds ask something.  The device graph is filled through the product's insert
path and its filters are the oracle's byte for byte before anything is compared; every comparison is exact — record fields as integers, text
and bases as bytes, counts, scores and thresholds as bits, zeros behind the text — through compare() / check() of the calls' own device test
files; the filters' folds are what they were afterwards."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rnabloom import _native as N

import pair_worlds as PW
import test_gpu_extend_pe as GP
import test_gpu_extend_step as EX
import test_gpu_join as GJ
import test_gpu_overlap as OV
import test_overlap_rules as OR

IDS = [PW.case_id(c) for c in PW.CASES]
BIG = [c for c in PW.CASES if c.k >= 128]
OVERLAP_MINCOV2_CASE = next(c for c in BIG if c.k == 192 and c.hashes[0] != 2)          # (k >= 144: the pairs at isRepeat's wrap are in it)
JOIN_PIECE_CASE = next(c for c in BIG if c.k == 129 and c.hashes[2] != 2)
OV_FILTERS = (N.DBGBF, N.CBF, N.RPKBF)


def folds(g, filters):
    return [g.fold(f) for f in filters]


def device_of(mod, w):
    """the device twin through the call's own device test file: filled by the product's insert path, every filter equal to the oracle's"""
    g = mod.device(w)
    assert (g.exportFilter(N.DBGBF) == w.og.dbgbf_bytes()).all(), "dbgbf"
    assert (g.exportFilter(N.CBF) == w.og.cbf_bytes()).all(), "cbf"
    assert (g.exportFilter(N.RPKBF) == w.og.rpkbf_bytes()).all(), "rpkbf"
    return g


def release(mod, w):
    g = mod.DEVICES.pop(id(w), None)
    if g is not None:
        g.destroy()


def overlap_device(w):
    g = w.device()                                                 # (compares dbgbf and cbf)
    assert (g.exportFilter(N.DBGBF) == w.og.dbgbf_bytes()).all() and (g.exportFilter(N.CBF) == w.og.cbf_bytes()).all()
    assert (g.exportFilter(N.RPKBF) == w.og.rpkbf_bytes()).all(), "rpkbf"
    return g


def overlap_release(w):
    if w.gg is not None:
        w.gg.destroy(); w.gg = None


@pytest.mark.parametrize("case", PW.CASES, ids=IDS)
def test_overlap(case):
    mo, mincov = case.overlap
    w = PW.overlap_case(case)
    want = w.want(mincov)
    print("overlap %s: %d pairs, (outcome, why, swapped) %s" % (PW.case_id(case), len(want), PW.outcome_counts(rec[:3] for rec, _ in want)))
    try:
        g = overlap_device(w)
        before = folds(g, OV_FILTERS)
        OV.compare(w.pairs, want, OV.flat(g, w.pairs, mincov, mo), PW.case_id(case))
        assert folds(g, OV_FILTERS) == before
    finally:
        overlap_release(w)



def test_overlap_under_min_kmer_cov_2():
    """the singletons' own k-mers are below it, the k-mers held by a second read are not: other first bad indices, other answers"""
    case = OVERLAP_MINCOV2_CASE
    w = PW.overlap_case(case)
    mo = case.overlap[0]
    want1 = w.want(1.0)
    want2 = [OR.expected(l, r, w.k, mo, 2.0, w.o) for l, r in w.pairs]
    assert sum(a != b for a, b in zip(want1, want2)) >= 1          # (few records change: a pair below the floor is rescued or refused as before)
    try:
        g = overlap_device(w)
        before = folds(g, OV_FILTERS)
        OV.compare(w.pairs, want2, OV.flat(g, w.pairs, 2.0, mo), (PW.case_id(case), "mincov 2"))
        assert folds(g, OV_FILTERS) == before
    finally:
        overlap_release(w)


@pytest.mark.parametrize("case", PW.CASES, ids=IDS)
def test_extend_se_both_directions(case):
    w = PW.step_case(case)
    print("extend_se %s: %d queries, (outcome, why) %s" % (PW.case_id(case), len(w.queries), PW.outcome_counts((st.outcome, st.why) for st in w.want())))
    try:
        g = device_of(EX, w)
        before = folds(g, EX.FILTERS)
        EX.compare(w, g, PW.case_id(case))
        assert folds(g, EX.FILTERS) == before
    finally:
        release(EX, w)


@pytest.mark.parametrize("case", PW.CASES, ids=IDS)
def test_extend_pe_both_directions(case):
    w = PW.pe_case(case)
    print("extend_pe %s: %d queries, (outcome, why) %s" % (PW.case_id(case), len(w.queries), PW.outcome_counts((st.outcome, st.why) for st in w.want())))
    try:
        g = device_of(GP, w)                                       # (test_gpu_extend_pe.fill: addReads with pairs, then the fragments)
        assert (g.exportFilter(N.FPKBF) == w.og.fpkbf_bytes()).all(), "fpkbf"
        before = folds(g, GP.FILTERS)
        GP.compare(w, g, PW.case_id(case))
        assert folds(g, GP.FILTERS) == before
    finally:
        release(GP, w)


@pytest.mark.parametrize("case", PW.CASES, ids=IDS)
def test_join(case):
    w = PW.join_case(case)
    want = w.want()
    print("join %s: %d pairs, (outcome, why) %s" % (PW.case_id(case), len(want), PW.outcome_counts((r.outcome, r.why) for r in want)))
    try:
        g = device_of(GJ, w)
        before = folds(g, GJ.FILTERS)
        GJ.compare(w, g, PW.case_id(case))
        assert folds(g, GJ.FILTERS) == before
    finally:
        release(GJ, w)


def test_join_a_pair_a_piece(monkeypatch):
    """RB_QUERY_PIECE = 1: every pair alone in its piece, its rows at offset 0 — against the whole call, byte for byte"""
    case = JOIN_PIECE_CASE
    w = PW.join_case(case)
    pairs = w.pairs[:200] + w.pairs[-8:]
    try:
        g = device_of(GJ, w)
        whole = GJ.run(g, pairs, w.BOUND, w.GRAD, w.TIP, w.MIN_COV)
        GJ.check(whole, pairs, w.want()[:200] + w.want()[-8:], w.BOUND, w.d, w.k, (PW.case_id(case), "whole"))
        monkeypatch.setenv("RB_QUERY_PIECE", "1")
        pieces = GJ.run(g, pairs, w.BOUND, w.GRAD, w.TIP, w.MIN_COV)
        n = int(whole[1][-1])
        assert pieces[1].tolist() == whole[1].tolist() and pieces[0][:n].tobytes() == whole[0][:n].tobytes()
        assert pieces[2].tobytes() == whole[2].tobytes()
    finally:
        release(GJ, w)
