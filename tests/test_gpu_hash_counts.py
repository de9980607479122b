"""The five read-only graph calls — rb_graph_correct_mismatches, rb_graph_correct_errors, rb_graph_overlap_pairs, rb_graph_extend_se (both
directions) and rb_graph_paired_kmer_segments — on graphs whose filters have 1, 3 and mixed (2, 3, 1) hash functions: every other world of
these calls has (2, 2, 2), which the kernels serve by their "issue all probes first" fast paths, so this file is what runs the generic loops of
csrc/rb_lookup.hpp (count_code, count_codes4, pair_hit behind bits_lookup).  Worlds and expected results come from
tests/test_hash_counts_reach.py, which shows on the oracle alone that they are not vacuous; each call is compared by its own test file's compare
function against its restatement on the oracle — every record field, bytes, counts and scores as bits — after the device's three filters have
been found equal to the oracle's byte for byte."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rnabloom import _native as N
import test_gpu_error_correction as EC
import test_gpu_extend_step as EX
import test_gpu_mismatch_correction as MM
import test_gpu_overlap as OV
import test_gpu_paired_segments as PS
import test_hash_counts_reach as W


def assert_same_filters(g, og):
    assert (g.exportFilter(N.DBGBF) == og.dbgbf_bytes()).all(), "dbgbf"
    assert (g.exportFilter(N.CBF) == og.cbf_bytes()).all(), "cbf"
    assert (g.exportFilter(N.RPKBF) == og.rpkbf_bytes()).all(), "rpkbf"


def release(w):
    w.gg.destroy()
    w.gg = None


@pytest.mark.parametrize("hashes", W.HASHES)
def test_correct_mismatches(hashes):
    w, seqs, want = W.mismatch_case(hashes)
    assert_same_filters(w.device(), w.og)
    try:
        MM.check(w, seqs, MM.World.T, W.MINCOV, hashes)     # (works the restatement out again: a tenth of a second)
    finally:
        release(w)


@pytest.mark.parametrize("hashes", W.HASHES)
def test_correct_errors(hashes):
    w, seqs, want = W.errors_case(hashes)
    g = w.device()
    assert_same_filters(g, w.og)
    try:
        EC.compare(g, seqs, want, EC.T, W.MINCOV, W.MAX_INDEL, hashes)
    finally:
        release(w)


@pytest.mark.parametrize("hashes", W.HASHES)
def test_overlap_pairs(hashes):
    w, pairs, want = W.overlap_case(hashes)
    g = w.device()
    assert_same_filters(g, w.og)
    try:
        OV.compare(pairs, want, OV.flat(g, pairs, W.MINCOV), hashes)
    finally:
        release(w)


@pytest.mark.parametrize("hashes", W.HASHES)
def test_extend_se_both_directions(hashes):
    w, want = W.extend_case(hashes)
    g = EX.device(w)                                        # (asserts the three filters equal to the oracle's)
    try:
        assert_same_filters(g, w.og)
        EX.compare(w, g, hashes)
    finally:
        EX.DEVICES.pop(id(w)).destroy()


@pytest.mark.parametrize("hashes", W.HASHES)
def test_paired_kmer_segments(hashes):
    w, seqs, want, sups = W.segments_case(hashes, True)     # (the constructor asserts both pair filters equal to the oracle's)
    try:
        assert_same_filters(w.gg, w.og)
        assert (w.gg.exportFilter(N.FPKBF) == w.og.fpkbf_bytes()).all()
        for (which, npr), segs in want.items():
            got, so, ko, sup = PS.device(w, which, seqs, npr)
            assert got == segs, (hashes, which, npr)
            assert (ko == np.concatenate([[0], np.cumsum([s.size for s in sups[which]])])).all()
            assert (sup.astype(bool) == np.concatenate(sups[which])).all(), (hashes, which)
    finally:
        w.gg.destroy()
