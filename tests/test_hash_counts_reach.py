"""The worlds of tests/test_gpu_hash_counts.py — the five read-only graph calls on graphs whose filters do not all have two hash functions — and,
on the CPU oracle alone, the proof that those worlds ask something: per call and per combination of hash counts the restatement's results hold
at least one replacement, one corrected gap, one merged and one refused pair, the outcomes NONE, SINGLE and FIRST in each direction, one cut.
The worlds are the smallest the constructors of the five device test files give (k = 25, canonical, a handful of transcripts, a few hundred
reads, d = 30 for the extension); every restatement is computed once per combination and shared with the device test."""
import functools

import numpy as np
import pytest

from rnabloom import _native as N
import test_error_correction_rules as ER
import test_extend_step_rules as XR
import test_gpu_error_correction as EC
import test_gpu_mismatch_correction as MM
import test_gpu_overlap as OV
import test_gpu_paired_segments as PS
import test_overlap_rules as OR

# (dbgbf, cbf, pair filters): none of them the (2, 2, 2) of every other world; the last sends a filter WITH two functions down the generic path
# because the other has three
HASHES = [(1, 1, 1), (3, 3, 3), (2, 3, 1)]
K = 25
MINCOV = 1.0
MAX_INDEL = 1
NPR = (1, 2)                         # numPairsRequired


def seed_of(hashes, call):
    return 7000 + 100 * call + 16 * hashes[0] + 4 * hashes[1] + hashes[2]


@functools.lru_cache(maxsize=None)
def mismatch_case(hashes):
    """(world, sequences, the restatement's (text, n_fixed, counts) of each)"""
    w = MM.World(K, False, seed_of(hashes, 1), n_tx=6, n_reads=800, hashes=hashes)
    seqs = w.planted[:90] + w.rev_only + w.reads[300:320]
    return w, seqs, w.o.expected(seqs, MM.World.T, MINCOV)


@functools.lru_cache(maxsize=None)
def errors_case(hashes):
    """(world, sequences, the restatement's (text, flags, gap records) of each)"""
    w = EC.World(K, False, seed_of(hashes, 2), n_tx=5, n_reads=650, hashes=hashes)
    seqs = w.all_queries()
    return w, seqs, w.o.expected_errors(seqs, EC.T, MINCOV, MAX_INDEL)


@functools.lru_cache(maxsize=None)
def overlap_case(hashes):
    """(world, its pairs, the restatement's (record, text) of each)"""
    w = OV.World(K, False, seed_of(hashes, 3), n_tx=8, n_single=16, hashes=hashes)
    return w, w.pairs, w.want(MINCOV)


@functools.lru_cache(maxsize=None)
def extend_case(hashes):
    """(world, the restatement's step of each of its queries, both directions)"""
    w = XR.World(K, False, seed_of(hashes, 4), d=30, n_iso=3, hashes=hashes)
    return w, w.want()


def segments_case(hashes, device):
    """(world, sequences, {(filter, numPairsRequired): the restatement's segments of each sequence}, {filter: support rows}); with device True
    the world's constructor builds the device graph beside the oracle and compares their pair filters"""
    w = PS.World(K, False, hashes[2], 20, 60, seed_of(hashes, 5), hashes=hashes, device=device)
    sets = PS.query_sets(w, np.random.default_rng(seed_of(hashes, 6)))
    seqs = sets["chimeras"] + sets["reads"][:60] + sets["iupac"][:30] + sets["short"]
    sups = {which: w.support(which, seqs) for which in (N.RPKBF, N.FPKBF)}
    want = {(which, npr): PS.expected(sups[which], d, npr) for which, d in ((N.RPKBF, w.read_d), (N.FPKBF, w.frag_d)) for npr in NPR}
    return w, seqs, want, sups


@functools.lru_cache(maxsize=None)
def segments_case_on_the_oracle(hashes):
    return segments_case(hashes, False)


@pytest.mark.parametrize("hashes", HASHES)
def test_mismatch_world_has_replacements(hashes):
    w, seqs, want = mismatch_case(hashes)
    assert (w.og.h, w.og.pk_h) == (max(hashes[:2]), hashes[2])
    assert sum(n for _, n, _ in want) >= 1 and any(s != q for (s, _, _), q in zip(want, seqs))
    assert any(n == 0 for _, n, _ in want)                                          # ... and sequences that stay as they are


@pytest.mark.parametrize("hashes", HASHES)
def test_error_world_has_corrected_gaps(hashes):
    w, seqs, want = errors_case(hashes)
    assert sum(bool(f & ER.GAP) for _, f, _ in want) >= 1
    outcomes = {r["outcome"] for _, _, recs in want for r in recs}
    assert ER.REPLACED in outcomes and ER.KEPT in outcomes, outcomes


@pytest.mark.parametrize("hashes", HASHES)
def test_overlap_world_has_merged_and_refused_pairs(hashes):
    w, pairs, want = overlap_case(hashes)
    outcomes = [rec[0] for rec, _ in want]
    assert outcomes.count(OR.MERGED) >= 1 and outcomes.count(OR.NONE) >= 1, outcomes
    assert outcomes.count(OR.SPANNED) >= 1                                         # the outcome that asks the graph


@pytest.mark.parametrize("hashes", HASHES)
def test_extend_world_reaches_none_single_and_first(hashes):
    w, want = extend_case(hashes)
    for direction in (0, 1):
        outcomes = {st.outcome for st, q in zip(want, w.queries) if q[2] == direction}
        assert {XR.NONE, XR.SINGLE, XR.FIRST} <= outcomes, (direction, outcomes)


@pytest.mark.parametrize("hashes", HASHES)
def test_segment_world_has_cuts(hashes):
    w, seqs, want, sups = segments_case_on_the_oracle(hashes)
    for key, segs in want.items():
        assert sum(len(s) >= 2 for s in segs) >= 1, key
        assert sum(len(s) == 1 for s in segs) >= 1, key
