"""The inputs of tests/test_gpu_pair_correction.py ask something — conditions on the worlds of tests/pair_correction_worlds.py, met by the
restatement (tests/test_pair_correction_rules.py) on the CPU oracle's filters alone.  Per case: at least 20 pairs with a changing round, at
least 10 that enter a round after a change, a mate whose length changed, mates of unequal length, and every end but END_LOST_KMERS over the
calls the GPU file makes for that case (pair_correction_worlds.gpu_calls: four rounds, one, none) — END_ALL comes from the call with one
round, where every changing pair runs out of rounds, and from the call with none; with four rounds it needs a pair that changes in all of
them, which one refillable bubble of the world at k = 25, canonical, does.  Over all cases: a pair with two or more changing rounds.  Only the
planted mates with fewer than k letters are not judged.  Like tests/test_correction_reach.py this runs on a built tree (the restatement takes
SeqUtils.isLowComplexityShort from the package)."""
import collections

import pytest

import pair_correction_worlds as PW
from test_pair_correction_rules import (CORRECTED_PAIR, END_ALL, END_LOST_KMERS, END_LOW, END_NO_CHANGE, END_NO_KMER, NOT_JUDGED, UNCHANGED)


def changing(rec):
    return rec["left_changed"] + rec["right_changed"]


@pytest.mark.parametrize("case", PW.CASES, ids=PW.case_id)
def test_the_pairs_reach_every_outcome(case):
    w, pairs, want = PW.pair_case(case)
    calls = PW.gpu_calls(case)
    assert set(calls) == {PW.PARAMS["iterations"]} | set(PW.ROUND_COUNTS) and 1 in calls and 0 in calls
    one = calls[1]
    recs = [r for r, _, _ in want]
    ends = collections.Counter(r["end"] for r in recs)
    print(PW.case_id(case), len(pairs), "pairs; ends", sorted(ends.items()), "; one round:", sorted(collections.Counter(r["end"] for r, _, _ in one).items()))
    assert sum(1 for r in recs if changing(r) > 0) >= 20
    # a round entered after a change: a second run of the helper, or a threshold search that ended the pair (its thr_last is that round's)
    assert sum(1 for r in recs if changing(r) > 0 and (r["rounds_run"] >= 2 or r["end"] == END_LOW)) >= 10
    assert sum(1 for r in recs if r["rounds_run"] >= 2) >= 10
    assert any(len(lo) != len(l) or len(ro) != len(r_) for (_, lo, ro), (l, r_) in zip(want, pairs))
    assert any(len(l) != len(r_) and len(l) >= w.k and len(r_) >= w.k for l, r_ in pairs)
    assert {END_NO_CHANGE, END_LOW, END_NO_KMER} <= set(ends) and END_LOST_KMERS not in ends
    # END_ALL where a round was the last one allowed (round + 1 >= rounds), in a call the GPU file makes for THIS case
    assert any(r["end"] == END_ALL and r["rounds_run"] == it and it > 0 for it, want_it in calls.items() for r, _, _ in want_it)
    assert sum(1 for r, _, _ in one if r["end"] == END_ALL and r["rounds_run"] == 1) >= 20
    assert all(r["end"] == END_ALL and r["rounds_run"] == 0 for r, _, _ in calls[0])
    assert {r["status"] for r in recs} == {UNCHANGED, CORRECTED_PAIR, NOT_JUDGED}
    for (l, r_), rec in zip(pairs, recs):
        assert (rec["status"] == NOT_JUDGED) == (len(l) < w.k or len(r_) < w.k) == (rec["end"] == END_NO_KMER)


def test_a_pair_changes_in_two_or_more_rounds():
    best = 0
    for case in PW.CASES:
        for rec, _, _ in PW.pair_case(case)[2]:
            best = max(best, rec["left_changed"], rec["right_changed"])
    print("most changing rounds of one mate:", best)
    assert best >= 2
    assert any(r["end"] == END_ALL and r["rounds_run"] == PW.PARAMS["iterations"] for r, _, _ in PW.pair_case(PW.CASES[0])[2])


@pytest.mark.parametrize("case", PW.CASES[:2], ids=PW.case_id)
def test_the_single_reads_reach_every_outcome(case):
    w, seqs, want = PW.single_case(case)
    ends = collections.Counter(r["end"] for r, _ in want)
    print(PW.case_id(case), len(seqs), "reads; ends", sorted(ends.items()))
    assert set(ends) == {END_ALL, END_NO_CHANGE, END_LOW, END_NO_KMER}
    assert sum(1 for r, _ in want if r["status"] == CORRECTED_PAIR) >= 60 and all(r["status"] != NOT_JUDGED for r, _ in want)
    assert any(len(t) != len(s) for (_, t), s in zip(want, seqs))
