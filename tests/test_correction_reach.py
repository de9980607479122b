"""On the CPU oracle alone: the proof that the worlds of tests/correction_worlds.py ask something.  tests/test_gpu_correction_matrix.py compares
rb_graph_correct_mismatches and rb_graph_correct_errors with the restatements on these worlds; a world whose planted substitutions are not
replaced, whose gaps are all kept or whose long gaps fall short of the Levenshtein row's LDS limit would let a wrong kernel pass.  Every condition
here is hard: a world that stops meeting one is changed, not the assertion.  Each test prints the counts it rests on (-s shows them)."""
import pytest

import correction_worlds as CW
from test_error_correction_rules import (GAP, KEPT, LEFT_EDGE, MISMATCH, PATH, REPLACED, RIGHT_EDGE, SNV, TRIMMED)
from test_gpu_error_correction import ALL_OUTCOMES, outcome_counts

IDS = [CW.case_id(c) for c in CW.CASES]
ACTING = ((LEFT_EDGE, REPLACED), (LEFT_EDGE, TRIMMED), (RIGHT_EDGE, REPLACED), (RIGHT_EDGE, TRIMMED), (SNV, REPLACED), (PATH, REPLACED))


def test_matrix_spreads_the_axes():
    assert len(set(c[:2] for c in CW.CASES)) == len(CW.CASES) == 2 * len(CW.KS)
    for k in CW.KS:
        assert {c[1] for c in CW.CASES if c[0] == k} == {False, True}                       # every k stranded and canonical
    for h in CW.HASHES:
        mine = [c for c in CW.CASES if c[2] == h + (2,)]
        assert len(mine) >= 2 and any(c[0] >= 64 for c in mine) and {c[1] for c in mine} == {False, True}, h
    big = [c for c in CW.CASES if c[0] >= 64]
    assert {c[5] for c in big} == {1, 3} and {c[4] for c in big} == {1.0, 2.0} and {c[3] for c in big} == {0.0, 1.0, 2.0}
    for stranded in (False, True):
        assert {c[4:] for c in CW.CASES if c[1] == stranded} == {(1.0, 1), (1.0, 3), (2.0, 1), (2.0, 3)}
    # a lane of k_mismatch owns a second window from k = 65 on, a third from 129, a fourth from 193; a lane of k_resolve_snv (k + 2 windows) a
    # second from k = 63 on and a third from 127
    assert {65, 129, 193, 256} <= set(CW.KS) and {62, 63, 64, 127, 128, 192} <= set(CW.KS)
    assert CW.LONG_ROW_CASE[0] >= 65
    assert {c[1] for c in CW.LONG_GAP_CASES} == {False, True} and any(c[0] > 64 for c in CW.LONG_GAP_CASES)


@pytest.mark.parametrize("case", CW.CASES, ids=IDS)
def test_planted_substitutions_are_replaced(case):
    w, sets, (changed, reverse_only) = CW.mismatch_case(case)               # assert_not_vacuous: half of them change, one by the reverse scan alone
    n = len(w.planted) + len(w.rev_only)
    print("mismatch %s mincov=%g read_len=%d reads=%d: %d of %d planted sequences change, %d by the reverse scan only" % (
        CW.case_id(case), case[3], w.read_len, len(w.reads), changed, n, reverse_only))
    assert n == CW.MM_PLANTED + CW.MM_REV and changed * 2 >= n and reverse_only >= 1
    assert w.read_len == max(250, 5 * w.k + 60) and all(len(s) == w.read_len for s in w.planted)


@pytest.mark.parametrize("case", CW.CASES, ids=IDS)
def test_gaps_of_every_acting_outcome(case):
    w, seqs, want = CW.errors_case(case)
    cnt = outcome_counts(want)
    gap, mismatch = sum(bool(f & GAP) for _, f, _ in want), sum(bool(f & MISMATCH) for _, f, _ in want)
    print("errors %s mincov=%g max_indel=%d read_len=%d reads=%d: %s; %d of %d sequences flagged GAP, %d MISMATCH" % (
        CW.case_id(case), case[4], case[5], w.read_len, len(w.reads), sorted(cnt.items()), gap, len(want), mismatch))
    for key in ACTING:
        assert cnt.get(key, 0) >= 2, (key, cnt)
    assert gap >= 10 and mismatch >= 5
    _, _, want2 = CW.errors_second_call(case)
    assert sum(len(recs) for _, _, recs in want2) >= 10


def test_every_kind_and_outcome_occurs_over_the_matrix():
    total = {}
    for case in CW.CASES:
        for key, v in outcome_counts(CW.errors_case(case)[2]).items():
            total[key] = total.get(key, 0) + v
    print("kind x outcome over the matrix:", sorted(total.items()))
    assert set(total) == ALL_OUTCOMES, sorted(ALL_OUTCOMES - set(total))


@pytest.mark.parametrize("long_case", CW.LONG_GAP_CASES, ids=["k%d" % c[0] for c in CW.LONG_GAP_CASES])
def test_long_gaps_of_every_kind_replaced_and_kept(long_case):
    """a gap of `run` bad k-mers is compared over run + k - 1 letters: past LEV_LDS columns the row is in device scratch"""
    w, long_q, seqs, want, at = CW.long_gap_case(long_case)
    assert set(long_q) == {(kind, oc) for kind in (PATH, LEFT_EDGE, RIGHT_EDGE) for oc in (REPLACED, KEPT)}
    for (kind, outcome), i in at.items():
        assert seqs[i] == long_q[(kind, outcome)]
        recs = [r for r in want[i][2] if r["run"] + w.k - 1 > CW.LEV_LDS]
        print("long gaps k=%d: aimed at %s, records %s" % (w.k, (kind, outcome), [(r["kind"], r["outcome"], r["first"], r["run"], r["repl_len"]) for r in want[i][2]]))
        assert [(r["kind"], r["outcome"]) for r in recs] == [(kind, outcome)], (kind, outcome, want[i][2])
        assert recs[0]["run"] >= 5                                         # >= lookahead: the host gives such a gap a row in scratch
    # ... next to gaps whose rows fit LDS, in the same call
    short = [r for i, (_, _, recs) in enumerate(want) if i not in at.values() for r in recs]
    assert sum(r["kind"] != SNV and 5 <= r["run"] and r["run"] + w.k - 1 <= CW.LEV_LDS and r["outcome"] == REPLACED for r in short) >= 5


def test_long_row_past_a_slot_boundary():
    """more than MM_LDS_ROW windows (k_mismatch<false>: the code row in device memory) at a k where a lane owns three windows"""
    w, seqs, want = CW.long_row_case()
    nk = len(seqs[0]) - w.k + 1
    print("long row k=%d: %d windows, %d replacements (and %d in the short sequence next to it)" % (w.k, nk, want[0][1], want[1][1]))
    assert w.k >= 65 and nk > CW.MM_LDS_ROW and want[0][1] >= 2
