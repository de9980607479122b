"""A condition on the inputs of tests/test_gpu_long_correction.py, checked without a GPU: over the worlds of tests/long_worlds.py the restatement of
tests/test_long_correction_rules.py alone drives every counter of rb_long_rec to at least 1, produces every status, trims a sequence to nothing
and makes one outgrow its own length (the overflow flag of a call that gives no slack) — so the comparison on the GPU cannot pass by never
asking the question.  The answers are computed once per case (long_worlds.want) and shared with the GPU test."""
import pytest

import long_worlds as LW
from test_long_correction_rules import CHANGED, CTRS, FIELDS, NO_KMER, NULL, TRIMMED_TO_NOTHING, UNCHANGED

F = {f: i for i, f in enumerate(FIELDS)}


def totals():
    ctr, status, flags, grown, passes, trims = dict.fromkeys(CTRS, 0), set(), 0, 0, set(), set()
    for i in range(len(LW.CASES)):
        w, want = LW.want(i)
        for s, (text, rec) in zip(w.queries, want):
            for c in CTRS:
                ctr[c] += rec[F[c]]
            status.add(rec[F["status"]])
            flags |= rec[F["flags"]]
            grown += rec[F["out_len"]] > len(s)
            passes.add(rec[F["passes"]])
            trims.add("none" if rec[F["trim_begin"]] < 0 else "nothing" if rec[F["flags"]] & TRIMMED_TO_NOTHING else "cut")
    return ctr, status, flags, grown, passes, trims


def test_every_counter_status_and_flag_is_reached():
    ctr, status, flags, grown, passes, trims = totals()
    print("counters:", ctr, "statuses:", sorted(status), "grown:", grown, "passes:", sorted(passes), "trims:", sorted(trims))
    assert all(v >= 1 for v in ctr.values()), ctr
    assert status == {NULL, UNCHANGED, CHANGED, NO_KMER}
    assert flags & TRIMMED_TO_NOTHING and grown >= 1
    assert {0, 1, 2} <= passes                                  # no pass, one, and a second pass that corrected what the first exposed
    assert trims == {"none", "cut", "nothing"}


@pytest.mark.parametrize("i", range(len(LW.CASES)), ids=[LW.case_id(c) for c in LW.CASES])
def test_every_case_asks_something(i):
    w, want = LW.want(i)
    c = LW.CASES[i]
    events = sum(sum(rec[F[x]] for x in CTRS) for _, rec in want)
    changed = sum(rec[F["status"]] == CHANGED for _, rec in want)
    print(LW.case_id(c), "events", events, "changed", changed, "of", len(want))
    assert len(want) >= (220 if c["big"] else 300)
    assert changed >= 10 and (events >= 100 or c["maxItr"] == 0)
