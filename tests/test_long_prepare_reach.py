"""A condition on the inputs of tests/test_gpu_long_prepare.py, checked without a GPU: over the worlds of tests/long_prepare_worlds.py the
restatement of tests/test_long_prepare_rules.py alone produces every status and every flag bit, all three complexity routes, a cut that fires
with a run from window 0, with a run open at the end and with several segments, a cut that does NOT fire with one to four low windows, chains
of three and more seed searches, a join that only percentA allows, every branch of the five-way rule and the clearing of hasPolyA by several
segments — so the comparison on the GPU cannot pass by never asking the question.  The answers are computed once per case
(long_prepare_worlds.want) and shared with the GPU test."""
import pytest

import long_prepare_worlds as W
from long_prepare_worlds import F
from test_long_prepare_rules import (CUT_FIRED, HAS_POLYA, HEAD_FOUND, LOW_COMPLEXITY, MAPPED_TWICE, REVCOMP, ROUTE_WHOLE, ROUTE_WINDOWED,
                                     ROUTE_WINDOWS, SEGMENTS, SHORT, TAIL_FOUND, Finder, prepare)


def everything():
    for i, c in enumerate(W.CASES):
        reads, got, bridged = W.want(i)
        for r, (rec, segs, seq) in zip(reads, got):
            yield c["P"], r, rec, segs, seq


def test_every_status_flag_and_route_is_reached():
    status, flags = set(), {}
    for P, r, rec, segs, seq in everything():
        status.add(rec[F["status"]])
        for b in range(9):
            if rec[F["flags"]] >> b & 1:
                flags[1 << b] = flags.get(1 << b, 0) + 1
    print("statuses", sorted(status), "flags", flags)
    assert status == {SHORT, LOW_COMPLEXITY, SEGMENTS}
    for b in (REVCOMP, HAS_POLYA, TAIL_FOUND, HEAD_FOUND, CUT_FIRED, ROUTE_WINDOWS, ROUTE_WINDOWED, ROUTE_WHOLE, MAPPED_TWICE):
        assert flags.get(b, 0) >= 3, (b, flags)


def test_the_cut_is_reached_every_way():
    from0 = open_end = several = none_left = 0
    not_fired = set()
    for P, r, rec, segs, seq in everything():
        fl = rec[F["flags"]]
        if not fl & ROUTE_WINDOWS:
            continue
        if fl & CUT_FIRED:
            from0 += bool(segs) and segs[0][0] == 0 and segs[0][1] < len(seq)
            open_end += bool(segs) and segs[-1][1] == len(seq) and segs[-1][0] > 0
            several += len(segs) >= 2
            none_left += not segs
            assert len(segs) <= max(1, (len(r) // P["lc_window"] + 1) // 2)             # the room the call asks for is enough
        else:
            not_fired.add(rec[F["n_low"]])
    print("from 0:", from0, "open at the end:", open_end, "several:", several, "nothing left:", none_left, "low windows without a cut:", sorted(not_fired))
    assert from0 >= 3 and open_end >= 3 and several >= 3 and none_left >= 1
    assert {0, 1, 2, 3, 4} <= not_fired


def test_the_chains_are_reached():
    tails = max(rec[F["tail_searches"]] for P, r, rec, segs, seq in everything())
    heads = max(rec[F["head_searches"]] for P, r, rec, segs, seq in everything())
    long_chains = sum(rec[F["tail_searches"]] >= 3 or rec[F["head_searches"]] >= 3 for P, r, rec, segs, seq in everything())
    bridged = sum(W.want(i)[2] for i in range(len(W.CASES)))
    print("longest chains:", tails, heads, "chains of three and more:", long_chains, "joins by percentA / percentT:", bridged)
    assert tails >= 3 and heads >= 3 and long_chains >= 10 and bridged >= 1
    # a tail whose start sits on a letter that is no A, and one that reaches letter 0
    on_other = sum(rec[F["tail_start"]] > 0 and not (P["reverse_complement"] or r[rec[F["tail_start"]]] in b"Aa") for P, r, rec, segs, seq in everything())
    at_zero = sum(rec[F["tail_start"]] == 0 for P, r, rec, segs, seq in everything())
    assert on_other >= 1 and at_zero >= 1


def test_every_branch_of_the_five_way_rule_is_reached():
    seen = set()
    for P, r, rec, segs, seq in everything():
        if not P["polya"]:
            seen.add("off")
            continue
        fl, n = rec[F["flags"]], len(r)
        tail, head = bool(fl & TAIL_FOUND), bool(fl & HEAD_FOUND)
        if rec[F["status"]] == SHORT:
            continue
        if P["strand_specific"]:
            seen.add(("stranded", tail, tail and rec[F["tail_end"]] < n))
        elif tail and not head:
            seen.add(("tail", rec[F["tail_end"]] < n))
        elif head and not tail:
            seen.add(("head", rec[F["head_start"]] > 0))
        elif head and tail:
            seen.add(("both", rec[F["head_end"]] < rec[F["tail_start"]]))
        else:
            seen.add("none")
    want = {"off", "none", ("stranded", False, False), ("stranded", True, False), ("stranded", True, True), ("tail", False), ("tail", True),
            ("head", False), ("head", True), ("both", False), ("both", True)}
    assert want <= seen, want - seen


def test_several_segments_clear_has_polya():
    cleared = 0
    for P, r, rec, segs, seq in everything():
        if len(segs) > 1:
            assert not rec[F["flags"]] & HAS_POLYA
            one = prepare(r, dict(P, lc_min_length=10 ** 9))[0]              # the same read with a cut that cannot fire
            cleared += bool(one[F["flags"]] & HAS_POLYA)
    assert cleared >= 3


@pytest.mark.parametrize("i", range(len(W.CASES)), ids=[W.case_id(c) for c in W.CASES])
def test_every_case_asks_something(i):
    reads, got, _ = W.want(i)
    big = sum(len(r) for r in reads if len(r) >= 70_000)
    assert 60 <= len(reads) <= 120 and (big == 370_001) == W.CASES[i]["big"]
    # (with windows of 37 and no finder three combinations are all there is: too short, the windows, the whole read)
    assert len({rec[F["flags"]] for rec, _, _ in got}) >= 3 and sum(len(s) for _, s, _ in got) >= 30
