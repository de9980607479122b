"""On the CPU oracle alone: the proof that the worlds of tests/traversal_worlds.py ask something.  tests/test_gpu_traversal_matrix.py compares the
traversal kernels with the oracle's restatements on these worlds; a world whose walks all end at once, whose filters make no false neighbour or
whose naive extensions never meet a terminator would let a wrong kernel pass.  Every condition here is hard: a world that stops meeting one is
changed, not the assertion."""
import numpy as np
import pytest

import traversal_worlds as TW

IDS = [TW.case_id(c) for c in TW.CASES]


def test_matrix_spreads_the_axes():
    assert len(set(TW.CASES)) == 2 * len(TW.KS)
    for k in TW.KS:
        assert {c[1] for c in TW.CASES if c[0] == k} == {False, True}                       # every k stranded and canonical
        assert {c[3] for c in TW.CASES if c[0] == k} == {False, True}                       # ... one of them branchy, one clean
    for h in TW.HASHES:
        mine = [c for c in TW.CASES if c[2] == h]
        assert len(mine) >= 2 and any(c[0] >= 64 for c in mine) and {c[1] for c in mine} == {False, True}, h
    assert {c[3] for c in TW.CASES if c[1]} == {c[3] for c in TW.CASES if not c[1]} == {False, True}
    assert all(c[0] != 25 for c in TW.PATH_CASES) and {c[1] for c in TW.PATH_CASES} == {False, True}
    assert sorted(TW.GATE_CASES.values()) == [1, 3]
    a, b = TW.SHARD_CASES
    assert a[0] in (32, 33) and b[0] >= 64 and b[2] != (2, 2)


@pytest.mark.parametrize("case", TW.CASES, ids=IDS)
def test_few_seeds_are_invalid(case):
    w = TW.world(case)
    assert 1 <= w.n_invalid <= 3 and len(w.seeds) == 100
    assert w.seeds[2] != w.plain(w.seeds[2]) and b"U" in w.seeds[3] and w.seeds[4] in w.repeat_read


@pytest.mark.parametrize("case", TW.CASES, ids=IDS)
def test_walks_reach_every_stop_reason(case):
    wa = TW.walk_answers(case)
    reasons, lengths = set(), []
    for key, (_, res) in wa.items():
        if key[1] != "repeat":
            reasons |= {why for _, _, why, _, _ in res}
            lengths += [len(b) for b, _, _, _, _ in res]
    assert reasons >= {0, 1, 3, 4}, reasons
    assert max(lengths) == 60 and sum(n >= 10 for n in lengths) > len(lengths) // 10
    for direction in (0, 1):
        # the tandem repeat without a target, under a bound above its period: the walk meets the first k-mer it appended
        for key in ((direction, "repeat"), (direction, 1.0, 60, False)):
            b, _, why, _, _ = wa[key][1][4 if key[1] != "repeat" else 0]
            assert (len(b), why) == (TW.REPEAT_PERIOD, 2), (key, len(b), why)
        # ... and a target along the walk stops walks before the free walk's end
        free, aimed = wa[(direction, 1.0, 60, False)][1], wa[(direction, 1.0, 60, True)][1]
        assert sum(a[2] == 1 and len(a[0]) < len(f[0]) for a, f in zip(aimed, free)) >= 10


@pytest.mark.parametrize("case", TW.CASES, ids=IDS)
def test_greedy_lookahead_has_decisions_to_make(case):
    w = TW.world(case)
    ga = TW.greedy_answers(case)
    seeds = TW.greedy_seeds(w)
    assert len(seeds) == TW.GREEDY_N
    if w.branchy:           # lookahead 3 changes at least one walk relative to the plain maximum-count walk
        changed = sum(a[0] != b for d in (0, 1) for a, b in zip(ga[(d, 3, 30, False)], ga[(d, "plain")]))
        assert changed >= 1
    else:                   # lookahead 16 has forks to score (the worlds give 20 ... 48) and decides otherwise than lookahead 0 does (11 ... 21 of 40 walks)
        forks = 0
        for d in (0, 1):
            for sd, (app, _) in zip(seeds, ga[(d, 16, 8, False)]):
                for km in [sd] + w.walk_kmers(sd, app, d)[:-1]:
                    f, r, _ = w.og.get_kmers(km)
                    forks += int((w.og.neighbors(f[0], r[0], km[0] if d == 0 else km[-1], d)[2] >= 1).sum() >= 2)
        assert forks >= 10, forks
        assert sum(a[0] != b[0][:8] for d in (0, 1) for a, b in zip(ga[(d, 16, 8, False)], ga[(d, 0, 10, False)])) >= 5
    assert any(len(a[0]) == 30 for d in (0, 1) for a in ga[(d, 3, 30, False)])
    if case in TW.GATE_CASES:                                   # the gate does cut walks short
        assert sum(len(g[0]) < len(a[0]) for d in (0, 1) for g, a in zip(ga[(d, 3, 30, True)], ga[(d, 3, 30, False)])) >= 1


def test_deep_cases_are_branchy_and_spread():
    assert all(c[3] for c in TW.DEEP_CASES) and any(c[0] >= 64 for c in TW.DEEP_CASES)
    assert {c[1] for c in TW.DEEP_CASES} == {False, True} and len({c[2] for c in TW.DEEP_CASES}) == len(TW.DEEP_CASES)


@pytest.mark.parametrize("case", TW.DEEP_CASES, ids=[TW.case_id(c) for c in TW.DEEP_CASES])
def test_lookahead_16_fills_every_level_of_the_search_in_a_branchy_world(case):
    """every second absent k-mer is a false neighbour there, so the search tree about doubles from level to level: at each distance 1 ... 15
    from the seed the restatement opened neighbourhoods with two or more live neighbours — the kernel's frontier rows hold siblings at every
    depth and its backtracking returns to each of them — and at the last level it opened thousands of neighbourhoods"""
    da = TW.deep_answers(case)
    for direction in (0, 1):
        seeds, res, levels = da[direction]
        assert len(seeds) == TW.DEEP_N and all(len(b) == 1 for b, _ in res)
        for lv in levels:
            assert len(lv) == 16 and all(x >= 1 for x in lv), lv
            assert sum(x >= 2 for x in lv[1:]) >= 12 and lv[15] >= 1000, lv


@pytest.mark.parametrize("case", TW.CASES, ids=IDS)
def test_naive_extension_reaches_its_reasons(case):
    na = TW.naive_answers(case)
    reasons = {why for res in na.values() for _, why in res}
    assert reasons >= ({1, 2, 4} if case[3] else {0, 3, 5, 6}), reasons
    assert any(len(b) >= 3 for res in na.values() for b, _ in res)


def test_naive_extension_reaches_all_reasons_over_the_matrix():
    assert {why for case in TW.CASES for res in TW.naive_answers(case).values() for _, why in res} == set(range(8))


@pytest.mark.parametrize("case", TW.CASES, ids=IDS)
def test_neighbour_queries_meet_false_positives_where_they_should(case):
    f, r, by_dir = TW.neighbor_answers(case)
    assert f.size >= 200
    for direction in range(4):
        c4 = by_dir[direction][3]
        assert (c4[:-20] > 0).sum() >= f.size - 20                 # k-mers of the reads have their neighbours / are their own variants
    if case[3]:                                                    # branchy: k-mers that are not in the graph still get neighbours
        assert sum(int((by_dir[d][3][-20:] > 0).sum()) for d in range(4)) >= 1


@pytest.mark.parametrize("case", TW.PATH_CASES, ids=[TW.case_id(c) for c in TW.PATH_CASES])
def test_paths_of_every_kind(case):
    lefts, rights, want, trace = TW.path_answers(case)
    kinds = {None if p is None else len(p) > 0 for res in want.values() for p in res}
    assert kinds == {None, True, False}
    assert trace == {"from the left", "from the right", "walks meet"}, trace


@pytest.mark.parametrize("stranded", [False, True])
def test_hash_equal_kmers_are_told_apart_by_the_oracle(stranded):
    """k = 64, the read (AC) x 50: four different k-mers with the same (f, r).  The oracle's restatements compare bases, so they give the left
    column of the issue's table; a traversal that stopped at `hashes equal` would give another"""
    w = TW.hash_equal_world(stranded)
    fr = {tuple(int(x[0]) for x in w.og.get_kmers(km)[:2]) for km in TW.HASH_EQUAL_TWINS}
    assert fr == {(0, 0)}
    for direction in (0, 1):
        got = TW.hash_equal_answers(stranded, direction)
        assert {name: (len(v[0]), v[1]) for name, v in got.items()} == TW.HASH_EQUAL_TABLE, direction


@pytest.mark.parametrize("k", [64, 128])
@pytest.mark.parametrize("stranded", [False, True])
def test_homopolymer_twins_are_told_apart_by_the_oracle(k, stranded):
    w = TW.homopolymer_world(k, stranded)
    true, false = b"A" * k, TW.HOMOPOLYMER_FALSE_TARGET[k] * k
    ft, rt, _ = w.og.get_kmers(true); ff, rf, _ = w.og.get_kmers(false)
    assert ft[0] == ff[0] and (stranded or rt[0] == rf[0])
    want = TW.homopolymer_answers(k, stranded)
    assert (len(want["true"][1]), want["true"][3]) == (39, 1)                       # stops in front of A^k
    assert want["false"][1:] == want["unrelated"][1:] and (len(want["false"][1]), want["false"][3]) == (40, 2)   # A^k follows itself
