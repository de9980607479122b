"""The rules of rb_graph_paired_kmer_segments restated in Python from the reference's Java, and checked against hand-worked support
patterns.  tests/test_gpu_paired_segments.py applies the same restatement to support computed from the CPU oracle's pair filters.

  GraphUtils.breakWithReadPairedKmers, range form (R/util/GraphUtils.java:4184-4246) and whole-list form (:4248-4310);
  breakWithFragPairedKmers with numPairsRequired (:4312-4374) and without (:4376-4405).  interlockDistance is 0 in all four.
support[i] stands for graph.lookup{Read,Fragment}KmerPair(kmers.get(i), kmers.get(i+d)); it is only read for i <= lastIndex."""
import numpy as np
import pytest


def break_range(support, d, num_pairs_required, range_start, range_end):
    """breakWithReadPairedKmers(kmers, graph, numPairsRequired, rangeStart, rangeEnd), both branches, as written"""
    segments = []
    last_index = range_end - 1 - d
    start = end = -1
    if num_pairs_required == 1:
        for i in range(range_start, last_index + 1):
            if support[i]:
                if start < 0:
                    start = i
                end = i + d
            elif start >= 0 and i >= end:
                segments.append((start, end + 1))
                start = end = -1
    else:
        previous = 0
        for i in range(range_start, last_index + 1):
            if support[i]:
                previous += 1
                if previous >= num_pairs_required:
                    if start < 0:
                        start = i - num_pairs_required + 1
                    end = i + d
            else:
                if start >= 0 and i >= end:
                    segments.append((start, end + 1))
                    start = end = -1
                previous = 0
    if start >= 0:
        segments.append((start, end + 1))
    return segments


def break_read(support, nk, d, num_pairs_required, rng=None):
    """breakWithReadPairedKmers in its range form (rng = (rangeStart, rangeEnd)) or its whole-list form (rng None: [0, nk))"""
    a, b = rng if rng is not None else (0, nk)
    return break_range(support, d, num_pairs_required, a, b)


def break_frag(support, nk, d, num_pairs_required=None):
    """breakWithFragPairedKmers(kmers, graph[, numPairsRequired]): the whole-list loop; the two-argument form is the first branch"""
    return break_range(support, d, 1 if num_pairs_required is None else num_pairs_required, 0, nk)


def capacity(d, range_start, range_end):
    """the slots rb_graph_paired_kmer_segments reserves per sequence: consecutive segment starts are at least d + 1 apart"""
    span = range_end - 1 - d - range_start
    return span // (d + 1) + 1 if span >= 0 else 0


def pattern(s):
    """'1101' -> [True, True, False, True]"""
    return [c == "1" for c in s]


def test_a_miss_inside_the_last_pairs_span_does_not_close():
    # d = 3, nk = 10, lastIndex 6.  The hit at 0 sets end 3; the misses at 1 and 2 lie inside the span; the hit at 3 sets end 6; the misses
    # at 4 and 5 keep it open and the miss at 6 == end closes it
    assert break_read(pattern("1001000"), 10, 3, 1) == [(0, 7)]
    assert break_read(pattern("1010000"), 10, 3, 1) == [(0, 6)]


def test_a_miss_at_exactly_end_closes():
    # d = 2, nk = 10, lastIndex 7.  Hit at 0 -> end 2; the miss at 1 (< 2) keeps it; the miss at 2 == end closes [0, 3); the hit at 3 reopens
    assert break_read(pattern("10011000"), 10, 2, 1) == [(0, 3), (3, 7)]
    # a hit at 2 == end is a hit: it moves end to 4, and the miss at 3 stays inside; the miss at 4 == end closes
    assert break_read(pattern("10100000"), 10, 2, 1) == [(0, 5)]
    # the > 1 branch closes at i == end too: run 0..1 with n = 2 -> end 3, misses 2 (< 3) and 3 (== 3)
    assert break_read(pattern("11001100"), 10, 2, 2) == [(0, 4), (4, 8)]


def test_n_above_one_opens_at_i_minus_n_plus_one():
    # d = 2, n = 3: hits at 2, 3, 4; the count reaches 3 at i = 4 -> start = 4 - 3 + 1 = 2, end = 6
    assert break_read(pattern("0011100000"), 12, 2, 3) == [(2, 7)]
    # a run of 5 moves end with every hit from the third on
    assert break_read(pattern("0111110000"), 12, 2, 3) == [(1, 8)]


def test_hits_below_n_neither_open_nor_extend():
    # n = 3: runs of 2 never open
    assert break_read(pattern("1101101100"), 12, 2, 3) == []
    # opened by the run 0..2 (end 4); the run of 2 at 4..5 does not move end: the miss at 6 >= 4 closes [0, 5)
    assert break_read(pattern("11101100000"), 13, 2, 3) == [(0, 5)]
    # where n = 1 moves end to 5 + 2
    assert break_read(pattern("11101100000"), 13, 2, 1) == [(0, 8)]


def test_a_segment_left_open_at_the_end():
    assert break_read(pattern("0001111"), 10, 3, 1) == [(3, 10)]
    assert break_read(pattern("0001111"), 10, 3, 4) == [(3, 10)]
    assert break_frag(pattern("0001111"), 10, 3) == [(3, 10)]
    # a miss inside the span at the last index does not close it either: emitted after the loop
    assert break_read(pattern("0001110"), 10, 3, 1) == [(3, 9)]


def test_ranges_clip_last_index():
    # nk = 20, d = 3, support everywhere: the range [5, 12) has lastIndex 8 -> [5, 12)
    sup = [True] * 17
    assert break_read(sup, 20, 3, 1, (5, 12)) == [(5, 12)]
    assert break_read(sup, 20, 3, 2, (5, 12)) == [(5, 12)]
    # positions past lastIndex are never read, even where they would extend or close
    sup = pattern("11110000" + "1" * 9)
    assert break_read(sup, 20, 3, 1, (0, 7)) == [(0, 7)]
    assert break_read(sup, 20, 3, 1) == [(0, 7), (8, 20)]
    # the run count starts at rangeStart: a run that began before it counts from rangeStart only
    sup = pattern("1111100000" + "0" * 7)
    assert break_read(sup, 20, 3, 3, (2, 20)) == [(2, 8)]
    assert break_read(sup, 20, 3, 3, (3, 20)) == []


def test_range_shorter_than_the_distance():
    # rangeEnd - 1 - d < rangeStart: no position at all
    sup = [True] * 20
    assert break_read(sup, 25, 5, 1, (10, 15)) == []
    assert break_read(sup, 25, 5, 1, (10, 16)) == [(10, 16)]
    assert capacity(5, 10, 15) == 0 and capacity(5, 10, 16) == 1


def test_distance_at_least_the_list():
    assert break_read([], 4, 4, 1) == []
    assert break_read([], 4, 9, 2) == []
    assert break_frag([], 3, 3) == [] and capacity(3, 0, 3) == 0 and capacity(9, 0, 4) == 0


def test_empty_lists():
    assert break_read([], 0, 1, 1) == [] and break_frag([], 0, 1, 3) == [] and capacity(1, 0, 0) == 0
    assert break_read([], 5, 1, 1, (2, 2)) == []


def test_frag_two_argument_form_is_the_first_branch():
    sup = pattern("1100110011")
    assert break_frag(sup, 12, 2) == break_frag(sup, 12, 2, 1) == [(0, 4), (4, 8), (8, 12)]


def test_capacity_is_reached():
    # the bound is tight: alternating single hits d + 1 apart, each closed at its own end
    d, k_segs = 3, 5
    sup = pattern(("1" + "0" * d) * k_segs)
    nk = len(sup) + d
    got = break_read(sup, nk, d, 1)
    assert len(got) == k_segs == capacity(d, 0, nk)


@pytest.mark.parametrize("seed", range(6))
def test_capacity_bounds_the_segment_count(seed):
    rng = np.random.default_rng(seed)
    for _ in range(400):
        nk = int(rng.integers(0, 90))
        d = int(rng.integers(1, 25))
        n = int(rng.choice([1, 2, 3, 10]))
        sup = list(rng.random(max(nk - d, 0)) < rng.choice([0.1, 0.5, 0.9]))
        a = int(rng.integers(0, nk + 1)); b = int(rng.integers(a, nk + 1))
        for r in ((0, nk), (a, b)):
            got = break_read(sup, nk, d, n, r)
            assert len(got) <= capacity(d, *r)
            # segments lie in the range, in order, their starts at least d + 1 apart
            for (s0, e0), (s1, _) in zip(got, got[1:]):
                assert s1 >= s0 + d + 1 and s1 >= e0
            assert all(r[0] <= s < e <= r[1] for s, e in got)
