"""The worlds of tests/subsample_worlds.py ask something: with the restatement alone (no GPU), every status and every deciding line occurs, reads are
kept and dropped in comparable numbers, hashes repeat inside a read, increments of one read share counters, and the random draw matters."""
import numpy as np
import pytest

import subsample_worlds as W
from oracle import rbo
from rnabloom import _native as N
from test_subsample_rules import DROPPED, F, KEPT_SCAN, KEPT_START_FAILED, KEPT_TAIL, NOT_JUDGED

IDS = [W.world_id(w) for w in W.WORLDS]


def of_mode(mode):
    return [i for i, w in enumerate(W.WORLDS) if w["mode"] == mode]


def test_every_status_and_every_deciding_line_occurs():
    got = {"strobemer": set(), "kmer": set()}
    for i, w in enumerate(W.WORLDS):
        keep, recs, _, _ = W.want(i)
        got[w["mode"] + ("-c" if w["canonical"] else "")] = got.get(w["mode"] + ("-c" if w["canonical"] else ""), set()) | {(int(r[0]), int(r[1])) for r in recs}
        assert ((recs[:, 0] == DROPPED) | (recs[:, 0] == NOT_JUDGED)).tolist() == (keep == 0).tolist()
    assert got["strobemer"] == {(KEPT_SCAN, N.SUB_LINE_SEEN_BEYOND_EDGE), (KEPT_SCAN, N.SUB_LINE_MERGE_FAILED), (KEPT_SCAN, N.SUB_LINE_UNSEEN_BEYOND_EDGE),
                                (KEPT_SCAN, N.SUB_LINE_GAP), (KEPT_TAIL, N.SUB_LINE_TAIL), (DROPPED, N.SUB_LINE_TAIL),
                                (KEPT_START_FAILED, N.SUB_LINE_START_FAILED)}
    assert got["kmer"] == {(DROPPED, N.SUB_LINE_KMER_START_FAILED), (NOT_JUDGED, N.SUB_LINE_KMER_RANGE), (KEPT_SCAN, N.SUB_LINE_KMER_CHAIN),
                           (DROPPED, N.SUB_LINE_KMER_NO_CHAIN)}
    assert got["kmer-c"] == {(DROPPED, N.SUB_LINE_KMER_START_FAILED_C), (NOT_JUDGED, N.SUB_LINE_KMER_RANGE_C), (KEPT_SCAN, N.SUB_LINE_KMER_CHAIN_C),
                             (DROPPED, N.SUB_LINE_KMER_NO_CHAIN_C)}


def test_the_tail_test_keeps_with_and_without_an_interval():
    recs = np.concatenate([W.want(i)[1] for i in of_mode("strobemer")])
    tail = recs[recs[:, 0] == KEPT_TAIL]
    assert (tail[:, F["nam_end"]] == -1).any() and (tail[:, F["nam_end"]] >= 0).any()


def test_reads_are_kept_and_dropped():
    kept = total = 0
    for i in range(len(W.WORLDS)):
        keep = W.want(i)[0]
        print(IDS[i], "kept %d of %d" % (keep.sum(), keep.size))
        kept += int(keep.sum()); total += keep.size
        assert 0 < keep.sum() < keep.size
    assert 0.2 <= kept / total <= 0.8, kept / total
    for mode in ("strobemer", "kmer"):                              # and so in either mode
        k = sum(int(W.want(i)[0].sum()) for i in of_mode(mode)); t = sum(W.want(i)[0].size for i in of_mode(mode))
        assert 0.2 <= k / t <= 0.8, (mode, k / t)


def test_one_reads_increments_share_counters_in_the_small_filters():
    """a kept read with more distinct hashes than the filter has counters: two of them share one, whatever the hash functions"""
    for i, w in enumerate(W.WORLDS):
        if w["size"] == W.SMALL:
            keep, recs, _, _ = W.want(i)
            assert (recs[keep == 1, F["incremented"]] > W.SMALL).any(), IDS[i]
            assert (recs[keep == 1, F["incremented"]] > 0).sum() >= 3, IDS[i]       # and later reads meet counters that earlier ones moved


def test_hashes_repeat_inside_a_read():
    for mode in ("strobemer", "kmer"):
        hit = 0
        for i in of_mode(mode):
            keep, recs, _, _ = W.want(i)
            if mode == "strobemer":
                hit += int(((keep == 1) & (recs[:, F["incremented"]] < recs[:, F["unseen"]])).sum())
            else:                                                   # three lists of end - start, - 1 and + 1 pairs
                hit += int(((keep == 1) & (recs[:, F["incremented"]] < 3 * recs[:, F["elements"]])).sum())
        assert hit >= 2, mode
    homo = b"A" * 300
    assert any(homo in W.reads_of(i) for i in range(len(W.WORLDS)))
    assert len(set(rbo.strobemers(homo, W.K, 3, W.W_MIN, W.W_MAX)[0].tolist())) == 1


def test_the_random_draw_matters_in_a_kmer_world():
    """MiniFloat.increment is deterministic up to 15 (R/util/MiniFloat.java:31-37): a counter above 16 went through the generator"""
    tops = {IDS[i]: int(W.want(i)[2].max()) for i in of_mode("kmer")}
    assert max(tops.values()) > 16, tops
    assert any(int(W.want(i)[2].max()) > 16 for i in of_mode("kmer") if W.WORLDS[i]["size"] == W.SMALL), tops


def test_the_edges_of_the_walker_are_in_every_world():
    for i, w in enumerate(W.WORLDS):
        recs = W.want(i)[1]
        el = set(recs[:, F["elements"]].tolist())
        assert {63, 64, 65, 255, 256, 257, 1023, 1024, 1025} <= el, (IDS[i], sorted(el)[:20])
        assert recs[:, F["elements"]].max() > N.SUB_LDS_ELEMS
        reads = W.reads_of(i)
        big = [len(r) for r in reads].index(3000)                  # kept, with more candidates for the set than LDS holds (a filter of 257 counters
        if w["size"] == W.REAL or w["mode"] == "kmer":             # is full of false positives by then, and in strobemer mode they bridge the read)
            assert recs[big, 0] == KEPT_SCAN and (recs[big, F["unseen"]] if w["mode"] == "strobemer" else 3 * recs[big, F["elements"]]) > N.SUB_LDS_ELEMS
        assert len(reads) >= len(set(reads)) + 7 and 240 <= len(reads) <= 320
        if w["mode"] == "strobemer":
            assert {0, W.W_MAX + 1 - W.W_MIN} <= el               # 2 * wMax + k - 1 letters: start() fails; one letter more: wMax + 1 - wMin strobemers


@pytest.mark.parametrize("i", range(len(W.WORLDS)), ids=IDS)
def test_every_world_keeps_drops_and_counts(i):
    keep, recs, data, ordinal = W.want(i)
    assert ordinal == int(recs[:, F["incremented"]].sum()) > 0
    assert int((data != 0).sum()) > 0 and (recs[keep == 0, F["incremented"]] == 0).all()
