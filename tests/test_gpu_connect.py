"""rb_graph_connect_segments (GraphUtils.connect over a segment list on the device), connectSegments and graphutils.connect against the
reference's lines (restated in tests/test_connect_rules.py) run on the CPU oracle; the device graph and the oracle are built from the same reads
and their filters' bytes are equal.  Compared per read and per gap: every record field, the text byte for byte and zeros behind it up to the
read's capacity, out_offsets against the formula, the filters' digests before and after.  Worlds: k = 25, stranded and canonical, with the reach
assertion first; k = 16, 64 and 200 with hash counts (1, 1) and (3, 2); k = 64 with k-mers that hash alike and differ; n = 1, 63, 64, 65; a read
of 41 entries with runs of equal length; bounds at the LDS limit, one below, one above, and a placeholder of 3000; 20 003 reads in one call and
in pieces; the size query; every refusal; the public forms against the restatement and against the composed route on the same device graph."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rnabloom import _native as N
from rnabloom import graphutils, sharded
from rnabloom.graph import BloomFilterDeBruijnGraph, _pack
import test_extend_step_rules as R
import test_connect_rules as T

ERR_INVALID = 1                     # RB_ERR_INVALID
FILTERS = (N.DBGBF, N.CBF)
REC = ("outcome", "why", "gaps", "connected", "first_seg", "last_seg", "out_len", "pad")
GAP = ("connected", "how", "l_end", "r_end", "l_added", "r_added", "index", "path_len")
LDS_BOUND = 128                     # CN_LDS_BOUND of rb_connect.hip
DEVICES = {}


@pytest.fixture(scope="module", autouse=True)
def release_the_device_graphs():
    yield
    for g in DEVICES.values():
        g.destroy()
    DEVICES.clear()


def device(w):
    """the device twin of a world's oracle graph: the same reads through addReads, the filters' bytes equal to the oracle's"""
    if id(w) not in DEVICES:
        g = BloomFilterDeBruijnGraph(w.sizes[0], w.sizes[1], 1_000_003, w.hashes[0], w.hashes[1], 2, w.k, w.stranded, False, rngSeed=5)
        g.addReads(*w.packed, 3)
        assert (g.exportFilter(N.DBGBF) == w.og.dbgbf_bytes()).all() and (g.exportFilter(N.CBF) == w.og.cbf_bytes()).all()
        DEVICES[id(w)] = g
    return DEVICES[id(w)]


def flat(lists):
    seq, so = _pack([s for segs in lists for s in segs])
    rs = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(segs) for segs in lists], out=rs[1:])
    return seq, so, rs


def run(g, lists):
    return g.connectSegmentsFlat(*flat(lists))


def capacity(lists):
    return np.cumsum([0] + [sum(len(s) + (i & 1) for i, s in enumerate(segs)) for segs in lists])


def check(got, lists, want, label):
    out, oo, recs, grecs = got
    assert oo.tolist() == capacity(lists).tolist(), label
    assert len(grecs) == sum(len(s) // 2 for s in lists)
    at = 0
    for i, (rc, w) in enumerate(zip(recs, want)):
        assert tuple(int(rc[f]) for f in REC) == w.record(), (label, i, lists[i], rc, w)
        for j, gw in enumerate(w.gaps):
            assert tuple(int(grecs[at + j][f]) for f in GAP) == gw.record(), (label, i, j, lists[i], grecs[at + j], gw)
        at += len(w.gaps)
        n = len(w.text)
        assert out[oo[i]:oo[i] + n].tobytes() == w.text and not out[oo[i] + n:oo[i + 1]].any(), (label, i, lists[i], out[oo[i]:oo[i + 1]].tobytes(), w)


def digests(h):
    out = []
    for f in FILTERS:
        v = C.c_uint64()
        out.append(v.value if N.lib.rb_filter_fold(h, f, C.byref(v)) == 0 else None)
    return out


@pytest.mark.parametrize("stranded", [False, True])
def test_records_and_text_match_the_restatement(stranded):
    w = T.world(25, stranded)
    w.assert_every_branch_is_reached()
    g = device(w)
    before = digests(g.h)
    assert None not in before and 0 not in before
    check(run(g, w.lists), w.lists, w.want(), ("k25", stranded))
    assert digests(g.h) == before                                                          # read-only over a full run
    # the public forms: lists of strings or bytes in, (bytes, outcome, why) out; graphutils.connect: bytes or None
    some = w.lists[-60:]
    got = g.connectSegments([[s.decode("latin1") for s in segs] for segs in some[:30]] + some[30:])
    assert got == [(x.text, x.outcome, x.why) for x in w.want()[-60:]]
    assert graphutils.connect(g, some) == [None if x.outcome == T.NOT_JUDGED else x.text for x in w.want()[-60:]]
    assert g.connectSegments([]) == [] and graphutils.connect(g, []) == []


@pytest.mark.parametrize("k,stranded,hashes", [(16, False, (1, 1)), (16, True, (3, 2)), (64, False, (3, 2)), (64, True, (1, 1)), (200, False, (3, 2)), (200, True, (1, 1))])
def test_other_k_and_hash_counts(k, stranded, hashes):
    w = T.world(k, stranded, hashes)
    want = w.want()
    hows = {x.how for r in want for x in r.gaps}
    assert {T.LEFT_ARRIVED, T.PATHS_MEET, T.EXHAUSTED, T.HOW_NOT_RUN} <= hows, hows           # (every branch is the k = 25 worlds' business)
    check(run(device(w), w.lists), w.lists, want, (k, stranded, hashes))


class TwinWorld:
    """the graph of the single read (AC) x 50 at k = 64: (AC)^32, (CA)^32, (GT)^32 and (TG)^32 all hash to f = 0, r = 0 (tests/test_join_rules.py)"""
    LISTS = [[b"AC" * 32, b"N" * 6, b"GT" * 32], [b"AC" * 32, b"N" * 6, b"TG" * 32], [b"AC" * 33, b"N" * 6, b"GT" * 32], [b"AC" * 32, b"N" * 6, b"AC" * 32],
             [b"CA" * 32 + b"C", b"", b"CA" * 32], [b"AC" * 32, b"N", b"CA" * 32, b"NN", b"AC" * 33]]

    def __init__(self, stranded):
        from oracle import rbo
        self.k, self.stranded, self.hashes, self.sizes = 64, stranded, (2, 2), (400_009, 400_009)
        self.og = rbo.Graph(self.sizes[0], self.sizes[1], 1_000_003, 2, 2, 2, self.k, stranded, False, 5)
        reads = [b"AC" * 50]
        self.packed = rbo.pack_reads(reads, [b"I" * len(s) for s in reads])
        self.og.add_reads(*self.packed, 3, 0)
        self.o = R.OracleSide(self.og)


def test_kmers_that_hash_alike_and_differ():
    for stranded in (False, True):
        w = TwinWorld(stranded)
        want = [T.connect(w.o, s, 0, 64) for s in w.LISTS]
        # the left path holds (CA)^32 and (AC)^32; by hash alone the first neighbour would "be" (GT)^32 and the left walk would arrive at once
        assert want[0].gaps[0].l_end == T.LOOP and want[0].gaps[0].l_added == 2 and want[3].gaps[0].record()[:3] == (1, T.LEFT_ARRIVED, T.ARRIVED)
        if not stranded:                                                                   # the right walk proposes (TG)^32, which hashes like the left path's k-mers
            assert want[0].gaps[0].record() == (0, T.RIGHT_LOOP, T.LOOP, T.LOOP, 2, 2, -1, 0)
        check(run(device(w), w.LISTS), w.LISTS, want, ("twins", stranded))


@pytest.mark.parametrize("stranded", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_read_counts_around_the_wavefront(n, stranded):
    w = T.world(25, stranded)
    check(run(device(w), w.lists[:n]), w.lists[:n], w.want()[:n], ("n", n, stranded))


def test_a_read_of_41_entries_with_runs_of_equal_length():
    w = T.world(25, False)
    k, s = w.k, w.k + 5
    t = w.plain[0]
    segs, at = [], 0
    for i in range(21):
        seg = t[at:at + s]
        if i % 2 == 1:                                                                     # every second segment ends in an error: the gap behind it stays open
            seg = R.put(seg, s - 1, "ACGT"[(T.ACGT.index(seg[-1:]) + 1) % 4])
        segs += [seg, b"N"]
        at += s + 1
    segs.pop()
    assert len(segs) == 41
    want = T.connect(w.o, segs, 0, k)
    assert [x.connected for x in want.gaps] == [1, 0] * 10 and (want.first_seg, want.last_seg, len(want.text)) == (0, 2, 2 * s + 1)
    lists = [segs, segs[2:], segs[:39]]
    check(run(device(w), lists), lists, [want] + [T.connect(w.o, x, 0, k) for x in lists[1:]], "41 entries")


def test_bounds_around_the_lds_limit_and_rows_in_device_scratch():
    w = T.world(25, False)
    k = w.k
    t = w.plain[0]
    lists = []
    for bound in (LDS_BOUND - 1, LDS_BOUND, LDS_BOUND + 1):                                 # the true gap under its placeholder: the left walk needs bound - 1 steps ...
        m = bound - k
        lists.append([t[20:60], b"N" * m, t[60 + m:120 + m]])
        lists.append([t[20:60], b"N" * m, t[61 + m:120 + m]])                              # ... and one more than the bound gives: the walks meet
        lists.append([t[20:60], b"N" * m, R.put(t[60 + m:120 + m], 0, "ACGT"[(T.ACGT.index(t[60 + m:61 + m]) + 1) % 4])])
    lists.append([t[20:60], b"N" * 3000, t[65:120]])                                        # a placeholder of 3000 over a gap of 5
    lists.append([t[20:60], b"N" * 3000, t[600:700]])                                       # ... and over 540 letters: a long path in a scratch row
    lists.append([t[20:60], b"N" * 3000, w.plain[1][300:340], b"N" * 2, w.plain[1][342:380]])   # ... and to another transcript: both walks run to dead ends
    lists.append([t[20:60], b"N" * 3, t[63:100]])                                           # (a launch of each instantiation in one piece)
    want = [T.connect(w.o, x, 0, k) for x in lists]
    assert [want[i].gaps[0].how for i in (0, 3, 6)] == [T.LEFT_ARRIVED] * 3 and want[10].gaps[0].path_len == 540 + k - 1
    assert {want[i].gaps[0].how for i in (1, 4, 7)} == {T.PATHS_MEET}
    check(run(device(w), lists), lists, want, "lds limit")


def test_twenty_thousand_reads_and_small_pieces(monkeypatch):
    w = T.world(25, False)
    g = device(w)
    idx = [i % len(w.lists) for i in range(20_003)]
    lists = [w.lists[i] for i in idx]
    args = flat(lists)
    whole = g.connectSegmentsFlat(*args)
    assert [tuple(int(rc[f]) for f in REC) for rc in whole[2]] == [w.want()[i].record() for i in idx]
    for piece in ("100000", "4099"):
        monkeypatch.setenv("RB_QUERY_PIECE", piece)
        got = g.connectSegmentsFlat(*args)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, whole)), piece
    monkeypatch.setenv("RB_QUERY_PIECE", "1")              # a read a piece
    got = run(g, lists[:300])
    n, ng = int(got[1][-1]), len(got[3])
    assert got[0][:n].tobytes() == whole[0][:n].tobytes() and got[2].tobytes() == whole[2][:300].tobytes() and got[3].tobytes() == whole[3][:ng].tobytes()


def raw_call(h, lists, min_cov=1.0, lookahead=3, seq=True, so=True, rs=True, oo=True, out=True, recs=True, gaps=True, seg_offsets=None, read_segs=None, n=None):
    a_seq, a_so, a_rs = flat(lists)
    a_seq = np.concatenate([a_seq, np.zeros(70_000, np.uint8)])
    if seg_offsets is not None:
        a_so = np.asarray(seg_offsets, np.int64)
    if read_segs is not None:
        a_rs = np.asarray(read_segs, np.int64)
    n = len(a_rs) - 1 if n is None else n
    a_oo = np.full(len(a_rs), 7, np.int64); a_out = np.full(300_000, 7, np.uint8); a_rec = np.full(max(n, 1) * 8, 7, np.int32)
    a_gap = np.full(8 * max(1, len(a_so)), 7, np.int32)
    p = lambda a, use: a.ctypes.data_as(C.c_void_p) if use else None
    rc = N.lib.rb_graph_connect_segments(h, p(a_seq, seq), p(a_so, so), p(a_rs, rs), n, lookahead, min_cov, p(a_oo, oo), p(a_out, out), p(a_rec, recs), p(a_gap, gaps))
    return rc, a_oo, a_out, a_rec, a_gap


def refused(h, lists, **kw):
    """one refused call: RB_ERR_INVALID with a message, no output byte written (the offsets are host bookkeeping), the handle's filters as they were"""
    before = digests(h) if h is not None else None
    r = raw_call(h, lists, **kw)
    assert r[0] == ERR_INVALID and N.lib.rb_last_error(), kw
    assert (r[2] == 7).all() and (r[3] == 7).all() and (r[4] == 7).all(), kw
    if h is not None:
        assert digests(h) == before and any(d is not None for d in before), kw


def test_size_query_and_refusals_leave_everything_alone():
    w = T.world(25, False)
    g = device(w)
    lists = [x for x in w.lists[:40] if x]
    before = digests(g.h)
    untouched = lambda r: (r[2] == 7).all() and (r[3] == 7).all() and (r[4] == 7).all()
    r = raw_call(g.h, lists)
    assert r[0] == 0 and r[1].tolist() == capacity(lists).tolist() and r[1][-1] <= 300_000 and not untouched(r)
    r = raw_call(g.h, lists, gaps=False)                                                   # the gap records are optional
    assert r[0] == 0 and (r[4] == 7).all() and (r[3] != 7).any()
    r = raw_call(g.h, lists, out=False, recs=False, gaps=False)                            # the size query: offsets only
    assert r[0] == 0 and r[1].tolist() == capacity(lists).tolist() and untouched(r)
    r = raw_call(g.h, lists, out=False)                                                    # ... with records given: still nothing but offsets
    assert r[0] == 0 and untouched(r)
    r = raw_call(g.h, [])
    assert r[0] == 0 and untouched(r) and (r[1] == 7).all()                                 # n == 0 touches nothing
    assert raw_call(g.h, [], seq=False, so=False, rs=False, oo=False, out=False, recs=False, gaps=False)[0] == 0
    assert digests(g.h) == before
    _, so, rs = flat(lists)
    down_so = so.copy(); down_so[3] = down_so[2] - 1
    down_rs = rs.copy(); down_rs[2] = down_rs[1] - 1
    far = [[lists[0][0], b"N" * (65536 - 25 + 1), lists[0][0]]]
    for kw in (dict(so=False), dict(rs=False), dict(oo=False), dict(recs=False), dict(seq=False), dict(n=-1), dict(min_cov=float("nan")),
               dict(min_cov=float("inf")), dict(min_cov=-1.0), dict(seg_offsets=down_so), dict(read_segs=down_rs)):
        refused(g.h, lists, **kw)
    refused(g.h, far)                                                                       # a bound above RB_CONNECT_MAX_BOUND
    assert raw_call(g.h, [[lists[0][0], b"N" * (65536 - 25), lists[0][0]]], out=False, recs=False, gaps=False)[0] == 0      # the ceiling itself is accepted
    refused(None, lists)
    rk = sharded.ShardRank((100_003, 200_003, 30_011, 2, 2, 2, 25, 0, 1, 0, 0, 9, 0), 0, 1, 0, "split")
    refused(rk.h, lists)                                                                    # a shard handle
    rk.destroy()
    for destroy, gone in (("destroyCbf", N.CBF), ("destroyDbgbf", N.DBGBF)):
        g2 = BloomFilterDeBruijnGraph(400_009, 800_011, 400_031, 2, 2, 2, 25, False, False)
        g2.addReads(*w.packed, 3)
        full = digests(g2.h)
        assert None not in full and 0 not in full
        assert raw_call(g2.h, lists)[0] == 0 and digests(g2.h) == full
        getattr(g2, destroy)()
        left = digests(g2.h)
        assert [d is None for d in left] == [f == gone for f in FILTERS]
        refused(g2.h, lists)                                                                # the filter that remains is as it was
        g2.destroy()
    with pytest.raises(N.NativeError):
        g.connectSegmentsFlat(np.zeros(10, np.uint8), [0, 5, 3], [0, 2])
    assert digests(g.h) == before


def test_lookahead_is_not_read_and_min_kmer_cov_is():
    w = T.world(25, True)
    g = device(w)
    lists = w.lists[:80]
    a = g.connectSegmentsFlat(*flat(lists), lookahead=0)
    b = g.connectSegmentsFlat(*flat(lists), lookahead=7)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    c = g.connectSegmentsFlat(*flat(lists), minKmerCov=1.0e6)                               # no neighbour is that heavy: every walk ends at once
    run_gaps = [x for x in c[3] if x["how"] != T.HOW_NOT_RUN]
    assert run_gaps and all((x["how"], x["l_end"], x["r_end"]) == (T.EXHAUSTED, T.NO_NEIGHBOR, T.NO_NEIGHBOR) for x in run_gaps)


def test_profile_entry():
    w = T.world(25, True)
    g = device(w)
    g.profileEnable(True)
    run(g, w.lists[:100])
    prof = g.profileGet()
    assert prof["connect"][0] > 0 and prof["connect"][1] == 1, prof
    g.profileEnable(False)


@pytest.mark.parametrize("stranded", [False, True])
def test_the_composed_route_on_the_same_device_graph_agrees(stranded):
    """graphutils.connectComposed (getMaxCoveragePaths in two lane-per-walk launches per bound, stitched on the host) and graph.connectSegments are
    two implementations in the library: they agree on every list both can be asked about, and with the restatement"""
    w = T.world(25, stranded)
    g = device(w)
    pick = [(s, x) for s, x in zip(w.lists, w.want()) if x.outcome in (T.EMPTY, T.SINGLE, T.CHAINED) and all(T.is_acgtu(e) and e == e.upper() and b"U" not in e for e in s[::2])][:150]
    lists = [s for s, _ in pick]
    fused = graphutils.connect(g, lists)
    assert fused == [x.text for _, x in pick]
    assert graphutils.connectComposed(g, lists) == fused
