"""rb_graph_join_pairs (GraphUtils.join on the device) and graphutils.overlapAndConnect against the reference's lines (restated in
tests/test_join_rules.py) run on the CPU oracle, a device graph and the oracle built from the same reads through addReads with
storeReadPairedKmers.  Compared per pair: every record field, the two thresholds as bits, the text byte for byte and zeros behind it up to the
pair's capacity.  Worlds: k = 25, stranded and canonical, d = 30; d = 2 and 3; d = 256 (the last distance whose step rows live in LDS) and 300
(rows in device scratch) with reads longer than d k-mers; k = 64 with k-mers that hash alike and differ; n = 1, 63, 64, 65; bounds 0, 1,
below and far beyond the gaps; 20 003 pairs in one call and in pieces; the size query; every refusal with the filters' digests before and
after.  Each world first shows on the oracle alone that its branches are reached (the rules file's reach check)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rnabloom import _native as N
from rnabloom import graphutils, sharded
from rnabloom.graph import BloomFilterDeBruijnGraph, _pack
import test_join_rules as J

ERR_INVALID = 1                     # RB_ERR_INVALID
FILTERS = (N.DBGBF, N.CBF, N.RPKBF)
FIELDS = ("outcome", "why", "l_end", "r_end", "l_added", "r_added", "l_forks", "r_forks", "index", "out_len")
DEVICES = {}
bits = lambda x: np.float32(x).view(np.uint32)


@pytest.fixture(scope="module", autouse=True)
def release_the_device_graphs():
    """the worlds' device graphs are shared by the tests of this file and destroyed behind the last one"""
    yield
    for g in DEVICES.values():
        g.destroy()
    DEVICES.clear()


def device(w):
    """the device twin of a world's oracle graph: the same reads through addReads, the filters' bytes equal to the oracle's"""
    if id(w) not in DEVICES:
        g = BloomFilterDeBruijnGraph(*w.sizes, *w.hashes, w.k, w.stranded, True, rngSeed=5)
        g.setReadPairedKmerDistance(w.d)
        g.addReads(*w.packed, 3, storeReadPairedKmers=True)
        assert (g.exportFilter(N.DBGBF) == w.og.dbgbf_bytes()).all() and (g.exportFilter(N.CBF) == w.og.cbf_bytes()).all()
        assert (g.exportFilter(N.RPKBF) == w.og.rpkbf_bytes()).all()
        DEVICES[id(w)] = g
    return DEVICES[id(w)]


def run(g, pairs, bound, grad, tip, min_cov):
    (lseq, lo), (rseq, ro) = _pack([l for l, _ in pairs]), _pack([r for _, r in pairs])
    return g.joinPairsFlat(lseq, lo, rseq, ro, bound, grad, tip, min_cov)


def capacity(pairs, bound, d, k):
    nk = lambda s: max(0, len(s) - k + 1)
    return np.cumsum([0] + [nk(l) + nk(r) + 2 * (bound + d + 2) + k - 1 for l, r in pairs])


def check(got, pairs, want, bound, d, k, label):
    out, oo, recs = got
    assert oo.tolist() == capacity(pairs, bound, d, k).tolist(), label
    for i, (rc, w) in enumerate(zip(recs, want)):
        have = tuple(int(rc[f]) for f in FIELDS)
        assert have == w.record(), (label, i, pairs[i], have, w)
        assert bits(rc["l_threshold"]) == bits(w.l_thr) and bits(rc["r_threshold"]) == bits(w.r_thr), (label, i, rc, w)
        n = len(w.text)
        assert out[oo[i]:oo[i] + n].tobytes() == w.text and not out[oo[i] + n:oo[i + 1]].any(), (label, i)


def compare(w, g, label, take=None, bound=None):
    pairs = w.pairs[:take]
    bound = w.BOUND if bound is None else bound
    want = w.want()[:take] if bound == w.BOUND else [J.join(w.o, l, r, bound, w.GRAD, w.TIP, w.MIN_COV, w.d, w.k) for l, r in pairs]
    check(run(g, pairs, bound, w.GRAD, w.TIP, w.MIN_COV), pairs, want, bound, w.d, w.k, label)
    return want


def digests(h):
    """rb_filter_fold of the three filters of a handle, None for one that is not there (destroyed, or never made)"""
    out = []
    for f in FILTERS:
        v = C.c_uint64()
        out.append(v.value if N.lib.rb_filter_fold(h, f, C.byref(v)) == 0 else None)
    return out


@pytest.mark.parametrize("stranded", [False, True])
def test_records_and_text_match_the_restatement(stranded):
    w = J.world(25, stranded)
    w.assert_every_branch_is_reached()
    g = device(w)
    before = digests(g.h)
    assert None not in before and 0 not in before
    compare(w, g, ("d30", stranded))
    assert digests(g.h) == before                                                          # read-only over a full run
    # the public form: strings in, (bytes | None, outcome, why) out
    got = g.joinPairs([l.decode("latin1") for l, _ in w.pairs[:60]], [r for _, r in w.pairs[:60]], w.BOUND, w.GRAD, w.TIP, w.MIN_COV)
    assert got == [(x.text if x.outcome == J.JOINED else None, x.outcome, x.why) for x in w.want()[:60]]
    assert g.joinPairs([], [], 5, 0.5, 1, 1.0) == []


SMALL = {}


def small_world(d):
    """worlds for the edges of the step's mapping: d = 2, 3; d = 256, 300 with reads of more than d k-mers, so that a step reads d k-mers of a path"""
    if d not in SMALL:
        if d <= 3:
            SMALL[d] = J.JoinWorld(25, False, seed=800 + d, d=d, n_pairs=200, n_iso=3)
        else:
            SMALL[d] = J.JoinWorld(25, d % 2 == 1, seed=800 + d, d=d, n_pairs=120, read_len=d + 35, n_iso=3, tile=50, tx_len=4 * (d + 100))
    return SMALL[d]


@pytest.mark.parametrize("d", [2, 3, 256, 300])
def test_edges_of_the_distance(d):
    w = small_world(d)
    want = w.want()
    assert {J.NONE, J.JOINED} <= {x.outcome for x in want} and any(x.l_forks or x.r_forks for x in want), d
    compare(w, device(w), ("d", d))


@pytest.mark.parametrize("stranded", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_pair_counts_around_the_wavefront(n, stranded):
    w = J.world(25, stranded)
    compare(w, device(w), ("n", n, stranded), take=n)


@pytest.mark.parametrize("bound", [0, 1, 5, 60])
def test_bounds(bound):
    """0 and 1; 5, below most gaps; 60, far beyond every gap (1 .. 25 k-mers)"""
    w = J.world(25, False)
    want = compare(w, device(w), ("bound", bound), take=150, bound=bound)
    if bound == 0:
        assert all(x.outcome != J.JOINED and x.l_added == 0 == x.r_added for x in want)
    if bound == 60:
        assert sum(x.outcome == J.JOINED for x in want) > sum(x.outcome == J.JOINED for x in w.want()[:150])


def test_kmers_that_hash_alike_and_differ():
    for stranded in (False, True):
        w = J.TwinWorld(stranded)
        g = device(w)
        want = w.want()
        assert all((x.outcome, x.why) == (J.NONE, J.RIGHT_LOOP) for x in want)              # by hash alone: JOINED, REACHED_RIGHT (the rules file)
        check(run(g, w.PAIRS, w.BOUND, w.GRAD, 1, 1.0), w.PAIRS, want, w.BOUND, w.d, w.k, ("twins", stranded))


def test_twenty_thousand_pairs_and_small_pieces(monkeypatch):
    w = J.world(25, False)
    g = device(w)
    idx = [i % len(w.pairs) for i in range(20_003)]
    pairs = [w.pairs[i] for i in idx]
    whole = run(g, pairs, w.BOUND, w.GRAD, w.TIP, w.MIN_COV)
    assert [tuple(int(rc[f]) for f in FIELDS) for rc in whole[2]] == [w.want()[i].record() for i in idx]
    for piece in ("100000", "4099"):                       # 640 000 k-mers: 7 and 160 pieces
        monkeypatch.setenv("RB_QUERY_PIECE", piece)
        got = run(g, pairs, w.BOUND, w.GRAD, w.TIP, w.MIN_COV)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, whole)), piece
    monkeypatch.setenv("RB_QUERY_PIECE", "1")              # a pair a piece
    got = run(g, pairs[:300], w.BOUND, w.GRAD, w.TIP, w.MIN_COV)
    n = int(got[1][-1])
    assert got[0][:n].tobytes() == whole[0][:n].tobytes() and got[2].tobytes() == whole[2][:300].tobytes()


def raw_call(h, pairs, bound=20, grad=0.5, tip=10, min_cov=1.0, lseq=True, loff=True, rseq=True, roff=True, oo=True, out=True, recs=True, loffsets=None):
    (ls, lo), (rs, ro) = _pack([l for l, _ in pairs]), _pack([r for _, r in pairs])
    if loffsets is not None:
        lo = np.asarray(loffsets, np.int64)
    n = len(lo) - 1
    a_oo = np.full(n + 1, 7, np.int64); a_out = np.full(200_000, 7, np.uint8); a_rec = np.full(max(n, 1) * 12, 7, np.int32)
    p = lambda a, use: a.ctypes.data_as(C.c_void_p) if use else None
    rc = N.lib.rb_graph_join_pairs(h, p(ls, lseq), p(lo, loff), p(rs, rseq), p(ro, roff), n, bound, grad, tip, min_cov, p(a_oo, oo), p(a_out, out), p(a_rec, recs))
    return rc, a_oo, a_out, a_rec


def refused(h, pairs, **kw):
    """one refused call: RB_ERR_INVALID with a message, no output byte written, the handle's filters as they were"""
    before = digests(h) if h is not None else None
    r = raw_call(h, pairs, **kw)
    assert r[0] == ERR_INVALID and N.lib.rb_last_error(), kw
    assert (r[1] == 7).all() and (r[2] == 7).all() and (r[3] == 7).all(), kw               # nothing was launched, nothing written
    if h is not None:
        assert digests(h) == before and any(d is not None for d in before), kw


def test_size_query_and_refusals_leave_everything_alone():
    w = J.world(25, False)
    g = device(w)
    pairs = w.pairs[:40]
    before = digests(g.h)
    untouched = lambda r: (r[2] == 7).all() and (r[3] == 7).all()
    r = raw_call(g.h, pairs)
    assert r[0] == 0 and r[1].tolist() == capacity(pairs, 20, w.d, w.k).tolist() and r[1][-1] <= 200_000
    r = raw_call(g.h, pairs, out=False, recs=False)                                        # the size query: offsets only
    assert r[0] == 0 and r[1].tolist() == capacity(pairs, 20, w.d, w.k).tolist() and untouched(r)
    r = raw_call(g.h, pairs, out=False)                                                    # ... with recs given: still nothing but offsets
    assert r[0] == 0 and untouched(r)
    r = raw_call(g.h, [])
    assert r[0] == 0 and untouched(r) and (r[1] == 7).all()                                 # n == 0 touches nothing
    assert raw_call(g.h, [], lseq=False, loff=False, rseq=False, roff=False, oo=False, out=False, recs=False)[0] == 0
    assert digests(g.h) == before
    nq = len(pairs)
    for kw in (dict(loff=False), dict(roff=False), dict(oo=False), dict(recs=False), dict(lseq=False), dict(rseq=False), dict(bound=-1),
               dict(bound=65537), dict(grad=float("nan")), dict(grad=float("inf")), dict(grad=-0.5), dict(min_cov=float("nan")),
               dict(min_cov=float("inf")), dict(min_cov=-1.0), dict(loffsets=[0, 90, 40] + [40] * (nq - 2))):
        refused(g.h, pairs, **kw)
    assert raw_call(g.h, pairs, bound=65536, out=False, recs=False)[0] == 0                 # the ceiling itself is accepted
    refused(None, pairs)
    rk = sharded.ShardRank((100_003, 200_003, 30_011, 2, 2, 2, 25, 0, 1, 0, 0, 9, 0), 0, 1, 0, "split")
    refused(rk.h, pairs)                                                                    # a shard handle
    rk.destroy()
    for destroy, gone in (("destroyCbf", N.CBF), ("destroyDbgbf", N.DBGBF), ("destroyRpkbf", N.RPKBF)):
        g2 = BloomFilterDeBruijnGraph(400_009, 800_011, 400_031, 2, 2, 2, 25, False, True)
        refused(g2.h, pairs)                                                                # no distance yet: d = -1
        g2.setReadPairedKmerDistance(30)
        g2.addReads(*w.packed, 3, storeReadPairedKmers=True)
        full = digests(g2.h)
        assert None not in full and 0 not in full
        g2.setReadPairedKmerDistance(1)
        refused(g2.h, pairs)                                                                # d < 2
        g2.setReadPairedKmerDistance(30)
        assert raw_call(g2.h, pairs)[0] == 0 and digests(g2.h) == full
        getattr(g2, destroy)()
        left = digests(g2.h)
        assert [d is None for d in left] == [f == gone for f in FILTERS]
        refused(g2.h, pairs)                                                                # the two filters that remain are as they were
        g2.destroy()
    g3 = BloomFilterDeBruijnGraph(100_003, 200_003, 30_011, 2, 2, 2, 25, False, False)      # made without read-paired k-mers
    g3.setReadPairedKmerDistance(30)
    refused(g3.h, pairs)
    g3.destroy()
    with pytest.raises(N.NativeError):
        g.joinPairs([b"ACGT" * 20], [b"ACGT" * 20], -3, 0.5, 1, 1.0)
    assert digests(g.h) == before


def test_profile_entry():
    w = J.world(25, True)
    g = device(w)
    g.profileEnable(True)
    run(g, w.pairs[:100], w.BOUND, w.GRAD, w.TIP, w.MIN_COV)
    prof = g.profileGet()
    assert prof["join"][0] > 0 and prof["join"][1] == 1, prof
    g.profileEnable(False)


@pytest.mark.parametrize("stranded", [False, True])
def test_overlap_and_connect_end_to_end(stranded):
    w = J.world(25, stranded)
    g = device(w)
    pairs = J.connect_pairs(w)
    got = graphutils.overlapAndConnect(g, [l for l, _ in pairs], [r for _, r in pairs], w.BOUND, 10, w.GRAD, w.TIP, w.MIN_COV)
    want = [J.restated_overlap_and_connect(w.o, l, r, w.BOUND, 10, w.GRAD, w.TIP, w.MIN_COV, w.d, w.k) for l, r in pairs]
    assert got == want
    assert {how for _, how in want} >= {"overlap", "join", "none", "not_judged"}


def java_join_pairs(g, lefts, rights, bound, grad, tip, min_cov, records):
    """BloomFilterDeBruijnGraph.joinPairs(String[], String[], int, float, int, float, int[]) as the Java class does it: text into two buffers,
    the size query, the call, 12 ints a record; strings or null back"""
    n = len(lefts)
    lo, ro = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    lo[1:], ro[1:] = np.cumsum([len(s) for s in lefts]), np.cumsum([len(s) for s in rights])
    lt, rt = np.frombuffer("".join(lefts).encode("latin1") + b"\0", np.uint8), np.frombuffer("".join(rights).encode("latin1") + b"\0", np.uint8)
    oo = np.zeros(n + 1, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = (g.h, p(lt), p(lo), p(rt), p(ro), n, bound, grad, tip, min_cov, p(oo))
    assert N.lib.rb_graph_join_pairs(*args, None, None) == 0
    out = np.zeros(max(int(oo[n]), 1), np.uint8)
    assert N.lib.rb_graph_join_pairs(*args, p(out), p(records)) == 0
    return [out[oo[i]:oo[i] + records[12 * i + 9]].tobytes().decode("latin1") if records[12 * i] == 1 else None for i in range(n)]


def test_java_shaped_join_pairs():
    w = J.world(25, False)
    g = device(w)
    pairs, want = w.pairs[-40:] + w.pairs[:40], w.want()[-40:] + w.want()[:40]
    records = np.zeros(12 * len(pairs), np.int32)
    got = java_join_pairs(g, [l.decode("latin1") for l, _ in pairs], [r.decode("latin1") for _, r in pairs], w.BOUND, w.GRAD, w.TIP, w.MIN_COV, records)
    assert got == [x.text.decode("latin1") if x.outcome == J.JOINED else None for x in want]
    for i, x in enumerate(want):
        assert tuple(records[12 * i:12 * i + 10]) == x.record()
        assert records[12 * i + 10:12 * i + 12].view(np.uint32).tolist() == [int(bits(x.l_thr)), int(bits(x.r_thr))]
