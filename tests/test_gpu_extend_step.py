"""rb_graph_extend_se (GraphUtils.extendRightSE / extendLeftSE on the device) and graphutils.extendSE against the reference's lines (restated in
tests/test_extend_step_rules.py) run on the CPU oracle, a device graph and the oracle built from the same reads through addReads with
storeReadPairedKmers.  Compared per sequence: every record field, the bases, and — as bits — counts and score.  Worlds: k = 25, stranded and
canonical, d = 30 (isoform forks at coverage 1:1, 1:3, 1:10, second forks fewer than d - 1 k-mers on, junctions of k - 1 shared letters,
tandem repeats, homopolymers, N in the last d k-mers and in the last k-mer, floors 1 / 2 / 5 / above every count inside one call); d = 2
and d = 3; d = 256 (the last distance whose walk rows live in LDS) and d = 300 (rows in device scratch); n = 1, 63, 64, 65; 20 003 sequences
in one call and in pieces; a 3000-base sequence; every refusal with the filters' digests before and after.  Each world first shows on the
oracle alone that every branch is reached (the rules file's reach check)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rnabloom import _native as N
from rnabloom import graphutils, sharded
from rnabloom.graph import BloomFilterDeBruijnGraph, _pack
import test_extend_step_rules as R

ERR_INVALID = 1                     # RB_ERR_INVALID
LDS_D = 256                         # the kernel's row: a larger distance keeps the walks' rows in device scratch
FILTERS = (N.DBGBF, N.CBF, N.RPKBF)
DEVICES = {}


@pytest.fixture(scope="module", autouse=True)
def release_the_device_graphs():
    """the worlds' device graphs are shared by the tests of this file and destroyed behind the last one"""
    yield
    for g in DEVICES.values():
        g.destroy()
    DEVICES.clear()


def device(w):
    """the device twin of a world's oracle graph: the same reads through addReads, the read-pair filter filled by the product path"""
    if id(w) not in DEVICES:
        g = BloomFilterDeBruijnGraph(*w.sizes, *w.hashes, w.k, w.stranded, True, rngSeed=5)
        g.setReadPairedKmerDistance(w.d)
        g.addReads(*w.packed, 3, storeReadPairedKmers=True)
        assert (g.exportFilter(N.DBGBF) == w.og.dbgbf_bytes()).all() and (g.exportFilter(N.CBF) == w.og.cbf_bytes()).all()
        assert (g.exportFilter(N.RPKBF) == w.og.rpkbf_bytes()).all()
        DEVICES[id(w)] = g
    return DEVICES[id(w)]


def run(g, queries, floors, direction):
    seq, off = _pack([s for s in queries])
    return g.extendStepSEFlat(seq, off, direction, np.asarray(floors, np.float32), counts=True)


def compare(w, g, label, take=None):
    """every query of the world (or the first `take` of each direction), direction by direction, against the restatement"""
    for direction in (0, 1):
        idx = [i for i, q in enumerate(w.queries) if q[2] == direction][:take]
        bases, recs, cnt = run(g, [w.queries[i][1] for i in idx], [w.floors[i] for i in idx], direction)
        assert bases.shape == (len(idx), w.d + 2)
        for j, i in enumerate(idx):
            st, rc = w.want()[i], recs[j]
            have = tuple(int(rc[f]) for f in ("outcome", "why", "n_candidates", "out_len", "pairs", "last_partnered", "winner"))
            assert have == st.record(), (label, direction, w.queries[i][0], have, st.record())
            n = st.out_len
            assert bases[j, :n].tobytes() == st.bases and not bases[j, n:].any(), (label, direction, w.queries[i][0])
            assert cnt[j, :n].view(np.uint32).tolist() == np.asarray(st.counts, np.float32).view(np.uint32).tolist() and not cnt[j, n:].any()
            assert np.float32(rc["score"]).view(np.uint32) == np.float32(st.score).view(np.uint32), (label, direction, w.queries[i][0], rc["score"], st.score)


@pytest.mark.parametrize("stranded", [False, True])
def test_steps_match_the_restatement_on_the_oracle(stranded):
    w = R.world(25, stranded)
    w.assert_every_branch_is_reached()
    g = device(w)
    before = [g.fold(f) for f in FILTERS]
    compare(w, g, ("d30", stranded))
    assert [g.fold(f) for f in FILTERS] == before                                          # read-only
    # the public form: strings, None where the reference returns null
    idx = [i for i, q in enumerate(w.queries) if q[2] == 0][:50]
    ext, recs = g.extendStepSE([w.queries[i][1].decode("latin1") for i in idx], 0, [w.floors[i] for i in idx])
    assert ext == [w.want()[i].bases if w.want()[i].outcome != R.NONE else None for i in idx] and len(recs) == len(idx)
    assert g.extendStepSE([], 1, 1.0)[0] == []


SMALL = {}


def small_world(d):
    """worlds for the edges of the mapping: reads long enough to hold pairs d apart"""
    if d not in SMALL:
        if d <= 3:
            SMALL[d] = R.World(25, False, seed=500 + d, d=d, n_iso=3)
        else:
            SMALL[d] = R.World(25, d % 2 == 1, seed=500 + d, d=d, n_iso=3, read_len=d + 150, tile=50, tx_len=2 * (d + 100))
    return SMALL[d]


@pytest.mark.parametrize("d", [2, 3, LDS_D, 300])
def test_edges_of_the_distance(d):
    w = small_world(d)
    outcomes = {st.outcome for st in w.want()}
    assert {R.NONE, R.SINGLE, R.FIRST} <= outcomes, outcomes
    if d > 3:
        assert R.SECOND in outcomes and any(st.out_len >= d - 1 for st in w.want())     # rows filled to their end
    g = device(w)
    compare(w, g, ("d", d))


@pytest.mark.parametrize("stranded", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sequence_counts_around_the_wavefront(n, stranded):
    """a call of n sequences in each direction: every record field, the bases, the counts and the score of each, the last workgroup's too"""
    w = R.world(25, stranded)
    assert min(sum(q[2] == direction for q in w.queries) for direction in (0, 1)) >= 65
    compare(w, device(w), ("n", n, stranded), take=n)


def test_twenty_thousand_sequences_and_small_pieces(monkeypatch):
    w = R.world(25, False)
    g = device(w)
    idx0 = [i for i, q in enumerate(w.queries) if q[2] == 0]
    idx = [idx0[i % len(idx0)] for i in range(20_003)]
    queries, floors = [w.queries[i][1] for i in idx], [w.floors[i] for i in idx]
    whole = run(g, queries, floors, 0)
    assert [int(r["outcome"]) for r in whole[1]] == [w.want()[i].outcome for i in idx]
    assert [int(r["out_len"]) for r in whole[1]] == [w.want()[i].out_len for i in idx]
    for piece in ("100000", "4099"):
        monkeypatch.setenv("RB_QUERY_PIECE", piece)
        got = run(g, queries, floors, 0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, whole)), piece
    monkeypatch.setenv("RB_QUERY_PIECE", "1")
    got = run(g, queries[:300], floors[:300], 0)
    assert all(a.tobytes() == b[:300].tobytes() for a, b in zip(got, whole))


def raw_call(g, queries, direction=0, floors=None, seq=True, off=True, fl=True, out=True, cnt=True, recs=True, offsets=None, d=30):
    s, o = _pack(queries)
    if offsets is not None:
        o = np.asarray(offsets, np.int64)
    n = len(o) - 1
    f = np.asarray(floors if floors is not None else [1.0] * n, np.float32)
    a_out = np.full(max(n, 1) * (d + 2), 7, np.uint8); a_cnt = np.full(max(n, 1) * (d + 2), 7, np.float32); a_rec = np.full(max(n, 1) * 8, 7, np.int32)
    p = lambda a, use: a.ctypes.data_as(C.c_void_p) if use else None
    rc = N.lib.rb_graph_extend_se(g, p(s, seq), p(o, off), n, direction, p(f, fl), p(a_out, out), p(a_cnt, cnt), p(a_rec, recs))
    return rc, a_out, a_cnt, a_rec


def digests(h):
    """rb_filter_fold of the three filters of a handle, None for one that is not there (destroyed, or never made)"""
    out = []
    for f in FILTERS:
        v = C.c_uint64()
        out.append(v.value if N.lib.rb_filter_fold(h, f, C.byref(v)) == 0 else None)
    return out


def refused(h, queries, **kw):
    """one refused call: RB_ERR_INVALID with a message, no output byte written, the handle's filters as they were"""
    before = digests(h) if h is not None else None
    r = raw_call(h, queries, **kw)
    assert r[0] == ERR_INVALID and N.lib.rb_last_error(), kw
    assert (r[1] == 7).all() and (r[2] == 7).all() and (r[3] == 7).all(), kw               # nothing was launched
    if h is not None:
        assert digests(h) == before and any(d is not None for d in before), kw


def test_refusals_leave_everything_alone():
    w = R.world(25, False)
    g = device(w)
    queries = [q[1] for q in w.queries if q[2] == 0][:40]
    before = digests(g.h)
    assert None not in before and 0 not in before
    untouched = lambda r: (r[1] == 7).all() and (r[2] == 7).all() and (r[3] == 7).all()
    assert raw_call(g.h, queries)[0] == 0 and raw_call(g.h, queries, cnt=False)[0] == 0
    r = raw_call(g.h, [])
    assert r[0] == 0 and untouched(r)                                                       # n == 0 touches nothing
    r = raw_call(g.h, [], seq=False, off=False, fl=False, out=False, cnt=False, recs=False)
    assert r[0] == 0
    assert digests(g.h) == before                                                           # the accepted calls are read-only too
    nq = len(queries)
    for kw in (dict(off=False), dict(fl=False), dict(out=False), dict(recs=False), dict(seq=False), dict(direction=2), dict(direction=-1),
               dict(floors=[1.0] * (nq - 1) + [float("nan")]), dict(floors=[float("inf")] + [1.0] * (nq - 1)), dict(floors=[-1.0] + [1.0] * (nq - 1)),
               dict(offsets=[0, 90, 40] + [40] * (nq - 2))):
        refused(g.h, queries, **kw)
    refused(None, queries)
    rk = sharded.ShardRank((100_003, 200_003, 30_011, 2, 2, 2, 25, 0, 1, 0, 0, 9, 0), 0, 1, 0, "split")
    refused(rk.h, queries)                                                                  # a shard handle
    rk.destroy()
    for destroy, gone in (("destroyCbf", N.CBF), ("destroyDbgbf", N.DBGBF), ("destroyRpkbf", N.RPKBF)):
        g2 = BloomFilterDeBruijnGraph(400_009, 800_011, 400_031, 2, 2, 2, 25, False, True)
        refused(g2.h, queries)                                                              # no distance yet: d = -1
        g2.setReadPairedKmerDistance(30)
        g2.addReads(*w.packed, 3, storeReadPairedKmers=True)
        full = digests(g2.h)
        assert None not in full and 0 not in full
        g2.setReadPairedKmerDistance(1)
        refused(g2.h, queries)                                                              # d < 2
        g2.setReadPairedKmerDistance(30)
        assert raw_call(g2.h, queries)[0] == 0 and digests(g2.h) == full
        getattr(g2, destroy)()
        left = digests(g2.h)
        assert [d is None for d in left] == [f == gone for f in FILTERS]
        refused(g2.h, queries)                                                              # the two filters that remain are as they were
        g2.destroy()
    g3 = BloomFilterDeBruijnGraph(100_003, 200_003, 30_011, 2, 2, 2, 25, False, False)      # made without read-paired k-mers
    g3.setReadPairedKmerDistance(30)
    refused(g3.h, queries)
    g3.destroy()
    with pytest.raises(N.NativeError):
        g.extendStepSE([b"ACGT" * 20], 3, 1.0)
    assert digests(g.h) == before


def test_profile_entry():
    w = R.world(25, True)
    g = device(w)
    g.profileEnable(True)
    run(g, [q[1] for q in w.queries if q[2] == 0], [1.0] * sum(q[2] == 0 for q in w.queries), 0)
    prof = g.profileGet()
    assert prof["extend_se"][0] > 0 and prof["extend_se"][1] == 1, prof
    g.profileEnable(False)


@pytest.mark.parametrize("stranded", [False, True])
def test_extend_se_driver_matches_the_restatement(stranded):
    """graphutils.extendSE (the step on the device, one call a round) against extendSE restated over the oracle: 200 sequences — seeds inside
    transcripts, before forks, inside the circular tandem repeats (the loop ends by usedKmers + hasDuplicatedKmerPair) and behind the
    stretches covered 150 times more (the floor has to fall twice)"""
    w = R.world(25, stranded)
    g = device(w)
    seeds = R.driver_seeds(w)
    trace = set()
    want = [R.extend_se(w.o, s, 1.0, w.d, w.k, trace=trace) for s in seeds]
    assert {"stopped_by_used", "floor_fell_twice"} <= trace, trace
    texts, ranges = graphutils.extendSE(g, seeds, 1.0)
    for i, (t, r) in enumerate(zip(texts, ranges)):
        assert (t, r) == want[i], (i, seeds[i], len(t), len(want[i][0]), r, want[i][1])
    with pytest.raises(RuntimeError):
        graphutils.extendSE(g, seeds[:20], 1.0, max_rounds=1)
