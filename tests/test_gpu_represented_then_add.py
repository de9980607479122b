"""rb_graph_represented_then_add (the in-order loop of TranscriptWriter.write and GraphUtils.reduceRedundancy on the device) against the
reference's loop restated in tests/represented_then_add_worlds.py and run on the CPU oracle.  The device graph is the world's twin, built as
in tests/test_gpu_represented.py; every test takes a FRESH device gate, since the call writes it.  Compared: all 12 ints of every record,
keep, median as bits, n_done, and the gate's bytes afterwards; the graph's three filters keep their digests.  The duplicates and the orders
fail for any implementation that judges against a snapshot of the gate: they hold the kernel's visibility rule."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rnabloom import _native as N
from rnabloom import graphutils, sharded
from rnabloom.bloom import BloomFilter
from rnabloom.graph import BloomFilterDeBruijnGraph, _pack
import represented_then_add_worlds as W
import test_represented_rules as R

ERR_INVALID = 1                     # RB_ERR_INVALID
FILTERS = (N.DBGBF, N.CBF, N.RPKBF)
GRAPHS = {}


@pytest.fixture(scope="module", autouse=True)
def release_the_device_graphs():
    yield
    for g, _ in GRAPHS.values():
        g.destroy()
    GRAPHS.clear()


def device(w):
    """the device twin of a world's oracle graph, and the bytes of its gate built on the device as the worker builds it"""
    if id(w) not in GRAPHS:
        g = BloomFilterDeBruijnGraph(*w.sizes, *w.hashes, w.k, w.stranded, True, rngSeed=5)
        g.setReadPairedKmerDistance(w.d)
        g.addReads(*w.packed, 3, storeReadPairedKmers=True)
        assert (g.exportFilter(N.DBGBF) == w.og.dbgbf_bytes()).all() and (g.exportFilter(N.CBF) == w.og.cbf_bytes()).all()
        assert (g.exportFilter(N.RPKBF) == w.og.rpkbf_bytes()).all()
        bf = BloomFilter(w.gate_size, w.gate_h, w.k)
        for s in w.gate_seqs:
            _, f, r, _ = g.getKmers([s])
            bf.add(f if w.stranded else np.where(r.view(np.int64) < f.view(np.int64), r, f))
        gate_bytes = bf.toBytes().copy()
        bf.destroy()
        assert (gate_bytes == w.gate_og.dbgbf_bytes()).all()
        GRAPHS[id(w)] = (g, gate_bytes)
    return GRAPHS[id(w)]


class fresh_gate:
    """a device gate of the world's size: the world's (`world`) or an empty one; destroyed behind the test"""

    def __init__(self, w, start):
        self.w, self.start = w, start

    def __enter__(self):
        g, gate_bytes = device(self.w)
        self.bf = BloomFilter(self.w.gate_size, self.w.gate_h, self.w.k)
        if self.start == "world":
            self.bf.fromBytes(gate_bytes)
        return g, self.bf

    def __exit__(self, *exc):
        self.bf.destroy()


def folds(g):
    return [g.fold(f) for f in FILTERS]


def records(recs):
    return [tuple(int(rc[f]) for f in R.FIELDS) for rc in recs]


def same(label, got, want, names=None):
    """a device call's (records, keep, median, n_done) against a Walked"""
    recs, keep, median, done = got
    for i, (have, exp) in enumerate(zip(records(recs), want.records)):
        assert have == exp, (label, i if names is None else names[i], have, exp)
    assert len(recs) == len(want.records) and keep.tolist() == want.keep, label
    assert median.view(np.uint32).tolist() == want.median.view(np.uint32).tolist(), label
    assert done == want.n_done, label


@pytest.mark.parametrize("start", ["world", "empty"])
@pytest.mark.parametrize("order", ["list", "reverse", "length"])
@pytest.mark.parametrize("stranded", [False, True])
def test_everything_matches_the_restated_loop(stranded, order, start):
    w = R.world(25, stranded)
    want = W.walked(w, start, order, W.BASE)
    with fresh_gate(w, start) as (g, bf):
        before = folds(g)
        got = g.representedThenAdd(W.ordered([s for _, s in w.queries], order), bf, *W.BASE)
        same((stranded, order, start), got, want)
        assert (bf.toBytes() == want.gate_bytes()).all()
        assert folds(g) == before                                 # the graph is read-only
    assert 0 < sum(want.keep) < len(want.keep) and want.n_done == len(want.keep)


@pytest.mark.parametrize("which", ["hashes", "k143"])
def test_other_hash_counts_and_k_143(which):
    w, setting = (R.world_hashes(), W.CLIP40) if which == "hashes" else (R.world_143(), W.BASE)
    want = W.walked(w, "world", "list", setting)
    with fresh_gate(w, "world") as (g, bf):
        same(which, g.representedThenAdd([s for _, s in w.queries], bf, *setting), want, w.names)
        assert (bf.toBytes() == want.gate_bytes()).all()


def test_the_hand_made_list():
    w = R.world(25, False)
    hm = W.hand_made(w)
    want = W.walked(w, "empty", "list", W.BASE, seqs=[s for _, s, _, _ in hm], tag="hand-made")
    with fresh_gate(w, "empty") as (g, bf):
        got = g.representedThenAdd([s for _, s, _, _ in hm], bf, *W.BASE)
        same("hand-made", got, want, [what for what, _, _, _ in hm])
        for (what, _, flags, why), rec, keep in zip(hm, records(got[0]), got[1]):
            assert rec[0] == flags and (why is None or rec[1] == why) and keep == (flags == 0), (what, rec)
        assert (bf.toBytes() == want.gate_bytes()).all()


def test_a_sequence_directly_behind_itself_is_represented():
    """the second copy reads the bits the first one set a moment earlier: the visibility rule.  (A sequence of fewer k-mers than the lookahead
    of 3 is its own exception in the reference: a run that short never counts, so it is kept again — R/util/GraphUtils.java:742.)"""
    w = R.world(25, False)
    doubled = [s for _, s in w.queries for _ in (0, 1)]
    want = W.walked(w, "empty", "list", W.BASE, seqs=doubled, tag="doubled")
    with fresh_gate(w, "empty") as (g, bf):
        got = g.representedThenAdd(doubled, bf, *W.BASE)
        same("doubled", got, want)
        recs = records(got[0])
        for i in range(0, len(doubled), 2):
            first, second = recs[i], recs[i + 1]
            if first[0] & (R.NO_KMER | R.BAD_LETTER) or len(doubled[i]) - w.k + 1 < W.BASE[0]:
                assert second == first and got[1][i + 1] == got[1][i]
            else:
                assert second[:2] == (R.REPRESENTED, R.WHY_TRUE) and not got[1][i + 1], (w.names[i // 2], first, second)
        assert (bf.toBytes() == want.gate_bytes()).all()
    assert sum(want.keep) >= 40


@pytest.mark.parametrize("nk", [1, 63, 64, 65, 1023, 1024, 1025])
def test_fill_and_add_strides(nk):
    """k-mer counts around the wavefront's and the workgroup's width: the fill (every call) and the add (the first copy, from an empty gate)"""
    w = R.world(25, False)
    big = w.tx[6][0]
    s = big[7:7 + nk + w.k - 1]
    assert len(s) == nk + w.k - 1
    want = W.walked(w, "empty", "list", W.BASE, seqs=[s, s], tag=("stride", nk))
    assert want.keep == ([1, 0] if nk >= W.BASE[0] else [1, 1])   # (a run shorter than the lookahead never counts: kept again)
    with fresh_gate(w, "empty") as (g, bf):
        same(("stride", nk), g.representedThenAdd([s, s], bf, *W.BASE), want)
        assert (bf.toBytes() == want.gate_bytes()).all()


def test_cuts_of_the_list_and_pieces(monkeypatch):
    """the gate carries the state: one call, three calls and every size of piece leave the restatement's records, keep flags and gate bytes"""
    w = R.world(25, False)
    seqs = [s for _, s in w.queries]
    want = W.walked(w, "world", "list", W.BASE)
    with fresh_gate(w, "world") as (g, bf):
        parts = [g.representedThenAdd(seqs[a:b], bf, *W.BASE) for a, b in ((0, 37), (37, 38), (38, len(seqs)))]
        got = tuple(np.concatenate([p[j] for p in parts]) for j in range(3)) + (sum(p[3] for p in parts),)
        same("three calls", got, want, w.names)
        assert (bf.toBytes() == want.gate_bytes()).all()
    for piece in ("100000", "4099", "1"):
        monkeypatch.setenv("RB_QUERY_PIECE", piece)
        with fresh_gate(w, "world") as (g, bf):
            same(("piece", piece), g.representedThenAdd(seqs, bf, *W.BASE), want, w.names)
            assert (bf.toBytes() == want.gate_bytes()).all(), piece


def test_the_composed_route_agrees():
    w = R.world(25, False)
    seqs = [s for _, s in w.queries]
    want = W.walked(w, "world", "list", W.BASE)
    with fresh_gate(w, "world") as (g, bf):
        recs, keep, done = graphutils.representedThenAddComposed(g, bf, seqs, *W.BASE)
        assert records(recs) == want.records and keep.tolist() == want.keep and done == want.n_done
        assert (bf.toBytes() == want.gate_bytes()).all()


def test_the_walk_stops_at_a_sequence_over_its_budget_and_resumes_behind_it():
    w = R.world(25, False)
    seqs, budget, p = W.stop_case(w)
    stopped = W.walked(w, "world", "list", W.CLIP40, max_visits=budget, seqs=seqs, tag="stop")
    left_out = W.walked(w, "world", "list", W.CLIP40, seqs=seqs[:p] + seqs[p + 1:], tag="stop-left-out")
    assert stopped.n_done == p and 0 < p < len(seqs) - 1
    with fresh_gate(w, "world") as (g, bf):
        got = g.representedThenAdd(seqs, bf, *W.CLIP40, budget)
        same("stopped", got, stopped)
        assert records(got[0])[p] == tuple(R.blank(R.OVER_BUDGET))
        assert all(r == tuple(R.blank(N.SCREEN_NOT_REACHED)) for r in records(got[0])[p + 1:])
        assert (bf.toBytes() == stopped.gate_bytes()).all()       # no k-mer of a sequence at or behind the stop
        # the caller leaves the stopped sequence out and goes on with the default budget
        recs, keep, median, done = g.representedThenAdd(seqs[p + 1:], bf, *W.CLIP40)
        assert records(recs) == left_out.records[p:] and keep.tolist() == left_out.keep[p:] and done == len(seqs) - p - 1
        assert median.view(np.uint32).tolist() == left_out.median[p:].view(np.uint32).tolist()
        assert (bf.toBytes() == left_out.gate_bytes()).all()
    # graphutils.writeTranscripts does the same with its default decision
    with fresh_gate(w, "world") as (g, bf):
        kept, recs = graphutils.writeTranscripts(g, bf, seqs, *W.CLIP40, maxVisits=budget, decide=lambda i, s: False)
        want_idx = [i + (i >= p) for i in np.flatnonzero(left_out.keep)]
        assert [i for i, _, _ in kept] == want_idx
        assert records(recs)[:p] == left_out.records[:p] and records(recs)[p] == tuple(R.blank(R.OVER_BUDGET))
        assert (bf.toBytes() == left_out.gate_bytes()).all()


POISON = 7


def raw_call(g, gate, queries, lookahead=3, max_indel=1, clip=10, identity=0.9, max_visits=0, seq=True, off=True, out=True, keep=True, median=True,
             done=True, offsets=None):
    s, o = _pack(queries)
    if offsets is not None:
        o = np.asarray(offsets, np.int64)
    n = len(o) - 1
    a_rec = np.full(max(n, 1) * 12, POISON, np.int32)
    a_keep = np.full(max(n, 1), POISON, np.uint8)
    a_med = np.full(max(n, 1), POISON, np.float32)
    a_done = np.full(1, POISON, np.int64)
    p = lambda a, use: a.ctypes.data_as(C.c_void_p) if use else None
    rc = N.lib.rb_graph_represented_then_add(g, gate, p(s, seq), p(o, off), n, lookahead, max_indel, clip, identity, max_visits, p(a_rec, out),
                                             p(a_keep, keep), p(a_med, median), p(a_done, done))
    return rc, (a_rec, a_keep, a_med, a_done)


def digests(h):
    out = []
    for f in FILTERS:
        v = C.c_uint64()
        out.append(v.value if N.lib.rb_filter_fold(h, f, C.byref(v)) == 0 else None)
    return out


def refused(h, gate, queries, also=(), **kw):
    """one refused call: RB_ERR_INVALID with a message, no output byte written, the handles' filters as they were"""
    handles = [x for x in (h, gate) + tuple(also) if x is not None]
    before = [digests(x) for x in handles]
    rc, outs = raw_call(h, gate, queries, **kw)
    assert rc == ERR_INVALID and N.lib.rb_last_error(), kw
    assert all((a == POISON).all() for a in outs), kw
    assert [digests(x) for x in handles] == before, kw


def test_refusals_leave_everything_alone():
    w = R.world(25, False)
    queries = [s for _, s in w.queries][:40]
    nq = len(queries)
    with fresh_gate(w, "world") as (g, bf):
        before = folds(g) + [bf._g.fold(N.DBGBF)]
        rc, outs = raw_call(g.h, bf._g.h, [])
        assert rc == 0 and all((a == POISON).all() for a in outs)   # n == 0 touches nothing
        assert raw_call(g.h, bf._g.h, [], seq=False, off=False, out=False, keep=False, median=False, done=False)[0] == 0
        for kw in (dict(off=False), dict(out=False), dict(seq=False), dict(lookahead=17), dict(lookahead=-1), dict(max_indel=-1), dict(clip=-1),
                   dict(clip=(1 << 20) + 1), dict(identity=float("nan")), dict(identity=float("inf")), dict(identity=float("-inf")), dict(max_visits=-1),
                   dict(offsets=[0, 90, 40] + [40] * (nq - 2)), dict(keep=False), dict(done=False)):
            refused(g.h, bf._g.h, queries, **kw)
        refused(g.h, None, queries)                               # the gate is required
        refused(None, bf._g.h, queries)
        refused(g.h, g.h, queries)                                # the gate is written, the graph is read: two handles
        other_k = BloomFilter(w.gate_size, w.gate_h, 27)
        refused(g.h, other_k._g.h, queries)                       # a gate with another k
        other_k.destroy()
        rk = sharded.ShardRank((100_003, 200_003, 30_011, 2, 2, 2, 25, 0, 1, 0, 0, 9, 0), 0, 1, 0, "split")
        refused(rk.h, bf._g.h, queries)                           # a shard handle as the graph
        refused(g.h, rk.h, queries)                               # ... and as the gate
        rk.destroy()
        g2 = BloomFilterDeBruijnGraph(*w.sizes, *w.hashes, 25, False, True, rngSeed=5)
        g2.destroyCbf()
        refused(g2.h, bf._g.h, queries)
        g2.destroy()
        gone = BloomFilter(w.gate_size, w.gate_h, 25)
        gone._g.destroyDbgbf()
        refused(g.h, gone._g.h, queries)                          # a gate without its filter
        gone.destroy()
        with pytest.raises(N.NativeError):
            g.representedThenAdd([b"ACGT" * 20], bf, 17, 1, 10, 0.9)
        assert folds(g) + [bf._g.fold(N.DBGBF)] == before
        recs, keep, median, done = g.representedThenAdd([], bf, *W.BASE)
        assert recs.size == 0 and keep.size == 0 and done == 0
        # a null median is allowed
        rc, (a_rec, a_keep, a_med, a_done) = raw_call(g.h, bf._g.h, queries, median=False)
        want = W.walked(w, "world", "list", W.BASE)
        assert rc == 0 and (a_med == POISON).all() and a_done[0] == nq and a_keep.tolist() == want.keep[:nq]


def test_strings_bytes_and_the_profile_entry():
    w = R.world(25, True)
    want = W.walked(w, "world", "list", W.BASE)
    with fresh_gate(w, "world") as (g, bf):
        g.profileEnable(True)
        g.profileGet(reset=True)
        got = g.representedThenAdd([s.decode("latin1") for _, s in w.queries], bf, *W.BASE)
        prof = g.profileGet()
        g.profileEnable(False)
        assert prof["represented_then_add"][0] > 0 and prof["represented_then_add"][1] == 1, prof
        same("strings", got, want, w.names)
        assert got[0].dtype == g.REPR_DTYPE and got[1].dtype == np.uint8 and got[2].dtype == np.float32
        assert g.SCREEN_NOT_REACHED == 64 and not g.SCREEN_NOT_REACHED & (g.SCREEN_NOT_JUDGED | g.REPR_REPRESENTED)


def test_reduce_redundancy_and_write_transcripts():
    w = R.world(25, False)
    seqs = [s for _, s in w.queries]
    shuffled = [seqs[i] for i in np.random.default_rng(7).permutation(len(seqs))]
    want = W.walked(w, "world", "length", W.BASE, seqs=shuffled, tag="shuffled")
    by_length = W.ordered(shuffled, "length")
    with fresh_gate(w, "world") as (g, bf):
        kept, removed = graphutils.reduceRedundancy(g, bf, shuffled, *W.BASE)
        exp = [by_length[i] for i in np.flatnonzero(want.keep)]
        assert [s for _, _, s in kept] == exp and [(cid, l) for cid, l, _ in kept] == [(j + 1, len(s)) for j, s in enumerate(exp)]
        assert removed == len(seqs) - len(exp) and (bf.toBytes() == want.gate_bytes()).all()
    want = W.walked(w, "world", "list", W.BASE)
    with fresh_gate(w, "world") as (g, bf):
        kept, recs = graphutils.writeTranscripts(g, bf, seqs, *W.BASE)
        assert kept == [(int(i), len(seqs[i]), "%.1f" % float(want.median[i])) for i in np.flatnonzero(want.keep)]
        assert records(recs) == want.records and (bf.toBytes() == want.gate_bytes()).all()
