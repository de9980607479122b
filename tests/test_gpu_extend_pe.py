"""rb_graph_extend_pe (GraphUtils.extendRightPE / extendLeftPE on the device) and graphutils.extendPE against the reference's lines (restated in
tests/test_extend_pe_rules.py) run on the CPU oracle, a device graph and the oracle built from the same reads through addReads with
storeReadPairedKmers and the same fragments through addFragments with loadPairedKmers (k = 143: fragment by fragment, that path takes
k <= 64); all four filters are byte-equal before anything is compared.  Compared per sequence: every record field, the bases, and — as
bits — counts and score.  Worlds: k = 25, stranded and canonical, (d_r, d_f) = (30, 80) with floors 1 / 2 / 5 / above every count inside one call; the edges (2, 2), (2, 3), (30, 20) (the read distance above
the fragment distance), (30, 256) (the last rows in LDS) and (30, 300) (rows in device scratch); k = 143 with a 143-mer of 130 A in front of a
fork (isRepeat's byte counters); n = 1, 63, 64, 65; 20 003 sequences in one call and in pieces; every refusal with the filters' digests before
and after.  Each world first shows on the oracle alone that the branches it is there for are reached."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rnabloom import _native as N
from rnabloom import graphutils, sharded
from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch, _pack
import test_extend_step_rules as R
import test_extend_pe_rules as P

ERR_INVALID = 1                     # RB_ERR_INVALID
LDS_D = 256                         # the kernel's row: a larger fragment distance keeps the walks' rows in device scratch
FILTERS = (N.DBGBF, N.CBF, N.RPKBF, N.FPKBF)
FIELDS = ("outcome", "why", "n_candidates", "out_len", "read_pairs", "frag_pairs", "last_partnered", "winner", "max_ext")
DEVICES = {}


@pytest.fixture(scope="module", autouse=True)
def release_the_device_graphs():
    """the worlds' device graphs are shared by the tests of this file and destroyed behind the last one"""
    yield
    for g in DEVICES.values():
        g.destroy()
    DEVICES.clear()


def fill(g, w):
    """a world's reads and fragments through the product path"""
    g.setReadPairedKmerDistance(w.d_r)
    g.addReads(*w.packed, 3, storeReadPairedKmers=True)
    if w.extra_packed is not None:
        g.addReads(*w.extra_packed, 3, storeReadPairedKmers=True)
    g.initializePairKmersBloomFilter(w.FSIZE, w.frag_h)
    g.setFragPairedKmerDistance(w.d_f)
    if w.k > 64:
        # addFragments' paired-k-mer path takes k <= 64 only: fragment by fragment through the calls FragmentsToGraphWorker's steps map to
        for s in w.frags:
            _, f, r, _ = g.getKmers([s])
            g.addDbgOnly(f if w.stranded else np.where(r.view(np.int64) < f.view(np.int64), r, f))
            g.addReadPairedKmers(f, r)
            g.addFragmentPairKmers(f, r)
        return
    fseq, foff = _pack(w.frags)
    g.addFragments(ReadBatch.from_ascii(fseq, None, foff, 3), loadPairedKmers=True)


def device(w):
    """the device twin of a world's oracle graph; the four filters are the oracle's, byte for byte"""
    if id(w) not in DEVICES:
        g = BloomFilterDeBruijnGraph(*w.sizes, *w.hashes, w.k, w.stranded, True, rngSeed=5)
        fill(g, w)
        assert (g.exportFilter(N.DBGBF) == w.og.dbgbf_bytes()).all() and (g.exportFilter(N.CBF) == w.og.cbf_bytes()).all()
        assert (g.exportFilter(N.RPKBF) == w.og.rpkbf_bytes()).all() and (g.exportFilter(N.FPKBF) == w.og.fpkbf_bytes()).all()
        DEVICES[id(w)] = g
    return DEVICES[id(w)]


def run(g, queries, floors, direction):
    seq, off = _pack([s for s in queries])
    return g.extendStepPEFlat(seq, off, direction, np.asarray(floors, np.float32), counts=True)


def compare(w, g, label, take=None):
    """every query of the world (or the first `take` of each direction), direction by direction, against the restatement"""
    for direction in (0, 1):
        idx = [i for i, q in enumerate(w.queries) if q[2] == direction][:take]
        bases, recs, cnt = run(g, [w.queries[i][1] for i in idx], [w.floors[i] for i in idx], direction)
        assert bases.shape == (len(idx), w.d_f + 2)
        for j, i in enumerate(idx):
            st, rc = w.want()[i], recs[j]
            have = tuple(int(rc[f]) for f in FIELDS)
            assert have == st.record(), (label, direction, w.queries[i][0], have, st.record())
            n = st.out_len
            assert bases[j, :n].tobytes() == st.bases and not bases[j, n:].any(), (label, direction, w.queries[i][0])
            assert cnt[j, :n].view(np.uint32).tolist() == np.asarray(st.counts, np.float32).view(np.uint32).tolist() and not cnt[j, n:].any()
            assert np.float32(rc["score"]).view(np.uint32) == np.float32(st.score).view(np.uint32), (label, direction, w.queries[i][0], rc["score"], st.score)


@pytest.mark.parametrize("stranded", [False, True])
def test_steps_match_the_restatement_on_the_oracle(stranded):
    w = P.world(25, stranded)
    w.assert_every_branch_is_reached()
    g = device(w)
    before = [g.fold(f) for f in FILTERS]
    compare(w, g, ("30-80", stranded))
    assert [g.fold(f) for f in FILTERS] == before                                          # read-only
    # the public form: strings, None where the reference returns null
    idx = [i for i, q in enumerate(w.queries) if q[2] == 0][:50]
    ext, recs = g.extendStepPE([w.queries[i][1].decode("latin1") for i in idx], 0, [w.floors[i] for i in idx])
    assert ext == [w.want()[i].bases if w.want()[i].outcome != P.NONE else None for i in idx] and len(recs) == len(idx)
    assert g.extendStepPE([], 1, 1.0)[0] == []


SMALL = {}


def small_world(d_r, d_f):
    """worlds for the edges of the distances: transcripts long enough for walks of d_f k-mers behind a fork"""
    if (d_r, d_f) not in SMALL:
        kw = {} if d_f <= 80 else dict(tx_len=2 * (d_f + 100))
        SMALL[(d_r, d_f)] = P.WorldPE(25, d_f % 2 == 1, 900 + d_r + d_f, d_r, d_f, n_iso=3, **kw)
    return SMALL[(d_r, d_f)]


@pytest.mark.parametrize("d_r,d_f", [(2, 2), (2, 3), (30, 20), (30, LDS_D), (30, 300)])
def test_edges_of_the_distances(d_r, d_f):
    w = small_world(d_r, d_f)
    outcomes = {st.outcome for st in w.want()}
    assert {P.NONE, P.SINGLE, P.FIRST} <= outcomes, outcomes
    assert any(st.out_len >= d_f - 1 for st in w.want())                                     # rows filled to their end
    if d_f > 3:
        assert P.SECOND in outcomes
    compare(w, device(w), ("d", d_r, d_f))


def tail_143():
    """130 A and 13 C: no repeat for the reference, whose byte counters never reach t1 = 129 (tests/test_extend_pe_rules.py)"""
    km = bytearray(b"A" * 143)
    for p in range(5, 143, 11):
        km[p] = ord("C")
    return bytes(km)


def test_k_143_and_the_byte_counters():
    if "k143" not in SMALL:
        rng = np.random.default_rng(77)
        rnd = lambda n: np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()
        p = rnd(200) + tail_143()
        extra = [(p + rnd(300), 1, [("tail-fork", p), ("tail-fork-short", p[-(143 + 20):])]), (p + rnd(300), 2, [])]
        SMALL["k143"] = P.WorldPE(143, False, 1430, 30, 40, extra=extra, n_iso=2, read_len=400, tx_len=800)
    w = SMALL["k143"]
    assert not P.is_repeat(tail_143()) and P.is_repeat(tail_143(), byte_counters=False)
    tails = [st for st, q in zip(w.want(), w.queries) if q[0].startswith("tail-fork")]
    assert len(tails) == 4 and all(st.n_cand == 2 and st.max_ext == 38 for st in tails), [st.record() for st in tails]
    assert {P.NONE, P.SINGLE, P.FIRST} <= {st.outcome for st in w.want()}
    compare(w, device(w), "k143")


@pytest.mark.parametrize("stranded", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sequence_counts_around_the_wavefront(n, stranded):
    """a call of n sequences in each direction: every record field, the bases, the counts and the score of each, the last workgroup's too"""
    w = P.world(25, stranded)
    assert min(sum(q[2] == direction for q in w.queries) for direction in (0, 1)) >= 65
    compare(w, device(w), ("n", n, stranded), take=n)


def test_twenty_thousand_sequences_and_small_pieces(monkeypatch):
    w = P.world(25, False)
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


def raw_call(g, queries, direction=0, floors=None, seq=True, off=True, fl=True, out=True, cnt=True, recs=True, offsets=None, d=80):
    s, o = _pack(queries)
    if offsets is not None:
        o = np.asarray(offsets, np.int64)
    n = len(o) - 1
    f = np.asarray(floors if floors is not None else [1.0] * n, np.float32)
    a_out = np.full(max(n, 1) * (d + 2), 7, np.uint8); a_cnt = np.full(max(n, 1) * (d + 2), 7, np.float32); a_rec = np.full(max(n, 1) * 10, 7, np.int32)
    p = lambda a, use: a.ctypes.data_as(C.c_void_p) if use else None
    rc = N.lib.rb_graph_extend_pe(g, p(s, seq), p(o, off), n, direction, p(f, fl), p(a_out, out), p(a_cnt, cnt), p(a_rec, recs))
    return rc, a_out, a_cnt, a_rec


def digests(h):
    """rb_filter_fold of the four filters of a handle, None for one that is not there (destroyed, or never made)"""
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
    w = P.world(25, False)
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
    for destroy, gone in (("destroyCbf", N.CBF), ("destroyDbgbf", N.DBGBF), ("destroyRpkbf", N.RPKBF), ("destroyFpkbf", N.FPKBF)):
        g2 = BloomFilterDeBruijnGraph(*w.sizes, *w.hashes, 25, False, True, rngSeed=5)
        refused(g2.h, queries)                                                              # no distances, no fragment-pair filter yet
        g2.setReadPairedKmerDistance(w.d_r)
        refused(g2.h, queries)                                                              # a read distance, still no fragment-pair filter
        fill(g2, w)
        full = digests(g2.h)
        assert None not in full and 0 not in full
        g2.setReadPairedKmerDistance(1)
        refused(g2.h, queries)                                                              # d_r < 2
        g2.setReadPairedKmerDistance(w.d_r)
        g2.setFragPairedKmerDistance(1)
        refused(g2.h, queries)                                                              # d_f < 2
        g2.setFragPairedKmerDistance(w.d_f)
        assert raw_call(g2.h, queries)[0] == 0 and digests(g2.h) == full
        getattr(g2, destroy)()
        left = digests(g2.h)
        assert [d is None for d in left] == [f == gone for f in FILTERS]
        refused(g2.h, queries)                                                              # the three filters that remain are as they were
        g2.destroy()
    g3 = BloomFilterDeBruijnGraph(100_003, 200_003, 30_011, 2, 2, 2, 25, False, False)      # made without read-paired k-mers
    g3.setReadPairedKmerDistance(30)
    g3.initializePairKmersBloomFilter(30_011, 2)
    g3.setFragPairedKmerDistance(80)
    refused(g3.h, queries)
    g3.destroy()
    with pytest.raises(N.NativeError):
        g.extendStepPE([b"ACGT" * 20], 3, 1.0)
    assert digests(g.h) == before


def test_profile_entry():
    w = P.world(25, True)
    g = device(w)
    g.profileEnable(True)
    g.profileGet(reset=True)
    run(g, [q[1] for q in w.queries if q[2] == 0], [1.0] * sum(q[2] == 0 for q in w.queries), 0)
    prof = g.profileGet()
    assert prof["extend_pe"][0] > 0 and prof["extend_pe"][1] == 1 and "extend_se" not in prof, prof
    g.profileEnable(False)


@pytest.mark.parametrize("stranded", [False, True])
def test_extend_pe_driver_matches_the_restatement(stranded):
    """graphutils.extendPE (the step on the device, one call a round) against extendPE restated over the oracle: the 200 seeds of the rules
    file — inside transcripts, before forks, inside the circular tandem repeats (the loop ends by usedKmers + hasDuplicatedKmerPair) and
    behind the stretches covered 150 times more (the floor has to fall twice)"""
    w = P.world(25, stranded)
    g = device(w)
    seeds = P.driver_seeds(w)
    trace = set()
    want = [P.extend_pe(w.o, s, 1.0, w.d_r, w.d_f, w.k, trace=trace) for s in seeds]
    assert {"stopped_by_used", "floor_fell_twice"} <= trace, trace
    texts, ranges = graphutils.extendPE(g, seeds, 1.0)
    for i, (t, r) in enumerate(zip(texts, ranges)):
        assert (t, r) == want[i], (i, seeds[i], len(t), len(want[i][0]), r, want[i][1])
    with pytest.raises(RuntimeError):
        graphutils.extendPE(g, seeds[:20], 1.0, max_rounds=1)
