"""rb_graph_represented (GraphUtils.represented on the device) against the reference's lines restated in tests/test_represented_rules.py and
run on the CPU oracle.  A device graph and the oracle are built from the same reads through addReads, the gate — a
rnabloom.bloom.BloomFilter — and the oracle's gate from the same k-mers; all filters, the gate's included, are byte-equal before anything
is compared.  Compared per sequence: every one of the record's 12 ints.  Worlds: k = 25, stranded and canonical, at five settings of
(lookahead, max_indel, max_edge_clip, percent_identity); k = 143; hash counts 1 / 3 / 3.  The queries hold edges whose assembled text is 63,
64, 65, 128 and 129 letters (the alignment works 64 columns at a time) and one of 1021 k-mers and 1045 letters (the alignment row leaves
LDS, the edge walk passes the chimera screen's bound of 1000); n = 1, 63, 64, 65; 20 003 sequences in one call and in pieces; the budget
just below and just at one query's count; every refusal with the filters' digests before and after.  Each world first shows on the oracle
alone that the branches it is there for are reached."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rnabloom import _native as N
from rnabloom import sharded
from rnabloom.bloom import BloomFilter
from rnabloom.graph import BloomFilterDeBruijnGraph, _pack
import test_represented_rules as R

ERR_INVALID = 1                     # RB_ERR_INVALID
FILTERS = (N.DBGBF, N.CBF, N.RPKBF)
DEVICES = {}


@pytest.fixture(scope="module", autouse=True)
def release_the_device_graphs():
    """the worlds' device graphs and gates are shared by the tests of this file and destroyed behind the last one"""
    yield
    for g, bf in DEVICES.values():
        g.destroy(); bf.destroy()
    DEVICES.clear()


def device(w):
    """the device twins of a world's oracle graph and gate; every filter is the oracle's, byte for byte"""
    if id(w) not in DEVICES:
        g = BloomFilterDeBruijnGraph(*w.sizes, *w.hashes, w.k, w.stranded, True, rngSeed=5)
        g.setReadPairedKmerDistance(w.d)
        g.addReads(*w.packed, 3, storeReadPairedKmers=True)
        assert (g.exportFilter(N.DBGBF) == w.og.dbgbf_bytes()).all() and (g.exportFilter(N.CBF) == w.og.cbf_bytes()).all()
        assert (g.exportFilter(N.RPKBF) == w.og.rpkbf_bytes()).all()
        bf = BloomFilter(w.gate_size, w.gate_h, w.k)
        for s in w.gate_seqs:                                     # the assembled transcripts' k-mers, as the worker adds them
            _, f, r, _ = g.getKmers([s])
            bf.add(f if w.stranded else np.where(r.view(np.int64) < f.view(np.int64), r, f))
        assert (bf.toBytes() == w.gate_og.dbgbf_bytes()).all()
        DEVICES[id(w)] = (g, bf)
    return DEVICES[id(w)]


def folds(g, bf):
    return [g.fold(f) for f in FILTERS] + [bf._g.fold(N.DBGBF)]


def records(recs):
    return [tuple(int(rc[f]) for f in R.FIELDS) for rc in recs]


def compare(w, label, setting, take=None, max_visits=0):
    g, bf = device(w)
    queries = w.queries[:take]
    got = records(g.represented([s for _, s in queries], bf, *setting, max_visits))
    want = [st.record for st in w.judged(*setting, max_visits=max_visits)][:take]
    for (name, _), have, exp in zip(queries, got, want):
        assert have == exp, (label, name, have, exp)
    return got


@pytest.mark.parametrize("stranded", [False, True])
@pytest.mark.parametrize("setting", R.SETTINGS)
def test_records_match_the_restatement_on_the_oracle(stranded, setting):
    w = R.world(25, stranded)
    R.assert_every_branch_is_reached(w)
    g, bf = device(w)
    before = folds(g, bf)
    got = compare(w, (stranded, setting), setting)
    assert not any(r[0] & R.OVER_BUDGET for r in got)             # the default budget is far above every search of these worlds
    assert folds(g, bf) == before                                 # read-only on both handles


def test_k_143():
    compare(R.world_143(), "k143", (3, 1, 10, 0.9))


def test_other_hash_counts():
    compare(R.world_hashes(), "hashes", (3, 1, 40, 0.9))


@pytest.mark.parametrize("identity", [0.9, 1.0])
def test_alignment_rows_around_64_columns_and_beyond_lds(identity):
    """the edges of 63 .. 129 letters, and the one of 1021 k-mers whose row of 1045 columns lives in device scratch: the distance itself is
    on record where the identity test fails (1.0), its sum where it passes (0.9)"""
    w = R.world(25, False)
    g, bf = device(w)
    names = ["edge-%d-letters%s" % (n, m) for n in R.TILING for m in ("", "~")] + ["edge-long", "edge-long~"]
    want = w.named(3, 1, 10, identity)
    got = records(g.represented([w.queries[w.names.index(nm)][1] for nm in names], bf, 3, 1, 10, identity))
    for nm, have in zip(names, got):
        assert have == want[nm].record, (nm, have, want[nm].record)
        nk = R.LONG_EDGE if "long" in nm else int(nm.split("-")[1]) - w.k + 1
        changed = (nk - 1) // (w.k - 1) + 1                       # one changed letter every k - 1 letters: the distance
        if identity < 1.0:
            assert have[0] == R.REPRESENTED and have[7:9] == (1, changed), (nm, have)
        else:
            assert have[1] == (R.WHY_RIGHT_IDENTITY if nm.endswith("~") else R.WHY_LEFT_IDENTITY) and have[4:7] == (nk, nk, changed), (nm, have)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sequence_counts_around_the_wavefront(n):
    w = R.world(25, True)
    assert len(w.queries) >= 65
    compare(w, ("n", n), (3, 1, 10, 0.9), take=n)


def test_twenty_thousand_sequences_and_small_pieces(monkeypatch):
    w = R.world(25, False)
    g, bf = device(w)
    setting = (3, 1, 10, 0.9)
    short = [i for i, (_, s) in enumerate(w.queries) if len(s) < 400]
    idx = [short[i % len(short)] for i in range(20_003)]
    seq, off = _pack([w.queries[i][1] for i in idx])
    whole = g.representedFlat(seq, off, bf, *setting)
    want = w.judged(*setting)
    assert records(whole) == [want[i].record for i in idx]
    for piece in ("100000", "4099"):
        monkeypatch.setenv("RB_QUERY_PIECE", piece)
        assert g.representedFlat(seq, off, bf, *setting).tobytes() == whole.tobytes(), piece
    monkeypatch.setenv("RB_QUERY_PIECE", "1")
    assert g.representedFlat(seq[:off[300]], off[:301], bf, *setting).tobytes() == whole[:300].tobytes()


def test_the_budget_flips_exactly_one_query():
    w = R.world(25, False)
    setting = (3, 1, 40, 0.9)
    most = w.most_visits(*setting)
    base = compare(w, "budget-default", setting)
    at = compare(w, "budget-at", setting, max_visits=most)
    below = compare(w, "budget-below", setting, max_visits=most - 1)
    assert at == base
    flipped = [w.names[i] for i, (x, y) in enumerate(zip(below, base)) if x != y]
    assert flipped == ["edge-in-the-graph-deepest"]
    assert below[w.names.index("edge-in-the-graph-deepest")] == tuple(R.blank(R.OVER_BUDGET))


def raw_call(g, gate, queries, lookahead=3, max_indel=1, clip=10, identity=0.9, max_visits=0, seq=True, off=True, out=True, offsets=None):
    s, o = _pack(queries)
    if offsets is not None:
        o = np.asarray(offsets, np.int64)
    n = len(o) - 1
    a_rec = np.full(max(n, 1) * 12, 7, np.int32)
    p = lambda a, use: a.ctypes.data_as(C.c_void_p) if use else None
    rc = N.lib.rb_graph_represented(g, gate, p(s, seq), p(o, off), n, lookahead, max_indel, clip, identity, max_visits, p(a_rec, out))
    return rc, a_rec


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
    rc, rec = raw_call(h, gate, queries, **kw)
    assert rc == ERR_INVALID and N.lib.rb_last_error(), kw
    assert (rec == 7).all(), kw
    assert [digests(x) for x in handles] == before, kw


def test_refusals_leave_everything_alone():
    w = R.world(25, False)
    g, bf = device(w)
    queries = [s for _, s in w.queries][:40]
    nq = len(queries)
    before = folds(g, bf)
    assert raw_call(g.h, bf._g.h, queries)[0] == 0
    rc, rec = raw_call(g.h, bf._g.h, [])
    assert rc == 0 and (rec == 7).all()                           # n == 0 touches nothing
    assert raw_call(g.h, bf._g.h, [], seq=False, off=False, out=False)[0] == 0
    for kw in (dict(off=False), dict(out=False), dict(seq=False), dict(lookahead=17), dict(lookahead=-1), dict(max_indel=-1), dict(clip=-1),
               dict(clip=(1 << 20) + 1), dict(identity=float("nan")), dict(identity=float("inf")), dict(identity=float("-inf")), dict(max_visits=-1),
               dict(offsets=[0, 90, 40] + [40] * (nq - 2))):
        refused(g.h, bf._g.h, queries, **kw)
    refused(g.h, None, queries)                                   # the gate is required
    refused(None, bf._g.h, queries)
    other_k = BloomFilter(w.gate_size, w.gate_h, 27)
    refused(g.h, other_k._g.h, queries)                           # a gate with another k
    other_k.destroy()
    rk = sharded.ShardRank((100_003, 200_003, 30_011, 2, 2, 2, 25, 0, 1, 0, 0, 9, 0), 0, 1, 0, "split")
    refused(rk.h, bf._g.h, queries)                               # a shard handle as the graph
    refused(g.h, rk.h, queries)                                   # ... and as the gate
    rk.destroy()
    g2 = BloomFilterDeBruijnGraph(*w.sizes, *w.hashes, 25, False, True, rngSeed=5)
    g2.destroyCbf()
    refused(g2.h, bf._g.h, queries)
    g2.destroy()
    gone = BloomFilter(w.gate_size, w.gate_h, 25)
    gone._g.destroyDbgbf()
    refused(g.h, gone._g.h, queries)                              # a gate without its filter
    gone.destroy()
    with pytest.raises(N.NativeError):
        g.represented([b"ACGT" * 20], bf, 17, 1, 10, 0.9)
    assert folds(g, bf) == before
    assert g.represented([], bf, 3, 1, 10, 0.9).size == 0


def test_strings_and_the_profile_entry():
    w = R.world(25, True)
    g, bf = device(w)
    g.profileEnable(True)
    g.profileGet(reset=True)
    got = g.represented([s.decode("latin1") for _, s in w.queries[:50]], bf, 3, 1, 10, 0.9)
    prof = g.profileGet()
    g.profileEnable(False)
    assert prof["represented"][0] > 0 and prof["represented"][1] == 1, prof
    assert records(got) == [st.record for st in w.judged(3, 1, 10, 0.9)][:50]
    assert records(got) == records(g.represented([s for _, s in w.queries[:50]], bf, 3, 1, 10, 0.9))      # bytes as well
    assert got.dtype == g.REPR_DTYPE and g.REPR_DTYPE.itemsize == 48
    assert g.REPR_WHYS[R.WHY_PATH_IDENTITY] == "path_identity" and g.REPR_PATH_FORMS[R.PATH_SPLICED] == "spliced"
