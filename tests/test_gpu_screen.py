"""rb_graph_screen_fragments (GraphUtils.isBranchFree, isChimera and isBluntEndArtifact on the device) against the reference's lines restated in
tests/test_screen_rules.py and run on the CPU oracle.  A device graph and the oracle are built from the same reads through addReads, the
gate — a rnabloom.bloom.BloomFilter — and the oracle's gate from the same assembled transcripts; all filters, the gate's included, are
byte-equal before anything is compared.  Compared per sequence: every field of the record.  Worlds: k = 25, stranded and canonical,
lookahead 3 and 5, max_depth 0, 1, 2 and one above the longest unassembled tail; sequences of 1, 2, 3, 63, 64, 65 k-mers and of 5 000
bases; greedy walks that end at their bound of 1000 (a long assembled transcript, a tandem repeat); k = 143; hash counts 1 / 3 / 3;
n = 1, 63, 64, 65; 20 003 sequences in one call and in pieces; every single screen on its own; the budget just below and just at one
query's count; every refusal with the filters' digests before and after.  The kernel keeps no per-k-mer row in LDS (its rows are device
scratch whatever the length), so there is no row capacity to test around.  Each world first shows on the oracle alone that the branches
it is there for are reached."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rnabloom import _native as N
from rnabloom import sharded
from rnabloom.bloom import BloomFilter
from rnabloom.graph import BloomFilterDeBruijnGraph, _pack
import test_screen_rules as S

ERR_INVALID = 1                     # RB_ERR_INVALID
FILTERS = (N.DBGBF, N.CBF, N.RPKBF)
FIELDS = ("flags", "chim_why", "break_i", "break_j", "right_len", "left_len", "blunt_why", "boundary")
DEEP = S.ScreenWorld.LONGEST_TAIL + 16
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
    return [tuple(int(rc[f]) for f in FIELDS) for rc in recs]


def compare(w, label, lookahead, max_depth, what=7, take=None, max_visits=0):
    g, bf = device(w)
    queries = w.queries[:take]
    got = records(g.screenFragments([s for _, s in queries], bf, what, lookahead, max_depth, max_visits))
    want = [st.record for st in w.want(lookahead, max_depth, what, max_visits)][:take]
    for (name, _), have, exp in zip(queries, got, want):
        assert have == exp, (label, name, have, exp)
    return got


@pytest.mark.parametrize("stranded", [False, True])
@pytest.mark.parametrize("lookahead,max_depth", [(3, 2), (5, 1), (3, DEEP), (5, 0)])
def test_records_match_the_restatement_on_the_oracle(stranded, lookahead, max_depth):
    w = S.world(25, stranded)
    w.assert_every_branch_is_reached(3, 2)
    g, bf = device(w)
    before = folds(g, bf)
    got = compare(w, (stranded, lookahead, max_depth), lookahead, max_depth)
    assert not any(r[0] & S.OVER_BUDGET for r in got)             # the default budget is far above every search of these worlds
    assert folds(g, bf) == before                                 # read-only on both handles


@pytest.mark.parametrize("what", [1, 2, 4, 3, 6])
def test_every_screen_on_its_own(what):
    w = S.world(25, False)
    got = compare(w, ("what", what), 3, 2, what=what)
    for r in got:
        if not what & 2:
            assert r[1:6] == (0, -1, -1, 0, 0) and not r[0] & 2
        if not what & 4:
            assert r[6:] == (0, -1) and not r[0] & (4 | S.OVER_BUDGET)
        if not what & 1:
            assert not r[0] & 1
    if what == 1:                                                 # the branch-free screen alone needs no gate
        g, _ = device(w)
        assert records(g.screenFragments([s for _, s in w.queries], None, 1, 3, 2)) == got


def test_k_143():
    w = S.world_143()
    compare(w, "k143", 3, 2)


def test_other_hash_counts():
    w = S.world_hashes()
    compare(w, "hashes", 3, 2)
    compare(w, "hashes", 5, DEEP)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sequence_counts_around_the_wavefront(n):
    w = S.world(25, True)
    assert len(w.queries) >= 65
    compare(w, ("n", n), 3, 2, take=n)


def test_twenty_thousand_sequences_and_small_pieces(monkeypatch):
    w = S.world(25, False)
    g, bf = device(w)
    short = [i for i, (_, s) in enumerate(w.queries) if len(s) < 400]
    idx = [short[i % len(short)] for i in range(20_003)]
    seq, off = _pack([w.queries[i][1] for i in idx])
    whole = g.screenFragmentsFlat(seq, off, bf, 7, 3, 2)
    want = w.want(3, 2)
    assert records(whole) == [want[i].record for i in idx]
    for piece in ("100000", "4099"):
        monkeypatch.setenv("RB_QUERY_PIECE", piece)
        assert g.screenFragmentsFlat(seq, off, bf, 7, 3, 2).tobytes() == whole.tobytes(), piece
    monkeypatch.setenv("RB_QUERY_PIECE", "1")
    assert g.screenFragmentsFlat(seq[:off[300]], off[:301], bf, 7, 3, 2).tobytes() == whole[:300].tobytes()


def test_the_budget_flips_exactly_one_query():
    w = S.world(25, False)
    most = w.largest_visit_count(3, 2)
    base = compare(w, "budget-default", 3, 2)
    at = compare(w, "budget-at", 3, 2, max_visits=most)
    below = compare(w, "budget-below", 3, 2, max_visits=most - 1)
    assert at == base
    flipped = [w.names[i] for i, (x, y) in enumerate(zip(below, base)) if x != y]
    assert flipped == ["blunt-longest-tail"]
    r = below[w.names.index("blunt-longest-tail")]
    assert r[0] & S.OVER_BUDGET and not r[0] & S.BLUNT_END and r[6] == 0


def raw_call(g, gate, queries, what=7, lookahead=3, max_depth=2, max_visits=0, seq=True, off=True, out=True, offsets=None):
    s, o = _pack(queries)
    if offsets is not None:
        o = np.asarray(offsets, np.int64)
    n = len(o) - 1
    a_rec = np.full(max(n, 1) * 8, 7, np.int32)
    p = lambda a, use: a.ctypes.data_as(C.c_void_p) if use else None
    rc = N.lib.rb_graph_screen_fragments(g, gate, p(s, seq), p(o, off), n, what, lookahead, max_depth, max_visits, p(a_rec, out))
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
    w = S.world(25, False)
    g, bf = device(w)
    queries = [s for _, s in w.queries][:40]
    nq = len(queries)
    before = folds(g, bf)
    assert raw_call(g.h, bf._g.h, queries)[0] == 0 and raw_call(g.h, None, queries, what=1)[0] == 0
    rc, rec = raw_call(g.h, bf._g.h, [])
    assert rc == 0 and (rec == 7).all()                           # n == 0 touches nothing
    assert raw_call(g.h, bf._g.h, [], seq=False, off=False, out=False)[0] == 0
    for kw in (dict(off=False), dict(out=False), dict(seq=False), dict(what=0), dict(what=8), dict(what=-1), dict(lookahead=17), dict(lookahead=-1),
               dict(max_visits=-1), dict(max_depth=(1 << 20) + 1), dict(offsets=[0, 90, 40] + [40] * (nq - 2))):
        refused(g.h, bf._g.h, queries, **kw)
    for what in (2, 4, 6, 7):
        refused(g.h, None, queries, what=what)                    # the chimera and the blunt-end screen need the gate
    refused(None, bf._g.h, queries)
    other_k = BloomFilter(w.gate_size, w.gate_h, 27)
    refused(g.h, other_k._g.h, queries)                           # a gate with another k
    refused(g.h, other_k._g.h, queries, what=1)                   # ... also where the screen would not read it
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
        g.screenFragments([b"ACGT" * 20], bf, 7, 17, 2)
    assert folds(g, bf) == before
    assert g.screenFragments([], bf, 7, 3, 2).size == 0


def test_strings_and_the_profile_entry():
    w = S.world(25, True)
    g, bf = device(w)
    g.profileEnable(True)
    g.profileGet(reset=True)
    got = g.screenFragments([s.decode("latin1") for _, s in w.queries[:50]], bf, 7, 3, 2)
    prof = g.profileGet()
    g.profileEnable(False)
    assert prof["screen_fragments"][0] > 0 and prof["screen_fragments"][1] == 1, prof
    assert records(got) == [st.record for st in w.want(3, 2)][:50]
    assert got.dtype == g.SCREEN_DTYPE and g.CHIM_WHYS[S.CHIM_DISJOINT] == "disjoint" and g.BLUNT_WHYS[S.BLUNT_RIGHT_ARTIFACT] == "right_artifact"
