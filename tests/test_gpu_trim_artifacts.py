"""rb_graph_trim_rc_artifacts (the three overloads of GraphUtils.trimReverseComplementArtifact on the device) against the reference's lines
restated in tests/test_trim_artifact_rules.py and run on the CPU oracle.  A device graph and the oracle are built from the same reads through
addReads; their filters are byte-equal before anything is compared.  Compared per sequence: every one of the record's 16 ints.  Worlds: k = 25,
stranded and canonical, under twelve settings of (mode, max_edge_clip, max_cov_gradient); k = 143; hash counts 1 / 3 / 3; the k = 64 world whose
k-mers all hash to 0.  The queries hold lists of 1, 2, 63, 64, 65, 128 and 129 k-mers (scans take 64 candidates at a time) and lists of 511,
512, 513 and 812 (the hash table leaves LDS above 512); n = 1, 63, 64, 65; 20 003 sequences, most of them without an artifact, in one call and
in pieces; every refusal with the filters' digests before and after.  The rules file shows on the oracle alone that the queries reach every
branch."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rnabloom import _native as N
from rnabloom import graphutils, sharded
from rnabloom.graph import BloomFilterDeBruijnGraph, _pack
import test_trim_artifact_rules as R

ERR_INVALID = 1                     # RB_ERR_INVALID
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
    """the device twin of a world's oracle graph; both filters are the oracle's, byte for byte"""
    if id(w) not in DEVICES:
        g = BloomFilterDeBruijnGraph(*w.sizes, *w.hashes, w.k, w.stranded, False, rngSeed=3)
        g.addReads(w.seq, None, w.off, 3)
        assert (g.exportFilter(N.DBGBF) == w.og.dbgbf_bytes()).all() and (g.exportFilter(N.CBF) == w.og.cbf_bytes()).all()
        DEVICES[id(w)] = g
    return DEVICES[id(w)]


def digests(h):
    out = []
    for f in FILTERS:
        v = C.c_uint64()
        out.append(v.value if N.lib.rb_filter_fold(h, f, C.byref(v)) == 0 else None)
    return out


def records(recs):
    return [[int(x) for x in np.frombuffer(rc.tobytes(), np.int32)] for rc in recs]


def compare(w, setting, take=None):
    g = device(w)
    queries = w.queries[:take]
    got = records(g.trimArtifacts([s for _, s in queries], *setting))
    want = [rec for rec, _ in w.judged(*setting)][:take]
    assert len(got) == len(want)
    for (name, _), have, exp in zip(queries, got, want):
        assert have == exp, (setting, name, have, exp)
    return got


@pytest.mark.parametrize("stranded", [False, True])
@pytest.mark.parametrize("setting", R.K25_SETTINGS)
def test_records_match_the_restatement_on_the_oracle(stranded, setting):
    w = R.world(25, stranded)
    R.assert_every_branch_is_reached(w)
    g = device(w)
    before = digests(g.h)
    got = compare(w, setting)
    assert any(not r[0] & R.FOUND for r in got) and (setting[1] < 10 and setting[0] != R.HASHES or any(r[0] & R.FOUND for r in got))
    assert digests(g.h) == before                                 # read-only


@pytest.mark.parametrize("stranded", [False, True])
def test_k_143(stranded):
    w = R.world(143, stranded)
    for setting in w.settings:
        got = compare(w, setting)
        assert any(r[0] & R.FOUND for r in got)


def test_other_hash_counts():
    w = R.world(25, False, (1, 3, 3))
    for setting in ((R.HASHES, 0, 0.0), (R.EDGE, 60, 0.0), (R.LONG, 30, 0.5)):
        compare(w, setting)


@pytest.mark.parametrize("stranded", [False, True])
def test_kmers_that_hash_alike(stranded):
    """k = 64: every k-mer of (AC)^n hashes to f = r = 0.  HASHES counts them all (the set holds the hash 0); EDGE and LONG reject on the bases
    every candidate that is no reverse complement"""
    w = R.world_hash_equal(stranded)
    for setting in w.settings:
        compare(w, setting)


@pytest.mark.parametrize("mode", [R.HASHES, R.EDGE, R.LONG])
def test_lists_around_64_candidates_and_around_the_lds_table(mode):
    w = R.world(25, True)
    g = device(w)
    setting = (mode, 10, 0.5)
    names = [nm for nm in w.names if nm.startswith("tile-")]
    assert {"tile-%d" % n for n in (1, 2, 63, 64, 65, 128, 129, R.LDS_LIST - 1, R.LDS_LIST, R.LDS_LIST + 1, R.LDS_LIST + 300)} <= set(names)
    want = dict(zip(w.names, w.judged(*setting)))
    got = records(g.trimArtifacts([dict(w.queries)[nm] for nm in names], *setting))
    for nm, have in zip(names, got):
        assert have == want[nm][0], (nm, have, want[nm][0])
        nk = int(nm.split("-")[1])
        assert 0 <= have[1] <= have[2] <= nk and not (nm.endswith("plain") and have[0] & R.FOUND), (nm, have)
    assert sum(1 for have in got if have[0] & R.FOUND) >= (7 if mode != R.LONG else 4)
    # one at a time: a table in device scratch that only this sequence sizes
    for nm in ("tile-%d" % (R.LDS_LIST + 1), "tile-%d" % R.LDS_LIST):
        assert records(g.trimArtifacts([dict(w.queries)[nm]], *setting)) == [want[nm][0]]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sequence_counts_around_the_wavefront(n):
    w = R.world(25, False)
    assert len(w.queries) >= 65
    for setting in ((R.HASHES, 0, 0.0), (R.EDGE, 10, 0.0), (R.LONG, 30, 0.5)):
        compare(w, setting, take=n)


@pytest.mark.parametrize("mode", [R.HASHES, R.EDGE, R.LONG])
def test_twenty_thousand_sequences_and_small_pieces(mode, monkeypatch):
    """20 003 sequences, nine in ten of them without an artifact, some without a k-mer or with an N"""
    w = R.world(25, False)
    g = device(w)
    setting = (mode, 60 if mode == R.EDGE else 30, 0.5)
    want = w.judged(*setting)
    short = [i for i, (_, s) in enumerate(w.queries) if len(s) < 400]
    dull = [i for i in short if not want[i][0][0] & R.FOUND]
    assert len(dull) >= 10 and len(short) - len(dull) >= 10
    idx = [short[(i // 10) % len(short)] if i % 10 == 0 else dull[i % len(dull)] for i in range(20_003)]
    seq, off = _pack([w.queries[i][1] for i in idx])
    whole = g.trimArtifactsFlat(seq, off, *setting)
    assert records(whole) == [want[i][0] for i in idx]
    for piece in ("100000", "4099"):
        monkeypatch.setenv("RB_QUERY_PIECE", piece)
        assert g.trimArtifactsFlat(seq, off, *setting).tobytes() == whole.tobytes(), piece
    monkeypatch.setenv("RB_QUERY_PIECE", "1")
    assert g.trimArtifactsFlat(seq[:off[300]], off[:301], *setting).tobytes() == whole[:300].tobytes()


def raw_call(g, queries, mode=R.EDGE, clip=10, grad=0.5, seq=True, off=True, out=True, offsets=None, n=None):
    s, o = _pack(queries)
    if offsets is not None:
        o = np.asarray(offsets, np.int64)
    n = len(o) - 1 if n is None else n
    a_rec = np.full(max(len(o) - 1, 1) * 16, 7, np.int32)
    p = lambda a, use: a.ctypes.data_as(C.c_void_p) if use else None
    rc = N.lib.rb_graph_trim_rc_artifacts(g, p(s, seq), p(o, off), n, mode, clip, grad, p(a_rec, out))
    return rc, a_rec


def refused(h, queries, also=(), **kw):
    """one refused call: RB_ERR_INVALID with a message, no output byte written, the handles' filters as they were"""
    handles = [x for x in (h,) + tuple(also) if x is not None]
    before = [digests(x) for x in handles]
    rc, rec = raw_call(h, queries, **kw)
    assert rc == ERR_INVALID and N.lib.rb_last_error(), kw
    assert (rec == 7).all(), kw
    assert [digests(x) for x in handles] == before, kw


def test_refusals_leave_everything_alone():
    w = R.world(25, False)
    g = device(w)
    queries = [s for _, s in w.queries][:40]
    nq = len(queries)
    before = digests(g.h)
    assert raw_call(g.h, queries)[0] == 0
    rc, rec = raw_call(g.h, [])
    assert rc == 0 and (rec == 7).all()                           # n == 0 touches nothing
    assert raw_call(g.h, [], seq=False, off=False, out=False)[0] == 0
    for kw in (dict(off=False), dict(out=False), dict(seq=False), dict(mode=3), dict(mode=-1), dict(clip=-1), dict(clip=(1 << 20) + 1),
               dict(grad=float("nan")), dict(grad=float("inf")), dict(grad=float("-inf")), dict(n=-1),
               dict(mode=R.HASHES, clip=-1), dict(mode=R.HASHES, grad=float("nan")),
               dict(offsets=[0, 90, 40] + [40] * (nq - 2))):
        refused(g.h, queries, **kw)
    refused(None, queries)
    long_text = np.full((1 << 24) + 25, ord("A"), np.uint8)       # 2^24 + 1 k-mers
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    o, rec = np.array([0, long_text.size], np.int64), np.full(16, 7, np.int32)
    assert N.lib.rb_graph_trim_rc_artifacts(g.h, p(long_text), p(o), 1, R.EDGE, 10, 0.5, p(rec)) == ERR_INVALID and (rec == 7).all()
    assert digests(g.h) == before
    rk = sharded.ShardRank((100_003, 200_003, 30_011, 2, 2, 2, 25, 0, 1, 0, 0, 9, 0), 0, 1, 0, "split")
    refused(rk.h, queries, also=(g.h,))                           # a shard handle
    rk.destroy()
    for gone in ("destroyCbf", "destroyDbgbf"):
        g2 = BloomFilterDeBruijnGraph(*w.sizes, *w.hashes, 25, False, False, rngSeed=3)
        getattr(g2, gone)()
        refused(g2.h, queries)
        g2.destroy()
    with pytest.raises(N.NativeError):
        g.trimArtifacts([b"ACGT" * 20], 3)
    assert digests(g.h) == before
    assert g.trimArtifacts([], R.EDGE, 10).size == 0
    # the modes ignore the values they do not read
    base = g.trimArtifacts(queries, R.HASHES).tobytes()
    assert g.trimArtifacts(queries, R.HASHES, 77, 3.5).tobytes() == base
    assert g.trimArtifacts(queries, R.EDGE, 10, 0.0).tobytes() == g.trimArtifacts(queries, R.EDGE, 10, 9.0).tobytes()


def test_strings_and_the_profile_entry():
    w = R.world(25, True)
    g = device(w)
    g.profileEnable(True)
    g.profileGet(reset=True)
    got = g.trimArtifacts([s.decode("latin1") for _, s in w.queries[:50]], R.EDGE, 10)
    prof = g.profileGet()
    g.profileEnable(False)
    assert prof["trim_artifacts"][0] > 0 and prof["trim_artifacts"][1] == 1, prof
    assert records(got) == [rec for rec, _ in w.judged(R.EDGE, 10, 0.0)][:50]
    assert got.dtype == g.TRIM_DTYPE and g.TRIM_DTYPE.itemsize == 64
    assert [int(x) for x in got["pass"]["why"][:, 0]] == [rec[4] for rec, _ in w.judged(R.EDGE, 10, 0.0)][:50]


@pytest.mark.parametrize("stranded", [False, True])
def test_graphutils_returns_the_strings_the_returned_kmers_spell(stranded):
    w = R.world(25, stranded)
    g = device(w)
    judged_ok = [i for i, (rec, _) in enumerate(w.judged(R.HASHES)) if not rec[0] & (R.BAD_LETTER | R.NO_KMER | R.NOT_JUDGED)]
    seqs = [w.queries[i][1] for i in judged_ok]
    for setting in ((R.HASHES, 0, 0.0), (R.EDGE, 60, 0.0), (R.LONG, 30, 0.5)):
        want = [w.judged(*setting)[i][1] for i in judged_ok]
        got = graphutils.trimReverseComplementArtifact(g, seqs, *setting)
        assert got == want, setting
        if setting[0] == R.HASHES:
            assert any(x is None for x in got) and any(x for x in got)
        if setting[0] == R.LONG and not stranded:
            assert b"" in got                                     # the empty list
    everything = [s for _, s in w.queries]
    with pytest.raises(ValueError):
        graphutils.trimReverseComplementArtifact(g, everything, R.EDGE, 10)
    kept = graphutils.trimReverseComplementArtifact(g, everything, R.EDGE, 10, keepNotJudged=True)
    assert kept == [text for _, text in w.judged(R.EDGE, 10, 0.0)]
    assert graphutils.trimReverseComplementArtifact(g, [s.decode() for s in seqs[:5]], R.EDGE, 60) == [t.decode() for t in
                                                                                                       [w.judged(R.EDGE, 60, 0.0)[i][1] for i in judged_ok[:5]]]
