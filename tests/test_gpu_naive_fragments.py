"""rb_graph_naive_extend_fragments (GraphUtils.naiveExtend, R/util/GraphUtils.java:6935-6957) and graphutils.finishFragments (R/RNABloom.java:2182-2268)
on the device against their restatements over the CPU oracle (tests/naive_fragment_worlds.py).  A device graph and its oracle are built from
the same reads and nothing is compared before their filters are byte-equal (traversal_worlds.World._build)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rnabloom import _native as N
from rnabloom import graphutils, sharded
from rnabloom.graph import BloomFilterDeBruijnGraph, _pack
import naive_fragment_worlds as NW
import traversal_worlds as tw

ERR_INVALID = 1                     # RB_ERR_INVALID
FILTERS = (N.DBGBF, N.CBF)
WORLDS = {}


@pytest.fixture(scope="module", autouse=True)
def release_the_device_graphs():
    """the worlds' device graphs are shared by the tests of this file and destroyed behind the last one"""
    yield
    for w in WORLDS.values():
        w.destroy()
    WORLDS.clear()


def random_world(case):
    if ("random", case) not in WORLDS:
        WORLDS[("random", case)] = NW.random_world(case, device=True)
    return WORLDS[("random", case)]


def ring_world(case):
    if ("ring", case) not in WORLDS:
        WORLDS[("ring", case)] = NW.ring_world(*case, device=True)
    return WORLDS[("ring", case)]


def same(rc, want):
    for f in NW.FIELDS:
        if int(rc[f]) != int(want[f]):
            return f
    return None if not rc["pad"].any() else "pad"


def call(g, frags, min_cov, room, phase=None):
    """one device call, read-only"""
    before = [g.fold(f) for f in FILTERS]
    texts, recs = g.naiveExtendFragments(frags, min_cov, room, phase)
    assert [g.fold(f) for f in FILTERS] == before
    return texts, recs


def compare(w, frags, min_cov, room, label, phase=None):
    texts, recs = call(w.gg, frags, min_cov, room, phase)
    want = NW.answers(w.og, w.k, frags, min_cov, room, phase)
    for i, a in enumerate(want):
        assert texts[i] == a["text"] and same(recs[i], a) is None, (label, i, same(recs[i], a), recs[i], {f: a[f] for f in NW.FIELDS})
    return texts, recs


@pytest.mark.parametrize("min_cov", NW.MIN_COVS)
@pytest.mark.parametrize("case", NW.RANDOM_CASES, ids=tw.case_id)
def test_random_worlds_equal_the_restatement(case, min_cov):
    """every record field and the text; room 256 keeps the table in LDS (at most 150 k-mers + 512), room 4096 puts it in device scratch"""
    w = random_world(case)
    frags = NW.random_fragments(w, NW.N_RANDOM.get(w.k, 10), 1)
    assert max(len(f) - w.k + 1 for f in frags) + 2 * 256 <= N.NAIVE_FRAG_LDS_ENTRIES < 1 + 2 * NW.AMPLE
    a, _ = compare(w, frags, min_cov, 256, (case, min_cov, 256))
    b, _ = compare(w, frags, min_cov, NW.AMPLE, (case, min_cov, NW.AMPLE))
    assert a == b
    assert a == graphutils.naiveExtendComposed(w.gg, frags, min_cov, NW.AMPLE)
    assert a == graphutils.naiveExtend(w.gg, frags, 5, min_cov, room=3)


@pytest.mark.parametrize("case", NW.RING_CASES, ids=lambda c: "k%d-%s-%s" % (c[0], "stranded" if c[1] else "canonical", c[2]))
def test_ring_worlds_equal_the_restatement(case):
    """MEMBER on the fragment and on the left extension, walks of 550 k-mers, both homes of the table, a call that runs out of room"""
    w = ring_world(case)
    for min_cov in NW.MIN_COVS:
        for room in NW.RING_ROOMS:
            compare(w, [w.fragment], min_cov, room, (case, min_cov, room))
        want = NW.restate(w.og, w.k, w.fragment, min_cov)["text"]
        assert graphutils.naiveExtendComposed(w.gg, [w.fragment], min_cov, NW.AMPLE) == [want]
        # ... and with the cap of a call that runs out of room: no right walk behind a left walk that filled it
        assert graphutils.naiveExtendComposed(w.gg, [w.fragment], min_cov, 64) == [NW.restate(w.og, w.k, w.fragment, min_cov, 64)["text"]]


@pytest.mark.parametrize("stranded", [True, False])
def test_chained_calls_equal_one_call_with_ample_room(stranded):
    """room 4096 in one call against chained calls with room 64 and room 1: the texts, the extensions summed over the calls, the last call's ends
    and hits; phase 1 occurs (a right walk that runs out of room is resumed alone)"""
    phase_one = 0
    for spur in NW.RING_SPURS:
        w = ring_world((NW.K_MAIN, stranded, spur))
        for min_cov in NW.MIN_COVS:
            (one,), (rec,) = call(w.gg, [w.fragment], min_cov, NW.AMPLE)
            assert rec["status"] == N.NFRAG_DONE
            for room in (64, 1) if (spur, min_cov) == ("far", 2.0) else (64,):      # (room 1: 550 calls and more, for one world)
                text, phase, left, right, calls = w.fragment, None, 0, 0, 0
                while True:
                    (text,), (rc,) = w.gg.naiveExtendFragments([text], min_cov, room, phase)
                    left, right, calls = left + int(rc["left_ext"]), right + int(rc["right_ext"]), calls + 1
                    assert int(rc["left_ext"]) <= room and int(rc["right_ext"]) <= room
                    if rc["status"] != N.NFRAG_ROOM: break
                    phase = [0 if rc["left_end"] == N.NFRAG_END_ROOM else 1]
                    phase_one += phase[0]
                assert text == one and (left, right) == (int(rec["left_ext"]), int(rec["right_ext"])), (spur, min_cov, room)
                assert (rc["right_end"], rc["right_hit"]) == (rec["right_end"], rec["right_hit"]), (spur, min_cov, room)
                if rc["left_end"] != N.NFRAG_END_NOT_RUN:
                    assert (rc["left_end"], rc["left_hit"]) == (rec["left_end"], rec["left_hit"]), (spur, min_cov, room)
                assert room == 1 or calls == NW.restate_chain(w.og, w.k, w.fragment, min_cov, room)[4]
            assert graphutils.naiveExtend(w.gg, [w.fragment], 5, min_cov, room=64) == [one]
    assert phase_one > 0


def test_phase_one_runs_the_right_walk_only():
    w = random_world(NW.RANDOM_CASES[0])
    frags = NW.random_fragments(w, 30, 1)
    _, recs = compare(w, frags, 1.0, 256, "phase 1", phase=[1] * len(frags))
    assert (recs["left_end"] == N.NFRAG_END_NOT_RUN).all() and (recs["left_ext"] == 0).all()
    mixed = [i % 2 for i in range(len(frags))]
    compare(w, frags, 1.0, 256, "mixed phases", phase=mixed)


@pytest.mark.parametrize("stranded", [True, False])
def test_kmers_that_hash_alike(stranded):
    """k = 64: (AC)^32 and (CA)^32 have one hash; a table that trusted it would end the fragment (AC)^32's left walk at once"""
    key = ("hash_equal", stranded)
    if key not in WORLDS:
        WORLDS[key] = tw.hash_equal_world(stranded, device=True)
    w = WORLDS[key]
    _, recs = compare(w, NW.hash_equal_fragments(), 1.0, 64, key)
    if stranded:
        assert recs[0]["left_ext"] == 1 and recs[0]["left_end"] == N.NFRAG_END_MEMBER and recs[0]["left_hit"] == 1


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sequence_counts_around_the_wavefront(n):
    w = random_world(NW.RANDOM_CASES[2])
    frags = NW.random_fragments(w, 70, 2)[:n]
    compare(w, frags, 1.0, 256, n)


def test_small_pieces(monkeypatch):
    """RB_QUERY_PIECE in capacity k-mers (a fragment with room 256 has 513 .. 662): a few sequences a piece, then one"""
    w = random_world(NW.RANDOM_CASES[1])
    frags = NW.random_fragments(w, 40, 3) + [b"ACGT", b"acgt" * 20]
    whole = w.gg.naiveExtendFragmentsFlat(*_pack(frags), 1.0, 256)
    for piece in ("2100", "1"):
        monkeypatch.setenv("RB_QUERY_PIECE", piece)
        got = w.gg.naiveExtendFragmentsFlat(*_pack(frags), 1.0, 256)
        assert got[0].tobytes() == whole[0].tobytes() and (got[1] == whole[1]).all() and got[2].tobytes() == whole[2].tobytes(), piece


def test_sequences_that_are_not_judged_come_back_as_they_went_in():
    w = random_world(NW.RANDOM_CASES[0])
    k = w.k
    good = NW.random_fragments(w, 6, 4)
    f = good[3]
    odd = [f.lower(), f[:7] + b"N" + f[8:], f.replace(b"T", b"U", 1), f[:k - 1], b"", f[:5] + b"a" + f[6:]]
    whys = [N.NFRAG_WHY_LETTER] * 3 + [N.NFRAG_WHY_NO_KMER] * 2 + [N.NFRAG_WHY_LETTER]
    frags = [x for pair in zip(good, odd) for x in pair]
    texts, recs = compare(w, frags, 1.0, 64, "not judged")
    out, oo, _ = w.gg.naiveExtendFragmentsFlat(*_pack(frags), 1.0, 64)
    for j, (s, why) in enumerate(zip(odd, whys)):
        i = 2 * j + 1
        assert texts[i] == s and recs[i]["status"] == N.NFRAG_NOT_JUDGED and recs[i]["why"] == why, j
        assert not out[oo[i] + len(s):oo[i + 1]].any()
    assert graphutils.naiveExtend(w.gg, frags, 5, 1.0, room=64, keepNotJudged=True)[1::2] == odd
    with pytest.raises(ValueError):
        graphutils.naiveExtend(w.gg, frags, 5, 1.0, room=64)


# ---- refusals, the size query, the profile entry ----
def raw_call(h, frags, room=64, min_cov=1.0, phase=None, seq=True, off=True, oo=True, out=True, recs=True, offsets=None):
    s, o = _pack(frags)
    if offsets is not None:
        o = np.asarray(offsets, np.int64)
    n = len(o) - 1
    a_oo = np.full(n + 1, 7, np.int64)
    a_out = np.full(int(np.diff(o).clip(0).sum()) + (2 * room * n if 0 < room <= 4096 else 0) + 8, 7, np.uint8)      # (a larger room: size queries and refusals only)
    a_rec = np.full(max(n, 1) * 16, 7, np.int32)
    ph = None if phase is None else np.asarray(phase, np.uint8)
    p = lambda a, use: a.ctypes.data_as(C.c_void_p) if use and a is not None else None
    rc = N.lib.rb_graph_naive_extend_fragments(h, p(s, seq), p(o, off), n, p(ph, True), min_cov, room, p(a_oo, oo), p(a_out, out), p(a_rec, recs))
    return rc, a_oo, a_out, a_rec


def digests(h):
    out = []
    for f in FILTERS:
        v = C.c_uint64()
        out.append(v.value if N.lib.rb_filter_fold(h, f, C.byref(v)) == 0 else None)
    return out


def refused(h, frags, **kw):
    """one refused call: RB_ERR_INVALID with a message, no output byte written, the handle's filters as they were"""
    before = digests(h) if h is not None else None
    r = raw_call(h, frags, **kw)
    assert r[0] == ERR_INVALID and N.lib.rb_last_error(), kw
    assert (r[1] == 7).all() and (r[2] == 7).all() and (r[3] == 7).all(), kw                   # nothing was launched
    if h is not None:
        assert digests(h) == before and any(d is not None for d in before), kw


def test_refusals_leave_everything_alone():
    w = random_world(NW.RANDOM_CASES[0])
    g = w.gg
    frags = NW.random_fragments(w, 20, 5)
    nq = len(frags)
    before = digests(g.h)
    assert None not in before and 0 not in before
    untouched = lambda r: (r[1] == 7).all() and (r[2] == 7).all() and (r[3] == 7).all()
    for room in (1, 1 << 24):
        r = raw_call(g.h, frags[:2], room=room, out=False, recs=False)
        assert r[0] == 0 and (r[2] == 7).all() and (r[3] == 7).all()                           # the size query, the smallest and the largest room
    assert raw_call(g.h, frags, room=1)[0] == 0 and raw_call(g.h, frags, room=64, phase=[1] * nq)[0] == 0
    r = raw_call(g.h, [])
    assert r[0] == 0 and untouched(r)                                                           # n == 0 touches nothing
    assert raw_call(g.h, [], seq=False, off=False, oo=False, out=False, recs=False)[0] == 0
    assert digests(g.h) == before                                                               # the accepted calls are read-only too
    for kw in (dict(off=False), dict(oo=False), dict(recs=False), dict(seq=False), dict(phase=[0] * (nq - 1) + [2]), dict(min_cov=float("nan")),
               dict(min_cov=float("inf")), dict(min_cov=-1.0), dict(offsets=[0, 90, 40] + [40] * (nq - 2)), dict(room=0), dict(room=-5),
               dict(room=(1 << 24) + 1)):
        refused(g.h, frags, **kw)
    refused(None, frags)
    r = N.lib.rb_graph_naive_extend_fragments(g.h, None, None, -1, None, C.c_float(1.0), 64, None, None, None)
    assert r == ERR_INVALID                                                                     # n < 0
    rk = sharded.ShardRank((100_003, 200_003, 30_011, 2, 2, 2, 25, 0, 1, 0, 0, 9, 0), 0, 1, 0, "split")
    refused(rk.h, frags)                                                                        # a shard handle
    rk.destroy()
    for destroy, gone in (("destroyCbf", N.CBF), ("destroyDbgbf", N.DBGBF)):
        g2 = BloomFilterDeBruijnGraph(*w.sizes, 64, *w.hashes, 1, w.k, w.stranded, False, rngSeed=3)
        g2.addReads(w.seq, None, w.off, 3)
        assert raw_call(g2.h, frags)[0] == 0
        getattr(g2, destroy)()
        assert [d is None for d in digests(g2.h)] == [f == gone for f in FILTERS]
        refused(g2.h, frags)                                                                    # the filter that remains is as it was
        g2.destroy()
    with pytest.raises(N.NativeError):
        g.naiveExtendFragments(frags, 1.0, 0)
    assert digests(g.h) == before


def test_the_size_query():
    w = random_world(NW.RANDOM_CASES[0])
    frags = NW.random_fragments(w, 20, 6) + [b"", b"ACGTN"]
    r = raw_call(w.gg.h, frags, room=100, out=False, recs=False)
    assert r[0] == 0 and (r[2] == 7).all() and (r[3] == 7).all()
    assert r[1].tolist() == np.concatenate(([0], np.cumsum([len(s) + 200 for s in frags]))).tolist()
    out, oo, recs = w.gg.naiveExtendFragmentsFlat(*_pack(frags), 1.0, 100)
    assert oo.tolist() == r[1].tolist() and out.size == int(oo[-1])


def test_profile_entry():
    w = random_world(NW.RANDOM_CASES[0])
    g = w.gg
    g.profileEnable(True)
    g.profileGet(reset=True)
    g.naiveExtendFragments(NW.random_fragments(w, 20, 7), 1.0, 256)
    prof = g.profileGet()
    assert prof["naive_extend_fragments"][0] > 0 and prof["naive_extend_fragments"][1] == 1, prof
    g.profileEnable(False)


# ---- the worker's rules after overlapAndConnect ----
@pytest.mark.parametrize("stranded", [False, True])
def test_finish_fragments_equals_its_restatement(stranded):
    """outcomes, texts, preExtensionFragLen, whether the extension was adopted, and minCov as bits, with the extension and the trim on and off"""
    w = NW.finish_world(stranded)
    g = BloomFilterDeBruijnGraph(*w.sizes, *w.hashes, w.k, w.stranded, True, rngSeed=5)
    try:
        g.setReadPairedKmerDistance(w.d)
        g.addReads(*w.packed, 3, storeReadPairedKmers=True)
        assert (g.exportFilter(N.DBGBF) == w.og.dbgbf_bytes()).all() and (g.exportFilter(N.CBF) == w.og.cbf_bytes()).all()
        assert (g.exportFilter(N.RPKBF) == w.og.rpkbf_bytes()).all()
        frags = NW.finish_fragments(w)
        seen = set()
        for extend, trim in NW.FINISH_SWITCHES:
            got = graphutils.finishFragments(g, [f for f, _, _ in frags], [l for _, l, _ in frags], [r for _, _, r in frags], extendFragments=extend,
                                             trimArtifact=trim, **NW.FINISH)
            want = NW.finish_answers(w, extend, trim)
            for i, (a, b) in enumerate(zip(got, want)):
                assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and a[4] == b[4], (extend, trim, i, a, b)
                assert (a[2] is None) == (b[2] is None) and (a[2] is None or np.float32(a[2]).view(np.uint32) == np.float32(b[2]).view(np.uint32)), (i, a, b)
                seen.add(a[3])
        assert seen >= {NW.KEPT, NW.INCONSISTENT, NW.SPURIOUS, NW.NO_COMPLEX_KMER, NW.TOO_SHORT}
    finally:
        g.destroy()
