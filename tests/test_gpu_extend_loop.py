"""rb_graph_extend_loop (GraphUtils.extendSE / extendPE with the whole loop on the device) against the call restated in
tests/test_extend_loop_rules.py over the CPU oracle, a device graph and the oracle built from the same reads.  Compared per sequence: every
record field (the two floors as bits) and the text; texts and ranges also with graphutils.extendSE / extendPE (the host loop) on the same
device graph; the filters' digests before and after every call.  Worlds: k = 25, stranded and canonical, SE (d 30) and PE (d_r 30, d_f 80)
with 200 seeds, room 4096, 256 and D + 2 (chained); small pieces; n = 1, 63, 64, 65; 20 003 sequences in one call; phase 1; sequences that
are not judged; d = 2, 3, 256 (walk rows in LDS) and 300 (in device scratch); the matrix of tests/pair_worlds.py at k = 16 .. 256, both
strandednesses, SE and PE; every refusal; the size query; the profile entry."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rnabloom import _native as N
from rnabloom import graphutils, sharded
from rnabloom.graph import BloomFilterDeBruijnGraph, _pack
import pair_worlds as PW
import test_extend_loop_rules as L
import test_extend_pe_rules as P
import test_extend_step_rules as R
import test_gpu_extend_pe as GP
import test_gpu_extend_step as GS

ERR_INVALID = 1                     # RB_ERR_INVALID
SE, PE = L.SE, L.PE
FILTERS = (N.DBGBF, N.CBF, N.RPKBF, N.FPKBF)
DEVICES = {}


@pytest.fixture(scope="module", autouse=True)
def release_the_device_graphs():
    """the worlds' device graphs are shared by the tests of this file and destroyed behind the last one"""
    yield
    for g in DEVICES.values():
        g.destroy()
    DEVICES.clear()


def device(sd, keep=True):
    """the device twin of a side's world: tests/test_gpu_extend_step.py::device for an SE world, tests/test_gpu_extend_pe.py::device for a PE world"""
    w = sd.w
    if id(w) in DEVICES:
        return DEVICES[id(w)]
    g = BloomFilterDeBruijnGraph(*w.sizes, *w.hashes, w.k, w.stranded, True, rngSeed=5)
    if sd.which == PE:
        GP.fill(g, w)
        assert (g.exportFilter(N.FPKBF) == w.og.fpkbf_bytes()).all()
    else:
        g.setReadPairedKmerDistance(w.d)
        g.addReads(*w.packed, 3, storeReadPairedKmers=True)
    assert (g.exportFilter(N.DBGBF) == w.og.dbgbf_bytes()).all() and (g.exportFilter(N.CBF) == w.og.cbf_bytes()).all()
    assert (g.exportFilter(N.RPKBF) == w.og.rpkbf_bytes()).all()
    if keep:
        DEVICES[id(w)] = g
    return g


def folds(g, which):
    return [g.fold(f) for f in FILTERS[:4 if which == PE else 3]]


def same(rc, want):
    """every field of a device record against the restated call's, the floors as bits"""
    for f in L.FIELDS:
        if f.endswith("floor"):
            if np.float32(rc[f]).view(np.uint32) != np.float32(want[f]).view(np.uint32):
                return f
        elif int(rc[f]) != int(want[f]):
            return f
    return None if not rc["pad"].any() else "pad"


def call(sd, g, seeds, room, phase=None):
    """one device call, read-only"""
    before = folds(g, sd.which)
    texts, recs = g.extendLoop(seeds, sd.which, 1.0, room, phase)
    assert folds(g, sd.which) == before
    return texts, recs


def compare(sd, g, idx, room, label, phase=None):
    """seeds idx in one device call against the restated call of each"""
    seeds = [sd.seeds[i] for i in idx]
    texts, recs = call(sd, g, seeds, room, None if phase is None else [phase] * len(idx))
    for j, i in enumerate(idx):
        want = sd.ample(i)[:2] if room == L.AMPLE and not phase else sd.call(sd.seeds[i], room, phase or 0)
        assert texts[j] == want[0] and same(recs[j], want[1]) is None, (label, i, same(recs[j], want[1]), recs[j], want[1])
    return texts, recs


def ranges_of(sd, idx):
    return [[sd.ample(i)[1]["left_ext"], sd.ample(i)[1]["left_ext"] + len(sd.seeds[i]) - sd.k + 1] for i in idx]


def host_loop(sd):
    return graphutils.extendPE if sd.which == PE else graphutils.extendSE


def on_device(sd):
    return graphutils.extendPEOnDevice if sd.which == PE else graphutils.extendSEOnDevice


# ---- k = 25: the 200 seeds ----
@pytest.mark.parametrize("p", L.K25, ids=L.k25_id)
def test_ample_room_equals_the_restated_call_and_the_host_loop(p):
    sd = L.side25(*p)
    g = device(sd)
    idx = list(range(len(sd.seeds)))
    texts, recs = compare(sd, g, idx, L.AMPLE, p)
    assert all(int(rc["status"]) == L.DONE for rc in recs)
    before = folds(g, sd.which)
    htexts, hranges = host_loop(sd)(g, sd.seeds, 1.0)
    assert htexts == texts and hranges == ranges_of(sd, idx)
    dtexts, dranges = on_device(sd)(g, sd.seeds, 1.0)
    assert dtexts == texts and dranges == hranges and folds(g, sd.which) == before


@pytest.mark.parametrize("p", L.K25, ids=L.k25_id)
def test_chained_calls_with_the_smallest_room(p):
    """room D + 2 for the longest grower and a seed of each ending: call after call, every record against the restated chain's"""
    sd = L.side25(*p)
    g = device(sd)
    picks = sd.picks()
    room = sd.D + 2
    want = {i: sd.chain(sd.seeds[i], room) for i in picks}
    texts, got = {i: sd.seeds[i] for i in picks}, {i: [] for i in picks}
    todo, phase = list(picks), None
    while todo:
        t, recs = call(sd, g, [texts[i] for i in todo], room, phase)
        nxt, phase = [], []
        for i, text, rc in zip(todo, t, recs):
            texts[i] = text
            got[i].append(rc)
            if int(rc["status"]) == L.ROOM:
                nxt.append(i)
                phase.append(0 if int(rc["left_end"]) == L.END_ROOM else 1)
        todo = nxt
    for i in picks:
        assert texts[i] == want[i][0] == sd.ample(i)[0] and len(got[i]) == len(want[i][2]), i
        assert all(same(a, b) is None for a, b in zip(got[i], want[i][2])), i
        assert sum(int(rc["left_ext"]) for rc in got[i]) == want[i][1][0]
    assert max(len(v) for v in got.values()) > 4
    seeds = [sd.seeds[i] for i in picks]
    assert on_device(sd)(g, seeds, 1.0, room=room) == ([sd.ample(i)[0] for i in picks], ranges_of(sd, picks))


@pytest.mark.parametrize("p", L.K25, ids=L.k25_id)
def test_room_256(p):
    sd = L.side25(*p)
    g = device(sd)
    idx = list(range(len(sd.seeds)))
    _, recs = compare(sd, g, idx, 256, p)
    assert {int(rc["status"]) for rc in recs} == {L.DONE, L.ROOM}
    assert on_device(sd)(g, sd.seeds, 1.0, room=256) == ([sd.ample(i)[0] for i in idx], ranges_of(sd, idx))


@pytest.mark.parametrize("p", [(SE, False), (PE, True)], ids=L.k25_id)
def test_small_pieces(p, monkeypatch):
    """RB_QUERY_PIECE in capacity k-mers (a seed of 25 .. 79 letters with room 256 has some 540): 7 sequences a piece, then one"""
    sd = L.side25(*p)
    g = device(sd)
    whole = g.extendLoopFlat(*_pack(sd.seeds), sd.which, 1.0, 256)
    for piece, n in (("4099", len(sd.seeds)), ("1", 40)):
        monkeypatch.setenv("RB_QUERY_PIECE", piece)
        got = g.extendLoopFlat(*_pack(sd.seeds[:n]), sd.which, 1.0, 256)
        end = int(got[1][n])
        assert got[0][:end].tobytes() == whole[0][:end].tobytes() and (got[1] == whole[1][:n + 1]).all(), piece
        assert got[2].tobytes() == whole[2][:n].tobytes(), piece


@pytest.mark.parametrize("p", [(SE, True), (PE, False)], ids=L.k25_id)
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sequence_counts_around_the_wavefront(n, p):
    sd = L.side25(*p)
    compare(sd, device(sd), list(range(n)), L.AMPLE, (n, p))


@pytest.mark.parametrize("p", [(SE, False), (PE, False)], ids=L.k25_id)
def test_twenty_thousand_sequences(p):
    sd = L.side25(*p)
    g = device(sd)
    n = len(sd.seeds)
    texts, recs = call(sd, g, sd.seeds, 256)
    many, mrecs = call(sd, g, [sd.seeds[i % n] for i in range(20_003)], 256)
    assert mrecs.tobytes() == np.concatenate([recs] * 101)[:20_003].tobytes()
    assert many == [texts[i % n] for i in range(20_003)]


@pytest.mark.parametrize("p", L.K25, ids=L.k25_id)
def test_phase_one_runs_the_right_side_only(p):
    sd = L.side25(*p)
    g = device(sd)
    idx = [i for i in range(len(sd.seeds)) if sd.ample(i)[1]["left_ext"] > 0][:40]
    assert len(idx) == 40
    _, recs = compare(sd, g, idx, L.AMPLE, p, phase=1)
    assert all(int(rc["left_ext"]) == 0 and int(rc["left_end"]) == L.END_NOT_RUN and rc["left_floor"] == 0 for rc in recs)
    # both phases in one call
    mixed = [j % 2 for j in range(len(idx))]
    texts, recs = call(sd, g, [sd.seeds[i] for i in idx], L.AMPLE, mixed)
    for j, i in enumerate(idx):
        want = sd.call(sd.seeds[i], L.AMPLE, 1) if mixed[j] else sd.ample(i)[:2]
        assert texts[j] == want[0] and same(recs[j], want[1]) is None, (p, i)


@pytest.mark.parametrize("p", [(SE, False), (PE, True)], ids=L.k25_id)
def test_sequences_that_are_not_judged_come_back_as_they_went_in(p):
    sd = L.side25(*p)
    g = device(sd)
    fork = next(s for kind, s, dd in sd.w.queries if kind == "fork-0" and dd == 0)
    odd = [fork[:-1] + b"N", b"N" + fork[1:], fork[:40].lower() + fork[40:], fork.replace(b"T", b"U"), fork[:sd.k - 1], b"", b"acgu"]
    whys = [L.WHY_LETTER] * 4 + [L.WHY_NO_KMER] * 3
    seeds = sd.seeds[:3] + odd + sd.seeds[3:6]
    texts, recs = call(sd, g, seeds, L.AMPLE)
    for j, (s, why) in enumerate(zip(odd, whys)):
        assert texts[3 + j] == s and same(recs[3 + j], dict(L.blank(s), status=L.NOT_JUDGED, why=why)) is None, (j, recs[3 + j])
    for j, i in enumerate(range(6)):
        at = j if j < 3 else j + len(odd)
        assert texts[at] == sd.ample(i)[0] and same(recs[at], sd.ample(i)[1]) is None
    out, oo, _ = g.extendLoopFlat(*_pack(seeds), sd.which, 1.0, L.AMPLE)
    for j in range(len(seeds)):
        assert not out[int(oo[j]) + int(recs[j]["out_len"]):int(oo[j + 1])].any()                # zeros behind every text
    assert on_device(sd)(g, odd, 1.0) == host_loop(sd)(g, odd, 1.0)
    assert call(sd, g, odd, L.AMPLE)[0] == odd                                                  # a call without a judged sequence launches nothing


# ---- the edges of the distances: d = 2 and 3, 256 (the walks' rows in LDS) and 300 (in device scratch) ----
SMALL = {}


def small_side(which, d):
    if (which, d) not in SMALL:
        SMALL[(which, d)] = L.Side(GP.small_world(2 if d <= 3 else 30, d) if which == PE else GS.small_world(d), which)
    return SMALL[(which, d)]


@pytest.mark.parametrize("which", [SE, PE], ids=["se", "pe"])
@pytest.mark.parametrize("d", [2, 3, GS.LDS_D, 300])
def test_edges_of_the_distance(d, which):
    sd = small_side(which, d)
    assert sd.D == d and len(sd.seeds) >= 60
    g = device(sd)
    idx = list(range(60))
    _, recs = compare(sd, g, idx, L.AMPLE, (which, d))
    assert sum(int(rc["left_rounds"]) + int(rc["right_rounds"]) for rc in recs) > 60
    assert on_device(sd)(g, sd.seeds[:20], 1.0, room=d + 2) == ([sd.ample(i)[0] for i in idx[:20]], ranges_of(sd, idx[:20]))
    assert host_loop(sd)(g, sd.seeds[:20], 1.0) == ([sd.ample(i)[0] for i in idx[:20]], ranges_of(sd, idx[:20]))


# ---- the matrix: the k at which hash rotations and the bases' packing change slot ----
@pytest.mark.parametrize("which", [SE, PE], ids=["se", "pe"])
@pytest.mark.parametrize("case", L.MATRIX, ids=PW.case_id)
def test_matrix(case, which):
    sd = L.side_of_case(which, case)
    g = device(sd, keep=False)
    try:
        idx = list(range(80))
        texts, recs = compare(sd, g, idx, L.AMPLE, (PW.case_id(case), which))
        assert all(int(rc["status"]) == L.DONE for rc in recs) and sum(int(rc["left_ext"]) + int(rc["right_ext"]) for rc in recs) > 80
        assert on_device(sd)(g, sd.seeds[:80], 1.0, room=256) == (texts, ranges_of(sd, idx))
    finally:
        g.destroy()


# ---- refusals, the size query, the profile entry ----
def raw_call(h, seeds, which=SE, room=64, min_cov=1.0, phase=None, seq=True, off=True, oo=True, out=True, recs=True, offsets=None):
    s, o = _pack(seeds)
    if offsets is not None:
        o = np.asarray(offsets, np.int64)
    n = len(o) - 1
    a_oo = np.full(n + 1, 7, np.int64)
    a_out = np.full(int(np.diff(o).clip(0).sum()) + (2 * room * n if 0 < room <= 4096 else 0) + 8, 7, np.uint8)      # (a larger room: size queries and refusals only)
    a_rec = np.full(max(n, 1) * 16, 7, np.int32)
    ph = None if phase is None else np.asarray(phase, np.uint8)
    p = lambda a, use: a.ctypes.data_as(C.c_void_p) if use and a is not None else None
    rc = N.lib.rb_graph_extend_loop(h, which, p(s, seq), p(o, off), n, p(ph, True), min_cov, room, p(a_oo, oo), p(a_out, out), p(a_rec, recs))
    return rc, a_oo, a_out, a_rec


def digests(h):
    out = []
    for f in FILTERS:
        v = C.c_uint64()
        out.append(v.value if N.lib.rb_filter_fold(h, f, C.byref(v)) == 0 else None)
    return out


def refused(h, seeds, **kw):
    """one refused call: RB_ERR_INVALID with a message, no output byte written, the handle's filters as they were"""
    before = digests(h) if h is not None else None
    r = raw_call(h, seeds, **kw)
    assert r[0] == ERR_INVALID and N.lib.rb_last_error(), kw
    assert (r[1] == 7).all() and (r[2] == 7).all() and (r[3] == 7).all(), kw                   # nothing was launched
    if h is not None:
        assert digests(h) == before and any(d is not None for d in before), kw


def test_refusals_leave_everything_alone():
    sd = L.side25(PE, False)
    w, g = sd.w, device(sd)
    seeds = sd.seeds[:40]
    nq = len(seeds)
    before = digests(g.h)
    assert None not in before and 0 not in before
    untouched = lambda r: (r[1] == 7).all() and (r[2] == 7).all() and (r[3] == 7).all()
    for which, room in ((SE, w.d_r + 2), (PE, w.d_f + 2), (PE, 1 << 24)):
        r = raw_call(g.h, seeds[:2] if room > 4096 else seeds, which=which, room=room, out=False, recs=False)
        assert r[0] == 0 and (r[2] == 7).all() and (r[3] == 7).all()                           # the size query, the largest room included
    assert raw_call(g.h, seeds, which=SE, room=w.d_r + 2)[0] == 0 and raw_call(g.h, seeds, which=PE, room=w.d_f + 2, phase=[1] * nq)[0] == 0
    r = raw_call(g.h, [])
    assert r[0] == 0 and untouched(r)                                                           # n == 0 touches nothing
    assert raw_call(g.h, [], seq=False, off=False, oo=False, out=False, recs=False)[0] == 0
    assert digests(g.h) == before                                                               # the accepted calls are read-only too
    for kw in (dict(off=False), dict(oo=False), dict(recs=False), dict(seq=False), dict(which=2), dict(which=-1), dict(phase=[0] * (nq - 1) + [2]),
               dict(min_cov=float("nan")), dict(min_cov=float("inf")), dict(min_cov=-1.0), dict(offsets=[0, 90, 40] + [40] * (nq - 2)),
               dict(which=SE, room=w.d_r + 1), dict(which=PE, room=w.d_f + 1), dict(which=PE, room=0), dict(which=PE, room=-5),
               dict(which=PE, room=(1 << 24) + 1)):
        refused(g.h, seeds, **dict(dict(which=PE, room=w.d_f + 2), **kw))
    refused(None, seeds)
    rk = sharded.ShardRank((100_003, 200_003, 30_011, 2, 2, 2, 25, 0, 1, 0, 0, 9, 0), 0, 1, 0, "split")
    refused(rk.h, seeds)                                                                        # a shard handle
    rk.destroy()
    for destroy, gone in (("destroyCbf", N.CBF), ("destroyDbgbf", N.DBGBF), ("destroyRpkbf", N.RPKBF), ("destroyFpkbf", N.FPKBF)):
        g2 = BloomFilterDeBruijnGraph(*w.sizes, *w.hashes, 25, False, True, rngSeed=5)
        refused(g2.h, seeds, which=SE, room=4096)                                               # no distances yet
        g2.setReadPairedKmerDistance(w.d_r)
        refused(g2.h, seeds, which=PE, room=4096)                                               # a read distance, no fragment-pair filter
        GP.fill(g2, w)
        full = digests(g2.h)
        assert None not in full and 0 not in full
        g2.setReadPairedKmerDistance(1)
        refused(g2.h, seeds, which=SE, room=4096)                                               # d_r < 2
        refused(g2.h, seeds, which=PE, room=4096)
        g2.setReadPairedKmerDistance(w.d_r)
        g2.setFragPairedKmerDistance(1)
        refused(g2.h, seeds, which=PE, room=4096)                                               # d_f < 2
        assert raw_call(g2.h, seeds, which=SE, room=4096)[0] == 0                               # ... which extendSE does not read
        g2.setFragPairedKmerDistance(w.d_f)
        assert raw_call(g2.h, seeds, which=PE, room=4096)[0] == 0 and digests(g2.h) == full
        getattr(g2, destroy)()
        left = digests(g2.h)
        assert [d is None for d in left] == [f == gone for f in FILTERS]
        refused(g2.h, seeds, which=PE, room=4096)                                               # the three filters that remain are as they were
        if gone == N.FPKBF:
            assert raw_call(g2.h, seeds, which=SE, room=4096)[0] == 0                           # extendSE does not need it
        else:
            refused(g2.h, seeds, which=SE, room=4096)
        g2.destroy()
    g3 = BloomFilterDeBruijnGraph(100_003, 200_003, 30_011, 2, 2, 2, 25, False, False)          # made without read-paired k-mers
    g3.setReadPairedKmerDistance(30)
    refused(g3.h, seeds, which=SE, room=4096)
    g3.destroy()
    with pytest.raises(N.NativeError):
        g.extendLoop(seeds, 3, 1.0, 4096)
    assert digests(g.h) == before


def test_the_size_query():
    sd = L.side25(SE, True)
    g = device(sd)
    seeds = sd.seeds[:50] + [b"", b"ACGTN"]
    r = raw_call(g.h, seeds, which=SE, room=100, out=False, recs=False)
    assert r[0] == 0 and (r[2] == 7).all() and (r[3] == 7).all()
    assert r[1].tolist() == np.concatenate(([0], np.cumsum([len(s) + 200 for s in seeds]))).tolist()
    out, oo, recs = g.extendLoopFlat(*_pack(seeds), SE, 1.0, 100)
    assert oo.tolist() == r[1].tolist() and out.size == int(oo[-1])


def test_profile_entry():
    sd = L.side25(PE, True)
    g = device(sd)
    g.profileEnable(True)
    g.profileGet(reset=True)
    g.extendLoop(sd.seeds, PE, 1.0, 256)
    prof = g.profileGet()
    assert prof["extend_loop"][0] > 0 and prof["extend_loop"][1] == 1 and "extend_pe" not in prof, prof
    g.profileEnable(False)
