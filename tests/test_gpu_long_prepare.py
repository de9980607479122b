"""rb_long_prepare (what LongReadCorrectionWorker.run does to a raw read before its first graph call, on the device) against the restatement
of tests/test_long_prepare_rules.py over the worlds of tests/long_prepare_worlds.py.  Compared exactly: all 16 ints of every record, the
segments, and the transformed read letter for letter.  tests/test_long_prepare_reach.py shows on the restatement alone that these inputs reach
every status, flag, route and branch.  Then: many pieces equal one, no text wanted, no reads, every refusal with the outputs as they were,
the kernels' time, and the worker's whole chain over a device graph."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import long_prepare_worlds as W
from rnabloom import _native as N
from rnabloom import graphutils
from test_long_prepare_rules import FIELDS, SHORT, params, worker_chain

ERR_INVALID = 1
IDS = [W.case_id(c) for c in W.CASES]
NAMES = dict(min_len="k", reverse_complement="reverseComplement", strand_specific="strandSpecific", polya="minPolyATailLengthRequired",
             seed_length="seedLength", min_identity="minIdentity", max_gap="maxGap", window="window", lc_window="lcWindow", lc_min_length="lcMinLength")


def kw_of(P):
    """the restatement's parameters under graphutils' names"""
    kw = {NAMES[key]: v for key, v in P.items()}
    return kw.pop("k"), kw


def flat(reads):
    off = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    return np.frombuffer(b"".join(reads), np.uint8).copy(), off


def compare(reads, want, recs, so, segs, out, off):
    bad = []
    for j, (rec, wsegs, wseq) in enumerate(want):
        got = tuple(int(recs[j][f]) for f in recs.dtype.names[:14]) + tuple(int(x) for x in recs[j]["reserved"])
        gsegs = [tuple(x) for x in segs[so[j]:so[j] + max(0, got[11])].tolist()]
        ok = got == rec and gsegs == wsegs
        if ok and out is not None and wseq is not None:
            ok = out[off[j]:off[j] + len(wseq)].tobytes() == wseq
        if not ok:
            bad.append(j)
    assert not bad, (len(bad), bad[:8], [(len(reads[j]), reads[j][:80], want[j][:2]) for j in bad[:2]])


@pytest.mark.parametrize("i", range(len(W.CASES)), ids=IDS)
def test_records_segments_and_texts_match_the_restatement(i):
    reads, want, _ = W.want(i)
    k, kw = kw_of(W.CASES[i]["P"])
    seq, off = flat(reads)
    recs, so, segs, out = graphutils.prepareLongFlat(seq, off, k, **kw)
    compare(reads, want, recs, so, segs, out, off)
    # what the call does not fill stays as it was (zeros here): the tail of a read's region in out, and the slots behind its segments — the
    # kernel writes segments to its own slots before it knows whether the cut fires, and only n_segments of them may come back
    for j, (rec, wsegs, wseq) in enumerate(want):
        n = 0 if wseq is None else len(wseq)
        assert not out[off[j] + n:off[j + 1]].any(), j
        assert not segs[so[j] + len(wsegs):so[j + 1]].any(), j
    spare = sum(int(so[j + 1] - so[j]) - len(wsegs) for j, (rec, wsegs, wseq) in enumerate(want))
    speculative = sum(bool(rec[1] & 32) and rec[9] > 0 and not rec[1] & 16 for rec, _, _ in want)       # low windows seen, the cut did not fire
    assert spare > 0 and (speculative > 0 or W.CASES[i]["P"]["lc_min_length"] == 0)


@pytest.mark.parametrize("i", [0, 1], ids=[IDS[0], IDS[1]])
def test_the_wrapper_returns_segment_strings(i):
    reads, want, _ = W.want(i)
    k, kw = kw_of(W.CASES[i]["P"])
    recs, segments, texts = graphutils.prepareLongReads(reads[:60], k, **kw)
    assert texts == [seq for _, _, seq in want[:60]]
    assert segments == [[seq[b:e] for b, e in segs] for _, segs, seq in want[:60]]
    assert [int(x) for x in recs["status"]] == [rec[0] for rec, _, _ in want[:60]]
    assert any(t is None for t in texts) == (k > 0) and any(len(s) > 1 for s in segments)      # (with k = 0 no read is too short)


@pytest.mark.parametrize("piece", [1, 1000, 1 << 40])
def test_many_pieces_equal_one(piece, monkeypatch):
    i = 4
    reads, want, _ = W.want(i)
    k, kw = kw_of(W.CASES[i]["P"])
    seq, off = flat(reads)
    monkeypatch.setenv("RB_QUERY_PIECE", str(piece))
    recs, so, segs, out = graphutils.prepareLongFlat(seq, off, k, **kw)
    compare(reads, want, recs, so, segs, out, off)


def test_no_reads_no_text_and_the_kernel_time():
    reads, want, _ = W.want(2)
    k, kw = kw_of(W.CASES[2]["P"])
    seq, off = flat(reads)
    ms = np.full(1, -1.0)
    recs, so, segs, out = graphutils.prepareLongFlat(seq, off, k, wantText=False, kernelMs=ms, **kw)
    assert out is None and 0 < ms[0] < 10_000
    compare(reads, want, recs, so, segs, None, off)
    # n = 0 succeeds, touches nothing, and needs no array
    p = graphutils.prepParams(k, **kw)
    ms[0] = -1.0
    assert N.lib.rb_long_prepare(0, None, None, 0, C.byref(p), None, None, None, None, ms.ctypes.data_as(C.POINTER(C.c_double))) == 0 and ms[0] == 0
    assert N.lib.rb_long_prepare(0, None, None, 0, C.byref(p), None, None, None, None, None) == 0
    recs, segments, texts = graphutils.prepareLongReads([], k, **kw)
    assert recs.size == 0 and segments == [] and texts == []
    # reads without a letter need no text
    recs, segments, texts = graphutils.prepareLongReads([b"", b""], 0, **kw)
    assert texts == [b"", b""] and segments == [[b""], [b""]]


def test_every_refusal_writes_nothing():
    reads = [b"ACGT" * 200, b"A" * 300, b"GATTACA" * 10]
    seq, off = flat(reads)
    good = dict(graphutils.PREP_DEFAULTS)
    so = graphutils.prepSegmentRoom(off, 100)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(kw=None, n=3, p_null=False, so_=so, off_=off, seq_=seq, recs_null=False, segs_null=False):
        p = graphutils.prepParams(25, **dict(good, **(kw or {})))
        recs = np.full(3 * 16, 0x5A5A5A5A, np.int32)
        segs = np.full(2 * int(so[-1]) + 8, 0x5A5A5A5A, np.int32)
        out = np.full(seq.size, 0x5A, np.uint8)
        ms = np.full(1, -7.0)
        rc = N.lib.rb_long_prepare(0, ptr(seq_), ptr(off_), n, None if p_null else C.byref(p), ptr(so_), None if recs_null else ptr(recs),
                                   None if segs_null else ptr(segs), ptr(out), ms.ctypes.data_as(C.POINTER(C.c_double)))
        untouched = (recs == 0x5A5A5A5A).all() and (segs == 0x5A5A5A5A).all() and (out == 0x5A).all() and ms[0] == -7.0
        return rc, untouched, (N.lib.rb_last_error() or b"").decode()

    rc, untouched, _ = call()
    assert rc == 0 and not untouched                                          # the call itself is good
    short_room = so.copy(); short_room[2:] -= 1                               # read 1 (300 letters) needs (3 + 1) / 2 = 2 slots
    bad_off = off.copy(); bad_off[1] = off[2] + 1
    refusals = [(dict(kw=dict(seedLength=0)), "seed_length"), (dict(kw=dict(minIdentity=0.0)), "min_identity"), (dict(kw=dict(minIdentity=1.5)), "min_identity"),
                (dict(kw=dict(minIdentity=float("nan"))), "min_identity"), (dict(kw=dict(maxGap=-1)), "max_gap"), (dict(kw=dict(window=-1)), "window"),
                (dict(kw=dict(lcWindow=0)), "lc_window"), (dict(kw=dict(lcWindow=1025)), "lc_window"), (dict(kw=dict(lcMinLength=-1)), "lc_min_length"),
                (dict(n=-1), "n ="), (dict(p_null=True), "params"), (dict(so_=None), "null"), (dict(off_=None), "null"), (dict(recs_null=True), "null"),
                (dict(segs_null=True), "null"), (dict(seq_=None), "null sequence text"), (dict(so_=short_room), "room"), (dict(off_=bad_off), "offsets[1]")]
    for kw, word in refusals:
        rc, untouched, msg = call(**kw)
        assert rc == ERR_INVALID and untouched and "rb_long_prepare" in msg and word in msg, (kw, rc, untouched, msg)
    p = graphutils.prepParams(-1, **good)                                     # min_len < 0
    recs = np.full(3 * 16, 7, np.int32)
    segs = np.full(2 * int(so[-1]), 7, np.int32)
    assert N.lib.rb_long_prepare(0, ptr(seq), ptr(off), 3, C.byref(p), ptr(so), ptr(recs), ptr(segs), None, None) == ERR_INVALID
    assert (recs == 7).all() and (segs == 7).all() and b"min_len" in N.lib.rb_last_error()
    with pytest.raises(TypeError):
        graphutils.prepareLongReads(reads, 25, seed=4)


def test_the_workers_chain_from_the_raw_read():
    """correctLongReadsFromRaw on a small world of tests/long_worlds.py against worker_chain of the restatement, whose `correct` asks the same
    device graph one segment at a time; the graph's filters are as they were"""
    import long_worlds as LW
    from test_gpu_long_correction import digests
    w = LW.world(16, False, False)
    g = w.device()
    rng = np.random.default_rng(99)
    rich = lambda n, ch: W.rich(rng, n, ch)
    reads = []
    for j, q in enumerate(w.queries[:36]):
        t = w.tx[j % len(w.tx)]
        reads.append([q, q + rich(30, b"A"), rich(25, b"T") + q, q + rich(20, b"A") + b"CG", W.low(rng, 120) + t[:200] + W.low(rng, 260) + t[300:520],
                      t[:300] + W.low(rng, 250) + t[300:480] + rich(24, b"A"), W.low(rng, 140), q[:12]][j % 8])
    reads += [b"N" * 80, b"GN" * 40]              # corrected to themselves, every k-mer without a count and with an N: kept, nothing put out
    names = [b"read%d" % j for j in range(len(reads))]
    prep = dict(seedLength=12, window=40, lcWindow=40, lcMinLength=200)
    corr = dict(windowSize=40, maxIndelSize=1, percentIdentity=0.9, maxItr=2, lookahead=5)
    min_cov = 2
    P = params(min_len=16, strand_specific=0, seed_length=12, window=40, lc_window=40, lc_min_length=200)
    before = digests(g.h)
    got, kept, discarded = graphutils.correctLongReadsFromRaw(g, names, reads, minKmerCov=min_cov, prep=prep, **corr)
    empty_kept = []

    def correct(seg, trim):
        parts, alive = graphutils.correctLongReadsKept(g, [seg], minKmerCov=min_cov, trimLowCovEdges=trim, **corr)
        empty_kept.append(alive[0] and not parts[0])
        return parts[0] if alive[0] else None
    want, wkept, wdisc = worker_chain(names, reads, P, 16, min_cov, correct)
    assert digests(g.h) == before
    assert (kept, discarded) == (wkept, wdisc) and kept >= 10 and discarded >= 4
    assert sum(empty_kept) >= 2 and kept > len({o[0].split(b"_")[0] for o in got if not o[4]})      # reads kept with nothing put out
    assert got == want
    labels = b" ".join(o[0] for o in got)
    assert b"_s2" in labels and any(o[4] for o in got) and any(o[5] for o in got) and any(not o[5] for o in got)
