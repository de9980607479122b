"""rb_graph_correct_long (GraphUtils.correctLongSequenceWindowed on the device) against the restatement of tests/test_long_correction_rules.py run
on the CPU oracle's filters, a device graph and the oracle built from the same reads (tests/long_worlds.py).  Compared exactly: the final text,
its length and all 16 ints of every record.  The cases: k = 16 and 25, stranded and not, k = 64 with a repeat whose k-mers hash alike; windows of
40 (many windows in reads of 60 - 400 letters) and 500 (reads up to 1 500, windows merged at the end); max_indel_size 0, 1, 5; percent_identity
1.0 and 0.9; max_itr 0, 1, 5; the edge trim on and off; the solid-k-mer screen.  tests/test_long_correction_reach.py shows on the oracle alone
that these inputs reach every counter, status and flag.  Then: many pieces equal one, overflow and the wrapper's second call, letters outside
ACGTU, empty and short sequences, every refusal with the filters' digests before and after, the profile entry, the worker's chain."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import long_worlds as LW
from rnabloom import _native as N
from rnabloom import graphutils, sharded
from rnabloom.graph import BloomFilterDeBruijnGraph, _pack
from test_long_correction_rules import (CHANGED, CTRS, FIELDS, NO_KMER, NULL, OVERFLOW, TRIMMED_TO_NOTHING, UNCHANGED, assemble_valid_kmers,
                                        correct_long)

ERR_INVALID = 1
FILTERS = (N.DBGBF, N.CBF, N.RPKBF)
F = {f: i for i, f in enumerate(FIELDS)}
IDS = [LW.case_id(c) for c in LW.CASES]


def digests(h):
    out = []
    for f in FILTERS:
        v = C.c_uint64()
        out.append(v.value if N.lib.rb_filter_fold(h, f, C.byref(v)) == 0 else None)
    return out


def tuples(recs):
    return [tuple(int(rc[f]) for f in FIELDS) for rc in recs]


@pytest.mark.parametrize("i", range(len(LW.CASES)), ids=IDS)
def test_texts_and_records_match_the_restatement(i):
    w, want = LW.want(i)
    g = w.device()
    before = digests(g.h)
    texts, recs = g.correctLong(w.queries, **LW.params_of(LW.CASES[i]))
    got = tuples(recs)
    bad = [j for j in range(len(want)) if (texts[j], got[j]) != want[j]]
    assert not bad, (IDS[i], len(bad), bad[:5], [(w.queries[j], texts[j], got[j], want[j]) for j in bad[:2]])
    assert digests(g.h) == before                                            # read-only
    # graphutils: None for null and for no k-mer
    if i == 1:
        out = graphutils.correctLongSequenceWindowed(g, w.queries, **LW.params_of(LW.CASES[i]))
        assert out == [None if rec[F["status"]] in (NULL, NO_KMER) else t for t, rec in want]
        assert any(x is None for x in out) and any(x == b"" for x in out)


@pytest.mark.parametrize("i", [0, 3], ids=[IDS[0], IDS[3]])
def test_overflow_reports_the_room_and_writes_nothing(i):
    w, want = LW.want(i)
    g = w.device()
    seq, off = _pack(w.queries)
    for slack in (0, 1):
        room = np.array([len(s) + slack for s in w.queries], np.int64)
        oo = np.zeros(len(room) + 1, np.int64)
        np.cumsum(room, out=oo[1:])
        out, recs = g.correctLongFlat(seq, off, oo, **LW.params_of(LW.CASES[i]))
        got, over = tuples(recs), 0
        for j, (text, rec) in enumerate(want):
            assert got[j] == LW.with_overflow(rec, int(room[j])), (slack, j)
            mine = out[oo[j]:oo[j + 1]]
            if got[j][F["flags"]] & OVERFLOW:
                over += 1
                assert not mine.any(), (slack, j)                             # nothing written, nothing truncated
            else:
                assert mine[:len(text)].tobytes() == text and not mine[len(text):].any(), (slack, j)
        assert over >= 1 or slack
    assert sum(rec[F["out_len"]] > len(s) for s, (_, rec) in zip(w.queries, want)) >= 1


@pytest.mark.parametrize("i", [2, 3], ids=[IDS[2], IDS[3]])
def test_many_pieces_equal_one(i, monkeypatch):
    w, want = LW.want(i)
    g = w.device()
    for piece in ("1", "997", "20011"):
        monkeypatch.setenv("RB_QUERY_PIECE", piece)
        texts, recs = g.correctLong(w.queries, **LW.params_of(LW.CASES[i]))
        assert [(t, r) for t, r in zip(texts, tuples(recs))] == want, piece


def test_letters_outside_acgtu_and_short_sequences():
    w, want = LW.want(0)
    g = w.device()
    # the world's queries with N / R inside and at the edge of a bad run were compared above; here: that they ask something
    with_n = [j for j, s in enumerate(w.queries) if b"N" in s or b"R" in s]
    assert len(with_n) >= 10 and sum(sum(want[j][1][F[c]] for c in CTRS) for j in with_n) >= 50
    p = LW.params_of(LW.CASES[0])
    k = w.k
    t = w.tx[0]
    short = [b"", b"A", t[:k - 1], t[:k], t[:k + 1], b"N" * k, t[:k - 1] + b"N", b"N" + t[:k + 5]]
    texts, recs = g.correctLong(short, **p)
    assert list(zip(texts, tuples(recs))) == w.expected(short, **p)
    assert [int(r["status"]) for r in recs[:3]] == [NO_KMER] * 3 and int(recs[3]["status"]) == UNCHANGED
    # no k-mer at all: nothing is launched, the texts come back
    texts, recs = g.correctLong([b"", b"ACG"], **p)
    assert texts == [b"", b"ACG"] and [int(r["status"]) for r in recs] == [NO_KMER, NO_KMER] and [int(r["out_len"]) for r in recs] == [0, 3]
    texts, recs = g.correctLong([], **p)
    assert texts == [] and recs.size == 0


def raw_call(h, queries, seq=True, off=True, oo=True, out=True, rec=True, par=True, n=None, offsets=None, out_offsets=None, **params):
    s, o = _pack(queries)
    if offsets is not None:
        o = np.asarray(offsets, np.int64)
    nq = len(queries) if n is None else n
    cap = np.zeros(len(queries) + 1, np.int64)
    np.cumsum([len(x) + 16 for x in queries], out=cap[1:])
    if out_offsets is not None:
        cap = np.asarray(out_offsets, np.int64)
    a_out, a_rec = np.full(int(max(1, cap[-1] if len(cap) else 1)) + 64, 7, np.uint8), np.full(max(1, len(queries)) * 16, 7, np.int32)
    P = dict(maxItr=2, lookahead=5, maxIndelSize=1, minKmerCov=1, minNumSolidKmers=0, trimLowCovEdges=0, windowSize=40, maxCovGradient=0.5,
             percentIdentity=0.9)
    P.update(params)
    lp = N.LongParams(P["maxItr"], P["lookahead"], P["maxIndelSize"], P["minKmerCov"], P["minNumSolidKmers"], P["trimLowCovEdges"], P["windowSize"],
                      P["maxCovGradient"], P["percentIdentity"])
    p = lambda a, use: a.ctypes.data_as(C.c_void_p) if use else None
    rc = N.lib.rb_graph_correct_long(h, p(s, seq), p(o, off), nq, C.byref(lp) if par else None, p(cap, oo), p(a_out, out), p(a_rec, rec))
    return rc, a_out, a_rec


def refused(h, queries, also=(), **kw):
    handles = [x for x in (h,) + tuple(also) if x is not None]
    before = [digests(x) for x in handles]
    rc, a_out, a_rec = raw_call(h, queries, **kw)
    assert rc == ERR_INVALID and N.lib.rb_last_error(), kw
    assert (a_out == 7).all() and (a_rec == 7).all(), kw
    assert [digests(x) for x in handles] == before, kw


def test_refusals_leave_everything_alone():
    w, _ = LW.want(0)
    g = w.device()
    queries = w.queries[:30]
    nq = len(queries)
    before = digests(g.h)
    assert raw_call(g.h, queries)[0] == 0
    rc, a_out, a_rec = raw_call(g.h, [])
    assert rc == 0 and (a_out == 7).all() and (a_rec == 7).all()              # n == 0 touches nothing
    nan, inf = float("nan"), float("inf")
    for kw in (dict(off=False), dict(oo=False), dict(out=False), dict(rec=False), dict(seq=False), dict(par=False), dict(n=-1),
               dict(maxCovGradient=nan), dict(maxCovGradient=inf), dict(percentIdentity=nan), dict(percentIdentity=-inf),
               dict(windowSize=0), dict(windowSize=-3), dict(windowSize=(1 << 20) + 1), dict(lookahead=0), dict(lookahead=-1),
               dict(lookahead=(1 << 20) + 1), dict(maxItr=-1), dict(maxIndelSize=-1), dict(maxIndelSize=4097),
               dict(windowSize=1 << 20, maxIndelSize=1023), dict(windowSize=(1 << 18) + 1, maxIndelSize=4094),   # window_size * (2 + max_indel_size) > 2^30
               dict(offsets=[0, 90, 40] + [40] * (nq - 2)), dict(out_offsets=[0, 500, 400] + [400] * (nq - 2))):
        refused(g.h, queries, **kw)
    refused(None, queries)
    assert raw_call(g.h, queries, windowSize=4096)[0] == 0 and raw_call(g.h, queries, windowSize=1 << 20)[0] == 0
    assert raw_call(g.h, queries, windowSize=4096, maxIndelSize=4096)[0] == 0 and raw_call(g.h, queries, windowSize=1 << 20, maxIndelSize=1022)[0] == 0
    assert raw_call(g.h, queries, lookahead=1 << 20)[0] == 0                  # every window is shorter: copied
    # a null seq is taken where there is no letter: no sequence, and sequences that are all empty
    assert raw_call(g.h, [], seq=False)[0] == 0
    rc, a_out, a_rec = raw_call(g.h, [b"", b""], seq=False)
    assert rc == 0 and a_rec.reshape(-1, 16)[:, 0].tolist() == [NO_KMER, NO_KMER] and a_rec.reshape(-1, 16)[:, 2].tolist() == [0, 0]
    rk = sharded.ShardRank((100_003, 200_003, 30_011, 2, 2, 2, 25, 0, 1, 0, 0, 9, 0), 0, 1, 0, "split")
    refused(rk.h, queries, also=(g.h,))                                       # a shard handle
    rk.destroy()
    for gone in ("destroyCbf", "destroyDbgbf"):
        g2 = BloomFilterDeBruijnGraph(*LW.SIZES, 2, 2, 2, w.k, False, False, rngSeed=3)
        getattr(g2, gone)()
        refused(g2.h, queries)
        g2.destroy()
    g1 = BloomFilterDeBruijnGraph(*LW.SIZES, 2, 2, 2, 1, False, False, rngSeed=3)      # k = 1 makes a graph (rb_graph_create takes 1 .. 256)
    refused(g1.h, queries)
    assert raw_call(g1.h, queries)[0] == ERR_INVALID and b"k = 1" in N.lib.rb_last_error()
    g1.destroy()
    with pytest.raises(N.NativeError):
        g.correctLong(queries, windowSize=0)
    with pytest.raises(TypeError):
        g.correctLong(queries, window=40)
    assert digests(g.h) == before


def test_the_profile_entry():
    w, want = LW.want(0)
    g = w.device()
    g.profileEnable(True)
    g.profileGet(reset=True)
    texts, recs = g.correctLong(w.queries[:60], slack=64, **LW.params_of(LW.CASES[0]))
    prof = g.profileGet()
    g.profileEnable(False)
    assert prof["correct_long"][0] > 0 and prof["correct_long"][1] == 1, prof
    assert list(zip(texts, tuples(recs))) == want[:60]


def test_the_workers_chain_is_the_three_steps_composed():
    """correctLongReads = correctLongSequenceWindowed, the seven-argument trimReverseComplementArtifact taken if not empty and shorter, and
    assembleValidKmers — each step from its own restatement / its own tested call"""
    i = 2
    w, want = LW.want(i)
    g = w.device()
    p = LW.params_of(LW.CASES[i])
    # palindromic reads for the artifact trim: a read followed by its reverse complement
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    extra = [s[:120] + s[:120].translate(comp)[::-1] for s in w.queries[:60:6] if len(s) >= 120]
    seqs = w.queries + extra
    got = graphutils.correctLongReads(g, seqs, **p)
    exp_rows = want + w.expected(extra, **p)
    corrected = [None if rec[F["status"]] in (NULL, NO_KMER) else t for t, rec in exp_rows]
    alive = [j for j, t in enumerate(corrected) if t]
    texts = [corrected[j] for j in alive]
    grad = p.get("maxCovGradient", g.LONG_DEFAULTS["maxCovGradient"])
    trimmed = graphutils.trimReverseComplementArtifact(g, texts, g.TRIM_LONG, 150, grad, keepNotJudged=True)
    before_trim = texts
    texts = [t if t and len(t) < len(s) else s for s, t in zip(texts, trimmed)]
    # the kept-only-if-not-empty-and-shorter rule is asked: hairpins are shortened, other sequences stay, and an empty result is not taken
    n_extra = sum(1 for j in alive if j >= len(w.queries))
    assert n_extra >= 5 and sum(len(t) < len(s) for s, t in zip(before_trim[-n_extra:], texts[-n_extra:])) >= 1
    assert sum(t == s for s, t in zip(before_trim, texts)) >= 100 and all(texts)
    exp = [[] for _ in seqs]
    for j, t in zip(alive, texts):
        exp[j] = assemble_valid_kmers(t, w.k, w.o)
    assert got == exp
    assert sum(len(x) == 0 for x in got) >= 3 and sum(len(x) > 1 for x in got) >= 3 and sum(len(x) == 1 for x in got) >= 100
