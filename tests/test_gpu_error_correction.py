"""rb_graph_correct_errors (GraphUtils.correctErrorHelper on the device) against the restatement of tests/test_error_correction_rules.py run
on the CPU oracle's filters, a device graph and the oracle built from the same reads.  Compared exactly: the corrected text, its length, the
flags, every gap record.  Reads of random transcripts at k-mer coverage of about 17 (threshold 3) come back with planted substitutions
(isolated, two within k), insertions and deletions of 1-3 bases, erroneous tips shorter and longer than lookahead, foreign letters past a
transcript's end, N's, and SNV bubbles whose candidate windows were put into the graph.  k 25 / 21, stranded / canonical, min_kmer_cov 1 / 2,
max_indel_size 1 / 3.  Over the cases every kind x outcome of a gap occurs (checked on the oracle alone).  Then: composition with
rb_graph_correct_mismatches, many pieces, two threads on one handle, the refusals, the profile entries, 50 000 sequences in one call.
World takes the read length as an argument (read_len, 150 here): tests/correction_worlds.py builds the worlds of k = 16 ... 256 from it."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import rbo
from rnabloom import _native as N
from rnabloom import sharded
from rnabloom.graph import BloomFilterDeBruijnGraph, _pack
from rnabloom.graphutils import isLowComplexityShort
from test_error_correction_rules import (CORRECTED, GAP, KEPT, LEFT_EDGE, MISMATCH, PATH, REPLACED, RIGHT_EDGE, SNV, TRIMMED, capacity,
                                         correct_errors)
from test_gpu_mismatch_correction import OracleSide as MismatchOracle
from test_gpu_mismatch_correction import other_base, plant

ERR_INVALID = 1
ACGT = np.frombuffer(b"ACGT", np.uint8)
T = 3.0
LOOKAHEAD, PID = 5, 0.9
ALL_OUTCOMES = {(LEFT_EDGE, KEPT), (LEFT_EDGE, REPLACED), (LEFT_EDGE, TRIMMED), (RIGHT_EDGE, KEPT), (RIGHT_EDGE, REPLACED), (RIGHT_EDGE, TRIMMED),
                (SNV, KEPT), (SNV, REPLACED), (PATH, KEPT), (PATH, REPLACED)}


class OracleSide(MismatchOracle):
    """the callbacks of the rules file on rbo.Graph: getKmers' hashes of a k-mer, rbo.variant for variants, rbo.neighbors for
    neighbours, rbo.get_max_coverage_path, rbo.greedy_extend"""

    def _fr(self, kmer):
        f, r, _ = self.og.get_kmers(kmer)
        return int(f[0]), int(r[0])

    def variants(self, seq, j, side):
        km = seq[j:j + self.og.k]
        f, r = self._fr(km)
        ch = km[0] if side == "L" else km[-1]                  # {,Canonical}{Left,Right}VariantsNTHashIterator: rbo.variant, side 0 = the first base
        return [self.og.get_count(rbo.variant(f, r, ch, a, self.og.k, self.og.h, not self.og.stranded, 0 if side == "L" else 1)[2]) for a in b"ACGT"]

    def has_neighbors(self, seq, j, direction):
        km = seq[j:j + self.og.k]
        f, r = self._fr(km)
        return bool((self.og.neighbors(f, r, km[0] if direction == 0 else km[-1], direction)[2] > 0).any())

    def max_cov_path(self, left, right, bound, min_cov):
        return rbo.get_max_coverage_path(self.og, left, right, bound, float(min_cov), self.og.k, low_complexity=isLowComplexityShort)

    def greedy(self, source, direction, lookahead, bound):
        return rbo.greedy_extend(self.og, source, direction, lookahead, bound, self.og.k, stranded=self.og.stranded)

    def expected_errors(self, seqs, thr, mincov, max_indel, lookahead=LOOKAHEAD, pid=PID):
        thr = np.broadcast_to(np.asarray(thr, np.float32), (len(seqs),))
        return [correct_errors(s, self.og.k, t, lookahead, max_indel, pid, mincov, self) for s, t in zip(seqs, thr)]


class World:
    """an oracle graph from reads of random transcripts, the query sets, and — built on request — the device graph from the same reads.
    read_len (150 here), tx_len and the sizes of the query sets (n_sets over N_SETS) are arguments for tests/correction_worlds.py, whose reads grow
    with k; extra_reads go into the graph as they are"""

    N_SETS = dict(isolated=30, within_k=30, indels=45, tips=60, letters=12, several=10, clean=20, bubbles=12)

    def __init__(self, k, stranded, seed, n_tx=20, n_reads=2600, sizes=(1_600_033, 1_600_033, 1009), hashes=(2, 2, 2), read_len=150, tx_len=(600, 1000),
                 n_sets=None, extra_reads=()):
        rng = np.random.default_rng(seed)
        self.k, self.stranded, self.sizes, self.rng, self.hashes, self.read_len = k, stranded, sizes, rng, hashes, read_len
        ns = dict(self.N_SETS, **(n_sets or {}))
        L = read_len
        self.tx = [ACGT[rng.integers(0, 4, int(rng.integers(*tx_len)))].tobytes() for _ in range(n_tx)]
        self.reads = []
        for _ in range(n_reads):
            t = self.tx[int(rng.integers(0, len(self.tx)))]
            a = int(rng.integers(0, len(t) - L))
            self.reads.append(t[a:a + L])
        for t in self.tx:                                      # the transcripts' ends are covered as well as their middles
            self.reads += [t[:L]] * 8 + [t[-L:]] * 8
        q = self.sets = {}
        pick = iter(self.reads[:n_reads])
        q["isolated"] = [plant(next(pick), [int(rng.integers(k + 5, L - k - 5))], rng) for _ in range(ns["isolated"])]
        q["within_k"] = []
        for _ in range(ns["within_k"]):
            m = int(rng.integers(k + 5, L - 2 * k - 5))
            q["within_k"].append(plant(next(pick), [m, m + int(rng.integers(1, k))], rng))
        q["insertions"], q["deletions"] = [], []
        for i in range(ns["indels"]):
            s, m, j = next(pick), int(rng.integers(k + 5, L - k - 8)), i % 3 + 1
            q["insertions"].append(s[:m] + ACGT[rng.integers(0, 4, j)].tobytes() + s[m:])
            s, m = next(pick), int(rng.integers(k + 5, L - k - 8))
            q["deletions"].append(s[:m] + s[m + j:])
        q["tips"] = []
        for i in range(ns["tips"]):
            s, d = next(pick), (1, 2, 3, 4, 6, 9, 14, 20)[i % 8]           # shorter and longer than lookahead
            pos = [d - 1] if i % 2 == 0 else [L - d]
            if i % 10 >= 8:                                    # a tip that is wrong throughout: the identity check fails
                pos = list(range(0, d)) if i % 2 == 0 else list(range(L - d, L))
            q["tips"].append(plant(s, pos, rng))
        q["off_the_end"] = []
        for i, t in enumerate(self.tx):                        # foreign letters before a transcript's first / past its last base
            junk = ACGT[rng.integers(0, 4, int(rng.integers(1, 12)))].tobytes()
            q["off_the_end"].append(junk + t[:L - 10] if i % 2 == 0 else t[-(L - 10):] + junk)
        q["letters"] = []
        for _ in range(ns["letters"]):
            b = bytearray(next(pick))
            for p in rng.integers(0, L, 2):
                b[p] = ord("N")
            q["letters"].append(bytes(b))
        q["several"] = [plant(next(pick), [2, L // 2, L - 3], rng) for _ in range(ns["several"])]
        q["clean"] = [next(pick) for _ in range(ns["clean"])] + [b"", b"ACGT", self.tx[0][:k], self.tx[0][:k + 1], ACGT[rng.integers(0, 4, 80)].tobytes()]
        # SNV bubbles that can be refilled: the k + 2 windows of left + n + right of a planted substitution are put into the graph twice
        q["bubbles"] = []
        for _ in range(ns["bubbles"]):
            s, m = next(pick), int(rng.integers(k + 5, L - k - 5))
            bad = plant(s, [m], rng)
            g = m - k + 1
            cand = bad[g:g + k] + ACGT[rng.integers(0, 4, 1)].tobytes() + bad[g + k - 1:g + 2 * k - 1]
            self.reads += [cand] * 2
            q["bubbles"].append(bad)
        self.reads += list(extra_reads)
        self.og = rbo.Graph(*sizes, *hashes, k, stranded, True, 5)
        self.packed = rbo.pack_reads(self.reads, [b"I" * len(s) for s in self.reads])
        self.og.add_reads(*self.packed, 3, 0)
        self.o = OracleSide(self.og)
        self.gg = None

    def all_queries(self):
        return sum(self.sets.values(), [])

    def device(self):
        if self.gg is None:
            self.gg = BloomFilterDeBruijnGraph(*self.sizes, *self.hashes, self.k, self.stranded, True, rngSeed=5)
            self.gg.addReads(*self.packed, 3)
            assert (self.gg.exportFilter(N.DBGBF) == self.og.dbgbf_bytes()).all() and (self.gg.exportFilter(N.CBF) == self.og.cbf_bytes()).all()
        return self.gg


CASES = [  # k, stranded, min_kmer_cov, max_indel_size
    (25, False, 1.0, 1), (25, True, 2.0, 3), (21, False, 2.0, 3), (21, True, 1.0, 1), (25, False, 1.0, 3), (21, True, 2.0, 1)]


@functools.lru_cache(maxsize=None)
def case(k, stranded, mincov, max_indel):
    """the world of a case and what the restatement makes of all its queries (computed once: the branch-coverage test shares it)"""
    w = World(k, stranded, seed=k * 7 + stranded + 100 * max_indel + int(mincov))
    return w, w.o.expected_errors(w.all_queries(), T, mincov, max_indel)


def outcome_counts(want):
    cnt = {}
    for _, _, recs in want:
        for r in recs:
            cnt[(r["kind"], r["outcome"])] = cnt.get((r["kind"], r["outcome"]), 0) + 1
    return cnt


def compare(g, seqs, want, thr, mincov, max_indel, label, lookahead=LOOKAHEAD, pid=PID):
    seq, off = _pack(seqs)
    out, oo, ol, fl, rec, go = g.correctErrorsFlat(seq, off, thr, lookahead, max_indel, pid, mincov, gaps=True)
    assert (np.diff(oo) == [capacity(len(s), g.k, max_indel) for s in seqs]).all(), label
    for i, (s, f, recs) in enumerate(want):
        assert out[oo[i]:oo[i] + ol[i]].tobytes() == s, (label, i, recs, rec[go[i]:go[i + 1]])
        assert int(ol[i]) == len(s) and int(fl[i]) == f, (label, i, int(fl[i]), f)
        got = rec[go[i]:go[i + 1]]
        assert len(got) == len(recs), (label, i)
        for a, b in zip(got, recs):
            assert (int(a["seq"]), int(a["first"]), int(a["run"]), int(a["repl_len"]), int(a["kind"]), int(a["outcome"])) == (
                i, b["first"], b["run"], b["repl_len"], b["kind"], b["outcome"]), (label, i, a, b)
    # without the records: the same text
    out2, oo2, ol2, fl2, none, _ = g.correctErrorsFlat(seq, off, thr, lookahead, max_indel, pid, mincov)
    assert none is None and (out2 == out).all() and (ol2 == ol).all() and (fl2 == fl).all() and (oo2 == oo).all()
    return out, oo, ol, fl, rec, go


def test_every_kind_and_outcome_occurs():
    """a condition on the inputs, met by the restatement alone"""
    total = {}
    for c in CASES:
        for key, v in outcome_counts(case(*c)[1]).items():
            total[key] = total.get(key, 0) + v
    print("kind x outcome:", sorted(total.items()))
    assert set(total) == ALL_OUTCOMES, sorted(ALL_OUTCOMES - set(total))


@pytest.mark.parametrize("k,stranded,mincov,max_indel", CASES)
def test_corrections_match_the_oracle(k, stranded, mincov, max_indel):
    w, want = case(k, stranded, mincov, max_indel)
    cnt = outcome_counts(want)
    print("k=%d stranded=%d mincov=%g max_indel=%d: %s, %d of %d sequences corrected" % (
        k, stranded, mincov, max_indel, sorted(cnt.items()), sum(bool(f & CORRECTED) for _, f, _ in want), len(want)))
    assert sum(bool(f & GAP) for _, f, _ in want) >= 60 and sum(bool(f & MISMATCH) for _, f, _ in want) >= 20
    g = w.device()
    seqs = w.all_queries()
    compare(g, seqs, want, T, mincov, max_indel, "all")
    # per-sequence thresholds, another lookahead and identity
    thr = np.linspace(0.0, 8.0, len(seqs)).astype(np.float32)
    sub = list(range(0, len(seqs), 3))
    some = [seqs[i] for i in sub]
    compare(g, some, w.o.expected_errors(some, thr[sub], mincov, max_indel, lookahead=3, pid=0.97), thr[sub], mincov, max_indel, "thr", lookahead=3, pid=0.97)
    # the public form
    pub = g.correctErrors(seqs[:50], T, LOOKAHEAD, max_indel, PID, mincov)
    assert pub == [(s, bool(f & CORRECTED)) for s, f, _ in want[:50]]
    assert g.correctErrors([], T) == []


def test_composition_with_the_mismatch_pass():
    """inputs without gaps to repair — isolated substitutions make an SNV gap that is kept — come out as rb_graph_correct_mismatches makes them"""
    w, want = case(*CASES[0])
    g = w.device()
    seqs = w.sets["isolated"] + w.sets["clean"]
    seq, off = _pack(seqs)
    out, oo, ol, fl, rec, go = g.correctErrorsFlat(seq, off, T, LOOKAHEAD, 1, PID, 1.0, gaps=True)
    assert not (fl & GAP).any() and (rec["outcome"] == KEPT).all()
    mm, nf, _, _ = g.correctMismatchesFlat(seq, off, T, 1.0)
    assert nf.sum() >= 20
    for i in range(len(seqs)):
        assert out[oo[i]:oo[i] + ol[i]].tobytes() == mm[off[i]:off[i + 1]].tobytes()
        assert bool(fl[i] & MISMATCH) == (nf[i] > 0) == bool(fl[i] & CORRECTED)


def flat(w, seqs, max_indel=1, mincov=1.0):
    seq, off = _pack(seqs)
    return w.device().correctErrorsFlat(seq, off, T, LOOKAHEAD, max_indel, PID, mincov, gaps=True)


def same(a, b):
    return all((x == y).all() for x, y in zip(a, b))


def test_many_pieces_equal_one(monkeypatch):
    w, want = case(*CASES[0])
    seqs = w.all_queries()
    whole = flat(w, seqs)
    assert (whole[3] & GAP).sum() > 60
    for piece in ("1", "97", "5000"):
        monkeypatch.setenv("RB_QUERY_PIECE", piece)
        assert same(flat(w, seqs), whole), piece


def test_two_threads_on_one_handle():
    w, want = case(*CASES[1])
    a = w.sets["tips"] + w.sets["insertions"] + w.sets["bubbles"]
    b = w.sets["deletions"] + w.sets["within_k"] + w.sets["off_the_end"] + w.sets["letters"]
    ra, rb_ = flat(w, a, 3, 2.0), flat(w, b, 3, 2.0)
    res, errs = {}, []

    def work(name, seqs):
        try:
            for _ in range(5):
                res[name] = flat(w, seqs, 3, 2.0)
        except Exception as e:                     # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=("a", a)), threading.Thread(target=work, args=("b", b))]
    for t in ts: t.start()
    for t in ts: t.join()
    assert not errs, errs
    assert same(res["a"], ra) and same(res["b"], rb_)


def raw_call(g, seqs, thr=None, params=(5, 1, 0.9, 1.0), seq=True, offsets=True, thresholds=True, p=True, oo=True, out=True, olen=True, flags=True,
             gaps=False, gap_offsets=False, off=None):
    s, o = _pack(seqs)
    if off is not None:
        o = np.asarray(off, np.int64)
    n = len(o) - 1
    t = np.full(n, 3.0, np.float32) if thr is None else np.asarray(thr, np.float32)
    pr = N.CorrParams(*params)
    a_oo = np.zeros(n + 1, np.int64); a_out = np.zeros(1 << 16, np.uint8); a_len = np.zeros(n, np.int32); a_fl = np.zeros(n, np.uint32)
    a_gaps = np.zeros(1 << 12, BloomFilterDeBruijnGraph.GAP_DTYPE); a_go = np.zeros(n + 1, np.int64)
    ptr = lambda a, use: a.ctypes.data_as(C.c_void_p) if use else None
    return N.lib.rb_graph_correct_errors(g, ptr(s, seq), ptr(o, offsets), n, ptr(t, thresholds), C.byref(pr) if p else None, ptr(a_oo, oo), ptr(a_out, out),
                                         ptr(a_len, olen), ptr(a_fl, flags), ptr(a_gaps, gaps), ptr(a_go, gap_offsets))


def test_refusals():
    s = [b"ACGT" * 60, b"ACGTTGCA" * 20]
    g = BloomFilterDeBruijnGraph(100_003, 200_003, 30_011, 2, 2, 2, 25, False, True)
    assert raw_call(g.h, s) == 0
    assert raw_call(g.h, s, gaps=True, gap_offsets=True) == 0
    assert raw_call(g.h, s, out=False, olen=False, flags=False) == 0          # the size query
    assert raw_call(g.h, s, gap_offsets=True) == 0
    assert raw_call(None, s) == ERR_INVALID
    for name in ("offsets", "thresholds", "p", "oo", "olen", "flags", "seq"):
        assert raw_call(g.h, s, **{name: False}) == ERR_INVALID, name
    assert raw_call(g.h, s, gaps=True) == ERR_INVALID                         # gaps without gap_offsets
    for bad in (np.nan, np.inf, -np.inf):
        assert raw_call(g.h, s, thr=[3.0, bad]) == ERR_INVALID
        assert raw_call(g.h, s, params=(5, 1, bad, 1.0)) == ERR_INVALID
        assert raw_call(g.h, s, params=(5, 1, 0.9, bad)) == ERR_INVALID
    for la in (0, -1, 17):
        assert raw_call(g.h, s, params=(la, 1, 0.9, 1.0)) == ERR_INVALID
    assert raw_call(g.h, s, params=(1, 0, 0.9, 1.0)) == 0 and raw_call(g.h, s, params=(16, 0, 0.9, 1.0)) == 0
    assert raw_call(g.h, s, params=(5, -1, 0.9, 1.0)) == ERR_INVALID and raw_call(g.h, s, params=(5, 4097, 0.9, 1.0)) == ERR_INVALID
    assert raw_call(g.h, s, thr=[-1.0, 0.0]) == 0                             # T <= 0 is no refusal: nothing is below it
    assert raw_call(g.h, s, off=[0, 240, 100]) == ERR_INVALID                 # decreasing offsets
    with pytest.raises(N.NativeError):
        g.correctErrors(s, float("nan"))
    g.destroyCbf()
    assert raw_call(g.h, s) == ERR_INVALID
    g.destroy()
    g = BloomFilterDeBruijnGraph(100_003, 200_003, 30_011, 2, 2, 2, 25, False, True)
    g.destroyDbgbf()
    assert raw_call(g.h, s) == ERR_INVALID
    g.destroy()
    g = BloomFilterDeBruijnGraph(100_003, 200_003, 30_011, 2, 2, 2, 1, False, True)
    assert raw_call(g.h, s) == ERR_INVALID                                    # k < 2
    g.destroy()
    rk = sharded.ShardRank((100_003, 200_003, 30_011, 2, 2, 2, 25, 0, 1, 0, 0, 9, 0), 0, 1, 0, "split")
    assert raw_call(rk.h, s) == ERR_INVALID                                   # a shard handle


def test_profile_entries():
    w, want = case(*CASES[0])
    g = w.device()
    g.profileEnable(True)
    g.profileGet(reset=True)
    flat(w, w.all_queries())
    prof = g.profileGet()
    assert prof["correct_errors"][0] > 0 and prof["correct_errors"][1] == 1, prof
    for name in ("profile", "scan", "walks", "resolve", "stitch", "mismatch"):
        assert prof["correct_errors." + name][0] > 0, (name, prof)
    g.profileEnable(False)


def test_fifty_thousand_sequences_in_one_call():
    """a wavefront per sequence and per gap: 2 000 distinct planted reads — a substitution anywhere, every third also an insertion or a
    deletion — 25 times over, and a few whole transcripts with several errors, in one call"""
    w, _ = case(*CASES[0])
    rng = np.random.default_rng(50)
    base = []
    for i, s in enumerate(w.reads[:2000]):
        b = plant(s, [int(rng.integers(0, len(s)))], rng)
        if i % 3 == 0 and len(b) > 100:
            m = int(rng.integers(30, len(b) - 40))
            b = b[:m] + b[m + 1:] if i % 2 else b[:m] + b"G" + b[m:]
        base.append(b)
    long_ = [plant(t, [100, 300, 310, len(t) - 3], rng) for t in w.tx[:4]]
    want = w.o.expected_errors(base + long_, T, 1.0, 1)
    assert sum(bool(f & CORRECTED) for _, f, _ in want) * 2 >= len(want)
    seqs = base * 25 + long_
    want = want[:2000] * 25 + want[2000:]
    assert len(seqs) >= 50_000
    compare(w.device(), seqs, want, T, 1.0, 1, "50k")
