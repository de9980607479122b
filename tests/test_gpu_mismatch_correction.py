"""rb_graph_correct_mismatches (GraphUtils.correctMismatches on the device) against the reference's two loops (restated in
tests/test_mismatch_rules.py) run on the CPU oracle's getKmers / contains, a device graph and the oracle built from the same reads.
Compared exactly: the corrected bytes, n_fixed, koffsets, the final count rows — and those rows against rb_graph_kmers of the output.
Stranded and canonical graphs, k 25 / 35 / 47, min_kmer_cov 1 / 2 / 0, one threshold for all and coverageStats' se_threshold per
sequence, many pieces, every refusal, two threads on one handle, and 50 000 sequences in one call.  Before the device is asked each case
checks on the oracle alone that the fixture is not vacuous: most planted substitutions are replaced, some by the reverse scan only.
World takes the read length as an argument (read_len, 250 here): tests/correction_worlds.py builds the worlds of k = 16 ... 256 from it."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import rbo
from rnabloom import _native as N
from rnabloom import sharded
from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch, _pack
from test_mismatch_rules import correct_mismatches, forward_only

ERR_INVALID = 1                     # RB_ERR_INVALID
ACGT = np.frombuffer(b"ACGT", np.uint8)


def other_base(b, rng):
    return b"ACGT"[(b"ACGT".index(b) + 1 + int(rng.integers(0, 3))) % 4]


def plant(s, positions, rng):
    b = bytearray(s)
    for p in positions:
        b[p] = other_base(b[p], rng)
    return bytes(b)


class OracleSide:
    """the two callbacks of the rules file on rbo.Graph: contains(k-mer) = the dbgbf lookup of the k-mer's hashes as getKmers hashes a raw
    string, counts(sequence) = getKmers' counts"""

    def __init__(self, og):
        self.og = og

    def contains(self, kmer):
        f, r, _ = self.og.get_kmers(kmer)
        h0 = f[0] if self.og.stranded or f.view(np.int64)[0] <= r.view(np.int64)[0] else r[0]
        return self.og.contains(rbo.ntm64(int(h0), self.og.k, self.og.h))

    def counts(self, seq):
        return self.og.get_kmers(seq)[2]

    def expected(self, seqs, thr, mincov):
        thr = np.broadcast_to(np.asarray(thr, np.float32), (len(seqs),))
        return [correct_mismatches(s, self.counts(s), self.og.k, t, mincov, self.contains, self.counts) for s, t in zip(seqs, thr)]

    def forward(self, seqs, thr, mincov):
        return [forward_only(s, self.counts(s), self.og.k, thr, mincov, self.contains, self.counts) for s in seqs]


class World:
    """an oracle graph from reads of random transcripts (250 bases each, k-mer coverage about 20), plus six copies each of a few erroneous k-mers: the
    k-mer that ENDS with a planted substitution, which makes the forward scan's candidate one window late (it aims at the wrong base) and
    leaves the substitution to the reverse scan.  The device graph is built from the same reads on request.  read_len, tx_len and the numbers
    of planted sequences are arguments for tests/correction_worlds.py, whose reads grow with k; extra_reads go into the graph as they are."""
    T = 3.0

    def __init__(self, k, stranded, seed, n_tx=24, n_reads=3200, sizes=(1_600_033, 1_600_033, 1009), hashes=(2, 2, 2), read_len=250, tx_len=(900, 1500),
                 n_planted=240, n_rev=40, extra_reads=()):
        rng = np.random.default_rng(seed)
        self.k, self.stranded, self.sizes, self.rng, self.hashes, self.read_len = k, stranded, sizes, rng, hashes, read_len
        self.tx = [ACGT[rng.integers(0, 4, int(rng.integers(*tx_len)))].tobytes() for _ in range(n_tx)]
        self.reads = []
        for _ in range(n_reads):
            t = self.tx[int(rng.integers(0, len(self.tx)))]
            a = int(rng.integers(0, len(t) - read_len))
            self.reads.append(t[a:a + read_len])
        # planted-substitution queries: one in the middle, one near each end, two far apart, two within k, three
        self.planted, self.rev_only = [], []
        for i, s in enumerate(self.reads[:n_planted]):
            kind = i % 6
            L = len(s)
            pos = ([int(rng.integers(k, L - k))], [int(rng.integers(0, k))], [int(rng.integers(L - k, L))],
                   [k + 2, L - k - 3], [L // 2, L // 2 + int(rng.integers(1, k))], [k + 1, L // 2, L - k - 2])[kind]
            self.planted.append(plant(s, pos, rng))
        for s in self.reads[n_planted:n_planted + n_rev]:    # ... and the ones kept for the reverse scan
            m = int(rng.integers(k + 2, len(s) - k - 2))
            bad = plant(s, [m], rng)
            self.rev_only.append(bad)
            self.reads += [bad[m - k + 1:m + 1]] * 6
        self.reads += list(extra_reads)
        self.og = rbo.Graph(*sizes, *hashes, k, stranded, True, 5)
        self.packed = rbo.pack_reads(self.reads, [b"I" * len(s) for s in self.reads])
        self.og.add_reads(*self.packed, 3, 0)
        self.o = OracleSide(self.og)
        self.gg = None

    def device(self):
        if self.gg is None:
            self.gg = BloomFilterDeBruijnGraph(*self.sizes, *self.hashes, self.k, self.stranded, True, rngSeed=5)
            self.gg.addReads(*self.packed, 3)
            assert (self.gg.exportFilter(N.DBGBF) == self.og.dbgbf_bytes()).all() and (self.gg.exportFilter(N.CBF) == self.og.cbf_bytes()).all()
        return self.gg

    def query_sets(self):
        k, rng = self.k, self.rng
        reads = self.reads[300:420]
        chim, half = [], self.read_len * 4 // 5

        for i in range(30):
            a, b = self.tx[i % len(self.tx)], self.tx[(i + 5) % len(self.tx)]
            x, y = int(rng.integers(0, len(a) - half)), int(rng.integers(0, len(b) - half))
            chim.append(a[x:x + half] + b[y:y + half])
        letters = []
        for s in self.reads[420:520]:
            b = bytearray(s)
            for p in rng.integers(0, len(b), 2):
                b[p] = b"NKMSWYRnacgtuU"[int(rng.integers(0, 14))]
            letters.append(bytes(b))
        lower = [s.lower() for s in self.planted[:12]] + [s.replace(b"T", b"U") for s in self.planted[12:24]]
        short = [self.planted[i][:L] for i, L in enumerate([0, 1, k - 1, k, k + 1, 2 * k, 2 * k + 1, 2 * k + 2, 3 * k])]
        long_ = [plant(t, [len(t) // 3, 2 * len(t) // 3], rng) for t in self.tx[:4]]
        return {"planted": self.planted, "reverse": self.rev_only, "untouched": reads, "chimeras": chim, "letters": letters,
                "case": lower, "short": short, "transcripts": long_}

    def assert_not_vacuous(self, mincov):
        """on the oracle alone: at least half of the planted-substitution sequences change, and at least one sequence is changed by the
        reverse scan only"""
        seqs = self.planted + self.rev_only
        full = self.o.expected(seqs, self.T, mincov)
        fwd = self.o.forward(seqs, self.T, mincov)
        changed = sum(n > 0 for _, n, _ in full)
        reverse_only = sum(n > 0 and fn == 0 for (_, n, _), (_, fn) in zip(full, fwd))
        assert changed * 2 >= len(seqs), (changed, len(seqs))
        assert reverse_only >= 1, reverse_only
        return changed, reverse_only


def check(w, seqs, thr, mincov, label):
    g = w.device()
    want = w.o.expected(seqs, thr, mincov)
    seq, off = _pack(seqs)
    out, nf, ko, cnt = g.correctMismatchesFlat(seq, off, thr, mincov, counts=True)
    nk = [max(0, len(s) - w.k + 1) for s in seqs]
    assert (ko == np.concatenate([[0], np.cumsum(nk)])).all(), label
    for i, (s, n, c) in enumerate(want):
        assert out[off[i]:off[i + 1]].tobytes() == s, (label, i, n, int(nf[i]))
        assert int(nf[i]) == n, (label, i)
        assert (cnt[ko[i]:ko[i + 1]] == c).all(), (label, i)
    # the final rows are getKmers of the output
    outs = [out[off[i]:off[i + 1]].tobytes() for i in range(len(seqs))]
    assert (g.getKmers(outs)[3] == cnt).all(), label
    # without the count rows: the same text
    out2, nf2, _, none = g.correctMismatchesFlat(seq, off, thr, mincov)
    assert none is None and (out2 == out).all() and (nf2 == nf).all()
    return want


CASES = [  # k, stranded, min_kmer_cov
    (25, False, 1.0), (25, True, 2.0), (35, False, 0.0), (35, True, 1.0), (47, False, 2.0), (47, True, 0.0)]


@pytest.mark.parametrize("k,stranded,mincov", CASES)
def test_corrections_match_the_oracle(k, stranded, mincov):
    w = World(k, stranded, seed=k * 3 + stranded)
    changed, reverse_only = w.assert_not_vacuous(mincov)
    print("k=%d stranded=%d mincov=%g: %d of %d planted sequences change, %d by the reverse scan only" % (
        k, stranded, mincov, changed, len(w.planted) + len(w.rev_only), reverse_only))
    g = w.device()
    for name, seqs in w.query_sets().items():
        want = check(w, seqs, World.T, mincov, (name, "fixed"))
        if name == "untouched":
            assert sum(n for _, n, _ in want) <= len(seqs) // 10         # what stage 1 inserted is solid (a thin k-mer here and there aside)
        # per-sequence thresholds from the coverage statistics of the same sequences: the two features chain
        seq, off = _pack(seqs)
        if len(seq):
            rec, _ = g.coverageStats(ReadBatch.from_ascii(seq, None, off, 0), maxCovGradient=0.5, covFPR=0.0)
            check(w, seqs, rec["se_threshold"].copy(), mincov, (name, "se_threshold"))
    # the public form, scalar and per-sequence thresholds
    want = w.o.expected(w.planted[:40], World.T, mincov)
    assert g.correctMismatches(w.planted[:40], World.T, mincov) == [(s, n) for s, n, _ in want]
    thr = np.linspace(0.0, 8.0, 40).astype(np.float32)
    want = w.o.expected(w.planted[:40], thr, mincov)
    assert g.correctMismatches([s.decode() for s in w.planted[:40]], thr, mincov) == [(s, n) for s, n, _ in want]
    assert g.correctMismatches([], 3.0) == []
    g.destroy()


def flat(w, seqs, thr=World.T, mincov=1.0):
    seq, off = _pack(seqs)
    return w.device().correctMismatchesFlat(seq, off, thr, mincov, counts=True)


def test_many_pieces_equal_one(monkeypatch):
    w = World(25, False, seed=7)
    w.assert_not_vacuous(1.0)
    seqs = sum(w.query_sets().values(), [])
    whole = flat(w, seqs)
    assert whole[1].sum() > 100
    for piece in ("1", "97", "5000"):
        monkeypatch.setenv("RB_QUERY_PIECE", piece)
        got = flat(w, seqs)
        assert all((a == b).all() for a, b in zip(got, whole)), piece
    w.gg.destroy()


def test_two_threads_on_one_handle():
    w = World(25, True, seed=9)
    w.assert_not_vacuous(1.0)
    sets = w.query_sets()
    a, b = sets["planted"] + sets["reverse"], sets["letters"] + sets["transcripts"] + sets["chimeras"]
    ra, rb_ = flat(w, a), flat(w, b)
    res, errs = {}, []

    def work(name, seqs):
        try:
            for _ in range(6):
                res[name] = flat(w, seqs)
        except Exception as e:                     # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=("a", a)), threading.Thread(target=work, args=("b", b))]
    for t in ts: t.start()
    for t in ts: t.join()
    assert not errs, errs
    assert all((x == y).all() for x, y in zip(res["a"], ra)) and all((x == y).all() for x, y in zip(res["b"], rb_))
    w.gg.destroy()


def raw_call(g, seqs, thr=None, mincov=1.0, seq=True, offsets=True, thresholds=True, out=True, nfixed=True, koffsets=True, counts=False, off=None):
    s, o = _pack(seqs)
    if off is not None:
        o = np.asarray(off, np.int64)
    n = len(o) - 1
    t = np.full(n, 3.0, np.float32) if thr is None else np.asarray(thr, np.float32)
    a_out = np.zeros(max(s.size, 1), np.uint8); a_nf = np.zeros(n, np.int32); a_ko = np.zeros(n + 1, np.int64); a_c = np.zeros(1 << 16, np.float32)
    p = lambda a, use: a.ctypes.data_as(C.c_void_p) if use else None
    return N.lib.rb_graph_correct_mismatches(g, p(s, seq), p(o, offsets), n, p(t, thresholds), mincov, p(a_out, out), p(a_nf, nfixed),
                                             p(a_ko, koffsets), p(a_c, counts))


def test_refusals():
    s = [b"ACGT" * 60, b"ACGTTGCA" * 20]
    g = BloomFilterDeBruijnGraph(100_003, 200_003, 30_011, 2, 2, 2, 25, False, True)
    assert raw_call(g.h, s) == 0
    assert raw_call(g.h, s, counts=True) == 0
    assert raw_call(None, s) == ERR_INVALID
    assert raw_call(g.h, s, offsets=False) == ERR_INVALID
    assert raw_call(g.h, s, thresholds=False) == ERR_INVALID
    assert raw_call(g.h, s, out=False) == ERR_INVALID
    assert raw_call(g.h, s, nfixed=False) == ERR_INVALID
    assert raw_call(g.h, s, seq=False) == ERR_INVALID
    assert raw_call(g.h, s, counts=True, koffsets=False) == ERR_INVALID
    assert raw_call(g.h, s, koffsets=False) == 0                              # both are optional
    for bad in (np.nan, np.inf, -np.inf):
        assert raw_call(g.h, s, thr=[3.0, bad]) == ERR_INVALID
        assert raw_call(g.h, s, mincov=bad) == ERR_INVALID
    assert raw_call(g.h, s, thr=[-1.0, 0.0]) == 0                             # T <= 0 is no refusal: nothing is below it
    assert raw_call(g.h, s, off=[0, 240, 100]) == ERR_INVALID                 # decreasing offsets
    with pytest.raises(N.NativeError):
        g.correctMismatches(s, float("nan"))
    g.destroyCbf()
    assert raw_call(g.h, s) == ERR_INVALID
    g.destroy()
    g = BloomFilterDeBruijnGraph(100_003, 200_003, 30_011, 2, 2, 2, 25, False, True)
    g.destroyDbgbf()
    assert raw_call(g.h, s) == ERR_INVALID
    g.destroy()
    rk = sharded.ShardRank((100_003, 200_003, 30_011, 2, 2, 2, 25, 0, 1, 0, 0, 9, 0), 0, 1, 0, "split")
    assert raw_call(rk.h, s) == ERR_INVALID                                   # a shard handle


def test_profile_entry():
    w = World(25, False, seed=11, n_reads=1600)
    g = w.device()
    g.profileEnable(True)
    flat(w, w.planted)
    prof = g.profileGet()
    assert prof["mismatches"][0] > 0 and prof["mismatches"][1] == 1, prof
    g.destroy()


def test_fifty_thousand_sequences_in_one_call():
    """a wavefront per sequence: 50 000 sequences are several wavefronts per SIMD on every CU.  Every inserted read comes back with one
    planted substitution; a few whole transcripts of more than 4096 k-mers take the path whose count row lives in device memory."""
    k = 25
    rng = np.random.default_rng(50)
    tx = [ACGT[rng.integers(0, 4, int(rng.integers(1200, 1800)))].tobytes() for _ in range(200)]
    tx += [ACGT[rng.integers(0, 4, 6000)].tobytes() for _ in range(3)]
    reads = []
    for _ in range(50_000):
        t = tx[int(rng.integers(0, len(tx)))]
        a = int(rng.integers(0, len(t) - 150))
        reads.append(t[a:a + 150])
    reads += tx[-3:] * 4
    sizes = (8_000_009, 8_000_009, 1009)
    og = rbo.Graph(*sizes, 2, 2, 2, k, False, True, 5)
    packed = rbo.pack_reads(reads, [b"I" * len(s) for s in reads])
    og.add_reads(*packed, 3, 0)
    pos = rng.integers(0, 150, 50_000)
    queries = [plant(s, [int(p)], rng) for s, p in zip(reads[:50_000], pos)]
    queries += [plant(t, [1000, 3000, 3010, 5000], rng) for t in tx[-3:]]
    o = OracleSide(og)
    want = o.expected(queries, 3.0, 1.0)
    assert sum(n > 0 for _, n, _ in want) * 2 >= len(queries)
    g = BloomFilterDeBruijnGraph(*sizes, 2, 2, 2, k, False, True, rngSeed=5)
    g.addReads(*packed, 3)
    assert (g.exportFilter(N.DBGBF) == og.dbgbf_bytes()).all() and (g.exportFilter(N.CBF) == og.cbf_bytes()).all()
    seq, off = _pack(queries)
    out, nf, ko, cnt = g.correctMismatchesFlat(seq, off, 3.0, 1.0, counts=True)
    assert (nf == [n for _, n, _ in want]).all()
    assert out.tobytes() == b"".join(s for s, _, _ in want)
    assert (cnt == np.concatenate([c for _, _, c in want])).all()
    g.destroy()
