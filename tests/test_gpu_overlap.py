"""rb_graph_overlap_pairs (GraphUtils.overlap on the device) against the reference's lines (restated in tests/test_overlap_rules.py) run on the
CPU oracle's getKmers, a device graph and the oracle built from the same reads.  Compared field by field: outcome, why, flags, overlap, span,
out_len and the text bytes.  Stranded and canonical graphs at k = 25 and k = 21; reads inserted exactly once (singleton k-mers) whose junction
k-mers are in no read (invalid spans); a pair of one k-mer each and a short one; pairs longer than the kernel's LDS row in each role; 50 003
pairs in one call and in small pieces; the size query; every refusal with the filters' digests before and after; one rescue applied.
Before the device is asked, each world checks on the oracle alone that every outcome and every `why` is reached.  Two combinations cannot be:
a swapped LEFT or RIGHT needs the second attempt to end in a containment or at shift 0, and each such pair is already a hit of the first
attempt (its loop at shift 0, or its `right.contains(left)`)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import rbo
from rnabloom import _native as N
from rnabloom import sharded
from rnabloom.graph import BloomFilterDeBruijnGraph, _pack
import test_overlap_rules as R

ERR_INVALID = 1                     # RB_ERR_INVALID
ACGT = np.frombuffer(b"ACGT", np.uint8)
MO = 10                             # min_overlap
LDS_ROW = 1024                      # the kernel's row: pairs whose reads take more are read from device memory


class OracleSide:
    """the graph the rules file asks for, on rbo.Graph"""

    def __init__(self, og, d):
        self.og, self.d = og, d

    def counts(self, seq):
        return self.og.get_kmers(seq)[2]

    def _h0(self, kmer):
        f, r, _ = self.og.get_kmers(kmer)
        return int(f[0] if self.og.stranded or f.view(np.int64)[0] <= r.view(np.int64)[0] else r[0])

    def contains(self, kmer):
        return self.og.contains(rbo.ntm64(self._h0(kmer), self.og.k, self.og.h))

    def add_dbg_only(self, kmer):
        self.og.add_dbg_only(rbo.ntm64(self._h0(kmer), self.og.k, self.og.h))

    def add_read_paired_kmers(self, seq):
        p, _, _ = rbo.hash_pairs_region(seq, self.og.k, self.og.pk_h, self.d, rbo.FWD if self.og.stranded else rbo.CANON)
        for row in p:
            self.og.add_read_pair(row)


def put(s, pos, ch):
    b = bytearray(s); b[pos] = ord(ch); return bytes(b)


class World:
    """transcripts tiled with reads (every k-mer counts about 10), `single` transcripts of which only the two reads of one pair are inserted
    — once each, so that their k-mers count 1 and the k-mers across the junction are absent — and the pairs to ask about"""
    D = 30                          # read-paired k-mer distance
    SIZES = (2_400_011, 2_400_011, 400_009)
    # the lengths that do not follow from k by themselves, as the worlds at k = 25 and 21 have them (tests/pair_worlds.py derives them from k):
    # transcripts and the reads that tile them, the singleton transcripts and their two reads, the reads of the pairs cut from the covered
    # transcripts and where they may begin, the containments (left read, where the right read inside it begins at the latest and ends; the
    # read that is a prefix or lies in the middle of the other, and how far in), the long-* pairs (the overlap of k or more and the one
    # below k, the short read), how much longer than k the reads of the dovetail below k may be
    LENGTHS = dict(tx=500, long_tx=3000, read=100, tile=10, single_tx=300, single_read=(60, 110), pair_read=(40, 150), pair_start=150,
                   inside_left=150, inside_shift=40, inside_end=110, contained=60, middle_at=20, dovetail_span=7, long_merge=30, long_span=15, long_read=100)

    def __init__(self, k, stranded, seed, n_tx=40, n_single=48, hashes=(2, 2, 2), sizes=None, lengths=None, n_pairs=260, extra_reads=(), extra_pairs=()):
        """extra_reads go into the graph once each behind the world's own; extra_pairs: (kind, left, right) behind the world's own"""
        rng = np.random.default_rng(seed)
        self.k, self.stranded, self.rng, self.hashes = k, stranded, rng, hashes
        self.lengths = ln = dict(self.LENGTHS, **(lengths or {}))
        rnd = lambda n: ACGT[rng.integers(0, 4, n)].tobytes()
        self.tx = [rnd(ln["tx"]) for _ in range(n_tx)] + [rnd(ln["long_tx"]) for _ in range(2)]
        reads = [t[a:a + ln["read"]] for t in self.tx for a in range(0, len(t) - ln["read"] + 1, ln["tile"])]
        self.pairs, self.kind = [], []
        add = lambda kind, left, right: (self.pairs.append((left, right)), self.kind.append(kind))
        ri = lambda a, b: int(rng.integers(a, b + 1))
        # ---- singleton reads around a junction that no read covers ----
        for j in range(n_single):
            t, kind = rnd(ln["single_tx"]), j % 8
            small = kind == 6                                                   # the dovetail with fewer than k bases: reads of at most 4 (k - 1) / 3
            ll, rl = (ri(k + 3, k + 6), ri(k + 3, k + 6)) if small else (ri(*ln["single_read"]), ri(*ln["single_read"]))
            o = k - 2 if small else ri(MO, k - 1)
            if kind == 4:
                t = t[:ll - o] + (b"AC" * k)[:o] + t[ll:]                      # the shared bases are a dinucleotide repeat
            if kind == 5:
                o = k - 5; t = put(t, ll - o + 5, "N")                          # right's k-mers 6 .. and left's last but 6 are free of it
            left, right = t[:ll], t[ll - o:ll - o + rl]
            reads += [left, right] + ([right] if kind == 2 else []) + ([left] if kind == 3 else [])
            add("single%d" % kind, *((right, left) if small else (left, right)))
        # ---- pairs from the covered transcripts ----
        c_left, c_in, c_end, c_len, c_at = ln["inside_left"], ln["inside_shift"], ln["inside_end"], ln["contained"], ln["middle_at"]
        for i in range(n_pairs):
            t = self.tx[i % n_tx]
            kind = i % 13
            ll, rl = ri(*ln["pair_read"]), ri(*ln["pair_read"])
            a = ri(0, ln["pair_start"])
            if kind in (0, 1):
                o = ri(k, min(ll, rl) - 1)                                      # merged
            elif kind in (2, 3):
                o = ri(MO, k - 1)                                               # spanned
            elif kind == 4:
                o = ri(0, MO - 1)                                               # too little
            if kind <= 4:
                add("frag%d" % kind, t[a:a + ll], t[a + ll - o:a + ll - o + rl])
            elif kind == 5:
                add("other", t[a:a + ll], self.tx[(i + 7) % n_tx][a:a + rl])
            elif kind == 6:
                add("inside", t[a:a + c_left], t[a + ri(1, c_in):a + c_end])   # right in the middle of left
                add("suffix", t[a:a + c_left], t[a + c_left - rl:a + c_left])
            elif kind == 7:
                add("prefix", t[a:a + c_len], t[a:a + c_len + rl])              # left is a prefix of right
                add("middle", t[a + c_at:a + c_at + c_len], t[a:a + c_left])    # left in the middle of right: the `contains` fallback
            elif kind == 8:
                add("equal", t[a:a + ll], t[a:a + ll])
            elif kind == 9:
                n = min(ll, rl)
                o = ri(max(k, n * 3 // 4 - 2), n - 1)                           # the dovetail around the 3/4 boundary, k bases or more
                add("dovetail", t[a + ll - o:a + ll - o + rl], t[a:a + ll])
            elif kind == 10:
                ll, rl = ri(k + 1, k + ln["dovetail_span"]), ri(k + 1, k + ln["dovetail_span"])      # the dovetail with fewer than k bases shared
                o = ri(min(ll, rl) * 3 // 4 - 1, k - 1)
                add("dovetail-span", t[a + ll - o:a + ll - o + rl], t[a:a + ll])
            elif kind == 11:
                x, y, run = rnd(8), rnd(8), ri(k, k + 10)                       # a homopolymer of k or more shared (flanks short enough for the dovetail's 3/4)
                pa = (x + b"A" * run, b"A" * run + y)
                add("poly", *(pa if i % 2 else pa[::-1]))
            else:
                o = ri(MO + 2, k - 1)                                           # other letters inside the shared bases
                left, right = t[a:a + ll], t[a + ll - o:a + ll - o + rl]
                ch = "NnacgtU"[i % 7]
                add("letter-both", put(left, ll - o + 1, ch), put(right, 1, ch))
                add("letter-one", left, put(right, 1, ch.lower() if ch != "n" else "N"))
        # one k-mer each; a read below max(k, min_overlap); pairs longer than the LDS row in each role, the match at the far end
        t, big = self.tx[0], self.tx[-1]
        add("one-kmer", t[0:k], t[5:5 + k])
        add("short", t[0:k - 1], t[0:c_len])
        add("short", t[0:c_len], b"")
        om, os_, lr = ln["long_merge"], ln["long_span"], ln["long_read"]
        add("long-left", big[0:1500], big[1500 - om:1500 - om + lr])
        add("long-left-span", big[100:1500], big[1500 - os_:1500 + lr])
        add("long-right", big[100:100 + lr], big[100 + lr - om:1700])
        add("long-both", big[0:1400], big[1400 - os_:2900])
        add("long-none", big[0:1400], self.tx[-2][0:1400])
        for kind, left, right in extra_pairs:
            add(kind, left, right)
        self.reads = reads = reads + list(extra_reads)
        self.sizes = tuple(sizes or self.SIZES)
        self.og = rbo.Graph(*self.sizes, *hashes, k, stranded, True, 5)
        self.og.set_read_pair_distance(self.D)
        self.packed = rbo.pack_reads(reads, [b"I" * len(s) for s in reads])
        self.og.add_reads(*self.packed, 3, 0)
        self.o = OracleSide(self.og, self.D)
        self.gg = None
        self._want = None

    def device(self):
        if self.gg is None:
            self.gg = BloomFilterDeBruijnGraph(*self.sizes, *self.hashes, self.k, self.stranded, True, rngSeed=5)
            self.gg.setReadPairedKmerDistance(self.D)
            self.gg.addReads(*self.packed, 3)
            assert (self.gg.exportFilter(N.DBGBF) == self.og.dbgbf_bytes()).all() and (self.gg.exportFilter(N.CBF) == self.og.cbf_bytes()).all()
        return self.gg

    def want(self, mincov=1.0):
        """the restatement's records and texts, computed once"""
        if self._want is None or self._want[0] != mincov:
            self._want = (mincov, [R.expected(l, r, self.k, MO, mincov, self.o) for l, r in self.pairs])
        return self._want[1]

    def assert_every_branch_is_reached(self):
        """on the oracle alone: every outcome, unswapped and (where it can be) swapped, and every why"""
        got = {(rec[0], bool(rec[2])) for rec, _ in self.want()}
        whys = {rec[1] for rec, _ in self.want()}
        for key in [(o, False) for o in range(6)] + [(R.NONE, True), (R.MERGED, True), (R.SPANNED, True), (R.RESCUE, True)]:
            assert key in got, (key, sorted(got))
        assert whys == set(range(8)), whys
        long_paths = [rec[0] for (l, r), (rec, _) in zip(self.pairs, self.want()) if ((len(l) + 3) & ~3) + len(r) > LDS_ROW]
        assert {R.MERGED, R.SPANNED, R.NONE} <= set(long_paths), long_paths


def flat(g, pairs, mincov=1.0, mo=MO):
    (ls, lo), (rs, ro) = _pack([l for l, _ in pairs]), _pack([r for _, r in pairs])
    return g.overlapPairsFlat(ls, lo, rs, ro, mo, mincov)


def compare(pairs, want, got, label):
    out, oo, recs = got
    assert (oo == np.concatenate([[0], np.cumsum([len(l) + len(r) for l, r in pairs])])).all(), label
    for i, ((rec, text), rc) in enumerate(zip(want, recs)):
        have = tuple(int(rc[f]) for f in ("outcome", "why", "flags", "overlap", "out_len", "span_first", "span_n"))
        assert have == rec, (label, i, have, rec, pairs[i])
        assert out[oo[i]:oo[i] + rc["out_len"]].tobytes() == text, (label, i)
        assert rc["pad"] == 0


WORLDS = {}


def world(k, stranded):
    if (k, stranded) not in WORLDS:
        WORLDS[(k, stranded)] = World(k, stranded, seed=100 + k + stranded)
    return WORLDS[(k, stranded)]


@pytest.mark.parametrize("k,stranded", [(25, False), (25, True), (21, False)])
def test_overlaps_match_the_restatement_on_the_oracle(k, stranded):
    w = world(k, stranded)
    w.assert_every_branch_is_reached()
    g = w.device()
    before = [g.fold(f) for f in (N.DBGBF, N.CBF, N.RPKBF)]
    compare(w.pairs, w.want(), flat(g, w.pairs), (k, stranded))
    assert [g.fold(f) for f in (N.DBGBF, N.CBF, N.RPKBF)] == before                      # read-only
    # min_kmer_cov 2: the singletons' own k-mers would do, the spans of the covered pairs still hold
    want2 = [R.expected(l, r, k, MO, 2.0, w.o) for l, r in w.pairs]
    compare(w.pairs, want2, flat(g, w.pairs, 2.0), (k, stranded, "mincov 2"))
    # the public form
    res = g.overlapPairs([l for l, _ in w.pairs[:60]], [r.decode("latin1") for _, r in w.pairs[:60]], MO)
    assert res == [(text if rec[0] != R.NONE else None, rec[0], bool(rec[2])) for rec, text in w.want()[:60]]
    assert g.overlapPairs([], [], MO) == []


def test_fifty_thousand_pairs_and_small_pieces(monkeypatch):
    w = world(25, False)
    g = w.device()
    n = 50_003
    idx = np.arange(n) % len(w.pairs)
    pairs = [w.pairs[i] for i in idx]
    want = [w.want()[i] for i in idx]
    whole = flat(g, pairs)
    compare(pairs, want, whole, "50003")
    for piece in ("1000000", "4099"):
        monkeypatch.setenv("RB_QUERY_PIECE", piece)
        got = flat(g, pairs)
        assert all((a == b).all() for a, b in zip(got, whole)), piece
    monkeypatch.setenv("RB_QUERY_PIECE", "1")
    compare(w.pairs, w.want(), flat(g, w.pairs), "a pair a piece")


def raw_call(g, pairs, mo=MO, mincov=1.0, lseq=True, loff=True, rseq=True, roff=True, oo=True, out=True, recs=True, lo=None):
    (ls, lof), (rs, rof) = _pack([l for l, _ in pairs]), _pack([r for _, r in pairs])
    if lo is not None:
        lof = np.asarray(lo, np.int64)
    n = len(rof) - 1
    a_oo = np.full(n + 1, -1, np.int64); a_out = np.full(ls.size + rs.size + 1, 7, np.uint8); a_rec = np.full(n * 8, 7, np.int32)
    p = lambda a, use: a.ctypes.data_as(C.c_void_p) if use else None
    rc = N.lib.rb_graph_overlap_pairs(g, p(ls, lseq), p(lof, loff), p(rs, rseq), p(rof, roff), n, mo, mincov, p(a_oo, oo), p(a_out, out), p(a_rec, recs))
    return rc, a_oo, a_out, a_rec


def test_size_query_and_refusals():
    w = world(25, False)
    g = w.device()
    pairs = w.pairs[:40]
    before = [g.fold(f) for f in (N.DBGBF, N.CBF, N.RPKBF)]
    # the size query: out_offsets alone
    rc, oo, out, rec = raw_call(g.h, pairs, out=False)
    assert rc == 0 and (oo == np.concatenate([[0], np.cumsum([len(l) + len(r) for l, r in pairs])])).all()
    assert (out == 7).all() and (rec == 7).all()
    rc, oo2, out, rec = raw_call(g.h, pairs, out=False, recs=False)
    assert rc == 0 and (oo2 == oo).all()
    assert raw_call(g.h, pairs)[0] == 0
    for kw in (dict(loff=False), dict(roff=False), dict(oo=False), dict(recs=False), dict(lseq=False), dict(rseq=False), dict(mo=0), dict(mo=-3),
               dict(mincov=float("nan")), dict(mincov=float("inf")), dict(lo=[0, 90, 40] + [40] * (len(pairs) - 2))):
        rc, oo, out, rec = raw_call(g.h, pairs, **kw)
        assert rc == ERR_INVALID, kw
        assert (out == 7).all() and (rec == 7).all(), kw                                  # nothing was launched
    assert raw_call(None, pairs)[0] == ERR_INVALID
    assert raw_call(g.h, [(b"", b"")] * 3, lseq=False, rseq=False)[0] == 0                # no text: none is needed
    with pytest.raises(N.NativeError):
        g.overlapPairs([b"ACGT" * 20], [b"ACGT" * 20], 0)
    assert [g.fold(f) for f in (N.DBGBF, N.CBF, N.RPKBF)] == before
    rk = sharded.ShardRank((100_003, 200_003, 30_011, 2, 2, 2, 25, 0, 1, 0, 0, 9, 0), 0, 1, 0, "split")
    assert raw_call(rk.h, pairs)[0] == ERR_INVALID                                        # a shard handle
    for destroy in ("destroyCbf", "destroyDbgbf"):
        g2 = BloomFilterDeBruijnGraph(100_003, 200_003, 30_011, 2, 2, 2, 25, False, True)
        assert raw_call(g2.h, pairs)[0] == 0
        getattr(g2, destroy)()
        assert raw_call(g2.h, pairs)[0] == ERR_INVALID
        g2.destroy()


def test_profile_entry():
    w = world(25, True)
    g = w.device()
    g.profileEnable(True)
    flat(g, w.pairs)
    prof = g.profileGet()
    assert prof["overlap"][0] > 0 and prof["overlap"][1] == 1, prof
    g.profileEnable(False)


def test_apply_overlap_rescue_sets_what_the_reference_sets():
    """one rescued pair: the restatement runs :5018-5056 on the oracle (addDbgOnly of the missing spanning k-mers, correctMismatches with
    threshold 2, addReadPairedKmers), applyOverlapRescue does it on the device through the existing calls; dbgbf and rpkbf end up equal"""
    w = World(25, False, seed=77, n_tx=8, n_single=16)
    g = w.device()
    i = next(i for i, (rec, _) in enumerate(w.want()) if rec[0] == R.RESCUE and not rec[2])
    left, right = w.pairs[i]
    d0, p0 = w.og.dbgbf_bytes(), w.og.rpkbf_bytes()
    _, _, recs = flat(g, [w.pairs[i]])
    r = R.overlap(left, right, w.k, MO, 1.0, w.o, mutate=True)
    assert r.outcome == R.RESCUE and r.span_n > 0
    d1, p1 = w.og.dbgbf_bytes(), w.og.rpkbf_bytes()
    assert (d1 != d0).any() and (p1 != p0).any()                                          # the oracle's graph did change
    fixed = g.applyOverlapRescue(left, right, recs[0])
    assert fixed == r.fixed
    assert (g.exportFilter(N.DBGBF) == d1).all() and (g.exportFilter(N.RPKBF) == p1).all()
    assert (g.exportFilter(N.CBF) == w.og.cbf_bytes()).all()
    # judged again, the pair is an ordinary spanned overlap on both sides
    rec2, text2 = R.expected(left, right, w.k, MO, 1.0, w.o)
    assert rec2[0] == R.SPANNED
    compare([w.pairs[i]], [(rec2, text2)], flat(g, [w.pairs[i]]), "after the rescue")
    g.destroy()
