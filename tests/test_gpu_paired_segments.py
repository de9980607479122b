"""rb_graph_paired_kmer_segments (breakWithReadPairedKmers / breakWithFragPairedKmers / pairedKmerSupport) against the reference's loops
(restated in tests/test_paired_segment_rules.py) run on support taken from the CPU oracle: the oracle's getKmers hashes -> pair keys
-> its pair filters.  Segments, counts and support bytes are compared exactly, for stranded and canonical graphs, k 25 and 35, 1-3 pair
hashes, small and realistic distances, several numPairsRequired, whole lists and ranges, many pieces, and every refusal.  The hand-worked
support patterns of the rules file are planted in a pair filter and read back.  One invariant at size: every read stage 1 inserted its
pairs from comes back as one segment over its whole k-mer list."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import rbo
from rnabloom import _native as N
from rnabloom import sharded
from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch, _pack
from test_paired_segment_rules import break_range, capacity, pattern


ERR_INVALID = 1                     # RB_ERR_INVALID
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def combine(a, b):
    with np.errstate(over="ignore"):
        return a ^ (b + np.uint64(0xFFFFFFFF9E3779B9) + (a << np.uint64(6)) + (b >> np.uint64(2)))


def pair_keys(f, r, d, stranded):
    """Kmer.getKmerPairHashValue of positions [0, nk - d) (R/graph/Kmer.java:65-67, CanonicalKmer.java:61-72: the SIGNED min)"""
    if f.size <= d:
        return np.zeros(0, np.uint64)
    x = combine(f[:-d], f[d:])
    if stranded:
        return x
    y = combine(r[d:], r[:-d])
    return np.where(y.view(np.int64) < x.view(np.int64), y, x)


def filter_lookup(bits, size, num_hash, k, keys):
    """BloomFilter.lookup of each key on the oracle's filter bytes: NTM64 expansion, (h >>> 1) % size, bit i of byte i >> 3"""
    hit = np.ones(keys.size, bool)
    kmul = np.uint64((k * 0x90B45D39FB6DA1FA) & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        for j in range(num_hash):
            h = keys if j == 0 else keys * (np.uint64(j) ^ kmul)
            if j:
                h = h ^ (h >> np.uint64(27))
            i = (h >> np.uint64(1)) % np.uint64(size)
            hit &= ((bits[(i >> np.uint64(3)).astype(np.int64)] >> (i & np.uint64(7)).astype(np.uint8)) & 1).astype(bool)
    return hit


class World:
    """a device graph and the oracle built from the same reads (storeReadPairedKmers) and fragments (addFragments).  hashes: the numbers of
    hash functions of dbgbf, cbf and the pair filters ((2, 2, pk_h) unless given; its last entry then is pk_h).  device False: the oracle alone."""

    def __init__(self, k, stranded, pk_h, read_d, frag_d, seed, hashes=None, device=True):
        rng = np.random.default_rng(seed)
        self.hashes = hashes = (2, 2, pk_h) if hashes is None else tuple(hashes)
        pk_h = hashes[2]
        self.k, self.stranded, self.pk_h, self.read_d, self.frag_d = k, stranded, pk_h, read_d, frag_d
        self.tx = [ACGT[rng.integers(0, 4, int(rng.integers(800, 1600)))].tobytes() for _ in range(30)]
        left, right = [], []
        for _ in range(2500):
            t = self.tx[int(rng.integers(0, len(self.tx)))]
            a = int(rng.integers(0, len(t) - 300))
            left.append(t[a:a + 150]); right.append(t[a + 150:a + 300][::-1].translate(COMP))
        self.left, self.right = left, right
        self.sizes = (400_009, 1_000_003, 2_000_003)
        self.og = rbo.Graph(*self.sizes, *hashes, k, stranded, True, 5)
        self.gg = BloomFilterDeBruijnGraph(*self.sizes, *hashes, k, stranded, True, rngSeed=5) if device else None
        self.og.set_read_pair_distance(read_d)
        if device:
            self.gg.setReadPairedKmerDistance(read_d)
        for reads, rc in ((left, False), (right, True)):
            seq, q, off = rbo.pack_reads(reads, [b"I" * len(s) for s in reads])
            self.og.add_reads(seq, q, off, 3, rbo.STORE_READ_PAIRS | (rbo.REVCOMP if rc else 0))
            if device:
                self.gg.addReads(seq, q, off, 3, reverseComplement=rc, storeReadPairedKmers=True)
        # fragments: FragmentsToGraphWorker (addFragments) on the device, the same inserts one by one in the oracle
        self.fsize = 1_000_003
        self.og.init_fragment_pairs(self.fsize, pk_h, frag_d)
        if device:
            self.gg.initializePairKmersBloomFilter(self.fsize, pk_h); self.gg.setFragPairedKmerDistance(frag_d)
        self.frags = []
        for _ in range(120):
            t = self.tx[int(rng.integers(0, len(self.tx)))]
            L = int(rng.integers(300, 601)); a = int(rng.integers(0, len(t) - L))
            self.frags.append(t[a:a + L])
        mode = 0 if stranded else 1
        for s in self.frags:
            hv, _ = rbo.hash_region(s, k, self.og.h, mode)
            for i in range(hv.shape[0]):
                self.og.add_dbg_only(hv[i])
            for dd, add in ((read_d, self.og.add_read_pair), (frag_d, self.og.add_fragment_pair)):
                if len(s) >= k + dd:
                    p, _, _ = rbo.hash_pairs_region(s, k, pk_h, dd, mode)
                    for i in range(p.shape[0]):
                        add(p[i])
        self.bits = {N.RPKBF: self.og.rpkbf_bytes(), N.FPKBF: self.og.fpkbf_bytes()}
        if device:
            fseq, foff = _pack(self.frags)
            self.gg.addFragments(ReadBatch.from_ascii(fseq, None, foff, 3), loadPairedKmers=True)
            assert (self.gg.exportFilter(N.RPKBF) == self.bits[N.RPKBF]).all()
            assert (self.gg.exportFilter(N.FPKBF) == self.bits[N.FPKBF]).all()

    def support(self, which, seqs):
        """per sequence: bool support over [0, nk) (False where p + d >= nk), from the oracle"""
        d = self.read_d if which == N.RPKBF else self.frag_d
        size = self.sizes[2] if which == N.RPKBF else self.fsize
        out = []
        for s in seqs:
            f, r, _ = self.og.get_kmers(s)
            sup = np.zeros(f.size, bool)
            keys = pair_keys(f, r, d, self.stranded)
            sup[:keys.size] = filter_lookup(self.bits[which], size, self.pk_h, self.k, keys)
            out.append(sup)
        # the numpy lookup is the oracle's own lookup
        look = self.og.lookup_read_pair if which == N.RPKBF else self.og.lookup_fragment_pair
        for s, sup in list(zip(seqs, out))[:20]:
            f, r, _ = self.og.get_kmers(s)
            keys = pair_keys(f, r, d, self.stranded)
            assert [look(rbo.ntm64(int(x), self.k, self.pk_h)) for x in keys] == list(sup[:keys.size])
        return out


def mutated(reads, rng, n_sub):
    out = []
    for s in reads:
        b = bytearray(s)
        for p in rng.integers(0, len(b), n_sub):
            b[p] = b"ACGT"[(b"ACGT".index(b[p]) + 1 + int(rng.integers(0, 3))) % 4] if b[p] in b"ACGT" else b[p]
        out.append(bytes(b))
    return out


def query_sets(w, rng):
    k, d = w.k, w.read_d
    reads = [w.left[i] for i in range(0, 600, 3)] + [w.right[i][::-1].translate(COMP) for i in range(1, 600, 5)]
    chim = []
    for i in range(60):
        a, b = w.tx[i % len(w.tx)], w.tx[(i + 7) % len(w.tx)]
        x, y = int(rng.integers(0, len(a) - 200)), int(rng.integers(0, len(b) - 200))
        chim.append(a[x:x + 200] + b[y:y + 200])
    iupac = []
    for s in reads[:80]:
        b = bytearray(s)
        for p in rng.integers(0, len(b), 3):
            b[p] = b"NKMSWYnkuU"[int(rng.integers(0, 10))]
        iupac.append(bytes(b))
    short = [reads[i][:L] for i, L in enumerate([0, 1, k - 1, k, k + 1, k + d - 1, k + d, k + d + 1, k + d + 2, 2 * k])]
    return {"reads": reads, "substituted": mutated(reads[:150], rng, 2), "chimeras": chim, "iupac": iupac, "short": short + w.frags[:30]}


def expected(sups, d, npr, ranges=None):
    segs = []
    for i, sup in enumerate(sups):
        a, b = ranges[i] if ranges is not None else (0, sup.size)
        segs.append(break_range(sup, d, npr, a, b))
    return segs


def device(w, which, seqs, npr, ranges=None):
    seq, off = _pack(seqs)
    so, segs, ns, ko, sup = w.gg.pairedKmerSegmentsFlat(which, seq, off, npr, ranges, support=True)
    # without support rows the positions outside the ranges are not probed: the segments are the same
    so2, segs2, ns2, _, _ = w.gg.pairedKmerSegmentsFlat(which, seq, off, npr, ranges)
    assert (so2 == so).all() and (ns2 == ns).all()
    assert all((segs2[so[i]:so[i] + ns[i]] == segs[so[i]:so[i] + ns[i]]).all() for i in range(len(seqs)))
    got = [[tuple(map(int, x)) for x in segs[so[i]:so[i] + ns[i]]] for i in range(len(seqs))]
    return got, so, ko, sup


def random_ranges(seqs, k, rng):
    out = []
    for s in seqs:
        nk = max(0, len(s) - k + 1)
        a = int(rng.integers(0, nk + 1)); b = int(rng.integers(a, nk + 1))
        out.append((a, b))
    return np.array(out, np.int32).reshape(len(seqs), 2)


CASES = [  # k, stranded, pk_h, read_d, frag_d
    (25, False, 2, 115, 250), (25, True, 1, 20, 60), (35, False, 3, 30, 100), (35, True, 2, 105, 180), (25, False, 1, 7, 300)]


@pytest.mark.parametrize("k,stranded,pk_h,read_d,frag_d", CASES)
def test_segments_and_support_match_the_oracle(k, stranded, pk_h, read_d, frag_d):
    rng = np.random.default_rng(k * 7 + pk_h + read_d)
    w = World(k, stranded, pk_h, read_d, frag_d, seed=k + pk_h + read_d)
    sets = query_sets(w, rng)
    for which, d in ((N.RPKBF, read_d), (N.FPKBF, frag_d)):
        for name, seqs in sets.items():
            sups = w.support(which, seqs)
            for npr in (1, 2, 3, 10):
                got, so, ko, sup = device(w, which, seqs, npr)
                assert got == expected(sups, d, npr), (which, name, npr)
                assert (ko == np.concatenate([[0], np.cumsum([s.size for s in sups])])).all()
                assert (sup.astype(bool) == (np.concatenate(sups) if sups else np.zeros(0, bool))).all(), (which, name)
                assert (np.diff(so) == [capacity(d, 0, s.size) for s in sups]).all()
                rg = random_ranges(seqs, k, rng)
                got, so, _, _ = device(w, which, seqs, npr, rg)
                assert got == expected(sups, d, npr, rg), (which, name, npr, "ranges")
                assert (np.diff(so) == [capacity(d, int(a), int(b)) for a, b in rg]).all()
    # the public forms
    seqs = sets["chimeras"]
    sups = w.support(N.RPKBF, seqs)
    assert w.gg.breakWithReadPairedKmers(seqs, 1) == expected(sups, read_d, 1)
    assert w.gg.breakWithReadPairedKmers(seqs, 3, ranges=[(0, max(0, len(s) - k + 1) // 2) for s in seqs]) == \
        expected(sups, read_d, 3, [(0, s.size // 2) for s in sups])
    fs = w.support(N.FPKBF, w.frags)
    assert w.gg.breakWithFragPairedKmers(w.frags) == expected(fs, frag_d, 1)
    assert w.gg.breakWithFragPairedKmers(w.frags, 2) == expected(fs, frag_d, 2)
    assert [s.tolist() for s in w.gg.pairedKmerSupport(w.frags, N.FPKBF)] == [s.tolist() for s in fs]
    # what the reads were inserted from is supported: every inserted read is one whole segment, a chimera of two transcripts is cut
    reads = sets["reads"]
    if max(len(s) for s in reads) - k + 1 > read_d:
        assert all(s == [(0, len(r) - k + 1)] for s, r in zip(w.gg.breakWithReadPairedKmers(reads, 1), reads))
    if read_d + k < 200:                            # both halves of a chimera hold pairs
        assert sum(len(s) >= 2 for s in w.gg.breakWithReadPairedKmers(seqs, 1)) >= len(seqs) // 2
    w.gg.destroy()


HAND = [  # (support pattern, d, numPairsRequired, range or None, the segments worked out by hand in tests/test_paired_segment_rules.py)
    ("1001000", 3, 1, None, [(0, 7)]), ("1010000", 3, 1, None, [(0, 6)]), ("10011000", 2, 1, None, [(0, 3), (3, 7)]),
    ("10100000", 2, 1, None, [(0, 5)]), ("11001100", 2, 2, None, [(0, 4), (4, 8)]), ("0011100000", 2, 3, None, [(2, 7)]),
    ("0111110000", 2, 3, None, [(1, 8)]), ("1101101100", 2, 3, None, []), ("11101100000", 2, 3, None, [(0, 5)]),
    ("11101100000", 2, 1, None, [(0, 8)]), ("0001111", 3, 1, None, [(3, 10)]), ("0001111", 3, 4, None, [(3, 10)]),
    ("0001110", 3, 1, None, [(3, 9)]), ("1" * 17, 3, 2, (5, 12), [(5, 12)]), ("11110000" + "1" * 9, 3, 1, (0, 7), [(0, 7)]),
    ("11110000" + "1" * 9, 3, 1, None, [(0, 7), (8, 20)]), ("11111" + "0" * 12, 3, 3, (2, 20), [(2, 8)]), ("11111" + "0" * 12, 3, 3, (3, 20), []),
    ("1" * 20, 5, 1, (10, 15), []), ("1" * 20, 5, 1, (10, 16), [(10, 16)]), ("1000" * 5, 3, 1, None, [(0, 4), (4, 8), (8, 12), (12, 16), (16, 20)])]


@pytest.mark.parametrize("stranded", [False, True])
def test_planted_patterns(stranded):
    """support planted position by position (addReadSingleKmerPair of the pair keys of the chosen positions) into a pair filter large enough
    that nothing else is in it: the hand-worked patterns, then random patterns for d = 1, 5, 40 and every numPairsRequired"""
    k = 25
    rng = np.random.default_rng(21 + stranded)
    hasher = rbo.Graph(1009, 1009, 1009, 2, 2, 2, k, stranded, True, 1)
    g = BloomFilterDeBruijnGraph(100_003, 100_003, 512_000_009, 2, 2, 2, k, stranded, True)
    cases = [(pattern(p), d, n, r, want) for p, d, n, r, want in HAND]
    for d in (1, 5, 40):
        for _ in range(25):
            L = int(rng.integers(0, 300))
            sup = list(rng.random(L) < rng.choice([0.2, 0.6, 0.95]))
            nk = L + d
            a = int(rng.integers(0, nk + 1)); b = int(rng.integers(a, nk + 1))
            for n in (1, 2, 3, 10):
                cases.append((sup, d, n, (a, b) if rng.random() < 0.5 else None, None))
    seqs = []
    for sup, d, n, r, want in cases:
        s = ACGT[rng.integers(0, 4, len(sup) + d + k - 1)].tobytes()
        f, rv, _ = hasher.get_kmers(s)
        keys = pair_keys(f, rv, d, stranded)
        assert keys.size == len(sup)
        if any(sup):
            g.addReadSingleKmerPair(keys[np.array(sup, bool)])
        seqs.append(s)
    bits = g.exportFilter(N.RPKBF)
    for d in sorted({c[1] for c in cases}):
        g.setReadPairedKmerDistance(d)
        idx = [i for i, c in enumerate(cases) if c[1] == d]
        for n in sorted({cases[i][2] for i in idx}):
            sel = [i for i in idx if cases[i][2] == n]
            for ranged in (False, True):
                part = [i for i in sel if (cases[i][3] is not None) == ranged]
                if not part:
                    continue
                ss = [seqs[i] for i in part]
                rg = np.array([cases[i][3] for i in part], np.int32).reshape(-1, 2) if ranged else None
                seq, off = _pack(ss)
                so, segs, ns, ko, sup = g.pairedKmerSegmentsFlat(N.RPKBF, seq, off, n, rg, support=True)
                for j, i in enumerate(part):
                    p, _, _, r, want = cases[i]
                    f, rv, _ = hasher.get_kmers(seqs[i])
                    planted = filter_lookup(bits, 512_000_009, 2, k, pair_keys(f, rv, d, stranded))
                    assert list(planted) == list(p)                   # nothing but the planted keys answers
                    assert list(sup[ko[j]:ko[j] + len(p)].astype(bool)) == list(p) and not sup[ko[j] + len(p):ko[j + 1]].any()
                    nk = len(p) + d
                    expect = break_range(p, d, n, *(r if r is not None else (0, nk)))
                    if want is not None:
                        assert expect == want
                    got = [tuple(map(int, x)) for x in segs[so[j]:so[j] + ns[j]]]
                    assert got == expect, (d, n, r, "".join("1" if x else "0" for x in p))
                    assert so[j + 1] - so[j] == capacity(d, *(r if r is not None else (0, nk)))
    g.destroy()


def test_many_pieces_equal_one(monkeypatch):
    rng = np.random.default_rng(3)
    w = World(25, False, 2, 40, 150, seed=11)
    seqs = sum(query_sets(w, rng).values(), []) * 2
    rg = random_ranges(seqs, 25, rng)
    whole = [device(w, which, seqs, npr, r) for which in (N.RPKBF, N.FPKBF) for npr in (1, 3) for r in (None, rg)]
    for piece in ("1", "97", "5000"):
        monkeypatch.setenv("RB_QUERY_PIECE", piece)
        got = [device(w, which, seqs, npr, r) for which in (N.RPKBF, N.FPKBF) for npr in (1, 3) for r in (None, rg)]
        for a, b in zip(got, whole):
            assert a[0] == b[0] and (a[1] == b[1]).all() and (a[2] == b[2]).all() and (a[3] == b[3]).all(), piece
    w.gg.destroy()


def raw_call(g, which, seqs, npr=1, ranges=None, segs=True, n_segs=True, support=False, koffsets=True, offsets=True, so=True):
    seq, off = _pack(seqs)
    n = len(seqs)
    rg = None if ranges is None else np.ascontiguousarray(ranges, np.int32)
    a_so = np.zeros(n + 1, np.int64); a_ko = np.zeros(n + 1, np.int64)
    a_segs = np.zeros(4096, np.int32); a_ns = np.zeros(n, np.int32); a_sup = np.zeros(1 << 16, np.uint8)
    p = lambda a, use: a.ctypes.data_as(C.c_void_p) if use and a is not None else None
    return N.lib.rb_graph_paired_kmer_segments(g, which, p(seq, True), p(off, offsets), n, npr, p(rg, True), p(a_so, so), p(a_segs, segs),
                                               p(a_ns, n_segs), p(a_sup, support), p(a_ko, koffsets))


def test_refusals():
    s = [b"ACGT" * 60, b"ACGTTGCA" * 20]
    g = BloomFilterDeBruijnGraph(100_003, 200_003, 30_011, 2, 2, 2, 25, False, True)
    assert raw_call(g.h, N.RPKBF, s) == ERR_INVALID                          # read distance never set (-1)
    g.setReadPairedKmerDistance(0)
    assert raw_call(g.h, N.RPKBF, s) == ERR_INVALID                          # distance < 1
    g.setReadPairedKmerDistance(20)
    assert raw_call(g.h, N.RPKBF, s) == 0
    assert raw_call(g.h, N.FPKBF, s) == ERR_INVALID                          # rb_graph_init_fragment_pairs never called
    g.initializePairKmersBloomFilter(5003, 2)
    assert raw_call(g.h, N.FPKBF, s) == ERR_INVALID                          # ... and no fragment distance
    g.setFragPairedKmerDistance(30)
    assert raw_call(g.h, N.FPKBF, s) == 0
    for which in (N.DBGBF, N.CBF, 4, -1):
        assert raw_call(g.h, which, s) == ERR_INVALID
    for npr in (0, -3):
        assert raw_call(g.h, N.RPKBF, s, npr) == ERR_INVALID
    nk = [len(x) - 24 for x in s]
    for bad in ([(-1, 5), (0, 5)], [(3, 2), (0, 5)], [(0, nk[0] + 1), (0, 5)], [(0, 5), (nk[1] + 1, nk[1] + 1)]):
        assert raw_call(g.h, N.RPKBF, s, ranges=bad) == ERR_INVALID
    assert raw_call(g.h, N.RPKBF, s, ranges=[(0, nk[0]), (nk[1], nk[1])]) == 0
    assert raw_call(g.h, N.RPKBF, s, offsets=False) == ERR_INVALID
    assert raw_call(g.h, N.RPKBF, s, so=False) == ERR_INVALID
    assert raw_call(g.h, N.RPKBF, s, n_segs=False) == ERR_INVALID
    assert raw_call(g.h, N.RPKBF, s, support=True, koffsets=False) == ERR_INVALID
    assert raw_call(None, N.RPKBF, s) == ERR_INVALID
    assert raw_call(g.h, N.RPKBF, s, segs=False, n_segs=False) == 0          # the size query
    with pytest.raises(N.NativeError):
        g.breakWithReadPairedKmers(s, 0)
    g.destroy()
    g = BloomFilterDeBruijnGraph(100_003, 200_003, 30_011, 2, 2, 2, 25, False, False)     # useReadPairedKmers off
    g.setReadPairedKmerDistance(20)
    assert raw_call(g.h, N.RPKBF, s) == ERR_INVALID
    with pytest.raises(N.NativeError):
        g.breakWithReadPairedKmers(s, 1)
    g.destroy()
    rk = sharded.ShardRank((100_003, 200_003, 30_011, 2, 2, 2, 25, 0, 1, 0, 0, 9, 0), 0, 1, 0, "split")
    rk.set_read_pair_distance(20)
    assert raw_call(rk.h, N.RPKBF, s) == ERR_INVALID                         # a shard handle


def test_every_inserted_read_is_one_segment_at_size():
    """config-2-shaped library inserted with storeReadPairedKmers: every read with only usable bases and nk > d is [0, nk) for n = 1, 3"""
    pairs, d, k = 2_000_000, 115, 25
    batch = ReadBatch.synthetic(pairs, 64_000_000 * pairs // 50_000_000, seed=0x5EED)
    nk_all = 2 * pairs * (150 - k + 1)
    bits = N.lib.rb_expected_size(nk_all, 0.01, 2)
    pk = N.lib.rb_expected_size(2 * pairs * (150 - k + 1 - d), 0.01, 2)
    for stranded in (False, True):
        g = BloomFilterDeBruijnGraph(bits, bits, pk, 2, 2, 2, k, stranded, True, rngSeed=1)
        g.setReadPairedKmerDistance(d)
        g.addBatch(batch, first=0, n=pairs, storeReadPairedKmers=True)
        g.addBatch(batch, reverseComplement=True, first=pairs, n=pairs, storeReadPairedKmers=True)
        for half, rc in ((0, False), (1, True)):
            seq, off = batch.download(half * pairs, pairs)
            if rc and stranded:                     # the reverse file went in reverse-complemented: query it in that orientation
                lut = np.arange(256, dtype=np.uint8); lut[list(b"ACGT")] = list(b"TGCA")
                seq = lut[seq.reshape(pairs, -1)[:, ::-1]].reshape(-1)
            lens = np.diff(off)
            usable = np.add.reduceat(~np.isin(seq, np.frombuffer(b"ACGT", np.uint8)), off[:-1]) == 0
            nk = lens - k + 1
            want = usable & (nk > d)
            assert want.sum() > 0.8 * pairs
            for npr in (1, 3):
                so, segs, ns, _, _ = g.pairedKmerSegmentsFlat(N.RPKBF, seq, off, npr)
                first = segs[so[:-1].clip(max=max(len(segs) - 1, 0))]
                ok = (ns == 1) & (first[:, 0] == 0) & (first[:, 1] == nk)
                bad = np.nonzero(want & ~ok)[0]
                assert bad.size == 0, (stranded, half, npr, bad.size, bad[:5])
        g.destroy()
