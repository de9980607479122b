"""The counting filter at its ceiling: MiniFloat stops at byte 127 (R/util/MiniFloat.java:31-38, toFloat(127) = 245760), and the
engine has code written for that state alone — run_ops stops a run there, the prefilter caches remember a saturated k-mer (every
further occurrence is dropped), the light path treats reaching 127 as news, the heavy / conflict stores and cbf_step guard it, and
bit 7 of a counter byte is the sub-batch claim mark (a claimed 127 is 0xFF).  Here a workload built for it takes a few hundred
k-mers to 127 and a few hundred more to 119-126, and every engine variant is compared with the oracle byte for byte.

Workload: short hot transcripts (140-200 bases, 100-base reads, 0.15-0.8 M occurrences per k-mer — reaching 127 from 0 takes
about 8 (2^15 - 1) occurrences, with a wide spread) shuffled into an ordinary background library as read pairs, substitution
errors masked by quality (and a variant that keeps them), inserted in two calls: the left file, then the right file
reverse-complemented.  Two hot transcripts share 70 bases and then branch, so walks meet neighbours that tie at 245760.

Each oracle result is computed once per (k, strandedness, filter sizes, errors) for the module, the oracles in parallel (the
oracle releases the GIL), and every GPU variant is compared with it."""
import concurrent.futures as cf
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import rbo
from rnabloom import _native as N
from rnabloom import synth
from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch
from rnabloom.sharded import LoopbackCluster

SIZES = (2_000_003, 3_000_017, 400_009)          # dbgbf bits, counting-filter bytes (roomy), read-pair filter bits
SMALL_CBF = 400_009                              # a fifth of the counters shared, many of them by a saturated k-mer and a background one
RL, DIST, SEED = 100, 115, 23
TOP = 245760.0                                   # MiniFloat.toFloat(127): a saturated counter
GTOP = TOP + 1.0                                 # the graph's count of a saturated k-mer (getCount = counter + 1 for a k-mer in dbgbf)
HOT_PAIRS = {"A": 360_000, "B": 260_000, "C": 190_000}
CHUNK = 200_000                                  # reads per oracle add_reads call (one call of the engine = several of these)


def _rand(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]


def hot_transcripts():
    """A = X + YA and B = X + YB share their first 70 bases (so the last 24 of X are a (k-1)-mer followed by two different
    bases, both k-mers saturated); C stands alone and is read less deeply (its k-mers end near 119-126)"""
    rng = np.random.default_rng(SEED)
    X, YA, YB, Cc = _rand(rng, 70), _rand(rng, 70), _rand(rng, 70), _rand(rng, 200)
    YB[0] = {65: 67, 67: 71, 71: 84, 84: 65}[int(YA[0])]         # the branch: A and B differ right after X
    return {"A": np.concatenate([X, YA]), "B": np.concatenate([X, YB]), "C": Cc}


_WORK = {}


def workload(keep_errors):
    """(left, right): (seq, qual, offsets) of the two files; hot pairs and the background pairs in one shuffled order"""
    if keep_errors in _WORK:
        return _WORK[keep_errors]
    rng = np.random.default_rng(SEED + 1)
    lefts, rights = [], []
    for name, T in hot_transcripts().items():
        n = HOT_PAIRS[name]
        a = rng.integers(0, T.size - RL + 1, n)
        b = a + (rng.random(n) * (T.size - RL + 1 - a)).astype(np.int64)   # right end at or after the left one
        ar = np.arange(RL)
        lefts.append(T[a[:, None] + ar]); rights.append(synth.revcomp(T[b[:, None] + ar]))
    hl, hr = np.concatenate(lefts), np.concatenate(rights)
    out = []
    for reads in (hl, hr):
        reads = reads.copy()
        q = np.full(reads.shape, ord("I"), np.uint8)
        e = rng.random(reads.shape) < 0.002
        reads[e] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), reads[e])]
        if not keep_errors:
            q[e] = ord("#")
        reads[rng.random(reads.shape) < 1e-4] = ord("N")
        out.append((reads, q))
    bg = synth.generate_pairs(30_000, G=40_000, L=150, err=0.002, n_rate=1e-3, seed=SEED + 2)
    if keep_errors:
        bg["lqual"][:] = ord("I"); bg["rqual"][:] = ord("I")
    n_hot, n_bg = hl.shape[0], bg["left"].shape[0]
    order = rng.permutation(n_hot + n_bg)
    hot = order < n_hot
    off = np.concatenate([[0], np.cumsum(np.where(hot, RL, 150))]).astype(np.int64)
    files = []
    for (reads, q), (bs, bq) in zip(out, ((bg["left"], bg["lqual"]), (bg["right"], bg["rqual"]))):
        seq, qual = np.empty(off[-1], np.uint8), np.empty(off[-1], np.uint8)
        for sel, src, sq, width, row in ((hot, reads, q, RL, order[hot]), (~hot, bs, bq, 150, order[~hot] - n_hot)):
            at = off[:-1][sel][:, None] + np.arange(width)
            seq[at] = src[row]; qual[at] = sq[row]
        files.append((seq, qual, off))
    _WORK[keep_errors] = tuple(files)
    return _WORK[keep_errors]


def third_pass_reads(og, k):
    """error-free reads made only of k-mers the oracle holds at 127 after the two files: every stretch of saturated k-mers of every
    hot transcript (a stretch of one k-mer is a read of k bases), repeated to about 6 M k-mers — every occurrence of this pass is a
    no-op.  Among them are k-mers that reached 127 late in the second file, with no later occurrence that could have told the cache
    (only the news of reaching 127 did)"""
    pieces = []
    for T in hot_transcripts().values():
        T = T.tobytes()
        c = og.get_kmers(T)[2]
        i = 0
        while i < len(c):
            j = i
            while j < len(c) and c[j] == GTOP:
                j += 1
            if j > i:
                pieces.append(T[i:j + k - 1])
            i = j + 1
    n_kmers = sum(len(p) - k + 1 for p in pieces)
    assert n_kmers >= 150, n_kmers
    reps = 6_000_000 // n_kmers
    seq = np.tile(np.frombuffer(b"".join(pieces), np.uint8), reps)
    off = np.concatenate([[0], np.cumsum(np.tile([len(p) for p in pieces], reps))]).astype(np.int64)
    return seq, None, off


def _oracle_add(og, seq, qual, off, flags):
    """the oracle over one file in pieces (the ordinals continue from piece to piece, as in one call)"""
    tot = [0, 0]
    for a in range(0, len(off) - 1, CHUNK):
        b = min(len(off) - 1, a + CHUNK)
        o = off[a:b + 1] - off[a]
        st = og.add_reads(seq[off[a]:off[b]], None if qual is None else qual[off[a]:off[b]], o, 3, flags)
        tot[0] += st.kmers; tot[1] += st.pairs
    return tuple(tot)


class OracleRun:
    """the oracle's filters after each step of the fixed sequence: (1) left file, pairs stored; (2) right file reverse-complemented;
    (3) the third pass of saturated k-mers only; (4) count-if-present over the left file"""

    def __init__(self, k, stranded, cbf_bytes, keep_errors, steps):
        self.k, self.stranded, self.cbf_bytes, self.keep_errors = k, stranded, cbf_bytes, keep_errors
        self.og = rbo.Graph(SIZES[0], cbf_bytes, SIZES[2], 2, 2, 2, k, stranded, True, 5)
        self.og.set_read_pair_distance(DIST)
        (ls, lq, lo), (rs, rq, ro) = workload(keep_errors)
        self.snap, self.stats = [], []
        for step in range(steps):
            if step == 0:
                st = _oracle_add(self.og, ls, lq, lo, rbo.STORE_READ_PAIRS)
            elif step == 1:
                st = _oracle_add(self.og, rs, rq, ro, rbo.STORE_READ_PAIRS | rbo.REVCOMP)
            elif step == 2:
                self.third = third_pass_reads(self.og, k)
                st = _oracle_add(self.og, *self.third, 0)
            else:
                st = _oracle_add(self.og, ls, lq, lo, rbo.COUNT_IF_PRESENT)
            self.stats.append(st)
            self.snap.append((self.og.dbgbf_bytes(), self.og.cbf_bytes(), self.og.rpkbf_bytes()))


ORACLES = {   # name: (k, stranded, cbf bytes, keep errors, steps)
    "k25": (25, False, SIZES[1], False, 4),
    "small": (25, False, SMALL_CBF, False, 2),
    "k35": (35, False, SIZES[1], False, 2),
    "stranded": (25, True, SIZES[1], False, 2),
    "errors": (25, False, SIZES[1], True, 2),
    "k25_two_files": (25, False, SIZES[1], False, 2),      # (its graph stays at the state after the two files: sharded walks)
}


@pytest.fixture(scope="module")
def oracles():
    for ke in (False, True):
        workload(ke)
    with cf.ThreadPoolExecutor(len(ORACLES)) as ex:
        fut = {name: ex.submit(OracleRun, *args) for name, args in ORACLES.items()}
        runs = {name: f.result() for name, f in fut.items()}
    # the fixture's own edge: the ceiling is reached, some of it in the first file and more in the second, counters sit just below
    # it, and (small filter) saturated counters are shared; nothing exceeds 127
    report = []
    for name, o in runs.items():
        c1, c2 = o.snap[0][1], o.snap[1][1]
        at1, at2, near = int((c1 == 127).sum()), int((c2 == 127).sum()), int(((c2 >= 120) & (c2 <= 126)).sum())
        report.append("%s: %d counters at 127 after file 1, %d after file 2, %d at 120-126" % (name, at1, at2, near))
        assert c2.max() == 127 and c1.max() <= 127
        assert at1 >= 100 and at2 >= at1 + 100 and near >= 50, report[-1]
    o = runs["small"]
    hv = []
    for T in hot_transcripts().values():
        h, _ = rbo.hash_region(T.tobytes(), 25, 2, rbo.CANON)
        hv.append(h)
    hv = np.unique(np.concatenate(hv), axis=0)
    cnt = np.array([o.og.get_count(h) for h in hv])
    sat_idx = np.unique(((hv[cnt == GTOP] >> np.uint64(1)) % np.uint64(SMALL_CBF)).ravel())
    genome, _, _ = synth.make_transcriptome(40_000, SEED + 2)         # the background library's transcriptome
    bh, _ = rbo.hash_region(genome.tobytes(), 25, 2, rbo.CANON)
    bg_idx = np.unique(((bh >> np.uint64(1)) % np.uint64(SMALL_CBF)).ravel())
    shared = np.intersect1d(sat_idx, bg_idx).size
    report.append("small: %d counters of saturated hot k-mers also belong to background k-mers" % shared)
    assert shared >= 50, report[-1]
    print("\n" + "\n".join(report))
    return runs


def gpu_graph(o, max_batch=0):
    gg = BloomFilterDeBruijnGraph(SIZES[0], o.cbf_bytes, SIZES[2], 2, 2, 2, o.k, o.stranded, True, rngSeed=5, maxBatchKmers=max_batch)
    gg.setReadPairedKmerDistance(DIST)
    return gg


def assert_step(o, step, dbg, cbf, rpk, what):
    d, c, r = o.snap[step]
    assert cbf.max() <= 127, "%s step %d: a counter byte above 127 (%d)" % (what, step, cbf.max())
    bad = np.nonzero(cbf != c)[0]
    assert bad.size == 0, "%s step %d: cbf differs at %d bytes, first %s: gpu %s oracle %s" % (what, step, bad.size, bad[:5], cbf[bad[:5]], c[bad[:5]])
    assert (dbg == d).all(), "%s step %d: dbgbf differs" % (what, step)
    assert (rpk == r).all(), "%s step %d: rpkbf differs" % (what, step)


def gpu_steps(o, gg, steps):
    (ls, lq, lo), (rs, rq, ro) = workload(o.keep_errors)
    out = []
    for step in range(steps):
        if step == 0:
            st = gg.addReads(ls, lq, lo, 3, storeReadPairedKmers=True)
        elif step == 1:
            st = gg.addReads(rs, rq, ro, 3, reverseComplement=True, storeReadPairedKmers=True)
        elif step == 2:
            st = gg.addReads(*o.third, 3)
        else:
            st = gg.addReads(ls, lq, lo, 3, incrementIfPresent=True)
        assert (st.kmers, st.pairs) == o.stats[step], (step, st.kmers, st.pairs, o.stats[step])
        assert_step(o, step, gg.exportFilter(N.DBGBF), gg.exportFilter(N.CBF), gg.exportFilter(N.RPKBF), "single GPU")
        out.append(st)
    return out


@pytest.mark.parametrize("oracle,env,max_batch", [
    ("k25", {}, 0),
    ("k25", {"RB_NO_MPF": "1"}, 0),
    ("k25", {"RB_PF_SKIP": "0"}, 1 << 20),
    ("k25", {"RB_PF_SKIP": "2", "RB_NO_MPF": "1"}, 1 << 18),
    ("k25", {"RB_SWEEP": "1"}, 0),
    ("small", {}, 0),
    ("small", {"RB_ORDER_ALL_SHARED": "1"}, 1 << 18),
    ("small", {"RB_NO_MPF": "1", "RB_SWEEP": "1"}, 1 << 20),
    ("k35", {}, 0),
    ("k35", {"RB_PF_SKIP": "2"}, 1 << 19),
    ("stranded", {}, 0),
    ("errors", {}, 0),
    ("errors", {"RB_NO_MPF": "1"}, 1 << 19),
])
def test_saturating_inserts_match_oracle(monkeypatch, oracles, oracle, env, max_batch):
    """both files into one graph, the filters compared with the oracle's after each; the second call starts with a prefilter cache
    that already holds saturated k-mers"""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    o = oracles[oracle]
    gg = gpu_graph(o, max_batch)
    st = gpu_steps(o, gg, 2)
    assert sum(s.sorted_kmers for s in st) < sum(s.kmers for s in st), "the prefilter dropped nothing"
    gg.destroy()


def test_saturated_kmers_are_dropped_and_count_if_present(monkeypatch, oracles):
    """the hash-bucketed cache (the one with a true 'saturated' entry) with its walk on every sub-batch: a third pass made of
    saturated k-mers only must sort almost nothing — every occurrence is known to be a no-op — and leave the oracle's filters; then
    count-if-present over the saturated graph (the other mode that asks the prefilter)"""
    monkeypatch.setenv("RB_NO_MPF", "1")
    monkeypatch.setenv("RB_PF_SKIP", "0")
    o = oracles["k25"]
    gg = gpu_graph(o)
    st = gpu_steps(o, gg, 4)
    print("\nthird pass: %d of %d k-mers sorted" % (st[2].sorted_kmers, st[2].kmers))
    assert st[2].kmers > 1_000_000 and st[2].sorted_kmers <= st[2].kmers // 100, (st[2].sorted_kmers, st[2].kmers)
    # every k-mer of the pass reached 127 in an earlier call and the cache was told so: not one occurrence is left to sort
    assert st[2].sorted_kmers == 0, st[2].sorted_kmers
    gg.destroy()


@pytest.mark.parametrize("G,mode,native", [(2, "replicated", False), (8, "split", False), (2, "replicated", True), (8, "split", True)])
def test_sharded_engine_at_the_ceiling(oracles, G, mode, native):
    """the sharded engine (replicated cache entries shipped with s = 15 among them) against the same oracle result"""
    o = oracles["k25"]
    cl = LoopbackCluster(G, SIZES[0], o.cbf_bytes, SIZES[2], 2, 2, 2, 25, False, True, rngSeed=5, mode=mode, native=native)
    cl.setReadPairedKmerDistance(DIST)
    (ls, lq, lo), (rs, rq, ro) = workload(False)
    for step, (s, q, off, rc) in enumerate(((ls, lq, lo, False), (rs, rq, ro, True))):
        cl.addBatch(ReadBatch.from_ascii(s, q, off, 3), 150, reverseComplement=rc, storeReadPairedKmers=True)
        assert_step(o, step, cl.exportFilter(N.DBGBF), cl.exportFilter(N.CBF), cl.exportFilter(N.RPKBF), "G=%d %s" % (G, mode))
    cl.destroy()


def _hashes(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 63, n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)


def test_per_hash_adds_cross_127_in_one_call():
    """gg.add / gg.addCountIfPresent with a handful of hashes repeated a few hundred thousand times in one array each: the counters
    pass 127 inside the call, against the oracle's per-element loop in array order"""
    og = rbo.Graph(20_011, 30_011, 5_003, 2, 2, 2, 25, False, True, 7)
    gg = BloomFilterDeBruijnGraph(20_011, 30_011, 5_003, 2, 2, 2, 25, False, True, rngSeed=7)
    pool = _hashes(6, 3)
    rng = np.random.default_rng(4)
    L = og.L
    hv = [rbo.ntm64(int(h), 25, 2) for h in pool]
    for op_o, op_g, n in (("add", "add", 700_000), ("add_count_if_present", "addCountIfPresent", 900_000)):
        pick = rng.integers(0, pool.size - (1 if op_o == "add" else 0), n)       # (the last hash is absent until the second round)
        fn = getattr(L, "rbo_graph_" + op_o)
        for i in pick:
            fn(og.g, hv[i].ctypes.data_as(C.c_void_p))
        getattr(gg, op_g)(pool[pick])
        c_g, c_o = gg.exportFilter(N.CBF), og.cbf_bytes()
        assert (c_g == c_o).all(), (op_o, np.nonzero(c_g != c_o)[0][:5])
        assert (gg.exportFilter(N.DBGBF) == og.dbgbf_bytes()).all()
    exp = np.array([og.get_count(h) for h in hv], np.float32)
    assert (gg.getCount(pool) == exp).all() and (exp == GTOP).sum() >= 3, exp
    gg.destroy()


def test_increment_and_get_crosses_127_inside_a_chunk():
    """the stand-alone CountingBloomFilter.incrementAndGet: the same keys pass 127 in the middle of a chunk; every returned value
    (245760 included) against the oracle in array order"""
    from rnabloom.bloom import CountingBloomFilter
    L = rbo.lib()
    size, nh, k, seed = 5003, 2, 11, 9
    cbf = CountingBloomFilter(size, nh, k, rngSeed=seed)
    oc = L.rbo_cbf_new(size, nh)
    rng = np.random.default_rng(3)
    keys = _hashes(4, 8)
    h = keys[rng.integers(0, 4, 1_200_000)]
    ordinal, crossed = 0, 0
    hv = {int(x): rbo.ntm64(int(x), k, nh) for x in keys}
    for chunk in np.array_split(h, 5):
        got = cbf.incrementAndGet(chunk)
        exp = np.empty(chunk.size, np.float32)
        for i, x in enumerate(chunk):
            exp[i] = L.rbo_cbf_increment_and_get(oc, rbo._p(hv[int(x)]), L.rbo_rng31(seed, ordinal, 0))
            ordinal += 1
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (bad[:5], got[bad[:5]], exp[bad[:5]])
        crossed += int(0 < np.argmax(exp == TOP) < chunk.size - 1)
    n = C.c_int64()
    raw = np.ctypeslib.as_array(C.cast(L.rbo_cbf_bytes(oc, C.byref(n)), C.POINTER(C.c_uint8)), (n.value,)).copy()
    assert (cbf.toBytes() == raw).all() and raw.max() == 127
    assert crossed >= 1                                        # some chunk starts below the ceiling and reaches it
    val = np.array([float(b) if b <= 7 else float(((b & 7) | 8) << ((b >> 3) - 1)) for b in range(128)], np.float64)
    for min_cov in (122880, 131072, 229376, 245760, 245760.5, 1e9):
        bf = cbf.getBloomFilter(min_cov)
        assert (bf.toBytes() == np.packbits(val[raw] >= min_cov, bitorder="little")).all(), min_cov
        bf.destroy()
    L.rbo_cbf_free(oc)
    cbf.destroy()


@pytest.fixture(scope="module")
def saturated_graph(oracles):
    """the single-GPU graph after all four steps of the k25 sequence, beside the oracle's"""
    o = oracles["k25"]
    gg = gpu_graph(o)
    gpu_steps(o, gg, 4)
    yield o, gg
    gg.destroy()


def test_queries_at_the_ceiling(saturated_graph):
    """getCount / getCounts / batchCounts equal the oracle's floats (245760 included); getKmersMinCoverage and getBloomFilter(minCov)
    at thresholds on and beside the top levels"""
    from rnabloom.graphutils import getKmersMinCoverage
    o, gg = saturated_graph
    og = o.og
    seqs = [T.tobytes() for T in hot_transcripts().values()]
    (ls, _, lo), _ = workload(False)
    seqs += [bytes(ls[lo[i]:lo[i + 1]]) for i in range(0, 3000, 7)]
    ko, f, r, c = gg.getKmers(seqs)
    exp = np.concatenate([og.get_kmers(s)[2] for s in seqs])
    assert (c == exp).all() and (exp == GTOP).sum() >= 200 and ((exp >= 131072) & (exp < GTOP)).sum() >= 20
    h0 = np.where(f.view(np.int64) < r.view(np.int64), f, r)
    assert (gg.getCount(h0)[exp > 0] == exp[exp > 0]).all()
    b = ReadBatch.from_reads(seqs, None)
    bc = gg.batchCounts(b, koffsets=ko)
    assert (bc == exp).all()
    for min_cov in (122880.0, 131072.0, 245760.0, 245760.5, GTOP, GTOP + 0.5, 1e9):
        got = getKmersMinCoverage(gg, seqs, min_cov)
        for i, s in enumerate(seqs):
            e = rbo.get_kmers_min_coverage(og, s, min_cov)
            st, n, cnt = got[i]
            assert n == len(e) and (n == 0 or (st == e[0][0] and (cnt == np.array([x[1] for x in e], np.float32)).all())), (min_cov, i)
    raw = o.snap[3][1]
    val = np.array([float(x) if x <= 7 else float(((x & 7) | 8) << ((x >> 3) - 1)) for x in range(128)], np.float64)
    from rnabloom.bloom import BloomFilter
    for min_cov in (122880, 131072, 245760, 245760.5, 1e9):
        bf = BloomFilter(o.cbf_bytes, 2, 25)                      # rb_cbf_to_bloom of the graph's own counting filter
        N.check(N.lib.rb_cbf_to_bloom(gg.h, float(min_cov), bf._g.h, N.DBGBF))
        want = np.packbits(val[raw] >= min_cov, bitorder="little")
        assert (bf.toBytes() == want).all(), min_cov
        assert min_cov > TOP or want.any()
        bf.destroy()


def walk_seeds(k=25):
    T = hot_transcripts()
    out = []
    for name, t in T.items():
        t = t.tobytes()
        out += [t[p:p + k] for p in range(0, len(t) - k + 1, 3)]
    return out


def test_walks_over_saturated_kmers(saturated_graph):
    """walkMaxCov (first strict maximum), greedyExtend with lookahead and naiveExtend over saturated neighbours that tie at
    245760 (A and B branch after their shared 70 bases), against the oracle's restatements"""
    o, gg = saturated_graph
    og = o.og
    seeds = walk_seeds()
    last = hot_transcripts()["A"][45:70].tobytes()                # the last k-mer of X: its successors into A and into B tie
    f, r, _ = og.get_kmers(last)
    assert (og.neighbors(int(f[0]), int(r[0]), last[0], 0)[2] == GTOP).sum() == 2
    for direction in (0, 1):
        for bound, min_cov in ((60, 1.0), (30, TOP)):
            bases, _, _, c, ln, reason = gg.walkMaxCov(seeds, direction, bound, min_cov)
            for i, s in enumerate(seeds):
                eb, ec, er = rbo.walk_max_cov(og, s, direction, bound, min_cov)
                assert int(reason[i]) == er and int(ln[i]) == len(eb), (direction, bound, i)
                assert bytes(bases[i, :ln[i]]) == eb and (c[i, :ln[i]] == np.array(ec, np.float32)).all()
        for lookahead, bound in ((3, 40), (6, 20)):
            bases, c, ln, _ = gg.greedyExtend(seeds, direction, lookahead, bound)
            for i, s in enumerate(seeds):
                eb, ec = rbo.greedy_extend(og, s, direction, lookahead, bound)
                assert int(ln[i]) == len(eb) and bytes(bases[i, :ln[i]]) == eb and (c[i, :ln[i]] == np.array(ec, np.float32)).all(), (direction, i)
        for mode, kw in ((1, dict(bound=50)), (2, dict(bound=50, minKmerCov=TOP))):
            got, why = gg.naiveExtend(seeds, direction, mode, **kw)
            for i, s in enumerate(seeds):
                eb, er = rbo.naive_extend(og, s, direction, mode, bound=kw["bound"], min_cov=kw.get("minKmerCov", 1.0))
                assert got[i] == eb and int(why[i]) == er, (direction, mode, i)


def test_sharded_walks_over_saturated_kmers(oracles):
    """the same walks on a sharded graph (rb_shard_trav_*) built from the same two files, against the oracle's restatements"""
    o = oracles["k25_two_files"]
    og = o.og
    cl = LoopbackCluster(4, SIZES[0], o.cbf_bytes, SIZES[2], 2, 2, 2, 25, False, True, rngSeed=5)
    cl.setReadPairedKmerDistance(DIST)
    (ls, lq, lo), (rs, rq, ro) = workload(False)
    cl.addBatch(ReadBatch.from_ascii(ls, lq, lo, 3), 150, storeReadPairedKmers=True)
    cl.addBatch(ReadBatch.from_ascii(rs, rq, ro, 3), 150, reverseComplement=True, storeReadPairedKmers=True)
    assert (cl.exportFilter(N.CBF) == o.snap[1][1]).all()
    seeds = walk_seeds()
    cuts = [0, 10, 10, 60, len(seeds)]
    parts = [seeds[cuts[i]:cuts[i + 1]] for i in range(4)]
    for direction in (0, 1):
        got = cl.traverse(0, parts, direction, bound=50, min_cov=1.0)
        for rk in range(4):
            bases, _, _, c, ln, reason, _ = got[rk]
            for j, s in enumerate(parts[rk]):
                eb, ec, er = rbo.walk_max_cov(og, s, direction, 50, 1.0)
                assert int(reason[j]) == er and int(ln[j]) == len(eb) and bytes(bases[j, :ln[j]]) == eb
                assert (c[j, :ln[j]] == np.array(ec, np.float32)).all()
        got = cl.greedyExtend(parts, direction, 4, 30, answer_cap=1024)
        for rk in range(4):
            bases, c, ln, _ = got[rk]
            for j, s in enumerate(parts[rk]):
                eb, ec = rbo.greedy_extend(og, s, direction, 4, 30)
                assert int(ln[j]) == len(eb) and bytes(bases[j, :ln[j]]) == eb and (c[j, :ln[j]] == np.array(ec, np.float32)).all()
        got = cl.naiveExtend(parts, direction, 1, bound=50)
        for rk in range(4):
            eb_all, why = got[rk]
            for j, s in enumerate(parts[rk]):
                eb, er = rbo.naive_extend(og, s, direction, 1, bound=50)
                assert eb_all[j] == eb and int(why[j]) == er
    cl.destroy()
