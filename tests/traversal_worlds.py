"""The worlds of tests/test_gpu_traversal_matrix.py and tests/test_traversal_reach.py: graphs for the traversal calls (getNeighbors, walkMaxCov,
greedyExtend, naiveExtend, getMaxCoveragePaths and their sharded replay) at k = 16 ... 256, stranded and canonical, with hash counts other than
(2, 2), in two filter sizings — BRANCHY (small filters, reads with 2 % substitutions: false-positive neighbours) and CLEAN (large filters, 0.4 %).
A world holds the oracle graph (and, with device=True, the device graph built from the same reads, after comparing their filters byte for byte);
the oracle's answers (oracle/rbo.py: Graph.neighbors, Graph.get_kmers, walk_max_cov, get_max_coverage_path, greedy_extend, naive_extend, variant)
are computed once per world and shared by the CPU file (which proves that the worlds ask something) and the GPU file (which compares).
path_answers takes SeqUtils.isLowComplexityShort from rnabloom.graphutils (host code; importing the package needs the built library, not a GPU),
so the CPU file, like tests/test_hash_counts_reach.py, runs on a built tree."""
import ctypes as C
import functools
import math

import numpy as np

from oracle import rbo

ACGT = np.frombuffer(b"ACGT", np.uint8)
KS = (16, 31, 32, 33, 63, 64, 65, 96, 128, 143, 256)
HASHES = ((1, 1), (3, 4), (2, 3), (3, 1), (2, 2))               # (dbgbf, cbf)
# (k, stranded, (dbg_h, cbf_h), branchy).  Case number i = 2 * (index of k) + (0 stranded, 1 canonical); hash counts go round in i, so each
# occurs four or five times, on both strandednesses, once at least with k >= 64; per k one world is branchy and one clean, the strandedness
# of the branchy one alternating from k to k.
CASES = tuple((k, i % 2 == 0, HASHES[i % 5], (i // 2 + i) % 2 == 0) for i, k in ((2 * j + s, k) for j, k in enumerate(KS) for s in (0, 1)))
PATH_CASES = (CASES[6], CASES[17])                              # k = 33 stranded, k = 128 canonical (both clean)
GATE_CASES = {CASES[3]: 1, CASES[12]: 3}                        # world -> hash count of the stand-alone gate filter (k = 31 canonical, k = 65 stranded)
SHARD_CASES = (CASES[4], CASES[15])                             # k = 32 stranded (2, 2); k = 96 canonical (1, 1); both branchy

WALK_SETTINGS = ((1.0, 60), (2.0, 30), (4.0, 10), (1.0, 1))      # (min_cov, bound)
REPEAT_PERIOD = 12                                              # + 1 < every bound the repeat seed is asked to loop under (naive 20, walks 60 / 100)
REPEAT_BOUND = 100
GREEDY_N = 40


def greedy_settings(branchy):
    """(lookahead, bound, number of seeds).  Lookahead 16 — the most the C ABI takes — runs here in the clean worlds, eight steps of twenty
    seeds; where there are branches the depth-first search is exponential (in a branchy world the restatement opens 50 000 to 200 000
    neighbourhoods per step of ONE seed, seconds of Python, and a lane of the kernel as many): DEEP_CASES / deep_answers have the reduced form"""
    return ((0, 10, GREEDY_N), (1, 10, GREEDY_N), (2, 20, GREEDY_N), (3, 30, GREEDY_N)) + (() if branchy else ((16, 8, 20),))


# lookahead 16 in branchy worlds: ONE step of DEEP_N seed that has a decision to make, per direction, in three of them (k = 16 stranded (1, 1), k = 64 canonical
# (3, 4), k = 65 stranded (2, 3): 4 to 7 s of Python each).  Here nearly every level of the search holds two or more siblings: the kernel's frontier rows, their
# fr_n / fr_next backtracking down to depth 15 and the bases written ahead of the walk under repeated re-descents are all in use.
DEEP_CASES = (CASES[0], CASES[11], CASES[12])
DEEP_N = 1


class Memo:
    """the oracle graph with Graph.neighbors remembered: the restatement of the lookahead search asks for the same neighbourhoods over and over"""

    def __init__(self, og):
        self.og, self.known, self.by_hash = og, {}, {}

    def neighbors(self, f, r, char_out, direction):
        key = (int(f), int(r), int(char_out), direction)
        if key not in self.known:
            self.known[key] = self.by_hash[(int(f), int(r), direction)] = self.og.neighbors(f, r, char_out, direction)
        return self.known[key]

    def forks_per_level(self, f, r, direction, depth):
        """of the neighbourhoods a search from (f, r) opened: per distance from it, how many hold two or more neighbours with a count"""
        out, cur = [], {(int(f), int(r))}
        for _ in range(depth):
            nxt, forks = set(), 0
            for fr in cur:
                v = self.by_hash.get(fr + (direction,))
                if v is not None:
                    live = [i for i in range(4) if v[2][i] >= 1]
                    forks += len(live) >= 2
                    nxt |= {(int(v[0][i]), int(v[1][i])) for i in live}
            out.append(forks)
            cur = nxt
        return out


NAIVE_SETTINGS = ((0, dict(cap=64)), (0, dict(cap=3)), (1, dict(bound=20)), (1, dict(bound=0)), (2, dict(bound=20)), (2, dict(bound=0)),
                  (1, dict(bound=20, minKmerCov=2.0)), (2, dict(bound=20, minKmerCov=2.0)))
NAIVE_N = 60
PATH_SETTINGS = ((70, 1.0), (20, 2.0), (8, 1.0))                 # (bound, min_cov), as test_get_max_coverage_paths_match_oracle


def case_id(case):
    k, stranded, hashes, branchy = case
    return "k%d-%s-h%d%d-%s" % (k, "stranded" if stranded else "canonical", hashes[0], hashes[1], "branchy" if branchy else "clean")


def _prime_above(n):
    n = int(n) | 1
    while any(n % d == 0 for d in range(3, int(math.isqrt(n)) + 1, 2)):
        n += 2
    return n


def _filter_size(n_items, h, fpr):
    """slots for which a filter with h functions holding n_items reaches the false-positive rate fpr"""
    return _prime_above(-h * n_items / math.log(1.0 - fpr ** (1.0 / h)))


def pack(reads):
    seq = np.frombuffer(b"".join(reads), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    return seq, off


class World:
    N_READS = 300
    GENOME = 3500

    def __init__(self, k, stranded, hashes, branchy, device=False):
        self.case = (k, stranded, tuple(hashes), branchy)
        self.k, self.stranded, self.hashes, self.branchy = k, stranded, tuple(hashes), branchy
        rng = np.random.default_rng(1000 * k + 10 * hashes[0] + hashes[1] + (500 if stranded else 0))
        rnd = lambda n: bytes(ACGT[rng.integers(0, 4, n)])
        L = self.read_len = max(150, k + 120)
        genome = np.frombuffer(rnd(self.GENOME), np.uint8)
        err = 0.02 if branchy else 0.004
        reads = []
        for _ in range(self.N_READS):
            p = int(rng.integers(0, self.GENOME - L + 1))
            rd = genome[p:p + L].copy()
            e = np.nonzero(rng.random(L) < err)[0]
            rd[e] = ACGT[(np.searchsorted(ACGT, rd[e]) + rng.integers(1, 4, e.size)) % 4]       # a substitution is another base
            reads.append(rd.tobytes())
        self.genome_reads = list(reads)
        self.unit = rnd(REPEAT_PERIOD)
        self.repeat_read = (self.unit * (L // REPEAT_PERIOD + 1))[:L]
        X, Y, Z = (rnd(k + 15) for _ in range(3))
        self.fork = (X, Y, Z)
        reads += [self.repeat_read] + [X + Y] * 5 + [X + Z]
        self.reads = reads
        distinct = len({rd[p:p + k] for rd in reads for p in range(len(rd) - k + 1)})
        # false-positive rates of dbgbf and cbf.  A k-mer that dbgbf holds counts at least 1 (cbf counts the occurrences after the first), so
        # dbgbf's rate is the rate of false neighbours: every second absent k-mer in a branchy world (as the filters of
        # test_greedy_extend_with_lookahead_matches_oracle give), one in fifty in a clean one
        fd, fc = (0.5, 0.1) if branchy else (0.02, 0.002)
        self.sizes = (_filter_size(distinct, hashes[0], fd), _filter_size(distinct, hashes[1], fc))
        self._build(device)
        # seeds: k-mers of the reads; [1] has an N, [2] is in lower case, [3] has a U for a T, [4] lies in the tandem repeat; the last two are
        # the ends of the fork's rare arm (X + Z occurs once and is connected to nothing else: dead ends)
        seeds, self.seed_read = [], []
        while len(seeds) < 98:
            r = int(rng.integers(0, self.N_READS)); p = int(rng.integers(0, L - k + 1))
            sd = reads[r][p:p + k]
            if len(seeds) == 3 and b"T" not in sd:
                continue
            seeds.append(sd); self.seed_read.append(r)
        seeds[1] = seeds[1][:k // 3] + b"N" + seeds[1][k // 3 + 1:]
        seeds[2] = seeds[2].lower()
        seeds[3] = seeds[3].replace(b"T", b"U", 1)
        seeds[4] = self.repeat_read[17:17 + k]; self.seed_read[4] = self.N_READS
        seeds += [(X + Z)[-k:], (X + Z)[:k]]; self.seed_read += [len(reads) - 1] * 2
        self.seeds = seeds
        self.n_invalid = sum(any(c not in b"ACGTUacgtu" for c in sd) for sd in seeds)

    def _build(self, device):
        """the oracle graph of self.reads and, with device, the device graph; nothing is compared before their filters are byte-equal"""
        (dbg, cbf), (dh, ch) = self.sizes, self.hashes
        self.seq, self.off = pack(self.reads)
        self.og = rbo.Graph(dbg, cbf, 64, dh, ch, 1, self.k, self.stranded, False, 3)
        self.og.add_reads(self.seq, None, self.off, 3, 0)
        self.gg = None
        if device:
            from rnabloom import _native as N
            from rnabloom.graph import BloomFilterDeBruijnGraph
            self.gg = BloomFilterDeBruijnGraph(dbg, cbf, 64, dh, ch, 1, self.k, self.stranded, False, rngSeed=3)
            self.gg.addReads(self.seq, None, self.off, 3)
            assert (self.gg.exportFilter(N.DBGBF) == self.og.dbgbf_bytes()).all(), "dbgbf differs"
            assert (self.gg.exportFilter(N.CBF) == self.og.cbf_bytes()).all(), "cbf differs"

    @classmethod
    def small(cls, k, stranded, reads, device=False):
        """a world of a few given reads (two hash functions, filters far larger than the reads need): no seeds of its own"""
        w = cls.__new__(cls)
        w.k, w.stranded, w.hashes, w.branchy, w.reads, w.sizes = k, stranded, (2, 2), False, list(reads), (100_003, 200_003)
        w._build(device)
        return w

    def destroy(self):
        if self.gg is not None:
            self.gg.destroy(); self.gg = None

    def plain(self, sd):
        return sd.upper().replace(b"U", b"T")

    def walk_kmers(self, seed, appended, direction):
        """the k-mers of a walk in the order it found them"""
        k, n = self.k, len(appended)
        s = self.plain(seed) + appended if direction == 0 else appended[::-1] + self.plain(seed)
        return [s[j + 1:j + 1 + k] for j in range(n)] if direction == 0 else [s[n - 1 - j:n - 1 - j + k] for j in range(n)]

    def walk_hashes(self, seed, appended, direction):
        """(f, r) of those k-mers, from the oracle's getKmers of the walked string"""
        n = len(appended)
        if not n:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
        s = self.plain(seed) + appended if direction == 0 else appended[::-1] + self.plain(seed)
        f, r, _ = self.og.get_kmers(s)
        return (f[1:], r[1:]) if direction == 0 else (f[:n][::-1], r[:n][::-1])


@functools.lru_cache(maxsize=None)
def world(case):
    return World(*case)


def make_targets(w, free, direction):
    """as tests/test_gpu_sharded_walks.py: the k-mer the free walk reaches after a few steps (the targeted walk stops there), or an unrelated one"""
    k, tg = w.k, []
    for i, sd in enumerate(w.seeds):
        app = free[i][0]
        if len(app) >= 4 and i % 3:
            tg.append(w.walk_kmers(sd, app, direction)[3])
        else:
            tg.append(w.plain(w.seeds[(i + 7) % len(w.seeds)]).replace(b"N", b"A"))
    return tg


@functools.lru_cache(maxsize=None)
def walk_answers(case):
    """{(direction, min_cov, bound, targeted): (targets or None, [(bases, counts, reason, f, r) per seed])}, and the repeat seed's walk without
    a target under REPEAT_BOUND as key (direction, 'repeat')"""
    w = world(case)
    out = {}
    for direction in (0, 1):
        for min_cov, bound in WALK_SETTINGS:
            free = [rbo.walk_max_cov(w.og, sd, direction, bound, min_cov, None, k=w.k, stranded=w.stranded) for sd in w.seeds]
            tg = make_targets(w, free, direction)
            aimed = [rbo.walk_max_cov(w.og, sd, direction, bound, min_cov, tg[i], k=w.k, stranded=w.stranded) for i, sd in enumerate(w.seeds)]
            for targeted, res in ((False, free), (True, aimed)):
                out[(direction, min_cov, bound, targeted)] = (tg if targeted else None,
                                                              [(b, c, why) + w.walk_hashes(sd, b, direction) for sd, (b, c, why) in zip(w.seeds, res)])
        b, c, why = rbo.walk_max_cov(w.og, w.seeds[4], direction, REPEAT_BOUND, 1.0, None, k=w.k, stranded=w.stranded)
        out[(direction, "repeat")] = (None, [(b, c, why) + w.walk_hashes(w.seeds[4], b, direction)])
    return out


def greedy_seeds(w):
    return [sd for sd in w.seeds[4:] if sd == w.plain(sd)][:GREEDY_N]


class OracleGate:
    """a stand-alone Bloom filter of the oracle holding the k-mers of a third of the genome reads: the `bf` of the gated greedy extension"""

    def __init__(self, w, num_hash):
        self.L, self.k, self.nh = rbo.lib(), w.k, num_hash
        self.size = _prime_above(40 * w.GENOME)
        self.ob = self.L.rbo_bloom_new(self.size, num_hash)
        h0 = [rbo.hash_region(rd, w.k, 1, rbo.FWD if w.stranded else rbo.CANON)[0][:, 0] for rd in w.genome_reads[:w.N_READS // 3]]
        self.h0 = np.unique(np.concatenate(h0))
        for x in self.h0:
            self.L.rbo_bloom_add(C.c_void_p(self.ob), rbo._p(rbo.ntm64(int(x), self.k, self.nh)))

    def __del__(self):
        if getattr(self, "ob", None):
            self.L.rbo_bloom_free(C.c_void_p(self.ob))
            self.ob = None

    def __call__(self, h):
        return bool(self.L.rbo_bloom_lookup(C.c_void_p(self.ob), rbo._p(rbo.ntm64(int(h), self.k, self.nh))))

    def bytes(self):
        n = C.c_int64()
        p = self.L.rbo_bloom_bytes(C.c_void_p(self.ob), C.byref(n))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (n.value,)).copy()


@functools.lru_cache(maxsize=None)
def gate_of(case):
    return OracleGate(world(case), GATE_CASES[case])


@functools.lru_cache(maxsize=None)
def greedy_answers(case):
    """{(direction, lookahead, bound, gated): [(bases, counts) per greedy seed]}; (direction, 'plain'): the maximum-count walk's bases under the
    bound of lookahead 3; (direction, 'once', lookahead): one step"""
    w = world(case)
    seeds = greedy_seeds(w)
    out, og = {}, Memo(w.og)
    for direction in (0, 1):
        for lookahead, bound, n in greedy_settings(w.branchy):
            out[(direction, lookahead, bound, False)] = [rbo.greedy_extend(og, sd, direction, lookahead, bound, k=w.k, stranded=w.stranded) for sd in seeds[:n]]
        out[(direction, "plain")] = [rbo.walk_max_cov(w.og, sd, direction, 30, 1.0, None, k=w.k, stranded=w.stranded)[0] for sd in seeds]
        for lookahead in (0, 3):
            out[(direction, "once", lookahead)] = [rbo.greedy_extend(og, sd, direction, lookahead, 1, k=w.k, stranded=w.stranded) for sd in seeds]
        if case in GATE_CASES:
            gate = gate_of(case)
            out[(direction, 3, 30, True)] = [rbo.greedy_extend(og, sd, direction, 3, 30, k=w.k, gate=gate, stranded=w.stranded) for sd in seeds]
    return out


def deep_seeds(w, direction):
    """the first DEEP_N greedy seeds with two or more candidates in that direction: the others are extended without a search"""
    out = []
    for sd in greedy_seeds(w):
        f, r, _ = w.og.get_kmers(sd)
        if (w.og.neighbors(f[0], r[0], sd[0] if direction == 0 else sd[-1], direction)[2] >= 1).sum() >= 2:
            out.append(sd)
        if len(out) == DEEP_N:
            break
    return out


@functools.lru_cache(maxsize=None)
def deep_answers(case):
    """{direction: (seeds, [(bases, counts) per seed], [forks per level of the search, per seed])}: one step under lookahead 16"""
    w = world(case)
    out = {}
    for direction in (0, 1):
        seeds, res, levels = deep_seeds(w, direction), [], []
        for sd in seeds:
            og = Memo(w.og)
            res.append(rbo.greedy_extend(og, sd, direction, 16, 1, k=w.k, stranded=w.stranded))
            fr = rbo.hash_region(sd, w.k, 1, 1)[1]                       # the hashes greedy_extend starts from
            levels.append(og.forks_per_level(fr[0, 0], fr[0, 1], direction, 16))
        out[direction] = (seeds, res, levels)
    return out


def naive_inputs(w):
    """(seeds, terminators): the first NAIVE_N seeds and the two dead ends; every other seed lies inside its own terminator sequence (its read),
    the others get another read; three edge cases: a terminator shorter than k, one with an N in it, one in lower case"""
    idx = list(range(NAIVE_N)) + [len(w.seeds) - 2, len(w.seeds) - 1]
    seeds = [w.seeds[i] for i in idx]
    terms = [w.reads[w.seed_read[i]] if j % 2 == 0 else w.reads[(w.seed_read[i] + 11) % w.N_READS] for j, i in enumerate(idx)]
    terms[6] = terms[6][:w.k - 1]
    terms[8] = terms[8][:w.read_len // 2] + b"N" + terms[8][w.read_len // 2 + 1:]
    terms[10] = terms[10].lower()
    return seeds, terms


@functools.lru_cache(maxsize=None)
def naive_answers(case):
    """{(direction, number of the setting): [(bases, reason) per naive seed]}"""
    w = world(case)
    seeds, terms = naive_inputs(w)
    out = {}
    for direction in (0, 1):
        for s, (mode, kw) in enumerate(NAIVE_SETTINGS):
            out[(direction, s)] = [rbo.naive_extend(w.og, sd, direction, mode, bound=kw.get("bound", 0), min_cov=kw.get("minKmerCov", 1.0),
                                                    terminators=terms[i] if mode == 0 else b"", k=w.k, cap=kw.get("cap", 4096)) for i, sd in enumerate(seeds)]
    return out


@functools.lru_cache(maxsize=None)
def neighbor_answers(case):
    """(f, r, {direction: (char_out, f4, r4, c4)}) for about 200 k-mers of the reads and 20 that are not in the graph; directions 0 / 1 from
    Graph.neighbors, 2 / 3 (left / right variants) from rbo.variant and Graph.get_count"""
    w = world(case)
    k, og = w.k, w.og
    rng = np.random.default_rng(77 + k)
    kmers = []
    for r in rng.integers(0, len(w.reads), 40):
        rd = w.reads[int(r)]
        kmers += [rd[p:p + k] for p in range(int(rng.integers(0, 7)), len(rd) - k + 1, max(7, (len(rd) - k + 1) // 5))][:5]
    kmers += [bytes(ACGT[rng.integers(0, 4, k)]) for _ in range(20)]
    fr = [og.get_kmers(km) for km in kmers]
    f = np.array([x[0][0] for x in fr], np.uint64); r = np.array([x[1][0] for x in fr], np.uint64)
    out = {}
    for direction in range(4):
        ch = np.array([km[0] if direction in (0, 2) else km[-1] for km in kmers], np.uint8)
        f4 = np.zeros((len(kmers), 4), np.uint64); r4 = np.zeros((len(kmers), 4), np.uint64); c4 = np.zeros((len(kmers), 4), np.float32)
        for i in range(len(kmers)):
            if direction < 2:
                f4[i], r4[i], c4[i] = og.neighbors(f[i], r[i], int(ch[i]), direction)
            else:
                for b, base in enumerate(b"ACGT"):
                    vf, vr, vh = rbo.variant(int(f[i]), int(r[i]), int(ch[i]), base, k, og.h, not w.stranded, direction - 2)
                    f4[i, b], r4[i, b], c4[i, b] = vf, vr, og.get_count(vh)
        out[direction] = (ch, f4, r4, c4)
    return f, r, out


def kmer_texts(w):
    """sequences for getKmers: reads, the seed with an N, the lower-case one, one shorter than k, an empty one"""
    return w.reads[:6] + [w.repeat_read, w.seeds[1] + w.reads[7][:40], w.seeds[2], w.reads[9][:w.k - 1], b""]


@functools.lru_cache(maxsize=None)
def path_answers(case):
    """(lefts, rights, {(bound, min_cov): [path or None per pair]}, the set of ways a path was found)"""
    from rnabloom.graphutils import isLowComplexityShort
    w = world(case)
    k = w.k
    rng = np.random.default_rng(9 + k)
    X, Y, Z = w.fork
    # the fork: the walk from the left takes the arm seen five times; the walk from the right comes back along the rare arm and arrives at left
    lefts, rights = [X[-k:]], [(X + Z)[len(X) - k + 20:len(X) + 20]]              # 20 steps apart whatever k is
    for _ in range(160):
        r = int(rng.integers(0, w.N_READS)); p = int(rng.integers(0, 60)); d = int(rng.integers(1, 60))
        lefts.append(w.reads[r][p:p + k])
        rights.append(w.reads[r][p + d:p + d + k] if rng.random() < 0.85 else w.reads[int(rng.integers(0, w.N_READS))][3:3 + k])
    trace, out = [], {}
    for bound, min_cov in PATH_SETTINGS:
        out[(bound, min_cov)] = [rbo.get_max_coverage_path(w.og, lefts[i], rights[i], bound, min_cov, k=k, low_complexity=isLowComplexityShort, trace=trace)
                                 for i in range(len(lefts))]
    return lefts, rights, out, set(trace)


# ---- k-mers with equal hashes and different bases (ntHash at k = 64: a rotation by 64 is none) ----
def hash_equal_world(stranded, device=False):
    """the graph of the single read (AC) x 50 at k = 64: (AC)^32, (CA)^32, (GT)^32 and (TG)^32 all hash to f = 0, r = 0"""
    return World.small(64, stranded, [b"AC" * 50], device)


HASH_EQUAL_SEED = b"AC" * 32
HASH_EQUAL_TWINS = (b"AC" * 32, b"CA" * 32, b"GT" * 32, b"TG" * 32)
# call -> (number of appended bases, reason) the oracle must give; what a kernel that trusts the hash would give is in the right column of the
# table in the docstring of test_gpu_traversal_matrix.py::test_hash_equal_kmers_with_different_bases
HASH_EQUAL_TABLE = {"walk": (2, 2), "walk_to_seed": (1, 1), "naive2": (1, 7), "naive1": (21, 3), "naive0_gt": (2, 5), "naive0_ca": (0, 5)}


@functools.lru_cache(maxsize=None)
def hash_equal_answers(stranded, direction):
    """{call: (bases, reason[, counts])} of the oracle for the seed (AC)^32"""
    og, sd = hash_equal_world(stranded).og, HASH_EQUAL_SEED
    b1, c1, y1 = rbo.walk_max_cov(og, sd, direction, 50, 1.0, None, k=64, stranded=stranded)
    b2, c2, y2 = rbo.walk_max_cov(og, sd, direction, 50, 1.0, sd, k=64, stranded=stranded)
    out = {"walk": (b1, y1, c1), "walk_to_seed": (b2, y2, c2)}
    out["naive2"] = rbo.naive_extend(og, sd, direction, 2, bound=20, k=64)
    out["naive1"] = rbo.naive_extend(og, sd, direction, 1, bound=20, k=64)
    out["naive0_gt"] = rbo.naive_extend(og, sd, direction, 0, terminators=b"GT" * 40, k=64, cap=64)
    out["naive0_ca"] = rbo.naive_extend(og, sd, direction, 0, terminators=b"CA" * 32, k=64, cap=64)
    return out


def homopolymer_world(k, stranded, device=False):
    """the read P + A x (k + 6), P = 40 random bases: a walk to the right from the read's first k-mer runs into A^k after 40 steps"""
    P = bytes(ACGT[np.random.default_rng(k).integers(0, 4, 39)]) + b"C"
    w = World.small(k, stranded, [P + b"A" * (k + 6)], device)
    w.seeds = [w.reads[0][:k]]
    return w


HOMOPOLYMER_FALSE_TARGET = {64: b"C", 128: b"G"}               # at k = 64 C^64 hashes as A^64 does; at k = 128 all four homopolymers hash to (0, 0)


@functools.lru_cache(maxsize=None)
def homopolymer_answers(k, stranded):
    """{'true' | 'false' | 'unrelated': (target, bases, counts, reason)} of the oracle's walk to the right under bound 60"""
    w = homopolymer_world(k, stranded)
    out = {}
    for name, tg in (("true", b"A" * k), ("false", HOMOPOLYMER_FALSE_TARGET[k] * k), ("unrelated", bytes(ACGT[np.random.default_rng(5).integers(0, 4, k)]))):
        out[name] = (tg,) + rbo.walk_max_cov(w.og, w.seeds[0], 0, 60, 1.0, tg, k=k, stranded=stranded)
    return out
