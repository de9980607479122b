"""The graph traversals beyond k = 25 and two hash functions: rb_graph_neighbors, rb_graph_walk, rb_graph_greedy_extend, rb_graph_naive_extend
(k_neighbors, k_walk_max_cov, k_greedy_extend / walk_neighbors, k_naive_extend in csrc/rb_query.hip), graphutils.getMaxCoveragePaths on top of them
and rb_shard_trav_*, the sharded replay of the same kernel bodies, on the worlds of tests/traversal_worlds.py: k = 16 ... 256 (rotation distances
k and k - 1 mod 64 = 63 / 62, 0 / 63, 1 / 0, ...; from-scratch hashes with rotations of 64 and more; rows of k + bound bytes), stranded and
canonical, hash counts (1, 1), (3, 4), (2, 3), (3, 1), (2, 2), gate filters with 1 and 3 functions, lookahead up to the C ABI's 16.  Every
expected value is the CPU oracle's (oracle/rbo.py: Graph.neighbors, Graph.get_kmers, walk_max_cov, get_max_coverage_path, greedy_extend,
naive_extend, variant), computed once per world in traversal_worlds; tests/test_traversal_reach.py proves on the CPU that the worlds ask
something.  Every comparison is exact: bases, lengths and reasons as integers, counts and hashes as bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rnabloom import _native as N
from rnabloom.graph import ReadBatch

import traversal_worlds as TW

IDS = [TW.case_id(c) for c in TW.CASES]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_walks(w, got, want, seeds, bound, tag, hashes=True, counts=True):
    """walkMaxCov's (bases, f, r, count, len, reason) against the oracle's [(bases, counts, reason, f, r)]"""
    gb, gf, gr, gc, gl, gy = got
    assert gb.shape == (len(seeds), bound)
    for i, (eb, ec, ey, ef, er) in enumerate(want):
        n = int(gl[i])
        assert (n, int(gy[i])) == (len(eb), ey), (tag, i, n, int(gy[i]), len(eb), ey)
        assert bytes(gb[i, :n]) == eb, (tag, i)
        if counts:
            assert (bits(gc[i, :n]) == bits(ec)).all(), (tag, i)
        if hashes:
            assert (gf[i, :n] == ef).all(), (tag, i)
            if not w.stranded:
                assert (gr[i, :n] == er).all(), (tag, i)
    if not hashes:
        assert gf is None and gr is None
    if not counts:
        assert gc is None


def check_greedy(got, want, bound, tag):
    gb, gc, gl, gy = got
    for i, (eb, ec) in enumerate(want):
        n = int(gl[i])
        assert n == len(eb) and bytes(gb[i, :n]) == eb, (tag, i, n, len(eb))
        assert (bits(gc[i, :n]) == bits(ec)).all(), (tag, i)
        assert int(gy[i]) == (3 if len(eb) == bound else 0), (tag, i)


def split(x, cuts):
    return [x[cuts[i]:cuts[i + 1]] for i in range(len(cuts) - 1)]


@pytest.fixture(scope="module")
def worlds():
    """device worlds, built on first use and kept for the module (the sharded replay uses two of them again)"""
    made = {}

    def get(case):
        if case not in made:
            made[case] = TW.World(*case, device=True)
        return made[case]
    yield get
    for w in made.values():
        w.destroy()


@pytest.mark.parametrize("case", TW.CASES, ids=IDS)
def test_neighbours_variants_and_kmers(worlds, case):
    w = worlds(case)
    gg, og = w.gg, TW.world(case).og
    f, r, by_dir = TW.neighbor_answers(case)
    for direction in range(4):
        ch, ef4, er4, ec4 = by_dir[direction]
        f4, r4, c4 = gg.getNeighbors(f, r, ch, direction)
        assert (f4 == ef4).all() and (bits(c4) == bits(ec4)).all(), direction
        if not w.stranded:
            assert (r4 == er4).all(), direction
    texts = TW.kmer_texts(w)
    ko, gf, gr, gc = gg.getKmers(texts)
    for i, s in enumerate(texts):
        ef, er, ec = og.get_kmers(s)
        a, b = int(ko[i]), int(ko[i + 1])
        assert b - a == len(ef) and (gf[a:b] == ef).all() and (bits(gc[a:b]) == bits(ec)).all(), i
        if not w.stranded:
            assert (gr[a:b] == er).all(), i


@pytest.mark.parametrize("case", TW.CASES, ids=IDS)
def test_max_coverage_walks(worlds, case):
    w = worlds(case)
    wa = TW.walk_answers(case)
    for direction in (0, 1):
        for s, (min_cov, bound) in enumerate(TW.WALK_SETTINGS):
            for targeted in (False, True):
                tg, want = wa[(direction, min_cov, bound, targeted)]
                tag = (direction, min_cov, bound, targeted)
                check_walks(w, w.gg.walkMaxCov(w.seeds, direction, bound, min_cov, tg), want, w.seeds, bound, tag)
                if s == int(targeted):                            # the calls without the hash rows / without the count rows
                    check_walks(w, w.gg.walkMaxCov(w.seeds, direction, bound, min_cov, tg, hashes=False), want, w.seeds, bound, tag + ("no hashes",), hashes=False)
                    check_walks(w, w.gg.walkMaxCov(w.seeds, direction, bound, min_cov, tg, counts=False), want, w.seeds, bound, tag + ("no counts",), counts=False)
        # the tandem repeat under a bound of 100: the walk meets its own path after one period
        _, want = wa[(direction, "repeat")]
        assert (len(want[0][0]), want[0][2]) == (TW.REPEAT_PERIOD, 2)
        check_walks(w, w.gg.walkMaxCov([w.seeds[4]], direction, TW.REPEAT_BOUND, 1.0), want, [w.seeds[4]], TW.REPEAT_BOUND, (direction, "repeat"))


@pytest.mark.parametrize("case", TW.CASES, ids=IDS)
def test_greedy_extension(worlds, case):
    w = worlds(case)
    ga = TW.greedy_answers(case)
    seeds = TW.greedy_seeds(w)
    for direction in (0, 1):
        for lookahead, bound, n in TW.greedy_settings(w.branchy):
            check_greedy(w.gg.greedyExtend(seeds[:n], direction, lookahead, bound), ga[(direction, lookahead, bound, False)], bound, (direction, lookahead))
        for lookahead in (0, 3):
            bases, cnt = w.gg.greedyExtendOnce(seeds, direction, lookahead)
            for i, (eb, ec) in enumerate(ga[(direction, "once", lookahead)]):
                assert bases[i] == eb and (not eb or bits(cnt[i:i + 1])[0] == bits(ec)[0]), (direction, lookahead, i)
    with pytest.raises(N.NativeError, match=r"lookahead out of range \[0, 16\]"):
        w.gg.greedyExtend(seeds[:2], 0, 17, 4)
    if case in TW.GATE_CASES:
        from rnabloom.bloom import BloomFilter
        gate = TW.gate_of(case)
        bf = BloomFilter(gate.size, gate.nh, w.k)
        bf.add(gate.h0)
        assert (bf.toBytes() == gate.bytes()).all()
        for direction in (0, 1):
            check_greedy(w.gg.greedyExtend(seeds, direction, 3, 30, bf=bf), ga[(direction, 3, 30, True)], 30, (direction, "gate"))
            bases, cnt = w.gg.greedyExtendOnce(seeds, direction, 3, bf=bf)
            for i, (eb, ec) in enumerate(ga[(direction, 3, 30, True)]):
                assert bases[i] == eb[:1] and (not eb or bits(cnt[i:i + 1])[0] == bits(ec[:1])[0]), (direction, "gate once", i)
        bf.destroy()


@pytest.mark.parametrize("case", TW.DEEP_CASES, ids=[TW.case_id(c) for c in TW.DEEP_CASES])
def test_greedy_extension_with_lookahead_16_in_a_branchy_world(worlds, case):
    """one step of one seed per direction: the search tree doubles from level to level (tests/test_traversal_reach.py), so every frontier row of
    k_greedy_extend holds siblings, the backtracking returns to every depth and the bases ahead of the walk are rewritten on each re-descent"""
    w = worlds(case)
    da = TW.deep_answers(case)
    for direction in (0, 1):
        seeds, want, _ = da[direction]
        check_greedy(w.gg.greedyExtend(seeds, direction, 16, 1), want, 1, (direction, 16))
        bases, cnt = w.gg.greedyExtendOnce(seeds, direction, 16)
        for i, (eb, ec) in enumerate(want):
            assert bases[i] == eb and bits(cnt[i:i + 1])[0] == bits(ec)[0], (direction, i)


@pytest.mark.parametrize("case", TW.CASES, ids=IDS)
def test_naive_extension(worlds, case):
    w = worlds(case)
    na = TW.naive_answers(case)
    seeds, terms = TW.naive_inputs(w)
    for direction in (0, 1):
        for s, (mode, kw) in enumerate(TW.NAIVE_SETTINGS):
            got, why = w.gg.naiveExtend(seeds, direction, mode, terminators=terms if mode == 0 else None, **kw)
            for i, (eb, ey) in enumerate(na[(direction, s)]):
                assert (got[i], int(why[i])) == (eb, ey), (direction, mode, kw, i)


@pytest.mark.parametrize("case", TW.PATH_CASES, ids=[TW.case_id(c) for c in TW.PATH_CASES])
def test_max_coverage_paths(worlds, case):
    from rnabloom.graphutils import getMaxCoveragePaths
    w = worlds(case)
    lefts, rights, want, _ = TW.path_answers(case)
    for bound, min_cov in TW.PATH_SETTINGS:
        got = getMaxCoveragePaths(w.gg, lefts, rights, bound, min_cov)
        for i, exp in enumerate(want[(bound, min_cov)]):
            assert got[i] == exp, (bound, min_cov, i)


def cluster_of(w, G, reads=None, sizes=None, hashes=None):
    """the sharded graph of a world's reads on G virtual ranks, its filters compared with the oracle's"""
    from rnabloom.sharded import LoopbackCluster
    sizes, hashes = sizes or w.sizes, hashes or w.hashes
    cl = LoopbackCluster(G, sizes[0], sizes[1], 64, hashes[0], hashes[1], 1, w.k, w.stranded, False, rngSeed=3)
    seq, off = TW.pack(reads) if reads is not None else (w.seq, w.off)
    cl.addBatch(ReadBatch.from_ascii(seq, None, off, 3), max(len(r) for r in (reads or w.reads)), reads_per_substep=120)
    if reads is None:
        assert (cl.exportFilter(N.DBGBF) == w.og.dbgbf_bytes()).all() and (cl.exportFilter(N.CBF) == w.og.cbf_bytes()).all()
    return cl


def same_rows(got, want, a, b, tag):
    """a rank's rows of a sharded traversal against rows [a, b) of the single-GPU call: lengths, reasons, then every row up to its length"""
    ln, reason = got[-2], got[-1]
    assert (ln == want[-2][a:b]).all() and (reason == want[-1][a:b]).all(), tag
    assert not (reason == 8).any(), tag
    for g, e in zip(got[:-2], want[:-2]):
        m = np.arange(g.shape[1])[None, :] < ln[:, None]
        assert (g[m].view(np.uint8) == np.ascontiguousarray(e[a:b])[m].view(np.uint8)).all(), tag


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("case", TW.SHARD_CASES, ids=[TW.case_id(c) for c in TW.SHARD_CASES])
def test_sharded_replay(worlds, case, G):
    """rb_shard_trav_* (the kernels above with the counts coming from the owners through query exchanges) and the sharded getNeighbors against
    the single-GPU calls on the same world — themselves held to the oracle by the tests above — as tests/test_gpu_sharded_walks.py compares"""
    w = worlds(case)
    g1 = w.gg
    cl = cluster_of(w, G)
    seeds = w.seeds[:48]
    rng = np.random.default_rng(4 + G)
    cuts = [0] + sorted(rng.integers(0, len(seeds), G - 1).tolist()) + [len(seeds)]
    if G > 2:
        cuts[1] = cuts[0]                                      # rank 0 has no seeds at all
    wa = TW.walk_answers(case)
    for direction in (0, 1):
        for min_cov, bound in ((1.0, 60), (4.0, 10)):
            for targeted in (False, True):
                tg = wa[(direction, min_cov, bound, targeted)][0]
                tg = tg[:len(seeds)] if tg else None
                eb, ef, er_, ec, el, ey = g1.walkMaxCov(seeds, direction, bound, min_cov, tg)
                got = cl.traverse(0, split(seeds, cuts), direction, bound=bound, min_cov=min_cov, targets=split(tg, cuts) if tg else None)
                for rk in range(G):
                    bases, f, r, c, ln, reason, rounds = got[rk]
                    same_rows((bases, f, r, c, ln, reason), (eb, ef, er_, ec, el, ey), cuts[rk], cuts[rk + 1], (0, direction, min_cov, targeted, rk))
        gseeds = [sd for sd in seeds[4:] if sd == w.plain(sd)][:24]
        gcuts = [min(c, len(gseeds)) for c in cuts[:-1]] + [len(gseeds)]
        for lookahead, bound in ((0, 10), (3, 20)):
            eb, ec, el, ey = g1.greedyExtend(gseeds, direction, lookahead, bound)
            got = cl.greedyExtend(split(gseeds, gcuts), direction, lookahead, bound, answer_cap=1024)
            for rk in range(G):
                same_rows(got[rk], (eb, ec, el, ey), gcuts[rk], gcuts[rk + 1], (1, direction, lookahead, rk))
        nseeds, terms = TW.naive_inputs(w)
        nseeds, terms = nseeds[:len(seeds)], terms[:len(seeds)]
        for mode, kw in ((0, dict(cap=64)), (1, dict(bound=20)), (2, dict(bound=20))):
            eb, ey = g1.naiveExtend(nseeds, direction, mode, terminators=terms if mode == 0 else None, **kw)
            got = cl.naiveExtend(split(nseeds, cuts), direction, mode, terminators=split(terms, cuts) if mode == 0 else None, **kw)
            for rk in range(G):
                a, b = cuts[rk], cuts[rk + 1]
                assert got[rk][0] == eb[a:b] and (got[rk][1] == ey[a:b]).all() and not (got[rk][1] == 8).any(), (2, direction, mode, rk)
    f, r, by_dir = TW.neighbor_answers(case)
    ncuts = [c * f.size // len(seeds) for c in cuts]
    for direction in range(4):
        ch, ef4, er4, ec4 = by_dir[direction]
        got = cl.getNeighbors([(f[a:b], r[a:b], ch[a:b]) for a, b in zip(ncuts[:-1], ncuts[1:])], direction)
        for rk, (a, b) in enumerate(zip(ncuts[:-1], ncuts[1:])):
            f4, r4, c4 = got[rk]
            assert (f4 == ef4[a:b]).all() and (bits(c4) == bits(ec4[a:b])).all() and (w.stranded or (r4 == er4[a:b]).all()), (direction, rk)
    cl.destroy()


def hash_equal_calls(run_walk, run_naive, stranded, direction):
    """the six calls of the table below through the given runners, against the oracle"""
    sd = TW.HASH_EQUAL_SEED
    want = TW.hash_equal_answers(stranded, direction)
    assert {name: (len(v[0]), v[1]) for name, v in want.items()} == TW.HASH_EQUAL_TABLE
    for name, tg in (("walk", None), ("walk_to_seed", [sd])):
        bases, c, ln, reason = run_walk([sd], direction, 50, tg)
        eb, ey, ec = want[name]
        assert (int(ln[0]), int(reason[0]), bytes(bases[0, :ln[0]])) == (len(eb), ey, eb), (name, direction, int(ln[0]), int(reason[0]))
        assert (bits(c[0, :ln[0]]) == bits(ec)).all(), (name, direction)
    for name, mode, kw, term in (("naive2", 2, dict(bound=20), None), ("naive1", 1, dict(bound=20), None),
                                 ("naive0_gt", 0, dict(cap=64), b"GT" * 40), ("naive0_ca", 0, dict(cap=64), b"CA" * 32)):
        got, why = run_naive([sd], direction, mode, [term] if term else None, kw)
        assert (got[0], int(why[0])) == want[name], (name, direction, got[0], int(why[0]))


@pytest.mark.parametrize("stranded", [False, True])
def test_hash_equal_kmers_with_different_bases(stranded):
    """The reference's Kmer.equals compares bytes; the kernels compare the forward hash first and only then the bases — the visited set and the
    target of the walk, the used set and the terminators of naive mode 0, the seed and the last k-mer of mode 2.  ntHash at k = 64 gives k-mers
    that differ and hash alike: in the graph of the single read (AC) x 50, (AC)^32, (CA)^32, (GT)^32 and (TG)^32 all have f = 0, r = 0.  From
    the seed (AC)^32 the oracle gives (asserted here and, on the CPU, in test_traversal_reach.py):

        call                                              expected             a kernel that trusts the hash
        walkMaxCov, bound 50, no target                   len 2, reason 2      len 0 or 1
        walkMaxCov, target = the seed                     len 1, reason 1      len 0, reason 1
        naiveExtend mode 2, bound 20                      1 base, reason 7     0 bases, reason 7
        naiveExtend mode 1, bound 20                      21 bases, reason 3   unchanged (control)
        naiveExtend mode 0, cap 64, terminators GT x 40   2 bases, reason 5    0 bases
        naiveExtend mode 0, terminators (CA)^32           0 bases, reason 5    unchanged (control)

    on one GPU and, since the replay path rebuilds its visited bitmap from the hash rows on resume, on 2 virtual ranks."""
    w = TW.hash_equal_world(stranded, device=True)
    gg, cl = w.gg, None
    ko, f, r, c = gg.getKmers(list(TW.HASH_EQUAL_TWINS))
    assert ko.tolist() == [0, 1, 2, 3, 4] and len({(int(a), int(b)) for a, b in zip(f, r)}) == 1
    ef, er, ec = zip(*(w.og.get_kmers(km) for km in TW.HASH_EQUAL_TWINS))
    assert (f == np.concatenate(ef)).all() and (bits(c) == bits(np.concatenate(ec))).all() and (stranded or (r == np.concatenate(er)).all())

    def one_walk(seeds, direction, bound, tg):
        bases, _, _, c, ln, reason = gg.walkMaxCov(seeds, direction, bound, 1.0, tg)
        return bases, c, ln, reason

    def one_naive(seeds, direction, mode, terms, kw):
        return gg.naiveExtend(seeds, direction, mode, terminators=terms, **kw)

    def two_walk(seeds, direction, bound, tg):                      # rank 1 walks, rank 0 has nothing to do
        bases, _, _, c, ln, reason, _ = cl.traverse(0, [[], seeds], direction, bound=bound, min_cov=1.0, targets=[[], tg] if tg else None)[1]
        return bases, c, ln, reason

    def two_naive(seeds, direction, mode, terms, kw):
        return cl.naiveExtend([[], seeds], direction, mode, terminators=[[], terms] if terms else None, **kw)[1]

    try:
        cl = cluster_of(w, 2)
        for direction in (0, 1):
            hash_equal_calls(one_walk, one_naive, stranded, direction)
            hash_equal_calls(two_walk, two_naive, stranded, direction)
    finally:
        if cl is not None:
            cl.destroy()
        w.destroy()


@pytest.mark.parametrize("k", [64, 128])
@pytest.mark.parametrize("stranded", [False, True])
def test_homopolymer_target_with_the_hashes_of_another(k, stranded):
    """A^64 and C^64 share (f, r) = (~0, 0); at k = 128 all four homopolymers hash to (0, 0).  A walk that runs into A^k stops there when A^k is
    its target (reason 1); with C^64 (G^128) as the target it must do what it does with an unrelated one"""
    w = TW.homopolymer_world(k, stranded, device=True)
    want = TW.homopolymer_answers(k, stranded)
    assert want["true"][3] == 1 and want["false"][1:] == want["unrelated"][1:] and want["false"][3] == 2
    try:
        for name in ("true", "false", "unrelated"):
            tg, eb, ec, ey = want[name]
            bases, f, r, c, ln, reason = w.gg.walkMaxCov(w.seeds, 0, 60, 1.0, [tg])
            assert (int(ln[0]), int(reason[0]), bytes(bases[0, :ln[0]])) == (len(eb), ey, eb), (name, int(ln[0]), int(reason[0]))
            assert (bits(c[0, :ln[0]]) == bits(ec)).all(), name
    finally:
        w.destroy()
