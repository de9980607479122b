"""The worlds of tests/test_gpu_screen_matrix.py and tests/test_screen_reach.py: graphs, gates and queries for rb_graph_screen_fragments,
rb_graph_represented and rb_graph_trim_rc_artifacts at k = 16 ... 256, stranded and canonical, with hash counts other than (2, 2, 2) and a gate
of 1 to 4 hash functions, from the World classes of tests/test_screen_rules.py, tests/test_represented_rules.py and
tests/test_trim_artifact_rules.py.  Those classes were written at k = 25; here every length is derived from k by lengths_of(), so that a world
looks in K-MERS as the k = 25 world does (a length of n letters becomes n + (k - 25), as tests/pair_worlds.py has it), and the offsets inside
the classes were rewritten where they held a 25 in disguise.  Around the lane loops' boundaries k takes both neighbours: a k-mer's letters
go over the lanes 64 at a time, so 63 | 64 | 65, 127 | 128 | 129, 192 | 193 and 255 | 256 end a round, and the rotations by k and k - 1 are by 0,
31, 32 and 63 bits at k = 31 ... 33 and 63 ... 65.

On top of what the classes hold, the screen worlds get gap queries (gap_queries) that only k decides: gaps of exactly 2 k and 2 k + 1
k-mers, which isChimera's `<= maxGap` separates, a gap whose path arrives from the left after k steps, and gaps that getMaxCoveragePath
splices at entry k - 1 and 2 k - 1 of the left walk — beyond the 64 entries a wavefront looks through at a time from k = 65 on.

The CPU file proves that the worlds ask something, the GPU file compares; a world holds its restatement's answers, computed once."""
import collections
import functools
import hashlib

import numpy as np

import test_represented_rules as RR
import test_screen_rules as S
import test_trim_artifact_rules as T
from traversal_worlds import _prime_above

ACGT = b"ACGT"
KS = (16, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256)
# (dbgbf, cbf, pair filters) and the gate's hash count, going round together with the case number
TRIPLES = ((1, 1, 1), (3, 4, 3), (2, 2, 3), (3, 1, 2), (2, 2, 2))
GATES = (1, 3, 2, 4, 2)
DEEP = S.ScreenWorld.LONGEST_TAIL + 16
SCREEN_SETTINGS = ((3, 2), (5, DEEP))                             # (lookahead, max_depth)
IDENTITY_ONE = {(65, True), (192, False)}                         # (k, stranded) of the two cases whose represented runs at identity 1.0

# k, stranded, (dbgbf, cbf, pair) hash counts, the gate's, represented's clip and identity.  Case number i = 2 * (index of k) + (0 stranded,
# 1 canonical); triple and gate count go round in i, so each occurs five or six times, on both strandednesses and on both sides of k = 64.
Case = collections.namedtuple("Case", "k stranded hashes gate_h clip identity")
CASES = tuple(Case(k, s == 0, TRIPLES[(2 * j + s) % 5], GATES[(2 * j + s) % 5], (10, 40)[(j + s) % 2], 1.0 if (k, s == 0) in IDENTITY_ONE else 0.9)
              for j, k in enumerate(KS) for s in (0, 1))

# What a world's assert_every_branch_is_reached asks for and cannot exist at that k: {(call, k): {branch: why}}.  No `why` value of any
# record, none of gap_queries' tags at k >= 65.
EXCUSED = {
    # represented's blunt-artifact and edge-in-the-graph are an edge of 20 and of 15 k-mers that the graph does not spell; at k = 25 they end
    # on the identity test at 0.9.  An edge of n k-mers is a text of n + k - 1 letters of which only the n outermost can differ from the
    # walk's, and failing 0.9 takes more than a tenth of them: more than 14.1 of 15 at k = 127 — every letter of a random edge, which
    # agrees with the walk in one of four — and more than 15 from k = 137 on; of the tail's 20, 15 at k = 127 and more than 20 from 182 on.
    # The check then takes either end of the identity test; edge-a-quarter-off holds both identity `why` values at every k.
    ("repr", k): {"short_edges_fail_identity": "an edge of 15 k-mers cannot differ in a tenth of its k + 14 letters from k = 137 on, and at 127 ... 129 only if all 15 do"}
    for k in KS if k >= 127
}
# LONG's return without a middle stretch (stranded) and its empty range (unstranded) are one condition: the anchor's last k-mer i and the
# partner's first k-mer, matched to each other, are neighbours i and i + 1.  Then x[1 .. k] is the reverse complement of x[0 .. k - 1], letter
# x[j] the complement of x[k - j] for j = 1 .. k — and at an even k letter x[k / 2] its own complement.  No sequence has that.
EXCUSED.update({("trim", k): {"long_p0_no_middle": "two neighbouring k-mers are no reverse complements of each other at an even k",
                              "long_empty_range": "two neighbouring k-mers are no reverse complements of each other at an even k"} for k in KS if k % 2 == 0})

# Which of the rarer branches a world of random transcripts reaches is luck (the k = 25 worlds have their seeds for the same reason): a
# (call, k, stranded) listed here takes the n-th seed behind its own, the first with which its reach checks hold
RESEED = {("screen", 16, True): 3, ("screen", 16, False): 1, ("screen", 31, True): 2, ("screen", 32, False): 1, ("screen", 64, True): 4, ("screen", 65, True): 5,
          ("screen", 65, False): 8, ("screen", 127, True): 1, ("screen", 128, True): 1, ("screen", 129, False): 4, ("screen", 192, True): 2, ("screen", 193, True): 1,
          ("screen", 255, False): 1,
          ("trim", 32, False): 1, ("trim", 128, True): 1, ("trim", 128, False): 1, ("trim", 192, True): 1}      # (trim: the half of the even list began one k-mer off)

CALLS = dict(screen=1, trim=2)


def case_id(case):
    return "k%d-%s-h%d%d%d-g%d" % ((case.k, "stranded" if case.stranded else "canonical") + case.hashes + (case.gate_h,))


def seed_of(case, call):
    return 10_000_000 * RESEED.get((call, case.k, case.stranded), 0) + 1_000_000 * CALLS[call] + 1000 * case.k + 100 * case.hashes[0] + 10 * case.hashes[1] + 2 * case.hashes[2] + (1 if case.stranded else 0)


def grow(k):
    """letters a length of the k = 25 worlds gains"""
    return max(k - 25, 0)


def lengths_of(k):
    """THE rule: ScreenWorld's keywords at k.  Exons of 126 k-mers, reads of 76 k-mers every 10 letters (a k-mer in 7 or 8 reads), as at
    k = 25; the long transcript has more than 1100 k-mers and room for ReprWorld's query of 8 k letters around one changed letter"""
    g = grow(k)
    return dict(seg=150 + g, read_len=75 + k, tile=10, long_len=max(1300 + g, 8 * k + 60))


def sizes_of(case):
    """((dbgbf, cbf, pair filter), gate) slots.  The k = 25 and k = 143 worlds have 4 800 011 / 4 800 011 / 4 800 017 and a gate of 1 200 007
    bits.  Here a changed letter takes k k-mers out of the gate and a world asks some thousands of unassembled k-mers at k = 256: with
    1 200 007 bits and two functions one in 400 of them would count as assembled, and hardly a gap would be the run it was made to be.  The
    gate gets eight times the bits, and with ONE function 32 times — 4.8 MB, the size of the counting filter, the largest filter of
    today's worlds; no filter here is larger.  A dbgbf with one function gets as much: a k-mer counts where dbgbf holds it (getCount), and
    isBranchFree asks six variants of every k-mer of a query.  dbgbf and cbf differ in size, or with one function each a false positive of dbgbf would read
    the count of the very k-mer it collides with (tests/correction_worlds.py)"""
    return (_prime_above(38_400_000 if case.hashes[0] == 1 else 4_700_000), 4_800_011, 4_800_017), _prime_above(38_400_000 if case.gate_h == 1 else 9_600_000)


def digest(*parts):
    """SHA-256 over the repr of lists of reads, queries and records"""
    h = hashlib.sha256()
    for p in parts:
        h.update(repr(p).encode())
        h.update(b"|")
    return h.hexdigest()


def screen_digest(w, settings):
    return digest(w.reads, w.gate_seqs, w.queries, [[st.record for st in w.want(*s)] for s in settings])


def repr_digest(w, settings):
    return digest(w.reads, w.gate_seqs, w.queries, [[st.record for st in w.judged(*s)] for s in settings])


def trim_digest(w, settings):
    return digest(w.reads, w.queries, [[(rec, text) for rec, text in w.judged(*s)] for s in settings])


# ---- the screen and represented worlds ----
def flip(s, *positions):
    for p in positions:
        s = S.put(s, p, chr(S.other(s[p])[0]))
    return s


def gap_queries(w, rng):
    """[(name, sequence)], each to be mirrored.  An assembled stretch with letters changed: a letter at p takes the k k-mers p - k + 1 .. p
    out of the gate; letters at p and p + k a run of exactly 2 k, which isChimera still tries to bridge (`<= maxGap`), and a third at
    p + k + 1 a run of 2 k + 1, which it does not.  (Two letters k + 1 apart leave k-mer p + 1 whole between two runs of k.)  Bridging a
    run of g k-mers is getMaxCoveragePath with bound g between two k-mers g + 1 steps apart: the left walk stops one short, the right
    walk's first k-mer is entry g - 1 of the left walk's list, so a single changed letter is spliced at entry k - 1, the pair at 2 k - 1.
    Three letters inserted make a run of k + 2 whose ends are k steps apart in the graph: the left walk arrives, at its k-th step.
    And letters that are in no transcript between two assembled stretches far apart: nothing bridges them; k + 1 of them are a run of
    2 k (tried, then j - i = 2 k + 1: WIDE_GAP), k of them a run of 2 k - 1 (j - i = 2 k: the walks are compared)."""
    k = w.k
    b1 = w.tx[2][0]
    rnd = lambda n: bytes(ACGT[i] for i in rng.integers(0, 4, n))
    m = k + 35
    base, p = b1[5:4 * k + 60], k + 20
    x = p + k
    ins = [c for c in ACGT if c not in (base[x], base[x - 1])][:1]
    out = [("gap-2k-bridged", flip(base, p, p + k)), ("gap-2k+1", flip(base, p, p + k, p + k + 1)),
           ("insertion-bridged", base[:x] + bytes(ins * 3) + base[x:])]
    big = w.tx[6][0]
    # represented at an identity of 0.9: an edge of n k-mers spells n + k - 1 letters and only n of them can differ, so the tails of 20
    # k-mers pass from k = 182 on whatever they hold.  An edge of max(k, 45) k-mers with every second letter changed fails at every k
    nq = max(k, 45)
    out.append(("edge-a-quarter-off", RR.snvs_every(big[100:100 + nq + k + 35], nq - 1, 2)))
    left, right = b1[:m], big[100:100 + m]                 # (of two transcripts that share nothing)
    for name, n in (("gap-2k-unbridged", k + 1), ("gap-2k-1-unbridged", k)):
        mid = bytearray(rnd(n))
        mid[0] = S.other(b1[m])[0]                               # (the k-mers at the run's ends hold a letter the transcript has not)
        mid[-1] = S.other(big[99])[0]
        out.append((name, left + bytes(mid) + right))
    return out


class MatrixWorld(RR.ReprWorld):
    """ReprWorld (ScreenWorld's graph, gate and queries and more queries) at a case's k with gap_queries, mirrored, behind its own"""

    def __init__(self, case):
        sizes, gate_size = sizes_of(case)
        seed = seed_of(case, "screen")
        super().__init__(case.k, case.stranded, seed, hashes=case.hashes, gate_h=case.gate_h, sizes=sizes, gate_size=gate_size, **lengths_of(case.k))
        self.case = case
        q = gap_queries(self, np.random.default_rng(seed + 5))
        self.queries = self.queries + q + [(name + "~", s[::-1]) for name, s in q]
        self.names = [name for name, _ in self.queries]


@functools.lru_cache(maxsize=2)
def screen_case(case):
    return MatrixWorld(case)


def assert_gaps_are_reached(w, lookahead=3, max_depth=2):
    """the queries of gap_queries end as they were made to"""
    k = w.k
    got = dict(zip(w.names, w.want(lookahead, max_depth)))
    for tilde in ("", "~"):
        rec = lambda name: got[name + tilde].record
        tags = lambda name: got[name + tilde].tags
        assert rec("gap-2k-bridged")[1] == S.CHIM_ASSEMBLED and tags("gap-2k-bridged") >= {"bridged_by_the_forward_scan", "paths_spliced"}, rec("gap-2k-bridged")
        assert rec("gap-2k+1")[1] == S.CHIM_WIDE_GAP and rec("gap-2k+1")[3] - rec("gap-2k+1")[2] == 2 * k + 2, rec("gap-2k+1")
        assert rec("gap-2k-unbridged")[1] == S.CHIM_WIDE_GAP and rec("gap-2k-unbridged")[3] - rec("gap-2k-unbridged")[2] == 2 * k + 1, rec("gap-2k-unbridged")
        r = rec("gap-2k-1-unbridged")
        assert r[1] in (S.CHIM_PATHS_MEET, S.CHIM_DISJOINT) and r[3] - r[2] == 2 * k, r
        assert rec("insertion-bridged")[1] == S.CHIM_ASSEMBLED and "path_from_the_left" in tags("insertion-bridged")
        if k >= 65:
            assert "left_walk_arrives_after_64_steps" in tags("insertion-bridged")
            assert "spliced_at_entry_64_or_beyond" in tags("snv-bridged")
        if 2 * k - 1 >= 64:
            assert "spliced_at_entry_64_or_beyond" in tags("gap-2k-bridged")


def assert_edges_fail_at_every_k(w):
    """represented's two identity `why` values under (3, 1, 10 or 40, 0.9), whatever k"""
    for clip in (10, 40):
        got = w.named(3, 1, clip, 0.9)
        nq = max(w.k, 45)
        assert got["edge-a-quarter-off"].record[:6] == (0, RR.WHY_LEFT_IDENTITY, 0, nq, nq, nq), got["edge-a-quarter-off"].record
        r = got["edge-a-quarter-off~"].record
        assert r[:2] == (0, RR.WHY_RIGHT_IDENTITY) and r[4:6] == (nq, nq), r


def check_case(case, call):
    """what tests/test_screen_reach.py asserts of a case's world of one kind — the condition a seed of RESEED has to meet"""
    if call == "trim":
        T.assert_every_branch_is_reached(trim_case(case), set(EXCUSED.get(("trim", case.k), {})))
        return
    w = screen_case(case)
    w.assert_every_branch_is_reached(3, 2)
    assert_gaps_are_reached(w)
    for setting in SCREEN_SETTINGS:                               # as test_the_other_worlds_reach_their_branches has it
        got = w.want(*setting)
        assert {st.record[1] for st in got} == {0, 1, 2, 3, 4} and {st.record[6] for st in got} == {0, 1, 2, 3, 4, 5, 6}, setting
        assert 0 < w.largest_visit_count(*setting) < S.DEFAULT_VISITS // 4
    RR.assert_every_branch_is_reached(w, set(EXCUSED.get(("repr", case.k), {})))
    assert_edges_fail_at_every_k(w)


# ---- the trim worlds ----
def trim_settings(k):
    """(mode, max_edge_clip, max_cov_gradient): HASHES, and EDGE and LONG under a clip below k, one between k and the longest query's list
    (11 k + 51 k-mers, two-hairpins) and one above every query.  EDGE's low clip is 1: only then the match of seed 0 survives in a hairpin
    (a wider one goes on to seed 1, which matches too).  LONG's is k - 6: above the five letters in front of the stems and below the 2 k
    in front of the -tail queries' stems, so that the scan from the left passes them by and the one from the right runs; its middle clip
    is 3 k / 2 for the same reason, EDGE's 3 k.  LONG's gradient is 1.5 under the middle clip, so that a middle stretch fails
    the gradient test too, and 0.5 elsewhere"""
    return ((T.HASHES, 0, 0.0),) + tuple((mode, clip, grad) for mode, low, mid, grads in ((T.EDGE, 1, 3 * k, (0.0, 0.0, 0.0)), (T.LONG, k - 6, 3 * k // 2, (0.5, 1.5, 0.5))) for clip, grad in zip((low, mid, 5000), grads))


@functools.lru_cache(maxsize=2)
def trim_case(case):
    k = case.k
    rng = np.random.default_rng(seed_of(case, "trim"))
    q, boosts = T.hairpin_queries(k, rng, True)
    q += T.edge_cases(k, rng) + T.tiling_queries(k, rng, False)   # (the reduced list: the LDS table's boundary does not move with k)
    # LONG under a clip above 1: the first k-mer has its reverse complement behind a loop and the second has not — the match of seed 0 survives
    rnd = lambda n: bytes(T.ACGT[rng.integers(0, 4, n)])
    u, loop = rnd(k), rnd(k + 15)
    q.append(("first-kmer-pair", u + loop[:-1] + loop[:1] + T.revcomp(u) + rnd(5)))        # (the letters around the pair are no complements)
    reads = [s.upper().replace(b"U", b"T").replace(b"N", b"A") for _, s in q if len(s) >= k] + boosts
    return T.TrimWorld(k, case.stranded, case.hashes, reads, q, trim_settings(k))


def outcome_counts(records):
    return sorted(collections.Counter(records).items())
