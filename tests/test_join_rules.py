"""GraphUtils.join (R/util/GraphUtils.java:892-1147) restated line by line in Python over a graph that answers three questions — counts(seq)
(getKmers' counts), neighbors(kmer, direction) (the counts of the four successors / predecessors in the order A C G T) and
lookup_read_pair(left_kmer, right_kmer) — with extendRightSE / extendLeftSE taken from tests/test_extend_step_rules.py.  Float arithmetic goes
through numpy.float32.  Hand-worked cases run on dict-backed toy graphs; then the worlds of tests/test_gpu_join.py are built on the CPU oracle
alone and every `why` and every way a walk can end is shown to be reached.  No device is needed here.

What the restatement returns is what rb_join_rec and out_seq hold: (outcome, why, l_end, r_end, l_added, r_added, l_forks, r_forks, index,
out_len), the two final thresholds and the string the returned k-mer list spells.  Reads are read as everywhere in the library: lower case as
upper case, U as T; a pair the reference cannot be asked about (a read shorter than k: it throws in get(0); a letter outside ACGTU) is
NOT_JUDGED."""
import os

import numpy as np
import pytest

import test_extend_step_rules as R
from test_extend_step_rules import F32, ACGT, extend_step, neighbor, is_acgtu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, JOINED, NOT_JUDGED = range(3)
REACHED_RIGHT, INSIDE_RIGHT, REACHED_LEFT, PATHS_MEET, RIGHT_LOOP, EXHAUSTED, SHORT, INVALID_LETTER = range(8)
NOT_RUN, NO_NEIGHBOR, LOOP, STEP_NONE, EXT_HOMOPOLYMER, BOUND, RETURNED = range(7)
NORM = bytes.maketrans(b"acgtuU", b"ACGTTT")


class Joined:
    def __init__(self, outcome, why, l_end=NOT_RUN, r_end=NOT_RUN, l_added=0, r_added=0, l_forks=0, r_forks=0, index=-1, text=b"", l_thr=0.0, r_thr=0.0):
        self.outcome, self.why, self.l_end, self.r_end, self.l_added, self.r_added = outcome, why, l_end, r_end, l_added, r_added
        self.l_forks, self.r_forks, self.index, self.text, self.l_thr, self.r_thr = l_forks, r_forks, index, text, F32(l_thr), F32(r_thr)

    def record(self):
        return (self.outcome, self.why, self.l_end, self.r_end, self.l_added, self.r_added, self.l_forks, self.r_forks, self.index, len(self.text))

    def __repr__(self):
        return "Joined%r thr=(%r, %r) %r" % (self.record(), float(self.l_thr), float(self.r_thr), self.text)


def is_homopolymer(kmer):
    return all(c == kmer[0] for c in kmer)


def spell(kmers):
    return kmers[0] + b"".join(km[-1:] for km in kmers[1:])


def neighbors_at_least(g, kmer, direction, min_cov):
    """Kmer.getSuccessors / getPredecessors(k, numHash, graph, minKmerCov), R/graph/Kmer.java:232-255 -> [(k-mer, count)] in the order A C G T"""
    c4 = g.neighbors(kmer, direction)
    return [(neighbor(kmer, b, direction), F32(c4[b])) for b in range(4) if F32(c4[b]) >= F32(min_cov)]


def join(g, left, right, bound, grad, max_tip, min_cov, d, k, same=None, step=extend_step, trace=None):
    """:892-1147.  same(a, b): Kmer.equals — the bases unless a test passes another relation to show what it would change; every HashSet and
    indexOf of the reference goes through it."""
    if len(left) < k or len(right) < k:
        return Joined(NOT_JUDGED, SHORT)
    if not is_acgtu(left) or not is_acgtu(right):
        return Joined(NOT_JUDGED, INVALID_LETTER)
    left, right = left.translate(NORM), right.translate(NORM)
    if same is None:
        contains = lambda kms, x: x in kms                     # (a list scan, as the device's sweep; the lists are short)
        first_index = lambda kms, x: kms.index(x)
        last_index = lambda kms, x: len(kms) - 1 - kms[::-1].index(x)
        same = lambda a, b: a == b
    else:
        contains = lambda kms, x: any(same(y, x) for y in kms)
        first_index = lambda kms, x: next(i for i, y in enumerate(kms) if same(y, x))
        last_index = lambda kms, x: next(i for i in range(len(kms) - 1, -1, -1) if same(kms[i], x))
    G, M = F32(grad), F32(min_cov)
    kmers_of = lambda s: [s[i:i + k] for i in range(len(s) - k + 1)]
    left_kmers, right_kmers = kmers_of(left), kmers_of(right)
    lc, rc = [F32(c) for c in g.counts(left)], [F32(c) for c in g.counts(right)]
    out = Joined(NONE, EXHAUSTED)

    def returned(why, kmers, index=-1):
        out.outcome, out.why, out.index, out.text = JOINED, why, index, spell(kmers)
        return out

    # ---- the left walk :912-1030 ----
    thr = max(M, F32(min(lc) * G))
    path, pc = list(left_kmers), list(lc)
    max_size = bound + len(path)
    out.l_end = BOUND

    def meets_right(x):
        """:946-967 / :987-1008 -> the list to return, or None"""
        if contains(right_kmers, x):
            if same(x, right_kmers[0]):
                return returned(REACHED_RIGHT, path + right_kmers)
            j = first_index(right_kmers, x)
            path_cov, dangling = min(pc[max(0, len(path) - j):]), min(rc[:j])
            if dangling < path_cov:
                return returned(INSIDE_RIGHT, path + right_kmers[j:], j)
        return None

    def left_done(end):
        out.l_end, out.l_added, out.l_thr = end, len(path) - len(left_kmers), thr

    while len(path) < max_size:
        nb = neighbors_at_least(g, path[-1], 0, M)
        if not nb:
            out.l_end = NO_NEIGHBOR
            break
        best = None
        if len(nb) == 1:
            best = nb[0]
        else:
            nb = [x for x in nb if not x[1] < thr]
            if len(nb) == 1:
                best = nb[0]
        if best is not None:
            thr = max(M, min(thr, F32(best[1] * G)))
            if meets_right(best[0]) is not None:
                left_done(RETURNED)
                return out
            if is_homopolymer(best[0]) or contains(path, best[0]):
                out.l_end = LOOP
                break
            path.append(best[0]); pc.append(best[1])
        else:
            out.l_forks += 1
            e = step(g, spell(path[-d:]), 0, M, d, k).ext
            if not e:
                out.l_end = STEP_NONE
                break
            at_loop = False
            for cur, cnt, _ in e:
                if meets_right(cur) is not None:
                    left_done(RETURNED)
                    return out
                if is_homopolymer(cur):
                    at_loop = True
                    break
                path.append(cur); pc.append(F32(cnt))
                c = F32(G * F32(cnt))
                if c < thr:
                    thr = max(c, M)
            if at_loop:
                out.l_end = EXT_HOMOPOLYMER
                break
    left_done(out.l_end)

    # ---- the right walk :1032-1144 ----
    last_left = left_kmers[-1]
    thr = max(M, F32(min(rc) * G))
    rpath = right_kmers[::-1]
    max_size = bound + len(rpath)
    out.r_end = BOUND

    def right_done(end):
        out.r_end, out.r_added, out.r_thr = end, len(rpath) - len(right_kmers), thr

    def paths_meet(x):
        i = last_index(path, x)                                # :1079-1086 / :1114-1121: leftPath is cut behind the LAST equal k-mer
        if trace is not None:
            trace["first_index"] = first_index(path, x)
        return returned(PATHS_MEET, path[:i + 1] + rpath[::-1], i)

    while len(rpath) < max_size:
        nb = neighbors_at_least(g, rpath[-1], 1, M)
        if not nb:
            out.r_end = NO_NEIGHBOR
            break
        best = None
        if len(nb) == 1:
            best = nb[0]
        else:
            nb = [x for x in nb if not x[1] < thr]
            if len(nb) == 1:
                best = nb[0]
        if best is not None:
            thr = max(M, min(thr, F32(best[1] * G)))
            if contains(path, best[0]):
                if same(best[0], last_left):
                    returned(REACHED_LEFT, left_kmers + rpath[::-1])
                else:
                    paths_meet(best[0])
                right_done(RETURNED)
                return out
            if is_homopolymer(best[0]) or contains(rpath, best[0]):
                right_done(LOOP)
                out.why = RIGHT_LOOP
                return out
            rpath.append(best[0])
        else:
            out.r_forks += 1
            e = step(g, spell(rpath[-d:][::-1]), 1, M, d, k).ext
            if not e:
                out.r_end = STEP_NONE
                break
            for cur, cnt, _ in e:
                if contains(path, cur):
                    paths_meet(cur)
                    right_done(RETURNED)
                    return out
                if is_homopolymer(cur):
                    right_done(EXT_HOMOPOLYMER)
                    out.why = RIGHT_LOOP
                    return out
                rpath.append(cur)
                c = F32(G * F32(cnt))
                if c < thr:
                    thr = max(c, M)
    right_done(out.r_end)
    return out


# ---- hand-worked cases on toy graphs (k = 6, d = 3; X has distinct 5-mers, so inside X every 6-mer has one successor and one predecessor) ----
X = b"ACGATCTTGGCAGTACCGTTAGGATCCA"
K, D = 6, 3
Toy = R.Toy


def toy(reads, mult=None, k=K, d=D):
    return Toy(k, reads, mult).build(d)


def run(g, left, right, bound, grad=0.5, min_cov=1.0, k=K, d=D, **kw):
    return join(g, left, right, bound, grad, 1, min_cov, d, k, **kw)


def test_a_straight_gap_is_closed_by_the_left_walk():
    g = toy([X])
    # left = X[0:9] (k-mers 0..3), right = X[15:24] (k-mers 15..18): the walk adds k-mers 4..14 (11) and then meets right's first k-mer
    r = run(g, X[:9], X[15:24], 20)
    assert r.record() == (JOINED, REACHED_RIGHT, RETURNED, NOT_RUN, 11, 0, 0, 0, -1, 24) and r.text == X[:24]
    assert r.l_thr == F32(1.0) and r.r_thr == F32(0.0)
    # bound 12 is the smallest that lets the left walk see k-mer 15: sizes 4 .. 15 are admitted at the top of the loop
    assert run(g, X[:9], X[15:24], 12).why == REACHED_RIGHT
    # adjacent reads: the first neighbour is right's first k-mer
    r = run(g, X[:9], X[4:13], 1)
    assert r.record() == (JOINED, REACHED_RIGHT, RETURNED, NOT_RUN, 0, 0, 0, 0, -1, 13) and r.text == X[:13]
    # bound 0: neither loop runs
    assert run(g, X[:9], X[15:24], 0).record() == (NONE, EXHAUSTED, BOUND, BOUND, 0, 0, 0, 0, -1, 0)
    # bound 5: the left walk adds 4 .. 8, the right walk 14 .. 10: they do not meet
    assert run(g, X[:9], X[15:24], 5).record() == (NONE, EXHAUSTED, BOUND, BOUND, 5, 5, 0, 0, -1, 0)


def test_paths_meet_where_the_left_walk_stopped_at_its_bound():
    g = toy([X])
    # bound 11: the left walk adds k-mers 4 .. 14 and the loop ends (size 15 = 11 + 4).  The right walk's first predecessor, k-mer 14, is in
    # leftPath — the PATH, not the read — at index 14, and is not left's last k-mer: leftPath[0..14] + right
    r = run(g, X[:9], X[15:24], 11)
    assert r.record() == (JOINED, PATHS_MEET, BOUND, RETURNED, 11, 0, 0, 0, 14, 24) and r.text == X[:24]
    assert r.l_thr == F32(1.0) and r.r_thr == F32(1.0)


def test_paths_meet_with_truncation():
    # X and a tip that leaves it behind k-mer 14 with three times X's coverage: the left walk is led into the tip and the cut removes it again
    tip = X[:20] + b"TTTGCA"
    g = toy([X, tip], [1, 3])
    r = run(g, X[:9], X[18:27], 20, grad=0.5)
    # left walk: k-mers 4 .. 14 (count 4: threshold min(2, 4 * 0.5) = 2), then two successors: X's k-mer 15 (count 1 < 2: dropped) and the
    # tip's (count 3): best, threshold 1.5; the tip's six k-mers, then no neighbour.  17 added.
    # right walk from X's k-mer 18: 17, 16, 15 (single predecessors), then k-mer 14, in leftPath at index 14: leftPath[0..14] + 15 .. 21
    assert r.record() == (JOINED, PATHS_MEET, NO_NEIGHBOR, RETURNED, 17, 3, 0, 0, 14, 27) and r.text == X[:27]
    assert r.l_thr == F32(1.5) and r.r_thr == F32(1.0)


def test_the_right_walk_reaches_left():
    # an error in left's last base: its last k-mer is not in the graph and has no successor.  From right the predecessors lead back to
    # left's k-mer 2, which is in leftPath but is not its LAST k-mer: PATHS_MEET at index 2, the erroneous k-mer is cut off
    g = toy([X])
    assert X[8:9] != b"A"
    r = run(g, X[:8] + b"A", X[12:21], 20)
    assert r.record() == (JOINED, PATHS_MEET, NO_NEIGHBOR, RETURNED, 0, 9, 0, 0, 2, 21) and r.text == X[:21]
    # REACHED_LEFT needs a left walk that ends AT left's last k-mer although that k-mer has a successor: a fork the step cannot decide.  Three
    # reads, X[:14], X[9:] and X[9:14] + B: no read holds a k-mer of X[:14] together with one behind the fork, so no pair supports either branch
    B = b"CAATGAGC"
    g2 = toy([X[:14], X[9:], X[9:14] + B])
    r = run(g2, X[5:14], X[17:26], 20, grad=0.1)
    # left walk: successors X[9:15] and X[9:14] + C, both count 1 >= threshold 1: a fork, the step finds no support (STEP_NONE)
    # right walk from k-mer 17: 16 .. 9 (eight), then k-mer 8 = left's last k-mer: left + 9 .. 20
    assert r.record() == (JOINED, REACHED_LEFT, STEP_NONE, RETURNED, 0, 8, 1, 0, -1, 21) and r.text == X[5:26]


def test_inside_right_both_ways():
    g = toy([X], [5])
    # an error in right's second base: its k-mers 0, 1 are not in the graph (count 0), k-mer 2 = X's k-mer 14 is
    assert X[13:14] != b"A"
    right = X[12:13] + b"A" + X[14:24]
    r = run(g, X[:9], right, 20)
    # the left walk adds 4 .. 13 and finds k-mer 14 in right at index 2: danglingCov = 0 < pathCov = 5
    assert r.record() == (JOINED, INSIDE_RIGHT, RETURNED, NOT_RUN, 10, 0, 0, 0, 2, 24) and r.text == X[:24]
    assert r.l_thr == F32(2.5)
    # the other way: right's first k-mers are covered better than the path — it lies on a second transcript Z + X[14:] of coverage 20
    Z = b"GGTTCA"
    g2 = toy([X, Z + X[14:]], [1, 20])
    r = run(g2, X[:9], Z[4:] + X[14:24], 14, grad=0.01)
    # the left walk adds 4 .. 13, then meets right's k-mers 2, 3, 4, 5 in turn: danglingCov 20 >= pathCov 1 each time, so each is ADDED (it is
    # neither a homopolymer nor in leftPath), up to the bound: 14 added.  The right walk goes back along Z (4 k-mers) and finds no predecessor
    assert r.record() == (NONE, EXHAUSTED, BOUND, NO_NEIGHBOR, 14, 4, 0, 0, -1, 0)


def test_a_left_loop_is_followed_by_a_successful_right_walk():
    # a circle of eight k-mers: left = its k-mers 0 .. 4, right = one k-mer, TCATAC, which is the circle's k-mer 4 again
    unit = b"ACGGTCAT"
    g = toy([unit * 4])
    r = run(g, (unit * 2)[:10], b"TCATAC", 40)
    # left walk: 5, 6, 7, then k-mer 0 which leftPath holds: the loop BREAKS (no return).  The right walk's first predecessor is k-mer 3, in
    # leftPath at index 3: leftPath[0..3] + TCATAC
    assert r.record() == (JOINED, PATHS_MEET, LOOP, RETURNED, 3, 0, 0, 0, 3, 10) and r.text == (unit * 2)[:10]


def test_right_loop_returns_null():
    # left is off the graph; right lies in a circle: the right walk goes round it and meets a k-mer of rightPath — null, not a break
    unit = b"ACGGTCAT"
    g = toy([unit * 4])
    r = run(g, b"TTTTGTTTT", (unit * 2)[:9], 40)
    assert r.record() == (NONE, RIGHT_LOOP, NO_NEIGHBOR, LOOP, 0, 4, 0, 0, -1, 0) and r.r_thr == F32(1.5)
    # a homopolymer predecessor does the same: AAAACG, AAAAAC are added, AAAAAA is not
    g2 = toy([b"AAAAAAAAACGTCAGT"])
    assert run(g2, b"TTTTGTTTT", b"AAACGTCAGT", 40).record() == (NONE, RIGHT_LOOP, NO_NEIGHBOR, LOOP, 0, 2, 0, 0, -1, 0)


T_P = b"ACGTTGCAAGC"
T_A2 = T_P + b"TTAGGATCCATTGACC"
T_B2 = T_P + b"GGCTAATCGTACCGTA"


def test_a_fork_is_crossed_by_read_pairs_or_filtered_by_the_threshold():
    # test_extend_step_rules' fork (k = 4, d = 3): behind the prefix, branch A has count 1 and branch B count 3
    k, d = 4, 3
    g = Toy(k, [T_A2, T_B2], [1, 3]).build(d)
    # gradient 0.1: the threshold stays 1 and does not choose — the step does, by pairs and coverage, for B
    r = join(g, T_P[:8], T_B2[16:24], 30, 0.1, 1, 1.0, d, k)
    assert r.record() == (JOINED, REACHED_RIGHT, RETURNED, NOT_RUN, 11, 0, 3, 0, -1, 24) and r.text == T_B2[:24] and r.l_thr == F32(1.0)
    # gradient 0.5: threshold 4 * 0.5 = 2 drops branch A's k-mer (count 1) and leaves ONE neighbour: no fork is seen at all
    r = join(g, T_P[:8], T_B2[16:24], 30, 0.5, 1, 1.0, d, k)
    assert r.record() == (JOINED, REACHED_RIGHT, RETURNED, NOT_RUN, 11, 0, 0, 0, -1, 24) and r.text == T_B2[:24] and r.l_thr == F32(1.5)
    # ... and the pair on branch A is not joined from the left with that gradient; the right walk comes back along A and meets the left path
    r = join(g, T_P[:8], T_A2[16:24], 30, 0.5, 1, 1.0, d, k)
    assert (r.outcome, r.why, r.l_end, r.r_end) == (JOINED, PATHS_MEET, LOOP, RETURNED) and r.text == T_A2[:24]


def test_an_extension_may_overshoot_the_bound():
    k, d = 4, 3
    g = Toy(k, [T_A2, T_B2], [1, 3]).build(d)
    # left ends exactly at the fork, bound 1: the loop runs once and the step adds three k-mers
    r = join(g, T_P, b"CCCCCCCC", 1, 0.1, 1, 1.0, d, k)
    assert r.record() == (NONE, EXHAUSTED, BOUND, NO_NEIGHBOR, 3, 0, 1, 0, -1, 0)


def test_a_duplicate_enters_left_path_through_an_extension():
    """The step's k-mers are added without a set test (:1015).  A circle of four k-mers (ACGG CGGA GGAC GACG) entered from a tail, with an exit
    behind GGAC -> GACG | GACA: at d = 5 a step's walk goes once round the circle, so every step adds k-mers leftPath already holds.  The
    right walk comes back from the exit and meets GGAC, which leftPath holds at 6, 10 and 14: the cut is made behind the LAST (:1079-1086)."""
    k, d = 4, 5
    g = Toy(k, [b"TTGCA" + b"ACGG" * 6, b"ACGG" * 5 + b"A" + b"TTCAA"], [1, 1]).build(d)
    trace = {}
    r = join(g, b"TTGCAA", b"ATTCAA", 12, 0.1, 1, 1.0, d, k, trace=trace)
    assert r.record() == (JOINED, PATHS_MEET, BOUND, RETURNED, 12, 2, 2, 0, 14, 23) and trace == {"first_index": 6}
    assert r.text == b"TTGCAACGGACGGACGGATTCAA"              # a cut behind the first would spell TTGCAACGGATTCAA


# ---- the worlds of the device test, on the CPU oracle ----
class JoinWorld:
    """The transcripts and reads of test_extend_step_rules.World (isoform forks at 1:1, 1:3 and 1:10, second forks, junctions, tandem repeats,
    homopolymer runs; every transcript also reversed), and read pairs cut from the transcripts: gaps of 1 .. bound + 5 k-mers, pairs across the
    forks on either branch, a substitution near the start of the right read or the end of the left read, pairs inside the tandem repeats and
    the homopolymers, pairs in the wrong order, a read with an N, a lower-case read, a short read."""
    BOUND, GRAD, MIN_COV, TIP = 20, 0.5, 1.0, 10
    # the lengths that do not follow from k by themselves, as the worlds at k = 25 have them (tests/pair_worlds.py derives them from k): the
    # shortest transcript that has a fork or junction in its middle; the homopolymer runs a transcript is recognised by (A, C), how many of
    # the run's letters end the left read of the first pair, where its right read and the left read of the second pair begin in the run
    PAIR_LENGTHS = dict(fork_tx=260, a_run=40, c_run=100, run_left=5, run_right=55, run_second=20)

    def __init__(self, k, stranded, seed, d=30, n_pairs=700, read_len=None, world_read_len=None, pair_lengths=None, extra_pairs=(), **kw):
        if world_read_len is not None:                                    # (read_len is the length of the pairs' reads, not of the world's)
            kw["read_len"] = world_read_len
        pl = dict(self.PAIR_LENGTHS, **(pair_lengths or {}))
        self.w = w = R.World(k, stranded, seed, d=d, **kw)
        self.k, self.d, self.stranded, self.og, self.o, self.sizes, self.hashes, self.packed = k, d, stranded, w.og, w.o, w.sizes, w.hashes, w.packed
        rng = np.random.default_rng(seed + 1)
        L = read_len or k + 15
        pairs = []
        tx = [t for t, _ in w.tx if len(t) >= 3 * L]
        tx = tx + [t[::-1] for t in tx]
        sub = lambda s, p: R.put(s, p, "ACGT"[("ACGT".index(chr(s[p])) + 1 + int(rng.integers(0, 3))) % 4])
        while len(pairs) < n_pairs:
            t = tx[int(rng.integers(0, len(tx)))]
            kind = int(rng.integers(0, 10))
            gap = int(rng.integers(1, self.BOUND + 6))                    # missing k-mers between the reads
            a = int(rng.integers(0, max(1, len(t) - 2 * L - gap)))
            if kind < 2 and len(t) > pl["fork_tx"]:                       # across the fork / junction in the middle of the transcript
                a = max(0, min(len(t) - 2 * L - gap, len(t) // 2 - L - int(rng.integers(0, gap + 1))))
            b = a + L - k + 1 + gap
            left, right = t[a:a + L], t[b:b + L]
            if len(right) < k:
                continue
            if kind == 2:
                right = sub(right, int(rng.integers(0, 6)))               # its first k-mers are off the path
            elif kind == 3:
                left = sub(left, len(left) - 1 - int(rng.integers(0, 6)))
            elif kind == 4:
                left, right = right, left                                  # the wrong order
            elif kind == 5:
                right = sub(right, int(rng.integers(k, len(right))))
            pairs.append((left, right))
        a_run, c_run, r_l, r_r, r_s = b"A" * pl["a_run"], b"C" * pl["c_run"], pl["run_left"], pl["run_right"], pl["run_second"]
        for t in [t for t, _ in w.tx if a_run in t or c_run in t]:                # homopolymer runs
            p = t.find(a_run) if a_run in t else 10
            pairs += [(t[max(0, p - L + r_l):p + r_l][:L], t[p + r_r:p + r_r + L] if len(t) > p + r_r + k else t[-L:]), (t[p + r_s:p + r_s + L], t[-L:])]
        for kind, s, direction in w.queries:
            if kind in ("tandem", "circle") and direction == 0 and len(s) >= k + 4:
                pairs += [(s[:k + 4], s[-(k + 4):]), (s[-(k + 4):], s[:k + 4])]
        t0 = w.tx[0][0]
        pairs += [(R.put(t0[:L], 7, "N"), t0[L + 5:2 * L + 5]), (t0[:L].lower(), t0[L + 5:2 * L + 5].replace(b"T", b"U")), (t0[:k - 1], t0[L:2 * L]), (t0[:L], b""),
                  (t0[:L], t0[L + 3:L + 3 + k])]
        self.pairs = pairs + list(extra_pairs)
        self._want = None

    def want(self):
        if self._want is None:
            self._want = [join(self.o, l, r, self.BOUND, self.GRAD, self.TIP, self.MIN_COV, self.d, self.k) for l, r in self.pairs]
        return self._want

    def assert_every_branch_is_reached(self):
        want = self.want()
        whys = {r.why for r in want}
        assert whys == set(range(8)), sorted(set(range(8)) - whys)
        l_ends, r_ends = {r.l_end for r in want}, {r.r_end for r in want}
        assert l_ends == set(range(7)), sorted(set(range(7)) - l_ends)
        assert r_ends == set(range(7)), sorted(set(range(7)) - r_ends)
        assert {r.outcome for r in want} == {NONE, JOINED, NOT_JUDGED}
        assert sum(r.outcome == NOT_JUDGED for r in want) * 50 <= len(want)           # at most 2 %
        assert any(r.l_forks for r in want) and any(r.r_forks for r in want)
        assert any(r.l_added > self.BOUND for r in want) and any(r.r_added > self.BOUND for r in want)        # a step overshot the bound


WORLDS = {}


def world(k, stranded):
    if (k, stranded) not in WORLDS:
        WORLDS[(k, stranded)] = JoinWorld(k, stranded, seed=700 + stranded)
    return WORLDS[(k, stranded)]


@pytest.mark.parametrize("stranded", [False, True])
def test_worlds_reach_every_branch_on_the_oracle(stranded):
    world(25, stranded).assert_every_branch_is_reached()


# ---- two k-mers that hash alike and differ (ntHash at k = 64: a rotation by 64 is none; tests/traversal_worlds.py) ----
class TwinWorld:
    """the graph of the single read (AC) x 50 at k = 64: (AC)^32, (CA)^32, (GT)^32 and (TG)^32 all hash to f = 0, r = 0"""
    D, BOUND, GRAD = 4, 10, 0.5
    PAIRS = [(b"AC" * 32, b"GT" * 32), (b"AC" * 32, b"TG" * 32), (b"AC" * 33, b"GT" * 32), (b"CA" * 32 + b"C", b"TG" * 32)]

    def __init__(self, stranded):
        from oracle import rbo
        self.k, self.d, self.stranded, self.hashes = 64, self.D, stranded, (2, 2, 2)
        self.sizes = (400_009, 400_009, 400_031)
        self.og = rbo.Graph(*self.sizes, *self.hashes, self.k, stranded, True, 5)
        self.og.set_read_pair_distance(self.d)
        reads = [b"AC" * 50]
        self.packed = rbo.pack_reads(reads, [b"I" * len(s) for s in reads])
        self.og.add_reads(*self.packed, 3, rbo.STORE_READ_PAIRS)
        self.o = R.OracleSide(self.og)

    def forward_hash(self, kmer):
        return int(self.og.get_kmers(kmer)[0][0])

    def want(self, same=None):
        return [join(self.o, l, r, self.BOUND, self.GRAD, 1, 1.0, self.d, self.k, same=same) for l, r in self.PAIRS]


@pytest.mark.parametrize("stranded", [False, True])
def test_membership_by_hash_alone_would_give_another_record(stranded):
    w = TwinWorld(stranded)
    assert len({w.forward_hash(km) for km in (b"AC" * 32, b"CA" * 32, b"GT" * 32, b"TG" * 32)}) == 1
    by_bases = w.want()
    by_hash = w.want(same=lambda a, b: w.forward_hash(a) == w.forward_hash(b))
    # Kmer.equals: the left walk adds (CA)^32 and stops at (AC)^32 again (LOOP), the right walk ends in its own loop: null.  By hash alone the
    # left walk's first neighbour "is" right's first k-mer and the pair is joined
    for a, b in zip(by_bases, by_hash):
        assert (a.outcome, a.why, a.l_end, a.r_end) == (NONE, RIGHT_LOOP, LOOP, LOOP), a
        assert (b.outcome, b.why) == (JOINED, REACHED_RIGHT) and a.record() != b.record(), b


# ---- the package's overlapAndConnect without a device: its graph is a stand-in whose two calls are the restatements ----
class ConnectStandIn:
    """what graphutils.overlapAndConnect asks of a graph — overlapPairs, joinPairs and their constants — answered by the restated overlap
    (tests/test_overlap_rules.py) and the restated join over one graph"""
    OVL_NONE, OVL_RESCUE = 0, 5
    JOIN_NONE, JOIN_JOINED, JOIN_NOT_JUDGED = range(3)

    def __init__(self, g, k, d):
        self.g, self.k, self.d, self.join_calls, self.joined = g, k, d, 0, []

    def overlapPairs(self, lefts, rights, minOverlap, minKmerCov=1.0):
        import test_overlap_rules as O
        out = []
        for l, r in zip(lefts, rights):
            (outcome, _, flags, _, _, _, _), text = O.expected(l, r, self.k, minOverlap, minKmerCov, self.g)
            out.append((text if outcome != O.NONE else None, outcome, bool(flags)))
        return out

    def joinPairs(self, lefts, rights, bound, maxCovGradient, maxTipLen, minKmerCov=1.0):
        self.join_calls += 1
        self.joined += list(zip(lefts, rights))
        res = [join(self.g, l, r, bound, maxCovGradient, maxTipLen, minKmerCov, self.d, self.k) for l, r in zip(lefts, rights)]
        return [(r.text if r.outcome == JOINED else None, r.outcome, r.why) for r in res]


def restated_overlap_and_connect(g, left, right, bound, min_overlap, grad, max_tip, min_cov, d, k):
    """:5065-5090: overlap, and join where it returns null"""
    import test_overlap_rules as O
    (outcome, _, _, _, _, _, _), text = O.expected(left, right, k, min_overlap, min_cov, g)
    if outcome == O.RESCUE:
        return text, "rescue"
    if outcome != O.NONE:
        return text, "overlap"
    r = join(g, left, right, bound, grad, max_tip, min_cov, d, k)
    return (r.text, "join") if r.outcome == JOINED else (None, "not_judged" if r.outcome == NOT_JUDGED else "none")


def connect_pairs(w, n=160):
    """pairs of a world for overlapAndConnect: the gapped pairs, and pairs that overlap by 0 .. 2 k letters"""
    rng = np.random.default_rng(3)
    pairs = list(w.pairs[:n // 2]) + list(w.pairs[-5:])
    t = w.w.tx[0][0]
    for _ in range(n // 2):
        a, L, o = int(rng.integers(0, 150)), w.k + 15, int(rng.integers(0, 2 * w.k))
        pairs.append((t[a:a + L], t[a + L - o:a + 2 * L - o]))
    return pairs


@pytest.mark.parametrize("stranded", [False, True])
def test_the_package_s_overlap_and_connect_equals_restated_overlap_then_join(stranded):
    from rnabloom import graphutils
    w = world(25, stranded)
    pairs = connect_pairs(w)
    dev = ConnectStandIn(w.o, w.k, w.d)
    got = graphutils.overlapAndConnect(dev, [l for l, _ in pairs], [r for _, r in pairs], w.BOUND, 10, w.GRAD, w.TIP, w.MIN_COV)
    want = [restated_overlap_and_connect(w.o, l, r, w.BOUND, 10, w.GRAD, w.TIP, w.MIN_COV, w.d, w.k) for l, r in pairs]
    assert got == want
    assert dev.join_calls == 1 and 0 < len(dev.joined) < len(pairs)                   # ONE join call, over the pairs overlap returned null for
    assert {how for _, how in want} >= {"overlap", "join", "none", "not_judged"}


def test_header_python_java_and_jni_sides_exist():
    import re
    hdr = open(os.path.join(ROOT, "include", "rb_capi.h")).read()
    assert re.search(r"int rb_graph_join_pairs\(rb_graph \*g, const char \*lseq, const int64_t \*loffsets, const char \*rseq, const int64_t \*roffsets, int64_t n, int bound,", hdr)
    assert "lookahead, maxIndelLen and minPercentIdentity" in hdr and "RB_JOIN_MAX_BOUND" in hdr
    from rnabloom import _native as N
    from rnabloom.graph import BloomFilterDeBruijnGraph as G
    assert any(s[0] == "rb_graph_join_pairs" for s in N.SYMBOLS) and G.JOIN_DTYPE.itemsize == 48
    assert len(G.JOIN_WHYS) == 8 and len(G.JOIN_ENDS) == 7 and (G.JOIN_NONE, G.JOIN_JOINED, G.JOIN_NOT_JUDGED) == (NONE, JOINED, NOT_JUDGED)
    java = open(os.path.join(ROOT, "java", "rnabloom", "graph", "BloomFilterDeBruijnGraph.java")).read()
    assert "public String[] joinPairs(String[] lefts, String[] rights, int bound, float maxCovGradient, int maxTipLen, float minKmerCov, int[] records)" in java
    assert "FN(joinPairs)" in open(os.path.join(ROOT, "jni", "rb_jni.c")).read()
