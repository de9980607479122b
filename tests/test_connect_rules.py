"""GraphUtils.connect over a segment list (R/util/GraphUtils.java:4836-4872), the two-string connect (:4874-4896) and the six-argument
getMaxCoveragePath (:1591-1675) restated line by line over a graph that answers neighbors(kmer, direction): the CPU twin of
rb_graph_connect_segments (tests/test_gpu_connect.py compares the device with it).  Hand-worked cases on dict-backed toy graphs cover every
`how` and every walk end; ConnectWorld builds the worlds of the device test on the CPU oracle; rnabloom.io.filterFastq / filterFasta are checked
against hand-written cases."""
import numpy as np
import pytest

import test_extend_step_rules as R
from test_extend_step_rules import F32, ACGT, neighbor, is_acgtu
from rnabloom import graphutils

EMPTY, SINGLE, CHAINED, NOT_JUDGED = range(4)
WHY_NONE, EVEN_COUNT, SHORT, INVALID_LETTER = range(4)
HOW_NOT_RUN, LEFT_ARRIVED, RIGHT_ARRIVED, PATHS_MEET, MEET_LOW_COMPLEXITY, RIGHT_LOOP, EXHAUSTED = range(7)
NOT_RUN, NO_NEIGHBOR, LOOP, BOUND, ARRIVED, MET = range(6)
NORM = bytes.maketrans(b"acgtuU", b"ACGTTT")


class Gap:
    """rb_connect_gap_rec and the path"""

    def __init__(self):
        self.connected, self.how, self.l_end, self.r_end, self.l_added, self.r_added, self.index, self.path_len = 0, HOW_NOT_RUN, NOT_RUN, NOT_RUN, 0, 0, -1, 0

    def record(self):
        return (self.connected, self.how, self.l_end, self.r_end, self.l_added, self.r_added, self.index, self.path_len)

    def __repr__(self):
        return "Gap%r" % (self.record(),)


def max_cov_neighbor(g, kmer, direction, min_cov):
    """Kmer.getMaxCovSuccessor / getMaxCovPredecessor (R/graph/Kmer.java:301-355)"""
    best_count, best = F32(-1), None
    for b, c in enumerate(g.neighbors(kmer, direction)):
        if c >= F32(min_cov) and c > best_count:
            best_count, best = c, neighbor(kmer, b, direction)
    return best


def get_max_coverage_path(g, left, right, bound, lookahead, min_cov, rec, same=None):
    """:1591-1675.  same(a, b): Kmer.equals (the k bases); a test passes equality by hash alone to show what that would change"""
    same = same or (lambda a, b: a == b)
    contains = lambda kmers, x: any(same(x, y) for y in kmers)
    left_path = []
    best = left
    rec.l_end = BOUND
    for depth in range(bound):
        best = max_cov_neighbor(g, best, 0, min_cov)
        if best is None:
            rec.l_end = NO_NEIGHBOR
            break
        if same(best, right):
            rec.l_end, rec.how, rec.l_added = ARRIVED, LEFT_ARRIVED, len(left_path)
            return left_path
        if contains(left_path, best):
            rec.l_end = LOOP
            break
        left_path.append(best)
    rec.l_added = len(left_path)
    right_path = []                                             # addFirst: kept in walking order here, reversed where it is returned
    best = right
    rec.r_end = BOUND
    for depth in range(bound):
        best = max_cov_neighbor(g, best, 1, min_cov)
        if best is None:
            rec.r_end = NO_NEIGHBOR
            break
        if same(best, left):
            rec.r_end, rec.how, rec.r_added = ARRIVED, RIGHT_ARRIVED, len(right_path)
            return right_path[::-1]
        if contains(right_path, best):
            rec.r_end, rec.how, rec.r_added = LOOP, RIGHT_LOOP, len(right_path)
            return None
        if contains(left_path, best):
            rec.r_end, rec.r_added = MET, len(right_path)
            rec.index = max(i for i, x in enumerate(left_path) if same(best, x))           # the descending iterator stops at the LAST one
            if graphutils.isLowComplexityShort(best):
                rec.how = MEET_LOW_COMPLEXITY
                return None
            rec.how = PATHS_MEET
            return left_path[:rec.index] + [best] + right_path[::-1]
        right_path.append(best)
    rec.r_added, rec.how = len(right_path), EXHAUSTED
    return None


def connect2(g, left, right, bound, lookahead, k, rec, same=None):
    """:4874-4896"""
    path = get_max_coverage_path(g, left[-k:], right[:k], bound, lookahead, 1, rec, same)
    rec.path_len = 0 if path is None else len(path)
    if path is None or not path or len(path) > bound:
        return b""
    rec.connected = 1
    left_wing = left[:1] if len(left) == k else left[:len(left) - k + 1]
    return left_wing + path[0] + bytes(x[-1] for x in path[1:]) + right[k - 1:]


class Connected:
    def __init__(self, outcome, why, segments):
        self.outcome, self.why, self.n_gaps, self.connected, self.first_seg, self.last_seg, self.text, self.gaps = outcome, why, len(segments) // 2, 0, -1, -1, b"", []
        self.gaps = [Gap() for _ in range(self.n_gaps)]

    def record(self):
        return (self.outcome, self.why, self.n_gaps, self.connected, self.first_seg, self.last_seg, len(self.text), 0)

    def __repr__(self):
        return "Connected%r %r %r" % (self.record(), self.text, self.gaps)


def connect(g, segments, lookahead, k, same=None):
    """:4836-4872, with what the reference cannot be asked about named first"""
    n = len(segments)
    if n == 0:
        return Connected(EMPTY, WHY_NONE, segments)
    if n == 1:
        out = Connected(SINGLE, WHY_NONE, segments)
        out.first_seg = out.last_seg = 0
        out.text = segments[0]
        return out
    if n % 2 == 0:
        return Connected(NOT_JUDGED, EVEN_COUNT, segments)                                  # get(i + 1) throws
    if any(len(s) < k for s in segments[::2]):
        return Connected(NOT_JUDGED, SHORT, segments)
    if not all(is_acgtu(s) for s in segments[::2]):
        return Connected(NOT_JUDGED, INVALID_LETTER, segments)
    out = Connected(CHAINED, WHY_NONE, segments)
    seg = [s.translate(NORM) for s in segments]
    last, last_first = seg[0], 0
    longest, out.first_seg, out.last_seg = last, 0, 0
    for i in range(1, n, 2):
        current = seg[i + 1]
        rec = out.gaps[i // 2]
        connected = connect2(g, last, current, len(seg[i]) + k, lookahead, k, rec, same)
        if len(connected) > 0:
            last = connected
            out.connected += 1
            if len(connected) > len(longest):
                longest, out.first_seg, out.last_seg = connected, last_first, i + 1
        else:
            last, last_first = current, i + 1
            if len(current) > len(longest):
                longest, out.first_seg, out.last_seg = current, i + 1, i + 1
    out.text = longest
    return out


# ---- hand-worked cases on toy graphs (k = 6; X has distinct 5-mers, so inside X every 6-mer has one successor and one predecessor) ----
X = b"ACGATCTTGGCAGTACCGTTAGGATCCA"
K = 6


def toy(reads, mult=None, k=K):
    return R.Toy(k, reads, mult).build(3)


def gap(g, left, right, bound, k=K, **kw):
    rec = Gap()
    return connect2(g, left, right, bound, 0, k, rec, **kw), rec


def test_a_straight_gap_and_the_bound():
    g = toy([X])
    # left's last k-mer is k-mer 3 of X, right's first k-mer 15: the path is k-mers 4 .. 14, 11 of them.  With bound 12 the left walk sees k-mer 15
    text, r = gap(g, X[:9], X[15:24], 12)
    assert text == X[:24] and r.record() == (1, LEFT_ARRIVED, ARRIVED, NOT_RUN, 11, 0, -1, 11)
    # bound 11: the left walk adds its 11 k-mers and stops; the right walk's first predecessor, k-mer 14, is entry 10 of the left path: a path of
    # exactly bound k-mers connects
    text, r = gap(g, X[:9], X[15:24], 11)
    assert text == X[:24] and r.record() == (1, PATHS_MEET, BOUND, MET, 11, 0, 10, 11)
    # one k-mer more between them (4 .. 15) with the same bound: the right walk adds k-mer 15 and meets entry 10: 12 k-mers, not connected
    text, r = gap(g, X[:9], X[16:25], 11)
    assert text == b"" and r.record() == (0, PATHS_MEET, BOUND, MET, 11, 1, 10, 12)
    # far apart with a small bound: both walks run out (k-mers 1 .. 6 and 21 .. 16)
    text, r = gap(g, X[:6], X[22:], 6)
    assert text == b"" and r.record() == (0, EXHAUSTED, BOUND, BOUND, 6, 6, -1, 0)
    # bound 0: neither loop runs
    assert gap(g, X[:6], X[22:], 0)[1].record() == (0, EXHAUSTED, BOUND, BOUND, 0, 0, -1, 0)


def test_the_empty_path_and_the_overlapping_forms():
    g = toy([X])
    # right's first k-mer directly follows left's last: the left walk returns the empty path, and connect gives ""
    text, r = gap(g, X[:9], X[4:13], 8)
    assert text == b"" and r.record() == (0, LEFT_ARRIVED, ARRIVED, NOT_RUN, 0, 0, -1, 0)
    # paths of 1, k - 2 and k - 1 k-mers: right[k - 1:] lies over left's end and the string is X's all the same
    for n_path in (1, K - 2, K - 1, K):
        text, r = gap(g, X[:9], X[4 + n_path:14 + n_path], 8)
        assert text == X[:14 + n_path] and r.record() == (1, LEFT_ARRIVED, ARRIVED, NOT_RUN, n_path, 0, -1, n_path), n_path


P, A_S, B_ = X[:12], X[12:], b"TGTCAAGCGC"                      # a fork behind P: P + A_S is X (once), P + B_ three times


def fork():
    g = toy([P + A_S, P + B_], [1, 3])
    last = P[-K:]
    assert g.neighbors(last, 0) == [F32(0), F32(0), F32(1), F32(3)]                         # G goes on in X, T into the heavier branch
    return g


def test_the_right_walk_arrives_or_meets_the_left_path():
    g = fork()
    # left ends where P ends: the left walk follows the heavier branch to its end (5 + 5 k-mers: no neighbour), the right walk comes back through
    # X's k-mers 11 .. 7 to left's last k-mer, k-mer 6: the right path is returned
    text, r = gap(g, P, X[12:21], 20)
    assert text == X[:21] and r.record() == (1, RIGHT_ARRIVED, NO_NEIGHBOR, ARRIVED, 10, 5, -1, 5)
    # ... and when right's first k-mer is X's k-mer 7 its first predecessor is left's last k-mer: the EMPTY right path, ""
    text, r = gap(g, P, X[7:16], 20)
    assert text == b"" and r.record() == (0, RIGHT_ARRIVED, NO_NEIGHBOR, ARRIVED, 10, 0, -1, 0)
    # left ends three letters before P does: the left path holds k-mers 4, 5, 6 and the branch; the right walk meets entry 2 (k-mer 6)
    text, r = gap(g, P[:9], X[12:21], 20)
    assert text == X[:21] and r.record() == (1, PATHS_MEET, NO_NEIGHBOR, MET, 13, 5, 2, 8)
    # the same with a bound of 7: a path of 8 k-mers is not connected, and `how` still names the line
    text, r = gap(g, P[:9], X[12:21], 7)
    assert text == b"" and r.record() == (0, PATHS_MEET, BOUND, MET, 7, 5, 2, 8)


U7 = b"ACGATCT"                                                 # a circle of 7 k-mers: every 6-mer of U7 U7 U7 ... has one successor and one predecessor
Y = b"GGTTCAGTCCA"                                              # shares no 5-mer with X or the circle


def test_loops_and_dead_ends():
    g = toy([U7 * 4, Y])
    # left on the circle, right elsewhere with no predecessor.  The left walk adds the six other k-mers, then left's own k-mer — it is not in the set —
    # and ends at the k-mer it added first
    text, r = gap(g, (U7 * 2)[:9], Y, 12)
    assert text == b"" and r.record() == (0, EXHAUSTED, LOOP, NO_NEIGHBOR, 7, 0, -1, 0)
    # right on the circle, left at Y's end with no successor: the right walk returns null where it meets its own path
    text, r = gap(g, Y, (U7 * 2)[:9], 12)
    assert text == b"" and r.record() == (0, RIGHT_LOOP, NO_NEIGHBOR, LOOP, 0, 7, -1, 0)
    # both dead ends
    g = toy([X, Y])
    text, r = gap(g, X, Y, 12)
    assert text == b"" and r.record() == (0, EXHAUSTED, NO_NEIGHBOR, NO_NEIGHBOR, 0, 0, -1, 0)


def test_a_meeting_in_a_low_complexity_kmer_is_null():
    w, z = b"GCTTGACC", b"CGTAGGCT"
    g = toy([w + b"A" * 10 + z])
    # the left walk from TTGACC takes an A six times, adds AAAAAA last (entry 5) and ends at it again; the right walk comes back from CGTAGG over
    # five k-mers and meets AAAAAA: isLowComplexityShort
    text, r = gap(g, w, z, 16)
    assert text == b"" and r.record() == (0, MEET_LOW_COMPLEXITY, LOOP, MET, 6, 5, 5, 0)
    assert graphutils.isLowComplexityShort(b"AAAAAA") and not graphutils.isLowComplexityShort(b"CTTGAC")


def lists(g, segments, k=K, **kw):
    return connect(g, segments, 0, k, **kw)


def test_list_sizes_and_reads_that_are_not_judged():
    g = toy([X])
    assert lists(g, []).record() == (EMPTY, WHY_NONE, 0, 0, -1, -1, 0, 0)
    for one in (X[:9], b"acgNN", b""):                                                      # one entry: untouched, whatever it holds
        r = lists(g, [one])
        assert r.record() == (SINGLE, WHY_NONE, 0, 0, 0, 0, len(one), 0) and r.text == one
    for even in ([X[:9], b"N"], [X[:9], b"N", X[12:21], b"NN"]):
        r = lists(g, even)
        assert r.record() == (NOT_JUDGED, EVEN_COUNT, len(even) // 2, 0, -1, -1, 0, 0) and all(x.how == HOW_NOT_RUN for x in r.gaps)
    assert lists(g, [X[:9], b"NN", X[12:17]]).record() == (NOT_JUDGED, SHORT, 1, 0, -1, -1, 0, 0)
    assert lists(g, [X[:5], b"NN", X[12:21]]).record() == (NOT_JUDGED, SHORT, 1, 0, -1, -1, 0, 0)
    assert lists(g, [X[:9], b"NN", b"ACGNTT"]).record() == (NOT_JUDGED, INVALID_LETTER, 1, 0, -1, -1, 0, 0)
    assert lists(g, [X[:5], b"NN", b"ACGNTT"]).why == SHORT                                  # in this order
    # lower case and U are read as everywhere, and come back as upper-case A C G T — also where nothing connects and the run is one segment
    r = lists(g, [X[:9].lower().replace(b"t", b"u"), b"NNN", X[12:21].replace(b"T", b"U")])
    assert r.record() == (CHAINED, WHY_NONE, 1, 1, 0, 2, 21, 0) and r.text == X[:21]
    r = lists(g, [X[:9].lower(), b"", Y])
    assert r.record() == (CHAINED, WHY_NONE, 1, 0, 2, 2, len(Y), 0) and r.text == Y


def test_the_longest_run_and_ties():
    g = toy([X, Y])
    # X's pieces connect (9 + 3 + 9 = 21 letters); Y cannot be reached: the run of X wins over Y (11)
    r = lists(g, [X[:9], b"NNN", X[12:21], b"NN", Y])
    assert r.record() == (CHAINED, WHY_NONE, 2, 1, 0, 2, 21, 0) and r.text == X[:21] and [x.connected for x in r.gaps] == [1, 0]
    # a later run that is longer wins
    r = lists(g, [Y, b"NN", X[:9], b"NNN", X[12:21]])
    assert (r.first_seg, r.last_seg, r.text) == (2, 4, X[:21])
    # equal lengths: the earlier run stays
    r = lists(g, [Y, b"N", X[:11]])
    assert (r.first_seg, r.last_seg, r.text, r.connected) == (0, 0, Y, 0)
    r = lists(g, [X[:11], b"N", Y])
    assert (r.first_seg, r.last_seg, r.text) == (0, 0, X[:11])
    # the bound is the placeholder's length + k: k-mers 4 .. 14 lie between, 11 of them, and a placeholder of 5 is the shortest that connects them
    assert lists(g, [X[:9], b"N" * 5, X[15:24]]).text == X[:24]
    # ... with 4 the left walk adds k-mers 4 .. 13, the right walk k-mer 14 and meets entry 9: 11 k-mers for a bound of 10
    assert lists(g, [X[:9], b"N" * 4, X[15:24]]).gaps[0].record() == (0, PATHS_MEET, BOUND, MET, 10, 1, 9, 11)
    # three segments in a row: the second gap starts from the connected string, whose last k-mer is the middle segment's
    r = lists(g, [X[:8], b"N", X[9:16], b"NN", X[18:]])
    assert r.record() == (CHAINED, WHY_NONE, 2, 2, 0, 4, len(X), 0) and r.text == X


def test_kmers_that_hash_alike_and_differ_are_told_apart_by_their_bases():
    """ntHash at k = 64: a rotation by 64 is none, (AC)^32 and (CA)^32 hash alike (tests/traversal_worlds.py).  With equality by hash the left
    walk from (AC)^32 'arrives' at (CA)^32's twin at once"""
    k = 64
    g = toy([b"AC" * 50], k=k)
    left, right = b"AC" * 32, b"GT" * 32
    alike = lambda a, b: {a, b} <= {b"AC" * 32, b"CA" * 32, b"GT" * 32, b"TG" * 32} or a == b
    text, r = gap(g, left, right, 70, k=k)
    assert r.record() == (0, EXHAUSTED, LOOP, NO_NEIGHBOR, 2, 0, -1, 0)
    text, r = gap(g, left, right, 70, k=k, same=alike)
    assert r.how == LEFT_ARRIVED


# ---- the worlds of the device test, on the CPU oracle ----
class ConnectWorld:
    """Synthetic transcripts tiled with reads, and segment lists cut out of them as SeqUtils.filterFastq would cut a read with masked stretches:
    plain reads with one or two masked stretches of 1 .. 10 letters; a fork where a four times heavier isoform leads the left walk away
    (RIGHT_ARRIVED, PATHS_MEET); a poly-A run of k + 15 inside a transcript, the left walk looping on A^k and the right walk entering it
    (MEET_LOW_COMPLEXITY); a left segment ending in an erroneous base beside a tandem repeat that the right segment starts in (RIGHT_LOOP), and a
    left segment ending in that repeat (LOOP); a right segment that begins one letter behind the start of the left segment's last k-mer, with a
    zero-length placeholder (the empty path); placeholders shorter than what they stand for (BOUND, PATHS_MEET not connected); erroneous bases
    on both sides (NO_NEIGHBOR twice); lists of 0, 1 and an even number of entries, a short segment, an N in a segment, a lower-case read with U.
    Every branch is reached on these worlds; none is left to the toy graphs alone."""

    def __init__(self, k, stranded, seed, hashes=(2, 2), n_plain=260, sizes=(2_400_011, 2_400_011)):
        from oracle import rbo
        rng = np.random.default_rng(seed)
        self.k, self.stranded, self.hashes, self.sizes = k, stranded, hashes, sizes
        rnd = lambda n: np.frombuffer(ACGT, np.uint8)[rng.integers(0, 4, n)].tobytes()
        sub = lambda s, p: R.put(s, p, "ACGT"[("ACGT".index(chr(s[p])) + 1 + int(rng.integers(0, 3))) % 4])
        L = self.L = 4 * k + 50
        plain = self.plain = [rnd(5 * L) for _ in range(3)]
        fp, fa, fb = rnd(2 * L), rnd(2 * L), rnd(2 * L)
        fb = R.put(fb, 0, "ACGT"[(ACGT.index(fa[:1]) + 1) % 4])                            # the branches part at their first letter
        pw, pz = rnd(L + k), rnd(L + k)
        run = k + 15
        poly = pw + b"A" * run + pz
        u = k // 2 + 2
        unit, tw, tz = rnd(u), rnd(L + k), rnd(L + k)
        reps = (3 * k) // u + 3
        tandem = tw + unit * reps + tz
        tx = [(t, 1) for t in plain] + [(fp + fa, 1), (fp + fb, 4), (poly, 1), (tandem, 1)]
        reads = []
        for t, m in tx:
            starts = list(range(0, len(t) - L + 1, 7 if k <= 25 else k // 3))
            if starts[-1] != len(t) - L:
                starts.append(len(t) - L)
            reads += [t[a:a + L] for a in starts] * m
        self.og = rbo.Graph(sizes[0], sizes[1], 1_000_003, hashes[0], hashes[1], 2, k, stranded, False, 5)
        self.packed = rbo.pack_reads(reads, [b"I" * len(s) for s in reads])
        self.og.add_reads(*self.packed, 3, 0)
        self.o = R.OracleSide(self.og)

        def cut(t, masks):
            """t with the stretches (start, length, placeholder length) masked: the list filterFastq gives"""
            out, at = [], 0
            for s, n, p in masks:
                out += [t[at:s], b"N" * p]
                at = s + n
            return out + [t[at:]]

        lists = []
        for i in range(n_plain):
            t = plain[i % 3]
            a = int(rng.integers(0, len(t) - L))
            rd = t[a:a + L]
            m1 = int(rng.integers(1, 11))
            s1 = int(rng.integers(k, L - 2 * k - 30))
            masks = [(s1, m1, m1)]
            if i % 2:
                m2 = int(rng.integers(1, 11))
                s2 = int(rng.integers(s1 + m1 + k, L - k - m2))
                masks.append((s2, m2, m2))
            if i % 10 == 3:
                masks[0] = (s1, m1, max(0, m1 - int(rng.integers(1, 4))))                    # a placeholder that is too short
            lists.append(cut(rd, masks))
        t = fp + fa
        for back in range(0, 14):                                                          # the fork: left ends `back` letters before it
            for m in (3, 8):
                rd = t[2 * L - L // 2 - back:2 * L + L // 2]
                lists.append(cut(rd, [(L // 2, m, m)]))
        p0 = len(pw)
        for back in (2, 4, 9):                                                             # the poly-A run, masked from `back` letters before it
            rd = poly[p0 - back - k - 10:p0 + run + k + 12]
            lists.append(cut(rd, [(k + 10, back + run + 2, back + run + 2)]))
        t0 = len(tw)
        for j in (0, 3):                                                                   # the tandem repeat
            lists.append([sub(tw[-k - 20:], k + 19), b"N" * 5, tandem[t0 + u + 3 + j:t0 + u + 3 + j + k + 12]])
            lists.append([tandem[t0 - 9:t0 + k + u + 2 + j], b"N" * (2 * k), tz[5:k + 25]])
        for t in plain:                                                                    # the empty path; long gaps under short placeholders; errors
            lists.append([t[10:k + 30], b"", t[31:k + 60]])
            lists += [[t[10:k + 30], b"", t[31 + j:k + 60 + j]] for j in (1, k - 2, k - 1)]     # paths of 1, k - 2, k - 1 k-mers: the segments overlap
            lists.append([t[10:k + 30], b"N", t[k + 110:2 * k + 130]])
            lists.append([t[10:k + 30], b"NN", t[2 * k + 37:3 * k + 60]])
            lists.append([sub(t[10:k + 30], k + 19), b"NNNN", sub(t[k + 34:2 * k + 60], 0)])
            lists.append([t[10:k + 30], b"N" * 3, t[k + 33:2 * k + 60], b"N" * 2, t[2 * k + 62:3 * k + 92]])      # three segments, equal first and last
        t = plain[0]
        lists += [[], [t[:k + 9]], [t[:k - 3]], [b"acgtNNnn"], [t[:k + 9], b"NN"], [t[:k + 9], b"NN", t[k + 11:2 * k + 20], b"N"],
                  [t[:k - 1], b"NN", t[k + 1:2 * k + 20]], [t[:k + 9], b"NN", t[k + 11:2 * k + 9]], [R.put(t[:k + 9], 4, "N"), b"NN", t[k + 11:2 * k + 20]],
                  [t[:k + 9].lower().replace(b"t", b"u"), b"NN", t[k + 11:2 * k + 20].replace(b"T", b"U")], [t[:k + 9], b"NN", R.put(t[k + 11:2 * k + 40], k + 3, "R")]]
        self.lists = lists
        self._want = None

    def want(self):
        if self._want is None:
            self._want = [connect(self.o, s, 0, self.k) for s in self.lists]
        return self._want

    def assert_every_branch_is_reached(self):
        want = self.want()
        gaps = [g for r in want for g in r.gaps]
        hows = {g.how for g in gaps}
        assert hows == set(range(7)), sorted(set(range(7)) - hows)
        l_ends, r_ends = {g.l_end for g in gaps}, {g.r_end for g in gaps}
        assert l_ends == {NOT_RUN, NO_NEIGHBOR, LOOP, BOUND, ARRIVED}, l_ends                # (a left walk never meets anything)
        assert r_ends == {NOT_RUN, NO_NEIGHBOR, LOOP, BOUND, ARRIVED, MET}, r_ends
        assert {g.connected for g in gaps if g.how == PATHS_MEET} == {0, 1}
        assert any(g.how == LEFT_ARRIVED and g.path_len == 0 for g in gaps)                  # the empty path
        assert any(0 < g.path_len < self.k - 1 and g.connected for g in gaps)                # the overlapping form
        assert {r.outcome for r in want} == {EMPTY, SINGLE, CHAINED, NOT_JUDGED} and {r.why for r in want} == {WHY_NONE, EVEN_COUNT, SHORT, INVALID_LETTER}
        assert any(r.outcome == CHAINED and r.first_seg > 0 for r in want) and any(r.outcome == CHAINED and r.connected == 2 for r in want)


WORLDS = {}


def world(k, stranded, hashes=(2, 2)):
    key = (k, stranded, hashes)
    if key not in WORLDS:
        WORLDS[key] = ConnectWorld(k, stranded, seed=900 + k + stranded, hashes=hashes, n_plain=260 if k == 25 else 30)
    return WORLDS[key]


@pytest.mark.parametrize("stranded", [False, True])
def test_worlds_reach_every_branch_on_the_oracle(stranded):
    world(25, stranded).assert_every_branch_is_reached()


# ---- the composed route of the package (getMaxCoveragePaths + stitching) without a device: its graph is a stand-in over the restated walk ----
class WalkStandIn:
    """what graphutils.getMaxCoveragePaths asks of a graph: k and walkMaxCov, answered by the restated neighbour step"""

    def __init__(self, g, k):
        self.g, self.k = g, k

    def walkMaxCov(self, seeds, direction, bound, minKmerCov=1.0, targets=None, hashes=True, counts=True):
        n = len(seeds)
        bases, ln, reason = np.zeros((n, max(bound, 1)), np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int64)
        for i, seed in enumerate(seeds):
            cur, seen, reason[i] = seed, set(), 3
            for depth in range(bound):
                cur = max_cov_neighbor(self.g, cur, direction, minKmerCov)
                if cur is None:
                    reason[i] = 0
                    break
                if targets is not None and cur == targets[i]:
                    reason[i] = 1
                    break
                if cur in seen:
                    reason[i] = 2
                    break
                seen.add(cur)
                bases[i, ln[i]] = cur[-1] if direction == 0 else cur[0]
                ln[i] += 1
        return bases, None, None, None, ln, reason


def test_the_composed_route_equals_the_restatement_on_the_toy_graphs():
    g = fork()
    cases = [[P, b"N" * 14, X[12:21]], [P[:9], b"N" * 14, X[12:21]], [P[:9], b"N", X[12:21]], [X[:9], b"NNN", X[12:21], b"NN", X[22:]], [X[:9]], []]
    assert graphutils.connectComposed(WalkStandIn(g, K), cases) == [connect(g, s, 0, K).text for s in cases]


# ---- rnabloom.io.filterFastq / filterFasta against hand-written cases (SeqUtils.java:1833-1934) ----
def test_filter_fasta():
    from rnabloom.io import filterFasta
    assert filterFasta(b"ACGTACGT", 4) == [b"ACGTACGT"]
    assert filterFasta(b"acgunACGTTnnACGTA", 4) == [b"ACGU", b"N", b"ACGTT", b"NN", b"ACGTA"]              # upper case, U stays, "N" and a run of N
    assert filterFasta(b"NNACGTNACGNNACGTT", 4) == [b"ACGT", b"NNNNNN", b"ACGTT"]                          # a run under k joins the gap; the head is dropped
    assert filterFasta(b"ACGTNN", 4) == [b"ACGT"] and filterFasta(b"ACG", 4) == [] and filterFasta(b"", 4) == []
    assert filterFasta("ACGTRACGT", 4) == [b"ACGT", b"N", b"ACGT"]                                         # whatever the letter was, the placeholder is N


def test_filter_fastq():
    from rnabloom.io import filterFastq
    q = lambda s: bytes(33 + int(c) * 5 for c in s)                                                       # a digit a letter: quality 0, 5, 10, ...
    assert filterFastq(b"ACGTACGT", q("88888888"), 4, 3) == [b"ACGTACGT"]
    assert filterFastq(b"ACGTACGTA", q("888808888"), 4, 3) == [b"ACGT", b"N", b"CGTA"]                    # one low quality letter: "N"
    assert filterFastq(b"ACGTGGACGTA", q("88880088888"), 4, 3) == [b"ACGT", b"NN", b"ACGTA"]
    assert filterFastq(b"ACGTACGTA", q("888808888"), 4, 0) == [b"ACGTACGTA"]                              # minBaseQual 0 keeps everything
    assert filterFastq(b"ACGTNCGTA", q("888888888"), 4, 3) == [b"ACGT", b"N", b"CGTA"]                    # the letter filter behind the quality filter
    assert filterFastq(b"ACGTACG" + b"TTTTT", q("8888088" + "08888"), 4, 3) == [b"ACGT", b"NNNN", b"TTTT"]    # CG is a run under k: with its two neighbours one gap of four
    assert filterFastq(b"acguACGT", q("88888888"), 8, 3) == [b"ACGUACGT"]
    assert filterFastq(b"", b"", 4, 3) == [] and filterFastq(b"ACGT", b"", 4, 3) == [] and filterFastq(b"ACGT", q("0000"), 4, 3) == []
    # quality 2 is below 3 and 3 is not
    assert filterFastq(b"ACGTACGTA", b"IIII" + bytes([35]) + b"IIII", 4, 3) == [b"ACGT", b"N", b"CGTA"]
    assert filterFastq(b"ACGTACGTA", b"IIII" + bytes([36]) + b"IIII", 4, 3) == [b"ACGTACGTA"]


def test_header_python_java_and_jni_sides_exist():
    import os, re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "rb_capi.h")).read()
    for name, val in (("EMPTY", EMPTY), ("SINGLE", SINGLE), ("CHAINED", CHAINED), ("NOT_JUDGED", NOT_JUDGED), ("WHY_EVEN_COUNT", EVEN_COUNT), ("WHY_SHORT", SHORT),
                      ("WHY_INVALID_LETTER", INVALID_LETTER), ("HOW_LEFT_ARRIVED", LEFT_ARRIVED), ("HOW_RIGHT_ARRIVED", RIGHT_ARRIVED), ("HOW_PATHS_MEET", PATHS_MEET),
                      ("HOW_MEET_LOW_COMPLEXITY", MEET_LOW_COMPLEXITY), ("HOW_RIGHT_LOOP", RIGHT_LOOP), ("HOW_EXHAUSTED", EXHAUSTED), ("END_NOT_RUN", NOT_RUN),
                      ("END_NO_NEIGHBOR", NO_NEIGHBOR), ("END_LOOP", LOOP), ("END_BOUND", BOUND), ("END_ARRIVED", ARRIVED), ("END_MET", MET)):
        assert re.search(r"\bRB_CONNECT_%s = %d\b" % (name, val), hdr), name
    from rnabloom.graph import BloomFilterDeBruijnGraph as G
    assert G.CONNECT_DTYPE.itemsize == 32 and G.CONNECT_GAP_DTYPE.itemsize == 32
    assert G.CONNECT_HOWS[PATHS_MEET] == "paths_meet" and G.CONNECT_ENDS[MET] == "met" and G.CONNECT_WHYS[EVEN_COUNT] == "even_count"
    assert "connectSegments(" in open(os.path.join(root, "java", "rnabloom", "graph", "NativeGraph.java")).read()
    assert "rb_graph_connect_segments(" in open(os.path.join(root, "jni", "rb_jni.c")).read()
