"""The fragment screens of TranscriptAssemblyWorker.run (R/RNABloom.java:1816-1927) restated line by line in Python over the CPU oracle:
GraphUtils.isBranchFree (R/util/GraphUtils.java:7651-7672), isChimera (:7674-7760), isBluntEndArtifact (:8535-8586), the four static
hasDepthRight / hasDepthLeft (:6680-6778) and the gated getMaxCoveragePath (:1677-1776), over an oracle graph plus a second oracle graph whose
dbgbf is the `BloomFilter assembledKmers`.  The gated greedy walks and steps are oracle.rbo.greedy_extend(gate=...).  A restated screen
returns the 8 fields of rb_screen_rec and, per hasDepth* call, the number of getSuccessors / getPredecessors calls it made.
The worlds of tests/test_gpu_screen.py are built here on the oracle alone — a few genes with isoforms, reads at coverage, a gate filled with
the k-mers of the transcripts that count as assembled — and every branch the device test relies on is shown to be reached by a named query.
Everything is made once and mirrored: the reversed transcripts are inserted too and the reversed queries meet the other arm and the other
scan.  No device is needed here."""
import numpy as np
import pytest

from test_extend_step_rules import F32, ACGT, median_cov, neighbor

BRANCH_FREE, CHIMERA, BLUNT_END, BAD_LETTER, NO_KMER, OVER_BUDGET = 1, 2, 4, 8, 16, 32
CHIM_ENDS, CHIM_ASSEMBLED, CHIM_WIDE_GAP, CHIM_PATHS_MEET, CHIM_DISJOINT = range(5)
BLUNT_NO_ARM, BLUNT_LEFT_RANGE, BLUNT_RIGHT_RANGE, BLUNT_LEFT_FAILED, BLUNT_RIGHT_FAILED, BLUNT_LEFT_ARTIFACT, BLUNT_RIGHT_ARTIFACT = range(7)
DEFAULT_VISITS = 65536
GREEDY_BOUND = 1000


class OverBudget(Exception):
    """a hasDepth* search was about to make more calls than its budget allows"""


class Side:
    """what the restatement asks of the two oracle graphs, memoised per k-mer: graph.getCount and assembledKmers.lookup"""

    def __init__(self, og, gate_og):
        from oracle import rbo
        self.rbo, self.og, self.gate_og, self.k, self.stranded = rbo, og, gate_og, og.k, og.stranded
        self.mode = rbo.FWD if og.stranded else rbo.CANON
        self._c, self._g, self._g0 = {}, {}, {}

    def counts(self, seq):
        return [F32(c) for c in self.og.get_kmers(seq)[2]]

    def count(self, kmer):
        c = self._c.get(kmer)
        if c is None:
            c = self._c[kmer] = F32(self.og.get_kmers(kmer)[2][0])
        return c

    def gate(self, kmer):
        g = self._g.get(kmer)
        if g is None:
            hv, _ = self.rbo.hash_region(kmer, self.k, self.gate_og.h, self.mode)
            g = self._g[kmer] = self.gate_og.contains(hv[0])
        return g

    def gate_h0(self, h0):
        """the gate asked with a k-mer's hash value, as rbo.greedy_extend asks it"""
        g = self._g0.get(h0)
        if g is None:
            g = self._g0[h0] = self.gate_og.contains(self.rbo.ntm64(int(h0), self.k, self.gate_og.h))
        return g

    def neighbours(self, kmer, direction, gated):
        """Kmer.getSuccessors / getPredecessors(k, numHash, graph) (R/graph/Kmer.java:199-255: count >= 1) and the gated form (:257-299:
        bf.lookup first, then count > 0), in the order A C G T"""
        out = []
        for b in range(4):
            nb = neighbor(kmer, b, direction)
            if gated:
                if self.gate(nb) and self.count(nb) > 0:
                    out.append(nb)
            elif self.count(nb) >= 1:
                out.append(nb)
        return out

    def greedy_walk(self, kmer, direction, lookahead, bound):
        """greedyExtendRight / Left(graph, source, lookahead, bound, bf) (:1978-1997, :1940-1959) as the k-mers added, in walking order"""
        bases, _ = self.rbo.greedy_extend(self.og, kmer, direction, lookahead, bound, k=self.k, gate=self.gate_h0, stranded=self.stranded)
        out, cur = [], kmer
        for b in bases:
            cur = neighbor(cur, ACGT.index(bytes([b])), direction)
            out.append(cur)
        return out

    def greedy_once(self, kmer, direction, lookahead):
        """one neighbour taken as is, several through greedyExtend{Right,Left}Once(graph, neighbors, lookahead, bf) (:1703-1708, :1738-1743)"""
        w = self.greedy_walk(kmer, direction, lookahead, 1)
        return w[0] if w else None


def max_coverage_path(s, left, right, bound, lookahead, tags=None):
    """getMaxCoveragePath(graph, left, right, bound, lookahead, bf) (:1677-1776): the path as a list, or None"""
    left_set, left_path = set(), []
    best = left
    for step in range(bound):
        best = s.greedy_once(best, 0, lookahead)
        if best is None:
            break
        if best == right:
            if tags is not None:
                tags.add("path_from_the_left")
                if step >= 64: tags.add("left_walk_arrives_after_64_steps")     # its 65th step or a later one: the walk's set held 64 k-mers and more
            return left_path
        if best in left_set:
            break
        left_set.add(best); left_path.append(best)
    right_set, right_path = set(), []
    best = right
    for _ in range(bound):
        best = s.greedy_once(best, 1, lookahead)
        if best is None:
            break
        if best == left:
            if tags is not None: tags.add("path_from_the_right")
            return right_path
        elif best in left_set:
            right_path.insert(0, best)
            for idx in range(len(left_path) - 1, -1, -1):
                if left_path[idx] == best:
                    if tags is not None:
                        tags.add("paths_spliced")                 # (ScPath.form == 3, met at entry idx of the left walk)
                        if idx >= 64: tags.add("spliced_at_entry_64_or_beyond")
                    return left_path[:idx] + right_path
        elif best not in right_set:
            right_set.add(best); right_path.insert(0, best)
        else:
            if tags is not None: tags.add("right_path_loops")
            return None
    return None


def is_branch_free(s, seq, tags=None):
    """isBranchFree (:7651-7672).  var.hasDepthRight / hasDepthLeft are the MEMBER functions (R/graph/Kmer.java:407-486), which never consult
    the graph and always answer true: a variant with count >= 1 decides."""
    k = s.k
    for p in range(len(seq) - k + 1):
        kmer = seq[p:p + k]
        for b in range(4):                                       # getRightVariants (:382-405): the other last bases
            if ACGT[b] != kmer[-1] and s.count(kmer[:-1] + ACGT[b:b + 1]) >= 1:
                if tags is not None: tags.add("right_variant")
                return False
        for b in range(4):                                       # getLeftVariants (:357-380)
            if ACGT[b] != kmer[0] and s.count(ACGT[b:b + 1] + kmer[1:]) >= 1:
                if tags is not None: tags.add("left_variant")
                return False
    return True


def is_chimera(s, seq, lookahead, tags=None):
    """isChimera (:7674-7760) -> (answer, chim_why, i, j, right walk's length, left walk's length)"""
    k = s.k
    kmers = [seq[p:p + k] for p in range(len(seq) - k + 1)]
    n, max_gap = len(kmers), 2 * k
    tags = set() if tags is None else tags
    if not (s.gate(kmers[0]) and s.gate(kmers[n - 1])):
        return False, CHIM_ENDS, -1, -1, 0, 0
    i = 1
    while i < n - 1:
        if not s.gate(kmers[i]):
            left = kmers[i - 1]
            t = i + 1
            while t < n - 1:
                if s.gate(kmers[t]):
                    break
                t += 1
            if t < n - 1:
                right, d = kmers[t], t - i
                if d <= max_gap and max_coverage_path(s, left, right, d, lookahead, tags) is not None:
                    tags.add("bridged_by_the_forward_scan")
                    i = t
                    i += 1
                    continue
            break
        i += 1
    if i == n - 1:
        return False, CHIM_ASSEMBLED, -1, -1, 0, 0
    i -= 1
    j = n - 2
    while j > i:
        if not s.gate(kmers[j]):
            right = kmers[j + 1]
            t = j - 1
            while t > i:
                if s.gate(kmers[t]):
                    break
                t -= 1
            if t > i:
                left, d = kmers[t], j - t
                if d <= max_gap and max_coverage_path(s, left, right, d, lookahead, tags) is not None:
                    tags.add("bridged_by_the_backward_scan")
                    j = t
                    j -= 1
                    continue
            break
        j -= 1
    j += 1
    if j - i <= max_gap:
        w1 = s.greedy_walk(kmers[i], 0, lookahead, GREEDY_BOUND)
        w2 = s.greedy_walk(kmers[j], 1, lookahead, GREEDY_BOUND)
        if len(w1) == GREEDY_BOUND or len(w2) == GREEDY_BOUND:
            tags.add("walk_hits_the_bound")
        if any(len(s.neighbours(km, 0, True)) > 1 for km in [kmers[i]] + w1[:-1]) or any(len(s.neighbours(km, 1, True)) > 1 for km in [kmers[j]] + w2[:-1]):
            tags.add("walk_scores_candidates")                 # a step with several gated neighbours: the lookahead decides
        if not set(w1) & set(w2):
            return True, CHIM_DISJOINT, i, j, len(w1), len(w2)
        return False, CHIM_PATHS_MEET, i, j, len(w1), len(w2)
    return False, CHIM_WIDE_GAP, i, j, 0, 0


def has_depth(s, source, direction, depth, gated, budget=None):
    """the static hasDepthRight / hasDepthLeft(source, graph, depth[, bf]) (:6680-6778) -> (answer, getSuccessors / getPredecessors calls)"""
    calls = [0]

    def nbrs(kmer):
        if budget is not None and calls[0] >= budget:
            raise OverBudget()
        calls[0] += 1
        return s.neighbours(kmer, direction, gated)
    frontier = [nbrs(source)]
    while frontier:
        alts = frontier[-1]
        if not alts:
            frontier.pop()
        else:
            frontier.append(nbrs(alts.pop(0)))
        if len(frontier) >= depth:
            return True, calls[0]
    return False, calls[0]


def is_blunt_end_artifact(s, seq, max_depth, d, budget=None, visits=None, tags=None):
    """isBluntEndArtifact (:8535-8586) -> (answer, blunt_why, boundary).  visits collects the call count of every hasDepth* search made."""
    if max_depth <= 0:
        return False, BLUNT_NO_ARM, -1
    k = s.k
    kmers = [seq[p:p + k] for p in range(len(seq) - k + 1)]
    cnt = s.counts(seq)
    n = len(kmers)
    visits = [] if visits is None else visits
    tags = set() if tags is None else tags

    def depth(source, direction, dep, gated):
        ans, calls = has_depth(s, source, direction, dep, gated, budget)
        visits.append(calls)
        return ans
    left_edge, right_edge = min(cnt[0:min(max_depth, n)]), min(cnt[max(0, n - max_depth):n])
    if s.gate(kmers[0]) and (not s.gate(kmers[n - 1]) or left_edge > right_edge):
        i = 1
        while i < n:
            if not s.gate(kmers[i]):
                break
            i += 1
        if i == n or i < n - d:
            return False, BLUNT_LEFT_RANGE, i
        if depth(kmers[n - 1], 0, max_depth, False):
            tags.add("end_has_depth")
            return False, BLUNT_LEFT_FAILED, i
        if not median_cov(cnt[0:i]) > median_cov(cnt[i:n]):
            tags.add("median_not_above")
            return False, BLUNT_LEFT_FAILED, i
        if not depth(kmers[i - 1], 0, n - i, True):
            tags.add("assembled_path_too_short")
            return False, BLUNT_LEFT_FAILED, i
        return True, BLUNT_LEFT_ARTIFACT, i
    elif s.gate(kmers[n - 1]) and (not s.gate(kmers[0]) or left_edge < right_edge):
        j = n - 2
        while j >= 0:
            if not s.gate(kmers[j]):
                break
            j -= 1
        if j == -1 or j > d:
            return False, BLUNT_RIGHT_RANGE, j + 1
        if depth(kmers[0], 1, max_depth, False):
            tags.add("end_has_depth")
            return False, BLUNT_RIGHT_FAILED, j + 1
        if not median_cov(cnt[j + 1:n]) > median_cov(cnt[0:j + 1]):
            tags.add("median_not_above")
            return False, BLUNT_RIGHT_FAILED, j + 1
        if not depth(kmers[j + 1], 1, j + 1, True):
            tags.add("assembled_path_too_short")
            return False, BLUNT_RIGHT_FAILED, j + 1
        return True, BLUNT_RIGHT_ARTIFACT, j + 1
    return False, BLUNT_NO_ARM, -1


def is_acgtu(seq):
    return all(c in b"ACGTUacgtu" for c in seq)


class Screened:
    """the record of one sequence (rb_screen_rec) with what the restatement saw on its way"""

    def __init__(self, record, visits=(), tags=()):
        self.record, self.visits, self.tags = tuple(record), list(visits), set(tags)


def screen(s, seq, what, lookahead, max_depth, d, max_visits=0):
    """what rb_graph_screen_fragments reports for one sequence"""
    blank = [0, 0, -1, -1, 0, 0, 0, -1]
    if len(seq) < s.k:
        blank[0] = NO_KMER
        return Screened(blank)
    if not is_acgtu(seq):
        blank[0] = BAD_LETTER
        return Screened(blank)
    seq = seq.upper().replace(b"U", b"T")
    rec, tags, visits = blank, set(), []
    if what & BRANCH_FREE and is_branch_free(s, seq, tags):
        rec[0] |= BRANCH_FREE
    if what & CHIMERA:
        ans, rec[1], rec[2], rec[3], rec[4], rec[5] = is_chimera(s, seq, lookahead, tags)
        tags.add("chim_why_%d" % rec[1])
        if ans:
            rec[0] |= CHIMERA
    if what & BLUNT_END:
        try:
            ans, rec[6], rec[7] = is_blunt_end_artifact(s, seq, max_depth, d, max_visits or DEFAULT_VISITS, visits, tags)
            tags.add("blunt_why_%d" % rec[6])
            if ans:
                rec[0] |= BLUNT_END
        except OverBudget:
            # not judged: no answer, blunt_why 0; the arm's boundary is known before any search starts (asked again here without a budget)
            rec[0] |= OVER_BUDGET
            rec[6], rec[7] = 0, is_blunt_end_artifact(s, seq, max_depth, d, None, [], set())[2]
            tags.add("over_budget")
    return Screened(rec, visits, tags)


# ---- hand-worked: hasDepth's test of frontier.size() on a toy graph ----
class ToySide:
    def __init__(self, k, kmers, gated=()):
        self.k, self.present, self.gated = k, set(kmers), set(gated)

    def neighbours(self, kmer, direction, gated):
        return [nb for nb in (neighbor(kmer, b, direction) for b in range(4)) if nb in self.present and (not gated or nb in self.gated)]


def test_has_depth_counts_levels_empty_ones_included():
    text = b"ACGTTGCA"                                           # a path of five 4-mers without a branch
    kmers = [text[p:p + 4] for p in range(5)]
    t = ToySide(4, kmers, kmers[:3])
    assert has_depth(t, kmers[0], 0, 1, False) == (True, 2)      # the size is tested after the first push only: two calls for depth 1
    assert has_depth(t, kmers[4], 0, 1, False) == (False, 1)     # a dead end: the empty level is removed, size 0
    assert has_depth(t, kmers[0], 0, 5, False) == (True, 5)      # four k-mers behind the source, and the last one's empty level counts
    assert has_depth(t, kmers[0], 0, 6, False) == (False, 5)
    assert has_depth(t, kmers[0], 0, 3, True) == (True, 3) and has_depth(t, kmers[0], 0, 4, True) == (False, 3)
    assert has_depth(t, kmers[4], 1, 5, False) == (True, 5) and has_depth(t, kmers[4], 1, 6, False) == (False, 5)
    with pytest.raises(OverBudget):
        has_depth(t, kmers[0], 0, 5, False, budget=4)
    assert has_depth(t, kmers[0], 0, 5, False, budget=5) == (True, 5)
    fork = ToySide(4, [b"ACGT", b"CGTA", b"CGTC", b"GTCA"])      # A C G T order: the dead branch first, then the one that goes on
    assert has_depth(fork, b"ACGT", 0, 3, False) == (True, 4)    # ACGT, CGTA (empty, removed), CGTC, GTCA
    assert has_depth(fork, b"ACGT", 0, 4, False) == (False, 4)


# ---- the worlds of the device test, on the CPU oracle ----
def put(s, pos, ch):
    b = bytearray(s); b[pos] = ord(ch); return bytes(b)


def other(ch):
    return ACGT[(ACGT.index(bytes([ch])) + 1) % 4:][:1]


class ScreenWorld:
    """Transcripts tiled with reads (a k-mer counts about read_len / tile times its transcript's multiplicity), a gate holding the k-mers of
    those that count as assembled, and named queries.  d is the read-paired k-mer distance; the unassembled tails are at most 29 k-mers."""
    TAIL = 20
    LONGEST_TAIL = 29

    SIZES = (4_800_011, 4_800_011, 4_800_017)
    GATE_SIZE = 1_200_007

    def __init__(self, k, stranded, seed, d=30, hashes=(2, 2, 2), gate_h=2, read_len=100, tile=10, seg=150, long_len=1300, sizes=None, gate_size=None):
        from oracle import rbo
        rng = np.random.default_rng(seed)
        self.k, self.stranded, self.d, self.hashes, self.gate_h = k, stranded, d, hashes, gate_h
        rnd = lambda n: np.frombuffer(ACGT, np.uint8)[rng.integers(0, 4, n)].tobytes()
        tx, q, gate = [], [], []                                 # (transcript, multiplicity), (name, sequence), assembled transcripts
        only = []                                                # (name, sequence) queries that are not mirrored
        T = self.TAIL
        m = k + 35                                              # letters of a stretch of 36 k-mers
        # gene A: three exons; the full isoform is assembled, the exon-skipping one is not
        e1, e2, e3 = rnd(seg), rnd(seg), rnd(seg)
        a1, a2 = e1 + e2 + e3, e1 + e3
        tx += [(a1, 2), (a2, 1)]; gate.append(a1)
        # gene B: assembled; gene U: not assembled
        b1, u = rnd(3 * seg), rnd(2 * seg)
        tx += [(b1, 1), (u, 1)]; gate.append(b1)
        # gene C: two assembled isoforms that fork behind a shared first exon, covered 3 : 1 (the gated walk meets two candidates)
        f1, f2, f3 = rnd(seg), rnd(seg), rnd(seg)
        c1, c2 = f1 + f2, f1 + f3
        tx += [(c1, 3), (c2, 1)]; gate += [c1, c2]
        # an assembled transcript of more than 1100 k-mers, an assembled tandem repeat that is nothing else, and one inside a transcript
        big = rnd(long_len)
        unit = rnd(k + 9)
        circle = unit * max(4, (3 * k) // len(unit) + 3)
        w, z = rnd(seg), rnd(seg)
        tandem = w + unit[::-1] * 6 + z
        tx += [(big, 1), (circle, 1), (tandem, 1)]; gate += [big, circle, tandem]
        q += [("assembled", a1[40:2 * seg + 60]), ("assembled-long", big[:long_len - 7]), ("ends-not-assembled", u[10:seg + 40]),
              ("first-not-assembled", u[seg - m:seg] + a1[:m]), ("skipped-exon", a2[seg - m:seg + m]),
              ("chimera", a1[60:seg + 60] + b1[seg:2 * seg + 30]), ("chimera-fork", c1[20:seg - 10] + b1[seg + 5:2 * seg]),
              ("chimera-long", big[:m + 50] + b1[seg + 9:2 * seg]), ("chimera-circle", circle[3:3 + 2 * k] + b1[seg + 11:2 * seg]),
              ("chimera-tandem", tandem[seg - m:seg + 20] + b1[seg + 13:2 * seg]),
              ("wide-gap", a1[:m] + rnd(2 * k + 12) + a1[2 * seg:2 * seg + m]),
              ("snv-bridged", put(a1[30:2 * seg], k + 75, chr(other(a1[k + 105])[0]))),
              ("chimera-then-snv", a1[60:seg + 60] + put(b1[seg:3 * seg - 20], k + 105, chr(other(b1[seg + k + 105])[0]))),
              ("five-thousand-bases", ((big + a1 + b1 + c1 + tandem + u + c2 + big[::-1]) * 2)[:5000]),
              ("one-kmer-assembled", a1[70:70 + k]), ("two-kmers-assembled", a1[70:71 + k]), ("three-kmers-assembled", a1[70:72 + k]),
              ("one-kmer-not-assembled", u[70:70 + k]), ("branch-free", big[200:max(400, k + 257)])]        # (200 letters, and no fewer than 58 k-mers)
        for n_k in (63, 64, 65):
            q.append(("kmers-%d" % n_k, big[300:300 + n_k + k - 1]))
            q.append(("chimera-kmers-%d" % n_k, a1[60:70 + k] + b1[seg:seg + n_k - 11]))    # 11 k-mers of gene A, then gene B (k = 25)
        # a SNV pair, both in the reads: the k-mer that ends on it has a right variant, the one that starts on it a left variant
        v = rnd(2 * seg)
        tx += [(v, 2), (put(v, seg, chr(other(v[seg])[0])), 1)]
        q += [("right-variant-only", v[seg - m:seg + 1]), ("left-variant-only", v[seg:seg + m]), ("both-variants", v[seg - m:seg + m])]
        # blunt ends: an assembled transcript p + s covered five times, and reads that leave p's end by a tail that goes nowhere.  A tail's
        # reads start k - 1 letters before it, so they cover the tail's k-mers and nothing else.
        def blunt(name, tail_len, cover=5, tail_cover=1, s_len=seg, cut=0, lead=k + 75):
            p, s_, tail = rnd(seg), rnd(s_len), rnd(tail_len)
            tx.append((p + s_, cover)); gate.append(p + s_)
            tx.append((p[seg - k + 1:] + tail, tail_cover))
            return (name, p[seg - lead:] + tail[:tail_len - cut])
        q.append(blunt("blunt-artifact", T))
        q.append(blunt("blunt-end-has-depth", T, cut=6))                         # the query stops 6 letters before the tail does
        q.append(blunt("blunt-median-not-above", T, cover=1, tail_cover=8))
        q.append(blunt("blunt-assembled-path-short", T, s_len=T - 10))          # the assembled transcript ends 10 letters behind the fork
        q.append(blunt("blunt-tail-longer-than-d", d + 10))
        q.append(blunt("blunt-tail-of-d", d, cover=1, tail_cover=8, lead=k + 3))   # boundary == numKmers - d: the range test lets it pass
        only.append(blunt("blunt-longest-tail", self.LONGEST_TAIL))
        # both ends assembled, the edges' minima decide the arm: the first k-mers are covered more
        hi_lo = rnd(2 * seg)
        tx += [(hi_lo, 1), (hi_lo[:seg], 4)]; gate.append(hi_lo)
        q.append(("edges-decide", hi_lo[seg - m:seg + m + 20]))
        q += [("too-short", a1[:k - 1]), ("empty", b""), ("bad-letter", put(a1[40:100 + 2 * k], k + 2, "N")), ("bad-letter-short", put(a1[40:40 + k], 3, "N")),
              ("lower-case-and-u", a1[40:2 * seg + 60].lower().replace(b"t", b"u"))]
        self.tx, self.gate_tx = tx, gate
        self.queries = [(name, s_) for name, s_ in q] + [(name + "~", s_[::-1]) for name, s_ in q] + only
        self.names = [name for name, _ in self.queries]
        reads = []
        for t, m in tx:
            for tt in (t, t[::-1]):
                starts = list(range(0, max(len(tt) - read_len, 0) + 1, tile))
                if starts[-1] < len(tt) - read_len:
                    starts.append(len(tt) - read_len)
                reads += [tt[a:a + read_len] for a in starts] * m
        self.reads = reads
        self.sizes = tuple(sizes or self.SIZES)
        self.gate_size = gate_size or self.GATE_SIZE
        self.og = rbo.Graph(*self.sizes, *hashes, k, stranded, True, 5)
        self.og.set_read_pair_distance(d)
        self.packed = rbo.pack_reads(reads, [b"I" * len(s_) for s_ in reads])
        self.og.add_reads(*self.packed, 3, rbo.STORE_READ_PAIRS)
        self.gate_og = rbo.Graph(self.gate_size, 64, 0, gate_h, 1, 1, k, True, False, 0)
        self.gate_seqs = [t for g_ in gate for t in (g_, g_[::-1])]
        mode = rbo.FWD if stranded else rbo.CANON
        for t in self.gate_seqs:
            hv, _ = rbo.hash_region(t, k, self.gate_og.h, mode)
            for row in hv:
                self.gate_og.add_dbg_only(row)
        self.s = Side(self.og, self.gate_og)
        self._want = {}

    def want(self, lookahead, max_depth, what=7, max_visits=0):
        """the restatement's records for every query, computed once per setting"""
        key = (lookahead, max_depth, what, max_visits)
        if key not in self._want:
            self._want[key] = [screen(self.s, s_, what, lookahead, max_depth, self.d, max_visits) for _, s_ in self.queries]
        return self._want[key]

    def largest_visit_count(self, lookahead, max_depth):
        return max((max(st.visits) for st in self.want(lookahead, max_depth) if st.visits), default=0)

    def assert_every_branch_is_reached(self, lookahead=3, max_depth=2):
        got = dict(zip(self.names, self.want(lookahead, max_depth)))
        chim = {name: st.record[1] for name, st in got.items()}
        for name, why in (("ends-not-assembled", CHIM_ENDS), ("first-not-assembled", CHIM_ENDS), ("assembled", CHIM_ASSEMBLED),
                          ("assembled-long", CHIM_ASSEMBLED), ("wide-gap", CHIM_WIDE_GAP), ("skipped-exon", CHIM_PATHS_MEET),
                          ("chimera", CHIM_DISJOINT), ("chimera-fork", CHIM_DISJOINT), ("chimera-long", CHIM_DISJOINT),
                          ("chimera-circle", CHIM_DISJOINT), ("snv-bridged", CHIM_ASSEMBLED), ("chimera-then-snv", CHIM_DISJOINT),
                          ("one-kmer-assembled", CHIM_DISJOINT), ("two-kmers-assembled", CHIM_ASSEMBLED)):
            for nm in (name, name + "~"):
                assert chim[nm] == why, (nm, got[nm].record, why)
                assert bool(got[nm].record[0] & CHIMERA) == (why == CHIM_DISJOINT), nm
        assert "bridged_by_the_forward_scan" in got["snv-bridged"].tags and "bridged_by_the_forward_scan" in got["snv-bridged~"].tags
        assert "bridged_by_the_backward_scan" in got["chimera-then-snv"].tags and "bridged_by_the_backward_scan" not in got["snv-bridged"].tags
        assert "bridged_by_the_backward_scan" in got["chimera-then-snv~"].tags or "bridged_by_the_forward_scan" in got["chimera-then-snv~"].tags
        assert self.k - 2 <= got["chimera"].record[3] - got["chimera"].record[2] <= self.k         # the breakpoints sit k k-mers apart (less a letter the two sides may share)
        for name in ("chimera-long", "chimera-circle"):
            assert "walk_hits_the_bound" in got[name].tags and GREEDY_BOUND in got[name].record[4:6], (name, got[name].record)
        assert got["skipped-exon"].record[4] > 0 and got["skipped-exon"].record[5] > 0
        assert "walk_scores_candidates" in got["chimera-fork"].tags and "walk_scores_candidates" in got["chimera-fork~"].tags
        blunt = {name: st.record[6] for name, st in got.items()}
        for name, why, tag in (("blunt-artifact", BLUNT_LEFT_ARTIFACT, None), ("blunt-longest-tail", BLUNT_LEFT_ARTIFACT, None),
                               ("blunt-end-has-depth", BLUNT_LEFT_FAILED, "end_has_depth"), ("blunt-median-not-above", BLUNT_LEFT_FAILED, "median_not_above"),
                               ("blunt-assembled-path-short", BLUNT_LEFT_FAILED, "assembled_path_too_short"),
                               ("blunt-tail-longer-than-d", BLUNT_LEFT_RANGE, None), ("blunt-tail-of-d", BLUNT_LEFT_FAILED, "median_not_above"),
                               ("assembled", None, None), ("ends-not-assembled", BLUNT_NO_ARM, None), ("edges-decide", BLUNT_LEFT_RANGE, None)):
            for nm, shift in ((name, 0), (name + "~", 1)):
                if nm not in got:
                    continue
                if why is not None:
                    assert blunt[nm] == (why + shift if why else why), (nm, got[nm].record)
                assert bool(got[nm].record[0] & BLUNT_END) == (why == BLUNT_LEFT_ARTIFACT), nm
                if tag:                                          # that clause failed, and alone: the other two hold when asked on their own
                    assert tag in got[nm].tags and len(got[nm].tags & {"end_has_depth", "median_not_above", "assembled_path_too_short"}) == 1, (nm, got[nm].tags)
        assert got["blunt-tail-of-d"].record[7] == len(self.queries[self.names.index("blunt-tail-of-d")][1]) - self.k + 1 - self.d
        assert got["edges-decide"].record[7] == len(self.queries[self.names.index("edges-decide")][1]) - self.k + 1          # boundary == numKmers
        for name, flag in (("branch-free", True), ("right-variant-only", False), ("left-variant-only", False), ("both-variants", False)):
            for nm in (name, name + "~"):
                assert bool(got[nm].record[0] & BRANCH_FREE) == flag, nm
        assert got["right-variant-only"].tags & {"right_variant", "left_variant"} == {"right_variant"}
        assert got["left-variant-only"].tags & {"right_variant", "left_variant"} == {"left_variant"}
        assert got["left-variant-only~"].tags & {"right_variant", "left_variant"} == {"right_variant"}
        for name in ("too-short", "empty", "too-short~"):
            assert got[name].record == (NO_KMER, 0, -1, -1, 0, 0, 0, -1)
        for name in ("bad-letter", "bad-letter-short", "bad-letter~"):
            assert got[name].record == (BAD_LETTER, 0, -1, -1, 0, 0, 0, -1)
        assert got["lower-case-and-u"].record == got["assembled"].record
        # the budget: no query comes near the default, so no device record may carry the over-budget bit
        assert not any(st.record[0] & OVER_BUDGET for st in got.values())
        assert 0 < self.largest_visit_count(lookahead, max_depth) < DEFAULT_VISITS // 4


WORLDS = {}


def world(k, stranded):
    if (k, stranded) not in WORLDS:
        WORLDS[(k, stranded)] = ScreenWorld(k, stranded, seed=900 + stranded)
    return WORLDS[(k, stranded)]


def world_143():
    if 143 not in WORLDS:
        WORLDS[143] = ScreenWorld(143, False, seed=943, read_len=400, tile=40, seg=500, long_len=1400)
    return WORLDS[143]


def world_hashes():
    """hash counts other than 2 / 2 / 2: dbgbf 1, counting filter 3, gate 3"""
    if "h" not in WORLDS:
        WORLDS["h"] = ScreenWorld(25, False, seed=977, hashes=(1, 3, 2), gate_h=3)
    return WORLDS["h"]


@pytest.mark.parametrize("stranded", [False, True])
def test_worlds_reach_every_branch_on_the_oracle(stranded):
    w = world(25, stranded)
    w.assert_every_branch_is_reached(3, 2)
    # max_depth 0 answers false before anything is looked at; a depth above the longest tail makes other searches (and other edge minima)
    for st in w.want(3, 0):
        assert st.record[6:] == (0, -1) and not st.visits and not st.record[0] & BLUNT_END
    deep = w.want(5, ScreenWorld.LONGEST_TAIL + 16)
    assert {st.record[6] for st in deep} == {0, 1, 2, 3, 4, 5, 6} and {st.record[1] for st in deep} == {0, 1, 2, 3, 4}
    assert w.largest_visit_count(5, ScreenWorld.LONGEST_TAIL + 16) < DEFAULT_VISITS // 4


def test_the_budget_flips_exactly_the_query_with_the_most_calls():
    w = world(25, False)
    base = w.want(3, 2)
    most = w.largest_visit_count(3, 2)
    who = [i for i, st in enumerate(base) if st.visits and max(st.visits) == most]
    assert [w.names[i] for i in who] == ["blunt-longest-tail"] and most >= ScreenWorld.LONGEST_TAIL - 1
    at, below = w.want(3, 2, max_visits=most), w.want(3, 2, max_visits=most - 1)
    assert [st.record for st in at] == [st.record for st in base]
    flipped = [i for i, (x, y) in enumerate(zip(below, base)) if x.record != y.record]
    assert flipped == who
    r = below[who[0]].record
    assert r[0] & OVER_BUDGET and not r[0] & BLUNT_END and r[6] == 0 and r[7] == base[who[0]].record[7] and r[1:6] == base[who[0]].record[1:6]


def test_the_other_worlds_reach_their_branches():
    for w in (world_143(), world_hashes()):
        got = dict(zip(w.names, w.want(3, 2)))
        assert {st.record[1] for st in got.values()} == {0, 1, 2, 3, 4}
        assert {st.record[6] for st in got.values()} == {0, 1, 2, 3, 4, 5, 6}
        assert "bridged_by_the_forward_scan" in got["snv-bridged"].tags and "walk_hits_the_bound" in got["chimera-long"].tags
        assert w.largest_visit_count(3, 2) < DEFAULT_VISITS // 4
