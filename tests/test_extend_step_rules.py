"""GraphUtils.extendRightSE / extendLeftSE (R/util/GraphUtils.java:6018-6204) and the loop on top of them, extendSE (:6454-6565), restated line by
line in Python — with countKmerPairsSE / countKmerPairsReversedSE (:5718-5790), naiveExtend{Right,Left}NoBackChecks (:6888-6933, :7067-7112),
getMedianKmerCoverage(Collection) (:229-247), getMinimumKmerCoverage (:133-145) and hasDuplicatedKmerPair (:6416-6452) — over a graph that
answers three questions: counts(seq) (getKmers' counts), neighbors(kmer, direction) (the counts of the four successors / predecessors in the
order A C G T) and lookup_read_pair(left_kmer, right_kmer).  Float arithmetic goes through numpy.float32.  Hand-worked cases run on a
dict-backed toy graph; then the worlds of tests/test_gpu_extend_step.py are built on the CPU oracle alone and every branch the device test
relies on is shown to be reached, in both directions.  No device is needed here."""
import numpy as np
import pytest

F32 = np.float32
ACGT = b"ACGT"
NONE, SINGLE, FIRST, SECOND = range(4)
WHY_FOUND, WHY_NO_CANDIDATE, WHY_NO_SUPPORT, WHY_INVALID_SEED, WHY_SHORT = range(5)


def neighbor(kmer, b, direction):
    return kmer[1:] + ACGT[b:b + 1] if direction == 0 else ACGT[b:b + 1] + kmer[:-1]


def naive_extend_no_back_checks(g, kmer, direction, bound, min_cov, tags=None):
    """:6888-6933 / :7067-7112 -> [(k-mer, count, base)].  hasDepthRight / hasDepthLeft always answer true (R/graph/Kmer.java:407-486), so
    two neighbours at or above the floor end the walk."""
    result, ext, cur = [], 0, kmer
    while True:
        c4 = g.neighbors(cur, direction)
        nb = [b for b in range(4) if F32(c4[b]) >= F32(min_cov)]
        if len(nb) != 1:                                                  # :6897 no neighbour, :6911-6914 too many good branches
            break
        best = neighbor(cur, nb[0], direction)
        if best == kmer or (result and best == result[-1][0]):            # :6919
            if tags is not None:
                tags.add("walk_repeat")
            break
        result.append((best, F32(c4[nb[0]]), nb[0]))
        ext += 1
        if ext > bound:                                                   # :6925
            break
        cur = best
    return result


def count_pairs(g, kmers, ext, d, direction, gap=0):
    """countKmerPairsSE (:5718-5753) / countKmerPairsReversedSE (:5755-5790): kmers is the sequence's list (reversed for the left-hand
    direction), ext the extension's k-mers in walking order"""
    n = len(kmers)
    max_idx = min(d - 1 - gap, len(ext) - 1)
    pi = n - d + gap
    pairs, last = 0, -1
    for i in range(max_idx + 1):
        if 0 <= pi < n:
            left, right = (kmers[pi], ext[i]) if direction == 0 else (ext[i], kmers[pi])
            if g.lookup_read_pair(left, right):
                pairs += 1
                last = i
        pi += 1
        if pi >= n:
            break
    return pairs, last


def median_cov(counts):
    """getMedianKmerCoverage(Collection) :229-247"""
    c = np.sort(np.asarray(counts, F32))
    n = len(c)
    if n % 2 == 0:
        return F32(F32(c[n // 2] + c[n // 2 - 1]) / F32(2.0))
    return F32(c[n // 2])


class Step:
    """what one extendRightSE / extendLeftSE returns (ext: [(k-mer, count, base)] or None) and the fields of rb_extend_rec"""

    def __init__(self, outcome, why, n_cand=0, ext=None, pairs=0, last=-1, winner=-1, score=0.0, tags=()):
        self.outcome, self.why, self.n_cand, self.ext, self.pairs, self.last, self.winner, self.score = outcome, why, n_cand, ext, pairs, last, winner, F32(score)
        self.tags = set(tags)

    @property
    def out_len(self):
        return len(self.ext) if self.ext else 0

    @property
    def bases(self):
        return bytes(ACGT[b] for _, _, b in self.ext) if self.ext else b""

    @property
    def counts(self):
        return [c for _, c, _ in self.ext] if self.ext else []

    def record(self):
        return (self.outcome, self.why, self.n_cand, self.out_len, self.pairs, self.last, self.winner)


def is_acgtu(kmer):
    return all(ch in b"ACGTUacgtu" for ch in kmer)


def extend_step(g, seq, direction, min_cov, d, k):
    """extendRightSE (direction 0, :6018-6110) / extendLeftSE (1, :6112-6204) of getKmers(seq); for the left-hand direction the list is
    reversed here, as the reference's callers reverse it"""
    n = len(seq) - k + 1
    if n < 1:
        return Step(NONE, WHY_SHORT)
    kmers = [seq[i:i + k] for i in range(n)]
    cnts = [F32(c) for c in g.counts(seq)]
    if direction:
        kmers.reverse(); cnts.reverse()
    tags = set()
    if n < d:
        tags.add("shorter_than_d")
    if n == 1:
        tags.add("one_kmer")
    last_kmer = kmers[-1]
    if not is_acgtu(last_kmer):
        return Step(NONE, WHY_INVALID_SEED, tags=tags)
    c4 = g.neighbors(last_kmer, direction)
    cands = [b for b in range(4) if F32(c4[b]) >= F32(1.0)]              # Kmer.getSuccessors(k, numHash, graph): count > 0
    if not cands:
        return Step(NONE, WHY_NO_CANDIDATE, tags=tags)                    # (bestExtension stays null)
    max_ext = d - 2
    walk = lambda km, bound: naive_extend_no_back_checks(g, km, direction, bound, min_cov, tags)
    if len(cands) == 1:                                                   # :6030-6035
        b = cands[0]
        c = neighbor(last_kmer, b, direction)
        return Step(SINGLE, WHY_FOUND, 1, [(c, F32(c4[b]), b)] + walk(c, max_ext), winner=b, tags=tags)
    path_min = min(cnts[max(n - d, 0):n])                                 # getMinimumKmerCoverage :133-145
    best_score, best_cov, best = F32(0), F32(0), None
    for b in cands:
        c = neighbor(last_kmer, b, direction)
        e = [(c, F32(c4[b]), b)] + walk(c, max_ext)
        pairs, last = count_pairs(g, kmers, [x[0] for x in e], d, direction)
        if last >= 0 and pairs > 0:
            cov = median_cov([x[1] for x in e])
            score = F32(F32(min(path_min, cov) * F32(pairs)) / F32(last + 1))
            if score > best_score or (score == best_score and cov > best_cov):
                if score == best_score and best is not None:
                    tags.add("tie_by_cov")
                best_score, best_cov = score, cov
                best = (FIRST, e[:last + 1], pairs, last, b, len(e))
        else:
            gap = len(e)
            if gap >= d - 1 and pairs == 0:
                tags.add("second_level_skipped")
                continue
            c4n = g.neighbors(e[-1][0], direction)
            for b2 in [x for x in range(4) if F32(c4n[x]) >= F32(1.0)]:
                nc = neighbor(e[-1][0], b2, direction)
                ne = e + [(nc, F32(c4n[b2]), b2)] + walk(nc, d - gap)
                pairs, last = count_pairs(g, kmers, [x[0] for x in ne], d, direction)
                if last >= 0 and pairs > 0:
                    cov = median_cov([x[1] for x in ne])
                    score = F32(F32(min(path_min, cov) * F32(pairs)) / F32(last + 1))
                    if score > best_score or (score == best_score and cov > best_cov):
                        if score == best_score and best is not None:
                            tags.add("tie_by_cov")
                        best_score, best_cov = score, cov
                        best = (SECOND, ne[:last + 1], pairs, last, b | (b2 << 4), len(ne))
    if best is None:
        return Step(NONE, WHY_NO_SUPPORT, len(cands), tags=tags)
    tags.add("trimmed" if len(best[1]) < best[5] else "untrimmed")
    return Step(best[0], WHY_FOUND, len(cands), best[1], best[2], best[3], best[4], best_score, tags)


def has_duplicated_kmer_pair(kmers, cursor, d, mate_index):
    """:6416-6452"""
    if mate_index >= 0:
        mate = kmers[mate_index]
        idx = [i for i, km in enumerate(kmers) if km == cursor]
        if idx:
            c2 = idx[-1]
            m2 = c2 - d
            if m2 >= 0:
                if mate == kmers[m2]:
                    return True
                c1 = idx[0]
                if c1 != c2:
                    m1 = c1 - d
                    if m1 >= 0 and mate == kmers[m1]:
                        return True
                    for i in idx[1:-1]:
                        if i - d >= 0 and mate == kmers[i - d]:
                            return True
    return False


def extend_se(g, seq, min_cov, d, k, step=extend_step, trace=None):
    """extendSE (:6454-6565) of getKmers(seq): (extended sequence, [leftExtLen, leftExtLen + origLen]).  Counts of the k-mers the
    extension added are the counts the step returned with them, as in the reference's list."""
    n0 = len(seq) - k + 1
    kmers = [seq[i:i + k] for i in range(n0)]
    cnts = [F32(c) for c in g.counts(seq)]
    used = set(kmers)
    text = seq
    left_len = 0
    for direction in (1, 0):
        if direction == 1:
            kmers.reverse(); cnts.reverse()
        while True:
            thr = min(cnts[max(0, len(kmers) - d):])
            drops = 0
            while True:
                thr = max(F32(min_cov), F32(thr * F32(0.1)))
                st = step(g, text, direction, thr, d, k)
                e = st.ext
                if e or thr == F32(min_cov):
                    break
                drops += 1
            if not e:
                break
            if trace is not None and drops >= 2:
                trace.add("floor_fell_twice")
            is_used = all(km in used for km, _, _ in e)
            end_index = max(0, len(kmers) - d + len(e))
            i = len(kmers) - 1
            while i >= end_index and is_used:
                is_used = kmers[i] in used
                i -= 1
            if is_used and (len(kmers) < d or has_duplicated_kmer_pair(kmers, e[-1][0], d, len(kmers) - 1 - d + len(e))):
                if trace is not None:
                    trace.add("stopped_by_used")
                break
            kmers += [km for km, _, _ in e]
            cnts += [c for _, c, _ in e]
            used.update(km for km, _, _ in e)
            add = bytes(ACGT[b] for _, _, b in e)
            text = add[::-1] + text if direction == 1 else text + add
        if direction == 1:
            left_len = len(kmers) - n0
            kmers.reverse(); cnts.reverse()
    return text, [left_len, left_len + n0]


# ---- a toy graph: k-mers with counts, read pairs as a set ----
class Toy:
    def __init__(self, k, reads, mult=None):
        self.k, self.cnt, self.pairs, self.d = k, {}, set(), None
        self.reads, self.mult = reads, mult or [1] * len(reads)

    def build(self, d):
        self.d = d
        for r, m in zip(self.reads, self.mult):
            km = [r[i:i + self.k] for i in range(len(r) - self.k + 1)]
            for x in km:
                self.cnt[x] = self.cnt.get(x, 0) + m
            for i in range(len(km) - d):
                self.pairs.add((km[i], km[i + d]))
        return self

    def counts(self, seq):
        return [F32(self.cnt.get(seq[i:i + self.k], 0)) if is_acgtu(seq[i:i + self.k]) else F32(0) for i in range(len(seq) - self.k + 1)]

    def neighbors(self, kmer, direction):
        return [F32(self.cnt.get(neighbor(kmer, b, direction), 0)) for b in range(4)]

    def lookup_read_pair(self, left, right):
        return (left, right) in self.pairs


#        0         1         2
#        0123456789012345678901234
T_A = b"ACGTTGCAAGCTTAGGATCCATTGA"          # prefix ACGTTGCAAGC (11), then branch A
T_B = b"ACGTTGCAAGCGGCTAATCGTACCG"          # the same prefix, branch B


def test_hand_worked_fork_is_decided_by_pairs_then_coverage():
    k, d = 4, 3
    g = Toy(k, [T_A, T_B], [1, 3]).build(d)
    # the sequence ends at the fork: its last k-mer AAGC has successors AGCT (count 1) and AGCG (count 3)
    st = extend_step(g, b"ACGTTGCAAGC", 0, 1.0, d, k)
    # both branches are walked d - 2 + 1 = 2 steps: AGCT GCTT CTTA / AGCG GCGG CGGC; k-mers i = 0, 1, 2 pair with the sequence's k-mers 5, 6, 7
    # (GCAA, CAAG, AAGC), which reads of both transcripts hold: 3 pairs each, last = 2.  pathMinCov = 4 (shared prefix), medians 1 and 3:
    # scores min(4, 1) * 3 / 3 = 1 and min(4, 3) * 3 / 3 = 3 -> branch B (base G = 2), untrimmed
    assert st.record() == (FIRST, WHY_FOUND, 2, 3, 3, 2, 2) and st.score == F32(3.0) and st.bases == b"GGC" and "untrimmed" in st.tags
    # the mirror image: the reversed transcripts fork to the left
    gl = Toy(k, [T_A[::-1], T_B[::-1]], [1, 3]).build(d)
    sl = extend_step(gl, b"ACGTTGCAAGC"[::-1], 1, 1.0, d, k)
    assert sl.record() == st.record() and sl.score == st.score and sl.bases == b"GGC"
    # a floor of 2 stops branch A's walk at once (its k-mers count 1): the candidate alone, one pair of one -> score 1; B is unchanged
    st2 = extend_step(g, b"ACGTTGCAAGC", 0, 2.0, d, k)
    assert st2.record() == st.record()
    # one k-mer of sequence: only i = d - 1 = 2 has a partner (index 1 - 3 + 2 = 0): one pair, last = 2 -> score min(4, 3) * 1 / 3 = 1
    st3 = extend_step(g, b"AAGC", 0, 1.0, d, k)
    assert st3.record() == (FIRST, WHY_FOUND, 2, 3, 1, 2, 2) and st3.score == F32(F32(3.0) / F32(3.0)) and {"one_kmer", "shorter_than_d"} <= st3.tags


def test_hand_worked_single_dead_end_invalid_and_short():
    k, d = 4, 3
    g = Toy(k, [T_A, T_B], [1, 3]).build(d)
    # mid-prefix: TTGC has one successor, TGCA, followed d - 2 + 1 = 2 steps (GCAA, CAAG), unscored
    st = extend_step(g, b"ACGTTGC", 0, 1.0, d, k)
    assert st.record() == (SINGLE, WHY_FOUND, 1, 3, 0, -1, 0) and st.bases == b"AAG"
    # the walk meets the fork after one step: candidate CAAG + AAGC, whose successors are two
    assert extend_step(g, b"ACGTTGCAA", 0, 1.0, d, k).bases == b"GC"
    # CGTT's only successor GTTG has two of its own (TTGC, and TTGA at branch A's end): the candidate alone
    assert extend_step(g, b"ACGTT", 0, 1.0, d, k).record() == (SINGLE, WHY_FOUND, 1, 1, 0, -1, 2)
    assert extend_step(g, T_A, 0, 1.0, d, k).record() == (NONE, WHY_NO_CANDIDATE, 0, 0, 0, -1, -1)
    assert extend_step(g, b"ACGTTGCANGC", 0, 1.0, d, k).record() == (NONE, WHY_INVALID_SEED, 0, 0, 0, -1, -1)
    assert extend_step(g, b"ACG", 0, 1.0, d, k).record() == (NONE, WHY_SHORT, 0, 0, 0, -1, -1)


def test_hand_worked_walk_stops_when_it_meets_its_start_again():
    k, d = 4, 12
    unit = b"ACGGT"
    g = Toy(k, [b"TTCA" + unit * 6]).build(d)
    tags = set()
    # from ACGG round the period-5 circle: CGGT GGTA GTAC TACG, then ACGG again — the start k-mer, not added (:6919)
    w = naive_extend_no_back_checks(g, b"ACGG", 0, 50, 1.0, tags)
    assert [x[0] for x in w] == [b"CGGT", b"GGTA", b"GTAC", b"TACG"] and tags == {"walk_repeat"}
    # a homopolymer's only successor is itself
    g2 = Toy(k, [b"CCAAAAAAAA"]).build(3)
    assert naive_extend_no_back_checks(g2, b"AAAA", 0, 50, 1.0) == []


def test_hand_worked_second_level():
    k, d = 4, 6
    # three transcripts P + TTAGG..., P + GTACC..., P + GTCAG...: the fork behind P = ...CAAGC has candidates AGCG (G) and AGCT (T)
    p = b"ACGTTGCAAGC"
    reads = [p + b"TTAGGATCCATTGACC", p + b"GTACCATGTGAGTT", p + b"GTCAGGTTCTACAA"]
    g = Toy(k, reads).build(d)
    # two k-mers of sequence (CAAG, AAGC): extension k-mers i = 4, 5 have partners 0, 1, smaller i have none.
    # G: AGCG GCGT, then GCGT has successors CGTA and CGTC: a first stretch of gap 2 without a partner -> one branch further, bound 4.
    #   (G, A): + CGTA GTAC, and GTAC has two successors (TACC; TACA from the third read's end): 4 k-mers, none with a partner.
    #   (G, C): + CGTC GTCA TCAG CAGG, and CAGG has two successors (AGGT; AGGA from the first read): 6 k-mers; TCAG pairs with CAAG and
    #           CAGG with AAGC in the third read: 2 pairs, last 5; counts 2 2 1 1 1 1, median 1; pathMinCov 3: score 1 * 2 / 6.
    # T: AGCT GCTT CTTA TTAG TAGG, and TAGG has two successors (AGGA, AGGT): 5 k-mers; TAGG pairs with CAAG: 1 pair, last 4: 1 * 1 / 5.
    st = extend_step(g, b"CAAGC", 0, 1.0, d, k)
    assert st.record() == (SECOND, WHY_FOUND, 2, 6, 2, 5, 2 | (1 << 4)) and st.bases == b"GTCAGG"
    assert st.score == F32(F32(1.0) * F32(2.0) / F32(6.0)) and {"untrimmed", "shorter_than_d"} <= st.tags
    assert count_pairs(g, [b"CAAG", b"AAGC"], [x[0] for x in st.ext], d, 0) == (2, 5)


def test_median_and_min_are_the_reference_s():
    assert median_cov([3, 1, 2]) == F32(2) and median_cov([4, 1, 3, 2]) == F32(2.5) and median_cov([7]) == F32(7)
    assert median_cov([1, 2]) == F32(1.5)


def test_has_duplicated_kmer_pair():
    km = [b"A", b"B", b"C", b"A", b"B", b"C", b"A"]
    assert has_duplicated_kmer_pair(km, b"C", 2, 3)                  # mate A at 3; the last C is at 5, its mate 3 is A
    assert not has_duplicated_kmer_pair(km, b"C", 2, 1)              # mate B: C's mates are A
    assert not has_duplicated_kmer_pair(km, b"Z", 2, 3) and not has_duplicated_kmer_pair(km, b"C", 2, -1)
    # neither the last C (8: its mate 6 is Q) nor the first (2: A) has the mate B, the one in between (5: its mate 3 is B) does
    assert has_duplicated_kmer_pair([b"A", b"X", b"C", b"B", b"Y", b"C", b"Q", b"R", b"C"], b"C", 2, 3)
    assert not has_duplicated_kmer_pair([b"A", b"X", b"C", b"B", b"Y", b"Z", b"Q", b"R", b"C"], b"C", 2, 3)
    assert has_duplicated_kmer_pair([b"A", b"X", b"C", b"B", b"B", b"C", b"B", b"R", b"C"], b"C", 1, 4)      # the middle C (5) follows B (4)


def test_extend_se_on_the_toy_graph():
    k, d = 4, 3
    g = Toy(k, [T_A, T_B], [1, 3]).build(d)
    # from the middle of the prefix: to the left up to the transcript's start, to the right through the fork along B to its end
    text, rng = extend_se(g, b"TTGCAA", 1.0, d, k)
    assert text == T_B and rng == [3, 6]
    trace = set()
    unit = b"ACGGTCA"
    circ = Toy(k, [unit * 8]).build(d)
    text, rng = extend_se(circ, (unit * 3)[:10], 1.0, d, k, trace=trace)
    assert "stopped_by_used" in trace and rng[1] - rng[0] == 7


# ---- the worlds of the device test, on the CPU oracle ----
class OracleSide:
    """the three questions on oracle.rbo.Graph, memoised per k-mer"""

    def __init__(self, og):
        from oracle import rbo
        self.rbo, self.og, self.k = rbo, og, og.k
        self.mode = rbo.FWD if og.stranded else rbo.CANON
        self._c, self._p = {}, {}

    def counts(self, seq):
        return self.og.get_kmers(seq)[2]

    def _count(self, kmer):
        c = self._c.get(kmer)
        if c is None:
            c = self._c[kmer] = F32(self.og.get_kmers(kmer)[2][0])
        return c

    def neighbors(self, kmer, direction):
        return [self._count(neighbor(kmer, b, direction)) for b in range(4)]

    def lookup_read_pair(self, left, right):
        hit = self._p.get((left, right))
        if hit is None:                                       # two k-mers side by side are a pair at distance k
            p, _, _ = self.rbo.hash_pairs_region(left + right, self.k, self.og.pk_h, self.k, self.mode)
            hit = self._p[(left, right)] = self.og.lookup_read_pair(p[0])
        return hit


def put(s, pos, ch):
    b = bytearray(s); b[pos] = ord(ch); return bytes(b)


class World:
    """Transcripts tiled with reads (every k-mer counts about 8 times its transcript's multiplicity) and the sequences to extend.  Everything
    is made for the right-hand direction and mirrored: the reversed transcripts are inserted too and the reversed queries go left."""
    FLOORS = (1.0, 2.0, 5.0, 1.0e6)
    SIZES = (4_800_011, 4_800_011, 4_800_017)
    # the lengths that do not follow from k by themselves (letters, or repeats of a unit), as the worlds at k = 25 have them; tests/pair_worlds.py
    # derives them from k: flanks of the tandem repeats and homopolymers, the tandem units, how often they repeat in the transcript, in the
    # `tandem` query and in the text the `circle` query is cut from, the homopolymer run inside a transcript, the transcript that is nothing else
    # and the run the `poly` query ends in, how far `mid` reaches behind the fork, the long transcript and its query
    LENGTHS = dict(flank=100, units=(14, 20), unit_reps=12, tandem_query_reps=2, circle_reps=4, poly_run=60, poly_tx=120, poly_query=30, mid=100,
                   long_tx=3000, long_query=2900)

    def __init__(self, k, stranded, seed, d=30, n_iso=6, read_len=100, tile=10, tx_len=500, hashes=(2, 2, 2), sizes=None, lengths=None, extra_tx=()):
        """extra_tx: (transcript, multiplicity, [(kind, query)]) behind the world's own, tiled and mirrored as they are"""
        from oracle import rbo
        rng = np.random.default_rng(seed)
        self.k, self.stranded, self.d, self.hashes = k, stranded, d, hashes
        self.lengths = ln = dict(self.LENGTHS, **(lengths or {}))
        rnd = lambda n: np.frombuffer(ACGT, np.uint8)[rng.integers(0, 4, n)].tobytes()
        half = tx_len // 2
        tx, q = [], []                                        # (transcript, multiplicity), (kind, sequence)
        ends = (0, 1, d - 1, d, d + 5)
        for i in range(n_iso):                                # isoform pairs: a shared prefix, coverage 1:1, 1:3, 1:10 either way
            p, a, b = rnd(half), rnd(half), rnd(half)
            ma, mb = ((1, 1), (3, 1), (1, 3), (10, 1), (1, 10), (1, 1))[i % 6]
            tx += [(p + a, ma), (p + b, mb)]
            for e in ends:
                q.append(("fork-%d" % e, p[:half - e]))
                q.append(("fork-short-%d" % e, p[half - e - k - 6:half - e]))                 # 7 k-mers: shorter than d
            q.append(("fork-one-kmer", p[half - k:]))
            q.append(("fork-n-back", put(p, half - k - 4, "N")))                              # an N inside the last d k-mers
            q.append(("fork-n-seed", put(p, half - 3, "N")))                                  # ... inside the last k-mer
            q.append(("mid", (p + a)[:half + ln["mid"]]))
            q.append(("dead-end", p + a))
        for i in range(n_iso):                                # a second fork g k-mers after the first
            g2 = max(1, (5, 20, d - 3, d - 2, d - 1, 12)[i % 6])
            p, a, bb, c1, c2 = rnd(half), rnd(half), rnd(g2), rnd(half - g2), rnd(half - g2)
            m1, m2 = ((1, 1), (3, 1), (1, 3))[i % 3]
            tx += [(p + a, 1), (p + bb + c1, m1), (p + bb + c2, m2)]
            q.append(("fork2", p))
            q.append(("fork2-short", p[half - k - 4:]))                                      # 5 k-mers: the first stretch has no partner
            q.append(("fork2-one-kmer", p[half - k:]))
            q.append(("fork2-n-back", put(p, half - k - 9, "N")))
        for i in range(n_iso):                                # two transcripts that share k - 1 letters only, and a third that ends on them
            p1, s1, p2, s2, p3 = rnd(half), rnd(half), rnd(half - k + 1), rnd(half), rnd(half - k + 1)
            j = p1[half - k + 1:]
            tx += [(p1 + s1, 1), (p2 + j + s2, 1 + i % 3), (p3 + j, 1)]
            q += [("junction-1", p1), ("junction-2", p2 + j), ("junction-3", p3 + j)]
        for i in range(2):                                    # a tandem repeat whose period is below d k-mers, and a homopolymer
            w, z, unit = rnd(ln["flank"]), rnd(ln["flank"]), rnd(ln["units"][i])
            tx += [(w + unit * ln["unit_reps"] + z, 1), (unit[::-1] * ln["unit_reps"], 1)]             # ... and one that is nothing else: every k-mer has one successor
            q += [("tandem", w + unit * ln["tandem_query_reps"]), ("circle", (unit[::-1] * ln["circle_reps"])[3:3 + k + 8])]
            w, z = rnd(ln["flank"]), rnd(ln["flank"])
            tx += [(w + b"A" * ln["poly_run"] + z, 1), (b"C" * ln["poly_tx"], 1)]
            q += [("poly", w + b"A" * ln["poly_query"]), ("poly-in", b"A" * (k + 3)), ("poly-only", b"C" * (k + 3))]
        self.hot = []
        for i in range(2):                                    # a fork behind 100 letters that are covered 150 times more: extendSE's floor falls twice
            p, a, b = rnd(half), rnd(half), rnd(half)
            tx += [(p + a, 1), (p + b, 1), (p[half - read_len:], 150)]
            self.hot.append(p[half - k - 4:])
        big = rnd(ln["long_tx"])
        tx.append((big, 1))
        q.append(("long", big[:ln["long_query"]]))
        q += [("too-short", tx[0][0][:k - 1]), ("empty", b"")]
        for t, m, qs in extra_tx:
            tx.append((t, m))
            q += list(qs)
        self.tx = tx
        self.queries = [(kind, s, 0) for kind, s in q] + [(kind, s[::-1], 1) for kind, s in q]
        self.floors = [self.FLOORS[i % 4] if kind.startswith(("fork", "junction")) and i % 3 == 0 else 1.0 for i, (kind, _, _) in enumerate(self.queries)]
        reads = []
        for t, m in tx:
            for tt in (t, t[::-1]):
                starts = list(range(0, max(len(tt) - read_len, 0) + 1, tile))
                if starts[-1] < len(tt) - read_len:
                    starts.append(len(tt) - read_len)
                reads += [tt[a:a + read_len] for a in starts] * m
        self.reads = reads
        self.sizes = tuple(sizes or self.SIZES)
        self.og = rbo.Graph(*self.sizes, *hashes, k, stranded, True, 5)
        self.og.set_read_pair_distance(d)
        self.packed = rbo.pack_reads(reads, [b"I" * len(s) for s in reads])
        self.og.add_reads(*self.packed, 3, rbo.STORE_READ_PAIRS)
        self.o = OracleSide(self.og)
        self._want = None

    def want(self):
        """the restatement's steps for the queries with their floors, computed once"""
        if self._want is None:
            self._want = [extend_step(self.o, s, direction, fl, self.d, self.k) for (_, s, direction), fl in zip(self.queries, self.floors)]
        return self._want

    def assert_every_branch_is_reached(self):
        for direction in (0, 1):
            steps = [st for st, (_, _, dd) in zip(self.want(), self.queries) if dd == direction]
            assert {st.outcome for st in steps} == {NONE, SINGLE, FIRST, SECOND}, direction
            assert {st.why for st in steps} == {WHY_FOUND, WHY_NO_CANDIDATE, WHY_NO_SUPPORT, WHY_INVALID_SEED, WHY_SHORT}, direction
            tags = set().union(*(st.tags for st in steps))
            need = {"tie_by_cov", "second_level_skipped", "trimmed", "untrimmed", "walk_repeat", "shorter_than_d", "one_kmer"}
            assert need <= tags, (direction, need - tags)


WORLDS = {}


def world(k, stranded):
    if (k, stranded) not in WORLDS:
        WORLDS[(k, stranded)] = World(k, stranded, seed=300 + stranded)
    return WORLDS[(k, stranded)]


@pytest.mark.parametrize("stranded", [False, True])
def test_worlds_reach_every_branch_on_the_oracle(stranded):
    world(25, stranded).assert_every_branch_is_reached()


# ---- the host loop of the package (rnabloom.graphutils.extendSE) without a device: its graph is a stand-in whose step is the restatement ----
class StepStandIn:
    """what graphutils.extendSE asks of a graph — the distance, k, getKmers' counts and the batched step — answered over a Toy / OracleSide"""

    def __init__(self, g, k, d):
        self.g, self.k, self.d, self.calls, self.most = g, k, d, 0, 0

    def getReadPairedKmerDistance(self):
        return self.d

    def getKmers(self, reads):
        ko, c = [0], []
        for r in reads:
            cc = list(self.g.counts(r)) if len(r) >= self.k else []
            c += cc
            ko.append(ko[-1] + len(cc))
        return np.array(ko, np.int64), None, None, np.array(c, F32)

    def extendStepSE(self, seqs, direction, floors):
        self.calls += 1
        self.most = max(self.most, len(seqs))
        steps = [extend_step(self.g, s, direction, fl, self.d, self.k) for s, fl in zip(seqs, floors)]
        return [st.bases if st.outcome != NONE else None for st in steps], None


def test_the_package_s_loop_equals_the_restated_loop_on_the_toy_graph():
    from rnabloom import graphutils
    k, d = 4, 3
    g = Toy(k, [T_A, T_B], [1, 3]).build(d)
    seeds = [t[a:a + n] for t in (T_A, T_B) for n in (4, 5, 6, 9) for a in range(0, len(t) - n + 1, 2)] + [b"ACG", b""]
    unit = b"ACGGTCA"
    circ = Toy(k, [unit * 8]).build(d)
    for graph, batch in ((g, seeds), (circ, [(unit * 3)[:10], (unit * 3)[2:9], unit[:4]])):
        dev = StepStandIn(graph, k, d)
        texts, ranges = graphutils.extendSE(dev, batch, 1.0)
        for s, t, r in zip(batch, texts, ranges):
            want = extend_se(graph, s, 1.0, d, k) if len(s) >= k else (s, [0, 0])
            assert (t, r) == want, (s, t, r, want)
        assert dev.most == sum(len(s) >= k for s in batch) and dev.calls < 4 * 30      # one call a round holds every sequence still growing
    with pytest.raises(RuntimeError):
        graphutils.extendSE(StepStandIn(g, k, d), [b"TTGCAA"], 1.0, max_rounds=1)


def driver_seeds(w):
    """200 sequences for extendSE: behind the stretches covered 150 times more, inside the circular tandem repeats, before forks and junctions,
    and random pieces of the transcripts"""
    rng = np.random.default_rng(9)
    seeds = list(w.hot) + [s[::-1] for s in w.hot]
    seeds += [s if dd == 0 else s[::-1] for kind, s, dd in w.queries if kind in ("circle", "poly-only", "tandem", "fork2-short", "junction-2")]
    while len(seeds) < 200:
        t = w.tx[int(rng.integers(0, len(w.tx)))][0]
        a = int(rng.integers(0, max(1, len(t) - 80)))
        seeds.append(t[a:a + int(rng.integers(w.k, 80))])
    return [s for s in seeds if len(s) >= w.k and is_acgtu(s)][:200]


@pytest.mark.parametrize("stranded", [False, True])
def test_the_package_s_loop_equals_the_restated_loop_on_the_oracle(stranded):
    """the seeds that end the loop by usedKmers + hasDuplicatedKmerPair and the ones whose floor falls twice, as in the device test"""
    from rnabloom import graphutils
    w = world(25, stranded)
    seeds = driver_seeds(w)
    trace = set()
    want = [extend_se(w.o, s, 1.0, w.d, w.k, trace=trace) for s in seeds]
    assert {"stopped_by_used", "floor_fell_twice"} <= trace, trace
    texts, ranges = graphutils.extendSE(StepStandIn(w.o, w.k, w.d), seeds, 1.0)
    assert list(zip(texts, ranges)) == want


def test_the_package_s_duplicated_pair_test_equals_the_restated_one():
    from rnabloom.graphutils import _has_duplicated_kmer_pair
    rng = np.random.default_rng(4)
    seen = set()
    for _ in range(4000):
        n = int(rng.integers(1, 10))
        km = [bytes([65 + int(x)]) for x in rng.integers(0, 3, n)]
        cursor, d, mate = bytes([65 + int(rng.integers(0, 4))]), int(rng.integers(1, 4)), int(rng.integers(-2, n))
        a = has_duplicated_kmer_pair(km, cursor, d, mate)
        assert _has_duplicated_kmer_pair(km, cursor, d, mate) == a, (km, cursor, d, mate)
        seen.add(a)
    assert seen == {True, False}
