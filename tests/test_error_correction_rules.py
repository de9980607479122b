"""The rules of rb_graph_correct_errors restated in Python from the reference's Java, and checked on hand-worked cases over a dictionary
graph.  tests/test_gpu_error_correction.py applies the same restatement to the CPU oracle's filters.

  GraphUtils.correctErrorHelper (R/util/GraphUtils.java:3711-3912): the gap scan :3730-3855, the left edge :3736-3781, the SNV bubble
  :3782-3818, the path :3819-3845, the right edge :3857-3902, correctMismatches :3904 (tests/test_mismatch_rules.py);
  getMaxCoveragePath :1591-1675, greedyExtendLeft / Right :1906-1921 / :1961-1976 with greedyExtend*Once :501-592 and
  getMaxMedianCoverage* :248-438; Kmer.getLeftVariants / getRightVariants (R/graph/Kmer.java:361-405), hasPredecessors / hasSuccessors
  :97-125; SeqUtils.getPercentIdentity / getDistance (R/util/SeqUtils.java:164-229), isLowComplexityShort :499-543.
The graph is an object with: counts(sequence) -> getKmers' counts; contains(k-mer); variants(sequence, j, side) -> the counts of the four
k-mers that have A C G T in place of the first (side 'L') or last ('R') base of k-mer j; has_neighbors(sequence, j, direction) ->
graph.contains of any successor (0) / predecessor (1) of k-mer j; max_cov_path(left, right, bound, min_cov) -> k-mers or None;
greedy(source, direction, lookahead, bound) -> (appended bases in walk order, their counts).  Seeds of walks are good k-mers (letters of
ACGTU only); they are handed over in upper case with U as T, which is how the walk kernels compare k-mers.
The last part of the file checks that the feature exists at every layer."""
import os
import re

import numpy as np
import pytest

from test_mismatch_rules import DictGraph, K, NORM, TRUE, alt_nucleotides, correct_mismatches, median, sub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LEFT_EDGE, RIGHT_EDGE, SNV, PATH = 0, 1, 2, 3
KEPT, REPLACED, TRIMMED = 0, 1, 2
CORRECTED, GAP, MISMATCH = 1, 2, 4
FLOAT_MIN_VALUE = np.float32(1.4e-45)              # Float.MIN_VALUE: the smallest positive float


def distance_literal(s, t):
    """SeqUtils.getDistance(String, String) :190-229, statement by statement — including System.arraycopy(v1, 0, v0, 0, tLen), which
    copies tLen of the tLen + 1 entries: v0[tLen] keeps its first value"""
    if s == t:
        return 0
    if len(s) == 0:
        return len(t)
    if len(t) == 0:
        return len(s)
    n = len(t)
    v0 = list(range(n + 1))
    v1 = [0] * (n + 1)
    for i in range(len(s)):
        v1[0] = i + 1
        for j in range(n):
            v1[j + 1] = min(v1[j] + 1, v0[j + 1] + 1, v0[j] + (0 if s[i] == t[j] else 1))
        v0[:n] = v1[:n]
    return v1[n]


def distance(s, t):
    """the same number from the true Levenshtein matrix D: every column but the last is D's, so the result is
    min(D[|s|][|t|-1] + 1, |t| + 1, D[|s|-1][|t|-1] + (s[-1] != t[-1])).  Rows as prefix minima (what the device does)."""
    if s == t:
        return 0
    if len(s) == 0:
        return len(t)
    if len(t) == 0:
        return len(s)
    n = len(t)
    ta = np.frombuffer(bytes(t[:-1]), np.uint8)
    j = np.arange(n)
    row = j.copy()
    prev_last = last = n - 1
    for i, ch in enumerate(bytes(s), 1):
        tmp = np.empty(n, np.int64)
        tmp[0] = i
        tmp[1:] = np.minimum(row[1:] + 1, row[:-1] + (ta != ch))
        row = np.minimum.accumulate(tmp - j) + j
        prev_last, last = last, int(row[n - 1])
    return min(last + 1, n + 1, prev_last + (0 if s[-1] == t[-1] else 1))


def percent_identity(a, b):
    """SeqUtils.getPercentIdentity(String, String) :164-175 in float32"""
    d = distance(a, b)
    m = len(b) if len(a) <= len(b) else len(a)
    return F32(F32(m - d) / F32(m))


def capacity(length, k, max_indel):
    """letters a sequence can have after gap repair (include/rb_capi.h): every interior gap has a good k-mer before the first and behind
    each, a path gap (>= 1 bad k-mer) grows by at most max_indel, an SNV gap (k bad k-mers) by exactly 2, an edge gap never grows"""
    nk = max(0, length - k + 1)
    if nk == 0:
        return length
    return length + ((nk - 1) // 2) * max_indel + ((nk - 1) // (k + 1)) * 2


def gap_scan(c, T):
    """:3730-3855 and :3857: (first bad k-mer, number of bad k-mers) of every gap"""
    gaps, nb, nk = [], 0, len(c)
    for i in range(nk):
        if c[i] >= T:
            if nb > 0:
                gaps.append((i - nb, nb))
            nb = 0
        else:
            nb += 1
    if 0 < nb < nk:
        gaps.append((nk - nb, nb))
    return gaps


def assemble(kmers):
    return kmers[0] + b"".join(km[-1:] for km in kmers[1:])


def correct_errors(seq, k, T, lookahead, max_indel, pid, min_cov, G):
    """correctErrorHelper on the k-mer list of `seq`.  Returns (bytes the reference's kmers2 spells — or seq where it returns null,
    flags, [gap records as dicts])."""
    seq = bytes(seq)
    c = [F32(x) for x in G.counts(seq)]
    nk = len(c)
    T, mincov, pid = F32(T), F32(min_cov), F32(pid)
    norm = lambda b: bytes(b).translate(NORM)
    out, cur, recs = bytearray(), 0, []
    gaps = gap_scan(c, T) if T > 0 else []
    for g, nb in gaps:
        kind = LEFT_EDGE if g == 0 else RIGHT_EDGE if g + nb == nk else SNV if nb == k else PATH
        a = 0 if kind == LEFT_EDGE else g + k - 1                  # the letters the gap's k-mers stand for in the spelled string
        outcome, repl = KEPT, seq[a:a + nb]
        if kind in (LEFT_EDGE, RIGHT_EDGE):
            left = kind == LEFT_EDGE
            j = nb - 1 if left else g                               # the bad k-mer next to the good one
            ch = seq[j] if left else seq[j + k - 1]
            vc = G.variants(seq, j, "L" if left else "R")
            if any(F32(vc[b"ACGT".index(x)]) >= mincov for x in alt_nucleotides(ch)):
                if nb < lookahead:
                    outcome, repl = TRIMMED, b""
                else:
                    tip_med = median(c[g:g + nb])
                    src = norm(seq[nb:nb + k]) if left else norm(seq[g - 1:g - 1 + k])
                    bases, cnts = G.greedy(src, 1 if left else 0, lookahead, nb)
                    if len(bases) == nb and median(cnts) > tip_med:
                        ext = bases[::-1] if left else bases
                        new = ext + src[:k - 1] if left else src[1:] + ext
                        old = seq[0:nb + k - 1] if left else seq[g:g + nb + k - 1]
                        if percent_identity(new, old) >= pid:
                            outcome, repl = REPLACED, ext
                        elif not G.has_neighbors(seq, 0 if left else nk - 1, 1 if left else 0) and nb < k:
                            outcome, repl = TRIMMED, b""
        elif kind == SNV:
            lk, rk = seq[g:g + k], seq[g + k - 1:g + 2 * k - 1]
            best, best_cov = None, FLOAT_MIN_VALUE
            for n in b"ACGT":
                s = lk + bytes([n]) + rk
                cs = [F32(x) for x in G.counts(s)]
                if cs and min(cs) >= mincov and median(cs) > best_cov:
                    best_cov, best = median(cs), s
            if best is not None and best_cov >= mincov:
                outcome, repl = REPLACED, best[k - 1:]              # the last letters of its k + 2 k-mers
        else:
            path = G.max_cov_path(norm(seq[g - 1:g - 1 + k]), norm(seq[g + nb:g + nb + k]), nb + max_indel, mincov)
            if path is not None:
                n = len(path)
                if nb - max_indel <= n <= nb + max_indel and (n <= k + max_indel or percent_identity(assemble(path), seq[g:g + nb + k - 1]) >= pid):
                    outcome, repl = REPLACED, bytes(p[-1] for p in path)
        out += seq[cur:a] + repl
        cur = a + nb
        recs.append(dict(first=g, run=nb, kind=kind, outcome=outcome, repl_len=len(repl)))
    out += seq[cur:]
    out = bytes(out)
    fixed, n_fixed, _ = correct_mismatches(out, G.counts(out), k, T, min_cov, G.contains, G.counts)
    flags = (GAP if any(r["outcome"] != KEPT for r in recs) else 0) | (MISMATCH if n_fixed else 0)
    return fixed, flags | (CORRECTED if flags else 0), recs


# ---- getMaxCoveragePath and greedyExtend over a count(k-mer) callback (the dictionary-graph versions of rbo.get_max_coverage_path / greedy_extend)
def is_low_complexity_short(seq):
    idx = {65: 0, 67: 1, 71: 2, 84: 3}
    jround = lambda x: int(np.floor(F32(x) + F32(0.5)))
    n = len(seq)
    t1, t2, t3 = (min(32767, jround(F32(m) * F32(0.95))) for m in (n, n // 2, n // 3))
    nf1, nf2, nf3 = [0] * 4, [0] * 16, [0] * 64
    c3, c2, c1 = idx[seq[0]], idx[seq[1]], idx[seq[2]]
    for x in (c3, c2, c1): nf1[x] += 1
    nf2[c3 * 4 + c2] += 1; nf2[c2 * 4 + c1] += 1; nf3[c3 * 16 + c2 * 4 + c1] += 1
    for ch in seq[3:]:
        c3, c2, c1 = c2, c1, idx[ch]
        nf1[c1] += 1
        if nf1[c1] >= t1: return True
        nf2[c2 * 4 + c1] += 1
        if nf2[c2 * 4 + c1] >= t2: return True
        nf3[c3 * 16 + c2 * 4 + c1] += 1
        if nf3[c3 * 16 + c2 * 4 + c1] >= t3: return True
    return any(nf1[a] + nf1[b] >= t1 for a in range(4) for b in range(a + 1, 4))


def dict_max_cov_path(count, left, right, bound, min_cov, low_complexity=None):
    low_complexity = low_complexity or is_low_complexity_short
    def step(cur, direction):                                       # Kmer.getMaxCovSuccessor / Predecessor :301-355
        best, best_c = None, -1.0
        for a in b"ACGT":
            nxt = cur[1:] + bytes([a]) if direction == 0 else bytes([a]) + cur[:-1]
            cc = count(nxt)
            if cc >= min_cov and cc > best_c:
                best, best_c = nxt, cc
        return best
    left_set, left_path, best = set(), [], left
    for _ in range(bound):
        best = step(best, 0)
        if best is None: break
        if best == right: return left_path
        if best in left_set: break
        left_set.add(best); left_path.append(best)
    right_set, right_path, best = set(), [], right
    for _ in range(bound):
        best = step(best, 1)
        if best is None: break
        if best == left: return right_path
        if best in right_set: return None
        if best in left_set:
            if low_complexity(best): return None
            right_path.insert(0, best)
            for i in range(len(left_path) - 1, -1, -1):
                if left_path[i] == best:
                    return left_path[:i] + right_path
        else:
            right_set.add(best); right_path.insert(0, best)
    return None


def dict_greedy(count, source, direction, lookahead, bound):
    def neighbours(km):
        out = []
        for a in b"ACGT":
            nxt = km[0][1:] + bytes([a]) if direction == 0 else bytes([a]) + km[0][:-1]
            if count(nxt) >= 1: out.append((nxt, float(count(nxt))))
        return out

    def score(src):                                                 # getMaxMedianCoverageRight / Left :248-310 / :375-438
        nbrs = neighbours(src)
        if not nbrs:
            return 0.0 if lookahead > 0 else src[1]
        path, cursor = [src], nbrs.pop(0)
        path.append(cursor)
        frontier, best = [nbrs], 0.0
        while frontier:
            if len(path) < lookahead:
                nbrs = neighbours(cursor)
                if nbrs:
                    cursor = nbrs.pop(0); path.append(cursor); frontier.append(nbrs)
                    continue
            if len(path) == lookahead:
                best = max(best, min(km[1] for km in path))
            while frontier:
                nbrs = frontier[-1]
                path.pop()
                if not nbrs: frontier.pop()
                else:
                    cursor = nbrs.pop(0); path.append(cursor)
                    break
        return best
    nxt, out, counts = (source, 0.0), bytearray(), []
    for _ in range(bound):
        cands = neighbours(nxt)
        if not cands: break
        best = cands[0]
        if len(cands) > 1:
            best_cov, best = -1.0, None
            for km in cands:
                sc = score(km)
                if sc > best_cov: best, best_cov = km, sc
                elif sc == best_cov and km[1] > best[1]: best = km
        nxt = best
        out += nxt[0][-1:] if direction == 0 else nxt[0][:1]
        counts.append(nxt[1])
    return bytes(out), counts


class EGraph(DictGraph):
    """test_mismatch_rules' dictionary graph (k = 5) with the other callbacks of the restatement"""

    def count1(self, km):
        km = bytes(km)
        return float(self.counts(km)[0])

    def variants(self, seq, j, side):
        km = seq[j:j + K]
        return [self.count1(bytes([a]) + km[1:] if side == "L" else km[:-1] + bytes([a])) for a in b"ACGT"]

    def has_neighbors(self, seq, j, direction):
        km = seq[j:j + K]
        return any(all(ch in b"ACGTUacgtu" for ch in nb) and self.contains(nb)
                   for nb in ((km[1:] + bytes([a]) if direction == 0 else bytes([a]) + km[:-1]) for a in b"ACGT"))

    low_complexity = None            # None: SeqUtils.isLowComplexityShort

    def max_cov_path(self, left, right, bound, min_cov):
        return dict_max_cov_path(self.count1, left, right, bound, float(min_cov), self.low_complexity)

    def greedy(self, source, direction, lookahead, bound):
        return dict_greedy(self.count1, source, direction, lookahead, bound)

    def run(self, seq, T=5.0, lookahead=2, max_indel=1, pid=0.8, mincov=1.0):
        return correct_errors(seq, K, T, lookahead, max_indel, pid, mincov, self)


def kinds(recs):
    return [(r["kind"], r["outcome"]) for r in recs]


HEAD, TAIL = TRUE[:20], TRUE[8:]


def test_distance_and_percent_identity():
    assert distance_literal(b"ACGT", b"ACGT") == 0 and distance_literal(b"", b"AC") == 2 and distance_literal(b"AC", b"") == 2
    assert distance_literal(b"ACGATC", b"AAGATC") == 1 and distance_literal(b"ACGATC", b"TTGATC") == 2
    assert distance_literal(b"KITTEN", b"SITTING") == 3
    # the stale last column: the true distance of AB and A is 1; the reference's rows give 2 (v0[1] is still 1 when row 2 reads it)
    assert distance_literal(b"AB", b"A") == 2
    assert distance_literal(b"ACGTACGTAA", b"ACGT") == 5          # true 6, but |t| + 1 = 5 caps it
    rng = np.random.default_rng(1)
    for _ in range(300):
        a = bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 40))).astype(np.uint8))
        b = bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 40))).astype(np.uint8))
        if rng.integers(0, 2):
            b = a[:len(a) // 2] + b[:3] + a[len(a) // 2:]
        assert distance(a, b) == distance_literal(a, b), (a, b)
    assert percent_identity(b"ACGATC", b"AAGATC") == F32(F32(5) / F32(6))
    assert percent_identity(b"ACGATC", b"TTGATC") == F32(F32(4) / F32(6))
    assert percent_identity(b"ACGT", b"ACGT") == 1 and percent_identity(b"ACGTAC", b"ACGT") == F32(F32(6 - distance(b"ACGTAC", b"ACGT")) / F32(6))


def test_capacity_bounds_every_gap_layout():
    rng = np.random.default_rng(2)
    for _ in range(2000):
        k, m = int(rng.integers(2, 12)), int(rng.integers(0, 4))
        nk = int(rng.integers(1, 80))
        good = rng.random(nk) < rng.random()
        c = [F32(1.0 if x else 0.0) for x in good]
        growth = 0
        for g, nb in gap_scan(c, F32(1.0)):
            if g != 0 and g + nb != nk:
                growth += 2 if nb == k else m                   # the most each kind can add
        length = nk + k - 1
        assert length + growth <= capacity(length, k, m), (k, m, list(good))
        assert len(gap_scan(c, F32(1.0))) <= (nk + 1) // 2
    assert capacity(3, 5, 3) == 3 and capacity(5, 5, 3) == 5 and capacity(7, 5, 3) == 7 + 3 and capacity(11, 5, 1) == 11 + 3 + 2


def test_left_tip_outcomes():
    g = EGraph([(TRUE, 10)])
    # no variants: two foreign letters before the transcript's first base — nothing is known left of ACGAT
    s = b"TT" + HEAD
    assert g.run(s) == (s, 0, [dict(first=0, run=2, kind=LEFT_EDGE, outcome=KEPT, repl_len=2)])
    # one bad k-mer, lookahead 2: dropped as soon as the true first base is a variant
    out, fl, recs = g.run(sub(HEAD, 0, "C"))
    assert (out, fl, kinds(recs)) == (HEAD[1:], CORRECTED | GAP, [(LEFT_EDGE, TRIMMED)]) and recs[0]["repl_len"] == 0
    # two bad k-mers: the greedy extension ACGATC against AAGATC, 5/6 >= 0.8: replaced
    out, fl, recs = g.run(sub(HEAD, 1, "A"))
    assert (out, fl, kinds(recs)) == (HEAD, CORRECTED | GAP, [(LEFT_EDGE, REPLACED)]) and recs[0]["repl_len"] == 2
    # both first letters wrong: 4/6 < 0.8; TTGAT has no predecessor in the graph and 2 < k: a blunt end, dropped
    s = b"TT" + HEAD[2:]
    out, fl, recs = g.run(s)
    assert (out, fl, kinds(recs)) == (HEAD[2:], CORRECTED | GAP, [(LEFT_EDGE, TRIMMED)])
    # ... unless something precedes it: kept
    g2 = EGraph([(TRUE, 10)], extra={b"ATTGA": 3})
    assert g2.run(s) == (s, 0, [dict(first=0, run=2, kind=LEFT_EDGE, outcome=KEPT, repl_len=2)])


def test_right_tip_outcomes():
    g = EGraph([(TRUE, 10)])
    n = len(TAIL)                                                    # 20 letters, 16 k-mers
    s = TAIL + b"TT"
    assert g.run(s) == (s, 0, [dict(first=16, run=2, kind=RIGHT_EDGE, outcome=KEPT, repl_len=2)])
    out, fl, recs = g.run(sub(TAIL, n - 1, "G"))
    assert (out, fl, kinds(recs)) == (TAIL[:-1], CORRECTED | GAP, [(RIGHT_EDGE, TRIMMED)])
    out, fl, recs = g.run(sub(TAIL, n - 2, "G"))
    assert (out, fl, kinds(recs)) == (TAIL, CORRECTED | GAP, [(RIGHT_EDGE, REPLACED)]) and recs[0]["first"] == 14
    s = TAIL[:-2] + b"GG"
    out, fl, recs = g.run(s)
    assert (out, fl, kinds(recs)) == (TAIL[:-2], CORRECTED | GAP, [(RIGHT_EDGE, TRIMMED)])
    g2 = EGraph([(TRUE, 10)], extra={b"TCGGA": 3})
    assert g2.run(s) == (s, 0, [dict(first=14, run=2, kind=RIGHT_EDGE, outcome=KEPT, repl_len=2)])


def test_snv_bubble():
    bad = sub(TRUE, 12, "T")                                         # k-mers 8 .. 12 hold the error: exactly k
    # the candidates start with the first BAD k-mer: with the erroneous k-mers absent every minimum is 0 — kept; the mismatch pass
    # then replaces the base (the sequence where only the mismatch pass acts)
    g = EGraph([(TRUE, 10)])
    out, fl, recs = g.run(bad)
    assert (out, fl, kinds(recs)) == (TRUE, CORRECTED | MISMATCH, [(SNV, KEPT)]) and recs[0]["first"] == 8 and recs[0]["run"] == K
    # every window of left + G + right known thinly (3 < T): G wins, the k + 2 k-mers go in, the sequence grows by two letters
    cand = bad[8:13] + b"G" + bad[12:17]
    extra = {cand[i:i + K]: 3 for i in range(K + 2)}
    g = EGraph([(TRUE, 10)], extra=extra)
    assert [g.counts(bad)[i] for i in (8, 12)] == [3, 3] and g.counts(bad)[9:12] == [0, 0, 0]
    out, fl, recs = g.run(bad, T=5.0)
    assert kinds(recs) == [(SNV, REPLACED)] and recs[0]["repl_len"] == K + 2 and fl & GAP
    assert len(out) == len(bad) + 2
    assert out[:13] == bad[:13] and out[15:] == bad[13:]            # bad[:13] + n + bad[12:], whatever the mismatch pass made of n's neighbourhood
    # min_kmer_cov above the thin windows: kept
    assert kinds(g.run(bad, T=5.0, mincov=4.0)[2]) == [(SNV, KEPT)]


def test_path_gaps():
    g = EGraph([(TRUE, 10)])
    # two substitutions two apart: 7 bad k-mers, the walk to the right arrives by itself; 7 > k + 1 k-mers, identity 9/11 >= 0.8
    bad = sub(sub(TRUE, 12, "T"), 14, "C")
    out, fl, recs = g.run(bad)
    assert (out, fl, kinds(recs)) == (TRUE, CORRECTED | GAP, [(PATH, REPLACED)]) and (recs[0]["first"], recs[0]["run"], recs[0]["repl_len"]) == (8, 7, 7)
    assert g.max_cov_path(TRUE[7:12], TRUE[15:20], 8, 1.0) == [TRUE[i:i + K] for i in range(8, 15)]
    # one base deleted: 4 bad k-mers, 5 true ones; the walk to the right stops at its bound of 5 one step short of the target, the walk back
    # meets it at once.  At k = 5 every k-mer is of low complexity to isLowComplexityShort (its trinucleotide threshold is round(0.95) = 1),
    # so the meeting is refused; with that test switched off the joined path of 5 k-mers goes in
    dele = TRUE[:12] + TRUE[13:]
    assert all(is_low_complexity_short(TRUE[i:i + K]) for i in range(24))
    assert g.run(dele) == (dele, 0, [dict(first=8, run=4, kind=PATH, outcome=KEPT, repl_len=4)])
    j = EGraph([(TRUE, 10)])
    j.low_complexity = lambda km: False
    out, fl, recs = j.run(dele)
    assert (out, fl, kinds(recs)) == (TRUE, CORRECTED | GAP, [(PATH, REPLACED)]) and (recs[0]["run"], recs[0]["repl_len"]) == (4, 5)
    # three bases deleted (the junction k-mer A|CCGT happens to be the true k-mer 14, so 3 bad k-mers): the joined path has 6 k-mers for a
    # gap of 3: refused for length
    dele3 = TRUE[:12] + TRUE[15:]
    assert j.max_cov_path(TRUE[7:12], TRUE[14:19], 4, 1.0) == [TRUE[i:i + K] for i in range(8, 14)]
    assert j.run(dele3) == (dele3, 0, [dict(first=8, run=3, kind=PATH, outcome=KEPT, repl_len=3)])
    # six letters scrambled: 10 bad k-mers, the true path has 10, but 8/14 < 0.8: refused for identity
    scr = TRUE[:10] + bytes(b"TGCA"[b"ACGT".index(x)] for x in TRUE[10:16]) + TRUE[16:]
    out, fl, recs = g.run(scr)
    assert kinds(recs) == [(PATH, KEPT)] and (recs[0]["first"], recs[0]["run"]) == (6, 10) and out == scr and fl == 0
    assert g.run(scr, pid=0.5)[:2] == (TRUE, CORRECTED | GAP)
    assert is_low_complexity_short(b"A" * 25) and is_low_complexity_short(b"AC" * 12 + b"A") and not is_low_complexity_short(b"ACGATCTTGGCAGTACCGTTAGGAT")


def test_sequences_without_gaps():
    g = EGraph([(TRUE, 10)])
    assert g.run(b"TTTTTTTTTTTT") == (b"TTTTTTTTTTTT", 0, [])         # bad throughout
    assert g.run(TRUE) == (TRUE, 0, [])
    assert g.run(b"ACG") == (b"ACG", 0, []) and g.run(b"") == (b"", 0, [])
    bad = sub(TRUE, 12, "T")
    assert g.run(bad, T=0.0) == (bad, 0, []) and g.run(bad, T=-1.0) == (bad, 0, [])
    # several gaps, each resolved by itself
    two = sub(sub(sub(TRUE, 0, "C"), 12, "T"), 14, "C")
    out, fl, recs = g.run(two)
    assert (out, kinds(recs)) == (TRUE[1:], [(LEFT_EDGE, TRIMMED), (PATH, REPLACED)])


# ---- the feature exists at every layer (these fail before it does) ----
def test_header_declares_the_entry_point():
    src = open(os.path.join(ROOT, "include", "rb_capi.h")).read()
    assert re.search(r"typedef struct rb_corr_params \{ int32_t lookahead, max_indel_size; float percent_identity, min_kmer_cov; \} rb_corr_params;", src)
    assert re.search(r"\bint rb_graph_correct_errors\(rb_graph \*g, const char \*seq, const int64_t \*offsets, int64_t n, const float \*cov_threshold, "
                     r"const rb_corr_params \*p,\s*int64_t \*out_offsets, char \*out_seq, int32_t \*out_len, uint32_t \*flags, rb_corr_gap \*gaps, "
                     r"int64_t \*gap_offsets\);", src)
    assert "GraphUtils.java:3711-3912" in src


def test_library_exports_and_python_binds_it():
    import ctypes as C
    from rnabloom import _native as N
    assert hasattr(C.CDLL(N.LIB_PATH), "rb_graph_correct_errors")
    assert "rb_graph_correct_errors" in {s[0] for s in N.SYMBOLS}
    from rnabloom.graph import BloomFilterDeBruijnGraph
    assert callable(getattr(BloomFilterDeBruijnGraph, "correctErrorsFlat", None))
    assert callable(getattr(BloomFilterDeBruijnGraph, "correctErrors", None))
    assert BloomFilterDeBruijnGraph.GAP_DTYPE.itemsize == 20


def test_java_and_jni_sides_exist():
    java = open(os.path.join(ROOT, "java", "rnabloom", "graph", "NativeGraph.java")).read()
    assert re.search(r"public static native int correctErrors\(long h, ByteBuffer seq, long\[\] offsets, int n, float\[\] covThreshold,", java)
    jni = open(os.path.join(ROOT, "jni", "rb_jni.c")).read()
    assert "FN(correctErrors)" in jni and "rb_graph_correct_errors(" in jni
    g = open(os.path.join(ROOT, "java", "rnabloom", "graph", "BloomFilterDeBruijnGraph.java")).read()
    assert "NativeGraph.correctErrors(handle" in g
