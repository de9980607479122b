"""GraphUtils.extendRightPE / extendLeftPE (R/util/GraphUtils.java:6206-6414) and the loop on top of them, extendPE (:6567-6678), restated line by
line in Python — with countKmerPairsPE / countKmerPairsReversedPE (:5792-5888) and graph.isRepeatKmer = SeqUtils.isRepeat(byte[])
(R/util/SeqUtils.java:458-497, its counters signed bytes) — over the graph of tests/test_extend_step_rules.py with one more question,
lookup_frag_pair(left_kmer, right_kmer).  The walks, the median, the record, the toy graph, the oracle side and the worlds are that file's.
Hand-worked cases run on a dict-backed toy graph; then the worlds of tests/test_gpu_extend_pe.py are built on the CPU oracle alone and every
branch the device test relies on is shown to be reached, in both directions.  No device is needed here."""
import numpy as np
import pytest

import test_extend_step_rules as R
from test_extend_step_rules import (F32, ACGT, NONE, SINGLE, FIRST, SECOND, WHY_FOUND, WHY_NO_CANDIDATE, WHY_NO_SUPPORT, WHY_INVALID_SEED, WHY_SHORT,
                                    naive_extend_no_back_checks, median_cov, Step, has_duplicated_kmer_pair, Toy, OracleSide, World, neighbor, is_acgtu)

WHY_REPEAT_THROWS = 5


class RepeatThrows(Exception):
    """nucleotideArrayIndex gave -1 and isRepeat indexed an array with it (ArrayIndexOutOfBoundsException)"""


def nucleotide_index(b):
    """SeqUtils.nucleotideArrayIndex(byte) :298-313"""
    return {65: 0, 67: 1, 71: 2, 84: 3, 85: 3}.get(b, -1)


def java_round(x):
    """Math.round(float)"""
    return int(np.floor(np.float64(F32(x)) + 0.5))


def is_repeat(kmer, byte_counters=True):
    """SeqUtils.isRepeat(byte[]) :458-497.  The counters are Java bytes: ++ wraps 127 to -128, so a threshold above 127 is never reached
    (byte_counters False: what plain integers would say)."""
    def inc(tab, key):
        v = tab.get(key, 0) + 1
        if byte_counters and v > 127:
            v -= 256
        tab[key] = v
        return v

    def idx(i):
        n = nucleotide_index(kmer[i])
        if n < 0:
            raise RepeatThrows()
        return n
    length = len(kmer)
    t1 = java_round(F32(length) * F32(0.9))
    nf1 = {}
    for i in range(length):
        if inc(nf1, idx(i)) >= t1:
            return True
    t2 = java_round(F32(length // 2) * F32(0.9))
    for start in range(2):
        nf2 = {}
        for i in range(start, length - 1, 2):
            if inc(nf2, (idx(i), idx(i + 1))) >= t2:
                return True
    t3 = java_round(F32(length // 3) * F32(0.9))
    for start in range(3):
        nf3 = {}
        for i in range(start, length - 2, 3):
            if inc(nf3, (idx(i), idx(i + 1), idx(i + 2))) >= t3:
                return True
    return False


def count_pairs_pe(g, kmers, ext, d_r, d_f, direction, gap=0):
    """countKmerPairsPE (:5792-5839) / countKmerPairsReversedPE (:5841-5888): kmers is the sequence's list (reversed for the left-hand
    direction), ext the extension's k-mers in walking order -> (read pairs, fragment pairs, last supported index)"""
    n = len(kmers)
    max_idx = min(d_f - 1 - gap, len(ext) - 1)
    ri, fi = n - d_r + gap, n - d_f + gap
    reads, frags, last = 0, 0, -1
    for i in range(max_idx + 1):
        if 0 <= ri < n:
            left, right = (kmers[ri], ext[i]) if direction == 0 else (ext[i], kmers[ri])
            if g.lookup_read_pair(left, right):
                reads += 1
                last = i
        if 0 <= fi < n:
            left, right = (kmers[fi], ext[i]) if direction == 0 else (ext[i], kmers[fi])
            if g.lookup_frag_pair(left, right):
                frags += 1
                last = i
        ri += 1
        fi += 1
        if ri >= n and fi >= n:
            break
    return reads, frags, last


class StepPE(Step):
    """what one extendRightPE / extendLeftPE returns and the fields of rb_extend_pe_rec: Step's, the fragment pairs and the first-level bound"""

    def __init__(self, outcome, why, n_cand=0, ext=None, pairs=0, fpairs=0, last=-1, winner=-1, score=0.0, max_ext=0, tags=()):
        Step.__init__(self, outcome, why, n_cand, ext, pairs, last, winner, score, tags)
        self.fpairs, self.max_ext = fpairs, max_ext

    def record(self):
        return (self.outcome, self.why, self.n_cand, self.out_len, self.pairs, self.fpairs, self.last, self.winner, self.max_ext)


def extend_step_pe(g, seq, direction, min_cov, d_r, d_f, k):
    """extendRightPE (direction 0, :6206-6309) / extendLeftPE (1, :6311-6414) of getKmers(seq); for the left-hand direction the list is
    reversed here, as the reference's callers reverse it.  max_ext of the record is max(bound of the first-level walks, 0).  Lower-case
    letters are read as upper-case ones, as everywhere in the library; the reference's isRepeat would throw on them."""
    n = len(seq) - k + 1
    m0 = d_f - 2
    if n < 1:
        return StepPE(NONE, WHY_SHORT, max_ext=m0)
    kmers = [seq[i:i + k] for i in range(n)]
    cnts = [F32(c) for c in g.counts(seq)]
    if direction:
        kmers.reverse(); cnts.reverse()
    tags = set()
    if n < d_f:
        tags.add("shorter_than_d")
    if n == 1:
        tags.add("one_kmer")
    last_kmer = kmers[-1]
    if not is_acgtu(last_kmer):
        return StepPE(NONE, WHY_INVALID_SEED, max_ext=m0, tags=tags)
    c4 = g.neighbors(last_kmer, direction)
    cands = [b for b in range(4) if F32(c4[b]) >= F32(1.0)]
    if not cands:
        return StepPE(NONE, WHY_NO_CANDIDATE, max_ext=m0, tags=tags)
    max_ext = m0                                                          # :6215
    walk = lambda km, bound: naive_extend_no_back_checks(g, km, direction, bound, min_cov, tags)
    if len(cands) == 1:                                                   # :6219-6224
        b = cands[0]
        c = neighbor(last_kmer, b, direction)
        return StepPE(SINGLE, WHY_FOUND, 1, [(c, F32(c4[b]), b)] + walk(c, max_ext), winner=b, max_ext=m0, tags=tags)
    try:
        for i in range(n - 1, -1, -1):                                    # :6226-6233
            if is_repeat(kmers[i].upper()):                               # (lower case is read as upper case: include/rb_capi.h, rb_graph_extend_pe)
                max_ext -= 1
            else:
                break
    except RepeatThrows:
        return StepPE(NONE, WHY_REPEAT_THROWS, len(cands), max_ext=m0, tags=tags)
    if max_ext < m0:
        tags.add("repeat_lowered_bound" if max_ext > 0 else "bound_not_positive")
    path_min = min(cnts[max(n - d_f, 0):n])                               # :6235
    best_score, best_cov, best = F32(0), F32(0), None
    for b in cands:
        c = neighbor(last_kmer, b, direction)
        e = [(c, F32(c4[b]), b)] + walk(c, max_ext)
        reads, frags, last = count_pairs_pe(g, kmers, [x[0] for x in e], d_r, d_f, direction)
        if frags > 0 and reads == 0:
            tags.add("frag_only_first_stretch")
        if last >= 0 and reads > 0 and frags > 0:
            cov = median_cov([x[1] for x in e])
            score = F32(F32(min(path_min, cov) * F32(reads + frags)) / F32(last + 1))
            if score > best_score or (score == best_score and cov > best_cov):
                if score == best_score and best is not None:
                    tags.add("tie_by_cov")
                best_score, best_cov = score, cov
                best = (FIRST, e[:last + 1], reads, frags, last, b, len(e))
        else:
            gap = len(e)
            by_read, by_frag = gap >= d_r - 1 and reads == 0, gap >= d_f - 1 and frags == 0
            if by_read or by_frag:                                        # :6268-6271
                if by_read:
                    tags.add("skipped_by_read")
                if by_frag:
                    tags.add("skipped_by_frag")
                continue
            if reads > 0 or frags > 0:
                tags.add("second_level_with_first_support")
            c4n = g.neighbors(e[-1][0], direction)
            for b2 in [x for x in range(4) if F32(c4n[x]) >= F32(1.0)]:
                nc = neighbor(e[-1][0], b2, direction)
                ne = e + [(nc, F32(c4n[b2]), b2)] + walk(nc, max_ext - gap)
                reads, frags, last = count_pairs_pe(g, kmers, [x[0] for x in ne], d_r, d_f, direction)
                if last >= 0 and reads > 0 and frags > 0:
                    cov = median_cov([x[1] for x in ne])
                    score = F32(F32(min(path_min, cov) * F32(reads + frags)) / F32(last + 1))
                    if score > best_score or (score == best_score and cov > best_cov):
                        if score == best_score and best is not None:
                            tags.add("tie_by_cov")
                        best_score, best_cov = score, cov
                        best = (SECOND, ne[:last + 1], reads, frags, last, b | (b2 << 4), len(ne))
    if best is None:
        return StepPE(NONE, WHY_NO_SUPPORT, len(cands), max_ext=max(max_ext, 0), tags=tags)
    tags.add("trimmed" if len(best[1]) < best[6] else "untrimmed")
    return StepPE(best[0], WHY_FOUND, len(cands), best[1], best[2], best[3], best[4], best[5], best_score, max(max_ext, 0), tags)


def extend_pe(g, seq, min_cov, d_r, d_f, k, trace=None):
    """extendPE (:6567-6678): line for line extendSE (:6454-6565) with d = the fragment-paired distance and the PE steps — the restated
    loop of the rules file with those two put in.  (A step in which the reference's isRepeat throws returns nothing here.)"""
    return R.extend_se(g, seq, min_cov, d_f, k, step=lambda gg, text, direction, thr, d, kk: extend_step_pe(gg, text, direction, thr, d_r, d_f, kk), trace=trace)


# ---- the toy graph with fragment pairs ----
class ToyPE(Toy):
    """Toy (k-mers with counts, read pairs d_r apart inside the reads) plus fragment pairs: k-mers d_f apart inside each of `frags`"""

    def build_pe(self, d_r, d_f, frags):
        self.build(d_r)
        self.fpairs = set()
        for f in frags:
            km = [f[i:i + self.k] for i in range(len(f) - self.k + 1)]
            for i in range(len(km) - d_f):
                self.fpairs.add((km[i], km[i + d_f]))
        return self

    def lookup_frag_pair(self, left, right):
        return (left, right) in self.fpairs


#       0         1         2         3
#       0123456789012345678901234567890123
P6 = b"CATGGTCAGTTCGATACC"                   # a prefix of 18 letters whose 6-mers are no repeats; the fork is behind it
A6 = P6 + b"GAGCTTACGGATTCAA"                # branch G
B6 = P6 + b"TCTAGGCATTGCAACG"                # branch T


def rec(st):
    return st.record(), st.bases, st.score


def test_hand_worked_fork_decided_by_fragment_pairs_only():
    k, d_r, d_f = 6, 3, 5
    # both transcripts once: every k-mer off the prefix counts 1, the prefix 2; reads give both branches the same read pairs; only B is a fragment
    g = ToyPE(k, [A6, B6]).build_pe(d_r, d_f, [B6])
    st = extend_step_pe(g, P6, 0, 1.0, d_r, d_f, k)
    # 13 k-mers of sequence, the last is GATACC; candidates ATACCG (G, 2) and ATACCT (T, 3).  No trailing repeat: M = d_f - 2 = 3, every walk
    # adds M + 1 = 4 k-mers: 5 k-mers a branch.  Read partners (d_r = 3): i = 0, 1, 2 pair with k-mers 10, 11, 12 — 3 read pairs for both.
    # Fragment partners (d_f = 5): i = 0 .. 4 pair with k-mers 8 .. 12 — 5 fragment pairs for T, none for G.  G: gap 5 >= d_f - 1 without a
    # fragment pair: skipped.  T: min(pathMinCov 2, median 1) * (3 + 5) / (4 + 1) = 1.6, untrimmed.
    assert st.record() == (FIRST, WHY_FOUND, 2, 5, 3, 5, 4, 3, 3) and st.bases == b"TCTAG" and st.score == F32(F32(8.0) / F32(5.0))
    assert {"skipped_by_frag", "untrimmed"} <= st.tags and "skipped_by_read" not in st.tags
    # mirrored to the left
    gl = ToyPE(k, [A6[::-1], B6[::-1]]).build_pe(d_r, d_f, [B6[::-1]])
    assert rec(extend_step_pe(gl, P6[::-1], 1, 1.0, d_r, d_f, k)) == rec(st)
    # without any fragment nothing is supported: both are skipped, the reference returns null
    g0 = ToyPE(k, [A6, B6]).build_pe(d_r, d_f, [])
    st0 = extend_step_pe(g0, P6, 0, 1.0, d_r, d_f, k)
    assert st0.record() == (NONE, WHY_NO_SUPPORT, 2, 0, 0, 0, -1, -1, 3) and st0.ext is None


def test_hand_worked_read_distance_above_fragment_distance_and_skip_by_read():
    k, d_r, d_f = 6, 7, 3
    # fragments of both branches, but read pairs (d_r = 7) of B only: behind the prefix A6 comes as reads of 12 letters, which hold no pair 7 apart
    g = ToyPE(k, [A6[:18], A6[13:25], A6[19:31], A6[22:], B6]).build_pe(d_r, d_f, [A6, B6])
    st = extend_step_pe(g, P6, 0, 1.0, d_r, d_f, k)
    # M = 1: a candidate and 2 more k-mers.  i runs to min(d_f - 1, 2) = 2; read partners 13 - 7 + i = 6, 7, 8; fragment partners 10, 11, 12.
    # G: 3 fragment pairs, no read pair, gap 3 < d_r - 1: not skipped by the read test, and it has fragment pairs: second level, bound
    #    M - gap = -2: its next candidate + one k-mer; the chain's i still ends at 2, so still no read pair: unscored.
    # T: 3 + 3 pairs, last 2: min(2, 1) * 6 / 3 = 2.
    assert st.record() == (FIRST, WHY_FOUND, 2, 3, 3, 3, 2, 3, 1) and st.bases == b"TCT" and st.score == F32(2.0)
    assert {"frag_only_first_stretch", "second_level_with_first_support"} <= st.tags
    # d_r = 3: the same stretch G is now d_r - 1 = 2 or more long without a read pair: skipped by the read test
    # (its three k-mers come from a read of their own, which holds no pair 3 apart)
    g2 = ToyPE(k, [A6[:18], A6[13:21], A6[16:], B6]).build_pe(3, d_f, [A6, B6])
    st2 = extend_step_pe(g2, P6, 0, 1.0, 3, d_f, k)
    assert "skipped_by_read" in st2.tags and st2.winner == 3 and st2.outcome == FIRST


#        the prefix, then a second fork 2 k-mers behind the first: P6 + GA | GCTT... / P6 + GA | TGCA... and the other branch P6 + T...
S_1 = P6 + b"GAGCTTACGGATTCAA"
S_2 = P6 + b"GATGCACTTGGCCATA"
S_3 = P6 + b"TCTAGGCATTGCAACG"


def test_hand_worked_second_level_wins_with_both_kinds_after_read_support_alone():
    k, d_r, d_f = 6, 3, 8
    # S_2 is read and fragment; S_1 and S_3 are reads only
    g = ToyPE(k, [S_1, S_2, S_3]).build_pe(d_r, d_f, [S_2])
    st = extend_step_pe(g, P6, 0, 1.0, d_r, d_f, k)
    # candidates G (ATACCG, count 2) and T (count 1), M = 6.  G's walk: TACCGA, then ACCGAG / ACCGAT are two: a first stretch of gap 2
    # with read pairs at i = 0, 1 (partners 10, 11) and fragment partners 5, 6: S_2 pairs them: 2 fragment pairs as well -> scored at once.
    # So fragment-less S_1 is taken for the fragment test instead: see the second graph below.
    assert st.outcome == FIRST and st.record()[4:6] == (2, 2)
    # the fragment S_2 cut so that it starts behind k-mer 6 of the prefix: the first stretch's partners 5, 6 have no fragment pair any more
    g2 = ToyPE(k, [S_1, S_2, S_3]).build_pe(d_r, d_f, [S_2[7:]])
    st2 = extend_step_pe(g2, P6, 0, 1.0, d_r, d_f, k)
    # G: first stretch ATACCG TACCGA: 2 read pairs, no fragment pair; gap 2 < d_f - 1 and it has read pairs: second level, bound 6 - 2 = 4.
    #   (G, A) ACCGAG + 5 k-mers along S_1: chain of 8; read pair also at i = 2 (partner 12): 3 read pairs, no fragment pair: unscored.
    #   (G, T) ACCGAT + 5 k-mers along S_2: chain of 8; 3 read pairs; fragment partners 5 + i: the fragment starts at letter 7, so k-mers
    #          7 .. 12 are its: i = 2 .. 7 -> 6 fragment pairs, last 7: min(pathMinCov 3, median 1) * 9 / 8.
    # T: 8 k-mers along S_3: 3 read pairs, no fragment pair, gap 8 >= d_f - 1: skipped by the fragment test.
    assert st2.record() == (SECOND, WHY_FOUND, 2, 8, 3, 6, 7, 2 | (3 << 4), 6) and st2.bases == b"GATGCACT"
    assert st2.score == F32(F32(9.0) / F32(8.0)) and {"second_level_with_first_support", "skipped_by_frag", "untrimmed"} <= st2.tags


def test_hand_worked_homopolymer_tail_lowers_the_bound():
    k, d_r, d_f = 6, 3, 8
    tail = b"GTCAAAAAAA"                                  # seven A: its last three 6-mers CAAAAA AAAAAA AAAAAA hold five or six, t1 = round(5.4) = 5
    ta, tb = b"CATGGTCC" + tail + b"CGTAGCTTGACC", b"CATGGTCC" + tail + b"GCTTAGGATCCA"
    g = ToyPE(k, [ta, tb]).build_pe(d_r, d_f, [ta, tb])
    q = b"CATGGTCC" + tail                                # 13 k-mers; every k-mer of the transcripts counts 2 up to the tail, AAAAAA 4
    assert [is_repeat(q[i:i + k]) for i in range(len(q) - k + 1)][-4:] == [False, True, True, True]
    st = extend_step_pe(g, q, 0, 1.0, d_r, d_f, k)
    # candidates of AAAAAA: itself (A), AAAAAC (C, along ta) and AAAAAG (G, along tb).  Three trailing repeats: M = 6 - 3 = 3.
    # A: AAAAAA has three successors, its walk adds nothing; no pair (no read holds CAAAAA 3 before AAAAAA); one branch further nothing scores:
    #    the chain repeats a k-mer, so k-mer i of it lies one place before the transcript's k-mer its partners were inserted with.
    # C: AAAAAC AAAACG AAACGT AACGTA ACGTAG (M + 1 = 4 added): read pairs at i = 0, 1, 2 (partners 10, 11, 12), fragment pairs at
    #    i = 0 .. 4 (partners 5 .. 9), last 4: min(pathMinCov 2, median 1) * 8 / 5 = 1.6.
    # G: AAAAAG AAAAGC AAAGCT AAGCTT, and AAGCTT has two successors (AGCTTA; AGCTTG of ta): 3 read pairs, 4 fragment pairs, last 3:
    #    1 * 7 / 4 = 1.75 wins, untrimmed.
    assert st.record() == (FIRST, WHY_FOUND, 3, 4, 3, 4, 3, 2, 3) and st.bases == b"GCTT" and st.score == F32(1.75)
    assert "repeat_lowered_bound" in st.tags
    # d_f = 5: M = 3 - 3 = 0: a candidate + 1 k-mer.  C: AAAAAC AAAACG: read pairs at i = 0, 1, fragment pairs at i = 0, 1 (partners 8, 9):
    # min(2, 1) * 4 / 2 = 2; G the same, and a tie with equal medians keeps the first
    g5 = ToyPE(k, [ta, tb]).build_pe(d_r, 5, [ta, tb])
    st5 = extend_step_pe(g5, q, 0, 1.0, d_r, 5, k)
    assert st5.record() == (FIRST, WHY_FOUND, 3, 2, 2, 2, 1, 1, 0) and st5.bases == b"CG" and st5.score == F32(2.0) and "bound_not_positive" in st5.tags
    # d_f = 4: M = 2 - 3 = -1 acts as 0 does, and the record says max(M, 0)
    g4 = ToyPE(k, [ta, tb]).build_pe(d_r, 4, [ta, tb])
    st4 = extend_step_pe(g4, q, 0, 1.0, d_r, 4, k)
    assert st4.record()[:4] == (FIRST, WHY_FOUND, 3, 2) and st4.max_ext == 0 and st4.bases == b"CG"
    # one candidate only (the sequence ends at TCAAAA): the scan does not run, the bound stays d_f - 2
    assert extend_step_pe(g5, q[:-3], 0, 1.0, d_r, 5, k).record() == (SINGLE, WHY_FOUND, 1, 1, 0, 0, -1, 0, 3)


def test_is_repeat_is_the_reference_s():
    assert is_repeat(b"AAAAAC") and not is_repeat(b"AAAACC") and is_repeat(b"ACACAC") and is_repeat(b"ACGACG") and not is_repeat(b"ACGTCA")
    assert is_repeat(b"TTUUTT")                                       # U counts as T
    # k = 4 and 5: t3 = round(1 * 0.9) = 1, the first trinucleotide reaches it — every k-mer is a repeat
    assert is_repeat(b"ACGT") and is_repeat(b"ACGTA")
    # k = 143: t1 = round(128.7) = 129 is above what a signed byte holds.  130 A's with 13 C's scattered so that no dinucleotide or
    # trinucleotide phase reaches t2 = 64 / t3 = 42: no repeat for the reference, a repeat with counters that do not wrap
    km = bytearray(b"A" * 143)
    for p in range(5, 143, 11):
        km[p] = ord("C")
    km = bytes(km)
    assert km.count(b"A") == 130 and len(km) == 143
    assert not is_repeat(km) and is_repeat(km, byte_counters=False)
    assert is_repeat(b"A" * 100 + b"C" * 10)
    # a letter outside ACGTU throws ... unless a base count reaches t1 in front of it
    with pytest.raises(RepeatThrows):
        is_repeat(b"ACNTCA")
    with pytest.raises(RepeatThrows):
        is_repeat(b"acgtca")
    assert is_repeat(b"AAAAAN")


def test_hand_worked_throw():
    k, d_r, d_f = 6, 3, 8
    tail = b"GTCAAAAAAA"
    ta, tb = b"CATGGTCC" + tail + b"CGTAGCTTGACC", b"CATGGTCC" + tail + b"GCTTAGGATCCA"
    g = ToyPE(k, [ta, tb]).build_pe(d_r, d_f, [ta, tb])
    # the scan passes three repeats (AAAAAA AAAAAA CAAAAA) and meets TCAAAA with its T replaced: N in front of any count of 5 -> the reference throws
    q = b"CATGGTCCGNCAAAAAAA"
    st = extend_step_pe(g, q, 0, 1.0, d_r, d_f, k)
    assert st.record() == (NONE, WHY_REPEAT_THROWS, 3, 0, 0, 0, -1, -1, 6) and st.ext is None
    # ... and with the N next to the A's: three times AAAAAA, then NAAAAA throws at its first letter
    assert extend_step_pe(g, b"CATGGTCCGNAAAAAAAA", 0, 1.0, d_r, d_f, k).why == WHY_REPEAT_THROWS
    # an N further back than the first k-mer that is no repeat is not seen
    q2 = b"CATNGTCC" + tail
    assert extend_step_pe(g, q2, 0, 1.0, d_r, d_f, k).why != WHY_REPEAT_THROWS


def test_count_pairs_pe_needs_no_order_of_the_distances():
    class Yes:
        def lookup_read_pair(self, a, b): return True
        def lookup_frag_pair(self, a, b): return True
    km, ext = [bytes([65 + i]) for i in range(6)], [bytes([97 + i]) for i in range(9)]
    # d_r = 4, d_f = 8: i to min(7, 8) = 7; read partners 2 + i < 6 -> i = 0 .. 3; fragment partners -2 + i in [0, 6) -> i = 2 .. 7
    assert count_pairs_pe(Yes(), km, ext, 4, 8, 0) == (4, 6, 7)
    # d_r = 8, d_f = 4: i to 3; read partners -2 + i -> i = 2, 3; fragment partners 2 + i -> i = 0 .. 3
    assert count_pairs_pe(Yes(), km, ext, 8, 4, 0) == (2, 4, 3)
    # both partners off the list's end after the first k-mer: the loop stops
    assert count_pairs_pe(Yes(), km[:1], ext, 1, 1, 0) == (1, 1, 0)


# ---- the worlds of the device test, on the CPU oracle ----
class OracleSidePE(OracleSide):
    def __init__(self, og, frag_h):
        OracleSide.__init__(self, og)
        self.frag_h, self._fp = frag_h, {}

    def lookup_frag_pair(self, left, right):
        hit = self._fp.get((left, right))
        if hit is None:
            p, _, _ = self.rbo.hash_pairs_region(left + right, self.k, self.frag_h, self.k, self.mode)
            hit = self._fp[(left, right)] = self.og.lookup_fragment_pair(p[0])
        return hit


NEED_TAGS = {"tie_by_cov", "trimmed", "untrimmed", "walk_repeat", "shorter_than_d", "one_kmer", "skipped_by_read", "skipped_by_frag",
             "second_level_with_first_support", "frag_only_first_stretch", "repeat_lowered_bound", "bound_not_positive"}


class WorldPE:
    """R.World (reads, read pairs at d_r, the queries and their floors) with a fragment-pair filter on the same oracle graph: fragments are
    transcript pieces of at least k + d_f letters, inserted as tests/test_gpu_paired_segments.py::World inserts them (add_dbg_only of their
    k-mers, read pairs, fragment pairs).  Of every three transcripts one is a fragment as a whole, one over its first 60 % only and one not at
    all, so that support by reads alone occurs; everything is mirrored for the left-hand direction as R.World mirrors its reads.  extra:
    (transcript, multiplicity, queries[, fragment]) added on top, second_level_by_fragments among them — their reads go in by a second
    add_reads call; a fragment given with a transcript replaces the one-in-three rule for it."""
    FSIZE = 2_400_011

    def __init__(self, k, stranded, seed, d_r, d_f, extra=(), fsize=None, second_level_lengths=None, frag_part=0.6, **kw):
        from oracle import rbo
        if fsize is not None:
            self.FSIZE = fsize
        self.w = w = World(k, stranded, seed, d=d_r, **kw)
        self.k, self.stranded, self.d_r, self.d_f, self.hashes, self.sizes = k, stranded, d_r, d_f, w.hashes, w.sizes
        self.og, self.packed = w.og, w.packed
        tx, queries, floors = list(w.tx), list(w.queries), list(w.floors)
        self.extra_packed = None
        extra, pieces = list(extra) + second_level_by_fragments(k, d_f, seed + 1, second_level_lengths), {}
        if extra:
            reads = []
            read_len, tile = kw.get("read_len", 100), kw.get("tile", 10)
            for t, m, qs, *piece in extra:
                if piece:
                    pieces[len(tx)] = piece[0]
                tx.append((t, m))
                for tt in (t, t[::-1]):
                    starts = list(range(0, max(len(tt) - read_len, 0) + 1, tile))
                    if starts[-1] < len(tt) - read_len:
                        starts.append(len(tt) - read_len)
                    reads += [tt[a:a + read_len] for a in starts] * m
                for kind, s in qs:
                    queries += [(kind, s, 0), (kind, s[::-1], 1)]
                    floors += [1.0, 1.0]
            self.extra_packed = rbo.pack_reads(reads, [b"I" * len(s) for s in reads])
            self.og.add_reads(*self.extra_packed, 3, rbo.STORE_READ_PAIRS)
        # queries whose sequence ends d_f - 1, d_f and d_f + 5 k-mers before a fork (R.World's ends follow d_r)
        for i in range(0, 2 * kw.get("n_iso", 6), 2):
            p = tx[i][0][:len(tx[i][0]) // 2]
            for e in (d_f - 1, d_f, d_f + 5):
                if len(p) - e >= k:
                    queries += [("fork-f%d" % e, p[:len(p) - e], 0), ("fork-f%d" % e, p[:len(p) - e][::-1], 1)]
                    floors += [1.0, 1.0]
        self.tx, self.queries, self.floors = tx, queries, floors
        self.frag_h = w.hashes[2]
        self.og.init_fragment_pairs(self.FSIZE, self.frag_h, d_f)
        frags = []
        for i, (t, _) in enumerate(tx):
            piece = pieces[i] if i in pieces else t if i % 3 == 0 else t[:int(len(t) * frag_part)] if i % 3 == 1 else b""
            if len(piece) >= k + d_f:
                frags += [piece, piece[::-1]]
        self.frags = frags
        mode = rbo.FWD if stranded else rbo.CANON
        for s in frags:
            hv, _ = rbo.hash_region(s, k, self.og.h, mode)
            for i in range(hv.shape[0]):
                self.og.add_dbg_only(hv[i])
            for dd, add in ((d_r, self.og.add_read_pair), (d_f, self.og.add_fragment_pair)):
                if len(s) >= k + dd:
                    p, _, _ = rbo.hash_pairs_region(s, k, self.frag_h, dd, mode)
                    for i in range(p.shape[0]):
                        add(p[i])
        self.o = OracleSidePE(self.og, self.frag_h)
        self._want = None

    def want(self):
        """the restatement's steps for the queries with their floors, computed once"""
        if self._want is None:
            self._want = [extend_step_pe(self.o, s, direction, fl, self.d_r, self.d_f, self.k) for (_, s, direction), fl in zip(self.queries, self.floors)]
        return self._want

    def assert_every_branch_is_reached(self):
        for direction in (0, 1):
            steps = [st for st, (_, _, dd) in zip(self.want(), self.queries) if dd == direction]
            assert {st.outcome for st in steps} == {NONE, SINGLE, FIRST, SECOND}, direction
            assert {st.why for st in steps} == {WHY_FOUND, WHY_NO_CANDIDATE, WHY_NO_SUPPORT, WHY_INVALID_SEED, WHY_SHORT, WHY_REPEAT_THROWS}, direction
            tags = set().union(*(st.tags for st in steps))
            assert NEED_TAGS <= tags, (direction, NEED_TAGS - tags)


SECOND_LEVEL_LENGTHS = dict(prefix=100, branch=50)      # letters beyond d_f of the shared prefix and of each branch, as at k = 25


def second_level_by_fragments(k, d_f, seed, lengths=None):
    """(transcript, multiplicity, queries, fragment): a fork, a second one five letters on, and fragments of the two far branches that begin
    so late that the first stretch's partners have no fragment pair and the chain's k-mers from the eighth on have one: the first stretch
    goes to the second level with read pairs alone and wins there with both kinds.  Nothing for d_f < 12 (the chain is too short)."""
    if d_f < 12:
        return []
    rng = np.random.default_rng(seed)
    rnd = lambda n: np.frombuffer(ACGT, np.uint8)[rng.integers(0, 4, n)].tobytes()
    ln = dict(SECOND_LEVEL_LENGTHS, **(lengths or {}))
    p, a, bb, c1, c2 = rnd(d_f + ln["prefix"]), rnd(d_f + ln["branch"]), rnd(5), rnd(d_f + ln["branch"]), rnd(d_f + ln["branch"])
    other = lambda x, y: ACGT[(ACGT.index(y[0:1]) + 1) % 4:][:1] + x[1:]          # x with a first letter that is not y's: the forks are forks
    bb, c2 = other(bb, a), other(c2, c1)
    s0 = len(p) - k + 1 - d_f + 8                             # the first k-mer with a fragment pair d_f on is the chain's k-mer 8
    t1, t2 = p + bb + c1, p + bb + c2
    return [(p + a, 1, [("frag-second", p), ("frag-second-short", p[-(k + 3):])], p + a), (t1, 1, [], t1[s0:]), (t2, 2, [], t2[s0:])]


EXTRAS_LENGTHS = dict(flank=150, circle_unit=40, circle_reps=8)     # as at k = 25; tests/pair_worlds.py derives them from k


def extras(k, d_f, seed, lengths=None):
    """what R.World has not: forks behind a short homopolymer stretch with queries whose trailing repeats end at a k-mer with an N (the
    reference's isRepeat throws) — within the d_f - 2 k-mers the device scans; the restatement, like the reference, would throw on an N
    further back in an unbroken run of repeats, where the device has stopped (rb_capi.h), so the worlds hold no such query —; forks behind
    more than d_f - 2 repeat k-mers (the bound is not positive); a circle of 40 k-mers (a walk meets its start again)"""
    rng = np.random.default_rng(seed)
    rnd = lambda n: np.frombuffer(ACGT, np.uint8)[rng.integers(0, 4, n)].tobytes()
    ln = dict(EXTRAS_LENGTHS, **(lengths or {}))
    flank, reps = ln["flank"], ln["circle_reps"]
    out = []
    for i in range(2):
        w, a, b = rnd(flank), rnd(flank), rnd(flank)
        run = b"ACGT"[i:i + 1] * (k + 6)
        p = w + run
        qs = [("rep-fork", p), ("rep-fork-n", R.put(p, len(w) - 3, "N")), ("rep-fork-n-far", R.put(p, 20, "N")), ("rep-fork-short", p[len(w) - 4:])]
        out += [(p + a, 1, qs), (p + b, 2, [])]
    for run in (b"C" * (k + d_f + 5), b"AG" * ((k + d_f + 6) // 2)):
        w, a, b = rnd(flank), rnd(flank), rnd(flank)
        p = w + run
        out += [(p + a, 1, [("rep-long", p), ("rep-long-short", p[-(k + 40):])]), (p + b, 2, [])]
    c = rnd(ln["circle_unit"])
    out.append((c * reps, 1, [("circle-40", (c * reps)[5:5 + k + 10])]))
    return out


WORLDS = {}


def world(k, stranded, d_r=30, d_f=80):
    key = (k, stranded, d_r, d_f)
    if key not in WORLDS:
        WORLDS[key] = WorldPE(k, stranded, 700 + stranded, d_r, d_f, extra=extras(k, d_f, 11 + stranded))
    return WORLDS[key]


@pytest.mark.parametrize("stranded", [False, True])
def test_worlds_reach_every_branch_on_the_oracle(stranded):
    world(25, stranded).assert_every_branch_is_reached()


# ---- the host loop of the package (rnabloom.graphutils.extendPE) without a device ----
class StepStandInPE(R.StepStandIn):
    """what graphutils.extendPE asks of a graph, answered over a ToyPE / OracleSidePE: R.StepStandIn with the fragment distance and the PE step"""

    def __init__(self, g, k, d_r, d_f):
        R.StepStandIn.__init__(self, g, k, d_r)
        self.d_f = d_f

    def getFragPairedKmerDistance(self):
        return self.d_f

    def extendStepPE(self, seqs, direction, floors):
        self.calls += 1
        self.most = max(self.most, len(seqs))
        steps = [extend_step_pe(self.g, s, direction, fl, self.d, self.d_f, self.k) for s, fl in zip(seqs, floors)]
        return [st.bases if st.outcome != NONE else None for st in steps], None


def test_the_package_s_pe_loop_equals_the_restated_loop_on_the_toy_graph():
    from rnabloom import graphutils
    k, d_r, d_f = 6, 3, 5
    g = ToyPE(k, [A6, B6], [1, 3]).build_pe(d_r, d_f, [A6, B6])
    seeds = [t[a:a + n] for t in (A6, B6) for n in (6, 7, 9, 12) for a in range(0, len(t) - n + 1, 3)] + [b"CATGG", b""]
    dev = StepStandInPE(g, k, d_r, d_f)
    texts, ranges = graphutils.extendPE(dev, seeds, 1.0)
    grown = 0
    for s, t, r in zip(seeds, texts, ranges):
        want = extend_pe(g, s, 1.0, d_r, d_f, k) if len(s) >= k else (s, [0, 0])
        assert (t, r) == want, (s, t, r, want)
        grown += len(t) > len(s)
    assert grown > len(seeds) // 2 and dev.most == sum(len(s) >= k for s in seeds)
    assert extend_pe(g, P6[4:12], 1.0, d_r, d_f, k)[0] == B6               # through the fork along the branch covered three times
    with pytest.raises(RuntimeError):
        graphutils.extendPE(StepStandInPE(g, k, d_r, d_f), [P6[4:12]], 1.0, max_rounds=1)


def driver_seeds(w):
    """R.driver_seeds over the PE world's queries and transcripts"""
    class View:
        pass
    v = View()
    v.hot, v.queries, v.tx, v.k = w.w.hot, w.queries, w.tx, w.k
    return R.driver_seeds(v)


@pytest.mark.parametrize("stranded", [False, True])
def test_the_package_s_pe_loop_equals_the_restated_loop_on_the_oracle(stranded):
    from rnabloom import graphutils
    w = world(25, stranded)
    seeds = driver_seeds(w)
    trace = set()
    want = [extend_pe(w.o, s, 1.0, w.d_r, w.d_f, w.k, trace=trace) for s in seeds]
    assert {"stopped_by_used", "floor_fell_twice"} <= trace, trace
    texts, ranges = graphutils.extendPE(StepStandInPE(w.o, w.k, w.d_r, w.d_f), seeds, 1.0)
    assert list(zip(texts, ranges)) == want


@pytest.mark.parametrize("stranded", [False, True])
def test_the_package_s_se_loop_still_equals_its_restated_loop(stranded):
    """graphutils.extendSE after its loop was factored out for extendPE: the SE world of the rules file, the SE restatement"""
    from rnabloom import graphutils
    w = R.world(25, stranded)
    seeds = R.driver_seeds(w)
    want = [R.extend_se(w.o, s, 1.0, w.d, w.k) for s in seeds]
    texts, ranges = graphutils.extendSE(R.StepStandIn(w.o, w.k, w.d), seeds, 1.0)
    assert list(zip(texts, ranges)) == want
