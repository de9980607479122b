"""The rules of rb_graph_overlap_pairs restated in Python from the reference's Java, line by line, and checked on hand-worked cases over a
dictionary graph.  tests/test_gpu_overlap.py applies the same restatement to the CPU oracle.

  GraphUtils.overlap (R/util/GraphUtils.java:4898-5063); SeqUtils.overlapMaximally (R/util/SeqUtils.java:1335-1379), isHomopolymer(byte[])
  :354-368, isRepeat(String) :417-456 over nucleotideArrayIndex(int) :315-330; graph.getKmers(seq, start, end)
  (R/bloom/hash/HashFunction.java:141-171, CanonicalHashFunction.java:137-169) over NTHashIterator.start(seq, start, end)
  (R/bloom/hash/NTHashIterator.java:47-54, 71-73).
The graph is an object with counts(sequence bytes) -> the counts of graph.getKmers(sequence) (every window; 0 for a window with a letter
outside ACGTU) and, for the rescue's mutation only, contains(k-mer), add_dbg_only(k-mer) and add_read_paired_kmers(sequence).  The last part
of the file checks that the feature exists at every layer: header, library, Python class, Java, JNI."""
import math
import os
import re
import zlib

import numpy as np

from test_mismatch_rules import correct_mismatches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

NONE, LEFT, RIGHT, MERGED, SPANNED, RESCUE = range(6)                     # rb_overlap_rec.outcome
FOUND, NO_MATCH, NO_COMPLEX, NO_RIGHT_SINGLETON, NO_LEFT_SINGLETON, REPEAT, SHORT, REPEAT_THROWS = range(8)        # rb_overlap_rec.why
MUTATED_THEN_NULL = 99          # the reference's `return null` at :5044-5046 after a rescue: asserted unreachable below
SWAPPED = 1


# ---- SeqUtils ----
def overlap_maximally(left, right, min_overlap):
    """SeqUtils.overlapMaximally :1335-1379 as it stands.  Returns (overlapped or None, the line that returned)."""
    prefix = right[:min_overlap]                                            # :1336
    ll, rl = len(left), len(right)
    lower, max_li = 0, ll - min_overlap                                     # :1340-1341
    while 0 <= lower <= max_li:                                             # :1343
        lower = left.find(prefix, lower)                                    # :1344
        if lower >= 0:
            upper = lower + rl                                              # :1347
            if upper < ll:
                if left[lower + min_overlap:upper] == right[min_overlap:]:  # :1350-1352
                    return left, "loop-contained"
            else:
                upper = ll                                                  # :1358
                if left[lower + min_overlap:upper] == right[min_overlap:upper - lower]:      # :1359-1361
                    return left + right[upper - lower:], "loop-joined"
            lower += 1                                                      # :1366
    if ll >= rl and right in left:                                          # :1370
        return left, "left-contains-right"
    if ll < rl and left in right:                                           # :1374
        return right, "right-contains-left"
    return None, None


def smallest_agreeing_shift(left, right, min_overlap):
    """the form the device uses: the smallest s in [0, |left| - min_overlap] at which right agrees with left over the whole extent they
    share; else right where it is the longer one and contains left"""
    ll, rl = len(left), len(right)
    for s in range(0, ll - min_overlap + 1):
        e = min(s + rl, ll)
        if left[s:e] == right[:e - s]:
            return left if s + rl < ll else left + right[ll - s:]
    if ll < rl and left in right:
        return right
    return None


def is_homopolymer(b):
    """SeqUtils.isHomopolymer(byte[]) :354-368"""
    return len(b) > 0 and all(x == b[0] for x in b[1:])


class RepeatThrows(Exception):
    """ArrayIndexOutOfBoundsException: nucleotideArrayIndex gave -1 and isRepeat indexed a count array with it"""


def nt_index(ch):
    """SeqUtils.nucleotideArrayIndex(int) :315-330"""
    return {65: 0, 67: 1, 71: 2, 84: 3, 85: 3}.get(ch, -1)


def jbyte_inc(v):
    """++ on a Java byte"""
    return v + 1 if v < 127 else -128


def jround(x):
    """Math.round(float)"""
    return int(math.floor(float(F32(x)) + 0.5))


def is_repeat(seq):
    """SeqUtils.isRepeat(String) :417-456"""
    thr, n = F32(0.9), len(seq)

    def idx(i):
        c = nt_index(seq[i])
        if c < 0:
            raise RepeatThrows()
        return c
    t1 = jround(F32(n) * thr)                                               # :422
    nf1 = [0] * 4
    for i in range(n):
        c = idx(i)
        nf1[c] = jbyte_inc(nf1[c])
        if nf1[c] >= t1:
            return True
    t2 = jround(F32(n // 2) * thr)                                          # :431
    for start in range(2):
        nf2 = {}
        for i in range(start, n - 1, 2):
            key = (idx(i), idx(i + 1))
            nf2[key] = jbyte_inc(nf2.get(key, 0))
            if nf2[key] >= t2:
                return True
    t3 = jround(F32(n // 3) * thr)                                          # :443
    for start in range(3):
        nf3 = {}
        for i in range(start, n - 2, 3):
            key = (idx(i), idx(i + 1), idx(i + 2))
            nf3[key] = jbyte_inc(nf3.get(key, 0))
            if nf3[key] >= t3:
                return True
    return False


# ---- GraphUtils.overlap ----
class Result:
    def __init__(self, outcome, why, swapped=False, overlap=0, text=b"", span_first=0, span_n=0, how=None, fixed=None):
        self.outcome, self.why, self.swapped, self.overlap, self.text = outcome, why, swapped, overlap, text
        self.span_first, self.span_n, self.how, self.fixed = span_first, span_n, how, fixed

    def record(self):
        """(outcome, why, flags, overlap, out_len, span_first, span_n) and the text: what rb_overlap_rec and out_seq hold"""
        return (self.outcome, self.why, SWAPPED if self.swapped else 0, self.overlap, len(self.text), self.span_first, self.span_n), self.text


def overlap(left, right, k, min_overlap, min_kmer_cov, g, mutate=False):
    """GraphUtils.overlap :4898-5063 on the k-mer lists of two strings.  mutate: run :5018-5056 on g for a pair that is rescued (the result
    then also carries `fixed`, the string the returned k-mers spell); without it the result describes the pair before the mutation."""
    mincov = F32(min_kmer_cov)
    overlapped, how = overlap_maximally(left, right, min_overlap)           # :4901
    swapped = False
    if overlapped is None:
        min_overlap = max(min_overlap, min(len(left), len(right)) * 3 // 4)  # :4907 (ints)
        overlapped, how = overlap_maximally(right, left, min_overlap)       # :4909
        if overlapped is not None:
            left, right, swapped = right, left, True                        # :4914-4921
    if overlapped is None:
        return Result(NONE, NO_MATCH)                                       # :5062
    n_ov, ll, rl = len(overlapped), len(left), len(right)
    o = ll + rl - n_ov
    same = dict(swapped=swapped, overlap=o, how=how)
    if n_ov <= ll + rl - k:                                                 # :4932
        if n_ov == max(ll, rl):                                             # :4935
            return Result(LEFT, FOUND, text=left, **same) if ll >= rl else Result(RIGHT, FOUND, text=right, **same)
        end = rl - (n_ov - ll) - k + 1                                      # :4948
        assert end == o - k + 1
        if not any(not is_homopolymer(right[i:i + k]) for i in range(end)):  # :4950-4960
            return Result(NONE, NO_COMPLEX, **same)
        spelled = left + right[end + k - 1:]                                # leftKmers, then rightKmers from `end`: :4962-4969
        assert spelled == overlapped
        return Result(MERGED, FOUND, text=overlapped, **same)
    # the overlap is smaller than k
    start, end = ll - k + 1, n_ov - (rl - k + 1)                            # :4979-4980
    # graph.getKmers(overlapped, start, end): NTHashIterator.start sets pos = start - 1 and max = end - k, hasNext is pos < max — the windows
    # start .. end - k; a window counts 0 iff one of its letters is outside ACGTU ([start, end) are exactly the bases those windows cover),
    # else graph.getCount: getKmers(overlapped)'s counts at those windows
    first, n_span = start, end - k - start + 1
    assert n_span == k - 1 - o
    all_counts = g.counts(overlapped)
    span = [(overlapped[i:i + k], F32(all_counts[i])) for i in range(first, first + n_span)]
    invalid = has_complex = False
    for km, c in span:                                                      # :4983-4994
        if c < mincov:
            invalid = True
            break
        if not has_complex and not is_homopolymer(km):
            has_complex = True
    same.update(span_first=first, span_n=n_span)
    fixed = None
    if invalid:                                                             # :4996
        lc, rc = g.counts(left), g.counts(right)
        if not any(rc[i] == 1 for i in range(min(o, len(rc)))):             # :5001-5007
            return Result(NONE, NO_RIGHT_SINGLETON, swapped=swapped, overlap=o, how=how)
        if not any(lc[i] == 1 for i in range(max(0, len(lc) - o), len(lc))):          # :5010-5016
            return Result(NONE, NO_LEFT_SINGLETON, swapped=swapped, overlap=o, how=how)
        try:
            if is_repeat(right[:o]):                                        # :5018
                return Result(NONE, REPEAT, swapped=swapped, overlap=o, how=how)
        except RepeatThrows:
            return Result(NONE, REPEAT_THROWS, swapped=swapped, overlap=o, how=how)
        counts = []
        for km, c in span:                                                  # :5020-5030
            if c == 0:
                if mutate:
                    g.add_dbg_only(km)
                c = F32(1)
            counts.append(c)
            if not has_complex and not is_homopolymer(km):
                has_complex = True
        if span and not has_complex:                                        # :5044-5046, after a rescue
            return Result(MUTATED_THEN_NULL, NO_COMPLEX, swapped=swapped, overlap=o, how=how)
        if mutate:                                                          # :5053-5056
            fixed, _, _ = correct_mismatches(overlapped, list(lc) + counts + list(rc), k, 2.0, min_kmer_cov, g.contains, g.counts)
            g.add_read_paired_kmers(fixed)
        return Result(RESCUE, FOUND, text=overlapped, fixed=fixed, **same)
    if span and not has_complex:                                            # :5044-5046
        return Result(NONE, NO_COMPLEX, swapped=swapped, overlap=o, how=how)
    return Result(SPANNED, FOUND, text=overlapped, **same)


def expected(left, right, k, min_overlap, min_kmer_cov, g):
    """what rb_graph_overlap_pairs reports for the pair: the reference's answer, and NONE / SHORT where the reference throws in substring or
    is never called (a read shorter than max(k, min_overlap))"""
    if min(len(left), len(right)) < max(k, min_overlap):
        return Result(NONE, SHORT).record()
    return overlap(left, right, k, min_overlap, min_kmer_cov, g).record()


# ---- a dictionary graph: getCount by k-mer (upper case, U as T), dbgbf membership, the read-paired k-mers that were added ----
NORM = bytes.maketrans(b"acgtuU", b"ACGTTT")


class DictGraph:
    def __init__(self, k, paths, extra=None, absent=(), d=3):
        self.k, self.d, self.count, self.pairs = k, d, {}, set()
        for seq, cov in paths:
            for i in range(len(seq) - k + 1):
                self.count[seq[i:i + k].translate(NORM)] = cov
        self.count.update(extra or {})
        self.dbg = set(self.count) - set(absent)

    def contains(self, kmer):
        return kmer.translate(NORM) in self.dbg

    def counts(self, seq):
        out = []
        for i in range(len(seq) - self.k + 1):
            w = seq[i:i + self.k]
            km = w.translate(NORM)
            out.append(F32(self.count.get(km, 1) if all(ch in b"ACGTUacgtu" for ch in w) and km in self.dbg else 0))
        return out

    def add_dbg_only(self, kmer):                       # (a k-mer the counting filter has not seen counts cbf + 1 = 1 afterwards)
        self.dbg.add(kmer.translate(NORM))

    def add_read_paired_kmers(self, seq):
        kms = [seq[i:i + self.k].translate(NORM) for i in range(len(seq) - self.k + 1)]
        self.pairs |= {(a, b) for a, b in zip(kms, kms[self.d:])}


X = b"ACGATCTTGGCAGTACCGTTAGGATCCA"          # 28 bases, distinct 5-mers (and so distinct 8-mers)
K, MO = 5, 3


def rec5(left, right, g=None, mo=MO, mincov=1.0):
    return expected(left, right, K, mo, mincov, g or DictGraph(K, [(X, 10)]))


def test_the_sequence_has_distinct_kmers():
    kms = [X[i:i + K] for i in range(len(X) - K + 1)]
    assert len(set(kms)) == len(kms) == 24


def test_an_overlap_of_exactly_k_merges_with_end_1():
    left, right = X[0:12], X[7:19]                               # left[7:12] = TGGCA = right[0:5]; TGG occurs in left at 7 only
    assert rec5(left, right) == ((MERGED, FOUND, 0, 5, 19, 0, 0), X[0:19])


def test_an_overlap_of_k_minus_1_has_an_empty_span():
    left, right = X[0:12], X[8:20]                               # 4 bases: no spanning k-mer, nothing to look up, nothing to be complex
    assert rec5(left, right) == ((SPANNED, FOUND, 0, 4, 20, 8, 0), X[0:20])
    assert rec5(left, right, DictGraph(K, [])) == ((SPANNED, FOUND, 0, 4, 20, 8, 0), X[0:20])


def test_an_overlap_of_min_overlap_and_one_less():
    left = X[0:12]
    # 3 bases: one spanning k-mer, window 8 of the joined text = X[8:13], count 10
    assert rec5(left, X[9:21]) == ((SPANNED, FOUND, 0, 3, 21, 8, 1), X[0:21])
    # 2 bases: the prefix CAG is not in left; the dovetail attempt wants max(3, 12 * 3 / 4) = 9 and finds nothing either
    assert rec5(left, X[10:22]) == ((NONE, NO_MATCH, 0, 0, 0, 0, 0), b"")
    # ... and with min_overlap 2 it is found: two spanning k-mers, windows 8 and 9
    assert rec5(left, X[10:22], mo=2) == ((SPANNED, FOUND, 0, 2, 22, 8, 2), X[0:22])


def test_containments():
    # right is a suffix of left: upperL == leftLength, the else-branch returns left + "" (:1357-1364)
    assert overlap_maximally(X[0:15], X[8:15], MO) == (X[0:15], "loop-joined")
    assert rec5(X[0:15], X[8:15]) == ((LEFT, FOUND, 0, 7, 15, 0, 0), X[0:15])
    # right in the middle of left (:1348-1356)
    assert overlap_maximally(X[0:15], X[4:11], MO) == (X[0:15], "loop-contained")
    assert rec5(X[0:15], X[4:11]) == ((LEFT, FOUND, 0, 7, 15, 0, 0), X[0:15])
    # left is a prefix of right: shift 0, left + right[8:] = right, the longer read's k-mers
    assert overlap_maximally(X[0:8], X[0:14], MO) == (X[0:14], "loop-joined")
    assert rec5(X[0:8], X[0:14]) == ((RIGHT, FOUND, 0, 8, 14, 0, 0), X[0:14])
    # left in the middle of right: right's prefix ACG is not in left, the `contains` fallback (:1374) answers
    assert overlap_maximally(X[4:11], X[0:15], MO) == (X[0:15], "right-contains-left")
    assert rec5(X[4:11], X[0:15]) == ((RIGHT, FOUND, 0, 7, 15, 0, 0), X[0:15])
    # equal reads: left wins the tie
    assert rec5(X[0:10], X[0:10]) == ((LEFT, FOUND, 0, 10, 10, 0, 0), X[0:10])


def test_the_dovetail_at_the_three_quarters_boundary():
    # right's tail is left's head.  12 and 12 bases: min_overlap becomes 12 * 3 / 4 = 9
    right = X[0:12]
    assert rec5(X[3:15], right) == ((MERGED, FOUND, SWAPPED, 9, 15, 0, 0), X[0:15])          # 9 bases shared: shift 3 <= 12 - 9
    assert rec5(X[4:16], right) == ((NONE, NO_MATCH, 0, 0, 0, 0, 0), b"")                     # 8 bases shared: shift 4 > 3
    # 11 and 12 bases: 11 * 3 / 4 = 8 in int arithmetic (8.25 would refuse 8 shared bases)
    assert rec5(X[4:15], right) == ((MERGED, FOUND, SWAPPED, 8, 15, 0, 0), X[0:15])
    assert rec5(X[5:16], right) == ((NONE, NO_MATCH, 0, 0, 0, 0, 0), b"")


def test_of_two_candidate_shifts_the_smaller_wins():
    left, right = b"GATTACATTACA", b"TTACATTACAGG"                # right agrees with left at shift 2 (10 bases) and at shift 7 (5 bases)
    assert left[2:] == right[:10] and left[7:] == right[:5]
    assert rec5(left, right) == ((MERGED, FOUND, 0, 10, 14, 0, 0), b"GATTACATTACAGG")


def test_a_homopolymer_overlap_of_k_or_more_is_not_complex():
    left, right = b"CGTACAAAAAA", b"AAAAAAGTCCGT"                  # shift 5: six A; end = 6 - 5 + 1 = 2 and both k-mers are AAAAA
    assert rec5(left, right) == ((NONE, NO_COMPLEX, 0, 6, 0, 0, 0), b"")
    assert rec5(b"CGTACAAAAAAG", b"AAAAAAGTCCGT") == ((MERGED, FOUND, 0, 7, 17, 0, 0), b"CGTACAAAAAAGTCCGT")      # AAAAAAG: k-mer 2 is AAAAG


def test_a_valid_span_is_always_complex():
    """the first spanning k-mer is left's last k - 1 letters and right[o]: were it a homopolymer of X, left would end in k - 1 >= o + 1 X and
    right would begin with o + 1 X, so the reads would agree one shift earlier and share o + 1 letters.  The reference's null at :5044-5046
    is dead code for a valid span too (the device keeps the test; the random pairs below never reach it)."""
    left, right = b"CGTCAAAA", b"AAAATCGG"                         # meant to share AAA around the k-mer AAAAA: they share AAAA, and the span is empty
    assert rec5(left, right) == ((SPANNED, FOUND, 0, 4, 12, 4, 0), b"CGTCAAAATCGG")


# k = 8: the smallest overlap for which isRepeat can be false is 6 (t3 = round(o / 3 * 0.9) is 1 for o = 3 .. 5, t2 = 1 for o = 2 .. 3,
# t1 = 1 for o = 1), so the rescue needs k >= 7; with k = 8 and 6 bases shared there is one spanning k-mer
K8 = 8
L8, R8 = X[0:14], X[8:22]                                          # share X[8:14] = GGCAGT; the spanning k-mer is window 7 = X[7:15]
SPAN8 = X[7:15]
RIGHT_EDGE = [X[8 + i:16 + i] for i in range(6)]                   # right's k-mers i < min(6, 7)
LEFT_EDGE = [X[i:i + 8] for i in range(1, 7)]                      # left's k-mers i >= max(0, 7 - 6)


def rec8(g, left=L8, right=R8, mincov=1.0):
    return expected(left, right, K8, MO, mincov, g)


def test_is_repeat_thresholds():
    assert not is_repeat(b"GGCAGT")
    assert is_repeat(b"ACACAC") and is_repeat(b"CACACA") and is_repeat(b"ACGACG") and is_repeat(b"AAAAAG") and not is_repeat(b"AAAACG")
    assert all(is_repeat(X[i:i + n]) for n in range(1, 6) for i in range(10))            # up to 5 letters everything is a repeat
    assert jround(F32(5) * F32(0.9)) == 5 and jround(F32(6) * F32(0.9)) == 5 and jround(F32(2) * F32(0.9)) == 2
    for bad in (b"GGNAGT", b"GGcAGT"):
        try:
            is_repeat(bad); assert False
        except RepeatThrows:
            pass
    assert is_repeat(b"AAAAAN")                                     # five A reach t1 = 5 before the N is looked at
    big = b"A" * 141 + b"C" * 9                                     # t1 = 135 > 127: a Java byte never gets there; t2 = 68 is reached
    assert jround(F32(150) * F32(0.9)) == 135 and is_repeat(big) and jbyte_inc(127) == -128


def test_an_invalid_span_and_the_three_conditions_of_the_rescue_in_turn():
    base = [(X, 10)]
    assert rec8(DictGraph(K8, base)) == ((SPANNED, FOUND, 0, 6, 22, 7, 1), X[0:22])
    # the spanning k-mer below min_kmer_cov (absent: count 0; or count 1 against min_kmer_cov 2)
    g = DictGraph(K8, base, absent=[SPAN8])
    assert g.counts(X[0:22])[7] == 0
    assert rec8(g) == ((NONE, NO_RIGHT_SINGLETON, 0, 6, 0, 0, 0), b"")
    assert rec8(DictGraph(K8, base, extra={SPAN8: 1}), mincov=2.0) == ((NONE, NO_RIGHT_SINGLETON, 0, 6, 0, 0, 0), b"")
    # a singleton among right's first k-mers (each position in turn), none among left's last
    for km in RIGHT_EDGE:
        assert rec8(DictGraph(K8, base, extra={km: 1}, absent=[SPAN8])) == ((NONE, NO_LEFT_SINGLETON, 0, 6, 0, 0, 0), b"")
    assert rec8(DictGraph(K8, base, extra={X[14:22]: 1}, absent=[SPAN8]))[0][1] == NO_RIGHT_SINGLETON      # right's k-mer 6 is past min(o, nk)
    assert rec8(DictGraph(K8, base, extra={RIGHT_EDGE[0]: 1, X[0:8]: 1}, absent=[SPAN8]))[0][1] == NO_LEFT_SINGLETON      # left's k-mer 0 is before nk - o
    # both singletons, but the shared bases are a repeat: ACACAC
    Y = b"GATTCGGAACACACTGCCTAGT"
    ly, ry = Y[0:14], Y[8:22]
    gy = DictGraph(K8, [(Y, 10)], extra={Y[9:17]: 1, Y[2:10]: 1}, absent=[Y[7:15]])
    assert overlap_maximally(ly, ry, MO) == (Y, "loop-joined") and is_repeat(ry[:6])
    assert rec8(gy, ly, ry) == ((NONE, REPEAT, 0, 6, 0, 0, 0), b"")
    # all three hold: the pair is reported for the rescue, as it is before the mutation
    for rk in RIGHT_EDGE:
        for lk in LEFT_EDGE:
            assert rec8(DictGraph(K8, base, extra={rk: 1, lk: 1}, absent=[SPAN8])) == ((RESCUE, FOUND, 0, 6, 22, 7, 1), X[0:22])


def test_a_rescue_that_succeeds_with_its_mutation():
    g = DictGraph(K8, [(X, 10)], extra={RIGHT_EDGE[2]: 1, LEFT_EDGE[1]: 1}, absent=[SPAN8], d=3)
    del g.count[SPAN8]                                              # the counting filter has not seen it either
    before = set(g.dbg)
    r = overlap(L8, R8, K8, MO, 1.0, g, mutate=True)
    assert r.record() == ((RESCUE, FOUND, 0, 6, 22, 7, 1), X[0:22])
    assert g.dbg - before == {SPAN8} and g.counts(X[0:22])[7] == 1                         # addDbgOnly: the k-mer counts 1 from now on
    assert r.fixed == X[0:22]                                       # correctMismatches(threshold 2) finds no variant in the graph
    kms = [X[i:i + 8] for i in range(15)]
    assert g.pairs == set(zip(kms, kms[3:]))                        # addReadPairedKmers of the joined list
    # judged again the pair is an ordinary spanned overlap
    assert expected(L8, R8, K8, MO, 1.0, g) == ((SPANNED, FOUND, 0, 6, 22, 7, 1), X[0:22])


def test_case_and_other_letters_inside_the_overlap():
    def put(s, pos, ch):
        b = bytearray(s); b[pos] = ord(ch); return bytes(b)
    left, right = X[0:12], X[7:19]
    # the comparison is byte-exact: a lower-case letter on one side only is a mismatch
    assert rec5(left, put(right, 1, "g")) == ((NONE, NO_MATCH, 0, 0, 0, 0, 0), b"")
    both = rec5(put(left, 8, "g"), put(right, 1, "g"))
    assert both == ((MERGED, FOUND, 0, 5, 19, 0, 0), put(X[0:19], 8, "g"))
    # an N on both sides matches itself; the spanning window that holds it counts 0, and so do right's k-mers 0 and 1
    ln, rn = put(X[0:12], 10, "N"), put(X[9:21], 1, "N")
    g = DictGraph(K, [(X, 10)], extra={X[11:16]: 1})
    assert g.counts(ln + rn[3:])[8] == 0 and g.counts(rn)[:3] == [0, 0, 1]
    assert rec5(ln, rn, g) == ((NONE, NO_LEFT_SINGLETON, 0, 3, 0, 0, 0), b"")
    assert rec5(ln, rn, DictGraph(K, [(X, 10)])) == ((NONE, NO_RIGHT_SINGLETON, 0, 3, 0, 0, 0), b"")
    # k = 8, an N at base 2 of the six shared ones: right's k-mers 3 .. 5 and left's k-mers 1 .. 2 are free of it; with a singleton on each
    # side the reference reaches isRepeat(GGNAGT), which throws
    ln, rn = put(L8, 10, "N"), put(R8, 2, "N")
    g = DictGraph(K8, [(X, 10)], extra={R8[3:11]: 1, L8[1:9]: 1})
    assert g.counts(rn)[:6] == [0, 0, 0, 1, 10, 10] and g.counts(ln)[1:7] == [1, 10, 0, 0, 0, 0]
    assert rec8(g, ln, rn) == ((NONE, REPEAT_THROWS, 0, 6, 0, 0, 0), b"")


def test_short_reads():
    assert rec5(X[0:4], X[0:12]) == ((NONE, SHORT, 0, 0, 0, 0, 0), b"")
    assert rec5(X[0:12], X[0:6], mo=7) == ((NONE, SHORT, 0, 0, 0, 0, 0), b"")
    assert rec5(X[0:5], X[0:5])[0][:2] == (LEFT, FOUND)                                    # one k-mer each


class HashedCounts:
    """a graph whose counts are a fixed function of the k-mer: 0, 1, 2 or 7 — every branch of the small-overlap case is common"""
    def __init__(self, k):
        self.k = k

    def counts(self, seq):
        out = []
        for i in range(len(seq) - self.k + 1):
            w = seq[i:i + self.k]
            ok = all(ch in b"ACGTUacgtu" for ch in w)
            out.append(F32((0, 1, 1, 2, 7, 1)[zlib.crc32(w.translate(NORM)) % 6] if ok else 0))
        return out


def random_pairs(n, seed, k):
    rng = np.random.default_rng(seed)
    alphabets = (b"ACGT", b"ACGT", b"ACGT", b"AC", b"A", b"ACGTNa", b"AAAC")
    for _ in range(n):
        al = alphabets[int(rng.integers(0, len(alphabets)))]
        src = bytes(al[int(x)] for x in rng.integers(0, len(al), 48))
        if rng.random() < 0.3:                                      # a low-complexity stretch somewhere
            p = int(rng.integers(0, 36)); src = src[:p] + bytes([src[p]]) * 12 + src[p + 12:]
        a, c = int(rng.integers(0, 20)), int(rng.integers(0, 28))
        left, right = src[a:a + int(rng.integers(k, 28))], src[c:c + int(rng.integers(k, 20))]
        if rng.random() < 0.15:
            right = bytes(al[int(x)] for x in rng.integers(0, len(al), len(right)))
        if rng.random() < 0.1 and len(right) > 3:
            b = bytearray(right); b[int(rng.integers(0, len(b)))] = ord("G"); right = bytes(b)
        yield left, right, int(rng.integers(1, k + 2))


def test_twenty_thousand_random_pairs():
    """the smallest agreeing shift is what the indexOf loop finds; `left.contains(right)` (:1370) never answers once the loop has run; the
    no-complex-k-mer return after a rescue (:5044-5046) is never reached: a span of homopolymers makes the shared bases one letter, and
    isRepeat is true of (or throws on) any such string"""
    k = 8
    g = HashedCounts(k)
    seen, hows = {}, {}
    for left, right, mo in random_pairs(20_000, 1, k):
        if min(len(left), len(right)) < max(k, mo):
            continue
        for a, b, m in ((left, right, mo), (right, left, max(mo, min(len(left), len(right)) * 3 // 4))):
            got, how = overlap_maximally(a, b, m)
            assert got == smallest_agreeing_shift(a, b, m), (a, b, m)
            assert how != "left-contains-right", (a, b, m)
            hows[how] = hows.get(how, 0) + 1
        r = overlap(left, right, k, mo, 1.0, g)
        assert r.outcome != MUTATED_THEN_NULL, (left, right, mo)
        assert not (r.why == NO_COMPLEX and r.overlap < k), (left, right, mo)
        seen[(r.outcome, r.why, r.swapped)] = seen.get((r.outcome, r.why, r.swapped), 0) + 1
    assert all(hows.get(h, 0) > 20 for h in ("loop-contained", "loop-joined", "right-contains-left", None)), hows
    for key in ((NONE, NO_MATCH, False), (LEFT, FOUND, False), (RIGHT, FOUND, False), (MERGED, FOUND, False), (MERGED, FOUND, True),
                (SPANNED, FOUND, False), (RESCUE, FOUND, False), (NONE, NO_COMPLEX, False), (NONE, NO_RIGHT_SINGLETON, False),
                (NONE, NO_LEFT_SINGLETON, False), (NONE, REPEAT, False), (NONE, REPEAT_THROWS, False)):
        assert seen.get(key, 0) > 0, (key, seen)


# ---- the feature exists at every layer (these fail before it does) ----
def test_header_declares_the_entry_point():
    src = open(os.path.join(ROOT, "include", "rb_capi.h")).read()
    assert re.search(r"\bint rb_graph_overlap_pairs\(rb_graph \*g, const char \*lseq, const int64_t \*loffsets, const char \*rseq, const int64_t "
                     r"\*roffsets, int64_t n,\s*int min_overlap, float min_kmer_cov, int64_t \*out_offsets, char \*out_seq, rb_overlap_rec \*recs\);", src)
    assert "GraphUtils.java:4898-5063" in src
    for i, name in enumerate(("NONE", "LEFT", "RIGHT", "MERGED", "SPANNED", "RESCUE")):
        assert re.search(r"\bRB_OVL_%s = %d\b" % (name, i), src), name
    for i, name in enumerate(("FOUND", "NO_MATCH", "NO_COMPLEX", "NO_RIGHT_SINGLETON", "NO_LEFT_SINGLETON", "REPEAT", "SHORT", "REPEAT_THROWS")):
        assert re.search(r"\bRB_OVL_WHY_%s = %d\b" % (name, i), src), name


def test_library_exports_and_python_binds_it():
    import ctypes as C
    from rnabloom import _native as N
    assert hasattr(C.CDLL(N.LIB_PATH), "rb_graph_overlap_pairs")
    assert "rb_graph_overlap_pairs" in {s[0] for s in N.SYMBOLS}
    from rnabloom.graph import BloomFilterDeBruijnGraph as G
    for name in ("overlapPairsFlat", "overlapPairs", "applyOverlapRescue"):
        assert callable(getattr(G, name, None)), name
    assert G.OVL_DTYPE.itemsize == 32 and G.OVL_DTYPE.names[:3] == ("outcome", "why", "flags")
    assert (G.OVL_NONE, G.OVL_LEFT, G.OVL_RIGHT, G.OVL_MERGED, G.OVL_SPANNED, G.OVL_RESCUE) == (NONE, LEFT, RIGHT, MERGED, SPANNED, RESCUE)
    assert G.OVL_WHYS.index("repeat_throws") == REPEAT_THROWS and G.OVL_WHYS.index("short") == SHORT


def test_java_and_jni_sides_exist():
    java = open(os.path.join(ROOT, "java", "rnabloom", "graph", "NativeGraph.java")).read()
    assert re.search(r"public static native int overlapPairs\(long h, ByteBuffer lseq, long\[\] loffsets, ByteBuffer rseq, long\[\] roffsets, int n,", java)
    jni = open(os.path.join(ROOT, "jni", "rb_jni.c")).read()
    assert "FN(overlapPairs)" in jni and "rb_graph_overlap_pairs(" in jni
    g = open(os.path.join(ROOT, "java", "rnabloom", "graph", "BloomFilterDeBruijnGraph.java")).read()
    assert "NativeGraph.overlapPairs(handle" in g
