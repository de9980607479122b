"""The rules of rb_graph_correct_mismatches restated in Python from the reference's Java, and checked on hand-worked cases over a
dictionary graph.  tests/test_gpu_mismatch_correction.py applies the same restatement to the CPU oracle's getKmers / contains.

  GraphUtils.correctMismatches (R/util/GraphUtils.java:3914-3996): the forward scan :3926-3958, the reverse scan :3960-3993;
  getMedianKmerCoverage(kmers, start, end) :208-217 (end exclusive), getMinMedMaxKmerCoverage :219-227 over Common.getMedian /
  getMinMedMax (R/util/Common.java:41-50, 74-83); BloomFilterDeBruijnGraph.getRightVariants(String) :1109-1120 and
  getLeftVariants(String) :1056-1068 over SeqUtils.getAltNucleotides (R/util/SeqUtils.java:147-162).
The graph is two callbacks: contains(kmer bytes) -> bool (graph.contains: dbgbf alone) and counts(sequence bytes) -> the counts of
graph.getKmers(sequence) (every window; 0 for a window with a letter outside ACGTU).  The last part of the file checks that the
feature exists at every layer: header, library, Python class."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def alt_nucleotides(ch):
    """SeqUtils.getAltNucleotides(char) :147-162: upper-case letters only; U has T's alternatives; anything else gets all four"""
    return {ord("A"): b"CGT", ord("C"): b"AGT", ord("G"): b"ACT", ord("T"): b"ACG", ord("U"): b"ACG"}.get(ch, b"ACGT")


def median(values):
    """Common.getMedian :41-50 in float32"""
    a = sorted(F32(v) for v in values)
    half = len(a) // 2
    if len(a) % 2 == 0:
        return F32(F32(a[half - 1] + a[half]) / F32(2.0))
    return a[half]


def correct_mismatches(seq, counts0, k, cov_threshold, min_kmer_cov, contains, counts):
    """correctMismatches(kmers, graph, covThreshold, minKmerCov) on the k-mer list of `seq` (counts0 = its getKmers counts).  The list
    of Kmer objects is the pair (s, c): s the bases the k-mers spell, c their counts.  Returns (bytes, number of replacements, counts)."""
    s, c = bytearray(seq), [F32(x) for x in counts0]
    num_kmers = len(c)
    T, mincov = F32(cov_threshold), F32(min_kmer_cov)
    n_fixed = 0
    for i in range(1, num_kmers - k):                                       # :3926
        if c[i] < T and c[i - 1] >= T and c[i + k] >= T:                   # :3928-3932
            tail = bytes(s[i + k:i + 2 * k - 1])                            # graph.getPrefix(right.toString())
            best_alt = None
            best_cov = median(c[i:i + k - 1])                               # getMedianKmerCoverage(kmers, i, i+k-1): k - 1 counts
            kmer = bytes(s[i:i + k])
            for a in alt_nucleotides(kmer[k - 1]):                          # getRightVariants(kmer.toString())
                var = kmer[:k - 1] + bytes([a])
                if not contains(var):
                    continue
                alt_counts = [F32(x) for x in counts(var + tail)]
                if alt_counts:
                    if min(alt_counts) >= mincov and median(alt_counts) > best_cov:
                        best_cov = median(alt_counts)
                        best_alt = (a, alt_counts)
            if best_alt is not None:
                s[i + k - 1] = best_alt[0]
                c[i:i + k] = best_alt[1]                                    # kmers.set(i+j, bestAlt.get(j)), j < k
                n_fixed += 1
    for i in range(num_kmers - 2, k - 1, -1):                               # :3960
        if c[i] < T and c[i + 1] >= T and c[i - k] >= T:                   # :3962-3966
            head = bytes(s[i - k + 1:i])                                    # graph.getSuffix(left.toString())
            best_alt = None
            best_cov = median(c[i - k + 1:i])                               # getMedianKmerCoverage(kmers, i-k+1, i)
            kmer = bytes(s[i:i + k])
            for a in alt_nucleotides(kmer[0]):                              # getLeftVariants(kmer.toString())
                var = bytes([a]) + kmer[1:]
                if not contains(var):
                    continue
                alt_counts = [F32(x) for x in counts(head + var)]
                if alt_counts:
                    if min(alt_counts) >= mincov and median(alt_counts) > best_cov:
                        best_cov = median(alt_counts)
                        best_alt = (a, alt_counts)
            if best_alt is not None:
                s[i] = best_alt[0]
                c[i - k + 1:i + 1] = best_alt[1]
                n_fixed += 1
    return bytes(s), n_fixed, np.array(c, np.float32)


def forward_only(seq, counts0, k, cov_threshold, min_kmer_cov, contains, counts):
    """the forward scan alone (what the sequence looks like when the reverse scan starts): correct_mismatches on a list whose reverse
    scan has no position — used by the tests to tell which scan made a replacement"""
    s, c = bytearray(seq), [F32(x) for x in counts0]
    T, mincov = F32(cov_threshold), F32(min_kmer_cov)
    n_fixed = 0
    for i in range(1, len(c) - k):
        if c[i] < T and c[i - 1] >= T and c[i + k] >= T:
            tail, kmer = bytes(s[i + k:i + 2 * k - 1]), bytes(s[i:i + k])
            best_alt, best_cov = None, median(c[i:i + k - 1])
            for a in alt_nucleotides(kmer[k - 1]):
                var = kmer[:k - 1] + bytes([a])
                if contains(var):
                    ac = [F32(x) for x in counts(var + tail)]
                    if ac and min(ac) >= mincov and median(ac) > best_cov:
                        best_cov, best_alt = median(ac), (a, ac)
            if best_alt is not None:
                s[i + k - 1] = best_alt[0]; c[i:i + k] = best_alt[1]; n_fixed += 1
    return bytes(s), n_fixed


# ---- a dictionary graph: k = 5, counts by k-mer (upper case, U as T), dbgbf membership kept apart from the counts ----
K = 5
NORM = bytes.maketrans(b"acgtuU", b"ACGTTT")


class DictGraph:
    def __init__(self, paths, extra=None, absent=()):
        """paths: [(sequence, count)] whose k-mers get that count (a k-mer of several paths: the sum); extra: {k-mer: count};
        absent: k-mers taken out of dbgbf while keeping their count"""
        self.count = {}
        for seq, cov in paths:
            for i in range(len(seq) - K + 1):
                km = seq[i:i + K].translate(NORM)
                self.count[km] = self.count.get(km, 0) + cov
        self.count.update(extra or {})
        self.dbg = set(self.count) - set(absent)

    def contains(self, kmer):
        return kmer.translate(NORM) in self.dbg

    def counts(self, seq):
        out = []
        for i in range(len(seq) - K + 1):
            w = seq[i:i + K]
            ok = all(ch in b"ACGTUacgtu" for ch in w)
            km = w.translate(NORM)
            out.append(F32(self.count.get(km, 0) if ok and km in self.dbg else 0))       # getCount: 0 unless dbgbf has it
        return out

    def run(self, seq, T, mincov=1.0):
        return correct_mismatches(seq, self.counts(seq), K, T, mincov, self.contains, self.counts)


TRUE = b"ACGATCTTGGCAGTACCGTTAGGATCCA"       # 28 bases, 24 distinct 5-mers


def sub(seq, pos, base):
    b = bytearray(seq); b[pos] = ord(base); return bytes(b)


def test_the_true_sequence_has_distinct_kmers():
    kms = [TRUE[i:i + K] for i in range(len(TRUE) - K + 1)]
    assert len(set(kms)) == len(kms) == 24


def test_one_substitution_in_the_middle_is_replaced_and_the_counts_follow():
    g = DictGraph([(TRUE, 10)])
    bad = sub(TRUE, 12, "T")                                  # G -> T at 12: windows 8..12 count 0; forward candidate i = 8
    assert g.counts(bad)[7:14] == [10, 0, 0, 0, 0, 0, 10]
    out, n, c = g.run(bad, 5.0)
    assert (out, n) == (TRUE, 1) and (c == 10).all()
    assert list(c) == g.counts(out)                           # the final rows are getKmers of the output
    assert g.run(TRUE, 5.0)[:2] == (TRUE, 0)                  # nothing below the threshold: untouched
    assert g.run(bad, 0.0)[:2] == (bad, 0) and g.run(bad, -1.0)[:2] == (bad, 0)        # T <= 0: no count is below it


def test_boundaries_of_both_scans():
    g = DictGraph([(TRUE, 10)])
    nk = len(TRUE) - K + 1                                     # 24: forward i = 1 .. 18, reverse i = 23 - 1 .. 5
    # an error at base m zeroes windows m-4 .. m; forward candidate i = m - 4, reverse candidate i = m: both want 5 <= m <= 22
    for m, fixed in ((4, False), (5, True), (6, True), (nk - K + 3, True), (nk - K + 4, False)):
        bad = sub(TRUE, m, "A" if TRUE[m:m + 1] != b"A" else "C")
        out, n, _ = g.run(bad, 5.0)
        assert (out == TRUE, n) == (fixed, 1 if fixed else 0), m
        fo, fn = forward_only(bad, g.counts(bad), K, 5.0, 1.0, g.contains, g.counts)
        assert fn == n                                         # a clean single error is always the forward scan's
    # i = 1 is the first forward position (m = 5) and i = nk - k - 1 the last (m = nk - k + 3 = 22): both taken above.
    # nk = k + 1: range(1, 1) and range(k - 1, k - 1, -1) are empty
    short = TRUE[:2 * K]
    assert len(g.counts(short)) == K + 1
    assert g.run(sub(short, 5, "A"), 5.0)[:2] == (sub(short, 5, "A"), 0)
    # nk = k + 2: forward i = 1 only (replaces base k = 5), reverse i = k only (replaces base 5 as well)
    s12 = TRUE[:2 * K + 2]
    assert g.run(sub(s12, 5, "A"), 5.0)[:2] == (s12, 1)
    assert g.run(sub(s12, 6, "A"), 5.0)[:2] == (s12, 1)       # forward i = 2 > nk - k - 1 = 1: the reverse scan's (i = nk - 2 = 6 ... k)


def test_reverse_boundaries_i_equals_k_and_nk_minus_2():
    """a replacement only the reverse scan can make: the first window that holds the error is solid by itself (another source put that
    k-mer in the graph), so the forward candidate is one window late, points at the wrong base and finds nothing"""
    for m in (5, len(TRUE) - K + 1 - 2):                      # reverse i = k and i = nk - 2 = 22
        base = "A" if TRUE[m:m + 1] != b"A" else "C"
        bad = sub(TRUE, m, base)
        g = DictGraph([(TRUE, 10)], extra={bad[m - 4:m + 1]: 7})
        c0 = g.counts(bad)
        assert c0[m - 4] == 7 and c0[m - 3:m + 1] == [0, 0, 0, 0]
        fo, fn = forward_only(bad, c0, K, 5.0, 1.0, g.contains, g.counts)
        assert (fo, fn) == (bad, 0)
        out, n, c = g.run(bad, 5.0)
        assert (out, n) == (TRUE, 1) and list(c) == g.counts(TRUE)


def test_the_baseline_is_the_median_of_k_minus_1_windows():
    """candidate i = 8 (error at 12).  Three of the erroneous k-mers exist thinly: the current windows 8 .. 12 count 0 0 3 3 3.  The
    true path is thin there too: the variant's five windows count 10 10 2 2 2, median 2.  The reference's baseline is the median of the
    first FOUR current windows, (0 + 3) / 2 = 1.5, so the variant wins (2 > 1.5); the median of all five, 3, would have kept the error."""
    bad = sub(TRUE, 12, "T")
    thin = {TRUE[i:i + K]: 2 for i in (10, 11, 12)}
    err = {bad[i:i + K]: 3 for i in (10, 11, 12)}
    g = DictGraph([(TRUE, 10)], extra={**thin, **err})
    c0 = g.counts(bad)
    assert c0[8:13] == [0, 0, 3, 3, 3] and g.counts(TRUE)[8:13] == [10, 10, 2, 2, 2]
    assert median(c0[8:12]) == 1.5 and median(c0[8:13]) == 3
    # T = 5: windows 10 .. 12 (count 3) are below it as well; candidate i = 8 has c[7] = 10, c[13] = 10
    out, n, c = g.run(bad, 5.0)
    assert (out, n) == (TRUE, 1) and list(c[8:13]) == [10, 10, 2, 2, 2]
    # min_kmer_cov = 3: the variant is in dbgbf but its windows fail the minimum (2 < 3): nothing happens in either scan
    assert g.run(bad, 5.0, 3.0)[:2] == (bad, 0)


def test_strictly_greater_and_the_first_of_equal_medians():
    """error at 12 (G -> T); besides the true G path a second path through A at 12 with the same counts: alternatives of T are tried in
    the order A C G, A comes first and G's equal median does not displace it.  A variant whose median only equals the baseline loses."""
    other = sub(TRUE, 12, "A")
    g = DictGraph([(TRUE, 10)], extra={other[i:i + K]: 10 for i in range(8, 13)})
    bad = sub(TRUE, 12, "T")
    assert g.run(bad, 5.0)[:2] == (other, 1)
    g2 = DictGraph([(TRUE, 10)], extra={other[i:i + K]: 11 for i in range(8, 13)})
    assert g2.run(sub(TRUE, 12, "C"), 5.0)[:2] == (other, 1)              # alternatives of C: A G T — the better median wins wherever it stands
    g3 = DictGraph([(TRUE, 10)], extra={other[i:i + K]: 9 for i in range(8, 13)})
    assert g3.run(bad, 5.0)[:2] == (TRUE, 1)                               # A (9) first, then G (10 > 9) displaces it
    # equal to the baseline: current windows count 4 (below T = 5), the variant's windows 4 as well
    flat = DictGraph([(TRUE[:8 + K - 1], 10), (TRUE[13:], 10)], extra={**{TRUE[i:i + K]: 4 for i in range(8, 13)}, **{bad[i:i + K]: 4 for i in range(8, 13)}})
    assert flat.counts(bad)[7:14] == [10, 4, 4, 4, 4, 4, 10]
    assert flat.run(bad, 5.0)[:2] == (bad, 0)


def test_alternatives_of_other_letters():
    g = DictGraph([(TRUE, 10)])
    for ch in "NnRy-":                                         # not ACGTU: window counts 0, all four alternatives, G found
        assert g.run(sub(TRUE, 12, ch), 5.0)[:2] == (TRUE, 1), ch
    # U is T to the hash and to the alternatives: a U where the truth is T is no error at all; a U where it is G is replaced
    assert TRUE[7:8] == b"T" and g.run(sub(TRUE, 7, "U"), 5.0)[:2] == (sub(TRUE, 7, "U"), 0)
    assert g.run(sub(TRUE, 12, "U"), 5.0)[:2] == (TRUE, 1)
    assert alt_nucleotides(ord("U")) == b"ACG" and alt_nucleotides(ord("T")) == b"ACG" and alt_nucleotides(ord("N")) == b"ACGT"
    # a lower-case letter hashes like its upper case but is "another letter" to getAltNucleotides: all four, its own upper case included.
    # With the true path thin (4 < T) a lower-case g at 12 is a candidate and `G` itself is among the alternatives: its 5 windows have
    # median 4 against the baseline of 4 windows, 4: not strictly better, nothing happens ...
    thin = DictGraph([(TRUE[:8 + K - 1], 10), (TRUE[13:], 10)], extra={TRUE[i:i + K]: 4 for i in range(8, 13)})
    low = sub(TRUE, 12, "g")
    assert thin.counts(low)[7:14] == [10, 4, 4, 4, 4, 4, 10] and thin.run(low, 5.0)[:2] == (low, 0)
    # ... unless the fifth window lifts the median of five above the median of four: counts 4 4 6 6 6 -> four windows 5, five windows 6
    lift = DictGraph([(TRUE[:8 + K - 1], 10), (TRUE[13:], 10)], extra={TRUE[i:i + K]: (4 if i < 10 else 6) for i in range(8, 13)})
    assert lift.counts(low)[8:13] == [4, 4, 6, 6, 6]
    assert lift.run(low, 7.0)[:2] == (TRUE, 1)                 # g -> G: the k - 1 window at work again


def test_contains_decides_not_the_count():
    """a variant k-mer that has counts but is not in dbgbf is not tried (getRightVariants: contains); with min_kmer_cov = 0 a variant
    whose other windows are missing is accepted as long as the variant k-mer itself is in dbgbf"""
    bad = sub(TRUE, 12, "T")
    # the forward variant k-mer is window 8 of the truth (it ends with the replaced base), the reverse one window 12 (it starts with it)
    g = DictGraph([(TRUE, 10)], absent=[TRUE[8:8 + K]])
    assert g.counts(TRUE)[8] == 0
    assert g.run(bad, 5.0)[:2] == (bad, 0)                     # min 0 < 1 in both scans
    out, n, c = g.run(bad, 5.0, 0.0)                           # minimum 0 is fine now: forward refused at the gate, reverse accepted
    assert forward_only(bad, g.counts(bad), K, 5.0, 0.0, g.contains, g.counts) == (bad, 0)
    assert (out, n) == (TRUE, 1) and list(c[8:13]) == [0, 10, 10, 10, 10]
    g = DictGraph([(TRUE, 10)], absent=[TRUE[8:8 + K], TRUE[12:12 + K]])
    assert g.run(bad, 5.0, 0.0)[:2] == (bad, 0)                # both gates shut although three windows of the variant count 10


def test_a_second_replacement_that_needs_the_first():
    """error at 8 (windows 4 .. 8 zero); the true window 8 is thin (count 2 < T) and a richer path leaves it through base 12.  The first
    replacement (i = 4: windows 4 .. 8 become 10 10 10 10 2) makes c[7] solid, and only then is i = 8 a candidate of the same forward
    scan: its baseline is the median of 2 10 10 10, the alternative's five windows count 20"""
    alt12 = sub(TRUE, 12, "A")                                 # G -> A at 12: windows 8 .. 12 of the richer path
    extra = {TRUE[8:8 + K]: 2, **{alt12[i:i + K]: 20 for i in range(8, 13)}}
    g = DictGraph([(TRUE, 10)], extra=extra)
    bad = sub(TRUE, 8, "A")
    c0 = g.counts(bad)
    assert c0[3:14] == [10, 0, 0, 0, 0, 0, 10, 10, 10, 10, 10]
    out, n, c = g.run(bad, 5.0)
    assert (out, n) == (alt12, 2) and list(c[4:14]) == [10] * 4 + [20] * 5 + [10]
    assert forward_only(bad, c0, K, 5.0, 1.0, g.contains, g.counts) == (alt12, 2)
    # without the first replacement (its k-mers taken out of dbgbf) position 8 never has a solid left neighbour
    g0 = DictGraph([(TRUE, 10)], extra=extra, absent=[TRUE[i:i + K] for i in range(4, 8)])
    assert g0.run(bad, 5.0)[:2] == (bad, 0)


def test_two_errors_within_k_stay():
    g = DictGraph([(TRUE, 10)])
    bad = sub(sub(TRUE, 10, "A"), 13, "C")                     # each one's solid neighbour is the other one's ruin
    assert g.run(bad, 5.0)[:2] == (bad, 0)
    far = sub(sub(TRUE, 8, "A"), 14, "C")                      # k + 1 apart: independent, both replaced by the forward scan
    assert g.run(far, 5.0)[:2] == (TRUE, 2)


# ---- the feature exists at every layer (these fail before it does) ----
def test_header_declares_the_entry_point():
    src = open(os.path.join(ROOT, "include", "rb_capi.h")).read()
    assert re.search(r"\bint rb_graph_correct_mismatches\(rb_graph \*g, const char \*seq, const int64_t \*offsets, int64_t n,\s*const float "
                     r"\*cov_threshold, float min_kmer_cov,\s*char \*out_seq, int32_t \*n_fixed, int64_t \*koffsets, float \*counts\);", src)
    assert "GraphUtils.java:3914-3996" in src


def test_library_exports_and_python_binds_it():
    import ctypes as C
    from rnabloom import _native as N
    assert hasattr(C.CDLL(N.LIB_PATH), "rb_graph_correct_mismatches")
    assert "rb_graph_correct_mismatches" in {s[0] for s in N.SYMBOLS}
    from rnabloom.graph import BloomFilterDeBruijnGraph
    assert callable(getattr(BloomFilterDeBruijnGraph, "correctMismatchesFlat", None))
    assert callable(getattr(BloomFilterDeBruijnGraph, "correctMismatches", None))


def test_java_and_jni_sides_exist():
    java = open(os.path.join(ROOT, "java", "rnabloom", "graph", "NativeGraph.java")).read()
    assert re.search(r"public static native void correctMismatches\(long h, ByteBuffer seq, long\[\] offsets, int n, float\[\] covThreshold,", java)
    jni = open(os.path.join(ROOT, "jni", "rb_jni.c")).read()
    assert "FN(correctMismatches)" in jni and "rb_graph_correct_mismatches(" in jni
    g = open(os.path.join(ROOT, "java", "rnabloom", "graph", "BloomFilterDeBruijnGraph.java")).read()
    assert "NativeGraph.correctMismatches(handle" in g
