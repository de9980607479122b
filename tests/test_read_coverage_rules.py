"""The rules of rb_graph_read_coverage restated in Python from the reference's Java, in the sorted-array form the reference runs them in,
and checked against hand-worked cases.  tests/test_gpu_read_coverage.py applies the same restatement to the oracle's count rows.

  getCoverageStats (R/util/GraphUtils.java:1799-1845), correctErrorsSE's threshold search (:4007-4034), correctErrorsPE's first-round
  search (:4063-4125) and pair rule (:4126-4142), the solid count and windows of correctLongSequenceWindowed (:3099-3140),
  SeqUtils.isRepeat (R/util/SeqUtils.java:458-497).
Java float arithmetic is float32 with one rounding per operation; Math.round(float) is floor(x + 1/2) taken exactly."""
import math

import numpy as np
import pytest

F = np.float32
FIELDS = ("n", "n_solid", "n_complex", "flags", "min", "q1", "median", "q3", "max", "dropoff", "se_threshold", "pe_threshold")
SE_FOUND, PE_FOUND = 1, 2


def java_round(x):
    """Math.round(float): floor(x + 0.5) of the float32 value, exactly (a double holds every float + 0.5 used here)"""
    return int(math.floor(float(F(x)) + 0.5))


def fmul(a, b):
    return F(F(a) * F(b))


def walk(covs, start, g, strict):
    """the downward threshold walk both correctors run: (found, threshold)"""
    thr = covs[start]
    for i in range(start - 1, -1, -1):
        c = covs[i]
        t = fmul(thr, g)
        if (t > c) if strict else (t >= c):
            return True, thr
        thr = c
    return False, thr


def coverage_stats(counts, lookahead, g, fpr, min_cov, mate_n=None, n_complex=0):
    """the record of one segment: counts in window order; mate_n = the other mate's k-mer count (PE fields), None without mates"""
    covs = sorted(F(c) for c in counts)
    n = len(covs)
    r = dict.fromkeys(FIELDS, 0)
    for f in FIELDS[4:]:
        r[f] = F(0)
    r["n"] = n
    r["n_complex"] = n_complex
    if n == 0:
        return r
    r["n_solid"] = sum(1 for c in covs if c >= F(min_cov))
    half, q1i = n // 2, n // 4
    q3i = half + q1i
    r["min"], r["max"] = covs[0], covs[-1]
    r["median"] = F(F(covs[half - 1] + covs[half]) / F(2)) if n % 2 == 0 else covs[half]
    if n % 4 == 0:
        r["q1"] = F(F(covs[q1i - 1] + covs[q1i]) / F(2))
        r["q3"] = F(F(covs[q3i - 1] + covs[q3i]) / F(2))
    else:
        r["q1"], r["q3"] = covs[q1i], covs[q3i]
    if n >= lookahead:
        found, last = walk(covs, n - lookahead, g, True)
        r["dropoff"] = last if found else F(0)
    start = n - 1 - java_round(fmul(F(n), fpr))
    if start >= 0:
        found, r["se_threshold"] = walk(covs, start, g, True)
        r["flags"] |= SE_FOUND if found else 0
    if mate_n is not None:
        nfp = java_round(fmul(F(max(n, mate_n)), fpr))
        start = n - 1
        if start > nfp:
            start -= nfp
        found, r["pe_threshold"] = walk(covs, start, g, False)
        r["flags"] |= PE_FOUND if found else 0
    return r


def pair_threshold(left, right):
    """correctErrorsPE's threshold for the pair, -1 when there is none"""
    lf, rf = bool(left["flags"] & PE_FOUND), bool(right["flags"] & PE_FOUND)
    lt, rt = left["pe_threshold"], right["pe_threshold"]
    if lf and rf:
        return min(lt, rt)
    if lf:
        return lt if lt <= rt else F(-1)
    if rf:
        return rt if rt <= lt else F(-1)
    return F(-1)


_NUC = {ord(c): i for i, c in enumerate("ACGT")}
_NUC[ord("U")] = 3


def is_repeat(kmer):
    """SeqUtils.isRepeat on upper-case bases (U counts as T)"""
    b = [_NUC[c] for c in kmer.upper()]
    L = len(b)
    t1 = java_round(fmul(F(L), F(0.9)))
    nf1 = [0] * 4
    for x in b:
        nf1[x] += 1
        if nf1[x] >= t1:
            return True
    t2 = java_round(fmul(F(L // 2), F(0.9)))
    for start in range(2):
        nf2 = {}
        for i in range(start, L - 1, 2):
            key = (b[i], b[i + 1])
            nf2[key] = nf2.get(key, 0) + 1
            if nf2[key] >= t2:
                return True
    t3 = java_round(fmul(F(L // 3), F(0.9)))
    for start in range(3):
        nf3 = {}
        for i in range(start, L - 2, 3):
            key = (b[i], b[i + 1], b[i + 2])
            nf3[key] = nf3.get(key, 0) + 1
            if nf3[key] >= t3:
                return True
    return False


USABLE = set(b"ACGTUacgtu")


def complex_windows(read, k):
    """windows of getKmers(read) whose bases are all usable and not a repeat"""
    return sum(1 for p in range(len(read) - k + 1)
               if all(c in USABLE for c in read[p:p + k]) and not is_repeat(read[p:p + k]))


def windows(nk, W):
    """[start, end) of the windows of correctLongSequenceWindowed's first pass over nk k-mers"""
    out, i, shift = [], 0, W // 2
    while i < nk:
        end = min(i + W, nk)
        if end + shift >= nk:
            end = nk
        out.append((i, end))
        i = end
    return out


def expected_records(rows, reads, k, lookahead, g, fpr, min_cov, window=0, mate_rows=None, mate_reads=None):
    """records of a whole call (reads mode, windows mode, or reads + mates), and the seg_offsets it reports"""
    recs, so = [], [0]
    for i, row in enumerate(rows):
        if window:
            for a, b in windows(len(row), window):
                recs.append(coverage_stats(row[a:b], lookahead, g, fpr, min_cov))
        else:
            mn = len(mate_rows[i]) if mate_rows is not None else None
            recs.append(coverage_stats(row, lookahead, g, fpr, min_cov, mn, complex_windows(reads[i], k)))
        so.append(len(recs))
    if mate_rows is not None:
        for i, row in enumerate(mate_rows):
            recs.append(coverage_stats(row, lookahead, g, fpr, min_cov, len(rows[i]), complex_windows(mate_reads[i], k)))
    return recs, so


# ---- hand-worked cases ----
def rec(counts, lookahead=1, g=0.5, fpr=0.0, min_cov=1.0, mate_n=None):
    return coverage_stats(counts, lookahead, F(g), F(fpr), min_cov, mate_n)


def test_empty_segment_is_all_zero():
    r = rec([], mate_n=5)
    assert all(r[f] == 0 for f in FIELDS)


def test_one_two_three_windows():
    r = rec([5], mate_n=1)
    assert (r["min"], r["q1"], r["median"], r["q3"], r["max"]) == (5, 5, 5, 5, 5)
    assert r["dropoff"] == 0 and r["se_threshold"] == 5 and r["pe_threshold"] == 5 and r["flags"] == 0
    r = rec([9, 3], mate_n=2)
    assert (r["min"], r["q1"], r["median"], r["q3"], r["max"]) == (3, 3, 6, 9, 9)
    assert r["dropoff"] == 9 and r["se_threshold"] == 9 and r["pe_threshold"] == 9 and r["flags"] == SE_FOUND | PE_FOUND
    assert rec([9, 3], lookahead=2)["dropoff"] == 0
    r = rec([2, 10, 2])
    assert (r["min"], r["q1"], r["median"], r["q3"], r["max"]) == (2, 2, 2, 2, 10)
    assert r["se_threshold"] == 10 and r["flags"] == SE_FOUND


def test_four_five_eight_windows():
    r = rec([4, 1, 8, 4], mate_n=4)
    assert (r["min"], r["q1"], r["median"], r["q3"], r["max"]) == (1, 2.5, 4, 6, 8)
    # SE's strict `>` walks through the tie 4, 4 and stops at 4 * 0.5 > 1; PE's `>=` stops at the tie 8 * 0.5 >= 4
    assert r["se_threshold"] == 4 and r["pe_threshold"] == 8 and r["dropoff"] == 4
    r = rec([1, 1, 1, 2, 3])
    assert (r["min"], r["q1"], r["median"], r["q3"], r["max"]) == (1, 1, 1, 2, 3)
    r = rec([0, 5, 2, 17, 3, 9, 0, 5], fpr=0.25, min_cov=3)
    assert (r["min"], r["q1"], r["median"], r["q3"], r["max"]) == (0, 1, 4, 7, 17)
    assert r["n_solid"] == 5
    assert r["se_threshold"] == 2 and r["flags"] == SE_FOUND          # nFP = 2: from covs[5] = 5 down to 2 * 0.5 > 0


def test_all_counts_equal_and_gradient_one():
    r = rec([7] * 5, g=1.0, mate_n=5)
    assert r["flags"] == PE_FOUND and r["se_threshold"] == 7 and r["pe_threshold"] == 7 and r["dropoff"] == 0
    r = rec([7] * 5, g=0.5, mate_n=5)
    assert r["flags"] == 0 and r["se_threshold"] == 7 and r["pe_threshold"] == 7
    r = rec([3, 3, 5, 5], g=1.0, mate_n=4)                            # ties end both walks at once: 5 * 1 >= 5, and 5 * 1 > 3
    assert r["se_threshold"] == 5 and r["pe_threshold"] == 5 and r["flags"] == SE_FOUND | PE_FOUND
    assert rec([0, 0, 0], g=1.0, mate_n=3)["flags"] == PE_FOUND       # 0 * g >= 0


def test_false_positive_allowance_at_and_beyond_n():
    r = rec([1, 2, 3], fpr=1.0, mate_n=3)
    assert r["se_threshold"] == 0 and not r["flags"] & SE_FOUND       # start = 3 - 1 - 3 < 0
    assert r["pe_threshold"] == 2 and r["flags"] & PE_FOUND           # PE subtracts nFP only while n - 1 > nFP: start stays 2
    r = rec([1, 2, 3], fpr=0.5, mate_n=10)                            # PE: nFP = round(10 * 0.5) = 5 >= n - 1
    assert r["pe_threshold"] == 2 and r["flags"] & PE_FOUND


def test_lookahead_longer_than_segment():
    assert rec([1, 9, 9], lookahead=4)["dropoff"] == 0
    assert rec([1, 9, 9], lookahead=3)["dropoff"] == 0                # start at covs[0]: nothing below it
    assert rec([1, 9, 9], lookahead=2)["dropoff"] == 9


def test_java_round_at_one_half():
    assert [java_round(x) for x in (0.5, 1.5, 2.5, -0.5, -1.5, 0.49999997)] == [1, 2, 3, 0, -1, 0]
    assert java_round(fmul(F(5), F(0.1))) == 1 and java_round(fmul(F(5), F(0.3))) == 2
    assert java_round(fmul(F(25), F(0.9))) == 23                       # 25 * 0.9f rounds to 22.5 in float32
    assert rec([1, 2, 3, 4, 5], g=1.0, fpr=0.1)["se_threshold"] == 4    # nFP = round(0.5) = 1: the walk starts at covs[3]
    assert rec([1, 2, 3, 4, 5], g=1.0, fpr=0.09)["se_threshold"] == 5


@pytest.mark.parametrize("k,t", [(25, (23, 11, 7)), (31, (28, 14, 9)), (63, (57, 28, 19)), (64, (58, 29, 19)), (127, (114, 57, 38))])
def test_is_repeat_thresholds_and_runs(k, t):
    t1, t2, t3 = t
    assert (java_round(fmul(F(k), F(0.9))), java_round(fmul(F(k // 2), F(0.9))), java_round(fmul(F(k // 3), F(0.9)))) == t
    assert is_repeat(b"A" * k) and is_repeat(b"U" * k) and is_repeat(b"u" * k)
    assert is_repeat((b"AC" * k)[:k]) and is_repeat((b"AU" * k)[:k]) and is_repeat((b"GAC" * k)[:k])
    assert not is_repeat((b"ACGT" * k)[:k]) and not is_repeat((b"ACGTTGCA" * k)[:k])
    assert is_repeat(b"A" * t1 + b"CGTCGTCGTCGTCGTCGT"[:k - t1])


def test_is_repeat_boundaries_at_25():
    assert not is_repeat(b"A" * 20 + b"CGTCG")        # A: 20 < 23; AA 10 / 9 < 11; AAA 6, 6, 6 < 7
    assert is_repeat(b"A" * 21 + b"CGTC")             # AAA at 0, 3, .. 18: 7 >= 7
    assert not is_repeat(b"A" * 18 + b"CGTCGTC")
    assert is_repeat(b"AC" * 11 + b"AGT")             # phase 0: AC x 11 >= 11
    assert not is_repeat(b"AC" * 10 + b"GGTTC")       # AC x 10
    assert is_repeat(b"ACG" * 7 + b"TTTT")            # phase 0: ACG x 7 >= 7
    assert not is_repeat(b"ACG" * 6 + b"TTTTTTT")     # ACG x 6, TTT x 2


def test_is_repeat_at_127():
    tail = b"CGTCGTCGTCGTC"
    assert is_repeat(b"A" * 114 + tail[:13])          # base count 114 >= 114
    assert not is_repeat(b"A" * 113 + b"C" + tail)    # 113; AA 56 < 57; AAA 37 < 38 in every phase


@pytest.mark.parametrize("W,n,want", [
    (4, 10, [(0, 4), (4, 10)]), (4, 9, [(0, 4), (4, 9)]), (4, 7, [(0, 4), (4, 7)]), (4, 6, [(0, 6)]), (4, 5, [(0, 5)]), (4, 4, [(0, 4)]),
    (4, 8, [(0, 4), (4, 8)]), (4, 0, []), (1, 3, [(0, 1), (1, 2), (2, 3)]), (5, 12, [(0, 5), (5, 12)]),
    (5, 13, [(0, 5), (5, 10), (10, 13)]), (5, 11, [(0, 5), (5, 11)]), (5, 10, [(0, 5), (5, 10)]), (100, 7, [(0, 7)]),
])
def test_window_segmentation(W, n, want):
    assert windows(n, W) == want


def test_complex_windows_count_usable_non_repeats():
    k = 25
    read = b"A" * 30 + b"ACGTTGCATGCCAGTACGGATCTAG" + b"N" + b"CCATGACGTTAGCATCGATCGGATC"
    want = sum(1 for p in range(len(read) - k + 1) if b"N" not in read[p:p + k] and not is_repeat(read[p:p + k]))
    assert complex_windows(read, k) == want and 0 < want < len(read) - k + 1


def test_pair_threshold_rule():
    a = dict(flags=PE_FOUND, pe_threshold=F(4))
    b = dict(flags=PE_FOUND, pe_threshold=F(6))
    nb = dict(flags=0, pe_threshold=F(6))
    nlow = dict(flags=0, pe_threshold=F(2))
    assert pair_threshold(a, b) == 4 and pair_threshold(a, nb) == 4 and pair_threshold(a, nlow) == -1
    assert pair_threshold(nb, a) == 4 and pair_threshold(nlow, a) == -1 and pair_threshold(nb, nlow) == -1


def test_ctypes_records_match_the_c_layout():
    import ctypes as C
    from rnabloom import _native as N
    from rnabloom.graph import BloomFilterDeBruijnGraph
    assert C.sizeof(N.CovParams) == 24 and C.sizeof(N.CovStats) == 48
    assert BloomFilterDeBruijnGraph.COV_DTYPE.itemsize == 48
    assert [f[0] for f in N.CovStats._fields_] == list(FIELDS) == list(BloomFilterDeBruijnGraph.COV_DTYPE.names)
    assert N.lib.rb_graph_read_coverage(None, None, 0, 0, None, 0, None, None, None, 0) != 0
    assert b"null argument" in N.lib.rb_last_error()
