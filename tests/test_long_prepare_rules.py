"""The rules of rb_long_prepare restated in Python from the reference's Java, statement by statement, and checked on hand-worked cases.
tests/test_gpu_long_prepare.py compares the device call with this restatement, letter for letter.

  LongReadCorrectionWorker.run (R/RNABloom.java:3700-3859); PolyATailFinder.findPolyASeed (R/util/PolyATailFinder.java:201-277), findPolyATail
  :319-338, findPolyTSeed :355-432, findPolyTHead :476-495, setWindow :99-101; SeqUtils.reverseComplement (R/util/SeqUtils.java:1120-1152),
  nucleotideArrayIndex :315-330, isLowComplexityLong :585-659, isLowComplexityLongWindowed :661-682, trimLowComplexityRegions :839-902.
A read is a bytes object; `float` of the reference is numpy float32.  P is a dict with the fields of rb_prep_params.  prepare(read, P) returns
the record of rb_prep_rec as a tuple in FIELDS' order, the segments as (begin, end) pairs in the transformed read's coordinates and the
transformed read; worker_chain is the worker's loop on top of it.  Two more forms are checked against the statement-by-statement one: the
final-count form of isLowComplexityLong (what a kernel may use) and the scan form of the seed search (the region as three scans of the
search range, which is how a wavefront finds it).
The last part of the file checks that the feature exists at every layer."""
import functools
import itertools
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SHORT, LOW_COMPLEXITY, SEGMENTS = 0, 1, 2
REVCOMP, HAS_POLYA, TAIL_FOUND, HEAD_FOUND, CUT_FIRED, ROUTE_WINDOWS, ROUTE_WINDOWED, ROUTE_WHOLE, MAPPED_TWICE = 1, 2, 4, 8, 16, 32, 64, 128, 256
FIELDS = ("status", "flags", "kept_begin", "kept_end", "tail_start", "tail_end", "head_start", "head_end", "n_windows", "n_low", "offset",
          "n_segments", "tail_searches", "head_searches", "reserved0", "reserved1")
# the worker's values: the finder's ONT profile with seed = minPolyATail and window = maxTipLength + minPolyATail (R/RNABloom.java:248-251), and
# trimLowComplexityRegions(seq, 100, 500) (:3768)
DEFAULTS = dict(min_len=25, reverse_complement=0, strand_specific=0, polya=1, seed_length=12, min_identity=0.9, max_gap=4, window=100,
                lc_window=100, lc_min_length=500)


def params(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


# ---- SeqUtils.reverseComplement :1120-1152 ----
_COMP = {65: 84, 67: 71, 71: 67, 84: 65, 85: 65}


def reverse_complement(seq):
    return bytes(_COMP.get(c, 78) for c in reversed(seq))


# ---- PolyATailFinder ----
def is_a(c):
    return c == 65 or c == 97


def is_t(c):
    return c == 84 or c == 116


def find_polya_seed(seq, searchStart, searchEnd, seedLength, minIdentity):
    """:201-277; [start, end] or None"""
    if searchStart < searchEnd and searchStart >= 0 and searchEnd >= 0 and searchEnd - searchStart >= seedLength:
        numA = 0
        for i in range(searchEnd - 1, searchEnd - seedLength - 1, -1):
            if is_a(seq[i]):
                numA += 1
        id_ = F32(numA) / F32(seedLength)
        best = None
        if id_ >= minIdentity:
            best = [searchEnd - seedLength, searchEnd]
        for i in range(searchEnd - seedLength - 1, searchStart - 1, -1):
            if numA > 0:
                if is_a(seq[i + seedLength]):
                    numA -= 1
            if is_a(seq[i]):
                numA += 1
                id_ = F32(numA) / F32(seedLength)
                if best is None:
                    if id_ >= minIdentity:
                        best = [i, i + seedLength]
                else:
                    if id_ >= minIdentity:
                        best[0] = i
                    else:
                        break
            elif best is not None and F32(numA) / F32(seedLength) < minIdentity:
                break
        if best is not None:
            while best[1] - best[0] > seedLength:
                if is_a(seq[best[1] - 1]):
                    break
                best[1] -= 1
            if best[0] == searchStart:
                while best[0] > 0:
                    if is_a(seq[best[0]]):
                        best[0] -= 1
                    else:
                        break
        return best
    return None


def find_polyt_seed(seq, searchStart, searchEnd, seedLength, minIdentity):
    """:355-432"""
    if searchStart < searchEnd and searchStart >= 0 and searchEnd >= 0 and searchEnd - searchStart >= seedLength:
        numT = 0
        for i in range(searchStart, searchStart + seedLength):
            if is_t(seq[i]):
                numT += 1
        id_ = F32(numT) / F32(seedLength)
        best = None
        if id_ >= minIdentity:
            best = [searchStart, searchStart + seedLength]
        for i in range(searchStart + seedLength, searchEnd):
            if numT > 0:
                if is_t(seq[i - seedLength]):
                    numT -= 1
            if is_t(seq[i]):
                numT += 1
                id_ = F32(numT) / F32(seedLength)
                if best is None:
                    if id_ >= minIdentity:
                        best = [i - seedLength, i + 1]
                else:
                    if id_ >= minIdentity:
                        best[1] = i + 1
                    else:
                        break
            elif best is not None and F32(numT) / F32(seedLength) < minIdentity:
                break
        if best is not None:
            while best[1] - best[0] > seedLength:
                if is_t(seq[best[0]]):
                    break
                best[0] += 1
            if best[1] == searchEnd:
                seqLen = len(seq)
                while best[1] < seqLen:
                    if is_t(seq[best[1]]):
                        best[1] += 1
                    else:
                        break
        return best
    return None


def percent(seq, start, end, letter):
    return F32(sum(1 for i in range(start, end) if letter(seq[i]))) / F32(end - start)


class Finder:
    def __init__(self, P, seed=find_polya_seed, seed_t=find_polyt_seed):
        self.seedLength, self.minIdentity, self.maxGap = P["seed_length"], F32(P["min_identity"]), P["max_gap"]
        self.window = max(self.seedLength, P["window"])              # setWindow :99-101
        self.seed, self.seed_t = seed, seed_t
        self.bridged = 0                                             # joins that only percentA / percentT allowed (for the tests' reach)

    def find_polya_tail(self, seq):
        """:319-338; (interval or None, seed searches made)"""
        seqLen = len(seq)
        searchEnd = seqLen
        searchStart = max(0, searchEnd - self.window)
        best = self.seed(seq, searchStart, searchEnd, self.seedLength, self.minIdentity)
        n = 1
        while best is not None and searchStart > 0:
            searchEnd = best[0]
            searchStart = max(0, searchEnd - self.window)
            prev = self.seed(seq, searchStart, searchEnd, self.seedLength, self.minIdentity)
            n += 1
            if prev is not None and (prev[1] + self.maxGap >= best[0] or self._bridge(seq, prev[1], best[0], is_a)):
                best[0] = prev[0]
            else:
                break
        return best, n

    def find_polyt_head(self, seq):
        """:476-495"""
        seqLen = len(seq)
        searchStart = 0
        searchEnd = min(seqLen, self.window)
        best = self.seed_t(seq, searchStart, searchEnd, self.seedLength, self.minIdentity)
        n = 1
        while best is not None and searchEnd < seqLen:
            searchStart = best[1]
            searchEnd = min(seqLen, best[1] + self.window)
            nxt = self.seed_t(seq, searchStart, searchEnd, self.seedLength, self.minIdentity)
            n += 1
            if nxt is not None and (best[1] + self.maxGap >= nxt[0] or self._bridge(seq, best[1], nxt[0], is_t)):
                best[1] = nxt[1]
            else:
                break
        return best, n

    def _bridge(self, seq, start, end, letter):
        ok = percent(seq, start, end, letter) >= self.minIdentity
        self.bridged += bool(ok)
        return ok


# ---- the scan form of the seed search: what a wavefront computes with a lane per position ----
def seed_threshold(seedLength, minIdentity):
    """the smallest count that passes numA / (float) seedLength >= minIdentity"""
    return next(c for c in range(seedLength + 1) if F32(c) / F32(seedLength) >= minIdentity)


def seed_by_scans(seq, s, e, seedLength, minIdentity, mirrored=False):
    """findPolyASeed as three scans of [s, e); mirrored: findPolyTSeed, on the mirrored read (position p is letter len - 1 - p) and in its
    coordinates — the two places where the reference's T form is not the mirror image of its A form are marked"""
    L = len(seq)
    hit = (lambda p: is_t(seq[L - 1 - p])) if mirrored else (lambda p: is_a(seq[p]))
    if not (s < e and s >= 0 and e - s >= seedLength):
        return None
    thr = seed_threshold(seedLength, minIdentity)
    ok = lambda i: sum(hit(i + q) for q in range(seedLength)) >= thr
    i0 = e - seedLength
    ic = next((i for i in range(i0, s - 1, -1) if (i == i0 or hit(i)) and ok(i)), None)
    if ic is None:
        return None
    stop = next((i for i in range(ic - 1, s - 1, -1) if not ok(i)), s - 1)
    start = next((i for i in range(stop + 1, ic) if hit(i)), ic)
    end = ic + seedLength + (1 if mirrored and ic != i0 else 0)                  # (Interval(i - seedLength, i + 1): one letter longer)
    end = next((i for i in range(end - 1, start + seedLength - 1, -1) if hit(i)), start + seedLength - 1) + 1
    if start == s:
        if mirrored:                                                             # (the head's end stops BEHIND the last T)
            start = next((i for i in range(start - 1, -1, -1) if not hit(i)), -1) + 1
        else:                                                                    # (the tail's start stops ON the letter that is no A, or at 0)
            start = next((i for i in range(start, 0, -1) if not hit(i)), 0)
    return [start, end]


def seed_t_by_scans(seq, s, e, seedLength, minIdentity):
    L = len(seq)
    r = seed_by_scans(seq, L - e, L - s, seedLength, minIdentity, mirrored=True)
    return None if r is None else [L - r[1], L - r[0]]


# ---- SeqUtils: complexity ----
_IDX = {65: 0, 67: 1, 71: 2, 84: 3, 85: 3}
T89 = F32(0.89)                                                                  # LOW_COMPLEXITY_THRESHOLD_LONG_SEQ :62


def java_round(x):
    return int(math.floor(float(x) + 0.5))                                       # Math.round(float)


@functools.lru_cache(maxsize=None)
def thresholds(length):
    return (java_round(F32(length) * T89), java_round(F32(length) * T89 / F32(2.0)), java_round(F32(length) * T89 / F32(3.0)))


def is_low_complexity_long(seq):
    """:585-659, statement by statement"""
    length = len(seq)
    if length <= 6:
        return False
    t1, t2, t3 = thresholds(length)
    nf1 = [0] * 4
    nf2 = [[0] * 4 for _ in range(4)]
    nf3 = [[[0] * 4 for _ in range(4)] for _ in range(4)]
    c3, c2, c1 = (_IDX.get(c, -1) for c in seq[:3])
    if c3 >= 0:
        nf1[c3] += 1
    if c2 >= 0:
        nf1[c2] += 1
    if c1 >= 0:
        nf1[c1] += 1
    if c3 != c2 or c2 != c1 or c3 != c1:
        if c3 >= 0 and c2 >= 0:
            nf2[c3][c2] += 1
        if c2 >= 0 and c1 >= 0:
            nf2[c2][c1] += 1
        if c3 >= 0 and c2 >= 0 and c1 >= 0:
            nf3[c3][c2][c1] += 1
    for ch in seq[3:]:
        c3 = c2
        c2 = c1
        c1 = _IDX.get(ch, -1)
        if c1 >= 0:
            nf1[c1] += 1
            if nf1[c1] >= t1:
                return True
        if c3 != c2 or c2 != c1 or c3 != c1:
            if c2 >= 0 and c1 >= 0:
                nf2[c2][c1] += 1
                if nf2[c2][c1] >= t2:
                    return True
            if c3 >= 0 and c2 >= 0 and c1 >= 0:
                nf3[c3][c2][c1] += 1
                if nf3[c3][c2][c1] >= t3:
                    return True
    if (nf1[0] + nf1[1] >= t1 or nf1[0] + nf1[2] >= t1 or nf1[0] + nf1[3] >= t1 or nf1[1] + nf1[2] >= t1 or nf1[1] + nf1[3] >= t1 or
            nf1[2] + nf1[3] >= t1):
        return True
    for i in range(4):
        for j in range(4):
            count = nf2[i][j]
            for k in range(i, 4):
                for l in range(j, 4):
                    if (i != k or j != l) and count + nf2[k][l] >= t2:
                        return True
    return False


def final_counts(seq):
    """the 4 + 16 + 64 counters of a window once every letter is counted: a letter at every position, and for every position p >= 2 whose
    three letters are not one value the pair (p - 1, p) and the triple — the pair (0, 1) goes with the first triple"""
    x = [_IDX.get(c, -1) for c in seq]
    cnt = [0] * 84
    for p in range(len(x)):
        c1 = x[p]
        if c1 >= 0:
            cnt[c1] += 1
        if p < 2:
            continue
        c2, c3 = x[p - 1], x[p - 2]
        if c3 == c2 and c2 == c1:
            continue
        if c2 >= 0 and c1 >= 0:
            cnt[4 + 4 * c2 + c1] += 1
        if p == 2 and c3 >= 0 and c2 >= 0:
            cnt[4 + 4 * c3 + c2] += 1
        if c3 >= 0 and c2 >= 0 and c1 >= 0:
            cnt[20 + 16 * c3 + 4 * c2 + c1] += 1
    return cnt


def is_low_by_final_counts(seq):
    length = len(seq)
    if length <= 6:
        return False
    t1, t2, t3 = thresholds(length)
    cnt = final_counts(seq)
    nf1, nf2, nf3 = cnt[:4], cnt[4:20], cnt[20:]
    if max(nf1) >= t1 or max(nf2) >= t2 or max(nf3) >= t3:
        return True
    if any(nf1[i] + nf1[j] >= t1 for i in range(4) for j in range(i + 1, 4)):
        return True
    return any((i != k or j != l) and nf2[4 * i + j] + nf2[4 * k + l] >= t2
               for i in range(4) for j in range(4) for k in range(i, 4) for l in range(j, 4))


def is_low_complexity_long_windowed(seq):
    """:661-682; (low, n_windows, n_low, offset) — 0, 1 if low, 0 where the whole sequence is judged"""
    seqLen = len(seq)
    windowSize = 50
    numWindows = seqLen // windowSize
    if numWindows >= 4:
        offset = (seqLen % windowSize) // 2
        numLow = 0
        for i in range(numWindows):
            start = i * windowSize + offset
            if is_low_complexity_long(seq[start:start + windowSize]):
                numLow += 1
        return numLow >= math.floor(0.75 * numWindows), numWindows, numLow, offset
    low = is_low_complexity_long(seq)
    return low, 0, int(low), 0


def trim_low_complexity_regions(seq, windowSize, minLowComplexityLength):
    """:839-902; (segments as (begin, end), route flags, n_windows, n_low, offset)"""
    segments = []
    seqLen = len(seq)
    numWindows = seqLen // windowSize
    if numWindows >= 5:
        complexityStatus = [False] * numWindows
        offset = (seqLen % windowSize) // 2
        numLow = 0
        for i in range(numWindows):
            start = i * windowSize + offset
            if is_low_complexity_long(seq[start:start + windowSize]):
                numLow += 1
            else:
                complexityStatus[i] = True
        flags = ROUTE_WINDOWS
        if numLow * windowSize >= minLowComplexityLength:
            flags |= CUT_FIRED
            start = end = -1
            for i in range(numWindows):
                if complexityStatus[i]:
                    if start < 0:
                        start = i
                    end = i
                elif start >= 0:
                    if start == 0:
                        segments.append((0, offset + (end + 1) * windowSize))
                    else:
                        segments.append((offset + start * windowSize, offset + (end + 1) * windowSize))
                    start = end = -1
            if start == 0:
                segments.append((0, seqLen))
            elif start > 0:
                segments.append((offset + start * windowSize, seqLen))
        else:
            segments.append((0, seqLen))
        return segments, flags, numWindows, numLow, offset
    low, nw, nl, off = is_low_complexity_long_windowed(seq)
    if not low:
        segments.append((0, seqLen))
    return segments, (ROUTE_WINDOWED if nw else ROUTE_WHOLE), nw, nl, off


# ---- the worker's steps before its first graph call (R/RNABloom.java:3705-3779) ----
def prepare(read, P, finder=None):
    """(record in FIELDS' order, segments, transformed read — None for a read that is too short)"""
    read = bytes(read)
    seq = reverse_complement(read) if P["reverse_complement"] else read
    length = len(seq)
    if length < P["min_len"]:
        return (SHORT, 0, 0, 0, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0), [], None
    flags, hasPolyA, turned = 0, False, False
    a, b = 0, length
    tail = head = None
    nt = nh = 0
    if P["polya"]:
        f = finder or Finder(P)
        tail, nt = f.find_polya_tail(seq)
        if P["strand_specific"]:
            if tail is not None and tail[1] < length:
                b = tail[1]
                hasPolyA = True
        else:
            head, nh = f.find_polyt_head(seq)
            if tail is not None and head is None:
                if tail[1] < length:
                    b = tail[1]
                hasPolyA = True
            elif tail is None and head is not None:
                if head[0] > 0:
                    a = head[0]
                turned = True
                hasPolyA = True
            elif tail is not None and head is not None:
                if head[1] < tail[0]:
                    a, b = head[1], tail[0]
                hasPolyA = False
    seq = seq[a:b]
    if turned:
        seq = reverse_complement(seq)
    segments, cflags, nw, nl, off = trim_low_complexity_regions(seq, P["lc_window"], P["lc_min_length"])
    if len(segments) > 1:
        hasPolyA = False
    flags |= cflags | (TAIL_FOUND if tail is not None else 0) | (HEAD_FOUND if head is not None else 0) | (HAS_POLYA if hasPolyA else 0)
    rc = bool(P["reverse_complement"])
    if rc != turned:
        flags |= REVCOMP
    if rc and turned:
        flags |= MAPPED_TWICE
    kb, ke = (length - b, length - a) if rc else (a, b)
    t = tail if tail is not None else (-1, -1)
    h = head if head is not None else (-1, -1)
    rec = (SEGMENTS if segments else LOW_COMPLEXITY, flags, kb, ke, t[0], t[1], h[0], h[1], nw, nl, off, len(segments), nt, nh, 0, 0)
    return rec, segments, seq


def worker_chain(names, reads, P, k, minKmerCov, correct):
    """LongReadCorrectionWorker.run's output queue (:3768-3849): [(name, seq, length, score, isRepeat, hasPolyA)], reads kept, reads discarded.
    correct(segment, trimEdges) is everything between graph.getKmers and assembleValidKmers: the strings of a segment, or None where the
    corrected list is null or empty (:3804, :3814).  A segment whose corrected list is not empty counts as kept even if assembleValidKmers
    makes no string of it (:3839)."""
    out, kept_n, discarded = [], 0, 0
    for name, read in zip(names, reads):
        rec, segments, seq = prepare(read, P)
        kept = False
        if rec[0] == LOW_COMPLEXITY:
            out.append((name, seq, len(seq), 0.0, True, False))
        elif rec[0] == SEGMENTS:
            hasPolyA = bool(rec[1] & HAS_POLYA)
            multi = len(segments) > 1
            for sid, (sb, se) in enumerate(segments, 1):
                segName = name + (b"_s%d" % sid if multi else b"")
                segment = seq[sb:se]
                if len(segment) < k:                                             # graph.getKmers(segment) is empty
                    continue
                parts = correct(segment, minKmerCov > 1 and not hasPolyA)
                if parts is None:
                    continue
                if len(parts) == 1:
                    out.append((segName, parts[0], len(parts[0]), float(len(parts[0])), False, hasPolyA))
                else:
                    hasPolyA = False
                    for pid, part in enumerate(parts, 1):
                        out.append((segName + b"_p%d" % pid, part, len(part), float(len(part)), False, hasPolyA))
                kept = True
        kept_n += kept
        discarded += not kept
    return out, kept_n, discarded


def rec_of(read, **kw):
    rec, segs, seq = prepare(read, params(**kw))
    return dict(zip(FIELDS, rec)), segs, seq


# ================= hand-worked answers: the finder =================
X20 = b"CG" * 10                             # twenty letters that are neither A nor T
BODY = b"GATCCGTAGCTAGGCTTACGGATCGCATGCCTAGGATCGTACGGCTAGCATCGGATGCAC"       # sixty letters without AAAA or TTTT, no low complexity
FIND = dict(min_len=0, seed_length=4, min_identity=0.9)                     # a seed is four A (3 / 4 = 0.75 < 0.9f)


def finder(**kw):
    return Finder(params(**dict(FIND, **kw)))


def test_seed_threshold_is_one_integer_per_call():
    # 0.9f: 9 of 10, 11 of 12, 4 of 4 (8 / 10, 10 / 12 = 0.833 and 3 / 4 fail); float32 9 / 10 IS 0.9f
    assert [seed_threshold(n, F32(0.9)) for n in (10, 12, 4)] == [9, 11, 4]
    assert F32(9) / F32(10) >= F32(0.9) and not F32(8) / F32(10) >= F32(0.9)
    assert seed_threshold(4, F32(0.5)) == 2 and seed_threshold(7, F32(1.0)) == 7 and seed_threshold(3, F32(1e-6)) == 1


def test_seed_at_the_identity_threshold_and_one_a_short_of_it():
    # seed 10, identity 0.9: a window of nine A and one C passes wherever the C is.  The region [20, 30) starts where the search does, so its
    # start walks down while seq[start] is an A: with the C at 20 it stays, else it goes to 19 and stops there, on the G
    for p in range(10):
        w = bytearray(b"A" * 10)
        w[p] = 67
        assert find_polya_seed(X20 + bytes(w), 20, 30, 10, F32(0.9)) == ([20, 30] if p == 0 else [19, 30]), p
    # eight A of ten: no seed, in the same range and in a wider one
    assert find_polya_seed(X20 + b"AAAACAAACA", 20, 30, 10, F32(0.9)) is None
    assert find_polya_seed(X20 + b"AAAACAAACA", 0, 30, 10, F32(0.9)) is None
    # the guard is searchEnd - searchStart >= seedLength
    assert find_polya_seed(b"A" * 9, 0, 9, 10, F32(0.9)) is None and find_polya_seed(b"A" * 10, 0, 10, 10, F32(0.9)) == [0, 10]
    assert find_polyt_seed(b"T" * 9, 0, 9, 10, F32(0.9)) is None and find_polyt_seed(b"T" * 10, 0, 10, 10, F32(0.9)) == [0, 10]


def test_refinement_leaves_the_start_on_a_letter_that_is_no_a():
    s = X20 + b"AAAA"
    # a search that begins at 20 finds [20, 24); the region starts where the search did, so start walks down WHILE seq[start] is A: 20 -> 19, and
    # seq[19] = G ends the walk with start = 19, on the G
    assert find_polya_seed(s, 20, 24, 4, F32(0.9)) == [19, 24]
    # a search that begins lower finds the same seed, start 20 != searchStart: no walk
    assert find_polya_seed(s, 10, 24, 4, F32(0.9)) == [20, 24]
    # the walk ends at 0 without looking at letter 0
    assert find_polya_seed(b"AAAAAA", 2, 6, 4, F32(0.9)) == [0, 6] and find_polya_seed(b"CAAAAA", 2, 6, 4, F32(0.9)) == [0, 6]
    # the T form walks its end up while the letter BEHIND the region is a T: it ends behind the last T
    assert find_polyt_seed(b"TTTT" + X20, 0, 4, 4, F32(0.9)) == [0, 4]
    assert find_polyt_seed(b"TTTTTT" + X20, 0, 4, 4, F32(0.9)) == [0, 6]
    # and where it does not open at the search start it opens one letter longer than the seed: C TTTT opens Interval(i - 4, i + 1) = [0, 5) and the
    # refinement drops the C; G C TTTT TT: the window [2, 6) opens [1, 6), grows to 8 and is refined to [2, 8)
    assert find_polyt_seed(b"CTTTT" + X20, 0, 25, 4, F32(0.9)) == [1, 5]
    assert find_polyt_seed(b"GCTTTTTT" + X20, 0, 28, 4, F32(0.9)) == [2, 8]
    # the far end loses its other letters only while the region is longer than the seed: ten A and a C with seed 10 — the window [21, 31) of nine A
    # opens, [20, 30) passes too, the C at 30 is dropped; the same C inside a region of exactly ten letters stays
    assert find_polya_seed(X20 + b"AAAAAAAAAAC", 0, 31, 10, F32(0.9)) == [20, 30]
    assert find_polya_seed(X20 + b"CAAAAAAAAAC", 0, 31, 10, F32(0.9)) == [21, 31]


def test_tail_chain_gap_of_max_gap_and_one_more_that_percent_a_bridges():
    # A A C C A C AAAAA, seed 3 at identity 0.5 (two A of three), window 5.  Search [6, 11): AAA at 8, the windows at 7 and 6 pass, the region
    # starts where the search did and walks to 5, on the C: best = [5, 11).  Search [0, 5): CCA and ACC fail, AAC at 0 passes: prev = [0, 3).  The gap
    # is letters 3 and 4, C A.  With max_gap 2 the first operand joins them (3 + 2 >= 5); with max_gap 1 it does not (4 < 5) and percentA = 1 / 2 =
    # 0.5 >= 0.5 does; with identity 0.51 (still two of three) nothing does, and the tail stays [5, 11)
    s = b"AACCACAAAAA"
    for gap, ident, want, bridged in ((2, 0.5, [0, 11], 0), (1, 0.5, [0, 11], 1), (1, 0.51, [5, 11], 0)):
        f = finder(seed_length=3, min_identity=ident, max_gap=gap, window=5)
        assert f.find_polya_tail(s) == (want, 2) and f.bridged == bridged, (gap, ident)
    # the head's chain is no mirror image of it.  TTTT GCGC TTTT, seed 4, window 8: [0, 4) opens at the search start and stops at the G.  Search
    # [4, 12): the window that ends at letter 11 is the first with four T and opens Interval(11 - 4, 12) = [7, 12), refined to [8, 12); it ends
    # where the search does, and the C behind it ends the walk.  4 + max_gap 4 >= 8 joins; with max_gap 3 percentT = 0 / 4 does not
    t = b"TTTTGCGCTTTT" + X20
    assert finder(window=8).find_polyt_head(t) == ([0, 12], 3) and finder(window=8, max_gap=3).find_polyt_head(t) == ([0, 4], 2)


def test_tail_that_reaches_letter_zero_and_a_window_larger_than_the_read():
    # thirty A, window 10: the first search [20, 30) opens at 26, grows to 20 = searchStart and walks down to 0; the loop goes on (searchStart was
    # 20 > 0) with the empty range [0, 0), which is null: two searches
    assert finder(window=10).find_polya_tail(b"A" * 30) == ([0, 30], 2)
    assert finder(window=10).find_polyt_head(b"T" * 30) == ([0, 30], 2)
    # a window larger than the read: one search over all of it, and the loop never runs
    assert finder(window=4000).find_polya_tail(b"A" * 30) == ([0, 30], 1)
    assert finder(window=4000).find_polya_tail(X20 + b"AAAAAA") == ([20, 26], 1)
    # a window smaller than the seed is the seed (setWindow)
    assert finder(window=1).window == 4
    # chains: AAAA every eight letters, window 8, max_gap 4 — each search finds the block below, four letters away; the fourth finds none
    s = X20 + b"AAAACGCGAAAACGCGAAAA"
    assert finder(window=8).find_polya_tail(s) == ([20, 40], 4)
    # an empty read and one shorter than the seed
    assert finder().find_polya_tail(b"") == (None, 1) and finder().find_polyt_head(b"TTT") == (None, 1)


def test_five_way_rule():
    R = ROUTE_WHOLE
    tail, junk, head = BODY + b"AAAAAA", BODY + b"AAAAAACG", b"TTTTTT" + BODY
    # tail only: hasPolyA either way, cut only where something follows the tail
    rec, segs, seq = rec_of(tail, **FIND)
    assert (rec["status"], rec["flags"], rec["kept_begin"], rec["kept_end"]) == (SEGMENTS, R | TAIL_FOUND | HAS_POLYA, 0, 66)
    assert (rec["tail_start"], rec["tail_end"], rec["head_start"], rec["head_end"], rec["tail_searches"], rec["head_searches"]) == (60, 66, -1, -1, 1, 1)
    assert segs == [(0, 66)] and seq == tail
    rec, segs, seq = rec_of(junk, **FIND)
    assert (rec["flags"], rec["kept_begin"], rec["kept_end"], rec["tail_start"], rec["tail_end"]) == (R | TAIL_FOUND | HAS_POLYA, 0, 66, 60, 66)
    assert segs == [(0, 66)] and seq == tail
    # stranded: cut AND hasPolyA only if tail.end < length; no head search
    rec, segs, seq = rec_of(tail, strand_specific=1, **FIND)
    assert (rec["flags"], rec["kept_end"], rec["head_searches"]) == (R | TAIL_FOUND, 66, 0) and seq == tail
    rec, segs, seq = rec_of(junk, strand_specific=1, **FIND)
    assert (rec["flags"], rec["kept_end"], rec["head_searches"]) == (R | TAIL_FOUND | HAS_POLYA, 66, 0) and seq == tail
    rec, segs, seq = rec_of(head, strand_specific=1, **FIND)                # a head means nothing to a stranded run
    assert (rec["flags"], rec["kept_begin"], rec["kept_end"], rec["head_start"]) == (R, 0, 66, -1) and seq == head
    # head only: cut what lies before it, turn the read
    rec, segs, seq = rec_of(head, **FIND)
    assert (rec["flags"], rec["kept_begin"], rec["kept_end"], rec["head_start"], rec["head_end"]) == (R | HEAD_FOUND | HAS_POLYA | REVCOMP, 0, 66, 0, 6)
    assert seq == reverse_complement(BODY) + b"AAAAAA"
    rec, segs, seq = rec_of(b"CG" + head, **FIND)
    assert (rec["flags"], rec["kept_begin"], rec["kept_end"], rec["head_start"], rec["head_end"]) == (R | HEAD_FOUND | HAS_POLYA | REVCOMP, 2, 68, 2, 8)
    assert seq == reverse_complement(BODY) + b"AAAAAA"
    # both, apart: what lies between them, and hasPolyA stays false
    rec, segs, seq = rec_of(b"TTTTTT" + BODY + b"AAAAAA", **FIND)
    assert (rec["flags"], rec["kept_begin"], rec["kept_end"]) == (R | TAIL_FOUND | HEAD_FOUND, 6, 66) and seq == BODY and segs == [(0, 60)]
    assert (rec["tail_start"], rec["tail_end"], rec["head_start"], rec["head_end"]) == (66, 72, 0, 6)
    # both, touching (head.end = tail.start is not <): nothing is cut.  TTTTAAAA is four T and four A: two letters make up all of it, low complexity
    rec, segs, seq = rec_of(b"TTTTAAAA", **FIND)
    assert (rec["status"], rec["flags"], rec["kept_begin"], rec["kept_end"]) == (LOW_COMPLEXITY, R | TAIL_FOUND | HEAD_FOUND, 0, 8)
    assert (rec["tail_start"], rec["tail_end"], rec["head_start"], rec["head_end"], rec["n_low"], rec["n_segments"]) == (4, 8, 0, 4, 1, 0) and segs == []
    # both, overlapping: TATATATATA at identity 0.5 — the tail is [1, 10), the head [0, 9)
    rec, segs, seq = rec_of(b"TATATATATA", min_len=0, seed_length=4, min_identity=0.5)
    assert (rec["tail_start"], rec["tail_end"], rec["head_start"], rec["head_end"], rec["kept_begin"], rec["kept_end"]) == (1, 10, 0, 9, 0, 10)
    assert not rec["flags"] & HAS_POLYA
    # no finder at all
    rec, segs, seq = rec_of(junk, polya=0, min_len=0)
    assert (rec["flags"], rec["kept_end"], rec["tail_start"], rec["tail_searches"], rec["head_searches"]) == (R, 68, -1, 0, 0) and seq == junk


def test_reverse_complement_first_and_the_second_turn():
    # the argument turns the read before anything else: a head in the input is a tail to the finder
    rec, segs, seq = rec_of(b"TTTTTT" + BODY, reverse_complement=1, **FIND)
    assert (rec["flags"], rec["kept_begin"], rec["kept_end"], rec["tail_start"], rec["tail_end"]) == (ROUTE_WHOLE | TAIL_FOUND | HAS_POLYA | REVCOMP, 0, 66, 60, 66)
    assert seq == reverse_complement(BODY) + b"AAAAAA"
    # something before the head in the input follows the tail in the finder's read and is cut: the kept letters are input letters [2, 68)
    rec, segs, seq = rec_of(b"CG" + b"TTTTTT" + BODY, reverse_complement=1, **FIND)
    assert (rec["kept_begin"], rec["kept_end"], rec["tail_start"], rec["tail_end"]) == (2, 68, 60, 66) and seq == reverse_complement(BODY) + b"AAAAAA"
    # a tail in the input is a head to the finder, and the head rule turns the read back: it runs with the input again, but every letter went
    # through the complement map twice — U is T now, and lower case and N are N
    raw = b"GAUCCgTANC" + BODY[10:] + b"AAAAAA" + b"CG"
    rec, segs, seq = rec_of(raw, reverse_complement=1, **FIND)
    assert (rec["flags"], rec["kept_begin"], rec["kept_end"], rec["head_start"], rec["head_end"]) == (ROUTE_WHOLE | HEAD_FOUND | HAS_POLYA | MAPPED_TWICE, 0, 66, 2, 8)
    assert seq == b"GATCCNTANC" + BODY[10:] + b"AAAAAA"
    # the length test is made on the raw length
    assert rec_of(BODY[:24])[0]["status"] == SHORT and rec_of(BODY[:25])[0]["status"] == SEGMENTS
    assert prepare(BODY[:24], params()) == ((SHORT, 0, 0, 0, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0), [], None)


# ================= hand-worked answers: complexity =================
def test_thresholds_and_short_sequences():
    assert thresholds(100) == (89, 45, 30) and thresholds(50) == (45, 22, 15) and thresholds(7) == (6, 3, 2)
    assert not is_low_complexity_long(b"AAAAAA") and is_low_complexity_long(b"AAAAAAA")          # six letters or less are never low
    # only upper-case A C G T U count, U as T: seven a are nothing, TTUUTTU is seven T
    assert not is_low_complexity_long(b"aaaaaaa") and is_low_complexity_long(b"TTUUTTU") and not is_low_complexity_long(b"NNNNNNN")
    # 100 letters: 89 A are low, 88 A and 12 N are not (no other counter moves: a triple with an N counts nothing)
    assert is_low_complexity_long(b"A" * 89 + b"N" * 11) and not is_low_complexity_long(b"A" * 88 + b"N" * 12)
    # (AC)^50: AC is counted 50 times >= 45.  Three equal letters count neither pair nor triple, one letter always
    assert is_low_complexity_long(b"AC" * 50)
    c = final_counts(b"AAAC")
    assert c[0] == 3 and c[1] == 1 and c[4 + 0] == 0 and c[4 + 1] == 1 and c[20 + 1] == 1 and sum(c) == 6       # AAA counts no AA; then AC and AAC
    c = final_counts(b"ACAA")
    assert c[4 + 1] == 1 and c[4 + 4] == 1 and c[4 + 0] == 1 and c[20 + 4] == 1 and c[20 + 16] == 1            # AC with the first triple, CA, AA; ACA, CAA


def block(kind, n, seed=0):
    if kind == "c":
        rng = np.random.default_rng(1234 + seed)
        return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()
    return (kind.encode() * n)[:n]


def test_trim_low_complexity_regions_segments():
    c = [block("c", 100, i) for i in range(8)]
    assert not any(is_low_complexity_long(x) for x in c)
    lo = [block("A", 100), block("AC", 100), block("ACG", 100), block("T", 100)]
    assert all(is_low_complexity_long(x) for x in lo)
    edge = block("c", 15, 99)
    # 730 letters: seven windows from offset 15.  complex, low, low, complex, complex, low, low: four low windows
    s = edge + c[0] + lo[0] + lo[1] + c[1] + c[2] + lo[2] + lo[3] + edge
    assert trim_low_complexity_regions(s, 100, 500) == ([(0, 730)], ROUTE_WINDOWS, 7, 4, 15)                       # 400 < 500: the cut does not fire
    assert trim_low_complexity_regions(s, 100, 400) == ([(0, 115), (315, 515)], ROUTE_WINDOWS | CUT_FIRED, 7, 4, 15)  # a run from window 0 starts at letter 0
    # 830 letters: low, complex, complex, low x 4, complex — the last run is open at the end and runs to seqLen
    s = edge + lo[0] + c[0] + c[1] + lo[1] + lo[2] + lo[3] + lo[0] + c[2] + edge
    assert trim_low_complexity_regions(s, 100, 500) == ([(115, 315), (715, 830)], ROUTE_WINDOWS | CUT_FIRED, 8, 5, 15)
    # lc_min_length 0 fires with no low window: the one run starts at window 0 and is open at the end
    s = b"".join(c[:5]) + edge
    assert trim_low_complexity_regions(s, 100, 0) == ([(0, 515)], ROUTE_WINDOWS | CUT_FIRED, 5, 0, 7)
    # every window low: fired, no segment
    assert trim_low_complexity_regions(b"A" * 500, 100, 500) == ([], ROUTE_WINDOWS | CUT_FIRED, 5, 5, 0)
    # 499 letters are four windows of 100: windows of 50 decide, nine of them from offset 24; low when numLow >= floor(0.75 * 9) = 6
    s = block("c", 24, 5) + b"".join(block("A", 50) if i < 6 else block("c", 50, i) for i in range(9)) + block("c", 25, 6)
    assert trim_low_complexity_regions(s, 100, 500) == ([], ROUTE_WINDOWED, 9, 6, 24)
    s = block("c", 24, 5) + b"".join(block("A", 50) if i < 5 else block("c", 50, i) for i in range(9)) + block("c", 25, 6)
    assert trim_low_complexity_regions(s, 100, 500) == ([(0, 499)], ROUTE_WINDOWED, 9, 5, 24)
    # 199 letters: three windows of 50, the whole sequence decides; 200: four windows
    assert trim_low_complexity_regions(b"A" * 177 + b"N" * 22, 100, 500) == ([], ROUTE_WHOLE, 0, 1, 0)          # round(199 * 0.89f) = 177
    assert trim_low_complexity_regions(b"A" * 176 + b"N" * 23, 100, 500) == ([(0, 199)], ROUTE_WHOLE, 0, 0, 0)
    assert trim_low_complexity_regions(b"A" * 200, 100, 500) == ([], ROUTE_WINDOWED, 4, 4, 0)
    # several segments clear hasPolyA; one keeps it
    s = edge + c[0] + lo[0] + c[1] + lo[1] + lo[2] + lo[3] + lo[0] + c[2] + b"A" * 15
    rec, segs, seq = rec_of(s)
    assert rec["flags"] == ROUTE_WINDOWS | CUT_FIRED | TAIL_FOUND and segs == [(0, 115), (215, 315), (715, 830)] and rec["n_segments"] == 3
    rec, segs, seq = rec_of(s, lc_min_length=501)
    assert rec["flags"] == ROUTE_WINDOWS | TAIL_FOUND | HAS_POLYA and segs == [(0, 830)]


# ================= the two other forms =================
def test_final_count_form_on_every_short_string():
    """every string over A, C, N of 7 to 11 letters: the counters only grow and the first three letters cannot reach a threshold, so the verdict
    is a function of the final counts"""
    low = n = 0
    for length in range(7, 12):
        for t in itertools.product(b"ACN", repeat=length):
            s = bytes(t)
            a = is_low_complexity_long(s)
            assert a == is_low_by_final_counts(s), s
            low += a
            n += 1
    assert n == sum(3 ** i for i in range(7, 12)) and 0 < low < n


def _near_threshold(rng, n):
    """a repeat of 1 to 3 letters, n long, with letters knocked out until the repeat's counter is at its threshold or one below it"""
    m = int(rng.integers(1, 4))
    unit = bytes(rng.permutation(np.frombuffer(b"ACGT", np.uint8))[:m].tolist())
    s = bytearray((unit * n)[:n])
    which = {1: _IDX[unit[0]], 2: 4 + 4 * _IDX[unit[0]] + _IDX[unit[-1]], 3: 20 + 16 * _IDX[unit[0]] + 4 * _IDX[unit[1 % m]] + _IDX[unit[2 % m]]}[m]
    goal = thresholds(n)[m - 1] - int(rng.integers(0, 2))
    for p in rng.permutation(n):
        if final_counts(bytes(s))[which] <= goal:
            break
        s[p] = int(rng.choice(np.frombuffer(b"Nacgt", np.uint8)))
    return bytes(s), m, final_counts(bytes(s))[which] - thresholds(n)[m - 1]


def test_final_count_form_on_random_strings():
    rng = np.random.default_rng(20240611)
    alphabet = np.frombuffer(b"ACGTUNacgt", np.uint8)
    low, margins = 0, {1: set(), 2: set(), 3: set()}                   # per threshold: how far the repeat's counter ended from it
    for it in range(20000):
        n = int(rng.integers(7, 200))
        if it % 2:
            s, m, margin = _near_threshold(rng, n)
            margins[m].add(margin)
        else:
            s = alphabet[rng.integers(0, 10, n)].tobytes()
        a = is_low_complexity_long(s)
        assert a == is_low_by_final_counts(s), s
        low += a
    # each of t1, t2, t3 is met exactly and missed by one (a knocked-out letter takes up to three counts off a triple's counter, so a counter
    # may pass its goal: those strings are compared all the same, and are not what this line counts)
    assert all({0, -1} <= margins[m] for m in (1, 2, 3)) and 2000 < low < 18000, ({m: sorted(v) for m, v in margins.items()}, low)


def test_scan_form_of_the_seed_search():
    """the region as three scans of the search range (the highest position where it opens, the first failing window below, the lowest letter
    above that) and two refinements equals the statement-by-statement loop, for both letters, on strings rich in them"""
    rng = np.random.default_rng(7)
    found = 0
    for it in range(12000):
        n = int(rng.integers(0, 40))
        alpha = np.frombuffer([b"AC", b"AAAC", b"ATC", b"AaTtCN", b"AAAAAC", b"TTTC"][it % 6], np.uint8)
        s = alpha[rng.integers(0, alpha.size, n)].tobytes()
        seed = int(rng.choice([1, 2, 3, 4, 5, 10]))
        ident = F32(rng.choice([0.9, 0.5, 0.75, 1.0, 0.3]))
        a, b = int(rng.integers(0, n + 1)), int(rng.integers(0, n + 1))
        x = find_polya_seed(s, a, b, seed, ident)
        assert x == seed_by_scans(s, a, b, seed, ident), (s, a, b, seed, ident)
        y = find_polyt_seed(s, a, b, seed, ident)
        assert y == seed_t_by_scans(s, a, b, seed, ident), (s, a, b, seed, ident)
        found += (x is not None) + (y is not None)
    assert found > 2000
    # ... and so do the chains built on it
    for it in range(3000):
        n = int(rng.integers(0, 120))
        alpha = np.frombuffer([b"AAAC", b"TTTG", b"AAAAAAAACT"][it % 3], np.uint8)
        s = alpha[rng.integers(0, alpha.size, n)].tobytes()
        P = params(seed_length=int(rng.choice([3, 4, 10])), min_identity=float(rng.choice([0.9, 0.5])), max_gap=int(rng.integers(0, 6)),
                   window=int(rng.choice([5, 12, 30])))
        f, g = Finder(P), Finder(P, seed_by_scans, seed_t_by_scans)
        assert f.find_polya_tail(s) == g.find_polya_tail(s) and f.find_polyt_head(s) == g.find_polyt_head(s), (s, P)


def test_worker_chain_names_and_flags():
    c = [block("c", 100, i) for i in range(8)]
    lo = block("A", 100)
    reads = [c[0] + lo + c[1] + lo * 4 + c[2],                      # three segments
             BODY + b"A" * 12,                                       # one segment with a tail
             b"A" * 300,                                             # low complexity
             BODY[:10],                                              # too short
             BODY + BODY[:30],                                       # one segment, no tail
             BODY[:40] + BODY[:40]]                                  # one segment that is corrected to something but assembled into nothing
    names = [b"r%d" % i for i in range(len(reads))]
    calls = []

    def correct(segment, trim_edges):
        calls.append((segment, trim_edges))
        if segment == reads[0][:100]:                               # the first segment of read 0 comes back in two parts
            return [segment[:40], segment[60:]]
        if segment == reads[4]:
            return None                                              # lost: the corrected list is null or empty
        if segment == reads[5]:
            return []                                                # every k-mer without coverage and with a foreign letter: kept, nothing put out
        return [segment]

    out, kept, discarded = worker_chain(names, reads, params(), 25, 2, correct)
    s0 = prepare(reads[0], params())[1]
    assert s0 == [(0, 100), (200, 300), (700, 800)]
    assert [o[0] for o in out] == [b"r0_s1_p1", b"r0_s1_p2", b"r0_s2", b"r0_s3", b"r1", b"r2"]
    assert out[0][1:] == (reads[0][:40], 40, 40.0, False, False) and out[3][1] == reads[0][700:800]
    assert out[4] == (b"r1", reads[1], 72, 72.0, False, True)       # hasPolyA: no edge trim for it
    assert out[5] == (b"r2", reads[2], 300, 0.0, True, False)
    assert (kept, discarded) == (3, 3)                              # read 5 is kept although nothing of it is put out (:3839)
    assert [t for _, t in calls] == [True, True, True, False, True, True]




# ---- the feature exists at every layer (these fail before it does) ----
def test_header_declares_the_entry_point():
    src = open(os.path.join(ROOT, "include", "rb_capi.h")).read()
    assert re.search(r"typedef struct rb_prep_params \{\s*int32_t min_len, reverse_complement, strand_specific, polya, seed_length, max_gap, window, "
                     r"lc_window, lc_min_length;\s*float min_identity;\s*\} rb_prep_params;", src)
    rec = re.search(r"typedef struct rb_prep_rec \{([^}]*)\} rb_prep_rec;", src)
    assert rec and len(re.findall(r"\b[a-z_0-9]+(?:\[2\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", rec.group(1)))) == 15      # 14 ints and reserved[2]
    assert re.search(r"\bint rb_long_prepare\(int device, const char \*seq, const int64_t \*offsets, int64_t n, const rb_prep_params \*p, "
                     r"const int64_t \*seg_offsets,\s*rb_prep_rec \*recs, int32_t \*out_segs, char \*out_seq, double \*kernel_ms\);", src)
    for cite in ("RNABloom.java:3700-3779", "PolyATailFinder.java:319-338", ":201-277", ":355-432", ":476-495", ":839-902", ":585-659", ":661-682", ":1120-1152"):
        assert cite in src, cite
    for name, value in (("SHORT", SHORT), ("LOW_COMPLEXITY", LOW_COMPLEXITY), ("SEGMENTS", SEGMENTS), ("REVCOMP", REVCOMP), ("HAS_POLYA", HAS_POLYA),
                        ("TAIL_FOUND", TAIL_FOUND), ("HEAD_FOUND", HEAD_FOUND), ("CUT_FIRED", CUT_FIRED), ("ROUTE_WINDOWS", ROUTE_WINDOWS),
                        ("ROUTE_WINDOWED", ROUTE_WINDOWED), ("ROUTE_WHOLE", ROUTE_WHOLE), ("MAPPED_TWICE", MAPPED_TWICE)):
        assert re.search(r"\bRB_PREP_%s = %d\b" % (name, value), src), name


def test_library_exports_and_python_binds_it():
    import ctypes as C
    from rnabloom import _native as N
    assert hasattr(C.CDLL(N.LIB_PATH), "rb_long_prepare")
    assert "rb_long_prepare" in {s[0] for s in N.SYMBOLS}
    assert C.sizeof(N.PrepParams) == 40 and [f[0] for f in N.PrepParams._fields_] == [f for f in DEFAULTS if f != "min_identity"] + ["min_identity"]
    assert (N.PREP_SHORT, N.PREP_LOW_COMPLEXITY, N.PREP_SEGMENTS) == (SHORT, LOW_COMPLEXITY, SEGMENTS)
    assert (N.PREP_REVCOMP, N.PREP_HAS_POLYA, N.PREP_TAIL_FOUND, N.PREP_HEAD_FOUND, N.PREP_CUT_FIRED, N.PREP_ROUTE_WINDOWS, N.PREP_ROUTE_WINDOWED,
            N.PREP_ROUTE_WHOLE, N.PREP_MAPPED_TWICE) == (REVCOMP, HAS_POLYA, TAIL_FOUND, HEAD_FOUND, CUT_FIRED, ROUTE_WINDOWS, ROUTE_WINDOWED,
                                                         ROUTE_WHOLE, MAPPED_TWICE)
    from rnabloom import graphutils
    assert graphutils.PREP_DTYPE.itemsize == 64 and graphutils.PREP_DTYPE.names[:14] == FIELDS[:14]
    for f in ("prepareLongReads", "prepareLongFlat", "correctLongReadsFromRaw", "prepSegmentRoom"):
        assert callable(getattr(graphutils, f, None)), f
    assert graphutils.prepSegmentRoom([0, 0, 99, 199, 499, 999], 100).tolist() == [0, 1, 2, 3, 5, 8]      # max(1, (len / 100 + 1) / 2): 1 1 1 2 3


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from rnabloom import _native as N
    from rnabloom import graphutils
    with pytest.raises(N.NativeError) as e:
        graphutils.prepareLongReads([BODY + b"A" * 20], 25)
    assert "hip" in str(e.value).lower()
    # ... while an argument error is the library's own, device or not
    with pytest.raises(N.NativeError) as e:
        graphutils.prepareLongReads([BODY], 25, seedLength=0)
    assert "rb_long_prepare: seed_length = 0" in str(e.value)


def test_java_and_jni_sides_exist():
    java = open(os.path.join(ROOT, "java", "rnabloom", "graph", "NativeGraph.java")).read()
    assert re.search(r"public static native void longPrepare\(int device, ByteBuffer seq, long\[\] offsets, int n, int\[\] params, float minIdentity,", java)
    jni = open(os.path.join(ROOT, "jni", "rb_jni.c")).read()
    assert "FN(longPrepare)" in jni and "rb_long_prepare(" in jni
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "NativeGraph.longPrepare" in text and "LongReadCorrectionWorker" in text
