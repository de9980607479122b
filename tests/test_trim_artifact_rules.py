"""GraphUtils.trimReverseComplementArtifact — the three overloads rb_graph_trim_rc_artifacts answers — restated line by line in Python over the
CPU oracle: (kmers, graph, stranded) (R/util/GraphUtils.java:8588-8661, mode HASHES), (seqKmers, maxEdgeClip, maxIndelSize, minPercentIdentity,
graph) (:7918-8057, EDGE) and the seven-argument one (:7762-7916, LONG), with getMinimumKmerCoverage (:133-145), getMedianKmerCoverage
(:208-217 over Common.getMedian) and SeqUtils.isReverseComplement (R/util/SeqUtils.java:1257-1271).  The oracle supplies what getKmers gives a
Kmer: its forward hash, its reverse-strand hash and its count.  A restatement returns the list it was asked to return and the passes' fields;
`judge` makes the 16 ints of rb_trim_rec of them and collects the names of the branches taken.
The worlds of tests/test_gpu_trim_artifacts.py are built here (k = 25 stranded and canonical, k = 143, hash counts 1 / 3 / 3, and the k = 64
world of tests/traversal_worlds.py whose k-mers all hash to 0); every `why` of every mode and pass and every quirk the device test relies on
is shown here to be reached by the queries, on the oracle alone.  No device is needed."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import rbo
from traversal_worlds import ACGT, _prime_above, hash_equal_world, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASHES, EDGE, LONG = 0, 1, 2
FOUND, TRIMMED, BAD_LETTER, NO_KMER, NOT_JUDGED = 1, 2, 8, 16, 32
BLANK = [-1, -1, -1, -1, -1]
F32 = np.float32
LDS_LIST = 512                      # the list length at which the kernel's hash table leaves LDS: both sides are in the worlds

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def sint(v):
    """a Java long of the 64 bits v"""
    v = int(v)
    return v - (1 << 64) if v >= 1 << 63 else v


class Kmer:
    """what the restatements read of a Kmer (R/graph/Kmer.java:57-63) or, in a canonical graph, a CanonicalKmer (R/graph/CanonicalKmer.java:51-58,
    :93-99); idx is its place in the input list"""
    __slots__ = ("bytes", "f", "r", "count", "stranded", "idx", "h", "rch")

    def __init__(self, text, f, r, count, stranded, idx):
        self.bytes, self.f, self.r, self.count, self.stranded, self.idx = text, sint(f), sint(r), F32(count), stranded, idx
        self.h = self.f if stranded else min(self.f, self.r)         # getHash(): fHashVal; CanonicalKmer: Math.min(fHashVal, rHashVal)
        self.rch = self.r if stranded else self.h                    # getReverseComplementHash(): NTP64RC(bytes); CanonicalKmer: getHash()

    def getHash(self):
        return self.h

    def getReverseComplementHash(self):
        return self.rch

    def getFHash(self):
        return self.f

    def getRHash(self):
        return self.r


def complement(b):
    return _COMP[b]


def isReverseComplement(seq1, seq2):
    """R/util/SeqUtils.java:1257-1271"""
    ln = len(seq1)
    if ln == 0 or len(seq2) != ln:
        return False
    for i in range(ln):
        if complement(seq1[i]) != seq2[ln - 1 - i]:
            return False
    return True


def getMinimumKmerCoverage(kmers, start, end):
    """:133-145 — k-mer `start` counts whatever `end` is"""
    mn = kmers[start].count
    for i in range(start + 1, end):
        c = kmers[i].count
        if c < mn:
            mn = c
    return mn


def getMedianKmerCoverage(kmers, start, end):
    """:208-217 over Common.getMedian (R/util/Common.java:41-50): float32 throughout"""
    covs = sorted(kmers[start + i].count for i in range(end - start))
    half = len(covs) // 2
    if len(covs) % 2 == 0:
        return F32(F32(covs[half] + covs[half - 1]) / F32(2.0))
    return covs[half]


def matches(seed, candidate):
    return candidate.h == seed.rch and isReverseComplement(seed.bytes, candidate.bytes)


_INDEX = {}


def candidates(kmers, h, start, stop, step):
    """the j of range(start, stop, step) with kmers[j].h == h, in that order: the candidates a scan `for j ...: if candidate.getHash() == h
    && ...` does not pass over at once.  (The places of every hash in a list are looked up once per list: a scan of a list of some
    thousand k-mers under a wide clip is millions of comparisons otherwise.)"""
    ent = _INDEX.get("list")
    if ent is None or ent[0] is not kmers:
        by = {}
        for j, km in enumerate(kmers):
            by.setdefault(km.h, []).append(j)
        ent = _INDEX["list"] = (kmers, by)
    pos = ent[1].get(h, ())
    return [j for j in pos if start <= j < stop] if step > 0 else [j for j in reversed(pos) if stop < j <= start]


# ---- mode HASHES (:8588-8661) ----
def trim_hashes(kmers, k, stranded, tags):
    """-> (the list returned or None, pass 0)"""
    numKmers = len(kmers)
    hash_of = (lambda km: km.getHash()) if stranded else (lambda km: km.getFHash())
    rc_of = (lambda km: km.getReverseComplementHash()) if stranded else (lambda km: km.getRHash())
    left = set()
    for i in range(numKmers // 2):
        left.add(rc_of(kmers[i]))
    if 0 in left: tags.add("hashes_set_holds_hash_0")
    start, numMatch = -1, 0
    for i in range(numKmers // 2, numKmers):
        if hash_of(kmers[i]) in left:
            if start < 0:
                start = i
            numMatch += 1
            if hash_of(kmers[i]) == 0: tags.add("hashes_hash_0_found")
            if not any(rc_of(kmers[j]) == hash_of(kmers[i]) and isReverseComplement(kmers[j].bytes, kmers[i].bytes) for j in range(numKmers // 2)):
                tags.add("hashes_counts_a_kmer_that_is_no_reverse_complement")
    at_8610 = (start, numMatch)
    if numMatch == k - 1: tags.add("hashes_num_match_k_minus_1")
    if numMatch == k: tags.add("hashes_num_match_k")
    if numMatch >= k:
        if start > numKmers // 2:
            tags.add("hashes_why_1")
            return kmers[start:numKmers], [1, at_8610[0], at_8610[1], start, -1]
        elif start == numKmers // 2:
            for i in range(numKmers // 2, -1, -1):                 # need to adjust start position: no break
                if hash_of(kmers[i]) in left:
                    start = i
                    numMatch += 1
            tags.add("hashes_why_2")
            tags.add("hashes_start_stays" if start == numKmers // 2 else "hashes_start_adjusted_to_0" if start == 0 else "hashes_start_adjusted_down")
            return kmers[start:numKmers], [2, at_8610[0], at_8610[1], start, -1]
    tags.add("hashes_why_0")
    return None, [0, at_8610[0], at_8610[1], -1, -1]


# ---- mode EDGE (:7918-8057) ----
def trim_edge(seqKmers, maxEdgeClip, k, tags):
    """-> (the list returned, pass 0, pass 1)"""
    # search from left to right
    numKmers = len(seqKmers)
    leftIndex = rightIndex = -1
    indexToStop = min(maxEdgeClip, numKmers)
    if maxEdgeClip > numKmers: tags.add("edge_clip_above_nk")
    for i in range(indexToStop):
        seed = seqKmers[i]
        rcHashVal = seed.rch
        for j in candidates(seqKmers, rcHashVal, i + 1, numKmers, 1):
            candidate = seqKmers[j]
            if candidate.h == rcHashVal and isReverseComplement(seed.bytes, candidate.bytes):
                if leftIndex == 0: tags.add("edge_seed0_match_overwritten")
                leftIndex, rightIndex = i, j
                break
        if leftIndex > 0:
            break
    if leftIndex == 0: tags.add("edge_seed0_match_survives")
    p0 = [0, leftIndex, rightIndex, -1, -1]
    if leftIndex > 0 and rightIndex - leftIndex >= k:
        cutIndex = leftIndex + 1
        steps = 0
        for i in range(k, rightIndex - leftIndex, k):
            if matches(seqKmers[leftIndex + i], seqKmers[rightIndex - i]):
                cutIndex = leftIndex + i
                steps += 1
            else:
                tags.add("edge_p0_stride_breaks_at_first_step" if steps == 0 else "edge_p0_stride_breaks_later")
                break
        else:
            tags.add("edge_p0_stride_runs_out" if steps else "edge_p0_stride_has_no_step")
        for i in range(cutIndex - leftIndex, rightIndex - leftIndex):
            if matches(seqKmers[leftIndex + i], seqKmers[rightIndex - i]):
                cutIndex = leftIndex + i
            else:
                tags.add("edge_p0_unit_breaks")
                break
        else:
            tags.add("edge_p0_unit_runs_out")
        if cutIndex > (leftIndex + rightIndex) // 2: tags.add("edge_p0_cut_held_at_midpoint")
        cutIndex = min(cutIndex, (leftIndex + rightIndex) // 2)
        p0[3] = cutIndex
        if rightIndex >= numKmers - maxEdgeClip:
            cutLength = cutIndex - leftIndex
            p0[4] = cutLength
            leftMinCov = getMinimumKmerCoverage(seqKmers, cutIndex, min(numKmers, cutIndex + k))
            rightMinCov = getMinimumKmerCoverage(seqKmers, max(0, numKmers - cutLength - k), numKmers - cutLength)
            tags.add("edge_p0_left_min_%s_right_min" % ("above" if leftMinCov > rightMinCov else "equals" if leftMinCov == rightMinCov else "below"))
            if leftMinCov > rightMinCov:
                p0[0] = 1
                seqKmers = seqKmers[0:max(1, numKmers - cutLength - k)]
            else:
                p0[0] = 2
                seqKmers = seqKmers[cutIndex:numKmers]
        else:
            p0[0] = 3
            seqKmers = seqKmers[min(numKmers - 1, cutIndex + k):numKmers]
    tags.add("edge_p0_why_%d" % p0[0])
    # search from right to left
    numKmers = len(seqKmers)
    leftIndex = rightIndex = -1
    indexToStop = max(0, numKmers - 1 - maxEdgeClip)
    for i in range(numKmers - 1, indexToStop - 1, -1):
        seed = seqKmers[i]
        rcHashVal = seed.rch
        for j in candidates(seqKmers, rcHashVal, i - 1, -1, -1):
            candidate = seqKmers[j]
            if candidate.h == rcHashVal and isReverseComplement(seed.bytes, candidate.bytes):
                rightIndex, leftIndex = i, j
                break
        if rightIndex > 0:
            break
    p1 = [0, leftIndex, rightIndex, -1, -1]
    if rightIndex > 0 and rightIndex - leftIndex >= k:
        cutIndex = rightIndex - 1
        steps = 0
        for i in range(k, rightIndex - leftIndex, k):
            if matches(seqKmers[rightIndex - i], seqKmers[leftIndex + i]):
                cutIndex = rightIndex - i
                steps += 1
            else:
                tags.add("edge_p1_stride_breaks_at_first_step" if steps == 0 else "edge_p1_stride_breaks_later")
                break
        else:
            tags.add("edge_p1_stride_runs_out" if steps else "edge_p1_stride_has_no_step")
        for i in range(rightIndex - cutIndex, rightIndex - leftIndex):
            if matches(seqKmers[rightIndex - i], seqKmers[leftIndex + i]):
                cutIndex = rightIndex - i
            else:
                tags.add("edge_p1_unit_breaks")
                break
        else:
            tags.add("edge_p1_unit_runs_out")
        cutIndex = max(cutIndex, (rightIndex + leftIndex) // 2)
        p1[3] = cutIndex
        if leftIndex < maxEdgeClip:
            cutLength = rightIndex - cutIndex
            p1[4] = cutLength
            leftMinCov = getMinimumKmerCoverage(seqKmers, cutLength, min(cutLength + k, numKmers))
            rightMinCov = getMinimumKmerCoverage(seqKmers, max(0, cutIndex - k), cutIndex)
            tags.add("edge_p1_left_min_%s_right_min" % ("above" if leftMinCov > rightMinCov else "equals" if leftMinCov == rightMinCov else "below"))
            if leftMinCov > rightMinCov:
                p1[0] = 1
                seqKmers = seqKmers[0:max(1, cutIndex - k)]
            else:
                p1[0] = 2
                seqKmers = seqKmers[min(cutLength + k, numKmers - 1):numKmers]
        else:
            p1[0] = 3
            seqKmers = seqKmers[0:max(1, cutIndex - k)]
    elif rightIndex > 0:
        tags.add("edge_p1_pair_closer_than_k")
    tags.add("edge_p1_why_%d" % p1[0])
    return seqKmers, p0, p1


# ---- mode LONG (:7762-7916) ----
def trim_long(seqKmers, k, stranded, maxEdgeClip, maxCovGradient, tags):
    """-> ((begin, end) of the subList returned, pass 0, pass 1 or BLANK)"""
    maxCovGradient = F32(maxCovGradient)
    minMatchLen = 2 * k
    numKmers = len(seqKmers)

    def cmp_tag(p, what, a, b):
        tags.add("long_p%d_%s_%s" % (p, what, "lt" if a < b else "eq" if a == b else "gt"))

    # scan from left to right
    anchorStartIndex = anchorEndIndex = partnerStartIndex = partnerEndIndex = -1
    anchorStopIndex = min(numKmers, maxEdgeClip)
    if maxEdgeClip > numKmers: tags.add("long_clip_above_nk")
    for i in range(anchorStopIndex):
        seed = seqKmers[i]
        rcHashVal = seed.rch
        for j in candidates(seqKmers, rcHashVal, i + 1, numKmers, 1):
            candidate = seqKmers[j]
            if candidate.h == rcHashVal and isReverseComplement(seed.bytes, candidate.bytes):
                if anchorStartIndex == 0: tags.add("long_seed0_match_overwritten")
                anchorStartIndex = anchorEndIndex = i
                partnerStartIndex = partnerEndIndex = j
                break
        if anchorStartIndex > 0:
            break
    if anchorStartIndex == 0: tags.add("long_seed0_match_survives")
    p0 = [0, anchorStartIndex, anchorEndIndex, partnerStartIndex, partnerEndIndex]
    if anchorStartIndex > 0:
        midPointIndex = (anchorStartIndex + partnerStartIndex) // 2
        for i in range(anchorEndIndex + 1, midPointIndex):
            seed = seqKmers[i]
            for j in range(partnerStartIndex - 1, midPointIndex - 1, -1):
                if matches(seed, seqKmers[j]):
                    anchorEndIndex = i
                    partnerStartIndex = j
                    break
        p0 = [1, anchorStartIndex, anchorEndIndex, partnerStartIndex, partnerEndIndex]
        for what, ln in (("anchor", anchorEndIndex - anchorStartIndex), ("partner", partnerEndIndex - partnerStartIndex)):
            if ln == minMatchLen - 1: tags.add("long_p0_%s_length_2k_minus_1" % what)
            if ln == minMatchLen: tags.add("long_p0_%s_length_2k" % what)
        if anchorStartIndex > 0 and anchorEndIndex - anchorStartIndex >= minMatchLen and partnerEndIndex - partnerStartIndex >= minMatchLen:
            anchorEndIndex += 1
            partnerEndIndex += 1
            if stranded:
                anchorCov = getMedianKmerCoverage(seqKmers, anchorStartIndex, anchorEndIndex)
                middleCov = getMedianKmerCoverage(seqKmers, anchorEndIndex, partnerStartIndex) if anchorEndIndex < partnerStartIndex else F32(0)
                if not anchorEndIndex < partnerStartIndex: tags.add("long_p0_no_middle")
                partnerCov = getMedianKmerCoverage(seqKmers, partnerStartIndex, partnerEndIndex)
                cmp_tag(0, "anchor_partner", anchorCov, partnerCov)
                if anchorCov < partnerCov:
                    cmp_tag(0, "a_middle_anchor", middleCov, anchorCov)
                    if middleCov >= anchorCov: cmp_tag(0, "a_middle_gradient", middleCov, F32(partnerCov * maxCovGradient))
                    if middleCov >= anchorCov and middleCov >= F32(partnerCov * maxCovGradient):
                        p0[0] = 3; out = (anchorEndIndex, numKmers)
                    else:
                        p0[0] = 4; out = (partnerStartIndex, numKmers)
                else:
                    cmp_tag(0, "b_middle_partner", middleCov, partnerCov)
                    if middleCov > partnerCov: cmp_tag(0, "b_middle_gradient", middleCov, F32(anchorCov * maxCovGradient))
                    if middleCov > partnerCov and middleCov >= F32(anchorCov * maxCovGradient):
                        p0[0] = 5; out = (0, partnerStartIndex)
                    else:
                        p0[0] = 6; out = (0, anchorEndIndex)
            else:
                p0[0] = 2; out = (anchorEndIndex, partnerStartIndex)
            tags.add("long_p0_why_%d" % p0[0])
            if out[0] == out[1]: tags.add("long_empty_range")
            return out, p0, list(BLANK)
    tags.add("long_p0_why_%d" % p0[0])
    # scan from right to left
    anchorStartIndex = anchorEndIndex = partnerStartIndex = partnerEndIndex = -1
    anchorStopIndex = max(0, numKmers - maxEdgeClip)
    for i in range(numKmers - 1, anchorStopIndex - 1, -1):
        seed = seqKmers[i]
        rcHashVal = seed.rch
        for j in candidates(seqKmers, rcHashVal, i - 1, -1, -1):
            candidate = seqKmers[j]
            if candidate.h == rcHashVal and isReverseComplement(seed.bytes, candidate.bytes):
                anchorStartIndex = anchorEndIndex = i
                partnerStartIndex = partnerEndIndex = j
                break
        if anchorStartIndex > 0:
            break
    p1 = [0, anchorStartIndex, anchorEndIndex, partnerStartIndex, partnerEndIndex]
    if anchorStartIndex > 0:
        midPointIndex = (anchorStartIndex + partnerStartIndex) // 2
        for i in range(anchorStartIndex - 1, midPointIndex, -1):
            seed = seqKmers[i]
            for j in range(partnerEndIndex + 1, midPointIndex + 1):
                if matches(seed, seqKmers[j]):
                    anchorStartIndex = i
                    partnerEndIndex = j
                    break
        p1 = [1, anchorStartIndex, anchorEndIndex, partnerStartIndex, partnerEndIndex]
        for what, ln in (("anchor", anchorEndIndex - anchorStartIndex), ("partner", partnerEndIndex - partnerStartIndex)):
            if ln == minMatchLen - 1: tags.add("long_p1_%s_length_2k_minus_1" % what)
            if ln == minMatchLen: tags.add("long_p1_%s_length_2k" % what)
        if anchorStartIndex > 0 and anchorEndIndex - anchorStartIndex >= minMatchLen and partnerEndIndex - partnerStartIndex >= minMatchLen:
            anchorEndIndex += 1
            partnerEndIndex += 1
            if stranded:
                partnerCov = getMedianKmerCoverage(seqKmers, partnerStartIndex, partnerEndIndex)
                middleCov = getMedianKmerCoverage(seqKmers, partnerEndIndex, anchorStartIndex) if partnerEndIndex < anchorStartIndex else F32(0)
                if not partnerEndIndex < anchorStartIndex: tags.add("long_p1_no_middle")
                anchorCov = getMedianKmerCoverage(seqKmers, anchorStartIndex, anchorEndIndex)
                cmp_tag(1, "partner_anchor", partnerCov, anchorCov)
                if partnerCov > anchorCov:
                    cmp_tag(1, "a_middle_anchor", middleCov, anchorCov)
                    if middleCov > anchorCov: cmp_tag(1, "a_middle_gradient", middleCov, F32(partnerCov * maxCovGradient))
                    if middleCov > anchorCov and middleCov >= F32(partnerCov * maxCovGradient):
                        p1[0] = 3; out = (0, anchorStartIndex)
                    else:
                        p1[0] = 4; out = (0, partnerEndIndex)
                else:
                    cmp_tag(1, "b_middle_partner", middleCov, partnerCov)
                    if middleCov > partnerCov: cmp_tag(1, "b_middle_gradient", middleCov, F32(anchorCov * maxCovGradient))
                    if middleCov > partnerCov and middleCov >= F32(anchorCov * maxCovGradient):
                        p1[0] = 5; out = (partnerEndIndex, numKmers)
                    else:
                        p1[0] = 6; out = (anchorStartIndex, numKmers)
            else:
                p1[0] = 2; out = (partnerEndIndex, anchorStartIndex)
            tags.add("long_p1_why_%d" % p1[0])
            if out[0] == out[1]: tags.add("long_empty_range")
            return out, p0, p1
    tags.add("long_p1_why_%d" % p1[0])
    return None, p0, p1


# ---- the record ----
def kmers_of(og, k, stranded, seq):
    """the getKmers list of an upper-case ACGT sequence: counts from the oracle's getKmers; forward and reverse-strand hash of every k-mer
    from its canonical hash iterator (a stranded graph's getKmers row holds 0 for the reverse strand: Kmer computes NTP64RC when asked)"""
    f, r, c = og.get_kmers(seq)
    fr = rbo.hash_region(seq, k, 1, rbo.CANON)[1] if len(seq) >= k else np.zeros((0, 2), np.uint64)
    assert (fr[:, 0] == f).all() and (stranded or (fr[:, 1] == r).all())
    return [Kmer(seq[i:i + k], fr[i, 0], fr[i, 1], c[i], stranded, i) for i in range(len(f))]


def judge(og, k, stranded, seq, mode, clip=0, grad=0.0, tags=None):
    """what rb_graph_trim_rc_artifacts reports for one sequence: (the 16 ints, the string the returned k-mers spell — None for HASHES' null)"""
    tags = set() if tags is None else tags
    plain = seq.upper().replace(b"U", b"T")
    nk = max(0, len(seq) - k + 1)
    if nk == 0 or any(c not in b"ACGT" for c in plain):
        return [NO_KMER if nk == 0 else BAD_LETTER, 0, nk, mode] + BLANK + BLANK + [0, 0], seq
    kmers = kmers_of(og, k, stranded, plain)
    tags.add("nk_%s" % ("odd" if nk % 2 else "even"))
    if nk <= 3: tags.add("nk_%d" % nk)
    found, begin, end, p1 = False, 0, nk, list(BLANK)
    if mode == HASHES:
        res, p0 = trim_hashes(kmers, k, stranded, tags)
        if res is not None:
            found, begin = True, res[0].idx
            assert [km.idx for km in res] == list(range(begin, nk))
    elif mode == EDGE:
        res, p0, p1 = trim_edge(kmers, clip, k, tags)
        found, begin, end = bool(p0[0] or p1[0]), res[0].idx, res[-1].idx + 1
        assert [km.idx for km in res] == list(range(begin, end))
    else:
        rng, p0, p1 = trim_long(kmers, k, stranded, clip, grad, tags)
        if rng is not None:
            found, (begin, end) = True, rng
    flags = (FOUND if found else 0) | (TRIMMED if begin > 0 or end < nk else 0)
    if found and not flags & TRIMMED: tags.add("found_and_nothing_trimmed")
    text = None if mode == HASHES and not found else seq[begin:end + k - 1] if end > begin else seq[:0]
    return [flags, begin, end, mode] + p0 + p1 + [0, 0], text


# ---- worlds ----
class TrimWorld:
    """an oracle graph of `reads`, the queries (name, sequence) and the settings (mode, max_edge_clip, max_cov_gradient) they are judged under"""

    def __init__(self, k, stranded, hashes, reads, queries, settings, og=None):
        self.k, self.stranded, self.hashes, self.reads, self.queries, self.settings = k, stranded, hashes, list(reads), list(queries), tuple(settings)
        self.names = [nm for nm, _ in queries]
        distinct = sum(max(0, len(r) - k + 1) for r in reads)
        self.sizes = (_prime_above(40 * distinct + 1000), _prime_above(20 * distinct + 1000), 64)
        self.seq, self.off = pack(self.reads)
        if og is None:
            og = rbo.Graph(*self.sizes, *hashes, k, stranded, False, 3)
            og.add_reads(self.seq, None, self.off, 3, 0)
        self.og = og
        self.tags = {}

    @functools.lru_cache(maxsize=None)
    def judged(self, mode, clip=0, grad=0.0):
        """[(record, text) per query] under one setting; the branches taken are added to self.tags[mode]"""
        tags = self.tags.setdefault(mode, set())
        return [judge(self.og, self.k, self.stranded, s, mode, clip, grad, tags) for _, s in self.queries]

    def all_tags(self):
        for st in self.settings:
            self.judged(*st)
        return set().union(*self.tags.values())


def hairpin_queries(k, rng, full=True):
    """(queries, reads that raise the coverage of parts of them).  U, V, X are stems, M a loop, L / T letters before and behind; a stem's
    k-mers pair with those of its reverse complement on one anti-diagonal."""
    rnd = lambda n: bytes(ACGT[rng.integers(0, 4, n)])
    q, boosts = [], []
    add = lambda name, s: q.append((name, s))
    X60, X30, L5, T100, T40, M40 = rnd(2 * k + 10), rnd(k + 5), rnd(5), rnd(4 * k), rnd(k + 15), rnd(k + 15)
    P = X60 + revcomp(X60)
    add("plain", rnd(6 * k))
    add("hairpin", P)                                             # seed 0 matches: survives under clip 1, is overwritten under a wider one
    add("hairpin-one-letter-behind", P + b"A")
    add("self-complementary-twice", P + P)                       # HASHES: start adjusted down to 0
    add("hairpin-then-letters", P + rnd(10))                     # HASHES: start adjusted down part of the way
    add("letters-then-twice", rnd(10) + P + P)                   # HASHES: start beyond the half
    # HASHES: numMatch around k.  P has 3 k + 21 k-mers and all of the right half match: 3 k + 21 - (3 k + 21 + z) // 2 of them, which is k
    # for z = k + 21 and k - 1 for z = k + 23 (the reduced set keeps the letters it has: 2 k - 6 ... is k + 19 ... at k = 25 alone)
    for z in ((k + 19 + 2 * t if full else 2 * k - 6 + 2 * t) for t in range(5)):
        add("hairpin-then-%d-letters" % z, P + rnd(z))
    add("prefix-hairpin", L5 + P)
    add("prefix-hairpin-tail", L5 + P + T100)                    # EDGE pass 0: the partner is far from the right end
    add("prefix-short-stems-loop", L5 + X30 + M40 + revcomp(X30))                # EDGE: the stride loop breaks at its first step
    add("prefix-short-stems-loop-tail", L5 + X30 + M40 + revcomp(X30) + T40)
    Xs = X60[:k + 12] + bytes([_COMP[X60[k + 12]]]) + X60[k + 13:]
    add("prefix-hairpin-one-letter-off", L5 + X60 + revcomp(Xs))  # EDGE: the runs break inside the stems
    add("tail-hairpin-suffix", T40 + P + L5)                     # the right-to-left passes
    add("tail-hairpin", T40 + P)
    add("tail-short-stems-loop-suffix", T40 + X30 + M40 + revcomp(X30) + L5)
    add("tail-hairpin-one-letter-off", T40 + X60 + revcomp(Xs) + L5)
    add("two-hairpins", L5 + P + T100 + revcomp(P) + L5)
    # coverage: the same shapes with parts of them seen more often
    for t, (a, b, c) in enumerate(((0, 0, 3), (3, 0, 0), (0, 3, 0), (2, 2, 0), (0, 2, 2), (1, 3, 1), (3, 1, 3))[:7 if full else 2]):
        lft, mid, rgt, tail = rnd(2 * k + 10), rnd(k + 15), None, rnd(k + 5)
        rgt = revcomp(lft)
        for name, s in (("cov%d-prefix" % t, L5 + lft + mid + rgt + tail), ("cov%d-tail" % t, rnd(k + 15) + lft + mid + rgt + L5),
                        ("cov%d-tight" % t, L5 + lft + rgt + tail[:8])):
            add(name, s)
        boosts += [lft] * a + [lft[-k + 1:] + mid + rgt[:k - 1]] * b + [rgt] * c
    # LONG: stems of 2k - 1 + k and 2k + k letters (match lengths 2k - 1 and 2k), with and without a loop, at either end
    for stem in (3 * k - 1, 3 * k, 4 * k):
        for t, (a, b, c) in enumerate(((0, 0, 0), (3, 0, 0), (0, 0, 3), (0, 3, 0), (3, 3, 0), (0, 3, 3), (2, 4, 2), (4, 1, 1), (1, 1, 4), (3, 2, 3), (2, 0, 4), (4, 0, 2))):
            if (stem != 4 * k and t > 2) or (not full and t > 1):
                continue
            U, M = rnd(stem), rnd(k + 15)
            add("long%d-%d-prefix" % (stem, t), L5 + U + M + revcomp(U) + rnd(k))
            add("long%d-%d-tail" % (stem, t), rnd(2 * k) + U + M + revcomp(U) + L5)
            boosts += [U] * a + [U[-k + 1:] + M + revcomp(U)[:k - 1]] * b + [revcomp(U)] * c
    U, V = rnd(3 * k + 6), rnd(k + 10)
    for ins in (1, 2):                                            # LONG: an inner hairpin one anti-diagonal off: the unstranded return is empty
        for lead in (5, 6):
            add("long-inner-%d-%d" % (ins, lead), rnd(lead) + U + V + revcomp(V) + rnd(ins) + revcomp(U) + rnd(k))
        W = rnd(4 * k)
    add("long-tight", L5 + W + revcomp(W) + rnd(k))
    add("long-tight-tail", rnd(2 * k) + W + revcomp(W) + L5)
    if k % 2 == 0:
        # HASHES at an even k: a hairpin's list has an odd length and its middle k-mer is its own reverse complement, so the half never
        # begins on a match.  A letter behind P + P makes the list even (the start is adjusted down to 0 as at an odd k); and stems around a
        # loop of m letters with m + k - 1 letters behind them put the half on the right stem's first k-mer, whose partner is the left
        # stem's last: the start stays
        add("self-complementary-twice-one-letter-behind", P + P + b"A")
        add("stems-loop-tail-at-the-half", X60 + M40 + revcomp(X60) + rnd(len(M40) + k - 1))
    return q, boosts


def edge_cases(k, rng):
    rnd = lambda n: bytes(ACGT[rng.integers(0, 4, n)])
    s = rnd(k + 2)
    return [("no-kmer", s[:k - 1]), ("empty", b""), ("one-kmer", s[:k]), ("two-kmers", s[:k + 1]), ("three-kmers", s), ("with-an-N", s[:5] + b"N" + rnd(2 * k)),
            ("lower-case", (rnd(20) + revcomp(rnd(20))).lower()), ("with-a-U", s.replace(b"T", b"U", 1) + rnd(k))]


def tiling_queries(k, rng, full=True):
    """lists of 1, 2, 63, 64, 65, 128 and 129 k-mers (scans take 64 candidates at a time), each a hairpin behind one letter where it is long
    enough, and lists just below and just above LDS_LIST, where the hash table leaves LDS"""
    rnd = lambda n: bytes(ACGT[rng.integers(0, 4, n)])
    out = []
    for nk in (1, 2, 63, 64, 65, 128, 129, LDS_LIST - 1, LDS_LIST, LDS_LIST + 1, LDS_LIST + 300) if full else (1, 64, 65, LDS_LIST, LDS_LIST + 1):
        letters = nk + k - 1
        half = (letters - 1) // 2
        X = rnd(half)
        s = (b"G" + X + revcomp(X) + rnd(letters))[:letters] if nk > 2 else rnd(letters)
        assert len(s) - k + 1 == nk
        out.append(("tile-%d" % nk, s))
        out.append(("tile-%d-plain" % nk, rnd(letters)))
    return out


K25_SETTINGS = ((HASHES, 0, 0.0), (EDGE, 0, 0.0), (EDGE, 1, 0.0), (EDGE, 10, 0.0), (EDGE, 60, 0.0), (EDGE, 5000, 0.0),
                (LONG, 0, 0.5), (LONG, 1, 0.5), (LONG, 30, 0.5), (LONG, 30, 1.5), (LONG, 150, 0.1), (LONG, 5000, 0.5))


@functools.lru_cache(maxsize=None)
def world(k, stranded, hashes=(2, 2, 1)):
    rng = np.random.default_rng(7000 + k + (1 if stranded else 0))
    q, boosts = hairpin_queries(k, rng, k == 25)
    q += edge_cases(k, rng) + tiling_queries(k, rng, k == 25)
    reads = [s.upper().replace(b"U", b"T").replace(b"N", b"A") for _, s in q if len(s) >= k] + boosts
    settings = K25_SETTINGS if k == 25 else ((HASHES, 0, 0.0), (EDGE, 40, 0.0), (LONG, 40, 0.5))
    return TrimWorld(k, stranded, hashes, reads, q, settings)


@functools.lru_cache(maxsize=None)
def world_hash_equal(stranded):
    """the k = 64 world of tests/traversal_worlds.py: (AC)^32, (CA)^32, (GT)^32 and (TG)^32 all hash to f = r = 0.  (AC)^n (GT)^n is its own
    reverse complement; (AC)^n alone holds k-mers that hash alike and are no reverse complements of each other."""
    w = hash_equal_world(stranded)
    q = [("ac-100", b"AC" * 100), ("ac-gt", b"AC" * 60 + b"GT" * 60), ("g-ac-gt-t", b"G" + b"AC" * 70 + b"GT" * 70 + b"T"), ("ac-50", b"AC" * 50),
         ("ca-tg-behind-letters", b"TTGAC" + b"CA" * 80 + b"TG" * 80 + b"ACCGT")]
    tw = TrimWorld(64, stranded, (2, 2, 1), w.reads, q, ((HASHES, 0, 0.0), (EDGE, 10, 0.0), (EDGE, 500, 0.0), (LONG, 10, 0.5), (LONG, 500, 0.5)), og=w.og)
    tw.sizes = w.sizes + (64,)
    return tw


REQUIRED = {
    HASHES: {"hashes_why_0", "hashes_why_1", "hashes_why_2", "hashes_start_stays", "hashes_start_adjusted_down", "hashes_start_adjusted_to_0",
             "hashes_num_match_k_minus_1", "hashes_num_match_k", "found_and_nothing_trimmed", "nk_1", "nk_2", "nk_3", "nk_odd", "nk_even"},
    EDGE: {"edge_p0_why_%d" % i for i in range(4)} | {"edge_p1_why_%d" % i for i in range(4)} |
          {"edge_seed0_match_survives", "edge_seed0_match_overwritten", "edge_clip_above_nk", "edge_p0_stride_breaks_at_first_step", "edge_p0_stride_runs_out",
           "edge_p0_unit_breaks", "edge_p0_unit_runs_out", "edge_p0_cut_held_at_midpoint", "edge_p1_stride_breaks_at_first_step", "edge_p1_stride_runs_out",
           "edge_p1_unit_breaks", "edge_p1_unit_runs_out", "edge_p1_pair_closer_than_k"} |
          {"edge_p%d_left_min_%s_right_min" % (p, c) for p in (0, 1) for c in ("above", "equals", "below")},
}
LONG_BOTH = {"long_seed0_match_survives", "long_seed0_match_overwritten", "long_clip_above_nk", "long_p0_why_0", "long_p0_why_1", "long_p1_why_0", "long_p1_why_1",
             "long_p0_anchor_length_2k_minus_1", "long_p0_anchor_length_2k", "long_p1_anchor_length_2k_minus_1", "long_p1_anchor_length_2k"}
LONG_UNSTRANDED = LONG_BOTH | {"long_p0_why_2", "long_p1_why_2", "long_empty_range"}
LONG_STRANDED = LONG_BOTH | {"long_p%d_why_%d" % (p, y) for p in (0, 1) for y in (3, 4, 5, 6)} | {
    "long_p0_anchor_partner_lt", "long_p0_anchor_partner_eq", "long_p0_anchor_partner_gt", "long_p1_partner_anchor_lt", "long_p1_partner_anchor_eq",
    "long_p1_partner_anchor_gt", "long_p0_a_middle_anchor_lt", "long_p0_a_middle_anchor_eq", "long_p0_a_middle_anchor_gt", "long_p0_a_middle_gradient_lt",
    "long_p0_a_middle_gradient_gt", "long_p0_b_middle_partner_lt", "long_p0_b_middle_partner_eq", "long_p0_b_middle_partner_gt", "long_p0_b_middle_gradient_lt",
    "long_p0_b_middle_gradient_gt", "long_p1_a_middle_anchor_lt", "long_p1_a_middle_anchor_eq", "long_p1_a_middle_anchor_gt", "long_p1_a_middle_gradient_lt",
    "long_p1_a_middle_gradient_gt", "long_p1_b_middle_partner_lt", "long_p1_b_middle_partner_eq", "long_p1_b_middle_partner_gt", "long_p1_b_middle_gradient_lt",
    "long_p1_b_middle_gradient_gt", "long_p0_no_middle"}


def assert_every_branch_is_reached(w, excused=()):
    """on the oracle alone: every `why` of every mode and pass and every quirk of the issue's list is taken by a query of the k = 25 world
    (LONG's unstranded return in the canonical graph, its four stranded ones in the stranded graph)"""
    w.all_tags()
    for mode in (HASHES, EDGE):
        assert not REQUIRED[mode] - w.tags[mode], (w.stranded, sorted(REQUIRED[mode] - w.tags[mode]))
    want = (LONG_STRANDED if w.stranded else LONG_UNSTRANDED) - set(excused)
    assert not want - w.tags[LONG], (w.stranded, sorted(want - w.tags[LONG]))


@pytest.mark.parametrize("stranded", [False, True])
def test_every_branch_is_reached(stranded):
    assert_every_branch_is_reached(world(25, stranded))


# ---- toy cases worked by hand ----
def toy(stranded, reads):
    return TrimWorld(25, stranded, (2, 2, 1), reads, [], ())


X = b"GATTACAGGCTTAACCGGATCTTGCAGTCCATGGCAATCGTTAGCCTAAGGCTTCAGGAT"           # 60 letters
P = X + revcomp(X)                                                              # 120 letters, 96 k-mers: k-mer p is the reverse complement of k-mer 95 - p


@pytest.mark.parametrize("stranded", [False, True])
def test_hand_worked_hashes(stranded):
    t = toy(stranded, [P, b"ACCGT" + P])
    # half = 48; the set holds R[0 .. 47] = F[95 .. 48]: all 48 k-mers of the right half match, start == half, and no k-mer at or below the
    # half but k-mer 48 itself has its forward hash in the set
    rec, text = judge(t.og, 25, stranded, P, HASHES)
    assert rec == [FOUND | TRIMMED, 48, 96, HASHES, 2, 48, 48, 48, -1] + BLANK + [0, 0] and text == P[48:]
    # five letters in front: 101 k-mers, half = 50, k-mer p >= 5 pairs with 105 - p; the set holds R[5 .. 49] = F[100 .. 56] (and five unpaired hashes),
    # so the right half matches from 56 on: 45 k-mers, start beyond the half
    rec, text = judge(t.og, 25, stranded, b"ACCGT" + P, HASHES)
    assert rec == [FOUND | TRIMMED, 56, 101, HASHES, 1, 56, 45, 56, -1] + BLANK + [0, 0] and text == (b"ACCGT" + P)[56:]
    # 46 k-mers of the right half would have to match for a list of 46: a random sequence has none
    rec, text = judge(t.og, 25, stranded, X, HASHES)
    assert rec == [0, 0, 36, HASHES, 0, -1, 0, -1, -1] + BLANK + [0, 0] and text is None


@pytest.mark.parametrize("stranded", [False, True])
def test_hand_worked_edge(stranded):
    S = b"ACCGT" + P                                               # 101 k-mers; k-mer p >= 5 pairs with k-mer 105 - p
    t = toy(stranded, [S])
    # seeds 0 .. 4 hold a letter of the prefix and match nothing; seed 5 finds 100.  Strides 25, 50, 75 and the single steps up to 94 all
    # match: cutIndex 99, held at the midpoint 52; 100 >= 101 - 10; every k-mer of both windows has the same count, so the line :7981 cuts:
    # subList(52, 101).  In those 49 k-mers k-mer p' = p - 52 pairs with 1 - p': the ten seeds from the right find nothing.
    rec, text = judge(t.og, 25, stranded, S, EDGE, 10)
    assert rec == [FOUND | TRIMMED, 52, 101, EDGE, 2, 5, 100, 52, 47, 0, -1, -1, -1, -1, 0, 0] and text == S[52:]
    # ... 49 seeds from the right reach seed 1, whose partner is k-mer 0: closer than k
    rec, _ = judge(t.og, 25, stranded, S, EDGE, 47)
    assert rec == [FOUND | TRIMMED, 52, 101, EDGE, 2, 5, 100, 52, 47, 0, 0, 1, -1, -1, 0, 0]
    # the bare hairpin under clip 1: seed 0 finds 95, the scan is over and `leftIndex > 0` is false: nothing is cut from the left.  From the
    # right seeds 95 and 94: 95 finds 0; strides and steps run out at 1, held at the midpoint 47; leftIndex 0 < 1, cutLength 48, equal counts:
    # the line :8048, subList(min(73, 95), 96)
    rec, text = judge(t.og, 25, stranded, P, EDGE, 1)
    assert rec == [FOUND | TRIMMED, 73, 96, EDGE, 0, 0, 95, -1, -1, 2, 0, 95, 47, 48, 0, 0] and text == P[73:]
    # clip 0: no seed from the left, one from the right; 0 < 0 is false: the line :8052, subList(0, max(1, 47 - 25))
    rec, text = judge(t.og, 25, stranded, P, EDGE, 0)
    assert rec == [FOUND | TRIMMED, 0, 22, EDGE, 0, -1, -1, -1, -1, 3, 0, 95, 47, -1, 0, 0] and text == P[:22 + 24]


def test_hand_worked_long():
    U = X + b"TTGACCAGTACGGAT"                                       # 75 letters: 51 k-mers, a match length of 2k exactly
    M = b"CCATAGGAGTTTCACGAAGACTGATTCCAAGTTGCATCAA"                  # 40 letters; its first and last are no complements
    S = b"ACCGT" + U + M + revcomp(U) + b"GGATTTACAGCACTTAGGCATCCAA"
    t = toy(False, [S])
    # k-mers 5 .. 55 lie in U, their partners 170 .. 120 in its reverse complement (p + q = 175); seed 5 anchors at 170, midpoint 87; the
    # extension takes anchorEnd to 55 and partnerStart to 120: 50 >= 50 on both sides; unstranded: subList(56, 120)
    rec, text = judge(t.og, 25, False, S, LONG, 30, 0.5)
    assert rec == [FOUND | TRIMMED, 56, 120, LONG, 2, 5, 55, 120, 170] + BLANK + [0, 0] and text == S[56:120 + 24]
    # one letter less of U: k-mers 5 .. 54 pair with 168 .. 119 (p + q = 173) and 49 < 50: the match-length test fails.  From the right the
    # seeds 193 .. 169 hold a letter of the tail; seed 168 anchors at 5, the extension takes anchorStart down to 119 and partnerEnd up to 54:
    # 49 < 50 again, and the list comes back as it is
    S2 = b"ACCGT" + U[:-1] + M + revcomp(U[:-1]) + b"GGATTTACAGCACTTAGGCATCCAA"
    t2 = toy(False, [S2])
    rec, text = judge(t2.og, 25, False, S2, LONG, 30, 0.5)
    assert rec == [0, 0, 194, LONG, 1, 5, 54, 119, 168, 1, 119, 168, 5, 54, 0, 0] and text == S2


# ---- the two strandednesses of HASHES read the same two hashes ----
def test_both_branches_of_hashes_read_the_forward_and_the_reverse_strand_hash():
    """the stranded branch asks getHash() / getReverseComplementHash() of a Kmer — fHashVal and NTP64RC(bytes) —, the canonical one getFHash() /
    getRHash(): with (f, r) of the canonical hash iterator both are f and r.  A stranded graph's getKmers row does not hold r (it is 0 there):
    the kernel computes it."""
    for stranded in (False, True):
        w = world(25, stranded)
        s = dict(w.queries)["prefix-hairpin"]
        f, r, _ = w.og.get_kmers(s)
        kms = kmers_of(w.og, 25, stranded, s)
        rc_text = revcomp(s)
        f_rc = rbo.hash_region(rc_text, 25, 1, rbo.CANON)[1][:, 0]
        assert [km.r for km in kms] == [sint(x) for x in f_rc[::-1]]          # NTP64RC of a k-mer: the forward hash of its reverse complement
        if stranded:
            assert not r.any() and all(km.getHash() == km.f and km.getReverseComplementHash() == km.r for km in kms)
        else:
            assert all(km.getFHash() == sint(a) and km.getRHash() == sint(b) for km, a, b in zip(kms, f, r))
        as_other = trim_hashes([Kmer(km.bytes, km.f, km.r, km.count, not stranded, km.idx) for km in kms], 25, not stranded, set())[1]
        assert as_other == trim_hashes(kms, 25, stranded, set())[1]


# ---- k-mers that hash alike ----
@pytest.mark.parametrize("stranded", [False, True])
def test_hash_equal_world(stranded):
    w = world_hash_equal(stranded)
    f, r, _ = w.og.get_kmers(b"AC" * 40)
    assert not f.any() and not rbo.hash_region(b"AC" * 40, 64, 1, rbo.CANON)[1].any()
    w.all_tags()
    assert {"hashes_set_holds_hash_0", "hashes_hash_0_found", "hashes_counts_a_kmer_that_is_no_reverse_complement"} <= w.tags[HASHES]
    by = {nm: rec for nm, (rec, _) in zip(w.names, w.judged(HASHES))}
    assert by["ac-100"][:9] == [FOUND, 0, 137, HASHES, 2, 68, 69, 0, -1]          # every k-mer of (AC)^100 counts: none is the reverse complement of another
    assert by["ac-50"][4:7] == [0, 18, 19]
    for mode, clip in ((EDGE, 500), (LONG, 500)):
        by = {nm: rec for nm, (rec, _) in zip(w.names, w.judged(mode, clip, 0.5 if mode == LONG else 0.0))}
        assert by["ac-100"][0] == 0 and by["ac-100"][5:7] == [-1, -1]              # rejected on the bases, 137 x 136 / 2 times
        # the real reverse complements among them are found: seed 0, (AC)^32, meets a (GT)^32 and seed 1, (CA)^32, overwrites it with (TG)^32
        # at 121; EDGE cuts there, LONG's match lengths stay below 2k (the extension goes through a tandem repeat)
        assert by["ac-gt"][5] == 1 and by["ac-gt"][4] == (2 if mode == EDGE else 1), by["ac-gt"]
        assert (by["ac-gt"][0] & FOUND != 0) == (mode == EDGE)


# ---- structure: fails before the call exists ----
def test_the_header_declares_the_call_and_a_record_of_16_ints():
    src = open(os.path.join(ROOT, "include", "rb_capi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+rb_graph_trim_rc_artifacts\s*\(\s*rb_graph\s*\*\s*g\s*,\s*const\s+char\s*\*\s*seq\s*,\s*const\s+int64_t\s*\*\s*offsets\s*,\s*int64_t\s+n\s*,"
                     r"\s*int\s+mode\s*,\s*int\s+max_edge_clip\s*,\s*float\s+max_cov_gradient\s*,\s*rb_trim_rec\s*\*\s*out\s*\)", src)
    ps = re.search(r"typedef\s+struct\s+rb_trim_pass\s*\{([^}]*)\}\s*rb_trim_pass\s*;", src)
    rec = re.search(r"typedef\s+struct\s+rb_trim_rec\s*\{([^}]*)\}\s*rb_trim_rec\s*;", src)
    assert ps and rec
    ints = lambda body: sum(int(m.group(1) or 1) for decl in re.findall(r"int32_t\s+([^;]*);", body) for m in re.finditer(r"\w+(?:\s*\[\s*(\d+)\s*\])?\s*(?:,|$)", decl.strip()))
    assert ints(ps.group(1)) == 5
    assert ints(rec.group(1)) + 2 * ints(ps.group(1)) == 16 and re.search(r"rb_trim_pass\s+pass\s*\[\s*2\s*\]", rec.group(1))
    for name, val in (("RB_TRIM_HASHES", 0), ("RB_TRIM_EDGE", 1), ("RB_TRIM_LONG", 2), ("RB_TRIM_FOUND", 1), ("RB_TRIM_TRIMMED", 2), ("RB_TRIM_NOT_JUDGED", 32)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, val), src), name


def test_the_python_layer_binds_the_entry_point():
    from rnabloom import _native as N
    from rnabloom import graphutils
    from rnabloom.graph import BloomFilterDeBruijnGraph as G
    assert "rb_graph_trim_rc_artifacts" in {s[0] for s in N.SYMBOLS} and hasattr(N.lib, "rb_graph_trim_rc_artifacts")
    assert G.TRIM_DTYPE.itemsize == 64 and (N.TRIM_HASHES, N.TRIM_EDGE, N.TRIM_LONG) == (HASHES, EDGE, LONG)
    assert callable(G.trimArtifactsFlat) and callable(G.trimArtifacts) and callable(graphutils.trimReverseComplementArtifact)
