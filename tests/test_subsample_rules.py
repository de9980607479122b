"""SeqSubsampler.strobemerBased (R/util/SeqSubsampler.java:339-481) and kmerBased (:120-337) restated statement by statement over the oracle's
counting filter, with hand-worked cases: what rb_subsample_reads has to compute (tests/test_gpu_subsample.py compares every record int, the
filter's bytes and the op ordinal).

The filter is an rbo.Graph of which only the counting filter is used: cbf.getCount(hash) is rbo_cbf_get_count on the graph's counting filter
(rbo.Graph.get_count is BloomFilterDeBruijnGraph.getCount, which asks dbgbf first — a filter the subsampler does not have), cbf.increment(hash) is
rbo.Graph.add_count_only, which draws rng31(seed, ordinal, 0) and moves the ordinal on.  The order of one read's increments, which the reference
leaves to parallelStream over a HashSet (:449-453), is the order of first occurrence: strobemers by i; pairs in the gap-1 list, then gap-2, then
gap-0 (:204-217).  Any serial order is an execution the reference may take.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import rbo
from oracle import rbo_py
from rnabloom import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = N.SUB_REC_FIELDS
F = {name: i for i, name in enumerate(FIELDS)}
DROPPED, KEPT_SCAN, KEPT_TAIL, KEPT_START_FAILED, NOT_JUDGED = range(5)
M64 = (1 << 64) - 1


class Filter:
    """the CountingBloomFilter of the loop: new CountingBloomFilter(bfSize, numHash, new HashFunction(k)) (:148, :231, :358)"""

    def __init__(self, size, num_hash, k, seed=0):
        self.size, self.H, self.k = int(size), int(num_hash), int(k)
        self.og = rbo.Graph(64, self.size, 0, 1, self.H, 1, k, True, False, seed)
        L = self.og.L
        self.cbf = C.c_void_p(L.rbo_graph_cbf(self.og.g))
        n = C.c_int64()
        p = L.rbo_cbf_bytes(self.cbf, C.byref(n))
        self.live = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (n.value,))      # the counters themselves, not a copy
        self.to_float = np.array([L.rbo_minifloat_to_float(b) for b in range(128)], np.float32)                  # MiniFloat.toFloat
        self.mult = [np.uint64((i ^ ((k * rbo_py.MULTI_SEED) & M64)) & M64) for i in range(self.H)]

    def get_count(self, h):                                       # CountingBloomFilter.getCount(long) :235-251
        return float(self.og.L.rbo_cbf_get_count(self.cbf, rbo._p(rbo.ntm64(int(h), self.k, self.H))))

    def increment(self, h):                                       # CountingBloomFilter.increment(long) :170-194
        self.og.add_count_only(rbo.ntm64(int(h), self.k, self.H))

    def counter_indices(self, h):
        """[len(h), numHash] counter indices: NTM64 (NTHash.java:518-527) and getIndex, over an array"""
        h = np.asarray(h, np.uint64)
        cols = [h]
        with np.errstate(over="ignore"):
            for i in range(1, self.H):
                t = h * self.mult[i]
                cols.append(t ^ (t >> np.uint64(rbo_py.MULTI_SHIFT)))
        return np.stack([(c >> np.uint64(1)) % np.uint64(self.size) for c in cols], axis=1).astype(np.int64)

    def get_counts(self, h):
        """get_count of every hash of an array at once (test_get_counts_is_get_count_of_each)"""
        h = np.asarray(h, np.uint64)
        if h.size == 0:
            return np.zeros(0, np.float32)
        mn = self.live[self.counter_indices(h)].min(axis=1)
        return self.to_float[mn]

    def ordinal(self):
        return int(self.og.L.rbo_graph_ordinal(self.og.g))

    def bytes(self):
        return self.og.cbf_bytes()


# ---- strobemer mode ----
def get_overlap(start1, end1, start2, end2):                      # IntervalUtils.getOverlap :53-55
    return max(0, min(end1, end2) - max(start1, start2))


def fold(seen, starts, ends, seq_len, max_edge_clip):
    """:394-434.  Returns (write, status, line, deciding index, nam or None)"""
    nam = None
    write, line, index = False, N.SUB_LINE_TAIL, -1
    for i in range(len(seen)):
        if seen[i]:
            pos1, pos2 = int(starts[i]), int(ends[i])
            if nam is None:
                if pos1 > max_edge_clip:
                    write, line, index = True, N.SUB_LINE_SEEN_BEYOND_EDGE, i
                    break
                nam = [pos1, pos2]
            else:
                overlap = get_overlap(nam[0], nam[1], pos1, pos2)                            # ComparableInterval.merge :23-32
                if overlap > 0:
                    nam = [min(nam[0], pos1), max(nam[1], pos2)]
                else:
                    write, line, index = True, N.SUB_LINE_MERGE_FAILED, i
                    break
        elif nam is None:
            if starts[i] > max_edge_clip:
                write, line, index = True, N.SUB_LINE_UNSEEN_BEYOND_EDGE, i
                break
        else:
            if starts[i] > nam[1]:
                write, line, index = True, N.SUB_LINE_GAP, i
                break
    status = KEPT_SCAN if write else DROPPED
    if not write and (nam is None or nam[0] > max_edge_clip or nam[1] < seq_len - max_edge_clip - 1):
        write, status = True, KEPT_TAIL
    return write, status, line, index, nam


def fold_as_scans(seen, ends, seq_len, max_edge_clip):
    """the same with start_i = i, as a prefix maximum and a first index: what the walker computes"""
    n = len(seen)
    first = next((i for i in range(n) if seen[i]), None)
    b0 = max_edge_clip + 1
    if b0 < n and (first is None or b0 <= first):
        return True, KEPT_SCAN, (N.SUB_LINE_SEEN_BEYOND_EDGE if b0 == first else N.SUB_LINE_UNSEEN_BEYOND_EDGE), b0, None
    if first is None:
        return True, KEPT_TAIL, N.SUB_LINE_TAIL, -1, None
    before = np.maximum.accumulate(np.where(seen, ends, -(1 << 30)))                          # inclusive; before[i - 1] is namInterval.end at i
    for i in range(first + 1, n):
        e = int(before[i - 1])
        if (min(e, int(ends[i])) <= i) if seen[i] else (i > e):
            return True, KEPT_SCAN, (N.SUB_LINE_MERGE_FAILED if seen[i] else N.SUB_LINE_GAP), i, [first, e]
    nam = [first, int(before[n - 1])]
    keep = nam[0] > max_edge_clip or nam[1] < seq_len - max_edge_clip - 1
    return keep, (KEPT_TAIL if keep else DROPPED), N.SUB_LINE_TAIL, -1, nam


def distinct_in_order(hashes):
    seen_set, out = set(), []
    for h in hashes:
        if int(h) not in seen_set:
            seen_set.add(int(h)); out.append(int(h))
    return out


def strobemer_read(cbf, seq, k, max_multiplicity, max_edge_clip, max_indel_size):
    """one pass of the loop body :374-460: (write, record)"""
    w_min, w_max = k + 1, k + max(k, max_indel_size)                                          # :361-362
    max_edge_clip = max(max_edge_clip, w_max)                                                 # :363
    h, s, e = rbo.strobemers(seq, k, 3, w_min, w_max)
    if len(h) == 0:                                                                           # strobeItr.start(seq) failed (:456-460)
        return True, [KEPT_START_FAILED, N.SUB_LINE_START_FAILED, -1, -1, -1, 0, 0, 0]
    seen = cbf.get_counts(h) >= max_multiplicity                                              # :389
    write, status, line, index, nam = fold(seen, s, e, len(seq), max_edge_clip)
    distinct = 0
    if write:
        todo = distinct_in_order(h[~seen])                                                    # :441-446
        for hv in todo:
            cbf.increment(hv)                                                                 # :449-453
        distinct = len(todo)
    return write, [status, line, index] + (nam if nam else [-1, -1]) + [len(h), int((~seen).sum()), distinct]


def strobemer_based(cbf, reads, k, max_multiplicity, max_edge_clip, max_indel_size):
    """the reads in the order given (the caller permutes, :371-373): (keep, records)"""
    out = [strobemer_read(cbf, r, k, max_multiplicity, max_edge_clip, max_indel_size) for r in reads]
    return np.array([w for w, _ in out], np.uint8), np.array([r for _, r in out], np.int32).reshape(len(reads), 8)


# ---- k-mer mode ----
def kmer_read(cbf, seq, k, canonical, max_multiplicity, max_edge_clip):
    """one pass of the loop body :150-226 (stranded) / :233-318 (canonical)"""
    line = (lambda a, b: b if canonical else a)
    shift, shift_d, shift_i = k + 1, k, k + 2                                                 # :129-131
    missing_chain_threshold = k + shift                                                       # :132
    if len(seq) < k:                                                                          # hashItr.start(seq) (NTHashIterator.java:47-54)
        return False, [DROPPED, line(N.SUB_LINE_KMER_START_FAILED, N.SUB_LINE_KMER_START_FAILED_C), -1, -1, -1, 0, 0, 0]
    seq_len = len(seq)
    too_short = seq_len < 3 * max_edge_clip
    num_kmers = seq_len - k + 1
    if too_short:
        start, end = 0, num_kmers - shift
    else:
        start, end = max_edge_clip, num_kmers - max_edge_clip - shift
    if end - start < 0:                                                                       # new boolean[end - start] throws
        return False, [NOT_JUDGED, line(N.SUB_LINE_KMER_RANGE, N.SUB_LINE_KMER_RANGE_C), -1, start, -1, 0, 0, 0]
    pairs = {s: rbo.kmer_pair_hashes(seq, k, s, canonical) for s in (shift, shift_d, shift_i)}
    seen = cbf.get_counts(pairs[shift][start:end]) >= max_multiplicity
    missing_chain_len, write, index = 0, False, -1
    for j, s in enumerate(seen):
        if s:
            missing_chain_len = 0
        else:
            missing_chain_len += 1
            if missing_chain_len >= missing_chain_threshold:
                write, index = True, start + j
                break
    distinct = 0
    if write:
        todo = distinct_in_order(list(pairs[shift][start:end]) + list(pairs[shift_i][start:end - 1]) + list(pairs[shift_d][start:end + 1]))
        for hv in todo:
            cbf.increment(hv)
        distinct = len(todo)
    return write, [KEPT_SCAN if write else DROPPED,
                   line(N.SUB_LINE_KMER_CHAIN, N.SUB_LINE_KMER_CHAIN_C) if write else line(N.SUB_LINE_KMER_NO_CHAIN, N.SUB_LINE_KMER_NO_CHAIN_C),
                   index, start, missing_chain_len, end - start, int((~seen).sum()), distinct]


def kmer_based(cbf, reads, k, canonical, max_multiplicity, max_edge_clip):
    out = [kmer_read(cbf, r, k, canonical, max_multiplicity, max_edge_clip) for r in reads]
    return np.array([w for w, _ in out], np.uint8), np.array([r for _, r in out], np.int32).reshape(len(reads), 8)


def chain_as_scan(seen, threshold):
    """the k-mer scan as a prefix maximum of `seen ? i : -1`: (first index where the chain reaches the threshold or None, chain length at the end)"""
    n = len(seen)
    if n == 0:
        return None, 0
    last = np.maximum.accumulate(np.where(seen, np.arange(n), -1))
    hit = np.flatnonzero(~np.asarray(seen, bool) & (np.arange(n) - last >= threshold))
    return (int(hit[0]), threshold) if hit.size else (None, int(n - 1 - last[-1]))


# ================================================================== tests
def rnd(seed, n):
    return bytes(np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", np.uint8), n))


def test_get_counts_is_get_count_of_each():
    cbf = Filter(257, 3, 11, seed=4)
    hs = np.random.default_rng(1).integers(0, 1 << 63, 400, dtype=np.uint64)
    for h in hs[:300]:
        cbf.increment(h)
    assert cbf.get_counts(hs).tolist() == [cbf.get_count(h) for h in hs]
    assert cbf.get_counts(hs).max() >= 3 and cbf.get_counts(hs).min() == 0


def test_the_fold_where_a_start_meets_the_interval_end():
    """write is not monotone in seen: with start_i == namInterval.end a SEEN strobemer fails the merge (overlap 0) and the read is written,
    an UNSEEN one is no gap (start_i > end is false) and the scan goes on"""
    ends = np.array([5, 6, 7, 8, 9, 12, 13, 14, 15, 16], np.int32)
    starts = np.arange(10)
    seen = np.array([1, 0, 0, 0, 0, 1, 1, 1, 1, 1], bool)          # namInterval = (0, 5); element 5 starts at its end
    assert fold(seen, starts, ends, 17, 0) == (True, KEPT_SCAN, N.SUB_LINE_MERGE_FAILED, 5, [0, 5])
    seen[5] = False                                                 # more unseen, and the read is NOT written at 5: 6 is seen and merges? no: 6 > 5
    assert fold(seen, starts, ends, 17, 0) == (True, KEPT_SCAN, N.SUB_LINE_MERGE_FAILED, 6, [0, 5])
    ends[0] = 6                                                     # namInterval = (0, 6): 5 unseen passes, 6 seen starts at the end: overlap 0
    assert fold(seen, starts, ends, 17, 0) == (True, KEPT_SCAN, N.SUB_LINE_MERGE_FAILED, 6, [0, 6])
    seen[6] = False                                                 # 6 unseen: 6 > 6 is false, no gap; 7 is seen, min(6, 14) - 7 < 0
    assert fold(seen, starts, ends, 17, 0) == (True, KEPT_SCAN, N.SUB_LINE_MERGE_FAILED, 7, [0, 6])
    seen[:] = [1, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    ends[0] = 9                                                     # nine unseen strobemers, none beyond the interval's end: no break;
    assert fold(seen, starts, ends, 10, 0) == (False, DROPPED, N.SUB_LINE_TAIL, -1, [0, 9])      # 9 < 10 - 0 - 1 is false: dropped
    assert fold(seen, starts, ends, 11, 0) == (True, KEPT_TAIL, N.SUB_LINE_TAIL, -1, [0, 9])     # one letter more and the tail test keeps it
    ends[0] = 8
    assert fold(seen, starts, ends, 10, 0) == (True, KEPT_SCAN, N.SUB_LINE_GAP, 9, [0, 8])


def test_the_fold_at_the_left_edge():
    ends = np.arange(10) + 4
    starts = np.arange(10)
    none = np.zeros(10, bool)
    assert fold(none, starts, ends, 14, 3) == (True, KEPT_SCAN, N.SUB_LINE_UNSEEN_BEYOND_EDGE, 4, None)
    assert fold(none, starts, ends, 14, 9) == (True, KEPT_TAIL, N.SUB_LINE_TAIL, -1, None)        # namInterval == null
    seen = none.copy(); seen[4] = True
    assert fold(seen, starts, ends, 14, 3) == (True, KEPT_SCAN, N.SUB_LINE_SEEN_BEYOND_EDGE, 4, None)
    seen[:] = True
    assert fold(seen, starts, ends, 14, 3) == (False, DROPPED, N.SUB_LINE_TAIL, -1, [0, 13])      # 13 < 14 - 3 - 1 is false
    assert fold(seen, starts, ends, 18, 3) == (True, KEPT_TAIL, N.SUB_LINE_TAIL, -1, [0, 13])     # 13 < 14


def test_the_scans_are_the_fold():
    from rnabloom import subsampler
    rng = np.random.default_rng(7)
    lines = set()
    for trial in range(4000):
        n = int(rng.integers(1, 40))
        ends = (np.arange(n) + rng.integers(1, 12, n)).astype(np.int32)
        seen = rng.random(n) < rng.choice([0.05, 0.3, 0.7, 0.95])
        clip, seq_len = int(rng.integers(0, 8)), n + int(rng.integers(0, 20))
        want = fold(seen, np.arange(n), ends, seq_len, clip)
        assert fold_as_scans(seen, ends, seq_len, clip) == want, (seen, ends, seq_len, clip)
        w, line, index, nam = subsampler.strobemer_scan(seen, ends, seq_len, clip)
        assert (w, line, index, nam) == (want[0], want[2], want[3], want[4])
        lines.add((want[1], want[2]))
        thr = int(rng.integers(1, 6))
        chain, write, index = 0, False, None
        for j in range(n):
            chain = 0 if seen[j] else chain + 1
            if chain >= thr:
                write, index = True, j
                break
        assert chain_as_scan(seen, thr) == (index, chain)
    assert len(lines) == 6                                          # the four breaks and the tail test both ways


def test_strobemer_reads_by_hand():
    k, indel = 11, 50                                               # wMin 12, wMax 61: start() needs more than 122 k-mers
    cbf = Filter(1_000_003, 2, k, seed=3)
    a = rnd(1, 400)
    w, rec = strobemer_read(cbf, a[:132], k, 1, 0, indel)           # 122 k-mers: start() fails, kept, nothing counted
    assert (w, rec) == (True, [KEPT_START_FAILED, N.SUB_LINE_START_FAILED, -1, -1, -1, 0, 0, 0]) and cbf.ordinal() == 0
    w, rec = strobemer_read(cbf, a[:133], k, 1, 0, indel)           # 123 k-mers: 123 - 61 - 12 = 50 strobemers, none seen, none beyond the edge (61)
    assert (w, rec) == (True, [KEPT_TAIL, N.SUB_LINE_TAIL, -1, -1, -1, 50, 50, 50]) and cbf.ordinal() == 50
    w, rec = strobemer_read(cbf, a[:133], k, 1, 0, indel)           # again: all seen; namInterval = (0, 132 at most) and 133 - 61 - 1 = 71
    assert not w and rec[:4] == [DROPPED, N.SUB_LINE_TAIL, -1, 0] and rec[4] >= 71 and rec[5:] == [50, 0, 0] and cbf.ordinal() == 50
    w, rec = strobemer_read(cbf, a, k, 1, 0, indel)                 # the whole transcript: unseen from some strobemer on, beyond the interval's end
    assert w and rec[0] == KEPT_SCAN and rec[1] == N.SUB_LINE_GAP and rec[F["elements"]] == 400 - 10 - 73 and rec[F["incremented"]] == rec[F["unseen"]]
    w, rec = strobemer_read(cbf, a, k, 2, 0, indel)                 # depth 2: nothing is seen twice but the first 133 letters' strobemers
    assert w and rec[F["unseen"]] >= 317 - 50
    b = rnd(2, 70) + a[100:]                                        # 70 new letters in front: the first seen strobemer lies beyond the edge region
    w, rec = strobemer_read(cbf, b, k, 1, 0, indel)
    assert w and rec[:3] == [KEPT_SCAN, N.SUB_LINE_UNSEEN_BEYOND_EDGE, 62] and rec[3:5] == [-1, -1]


def test_duplicate_hashes_are_counted_once():
    k = 11
    cbf = Filter(1_000_003, 2, k, seed=3)
    homo = b"A" * 300
    h, _, _ = rbo.strobemers(homo, k, 3, 12, 61)
    assert len(h) == 217 and len(set(h.tolist())) == 1
    w, rec = strobemer_read(cbf, homo, k, 1, 0, 50)
    assert w and rec[F["unseen"]] == 217 and rec[F["incremented"]] == 1 and cbf.ordinal() == 1
    assert cbf.get_count(h[0]) == 1.0
    cbf2 = Filter(1_000_003, 2, k, seed=3)
    w, rec = kmer_read(cbf2, homo, k, False, 1, 0)
    assert w and rec[:3] == [KEPT_SCAN, N.SUB_LINE_KMER_CHAIN, 22] and rec[F["incremented"]] == 1      # 3 lists, one hash


def test_kmer_reads_by_hand():
    k = 11
    cbf = Filter(1_000_003, 2, k, seed=9)
    a = rnd(5, 300)
    assert kmer_read(cbf, a[:10], k, False, 1, 0) == (False, [DROPPED, N.SUB_LINE_KMER_START_FAILED, -1, -1, -1, 0, 0, 0])
    assert kmer_read(cbf, a[:10], k, True, 1, 0) == (False, [DROPPED, N.SUB_LINE_KMER_START_FAILED_C, -1, -1, -1, 0, 0, 0])
    # 21 letters: 11 k-mers, end = 11 - 12 = -1 < start = 0 — new boolean[-1]
    assert kmer_read(cbf, a[:21], k, False, 1, 0) == (False, [NOT_JUDGED, N.SUB_LINE_KMER_RANGE, -1, 0, -1, 0, 0, 0])
    # 100 letters, maxEdgeClip 30: not tooShort (100 >= 90), start = 30, end = 90 - 30 - 12 = 48: 18 pairs, fewer than the chain of 23: dropped
    assert kmer_read(cbf, a[:100], k, True, 1, 30) == (False, [DROPPED, N.SUB_LINE_KMER_NO_CHAIN_C, -1, 30, 18, 18, 18, 0])
    # maxEdgeClip 40: tooShort (100 < 120), start = 0, end = 78; the 23rd unseen pair decides
    w, rec = kmer_read(cbf, a[:100], k, False, 1, 40)
    assert w and rec == [KEPT_SCAN, N.SUB_LINE_KMER_CHAIN, 22, 0, 23, 78, 78, 78 + 77 + 79] and cbf.ordinal() == 234
    w, rec = kmer_read(cbf, a[:100], k, False, 1, 40)
    assert not w and rec == [DROPPED, N.SUB_LINE_KMER_NO_CHAIN, -1, 0, 0, 78, 0, 0]
    # maxEdgeClip 45, 100 letters: not tooShort would need 135; tooShort.  110 letters with clip 36: 110 >= 108, start 36, end = 100 - 36 - 12 = 52
    w, rec = kmer_read(cbf, a[:110], k, False, 1, 36)
    assert not w and rec[:6] == [DROPPED, N.SUB_LINE_KMER_NO_CHAIN, -1, 36, 0, 16]
    # 60 letters with clip 20: not tooShort, start 20, end = 50 - 20 - 12 = 18 < 20
    assert kmer_read(cbf, a[:60], k, False, 1, 20)[1][:4] == [NOT_JUDGED, N.SUB_LINE_KMER_RANGE, -1, 20]


def test_the_feature_exists_at_every_layer():
    header = open(os.path.join(ROOT, "include", "rb_capi.h")).read()
    assert re.search(r"\bint rb_subsample_reads\(rb_graph \*cbf, const rb_subsample_params \*p,", header)
    assert "typedef struct rb_subsample_params" in header
    sym = {s[0]: s for s in N.SYMBOLS}
    assert "rb_subsample_reads" in sym and len(sym["rb_subsample_reads"][2]) == 8
    assert len(N.SUB_REC_FIELDS) == 8 and C.sizeof(N.SubsampleParams) == 32
    from rnabloom import subsampler
    for name in ("strobemerBased", "kmerBased", "strobemerBasedComposed", "subsample_reads"):
        assert callable(getattr(subsampler, name))
    java = open(os.path.join(ROOT, "java", "rnabloom", "graph", "NativeGraph.java")).read()
    assert re.search(r"public static native void subsampleReads\(long h, int\[\] params,", java)
    jni = open(os.path.join(ROOT, "jni", "rb_jni.c")).read()
    assert re.search(r"FN\(subsampleReads\)", jni) and "rb_subsample_reads(G(h)" in jni
    for doc, what in (("README.md", "rb_subsample_reads"), ("DESIGN.md", "Subsampling of long reads"), ("INTEGRATION.md", "subsampleReads")):
        assert what in open(os.path.join(ROOT, doc)).read(), doc
    assert os.path.exists(os.path.join(ROOT, "rna-bloom_amd", "csrc", "rb_subsample.hip"))
    # the header's constants are the binding's
    for name in ("STROBEMER", "KMER", "DROPPED", "KEPT_SCAN", "KEPT_TAIL", "KEPT_START_FAILED", "NOT_JUDGED", "LINE_SEEN_BEYOND_EDGE", "LINE_MERGE_FAILED",
                 "LINE_UNSEEN_BEYOND_EDGE", "LINE_GAP", "LINE_TAIL", "LINE_START_FAILED", "LINE_KMER_START_FAILED", "LINE_KMER_RANGE", "LINE_KMER_CHAIN",
                 "LINE_KMER_NO_CHAIN", "LINE_KMER_START_FAILED_C", "LINE_KMER_RANGE_C", "LINE_KMER_CHAIN_C", "LINE_KMER_NO_CHAIN_C"):
        m = re.search(r"\bRB_SUB_%s = (\d+)" % name, header)
        assert m and int(m.group(1)) == getattr(N, "SUB_" + name), name
    assert int(re.search(r"#define RB_SUB_LDS_ELEMS (\d+)", header).group(1)) == N.SUB_LDS_ELEMS
