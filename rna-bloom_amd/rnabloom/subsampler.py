"""rnabloom.util.SeqSubsampler with the reference's arguments: strobemerBased (R/util/SeqSubsampler.java:339-481, the default of -lrsub) and
kmerBased (:120-337).  The accept / reject loop runs on the device (rb_subsample_reads): the reads are judged in the reference's visiting
order against one CountingBloomFilter that only the loop writes, and nothing but the reads goes up and a byte a read comes back.

What the reference leaves open is fixed here: one read's distinct hashes are incremented as if one after the other in order of first
occurrence (the reference runs them through parallelStream over a HashSet, :449-453, so any serial order is one of its executions), and the
draws of MiniFloat.increment come from the library's counter-based generator, as everywhere.

strobemerBasedComposed is the same loop over the calls the library had before — rb_strobemers and getCount per read, the scan on the host,
increment of the chosen hashes: two calls and two trips over the link per read.  It is the cross-check and the baseline of
tools/subsample_bench.py.

The sort by length stays with the caller, as in RNABloom.main (R/RNABloom.java:7364-7391): `seqs` is visited as it is given."""
import ctypes as C

import numpy as np

from . import _native as N
from .bloom import CountingBloomFilter
from .graph import _pack, _ptr, strobemers

PIECE_READS = 1 << 16      # reads a call of the library takes (the filter and the op ordinal carry from call to call)


def subsample_reads(cbf, params, reads, piece_reads=PIECE_READS, want_recs=False):
    """rb_subsample_reads over reads (list of bytes, or (seq, offsets) arrays) in array order, piece by piece, against cbf (a
    CountingBloomFilter or a graph).  Returns (keep uint8[n], recs int32[n, 8] or None, totals int64[4])."""
    seq, off = reads if isinstance(reads, tuple) else _pack(reads)
    off = np.ascontiguousarray(off, np.int64)
    n = off.size - 1
    g = getattr(cbf, "_g", cbf)
    keep = np.zeros(n, np.uint8)
    recs = np.zeros((n, len(N.SUB_REC_FIELDS)), np.int32) if want_recs else None
    totals, t = np.zeros(4, np.int64), np.zeros(4, np.int64)
    for a in range(0, n, max(1, int(piece_reads))):
        b = min(n, a + max(1, int(piece_reads)))
        N.check(N.lib.rb_subsample_reads(g.h, C.byref(params), _ptr(seq), off[a:].ctypes.data, b - a, keep[a:].ctypes.data,
                                         recs[a:].ctypes.data if want_recs else None, t.ctypes.data))
        totals += t
    return keep, recs, totals


def strobemer_params(k, maxMultiplicity, maxEdgeClip, maxIndelSize):
    """:360-363: n = 3, wMin = k + 1, wMax = k + max(k, maxIndelSize) (the library takes max(maxEdgeClip, wMax) itself)"""
    return N.SubsampleParams(N.SUB_STROBEMER, k, k + 1, k + max(k, maxIndelSize), 0, maxMultiplicity, maxEdgeClip, 0)


def visiting_order(numSeq, increment=3):
    """:371-373: indices shift, shift + 3, ... for shift = 0, 1, 2"""
    return [i for shift in range(increment) for i in range(shift, numSeq, increment)]


def strobemerBased(seqs, bfSize, k, numHash, stranded, maxMultiplicity, maxEdgeClip, maxIndelSize, device=0, rngSeed=0, piece_reads=PIECE_READS):
    """SeqSubsampler.strobemerBased: (indices of the kept reads in output order, the filter's FPR).  `stranded` is not used, as in the
    reference (:356-357, :366-367: the canonical iterator is commented out)."""
    cbf = CountingBloomFilter(bfSize, numHash, k, device=device, rngSeed=rngSeed)                  # :357-358
    try:
        order = visiting_order(len(seqs))
        keep, _, _ = subsample_reads(cbf, strobemer_params(k, maxMultiplicity, maxEdgeClip, maxIndelSize), [seqs[i] for i in order], piece_reads)
        return [i for i, kp in zip(order, keep) if kp], cbf.getFPR()                                 # :466
    finally:
        cbf.destroy()


def kmerBased(seqs, bfSize, k, numHash, stranded, maxMultiplicity, maxEdgeClip, device=0, rngSeed=0, piece_reads=PIECE_READS):
    """SeqSubsampler.kmerBased: (indices of the kept reads in output order, the filter's FPR).  A read whose range of pairs is negative makes
    the reference throw (new boolean[end - start]); here it raises ValueError with the read's index, after the loop."""
    cbf = CountingBloomFilter(bfSize, numHash, k, device=device, rngSeed=rngSeed)                  # :148, :231
    try:
        p = N.SubsampleParams(N.SUB_KMER, k, 0, 0, 0 if stranded else 1, maxMultiplicity, maxEdgeClip, 0)
        keep, recs, totals = subsample_reads(cbf, p, list(seqs), piece_reads, want_recs=True)
        if totals[2]:
            raise ValueError("kmerBased: read %d has a negative range of k-mer pairs (NegativeArraySizeException in the reference)"
                             % int(np.flatnonzero(recs[:, 0] == N.SUB_NOT_JUDGED)[0]))
        return [int(i) for i in np.flatnonzero(keep)], cbf.getFPR()                                  # :323
    finally:
        cbf.destroy()


def strobemer_scan(seen, ends, seqLen, maxEdgeClip):
    """:394-434 statement by statement over seen[i] and the strobemers' ends (start_i = i): (write, line, index, nam or None)"""
    nam, write, line, index = None, False, N.SUB_LINE_TAIL, -1
    for i in range(len(seen)):
        if seen[i]:
            pos1, pos2 = i, int(ends[i])
            if nam is None:
                if pos1 > maxEdgeClip:
                    write, line, index = True, N.SUB_LINE_SEEN_BEYOND_EDGE, i
                    break
                nam = [pos1, pos2]
            elif max(0, min(nam[1], pos2) - max(nam[0], pos1)) > 0:                                 # ComparableInterval.merge
                nam = [min(nam[0], pos1), max(nam[1], pos2)]
            else:
                write, line, index = True, N.SUB_LINE_MERGE_FAILED, i
                break
        elif nam is None:
            if i > maxEdgeClip:
                write, line, index = True, N.SUB_LINE_UNSEEN_BEYOND_EDGE, i
                break
        elif i > nam[1]:
            write, line, index = True, N.SUB_LINE_GAP, i
            break
    if not write and (nam is None or nam[0] > maxEdgeClip or nam[1] < seqLen - maxEdgeClip - 1):
        write = True
    return write, line, index, nam


def strobemerBasedComposed(seqs, bfSize, k, numHash, stranded, maxMultiplicity, maxEdgeClip, maxIndelSize, device=0, rngSeed=0, want_filter=False):
    """The same loop over the per-read calls: rb_strobemers, getCount, the scan on the host, increment.  Returns what strobemerBased returns
    (and the filter's bytes and op ordinal with want_filter)."""
    cbf = CountingBloomFilter(bfSize, numHash, k, device=device, rngSeed=rngSeed)
    try:
        wMin, wMax = k + 1, k + max(k, maxIndelSize)
        maxEdgeClip = max(maxEdgeClip, wMax)
        kept = []
        for index in visiting_order(len(seqs)):
            seq = seqs[index]
            _, h, _, e = strobemers([seq], k, 3, wMin, wMax, device=device)
            if h.size == 0:                                                                          # start() failed: too short, kept (:456-460)
                kept.append(index)
                continue
            seen = cbf.getCount(h) >= maxMultiplicity
            if strobemer_scan(seen, e, len(seq), maxEdgeClip)[0]:
                kept.append(index)
                hv = h[~seen]
                _, first = np.unique(hv, return_index=True)                                          # the HashSet, in order of first occurrence
                if first.size:
                    cbf.increment(hv[np.sort(first)])
        out = (kept, cbf.getFPR())
        return out + (cbf.toBytes(), cbf._g.getOpOrdinal()) if want_filter else out
    finally:
        cbf.destroy()
