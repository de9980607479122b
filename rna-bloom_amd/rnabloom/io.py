"""Input formats of the reference at the C-ABI boundary: FASTQ text -> sequence / quality buffers
(rnabloom.io.FastqReader: R/io/FastqReader.java:140-186, gzip through R/util/FileUtils.java:50-57) and .nbits 2-bit
sequence files (R/io/NucleotideBitsReader.java / NucleotideBitsWriter.java).  Record splitting is the library's threaded
splitter; 2-bit encoding, quality segmentation and the .nbits bit permutation run on the GPU."""
import ctypes as C

import numpy as np

from . import _native as N
from ._native import check, lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def splitFastq(text, threads=0, with_qual=True):
    """FASTQ text (bytes / uint8 array) -> (seq uint8[], qual uint8[] or None, offsets int64[n+1])"""
    t = np.frombuffer(text, np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, np.uint8)
    n = C.c_int64()
    check(lib.rb_fastq_split(_ptr(t), t.size, threads, None, None, None, 0, C.byref(n)))
    off = np.zeros(n.value + 1, np.int64)
    seq = np.zeros(max(1, t.size), np.uint8)
    qual = np.zeros(max(1, t.size), np.uint8) if with_qual else None
    check(lib.rb_fastq_split(_ptr(t), t.size, threads, _ptr(seq), _ptr(qual), _ptr(off), n.value, C.byref(n)))
    tot = int(off[-1])
    return seq[:tot], (qual[:tot] if with_qual else None), off


def gunzip(data, threads=0):
    """every member of a gzip byte string (GZIPInputStream semantics) -> uint8 array; BGZF members are inflated in parallel"""
    a = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
    n = C.c_size_t()
    check(lib.rb_gunzip(_ptr(a), a.size, threads, None, 0, C.byref(n)))
    out = np.empty(max(1, n.value), np.uint8)
    check(lib.rb_gunzip(_ptr(a), a.size, threads, _ptr(out), out.size, C.byref(n)))
    return out[:n.value]


def readText(path, threads=0):
    """FileUtils.getTextFileReader: the file's text as a uint8 array, inflated when the name ends in .gz (R/util/FileUtils.java:50-57)"""
    path = str(path)
    raw = np.fromfile(path, np.uint8)
    return gunzip(raw, threads) if path.lower().endswith(".gz") else raw


def readFastq(path, threads=0, with_qual=True):
    """getTextFileReader + FastqReader over a whole file (.gz by extension, as FileUtils.getTextFileReader decides)"""
    return splitFastq(readText(path, threads), threads, with_qual)


def batchFromFastq(text, device=0, minBaseQual=3, final=True, with_qual=True):
    """FASTQ text -> ReadBatch on the device, records found and encoded there; returns (batch, bytes consumed)"""
    from .graph import ReadBatch
    t = np.frombuffer(text, np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, np.uint8)
    h = C.c_void_p(); used = C.c_size_t()
    check(lib.rb_batch_create_fastq(device, _ptr(t), t.size, int(final), minBaseQual, int(with_qual), C.byref(h), C.byref(used)))
    return ReadBatch(h, device), used.value


def batchFromFasta(text, device=0, final=True):
    """FASTA text -> ReadBatch on the device (FastaReader.next semantics, records found there); returns (batch, bytes consumed, ended)"""
    from .graph import ReadBatch
    t = np.frombuffer(text, np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, np.uint8)
    h = C.c_void_p(); used = C.c_size_t(); ended = C.c_int32()
    check(lib.rb_batch_create_fasta(device, _ptr(t), t.size, int(final), C.byref(h), C.byref(used), C.byref(ended)))
    return ReadBatch(h, device), used.value, bool(ended.value)


# ---- the segment lists GraphUtils.connect takes (BloomFilterDeBruijnGraph.connectSegments, graphutils.connect) ----
import re

_PHRED33 = bytes(range(33, 127))                   # R/util/SeqUtils.java:1426


def _nucleotide_pattern(k):
    """SeqUtils.getNucleotideCharsPattern (R/util/SeqUtils.java:1436-1438)"""
    return re.compile(b"[ACGTU]{%d,}" % k, re.IGNORECASE)


def _phred33_pattern(minBaseQual, k):
    """SeqUtils.getPhred33Pattern (R/util/SeqUtils.java:1432-1434): runs of at least k quality letters of minBaseQual or more"""
    return re.compile(b"[" + re.escape(_PHRED33[minBaseQual:]) + b"]{%d,}" % k)


def _runs_and_gaps(seq, pattern, keep):
    """the loop both functions run (R/util/SeqUtils.java:1842-1862): every match of pattern in upper case through keep(), and in front of
    every match but the first what lies between it and the match before: one 'N' for one letter, else that many 'N' (GAP_CHAR)"""
    end = 0
    for m in pattern.finditer(seq):
        if end > 0:
            keep(b"N" * (m.start() - end))
        end = m.end()
        keep(seq[m.start():end].upper())


def filterFasta(seq, k):
    """SeqUtils.filterFasta(seq, getNucleotideCharsPattern(k)) (R/util/SeqUtils.java:1833-1865): the runs of at least k letters of ACGTU (either
    case, returned in upper case; U stays U) at the even indices, placeholders of N — as long as what was left out between two runs — at the odd
    ones.  What lies before the first run and behind the last one is dropped.  bytes in, a list of bytes out."""
    seq = seq.encode() if isinstance(seq, str) else bytes(seq)
    out = []
    _runs_and_gaps(seq, _nucleotide_pattern(k), out.append)
    return out


def filterFastq(seq, qual, k, minBaseQual):
    """SeqUtils.filterFastq(seq, qual, getNucleotideCharsPattern(k), getPhred33Pattern(minBaseQual, k)) (R/util/SeqUtils.java:1871-1934): the
    letters under the Phred-33 runs of at least k qualities >= minBaseQual are kept, what lies between two such runs becomes N, and the result
    is filtered as filterFasta filters.  An empty seq or qual gives an empty list.  seq and qual have the same length."""
    seq = seq.encode() if isinstance(seq, str) else bytes(seq)
    qual = qual.encode() if isinstance(qual, str) else bytes(qual)
    if not seq or not qual:
        return []
    kept = []
    end = 0
    for m in _phred33_pattern(minBaseQual, k).finditer(qual):                   # (the same loop, with the matches found in qual and cut out of seq)
        if end > 0:
            kept.append(b"N" * (m.start() - end))
        end = m.end()
        kept.append(seq[m.start():end].upper())
    return filterFasta(b"".join(kept), k)


def writeNbits(path, seq, offsets, append=False):
    """NucleotideBitsWriter: 4-byte big-endian length + 2-bit bases (first base in the top bits, value - 128) per sequence"""
    seq = np.ascontiguousarray(seq, np.uint8); off = np.ascontiguousarray(offsets, np.int64)
    need = C.c_size_t()
    check(lib.rb_nbits_encode(_ptr(seq), _ptr(off), off.size - 1, None, 0, C.byref(need)))
    out = np.zeros(max(1, need.value), np.uint8)
    check(lib.rb_nbits_encode(_ptr(seq), _ptr(off), off.size - 1, _ptr(out), out.size, C.byref(need)))
    with open(str(path), "ab" if append else "wb") as f:
        f.write(out[:need.value].tobytes())
    return need.value


def batchFromNbits(data, device=0, max_reads=-1):
    """NucleotideBitsReader over a byte string -> ReadBatch on the device (decoded there); returns (batch, bytes consumed)"""
    from .graph import ReadBatch
    a = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
    h = C.c_void_p(); used = C.c_size_t()
    check(lib.rb_batch_create_nbits(device, _ptr(a), a.size, max_reads, C.byref(h), C.byref(used)))
    return ReadBatch(h, device), used.value
