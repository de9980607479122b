"""Seeded worlds for rb_subsample_reads: about 300 reads of 5 to 3 000 letters drawn with overlaps from a small set of transcripts, so that later
reads are mostly redundant, and the reads that sit on the walker's edges:
  * 2 * wMax + k - 1 and 2 * wMax + k letters (StrobeHashIterator.start fails / just passes), fewer than k letters and fewer than 2k (k-mer mode:
    start() fails / the range of pairs is negative);
  * element counts of 63 / 64 / 65, 255 / 256 / 257 and 1 023 / 1 024 / 1 025 (a wavefront, the two workgroup sizes of the walker), in either mode;
  * an early read of 3 000 new letters: more elements than the set in LDS holds (RB_SUB_LDS_ELEMS);
  * a homopolymer and a tandem repeat (duplicate hashes), exact duplicates of earlier reads;
  * reads that join two transcripts seen before (the first strobemer behind the junction starts where namInterval ends, or a gap comes first) and reads with 62 / 100 new
    letters in front of seen ones (the first seen strobemer at / beyond the left edge region).
want(i) runs the restatement of tests/test_subsample_rules.py once per world and keeps what it gives."""
import functools

import numpy as np

from oracle import rbo
from test_subsample_rules import Filter, fold, kmer_based, strobemer_based

K, INDEL = 11, 50
W_MIN, W_MAX = K + 1, K + max(K, INDEL)
SMALL, REAL = 257, 2_000_003

# mode, canonical (k-mer mode), numHash, maxMultiplicity, maxEdgeClip, filter size, transcripts, seed
WORLDS = [
    dict(mode="strobemer", canonical=False, H=2, M=1, clip=0, size=REAL, n_tx=8, seed=11),
    dict(mode="strobemer", canonical=False, H=1, M=3, clip=0, size=SMALL, n_tx=8, seed=12),
    dict(mode="strobemer", canonical=False, H=3, M=3, clip=0, size=SMALL, n_tx=8, seed=13),
    dict(mode="strobemer", canonical=False, H=4, M=3, clip=100, size=REAL, n_tx=3, seed=14),
    dict(mode="kmer", canonical=False, H=2, M=1, clip=30, size=REAL, n_tx=8, seed=15),
    dict(mode="kmer", canonical=True, H=3, M=3, clip=0, size=REAL, n_tx=3, seed=16),
    dict(mode="kmer", canonical=True, H=1, M=20, clip=20, size=SMALL, n_tx=8, seed=17),
    dict(mode="kmer", canonical=False, H=4, M=20, clip=0, size=REAL, n_tx=1, seed=18),
]


def world_id(w):
    return "%s%s-h%d-m%d-clip%d-%s" % (w["mode"], "-canonical" if w["canonical"] else "", w["H"], w["M"], w["clip"], "small" if w["size"] == SMALL else "real")


def rand(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))


def length_for(w, elements):
    """the read length that gives this many strobemers / judged pairs"""
    if w["mode"] == "strobemer":
        return elements + W_MAX + W_MIN + K - 1                    # numKmers - wMax - wMin strobemers
    n = elements + 2 * K                                           # tooShort: end - start = numKmers - (k + 1)
    return n if n < 3 * w["clip"] else n + 2 * w["clip"]


def junction_reads(x, y, count):
    """x[:p] + the start of y — two transcripts seen before, joined — for the first `count` places p where, if exactly the strobemers of x and y
    count as seen, the first strobemer of y starts where namInterval ends and fails the merge (R/util/SeqSubsampler.java:408), and for as many
    places where a gap breaks first (:421)"""
    known = set(rbo.strobemers(x, K, 3, W_MIN, W_MAX)[0].tolist()) | set(rbo.strobemers(y, K, 3, W_MIN, W_MAX)[0].tolist())
    fails, others = [], []
    for p in range(150, len(x)):
        r = x[:p] + y[:260]
        h, s, e = rbo.strobemers(r, K, 3, W_MIN, W_MAX)
        which = fails if fold(np.array([v in known for v in h.tolist()]), s, e, len(r), W_MAX)[2] == 408 else others
        if len(which) < count:
            which.append(r)
        if len(fails) == count and len(others) == count:
            break
    return fails + others


@functools.lru_cache(maxsize=None)
def reads_of(i):
    w = WORLDS[i]
    rng = np.random.default_rng(w["seed"])
    tx = [rand(rng, int(rng.integers(500, 1500))) for _ in range(w["n_tx"])]
    joined = rand(rng, 400)                                        # seen whole, early; later its start follows pieces of t0
    t0 = tx[0]
    # a filter of 257 counters is full after one long read: there a dozen shorter reads come first
    reads = [tx[1][:133], tx[2][:140], tx[0][:500]] + [tx[j % len(tx)][j:j + 133 + 5 * j] for j in range(9)] if w["size"] == SMALL else []
    reads += [rand(rng, 3000), t0, joined]
    for n in range(230):
        t = tx[min(int(rng.geometric(0.35)) - 1, len(tx) - 1)]
        ln = int(min(len(t), rng.choice([60, 150, 300, 450, 700, 900]) + rng.integers(0, 60)))
        a = int(rng.integers(0, len(t) - ln + 1))
        r = bytearray(t[a:a + ln])
        if rng.random() < 0.3:                                      # a few substitutions
            for p in rng.integers(0, ln, max(1, ln // 100)):
                r[p] = b"ACGT"[(b"ACGT".index(r[p]) + 1) % 4]
        reads.append(bytes(r))
    special = [t0[:2 * W_MAX + K - 1], t0[:2 * W_MAX + K], t0[:5], t0[:15], b"A" * 300, b"ACGTTGCA" * 50, 
               rand(rng, 61) + bytes([b"ACGT"[(b"ACGT".index(t0[99]) + 1) % 4]]) + t0[100:420], rand(rng, 100) + t0[100:420]]
    special += [rand(rng, length_for(w, e)) for e in (63, 64, 65, 255, 256, 257)]
    special += [tx[-1][:length_for(w, e)] for e in (64, 256)]
    special += junction_reads(t0, joined, 3)
    special += [reads[j] for j in (0, 1, 5, 13, 40, 99, 150)]      # exact duplicates
    for s in special:                                               # scattered over the second two thirds
        reads.insert(int(rng.integers(len(reads) // 3, len(reads) + 1)), s)
    rng2 = np.random.default_rng(w["seed"] + 1000)                 # (a stream of their own: the reads above stay what they were)
    for j, e in enumerate((1023, 1024, 1025)):
        reads.insert(len(reads) // 2 + 7 * j, rand(rng2, length_for(w, e)))
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def want(i):
    """(keep, records, the filter's bytes, the op ordinal, the largest counter) of world i, by the restatement"""
    w = WORLDS[i]
    cbf = Filter(w["size"], w["H"], K, seed=w["seed"])
    if w["mode"] == "strobemer":
        keep, recs = strobemer_based(cbf, reads_of(i), K, w["M"], w["clip"], INDEL)
    else:
        keep, recs = kmer_based(cbf, reads_of(i), K, w["canonical"], w["M"], w["clip"])
    keep.setflags(write=False); recs.setflags(write=False)
    data = cbf.bytes()
    data.setflags(write=False)
    return keep, recs, data, cbf.ordinal()
