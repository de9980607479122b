"""The worlds of tests/test_long_correction_reach.py (CPU) and tests/test_gpu_long_correction.py: seeded, the k-mer counts planted through the
oracle graph (oracle.rbo).  A world is a handful of random transcripts covered about 17-fold by error-free short reads, a few thinly covered
alleles (a substitution known to the graph once, twice or six times), and long query reads cut from the transcripts with the errors of long
reads: substitutions, deletions of one letter (the SNV bubble's case: k - 1 k-mers over the junction) and of more, insertions, a thin or thick
allele, a jump to another transcript with a substitution beside it, letters outside ACGTU inside and at the edge of a bad run, lower case
and U, foreign letters at both ends; and the odd ones: empty, shorter than k, k and k + 1 letters, a foreign letter before k + 1 good ones
(the edge trim leaves nothing), random letters (the solid-k-mer screen).  `want(case)` is what the restatement of
tests/test_long_correction_rules.py makes of the queries, computed once per case and shared."""
import functools

import numpy as np

from oracle import rbo
from test_gpu_error_correction import OracleSide
from test_long_correction_rules import CTRS, FIELDS, OVERFLOW, correct_long

ACGT = np.frombuffer(b"ACGT", np.uint8)
SIZES = (1_600_033, 1_600_033, 1009)

# k, stranded, big (reads up to 1 500 letters for windows of 500; else 60 - 400 letters for windows of 40), then the parameters
CASES = [
    dict(k=16, stranded=False, big=False, windowSize=40, maxIndelSize=1, percentIdentity=0.9, maxItr=5, trimLowCovEdges=False, minKmerCov=1, minNumSolidKmers=0, lookahead=5),
    dict(k=16, stranded=True, big=False, windowSize=40, maxIndelSize=0, percentIdentity=1.0, maxItr=1, trimLowCovEdges=True, minKmerCov=2, minNumSolidKmers=0, lookahead=3),
    dict(k=25, stranded=False, big=False, windowSize=40, maxIndelSize=5, percentIdentity=0.9, maxItr=5, trimLowCovEdges=True, minKmerCov=2, minNumSolidKmers=3, lookahead=5),
    dict(k=25, stranded=True, big=True, windowSize=500, maxIndelSize=1, percentIdentity=0.9, maxItr=5, trimLowCovEdges=False, minKmerCov=1, minNumSolidKmers=0, lookahead=5),
    dict(k=25, stranded=False, big=True, windowSize=500, maxIndelSize=5, percentIdentity=1.0, maxItr=1, trimLowCovEdges=True, minKmerCov=3, minNumSolidKmers=10, lookahead=7),
    dict(k=16, stranded=False, big=True, windowSize=500, maxIndelSize=1, percentIdentity=0.9, maxItr=0, trimLowCovEdges=True, minKmerCov=2, minNumSolidKmers=0, lookahead=5),
    dict(k=64, stranded=False, big=False, windowSize=40, maxIndelSize=1, percentIdentity=0.9, maxItr=5, trimLowCovEdges=True, minKmerCov=1, minNumSolidKmers=0, lookahead=5),
]


def case_id(c):
    return "k%d-%s-w%d-indel%d-pid%g-itr%d-trim%d-cov%d-solid%d" % (c["k"], "ss" if c["stranded"] else "ds", c["windowSize"], c["maxIndelSize"],
                                                                     c["percentIdentity"], c["maxItr"], c["trimLowCovEdges"], c["minKmerCov"], c["minNumSolidKmers"])


def params_of(c):
    return {key: v for key, v in c.items() if key not in ("k", "stranded", "big")}


def other(ch, rng):
    return int(rng.choice([x for x in b"ACGT" if x != ch]))


class LongWorld:
    def __init__(self, k, stranded, big, seed):
        rng = self.rng = np.random.default_rng(seed)
        self.k, self.stranded, self.big = k, stranded, big
        L = max(150, 3 * k)                                                  # the short reads the graph is made of
        n_tx, tx_len, n_q, q_len = (5, (1700, 2100), 216, (600, 1500)) if big else (8, (500, 700), 300, (max(60, k + 20), 400))
        self.tx = [ACGT[rng.integers(0, 4, int(rng.integers(*tx_len)))].tobytes() for _ in range(n_tx)]
        if k == 64:                                                          # (AC)^32 and (CA)^32 hash alike at k = 64: a repeat the walks run into
            t = self.tx[0]
            self.tx[0] = t[:200] + b"AC" * 50 + t[200:]
        reads = []
        for t in self.tx:
            for _ in range(len(t) * 20 // L):
                a = int(rng.integers(0, len(t) - L))
                reads.append(t[a:a + L])
            reads += [t[:L]] * 8 + [t[-L:]] * 8
        q = self.queries = []
        for i in range(n_q):
            t = self.tx[int(rng.integers(0, n_tx))]
            n = int(rng.integers(*q_len))
            a = int(rng.integers(0, len(t) - n))
            b = bytearray(t[a:a + n])
            kind = i % 12
            spots = sorted(int(x) for x in rng.choice(np.arange(k + 8, n - k - 8), max(1, n // 90), replace=False)) if n > 2 * k + 20 else []
            if kind == 1 or kind == 11:                                      # substitutions (11: a second one within k of each)
                for p in spots:
                    b[p] = other(b[p], rng)
                    if kind == 11:
                        b[p + 3] = other(b[p + 3], rng)
            elif kind in (2, 3, 4):                                          # deletions of 1, of 2 - 3, insertions of 1 - 3 letters
                for p in reversed(spots):
                    if kind == 4:
                        b[p:p] = ACGT[rng.integers(0, 4, int(rng.integers(1, 4)))].tobytes()
                    else:
                        del b[p:p + (1 if kind == 2 else int(rng.integers(2, 4)))]
            elif kind in (5, 6):                                             # an allele the graph knows thinly (1 or 2 reads) or well (6)
                for p in spots[:2]:
                    b[p] = other(b[p], rng)
                    reads += [bytes(b[p - k + 1:p + k])] * ((1, 2)[i % 24 < 12] if kind == 5 else 6)
            elif kind == 7 and spots:                                        # a jump into another transcript, a substitution three letters on
                p = spots[0]
                u = self.tx[(self.tx.index(t) + 1) % n_tx]
                b = bytearray(bytes(b[:p]) + u[50:50 + n - p])
                if p + 3 < len(b):
                    b[p + 3] = other(b[p + 3], rng)
            elif kind == 8:                                                  # letters outside ACGTU: inside a bad run, at its edge, by themselves
                for j, p in enumerate(spots[:3]):
                    if j == 0:
                        b[p], b[p + 2] = other(b[p], rng), ord("N")
                    elif j == 1:
                        b[p], b[p + k] = other(b[p], rng), ord("R")
                    else:
                        b[p] = ord("N")
            elif kind == 9:                                                  # lower case and U, and a substitution among them
                for p in spots[:2]:
                    b[p - 6:p + 6] = bytes(b[p - 6:p + 6]).lower().replace(b"t", b"u")
                    b[p + 8] = other(b[p + 8], rng)
            elif kind == 10:                                                 # foreign letters at both ends
                b = bytearray(ACGT[rng.integers(0, 4, int(rng.integers(2, 12)))].tobytes() + bytes(b) + ACGT[rng.integers(0, 4, int(rng.integers(2, 12)))].tobytes())
            q.append(bytes(b))
        t = self.tx[1]
        q += [b"", b"ACGT", t[:k - 1], t[100:100 + k], t[100:100 + k + 1], bytes([other(t[99], rng)]) + t[100:100 + k + 1],
              ACGT[rng.integers(0, 4, 3 * k)].tobytes(), b"N" * (k + 3)]
        self.reads = reads
        self.og = rbo.Graph(*SIZES, 2, 2, 2, k, stranded, True, 5)
        self.packed = rbo.pack_reads(reads, [b"I" * len(s) for s in reads])
        self.og.add_reads(*self.packed, 3, 0)
        self.o = OracleSide(self.og)
        self.gg = None

    def device(self):
        from rnabloom import _native as N
        from rnabloom.graph import BloomFilterDeBruijnGraph
        if self.gg is None:
            self.gg = BloomFilterDeBruijnGraph(*SIZES, 2, 2, 2, self.k, self.stranded, True, rngSeed=5)
            self.gg.addReads(*self.packed, 3)
            assert (self.gg.exportFilter(N.DBGBF) == self.og.dbgbf_bytes()).all() and (self.gg.exportFilter(N.CBF) == self.og.cbf_bytes()).all()
        return self.gg

    def expected(self, seqs, **params):
        """[(text — the input where the reference returns null —, the record as a tuple in FIELDS' order, overflow left out)]"""
        out = []
        for s in seqs:
            text, rec = correct_long(s, self.k, self.o, **params)
            out.append((s if text is None else text, tuple(rec[f] for f in FIELDS)))
        return out


@functools.lru_cache(maxsize=None)
def world(k, stranded, big):
    return LongWorld(k, stranded, big, seed=1000 + 10 * k + 2 * stranded + big)


@functools.lru_cache(maxsize=None)
def _want(i):
    c = CASES[i]
    w = world(c["k"], c["stranded"], c["big"])
    return w, w.expected(w.queries, **params_of(c))


def want(i):
    """the world of CASES[i] and the restatement's answers for its queries"""
    return _want(i)


def with_overflow(rec, room):
    """the expected record of a call that gave the sequence `room` letters"""
    rec = list(rec)
    if rec[FIELDS.index("out_len")] > room:
        rec[FIELDS.index("flags")] |= OVERFLOW
    return tuple(rec)
