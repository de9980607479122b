#!/usr/bin/env python3
"""Rates of the overlap of read pairs (rb_graph_overlap_pairs) on host sequences: its kernels alone (the graph's profile entry "overlap":
events around each piece's k_overlap launches), the call end to end, and pairs/s.
    python tools/overlap_bench.py [pairs=2000000]
Input: pairs of 150-base reads cut from the two ends of fragments of a random 8 M-base text, all of them inserted into a graph sized like
config 2 (rb_expected_size of their k-mers at FPR 0.01, two hash functions).  Fragment lengths are drawn so that about a third of the pairs
share k bases or more, a third min_overlap .. k - 1, and a third nothing.  For orientation only, the Python restatement of the reference's
lines (tests/test_overlap_rules.py) is timed on the first 20 000 pairs over a graph stub that counts every k-mer 10 — the string work of
GraphUtils.overlap in CPython, no Bloom filter look-up at all; it is no baseline and carries no pass/fail threshold.
Each device figure is the best of 3 calls after one warm-up call."""
import collections, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

K, MO, MINCOV, L = 25, 10, 1.0, 150


def main(n_pairs):
    import numpy as np
    import torch
    from rnabloom import _native as N
    from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch
    rng = np.random.default_rng(12)
    lut = np.frombuffer(b"ACGT", np.uint8)
    G = lut[rng.integers(0, 4, 8_000_000)]
    cls = rng.integers(0, 3, n_pairs)
    o = np.where(cls == 0, rng.integers(K, L, n_pairs), np.where(cls == 1, rng.integers(MO, K, n_pairs), -rng.integers(1, 200, n_pairs)))
    frag = 2 * L - o
    start = rng.integers(0, G.size - 2 * L - 200, n_pairs)
    col = np.arange(L)[None, :]
    lseq = G[start[:, None] + col].reshape(-1)
    rseq = G[(start + frag - L)[:, None] + col].reshape(-1)
    off = np.arange(n_pairs + 1, dtype=np.int64) * L
    nk = 2 * n_pairs * (L - K + 1)
    bits = N.lib.rb_expected_size(nk, 0.01, 2)
    g = BloomFilterDeBruijnGraph(bits, bits, 1009, 2, 2, 2, K, False, True, rngSeed=1)
    for s in (lseq, rseq):
        g.addBatch(ReadBatch.from_ascii(s, None, off, 0))
    call = lambda: g.overlapPairsFlat(lseq, off, rseq, off, MO, MINCOV)
    out, oo, recs = call()
    tally = collections.Counter(zip(recs["outcome"].tolist(), recs["why"].tolist()))
    print("overlap %d pairs of %d bases, k = %d, min_overlap = %d: %s" % (n_pairs, L, K, MO, ", ".join(
        "%s/%s %d" % (g.OVL_OUTCOMES[a], g.OVL_WHYS[b], c) for (a, b), c in sorted(tally.items()))))
    ts = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter(); call(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    g.profileEnable(True)
    g.profileGet(reset=True)
    dms = []
    for _ in range(3):
        call()
        dms.append(g.profileGet(reset=True)["overlap"][0] / 1e3)
    g.profileEnable(False)
    for what, dt in (("overlapPairs (device, kernels)", min(dms)), ("overlapPairs (end to end)", min(ts))):
        print("overlap %-34s %9.2f ms = %8.3f M pairs/s" % (what, dt * 1e3, n_pairs / dt / 1e6))
    # orientation: the restatement in CPython on a sample, every k-mer counted 10 (no look-up)
    import test_overlap_rules as R

    class Stub:
        def counts(self, seq):
            return [10.0] * max(0, len(seq) - K + 1)
    m = min(20_000, n_pairs)
    lb, rb = lseq[:m * L].tobytes(), rseq[:m * L].tobytes()
    t0 = time.perf_counter()
    got = [R.expected(lb[i * L:(i + 1) * L], rb[i * L:(i + 1) * L], K, MO, MINCOV, Stub())[0][0] for i in range(m)]
    dt = time.perf_counter() - t0
    same = int((np.array(got) == recs["outcome"][:m]).sum())
    print("overlap %-34s %9.2f ms = %8.3f M pairs/s (%d pairs; %d of them with the device's outcome — the stub knows no graph)" % (
        "restatement in CPython (orientation)", dt * 1e3, m / dt / 1e6, m, same))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000)
