#!/usr/bin/env python3
"""Rates of the connection of read segments through the graph (rb_graph_connect_segments) on host sequences: its kernels alone (the graph's
profile entry "connect": events around each piece's k_connect_gaps and k_connect_reads launches), the call end to end, and — in the same process,
alternating with it — the same input through the composed route a caller had before (graphutils.connectComposed: getMaxCoveragePaths in two
lane-per-walk launches per bound, letters copied to the host, stitched there).
    python tools/connect_bench.py [reads=200000]
Input: 150-base reads cut from a random 2 M-base text, each with one or two masked stretches of 1 .. 10 bases (the segment lists
SeqUtils.filterFastq makes of quality-masked reads), and the text itself in 150-base tiles inserted into a graph sized like config 2
(rb_expected_size of the tiles' k-mers at FPR 0.01, two hash functions); k = 25.  Random text has next to no forks: nearly every gap is closed
by the left walk.  There is no pass/fail threshold.  Each figure is the best of 3 calls after one warm-up call; the first line is the id of the
sources the library was built from."""
import collections, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd")):
    sys.path.insert(0, p)

K, L = 25, 150


def main(n_reads):
    import numpy as np
    import torch
    from rnabloom import _native as N
    from rnabloom import graphutils
    from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch
    print("build %s" % N.lib.rb_build_id().decode())
    rng = np.random.default_rng(22)
    lut = np.frombuffer(b"ACGT", np.uint8)
    G = lut[rng.integers(0, 4, 2_000_000)]
    col = np.arange(L)[None, :]
    tiles = np.arange(0, G.size - L + 1, L - K)               # every k-mer of the text inside some tile
    tseq = G[tiles[:, None] + col].reshape(-1)
    toff = np.arange(tiles.size + 1, dtype=np.int64) * L
    bits = N.lib.rb_expected_size(tiles.size * (L - K + 1), 0.01, 2)
    g = BloomFilterDeBruijnGraph(bits, bits, 1_000_003, 2, 2, 2, K, False, False, rngSeed=1)
    g.addBatch(ReadBatch.from_ascii(tseq, None, toff, 0))
    # the lists: a read's letters with its masked stretches turned into N, the entries' boundaries, three or five entries a read
    start = rng.integers(0, G.size - L, n_reads)
    reads = G[start[:, None] + col].copy()
    two = rng.integers(0, 2, n_reads) == 1
    m1, m2 = rng.integers(1, 11, n_reads), rng.integers(1, 11, n_reads)
    s1 = np.where(two, rng.integers(K, 41, n_reads), rng.integers(K, L - K - 10, n_reads))
    s2 = s1 + m1 + K + rng.integers(0, 21, n_reads)           # <= 40 + 10 + 25 + 20 = 95: the last segment keeps 45 letters or more
    so, rs = [0], [0]
    for i in range(n_reads):
        base = i * L
        reads[i, s1[i]:s1[i] + m1[i]] = 78
        cuts = [s1[i], s1[i] + m1[i]]
        if two[i]:
            reads[i, s2[i]:s2[i] + m2[i]] = 78
            cuts += [s2[i], s2[i] + m2[i]]
        so += [base + c for c in cuts] + [base + L]
        rs.append(rs[-1] + len(cuts) + 1)
    seq, so, rs = reads.reshape(-1), np.asarray(so, np.int64), np.asarray(rs, np.int64)
    text = seq.tobytes()
    lists = [[text[so[j]:so[j + 1]] for j in range(rs[i], rs[i + 1])] for i in range(n_reads)]
    fused = lambda: g.connectSegmentsFlat(seq, so, rs, 0, 1.0, gaps=True)
    composed = lambda: graphutils.connectComposed(g, lists)
    out, oo, recs, grecs = fused()
    texts = composed()                                        # (the warm-up of both, and the two routes must agree)
    same = sum(out[oo[i]:oo[i] + recs[i]["out_len"]].tobytes() == texts[i] for i in range(n_reads))
    tally = collections.Counter(grecs["how"].tolist())
    print("connect %d reads of %d bases, %d gaps of 1 .. 10 bases, k = %d: %s; gaps connected %d; reads whose text the composed route agrees on %d" % (
        n_reads, L, len(grecs), K, ", ".join("%s %d" % (g.CONNECT_HOWS[a], c) for a, c in sorted(tally.items())), int(grecs["connected"].sum()), same))
    tf, tc = [], []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fused(); torch.cuda.synchronize(); tf.append(time.perf_counter() - t0)
        torch.cuda.synchronize(); t0 = time.perf_counter(); composed(); torch.cuda.synchronize(); tc.append(time.perf_counter() - t0)
    g.profileEnable(True)
    g.profileGet(reset=True)
    dms = []
    for _ in range(3):
        fused()
        dms.append(g.profileGet(reset=True)["connect"][0] / 1e3)
    g.profileEnable(False)
    for what, dt in (("connectSegments (device, kernels)", min(dms)), ("connectSegments (end to end)", min(tf)), ("composed getMaxCoveragePaths route", min(tc))):
        print("connect %-36s %10.2f ms = %8.3f M reads/s" % (what, dt * 1e3, n_reads / dt / 1e6))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000)
