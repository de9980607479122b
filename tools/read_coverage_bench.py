#!/usr/bin/env python3
"""Rates of the stage-2 screening leg on reads resident in HBM, in G k-mers/s: the count profile (batchCounts) left on the device and
copied to the host, against the coverage statistics (coverageStats) left on the device and copied to the host.
    python tools/read_coverage_bench.py short [pairs=5000000]          150-base reads of a synthetic library, k = 25, reads mode
    python tools/read_coverage_bench.py long [reads=40000] [window=50]  2-5 kb reads with 1 % errors, k = 35, windows mode (and reads mode)
Each figure is the best of 5 calls after one warm-up call."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch
from rnabloom import _native as N
from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch


def best(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def report(name, nk, cases):
    for what, dt in cases:
        print("%s %-34s %8.2f ms = %6.2f G k-mers/s" % (name, what, dt * 1e3, nk / dt / 1e9))
    dev_p, dev_s = cases[0][1], cases[2][1]
    print("%s coverageStats on the device / batchCounts on the device: %.3f; to the host: %.3f" % (name, dev_s / dev_p, cases[3][1] / cases[1][1]))


def run(name, g, batch, n, ko, **kw):
    total = int(ko[-1]) if ko is not None else None
    if ko is None:
        stride = C_stride(g, batch)
        total = n * stride
    dev = torch.empty(total, dtype=torch.float32, device="cuda:0")
    host = np.empty(total, np.float32)
    cases = [("batchCounts(to_host=False)", best(lambda: g.batchCounts(batch, 0, n, koffsets=ko, to_host=False, out=dev))),
             ("batchCounts(to_host=True)", best(lambda: g.batchCounts(batch, 0, n, koffsets=ko, out=host))),
             ("coverageStats(to_host=False)", best(lambda: g.coverageStats(batch, 0, n, to_host=False, **kw))),
             ("coverageStats(to_host=True)", best(lambda: g.coverageStats(batch, 0, n, **kw)))]
    rec = g.coverageStats(batch, 0, n, **kw)[0]
    print("%s %d reads, %d k-mers, %d records; SE threshold found for %.1f %% of them" % (name, n, total, rec.size, 100.0 * (rec["flags"] & 1 != 0).mean()))
    report(name, total, cases)


def C_stride(g, batch):
    import ctypes as C
    s = C.c_int64(0)
    N.check(N.lib.rb_graph_batch_counts(g.h, batch.h, 0, 0, None, None, 0, C.byref(s)))
    return s.value


def short(pairs):
    nk = 450_000_000 * pairs // 50_000_000
    bits = N.lib.rb_expected_size(nk, 0.01, 2)
    batch = ReadBatch.synthetic(pairs, 64_000_000 * pairs // 50_000_000, seed=0x5EED)
    g = BloomFilterDeBruijnGraph(bits, bits, 10_007, 2, 2, 2, 25, False, False, rngSeed=1)
    g.addBatch(batch, first=0, n=pairs)
    g.addBatch(batch, reverseComplement=True, first=pairs, n=pairs)
    # the screen runs on reads as stage 1 left them: the first file's reads (the synthetic batch carries no quality mask)
    run("short", g, batch, pairs, None, lookahead=3, maxCovGradient=0.5, covFPR=0.01, minKmerCov=1.0)


def long(n_reads, window):
    rng = np.random.default_rng(4)
    T = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 20_000_000)]
    lens = rng.integers(2000, 5001, n_reads)
    starts = rng.integers(0, T.size - 5001, n_reads)
    off = np.zeros(n_reads + 1, np.int64); np.cumsum(lens, out=off[1:])
    seq = np.concatenate([T[s:s + L] for s, L in zip(starts, lens)])
    err = rng.random(seq.size) < 0.01
    seq[err] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(err.sum()))]
    nk = int(off[-1])
    bits = N.lib.rb_expected_size(nk, 0.01, 2)
    g = BloomFilterDeBruijnGraph(bits, bits, 10_007, 2, 2, 2, 35, False, False, rngSeed=1)
    g.addReads(seq, None, off, 0)
    batch = ReadBatch.from_ascii(seq, None, off, 0)
    ko = np.zeros(n_reads + 1, np.int64); np.cumsum(np.maximum(lens - 34, 0), out=ko[1:])
    run("long-windows", g, batch, n_reads, ko, window=window, lookahead=3, maxCovGradient=0.5, covFPR=0.0, minKmerCov=3.0)
    run("long-reads", g, batch, n_reads, ko, lookahead=3, maxCovGradient=0.5, covFPR=0.0, minKmerCov=3.0)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "short"
    if mode == "short":
        short(int(sys.argv[2]) if len(sys.argv) > 2 else 5_000_000)
    else:
        long(int(sys.argv[2]) if len(sys.argv) > 2 else 40_000, int(sys.argv[3]) if len(sys.argv) > 3 else 50)
