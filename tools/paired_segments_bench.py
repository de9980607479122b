#!/usr/bin/env python3
"""Rates of paired-k-mer segmentation (rb_graph_paired_kmer_segments) on host sequences, in G pair positions/s end to end, against the
host path it replaces (getKmers to the host + pair keys on the host + rb_filter_lookup, on the first 1 M sequences at most: 20 bytes a
k-mer come back; the segment loop itself is left out, so that path is timed optimistically) and against batchCounts on the same sequences resident in HBM (the random-line reference point).
    python tools/paired_segments_bench.py short [reads=5000000]     150-base reads of a synthetic library, k = 25, rpkbf, d = 115
    python tools/paired_segments_bench.py frags [frags=200000]      fragments of 300-600 bases, k = 25, rpkbf (d = 115) and fpkbf (d = 200)
Each figure is the best of 3 calls after one warm-up call.  The device-side figure is the time of the two kernels (k_pair_support,
k_pair_segments) of one call, from the graph's profile (rb_graph_profile_enable: events around each piece's kernels on the call's stream)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch
from rnabloom import _native as N
from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch, _ptr


def best(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def combine(a, b):
    with np.errstate(over="ignore"):
        return a ^ (b + np.uint64(0xFFFFFFFF9E3779B9) + (a << np.uint64(6)) + (b >> np.uint64(2)))


def host_path(g, which, seq, off, d):
    """getKmers of every sequence to the host, the canonical pair keys there, rb_filter_lookup of the keys: the support bytes only"""
    n = off.size - 1
    ko = np.zeros(n + 1, np.int64)
    N.check(N.lib.rb_graph_kmers(g.h, _ptr(seq), _ptr(off), n, _ptr(ko), None, None, None))
    t = int(ko[-1])
    f = np.empty(t, np.uint64); r = np.empty(t, np.uint64); c = np.empty(t, np.float32)
    N.check(N.lib.rb_graph_kmers(g.h, _ptr(seq), _ptr(off), n, _ptr(ko), _ptr(f), _ptr(r), _ptr(c)))
    nk = np.diff(ko)
    npos = np.maximum(nk - d, 0)
    row = np.repeat(np.arange(n), npos)
    p = np.arange(int(npos.sum())) - np.repeat(np.cumsum(npos) - npos, npos)
    i = ko[:-1][row] + p
    x = combine(f[i], f[i + d]); y = combine(r[i + d], r[i])
    keys = np.where(y.view(np.int64) < x.view(np.int64), y, x)
    out = np.empty(keys.size, np.uint8)
    N.check(N.lib.rb_filter_lookup(g.h, which, _ptr(keys), keys.size, _ptr(out)))
    return out


def run(name, g, which, seq, off, d):
    n = off.size - 1
    nk = np.maximum(np.diff(off) - g.k + 1, 0)
    pos = int(np.maximum(nk - d, 0).sum())
    so, segs, ns, _, _ = g.pairedKmerSegmentsFlat(which, seq, off, 1)
    print("%s %d sequences, %d k-mers, %d pair positions, %d segments (%.3f per sequence)" % (name, n, int(nk.sum()), pos, int(ns.sum()), ns.mean()))
    batch = ReadBatch.from_ascii(seq, None, off, 0)
    ko = np.zeros(n + 1, np.int64); np.cumsum(nk, out=ko[1:])
    dev = torch.empty(int(ko[-1]), dtype=torch.float32, device="cuda:0")
    m = min(n, 1_000_000)
    hseq, hoff = seq[:off[m]], off[:m + 1]
    hpos = int(np.maximum(nk[:m] - d, 0).sum())
    cases = [("pairedKmerSegments n=1 (end to end)", best(lambda: g.pairedKmerSegmentsFlat(which, seq, off, 1)), pos),
             ("pairedKmerSegments n=3 (end to end)", best(lambda: g.pairedKmerSegmentsFlat(which, seq, off, 3)), pos),
             ("host path, %d seqs: getKmers+keys+lookup" % m, best(lambda: host_path(g, which, hseq, hoff, d)), hpos),
             ("batchCounts(to_host=False), k-mers", best(lambda: g.batchCounts(batch, 0, n, koffsets=ko, to_host=False, out=dev)), int(ko[-1]))]
    g.profileEnable(True)
    g.profileGet(reset=True)
    dms = []
    for _ in range(3):
        g.pairedKmerSegmentsFlat(which, seq, off, 1)
        dms.append(g.profileGet(reset=True)["pair_segments"][0] / 1e3)
    g.profileEnable(False)
    cases.insert(0, ("pairedKmerSegments n=1 (device, kernels)", min(dms), pos))
    for what, dt, units in cases:
        print("%s %-42s %9.2f ms = %6.3f G/s" % (name, what, dt * 1e3, units / dt / 1e9))
    batch.close()


def short(n_reads):
    pairs = n_reads // 2
    k, d = 25, 115
    nk = pairs * 2 * (150 - k + 1)
    bits = N.lib.rb_expected_size(nk, 0.01, 2)
    pk = N.lib.rb_expected_size(pairs * 2 * (150 - k + 1 - d), 0.01, 2)
    batch = ReadBatch.synthetic(pairs, 64_000_000 * pairs // 50_000_000, seed=0x5EED)
    g = BloomFilterDeBruijnGraph(bits, bits, pk, 2, 2, 2, k, False, True, rngSeed=1)
    g.setReadPairedKmerDistance(d)
    g.addBatch(batch, first=0, n=pairs, storeReadPairedKmers=True)
    g.addBatch(batch, reverseComplement=True, first=pairs, n=pairs, storeReadPairedKmers=True)
    seq, off = batch.download()
    batch.close()
    run("short", g, N.RPKBF, seq, off, d)


def frags(n_frags):
    k, read_d, frag_d = 25, 115, 200
    rng = np.random.default_rng(4)
    T = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 20_000_000)]
    lens = rng.integers(300, 601, n_frags)
    starts = rng.integers(0, T.size - 601, n_frags)
    off = np.zeros(n_frags + 1, np.int64); np.cumsum(lens, out=off[1:])
    seq = np.concatenate([T[s:s + L] for s, L in zip(starts, lens)])
    err = rng.random(seq.size) < 0.002
    seq[err] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(err.sum()))]
    nk = int(np.maximum(lens - k + 1, 0).sum())
    bits = N.lib.rb_expected_size(nk, 0.01, 2)
    g = BloomFilterDeBruijnGraph(bits, bits, bits, 2, 2, 2, k, False, True, rngSeed=1)
    g.setReadPairedKmerDistance(read_d)
    g.initializePairKmersBloomFilter(bits, 2); g.setFragPairedKmerDistance(frag_d)
    fb = ReadBatch.from_ascii(seq, None, off, 0)
    g.addFragments(fb, loadPairedKmers=True)
    fb.close()
    run("frags-rpkbf", g, N.RPKBF, seq, off, read_d)
    run("frags-fpkbf", g, N.FPKBF, seq, off, frag_d)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "short"
    if mode == "short":
        short(int(sys.argv[2]) if len(sys.argv) > 2 else 5_000_000)
    else:
        frags(int(sys.argv[2]) if len(sys.argv) > 2 else 200_000)
