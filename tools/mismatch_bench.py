#!/usr/bin/env python3
"""Rates of mismatch correction (rb_graph_correct_mismatches) on host sequences: the call end to end, its kernels alone (the graph's
profile entry "mismatches": events around each piece's getKmers + k_mismatch kernels), and for context the host-driven form of the same
work through the entry points that existed before — getKmers of every sequence to the host, the first-round forward candidates found
there, and ONE getKmers over all their alternative strings (3 per candidate, 2k - 1 bases each).  That host path is timed optimistically:
no contains gate, no second round, no reverse scan, nothing rewritten.
    python tools/mismatch_bench.py                      both steps below, each in a child process under its own time limit
    python tools/mismatch_bench.py short [reads=2000000]    150-base reads of a config-2-shaped synthetic library, one substitution planted per read
    python tools/mismatch_bench.py frags [frags=200000]     fragments of 300-600 bases with substitutions at 0.2 %
Figures: sequences/s, candidate positions/s (positions of the initial profile that pass the forward test — the replacements made are
printed beside them) and k-mer lookups/s, a lookup being one k-mer's two dbgbf + two cbf probes: every window once for the profile plus
4 k per candidate on the device (3 k through the host path).  4 random lines a lookup against the 54 G random lines/s of DESIGN.md §5.
Each figure is the best of 3 calls after one warm-up call."""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd")):
    sys.path.insert(0, p)

K, T, MINCOV = 25, 10.0, 1.0
STEP_LIMIT_S = 420


def best(fn, reps=3):
    import torch
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def candidates(c, ko, k, thr):
    """forward candidates of the initial profile: global k-mer index of every i in [1, nk - k - 1] with c[i] < T, c[i-1] >= T, c[i+k] >= T"""
    import numpy as np
    nk = np.diff(ko)
    row = np.repeat(np.arange(nk.size), nk)
    p = np.arange(c.size) - ko[:-1][row]
    ok = (p >= 1) & (p <= nk[row] - k - 1)
    idx = np.nonzero(ok)[0]
    low = c < thr
    return idx[low[idx] & ~low[idx - 1] & ~low[idx + k]], row, p


def host_path(g, seq, off, thr):
    import numpy as np
    ko, f, r, c = kmers_flat(g, seq, off)
    cand, row, p = candidates(c, ko, g.k, thr)
    if cand.size == 0:
        return 0
    start = off[:-1][row[cand]] + p[cand]                       # text position of window i
    w = 2 * g.k - 1
    txt = seq[start[:, None] + np.arange(w)[None, :]]           # s[i .. i + 2k - 2]
    alts = np.repeat(txt, 3, axis=0)
    old = alts[:, g.k - 1]
    lut = np.frombuffer(b"ACGT", np.uint8)
    code = np.searchsorted(lut, np.where(np.isin(old, lut), old, lut[0]))
    alts[:, g.k - 1] = lut[(code + 1 + np.tile(np.arange(3), cand.size)) % 4]
    aoff = np.arange(alts.shape[0] + 1, dtype=np.int64) * w
    kmers_flat(g, alts.reshape(-1), aoff)
    return cand.size


def kmers_flat(g, seq, off):
    import numpy as np
    from rnabloom import _native as N
    from rnabloom.graph import _ptr
    n = off.size - 1
    ko = np.zeros(n + 1, np.int64)
    N.check(N.lib.rb_graph_kmers(g.h, _ptr(seq), _ptr(off), n, _ptr(ko), None, None, None))
    t = int(ko[-1])
    f = np.empty(t, np.uint64); r = np.empty(t, np.uint64); c = np.empty(t, np.float32)
    N.check(N.lib.rb_graph_kmers(g.h, _ptr(seq), _ptr(off), n, _ptr(ko), _ptr(f), _ptr(r), _ptr(c)))
    return ko, f, r, c


def run(name, g, seq, off):
    import numpy as np
    n = off.size - 1
    ko, _, _, c = kmers_flat(g, seq, off)
    ncand = candidates(c, ko, g.k, T)[0].size
    out, nf, _, _ = g.correctMismatchesFlat(seq, off, T, MINCOV)
    total = int(ko[-1])
    print("%s %d sequences, %d k-mers, %d forward candidates in the initial profile, %d replacements in %d sequences" % (
        name, n, total, ncand, int(nf.sum()), int((nf > 0).sum())))
    dev_lookups, host_lookups = total + 4 * g.k * ncand, total + 3 * g.k * ncand
    cases = [("correctMismatches (end to end)", best(lambda: g.correctMismatchesFlat(seq, off, T, MINCOV)), dev_lookups),
             ("host path: getKmers + candidates + getKmers(alts)", best(lambda: host_path(g, seq, off, T)), host_lookups)]
    g.profileEnable(True)
    g.profileGet(reset=True)
    dms = []
    for _ in range(3):
        g.correctMismatchesFlat(seq, off, T, MINCOV)
        dms.append(g.profileGet(reset=True)["mismatches"][0] / 1e3)
    g.profileEnable(False)
    cases.insert(0, ("correctMismatches (device, kernels)", min(dms), dev_lookups))
    for what, dt, lookups in cases:
        print("%s %-50s %9.2f ms = %7.3f M sequences/s, %7.3f M candidates/s, %6.3f G lookups/s (%5.2f G lines/s of 54)" % (
            name, what, dt * 1e3, n / dt / 1e6, ncand / dt / 1e6, lookups / dt / 1e9, 4 * lookups / dt / 1e9))


def short(n_reads):
    import numpy as np
    from rnabloom import _native as N
    from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch
    pairs = n_reads // 2
    nk = pairs * 2 * (150 - K + 1)
    bits = N.lib.rb_expected_size(nk, 0.01, 2)
    batch = ReadBatch.synthetic(pairs, 64_000_000 * pairs // 50_000_000, seed=0x5EED)
    g = BloomFilterDeBruijnGraph(bits, bits, 1009, 2, 2, 2, K, False, True, rngSeed=1)
    g.addBatch(batch, first=0, n=pairs)
    g.addBatch(batch, reverseComplement=True, first=pairs, n=pairs)
    seq, off = batch.download()
    batch.close()
    seq = np.array(seq, copy=True)
    rng = np.random.default_rng(8)
    pos = off[:-1] + rng.integers(K, 150 - K, off.size - 1)      # one substitution per read, where both scans can reach it
    lut = np.frombuffer(b"ACGT", np.uint8)
    code = np.searchsorted(lut, np.where(np.isin(seq[pos], lut), seq[pos], lut[0]))
    seq[pos] = lut[(code + rng.integers(1, 4, pos.size)) % 4]
    run("short", g, seq, off)


def frags(n_frags):
    import numpy as np
    from rnabloom import _native as N
    from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch
    rng = np.random.default_rng(4)
    lut = np.frombuffer(b"ACGT", np.uint8)
    G = lut[rng.integers(0, 4, 2_000_000)]
    lens = rng.integers(300, 601, n_frags)
    starts = rng.integers(0, G.size - 601, n_frags)
    off = np.zeros(n_frags + 1, np.int64); np.cumsum(lens, out=off[1:])
    seq = np.concatenate([G[s:s + L] for s, L in zip(starts, lens)])
    nk = int(np.maximum(lens - K + 1, 0).sum())
    bits = N.lib.rb_expected_size(nk, 0.01, 2)
    g = BloomFilterDeBruijnGraph(bits, bits, 1009, 2, 2, 2, K, False, True, rngSeed=1)
    g.addBatch(ReadBatch.from_ascii(seq, None, off, 0))
    err = rng.random(seq.size) < 0.002
    seq = np.array(seq, copy=True)
    seq[err] = lut[(np.searchsorted(lut, seq[err]) + rng.integers(1, 4, int(err.sum()))) % 4]
    run("frags", g, seq, off)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode == "short":
        short(int(sys.argv[2]) if len(sys.argv) > 2 else 2_000_000)
    elif mode == "frags":
        frags(int(sys.argv[2]) if len(sys.argv) > 2 else 200_000)
    else:
        # every GPU step is a child process with a time limit of its own; a step that fails or runs over ends the tool
        for step in ("short", "frags"):
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), step], timeout=STEP_LIMIT_S).returncode
            if rc:
                sys.exit(rc)
