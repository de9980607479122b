#!/usr/bin/env python3
"""Rates of error correction (rb_graph_correct_errors) on host sequences: the call end to end, its kernels by phase (the graph's profile
entries "correct_errors" and "correct_errors.<phase>"), and for context a host-driven round of the same work through the entry points
that existed before: rb_graph_kmers for the profiles, the gap scan in numpy, rb_graph_neighbors for the tips' variants,
rb_graph_greedy_extend for the tips and rb_graph_walk for the path gaps (one call per distinct bound — the bound is part of the rule —
and the walk back only for the gaps whose first walk did not arrive), then rb_graph_correct_mismatches.  That host path is timed
optimistically: no SNV candidates, no joins, no Levenshtein distances, nothing stitched.
    python tools/correct_errors_bench.py                    the step below in a child process under its own time limit
    python tools/correct_errors_bench.py short [reads=2000000]   150-base reads of the config-2-shaped synthetic library, errors kept
Each time is the best of 3 calls after one warm-up call."""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd")):
    sys.path.insert(0, p)

K, T, MINCOV, LOOKAHEAD, MAX_INDEL, PID = 25, 10.0, 1.0, 5, 1, 0.9
STEP_LIMIT_S = 540
PHASES = ("profile", "scan", "walks", "resolve", "stitch", "mismatch")


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


def gap_scan(c, ko, k, thr):
    """(sequence, first bad k-mer, run) of every gap, in numpy"""
    import numpy as np
    nk = np.diff(ko)
    row = np.repeat(np.arange(nk.size), nk)
    p = np.arange(c.size) - ko[:-1][row]
    low = c < thr
    prev = np.concatenate([[False], low[:-1]]); nxt = np.concatenate([low[1:], [False]])
    s = np.nonzero(low & ((p == 0) | ~prev))[0]
    e = np.nonzero(low & ((p == nk[row] - 1) | ~nxt))[0]
    run = e - s + 1
    keep = run < nk[row[s]]
    return row[s][keep], p[s][keep], run[keep], s[keep]


def host_path(g, seq, off):
    import numpy as np
    k = g.k
    ko, f, r, c = kmers_flat(g, seq, off)
    sq, first, run, gi = gap_scan(c, ko, k, T)
    nk = np.diff(ko)
    left, right = first == 0, first + run == nk[sq]
    path = ~left & ~right & (run != k)
    kmer_at = lambda s_, p_: seq[(off[:-1][s_] + p_)[:, None] + np.arange(k)[None, :]]
    # variants of the bad k-mer next to the good one
    for m, side in ((left, 2), (right, 3)):
        j = gi[m] + (run[m] - 1 if side == 2 else 0)
        if j.size:
            ch = seq[off[:-1][sq[m]] + (first[m] + run[m] - 1 if side == 2 else first[m] + k - 1)]
            g.getNeighbors(f[j], r[j], ch, side)
    # the tips, one call per bound
    for m, direction in ((left & (run >= LOOKAHEAD), 1), (right & (run >= LOOKAHEAD), 0)):
        for b in np.unique(run[m]):
            mm = m & (run == b)
            seeds = kmer_at(sq[mm], first[mm] + run[mm] if direction == 1 else first[mm] - 1)
            greedy_flat(g, seeds, direction, int(b))
    # the path gaps, one call per bound; the walk back for those that did not arrive
    for b in np.unique(run[path]):
        mm = path & (run == b)
        lk, rk = kmer_at(sq[mm], first[mm] - 1), kmer_at(sq[mm], first[mm] + run[mm])
        reason = walk_flat(g, lk, rk, 0, int(b) + MAX_INDEL)
        todo = reason != 1
        if todo.any():
            walk_flat(g, rk[todo], lk[todo], 1, int(b) + MAX_INDEL)
    g.correctMismatchesFlat(seq, off, T, MINCOV)
    return sq.size


def greedy_flat(g, seeds, direction, bound):
    import numpy as np
    from rnabloom import _native as N
    from rnabloom.graph import _ptr
    n = seeds.shape[0]
    sb = np.ascontiguousarray(seeds)
    bases = np.zeros((n, bound), np.uint8); ln = np.zeros(n, np.int32); reason = np.zeros(n, np.uint8); c = np.zeros((n, bound), np.float32)
    N.check(N.lib.rb_graph_greedy_extend(g.h, None, _ptr(sb), n, direction, LOOKAHEAD, bound, _ptr(bases), _ptr(c), _ptr(ln), _ptr(reason)))


def walk_flat(g, seeds, targets, direction, bound):
    import numpy as np
    from rnabloom import _native as N
    from rnabloom.graph import _ptr
    n = seeds.shape[0]
    sb, tb = np.ascontiguousarray(seeds), np.ascontiguousarray(targets)
    bases = np.zeros((n, bound), np.uint8); ln = np.zeros(n, np.int32); reason = np.zeros(n, np.uint8); f = np.zeros((n, bound), np.uint64)
    N.check(N.lib.rb_graph_walk(g.h, _ptr(sb), _ptr(tb), n, direction, bound, MINCOV, _ptr(bases), _ptr(f), None, None, _ptr(ln), _ptr(reason)))
    return reason


def run(name, g, seq, off):
    import numpy as np
    n = off.size - 1
    call = lambda gaps=False: g.correctErrorsFlat(seq, off, T, LOOKAHEAD, MAX_INDEL, PID, MINCOV, gaps=gaps)
    out, oo, ol, fl, rec, go = call(True)
    kinds = np.bincount(rec["kind"].astype(np.int64) * 3 + rec["outcome"], minlength=12).reshape(4, 3)
    print("%s %d sequences, %d gaps (rows left edge / right edge / SNV / path, columns kept / replaced / trimmed: %s), %d sequences corrected, "
          "%d by gap repair, %d by the mismatch pass" % (name, n, rec.size, kinds.tolist(), int((fl & 1).astype(bool).sum()),
                                                         int((fl & 2).astype(bool).sum()), int((fl & 4).astype(bool).sum())))
    ngaps = rec.size
    t_call = best(lambda: call())
    t_host = best(lambda: host_path(g, seq, off))
    g.profileEnable(True)
    g.profileGet(reset=True)
    runs = []
    for _ in range(3):
        call()
        runs.append(g.profileGet(reset=True))
    g.profileEnable(False)
    bestrun = min(runs, key=lambda p: p["correct_errors"][0])
    rows = [("correctErrors (device, first to last kernel)", bestrun["correct_errors"][0] / 1e3)]
    rows += [("  phase %s" % ph, bestrun.get("correct_errors." + ph, (0.0, 0))[0] / 1e3) for ph in PHASES]
    rows += [("correctErrors (end to end)", t_call), ("host path: kmers + numpy scan + neighbors + greedy + walks + mismatches", t_host)]
    for what, dt in rows:
        print("%s %-72s %9.2f ms = %7.3f M sequences/s, %7.3f M gaps/s" % (name, what, dt * 1e3, n / max(dt, 1e-9) / 1e6, ngaps / max(dt, 1e-9) / 1e6))
    print("%s end to end against the host path: %.2fx" % (name, t_host / t_call))


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
    run("short", g, np.ascontiguousarray(seq), np.ascontiguousarray(off))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode == "short":
        short(int(sys.argv[2]) if len(sys.argv) > 2 else 2_000_000)
    else:
        # the GPU step is a child process with a time limit of its own; a step that fails or runs over ends the tool
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "short"], timeout=STEP_LIMIT_S).returncode)
