#!/usr/bin/env python3
"""Preparation of raw long reads (rb_long_prepare: what LongReadCorrectionWorker.run does before its first graph call) timed on synthetic reads.
    python tools/long_prepare_bench.py [reads=200000] [out=profiles/long_prepare_bench.txt]
Input: `reads` random reads of 1 800 - 2 200 letters.  A quarter end in a poly-A tail and a quarter begin with a poly-T head of 15 - 60 letters
with 5 % foreign letters; a fifth carry one or two low-complexity stretches (a repeat of one to three letters) of 300 - 900 letters.  The call
runs with the worker's parameters (graphutils.PREP_DEFAULTS, k = 25) and returns the transformed text too.
Figures, each the median of 7 runs after one warm-up, with minimum and maximum: the kernels from a piece's first to its last (the call's
kernel_ms, by events); the call end to end (host text in, records, segments and text out); the upload of the same text alone in the same process,
from pageable and from pinned host memory (a torch copy).  Two ratios give the scale: kernel time to upload time, and kernel time per read
against rb_graph_correct_long's in profiles/long_correct_bench.txt.  Neither is a criterion; occupancy and the binding resource are not measured."""
import os, re, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd")):
    sys.path.insert(0, p)

import numpy as np

K = 25
ACGT = np.frombuffer(b"ACGT", np.uint8)


def make_reads(n_reads, rng):
    lens = rng.integers(1800, 2201, n_reads)
    off = np.zeros(n_reads + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    seq = ACGT[rng.integers(0, 4, int(off[-1]), dtype=np.uint8)]
    kind = rng.random(n_reads)
    n_tail = n_head = n_low = 0
    for i in range(n_reads):
        a, b = int(off[i]), int(off[i + 1])
        if kind[i] < 0.5:                                            # a tail (first quarter) or a head (second)
            m = int(rng.integers(15, 61))
            run = np.full(m, ord("A") if kind[i] < 0.25 else ord("T"), np.uint8)
            bad = rng.choice(m, max(1, m // 20), replace=False)
            run[bad] = ord("C")
            if kind[i] < 0.25:
                seq[b - m:b] = run; n_tail += 1
            else:
                seq[a:a + m] = run; n_head += 1
        elif kind[i] < 0.7:                                          # one or two low-complexity stretches
            for _ in range(int(rng.integers(1, 3))):
                m, u = int(rng.integers(300, 901)), int(rng.integers(1, 4))
                at = a + int(rng.integers(0, b - a - m))
                seq[at:at + m] = np.resize(rng.permutation(ACGT)[:u], m)
            n_low += 1
    return seq, off, (n_tail, n_head, n_low)


def stats(ts):
    return "median %9.2f ms (min %9.2f, max %9.2f)" % (1e3 * float(np.median(ts)), 1e3 * min(ts), 1e3 * max(ts))


def main(n_reads, out_path):
    import torch
    from rnabloom import _native as N
    from rnabloom import graphutils
    rng = np.random.default_rng(2500)
    seq, off, (n_tail, n_head, n_low) = make_reads(n_reads, rng)
    ms = np.zeros(1)
    run = lambda: graphutils.prepareLongFlat(seq, off, K, kernelMs=ms)
    recs, so, segs, out = run()
    fl = recs["flags"]
    lines = ["build %s" % N.lib.rb_build_id().decode(), "one run, nothing tuned",
             "long_prepare: %d reads (%d letters; %d with a tail, %d with a head, %d with low stretches), k = %d, %s"
             % (n_reads, seq.size, n_tail, n_head, n_low, K, ", ".join("%s %s" % kv for kv in sorted(graphutils.PREP_DEFAULTS.items()))),
             "long_prepare: status [short, low complexity, segments] %s; tail found %d, head found %d, hasPolyA %d, turned %d, cut fired %d; segments %d, "
             "reads with several %d; letters kept %d"
             % (np.bincount(recs["status"], minlength=3).tolist(), int((fl & N.PREP_TAIL_FOUND != 0).sum()), int((fl & N.PREP_HEAD_FOUND != 0).sum()),
                int((fl & N.PREP_HAS_POLYA != 0).sum()), int((fl & N.PREP_REVCOMP != 0).sum()), int((fl & N.PREP_CUT_FIRED != 0).sum()),
                int(recs["n_segments"].sum()), int((recs["n_segments"] > 1).sum()), int((recs["kept_end"] - recs["kept_begin"]).sum()))]
    ks, ts = [], []
    for _ in range(7):
        torch.cuda.synchronize(); t0 = time.perf_counter(); run(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        ks.append(ms[0] / 1e3)
    host = torch.from_numpy(seq)
    pinned = host.pin_memory()
    ups = {"pageable": [], "pinned": []}
    for name, src in (("pageable", host), ("pinned", pinned)):
        src.to("cuda"); torch.cuda.synchronize()
        for _ in range(7):
            torch.cuda.synchronize(); t0 = time.perf_counter(); d = src.to("cuda"); torch.cuda.synchronize(); ups[name].append(time.perf_counter() - t0)
            del d
    k_med, t_med = float(np.median(ks)), float(np.median(ts))
    lines += ["long_prepare kernels (first to last of a piece)   %s = %8.2f G letters/s = %8.3f M reads/s" % (stats(ks), seq.size / k_med / 1e9, n_reads / k_med / 1e6),
              "long_prepare the call end to end, text back       %s = %8.2f G letters/s = %8.3f M reads/s" % (stats(ts), seq.size / t_med / 1e9, n_reads / t_med / 1e6)]
    for name in ("pageable", "pinned"):
        u = float(np.median(ups[name]))
        lines.append("long_prepare upload of the text alone, %-9s  %s = %8.2f GB/s; kernels / upload = %.2f" % (name, stats(ups[name]), seq.size / u / 1e9, k_med / u))
    ref = os.path.join(ROOT, "profiles", "long_correct_bench.txt")
    m = re.search(r"^correct_long: (\d+) reads.*?^correct_long rb_graph_correct_long \(first to last kernel\)\s+([0-9.]+) ms", open(ref).read(), re.S | re.M) if os.path.exists(ref) else None
    if m:
        per_corr, per_prep = float(m.group(2)) * 1e3 / int(m.group(1)), k_med * 1e6 / n_reads
        lines.append("long_prepare kernels per read %.3f us; rb_graph_correct_long (profiles/long_correct_bench.txt) %.3f us per read: 1 to %.0f"
                     % (per_prep, per_corr, per_corr / per_prep))
    lines.append("occupancy and the binding resource: not measured")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000,
         sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "long_prepare_bench.txt"))
