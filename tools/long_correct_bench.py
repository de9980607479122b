#!/usr/bin/env python3
"""Windowed correction of long reads (rb_graph_correct_long: GraphUtils.correctLongSequenceWindowed) timed on synthetic long reads.
    python tools/long_correct_bench.py [reads=2000] [out=profiles/long_correct_bench.txt]
Input: 100 random transcripts of 4 000 bases; `reads` long reads of 1 800 - 2 200 bases cut from them (about ten-fold coverage).  The graph
(k = 35, canonical, filters of getExpectedSize(2 M, 0.01, 2)) is built from the error-free copies; the queries are the same reads with 1 %
substitutions, 1 % insertions and 1 % deletions.  The call runs with the reference's long-read defaults: windows of 500 k-mers, 2 passes,
lookahead 5, max_indel_size 1, percent_identity 0.7, min_kmer_cov 2, max_cov_gradient 0.5, the edge trim on.
Two figures, each the best of 3 after one warm-up: correctLongFlat end to end (host text in, texts and records out) and the profile entry
"correct_long" — the interval from a piece's first to its last kernel, which holds the host's work between the passes (the windows' results come
back, the next texts are laid out), so it is not pure device time.  They, a tally of the records, how many reads came back as their error-free
copy and rb_build_id() go to the output file; no figure is promised in advance."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd")):
    sys.path.insert(0, p)

import numpy as np

K = 35
PARAMS = dict(maxItr=2, maxCovGradient=0.5, lookahead=5, maxIndelSize=1, percentIdentity=0.7, minKmerCov=2, minNumSolidKmers=100, trimLowCovEdges=True,
              windowSize=500)
ACGT = np.frombuffer(b"ACGT", np.uint8)


def with_errors(s, rng, rate=0.01):
    out = bytearray()
    for ch in s:
        r = rng.random()
        if r < rate:
            out.append(int(rng.choice([x for x in b"ACGT" if x != ch])))
        elif r < 2 * rate:
            out.append(ch); out.append(int(ACGT[rng.integers(4)]))
        elif r >= 3 * rate:
            out.append(ch)
    return bytes(out)


def main(n_reads, out_path):
    import torch
    from rnabloom import _native as N
    from rnabloom.graph import BloomFilterDeBruijnGraph, _pack
    rng = np.random.default_rng(35)
    tx = [ACGT[rng.integers(0, 4, 4000)].tobytes() for _ in range(100)]
    clean = []
    for _ in range(n_reads):
        t, n = tx[rng.integers(len(tx))], int(rng.integers(1800, 2201))
        a = int(rng.integers(0, len(t) - n + 1))
        clean.append(t[a:a + n])
    noisy = [with_errors(s, rng) for s in clean]
    bits = N.lib.rb_expected_size(2_000_000, 0.01, 2)
    g = BloomFilterDeBruijnGraph(bits, bits, 1009, 2, 2, 2, K, False, False, rngSeed=1)
    cseq, coff = _pack(clean)
    g.addReads(cseq, np.full(cseq.size, ord("I"), np.uint8), coff, 3)
    seq, off = _pack(noisy)
    oo = np.zeros(len(noisy) + 1, np.int64)
    np.cumsum([len(s) + 64 for s in noisy], out=oo[1:])
    run = lambda: g.correctLongFlat(seq, off, oo, **PARAMS)
    out, recs = run()
    texts = [out[oo[i]:oo[i] + int(recs[i]["out_len"])].tobytes() for i in range(len(noisy))]
    restored = sum(t in c for t, c in zip(texts, clean))                  # (the edge trim takes a k-mer or more off either end)
    names = recs.dtype.names
    lines = ["build %s" % N.lib.rb_build_id().decode(), "one run, nothing tuned",
             "correct_long: %d reads (%d bases, %d k-mers), k = %d, %s" % (len(noisy), seq.size, int(np.maximum(np.diff(off) - K + 1, 0).sum()), K,
                                                                            ", ".join("%s %s" % kv for kv in sorted(PARAMS.items()))),
             "correct_long: status [null, unchanged, changed, no k-mer] %s; passes %s; overflowed %d; trimmed to nothing %d; a substring of the error-free "
             "copy afterwards: %d of %d (before: %d)" % (np.bincount(recs["status"], minlength=4).tolist(), np.bincount(recs["passes"]).tolist(),
                                                         int((recs["flags"] & 1 != 0).sum()), int((recs["flags"] & 2 != 0).sum()), restored, len(noisy),
                                                         sum(t in c for t, c in zip(noisy, clean))),
             "correct_long: events " + ", ".join("%s %d" % (f, int(recs[f].sum())) for f in names[5:15])]
    ts = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter(); run(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    g.profileEnable(True); g.profileGet(reset=True)
    ks = []
    for _ in range(3):
        run(); ks.append(g.profileGet(reset=True)["correct_long"][0] / 1e3)
    g.profileEnable(False)
    for what, dt in (("rb_graph_correct_long (first to last kernel)", min(ks)), ("rb_graph_correct_long (end to end)", min(ts))):
        lines.append("correct_long %-46s %9.2f ms = %8.3f k reads/s = %8.2f M bases/s" % (what, dt * 1e3, len(noisy) / dt / 1e3, seq.size / dt / 1e6))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    g.destroy()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 2_000,
         sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "long_correct_bench.txt"))
