#!/usr/bin/env python3
"""Trimming of reverse-complement artifacts (rb_graph_trim_rc_artifacts: GraphUtils.trimReverseComplementArtifact) timed on the config-2 graph.
    python tools/trim_artifacts_bench.py [fragments=20000] [out=profiles/trim_artifacts_bench.txt] [pairs=50000000] [long_reads=2000]
Input: the config-2 graph as tools/walk_bench.py builds it (50 M synthetic read pairs of 150 bases, k = 25, canonical, three filters of
getExpectedSize(450 M, 0.01, 2), read pairs stored at distance 115).  Modes HASHES and EDGE (max_edge_clip 10, the fragment assembler's
maxTipLength) run on the fragments of tools/screen_bench.py; mode LONG (max_edge_clip 150, max_cov_gradient 0.5) on synthetic long reads,
each thirteen or fourteen of the graph's reads joined, about 2 000 bases.  One sequence in ten (HAIRPIN_EVERY) of either set is made into a
hairpin: the sequence followed by the reverse complement of its last 40 to 100 % (fragments) or 10 to 30 % (long reads).
Per mode two figures, each the best of 3 after one warm-up: trimArtifactsFlat end to end (host text in, records out) and its kernels alone
(profile entry "trim_artifacts").  They, a tally of the records and rb_build_id() go to the output file; no figure is promised in advance."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd")):
    sys.path.insert(0, p)

import numpy as np

K, TX, HAIRPIN_EVERY, EDGE_CLIP, LONG_CLIP, GRADIENT = 25, 2_000, 10, 10, 150, 0.5
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def hairpin(s, share):
    tail = s[len(s) - max(K, int(len(s) * share)):]
    return s + tail.translate(_COMP)[::-1]


def main(n_frag, out_path, pairs, n_long):
    import torch
    from rnabloom import _native as N
    from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch, _pack
    nk = 450_000_000 * pairs // 50_000_000
    bits = N.lib.rb_expected_size(nk, 0.01, 2)
    batch = ReadBatch.synthetic(pairs, 64_000_000 * pairs // 50_000_000, seed=0x5EED)
    g = BloomFilterDeBruijnGraph(bits, bits, bits, 2, 2, 2, K, False, True, rngSeed=1)
    g.setReadPairedKmerDistance(115)
    g.addBatch(batch, storeReadPairedKmers=True, first=0, n=pairs)
    g.addBatch(batch, reverseComplement=True, storeReadPairedKmers=True, first=pairs, n=pairs)
    seq, off = batch.download(0, min(pairs, 200_000))
    rng = np.random.default_rng(11)
    reads = [seq[off[i]:off[i + 1]].tobytes() for i in rng.choice(off.size - 1, TX, replace=False)]
    reads = [s for s in reads if all(c in b"ACGT" for c in s)]
    frags = []
    for i in range(n_frag):
        a, b = reads[rng.integers(len(reads))], reads[rng.integers(len(reads))]
        frags.append(a[:90 + int(rng.integers(60))] + b[40:] if i % 3 == 0 else a[int(rng.integers(30)):])
    frags = [hairpin(s, 0.4 + 0.6 * rng.random()) if i % HAIRPIN_EVERY == 0 else s for i, s in enumerate(frags)]
    longs = [b"".join(reads[j] for j in rng.integers(0, len(reads), 13 + i % 2)) for i in range(n_long)]
    longs = [hairpin(s, 0.1 + 0.2 * rng.random()) if i % HAIRPIN_EVERY == 0 else s for i, s in enumerate(longs)]
    lines = ["build %s" % N.lib.rb_build_id().decode(), "one run, nothing tuned"]
    for name, mode, clip, grad, texts in (("HASHES", g.TRIM_HASHES, 0, 0.0, frags), ("EDGE", g.TRIM_EDGE, EDGE_CLIP, 0.0, frags),
                                          ("LONG", g.TRIM_LONG, LONG_CLIP, GRADIENT, longs)):
        fseq, foff = _pack(texts)
        run = lambda: g.trimArtifactsFlat(fseq, foff, mode, clip, grad)
        recs = run()
        fl = recs["flags"]
        lines.append("trim %s: %d sequences (%d bases, one in %d a hairpin), k = %d, max_edge_clip %d, max_cov_gradient %.2f: found %d, trimmed %d, not judged %d; "
                     "why of pass 0 %s, of pass 1 %s; k-mers kept %d of %d"
                     % (name, len(texts), fseq.size, HAIRPIN_EVERY, K, clip, grad, int((fl & 1 != 0).sum()), int((fl & 2 != 0).sum()), int((fl & 56 != 0).sum()),
                        np.bincount(recs["pass"]["why"][:, 0] + 1, minlength=8).tolist(), np.bincount(recs["pass"]["why"][:, 1] + 1, minlength=8).tolist(),
                        int((recs["end"] - recs["begin"]).sum()), int(np.maximum(np.diff(foff) - K + 1, 0).sum())))
        ts = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter(); run(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        g.profileEnable(True); g.profileGet(reset=True)
        ks = []
        for _ in range(3):
            run(); ks.append(g.profileGet(reset=True)["trim_artifacts"][0] / 1e3)
        g.profileEnable(False)
        for what, dt in (("rb_graph_trim_rc_artifacts %s (kernels)" % name, min(ks)), ("rb_graph_trim_rc_artifacts %s (end to end)" % name, min(ts))):
            lines.append("trim %-50s %9.2f ms = %8.3f M sequences/s" % (what, dt * 1e3, len(texts) / dt / 1e6))
    lines.append("(a why tally starts at the blank -1: [blank, 0, 1, ...])")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    g.destroy()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20_000,
         sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "trim_artifacts_bench.txt"),
         int(sys.argv[3]) if len(sys.argv) > 3 else 50_000_000,
         int(sys.argv[4]) if len(sys.argv) > 4 else 2_000)
