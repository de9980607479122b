#!/usr/bin/env python3
"""The represented screen (rb_graph_represented: GraphUtils.represented) timed on the config-2 graph, on the fragments of tools/screen_bench.py.
    python tools/represented_bench.py [fragments=20000] [out=profiles/represented_bench.txt] [pairs=50000000]
Input: the config-2 graph as tools/walk_bench.py builds it (50 M synthetic read pairs of 150 bases, k = 25, canonical, three filters of
getExpectedSize(450 M, 0.01, 2), read pairs stored at distance 115); 2 000 of its reads stand in for transcripts, and a gate — a stand-alone
BloomFilter — holds the k-mers of every other one.  Fragments: two thirds are one transcript less up to 30 leading bases, one third the
first 90 to 150 bases of one transcript joined to another from its base 40 on; each is judged with lookahead 3, maxIndelSize 1,
maxEdgeClipLength 25 and percentIdentity 0.9.
Two figures, each the best of 3 after one warm-up: representedFlat end to end (host text in, records out) and its kernels alone
(profile entry "represented").  They, a tally of the records and rb_build_id() go to the output file; no figure is promised in advance."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd")):
    sys.path.insert(0, p)

import numpy as np

K, LOOKAHEAD, MAX_INDEL, MAX_DEPTH, IDENTITY, TX = 25, 3, 1, 25, 0.9, 2_000


def main(n_frag, out_path, pairs):
    import torch
    from rnabloom import _native as N
    from rnabloom.bloom import BloomFilter
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
    bf = BloomFilter(N.lib.rb_expected_size(TX * 150, 0.005, 2), 2, K)
    for s in reads[::2]:
        _, f, r, _ = g.getKmers([s])
        bf.add(np.where(r.view(np.int64) < f.view(np.int64), r, f))
    frags = []
    for i in range(n_frag):
        a, b = reads[rng.integers(len(reads))], reads[rng.integers(len(reads))]
        frags.append(a[:90 + int(rng.integers(60))] + b[40:] if i % 3 == 0 else a[int(rng.integers(30)):])
    fseq, foff = _pack(frags)
    run = lambda: g.representedFlat(fseq, foff, bf, LOOKAHEAD, MAX_INDEL, MAX_DEPTH, IDENTITY)
    recs = run()
    fl = recs["flags"]
    lines = ["build %s" % N.lib.rb_build_id().decode(),
             "represented: %d fragments (%d bases), k = %d, lookahead %d, max_indel %d, max_edge_clip %d, identity %.2f, gate of %d of %d transcripts: "
             "represented %d, not judged %d; why %s; path_form %s; tests passed %d, tips skipped %d"
             % (n_frag, fseq.size, K, LOOKAHEAD, MAX_INDEL, MAX_DEPTH, IDENTITY, len(reads[::2]), len(reads), int((fl & 1 != 0).sum()), int((fl & 56 != 0).sum()),
                np.bincount(recs["why"][recs["why"] >= 0], minlength=10).tolist(), np.bincount(recs["path_form"], minlength=4).tolist(),
                int(recs["tests_passed"].sum()), int(recs["tips_skipped"].sum()))]
    ts = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter(); run(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    g.profileEnable(True); g.profileGet(reset=True)
    ks = []
    for _ in range(3):
        run(); ks.append(g.profileGet(reset=True)["represented"][0] / 1e3)
    g.profileEnable(False)
    for what, dt in (("rb_graph_represented (kernels)", min(ks)), ("rb_graph_represented (end to end)", min(ts))):
        lines.append("represented %-40s %9.2f ms = %8.3f M fragments/s" % (what, dt * 1e3, n_frag / dt / 1e6))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    g.destroy(); bf.destroy()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20_000,
         sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "represented_bench.txt"),
         int(sys.argv[3]) if len(sys.argv) > 3 else 50_000_000)
