#!/usr/bin/env python3
"""The fragment-paired branch extension (rb_graph_extend_pe, GraphUtils.extendRightPE) timed on the world of tools/extend_step_bench.py plus
fragments.
    python tools/extend_pe_bench.py [sequences=20000] [out=profiles/extend_pe_bench.txt]
Input: the isoform world of tests/test_extend_pe_rules.py at d_r = 100, d_f = 200 (k = 25, canonical, transcripts of 900 bases tiled every 25
bases with 250-base reads through addReads with storeReadPairedKmers; of every three transcripts one is a fragment as a whole, one over its
first 60 %, one not at all, through addFragments with loadPairedKmers), and as sequences the ones that world cuts so that they end at a fork
or at the first of two forks in a row (the whole prefix, its last 5 to 7 k-mers, its last k-mer), repeated up to the number asked for.
Floor 1 for every sequence, direction 0.
Two figures, each the best of 3 after one warm-up: extendStepPEFlat end to end (host text in, records and bases out), and its kernels alone
(profile entry "extend_pe").  They and rb_build_id() go to the output file; no figure is promised in advance."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np

K, D_R, D_F, FLOOR = 25, 100, 200, 1.0


def main(n_seq, out_path):
    import torch
    import test_extend_pe_rules as P
    from rnabloom import _native as N
    from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch, _pack
    w = P.WorldPE(K, False, 900, D_R, D_F, n_iso=12, read_len=250, tile=25, tx_len=900)
    g = BloomFilterDeBruijnGraph(*w.sizes, *w.hashes, K, False, True, rngSeed=5)
    g.setReadPairedKmerDistance(D_R)
    g.addReads(*w.packed, 3, storeReadPairedKmers=True)
    g.initializePairKmersBloomFilter(w.FSIZE, w.frag_h)
    g.setFragPairedKmerDistance(D_F)
    fseq, foff = _pack(w.frags)
    g.addFragments(ReadBatch.from_ascii(fseq, None, foff, 3), loadPairedKmers=True)
    at_fork = ("fork-0", "fork-short-0", "fork-one-kmer", "fork2", "fork2-short", "fork2-one-kmer")   # long, 7 k-mers, one k-mer
    pool = [s for kind, s, dd in w.queries if dd == 0 and kind in at_fork]
    seqs = [pool[i % len(pool)] for i in range(n_seq)]
    seq, off = _pack(seqs)
    new = lambda: g.extendStepPEFlat(seq, off, 0, FLOOR)
    bases, recs, _ = new()
    tally = np.bincount(recs["outcome"], minlength=4)
    lines = ["build %s" % N.lib.rb_build_id().decode(),
             "extend pe: %d sequences ending at forks (%d distinct), k = %d, d_r = %d, d_f = %d, floor %g: none %d, single %d, first %d, second %d; "
             "%d with a bound lowered by the repeat scan" % (n_seq, len(pool), K, D_R, D_F, FLOOR, *tally, int((recs["max_ext"] < D_F - 2).sum()))]
    ts = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter(); new(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    g.profileEnable(True); g.profileGet(reset=True)
    ks = []
    for _ in range(3):
        new(); ks.append(g.profileGet(reset=True)["extend_pe"][0] / 1e3)
    g.profileEnable(False)
    for what, dt in (("rb_graph_extend_pe (kernels)", min(ks)), ("rb_graph_extend_pe (end to end)", min(ts))):
        lines.append("extend pe %-40s %9.2f ms = %8.3f M sequences/s" % (what, dt * 1e3, n_seq / dt / 1e6))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    g.destroy()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20_000,
         sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "extend_pe_bench.txt"))
