#!/usr/bin/env python3
"""The extension loop of fragments (rb_graph_extend_loop: GraphUtils.extendSE / extendPE with every round on the device) timed on the config-2
graph against the host route it replaces (graphutils.extendSE / extendPE: one step call per round, the loop's bookkeeping in Python).
    python tools/extend_loop_bench.py [fragments=20000] [out=profiles/extend_loop_bench.txt] [pairs=50000000]
Input: the config-2 graph as tools/screen_bench.py builds it (50 M synthetic read pairs of 150 bases, k = 25, canonical, three filters of
getExpectedSize(450 M, 0.01, 2), read pairs stored at distance 115) with a fragment-pair filter of the same size at distance 80 that holds
the pairs of the fragments and of the 2 000 reads they are cut from; the fragments are screen_bench's (about 167 bases: two thirds a read less
up to 30 leading bases, one third the head of one read joined to the tail of another).
For SE and for PE, in one process: graphutils.extend{SE,PE}OnDevice (room 4096) — one warm-up call, then one timed call end to end and one
with profiling on for the kernels alone (profile entry "extend_loop") — and then graphutils.extend{SE,PE}, the host route, once; texts and
ranges of the two routes are asserted equal.  Reported with them: accepted rounds per sequence (median and maximum), the letters added, how
the sides ended, and rb_build_id().  No figure is promised in advance; the figure of merit is the ratio of the two routes in this one run."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd")):
    sys.path.insert(0, p)

import numpy as np

K, D_READ, D_FRAG, TX, ROOM = 25, 115, 80, 2_000, 4096


def main(n_frag, out_path, pairs):
    import torch
    from rnabloom import _native as N
    from rnabloom import graphutils
    from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch, _pack
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    nk = 450_000_000 * pairs // 50_000_000
    bits = N.lib.rb_expected_size(nk, 0.01, 2)
    batch = ReadBatch.synthetic(pairs, 64_000_000 * pairs // 50_000_000, seed=0x5EED)
    g = BloomFilterDeBruijnGraph(bits, bits, bits, 2, 2, 2, K, False, True, rngSeed=1)
    g.setReadPairedKmerDistance(D_READ)
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
    g.initializePairKmersBloomFilter(bits, 2)
    g.setFragPairedKmerDistance(D_FRAG)
    for part in (reads, frags):
        fseq, foff = _pack([s for s in part if len(s) >= K + D_FRAG])
        g.addFragments(ReadBatch.from_ascii(fseq, None, foff, 3), loadPairedKmers=True)
    say("build %s" % N.lib.rb_build_id().decode())
    say("extend_loop: %d fragments (%d bases), k = %d, read-pair distance %d, fragment-pair distance %d, room %d, minKmerCov 1; one run, nothing tuned"
        % (n_frag, sum(len(s) for s in frags), K, D_READ, D_FRAG, ROOM))
    for name, which, on_device, host in (("extendSE", g.EXTL_SE, graphutils.extendSEOnDevice, graphutils.extendSE),
                                         ("extendPE", g.EXTL_PE, graphutils.extendPEOnDevice, graphutils.extendPE)):
        on_device(g, frags, 1.0, room=ROOM)                    # warm-up
        torch.cuda.synchronize(); t0 = time.perf_counter(); texts, ranges = on_device(g, frags, 1.0, room=ROOM); torch.cuda.synchronize()
        t_dev = time.perf_counter() - t0
        g.profileEnable(True); g.profileGet(reset=True)
        on_device(g, frags, 1.0, room=ROOM)
        t_k, launches = g.profileGet(reset=True)["extend_loop"][:2]
        g.profileEnable(False)
        _, recs = g.extendLoop(frags, which, 1.0, ROOM)        # the first call's records: rounds, endings
        rounds = recs["left_rounds"] + recs["right_rounds"]
        added = sum(len(t) - len(s) for t, s in zip(texts, frags))
        say("%s rounds per sequence in the first call: median %d, maximum %d; steps %d; letters added %d (%.1f a sequence, the most %d); out of room after it %d; "
            "not judged %d; left ends %s, right ends %s" % (name, int(np.median(rounds)), int(rounds.max()), int(recs["steps"].sum()), added, added / n_frag,
                                                           max(len(t) - len(s) for t, s in zip(texts, frags)), int((recs["status"] == g.EXTL_ROOM).sum()),
                                                           int((recs["status"] == g.EXTL_NOT_JUDGED).sum()), np.bincount(recs["left_end"], minlength=5).tolist(),
                                                           np.bincount(recs["right_end"], minlength=5).tolist()))
        say("%s %-34s %10.2f ms  (%d pieces, resumed calls included)" % (name, "on the device, kernels", t_k, launches))
        say("%s %-34s %10.2f ms = %8.3f M fragments/s" % (name, "on the device, end to end", t_dev * 1e3, n_frag / t_dev / 1e6))
        torch.cuda.synchronize(); t0 = time.perf_counter(); htexts, hranges = host(g, frags, 1.0); torch.cuda.synchronize()
        t_host = time.perf_counter() - t0
        assert htexts == texts and hranges == ranges, name
        say("%s %-34s %10.2f ms = %8.3f M fragments/s; texts and ranges equal; host / device end to end = %.1f"
            % (name, "host route (a step call a round)", t_host * 1e3, n_frag / t_host / 1e6, t_host / t_dev))
    g.destroy()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20_000,
         sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "extend_loop_bench.txt"),
         int(sys.argv[3]) if len(sys.argv) > 3 else 50_000_000)
