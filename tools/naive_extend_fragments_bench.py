#!/usr/bin/env python3
"""Naive extension of fragments (rb_graph_naive_extend_fragments: GraphUtils.naiveExtend(kmers, graph, maxTipLength, minKmerCov)) timed on the
config-2 graph, beside the route a caller had before: two rb_graph_naive_extend mode-0 calls (graphutils.naiveExtendComposed).
    python tools/naive_extend_fragments_bench.py [fragments=200000] [out=profiles/naive_extend_fragments_bench.txt] [pairs=50000000]
Input: the config-2 graph and the fragments of tools/screen_bench.py — 2 000 of the graph's reads stand in for transcripts; two thirds of the
fragments are one transcript less up to 30 leading bases, one third the first 90 to 150 bases of one joined to another from its base 40 on: about
167 bases a fragment.  min_kmer_cov 1, room 256 (the composed route's cap is 256 too); ONE call of each route: a walk that fills its room is
not resumed by either, and both leave the right walk out behind a left walk that did.
Figures, each the median of 7 repeats behind one warm-up, with minimum and maximum; the two routes alternate inside every repeat, in one
process on one graph, and every repeat's texts are compared:
    the new call end to end (numpy text in; text, offsets and records out), profiling off;
    the composed route end to end (numpy text in, texts out: its two dependent calls with the host work between them);
    the new call's kernel from the profile entry "naive_extend_fragments", in runs of their own;
    whatever profile entries the composed route's calls add to, in runs of their own (rb_graph_naive_extend has none).
The composed route's calls have no profile entry: its kernel time alone is reported as not measured.
Also: the distribution of extension lengths and of the walks' ends — they say how much of the walk a fragment of this input exercises.
They and rb_build_id() go to the output file.  One run, nothing tuned; no figure is promised in advance."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd")):
    sys.path.insert(0, p)

import numpy as np

K, TX, MIN_COV, ROOM, REPEATS = 25, 2_000, 1.0, 256, 7


def spread(xs, scale=1.0, fmt="%.2f"):
    xs = sorted(float(x) * scale for x in xs)
    return ("median " + fmt + " (min " + fmt + ", max " + fmt + ")") % (xs[len(xs) // 2], xs[0], xs[-1])


def histogram(x, edges=(0, 1, 2, 4, 8, 16, 32, 64, 128, 256)):
    """counts of x in [e_i, e_i+1), the last bin closed: '0: n, 1: n, 2-3: n, ...'"""
    x = np.asarray(x)
    out = []
    for lo, hi in zip(edges, edges[1:] + (None,)):
        n = int(((x >= lo) & ((x < hi) if hi is not None else True)).sum())
        out.append("%s: %d" % (str(lo) if hi == lo + 1 else "%d+" % lo if hi is None else "%d-%d" % (lo, hi - 1), n))
    return ", ".join(out)


def main(n_frag, out_path, pairs):
    import torch
    from rnabloom import _native as N
    from rnabloom import graphutils
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
    fseq, foff = _pack(frags)
    sync = torch.cuda.synchronize

    def new():
        return g.naiveExtendFragmentsFlat(fseq, foff, MIN_COV, ROOM)

    def composed():
        return graphutils.naiveExtendComposed(g, frags, MIN_COV, ROOM)

    def timed(fn):
        sync()
        t0 = time.perf_counter(); r = fn(); sync()
        return time.perf_counter() - t0, r

    def texts_of(r):
        out, oo, recs = r
        return [out[oo[i]:oo[i] + recs["out_len"][i]].tobytes() for i in range(n_frag)]

    _, first = timed(new)                                        # warm-up, and the results every later run must repeat
    recs = first[2]
    want = texts_of(first)
    _, got = timed(composed)
    assert got == want
    ends = BloomFilterDeBruijnGraph.NFRAG_ENDS
    tally = lambda f: ", ".join("%s %d" % (ends[e], c) for e, c in enumerate(np.bincount(recs[f], minlength=6)) if c)
    lines = ["build %s" % N.lib.rb_build_id().decode(),
             "naive_extend_fragments: %d fragments (%d bases, %.1f a fragment), k = %d, min_kmer_cov %g, room %d, config-2 graph of %d read pairs: status %s; "
             "fragments extended on the left %d, on the right %d, on either side %d; letters added %d"
             % (n_frag, fseq.size, fseq.size / n_frag, K, MIN_COV, ROOM, pairs,
                ", ".join("%s %d" % (BloomFilterDeBruijnGraph.NFRAG_STATUSES[e], c) for e, c in enumerate(np.bincount(recs["status"], minlength=3)) if c), int((recs["left_ext"] > 0).sum()), int((recs["right_ext"] > 0).sum()),
                int(((recs["left_ext"] > 0) | (recs["right_ext"] > 0)).sum()), int(recs["left_ext"].sum() + recs["right_ext"].sum())),
             "naive_extend_fragments left_end:  %s" % tally("left_end"),
             "naive_extend_fragments right_end: %s" % tally("right_end"),
             "naive_extend_fragments left_ext  (k-mers: fragments): %s" % histogram(recs["left_ext"]),
             "naive_extend_fragments right_ext (k-mers: fragments): %s" % histogram(recs["right_ext"]),
             "naive_extend_fragments steps a fragment (look-up rounds of both walks: k-mers added + 2): mean %.2f"
             % (float(recs["left_ext"].sum() + recs["right_ext"].sum()) / n_frag + 2)]
    # end to end, profiling off, the routes alternating
    t_new, t_comp = [], []
    for _ in range(REPEATS):
        dt, r = timed(new); t_new.append(dt)
        assert r[2].tobytes() == recs.tobytes() and r[0].tobytes() == first[0].tobytes()
        dt, got = timed(composed); t_comp.append(dt)
        assert got == want
    # the kernels, in runs of their own
    g.profileEnable(True); g.profileGet(reset=True)
    k_new, k_comp, comp_entries = [], [], {}
    for _ in range(REPEATS):
        timed(new)
        prof = g.profileGet(reset=True)
        k_new.append(prof["naive_extend_fragments"][0] / 1e3)
        timed(composed)
        prof = g.profileGet(reset=True)
        comp_entries = {name: v[1] for name, v in prof.items()}
        k_comp.append(sum(v[0] for v in prof.values()) / 1e3)
    g.profileEnable(False)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    lines += ["naive_extend_fragments %-52s %s ms = %s us a fragment" % ("the new call, end to end", spread(t_new, 1e3), spread(t_new, 1e6 / n_frag)),
              "naive_extend_fragments %-52s %s ms = %s us a fragment (equal texts)" % ("composed (2 naive_extend calls), end to end", spread(t_comp, 1e3), spread(t_comp, 1e6 / n_frag)),
              "naive_extend_fragments %-52s %s ms" % ("the new call's kernel (profile entry)", spread(k_new, 1e3)),
              "naive_extend_fragments %-52s %s ms (profile entries and launches a route: %s)" % ("composed route's kernels (profile entries summed)", spread(k_comp, 1e3),
                                                                                                   ", ".join("%s %d" % kv for kv in sorted(comp_entries.items())) or "none"),
              "naive_extend_fragments end to end, composed / new (medians): %.2f;  kernels, composed / new (medians): %s"
              % (med(t_comp) / med(t_new), "%.2f" % (med(k_comp) / med(k_new)) if med(k_comp) > 0 else "not measured (the composed route has no profile entry)"),
              "not measured: the kernel's achieved occupancy (by its resources: 85 VGPRs and 32 KB of LDS a workgroup of two wavefronts, so LDS allows five "
              "workgroups = 10 wavefronts a CU), and what a narrower lane mapping than a wavefront per fragment would give (57 of 64 lanes idle in a step's look-ups)."]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    g.destroy()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200_000,
         sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "naive_extend_fragments_bench.txt"),
         int(sys.argv[3]) if len(sys.argv) > 3 else 50_000_000)
