#!/usr/bin/env python3
"""The in-order represented-then-add loop (rb_graph_represented_then_add: TranscriptWriter.write, GraphUtils.reduceRedundancy) timed on the
config-2 graph.
    python tools/represented_then_add_bench.py [fragments=20000] [out=profiles/represented_then_add_bench.txt] [pairs=50000000]
Input: the config-2 graph and the fragments of tools/represented_bench.py (which are tools/screen_bench.py's), in list order, with one in
ten replaced by an earlier fragment of the list or by a one-letter variant of one — what a writer sees when two fragments assemble to the same
transcript.  Parameters as tools/represented_bench.py: lookahead 3, maxIndelSize 1, maxTipLength 25, percentIdentity 0.9.  The gate starts EMPTY
before every timed call (bf.empty(), outside the timed window) and is sized for every k-mer of the list at an FPR of 0.005.
Figures, each the median of 7 repeats behind one warm-up, with minimum and maximum:
    the call end to end (host text in; records, keep flags and medians out), profiling off;
    its kernels — getKmers and the one-workgroup walker of every piece — from the profile entry "represented_then_add", in runs of their own;
    the kept count (it does not vary: the loop is exact);
    a two-parameter least-squares fit t = a * kept + b * represented over the list walked in calls of 500 against the one growing gate;
    the composed route (graph.represented with n = 1, then bf.add) on the first 1 500 fragments beside the one call on the same 1 500, in
    the same process, with equal records, keep flags and gate bytes.
They, a tally of the records and rb_build_id() go to the output file.  No figure is promised in advance."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd")):
    sys.path.insert(0, p)

import numpy as np

K, LOOKAHEAD, MAX_INDEL, MAX_TIP, IDENTITY, TX = 25, 3, 1, 25, 0.9, 2_000
REPEATS, CALL, COMPOSED = 7, 500, 1_500
SETTING = (LOOKAHEAD, MAX_INDEL, MAX_TIP, IDENTITY)


def spread(xs, scale=1.0, fmt="%.2f"):
    xs = sorted(float(x) * scale for x in xs)
    return ("median " + fmt + " (min " + fmt + ", max " + fmt + ")") % (xs[len(xs) // 2], xs[0], xs[-1])


def fragments(reads, n_frag, rng):
    """tools/represented_bench.py's fragments; then every tenth place takes an earlier fragment, or one with a letter changed"""
    frags = []
    for i in range(n_frag):
        a, b = reads[rng.integers(len(reads))], reads[rng.integers(len(reads))]
        frags.append(a[:90 + int(rng.integers(60))] + b[40:] if i % 3 == 0 else a[int(rng.integers(30)):])
    again = variants = 0
    for i in range(10, n_frag, 10):
        s = frags[int(rng.integers(i))]
        if rng.integers(2):
            p = int(rng.integers(len(s)))
            s = s[:p] + bytes([b"ACGT"[(b"ACGT".index(s[p]) + 1 + int(rng.integers(3))) % 4]]) + s[p + 1:]
            variants += 1
        else:
            again += 1
        frags[i] = s
    return frags, again, variants


def main(n_frag, out_path, pairs):
    import torch
    from rnabloom import _native as N
    from rnabloom import graphutils
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
    frags, again, variants = fragments(reads, n_frag, rng)
    fseq, foff = _pack(frags)
    bf = BloomFilter(N.lib.rb_expected_size(max(int(foff[-1]), 1000), 0.005, 2), 2, K)
    sync = torch.cuda.synchronize

    def whole():
        return g.representedThenAddFlat(fseq, foff, bf, *SETTING)

    def timed(fn):
        bf.empty(); sync()
        t0 = time.perf_counter(); r = fn(); sync()
        return time.perf_counter() - t0, r

    _, (recs, keep, median, done) = timed(whole)                 # warm-up, and the results every later run must repeat
    gate_after = bf.toBytes().copy()
    fl = recs["flags"]
    lines = ["build %s" % N.lib.rb_build_id().decode(),
             "represented_then_add: %d fragments (%d bases; %d places hold an earlier fragment again, %d a one-letter variant of one), k = %d, "
             "lookahead %d, max_indel %d, max_edge_clip %d, identity %.2f, the gate empty at the start: kept %d, represented %d, not judged %d, "
             "n_done %d; why %s; path_form %s; tests passed %d, tips skipped %d; gate bits set %d of %d"
             % (n_frag, fseq.size, again, variants, K, *SETTING, int(keep.sum()), int((fl & 1 != 0).sum()), int((fl & 120 != 0).sum()), done,
                np.bincount(recs["why"][recs["why"] >= 0], minlength=10).tolist(), np.bincount(recs["path_form"], minlength=4).tolist(),
                int(recs["tests_passed"].sum()), int(recs["tips_skipped"].sum()), int(np.unpackbits(gate_after).sum()), bf.getSize())]
    # end to end, profiling off
    ts, kept_counts = [], []
    for _ in range(REPEATS):
        dt, (r2, k2, m2, d2) = timed(whole)
        ts.append(dt); kept_counts.append(int(k2.sum()))
        assert r2.tobytes() == recs.tobytes() and k2.tobytes() == keep.tobytes() and m2.tobytes() == median.tobytes() and d2 == done
    assert (bf.toBytes() == gate_after).all()
    # the kernels, in runs of their own
    g.profileEnable(True); g.profileGet(reset=True)
    ks, launches = [], 0
    for _ in range(REPEATS):
        timed(whole)
        ms, launches = g.profileGet(reset=True)["represented_then_add"][:2]
        ks.append(ms / 1e3)
    g.profileEnable(False)
    # calls of 500 against the one growing gate: t = a * kept + b * represented
    fits = []
    for _ in range(REPEATS):
        bf.empty(); sync()
        rows, tcs = [], []
        for a in range(0, n_frag, CALL):
            b = min(n_frag, a + CALL)
            t0 = time.perf_counter()
            r, kp, _, _ = g.representedThenAddFlat(fseq[foff[a]:foff[b]], foff[a:b + 1] - foff[a], bf, *SETTING, wantMedian=False)
            sync(); tcs.append(time.perf_counter() - t0)
            rows.append((int(kp.sum()), int((r["flags"] & 1 != 0).sum())))
            assert r.tobytes() == recs[a:b].tobytes()
        fits.append(np.linalg.lstsq(np.asarray(rows, np.float64), np.asarray(tcs, np.float64), rcond=None)[0])
    assert (bf.toBytes() == gate_after).all()
    # the composed route beside the one call, on the head of the list
    nc = min(COMPOSED, n_frag)
    head = frags[:nc]
    hseq, hoff = _pack(head)
    one, comp = [], []
    for _ in range(REPEATS):
        dt, (r1, k1, _, _) = timed(lambda: g.representedThenAddFlat(hseq, hoff, bf, *SETTING))
        one.append(dt); gate1 = bf.toBytes().copy()
        dt, (rc, kc, _) = timed(lambda: graphutils.representedThenAddComposed(g, bf, head, *SETTING))
        comp.append(dt)
        assert rc.tobytes() == r1.tobytes() == recs[:nc].tobytes() and kc.tobytes() == k1.tobytes() and (bf.toBytes() == gate1).all()
    lines += ["represented_then_add %-44s %s ms = %s us a fragment" % ("the call, end to end", spread(ts, 1e3), spread(ts, 1e3 * 1e3 / n_frag)),
              "represented_then_add %-44s %s ms = %s us a fragment (%d launches of the bracket a call)"
              % ("its kernels (profile entry)", spread(ks, 1e3), spread(ks, 1e3 * 1e3 / n_frag), launches),
              "represented_then_add %-44s %s" % ("kept", spread(kept_counts, fmt="%d")),
              "represented_then_add %-44s per kept sequence %s us, per represented sequence %s us"
              % ("fit over calls of %d, end to end" % CALL, spread([f[0] for f in fits], 1e6), spread([f[1] for f in fits], 1e6)),
              "represented_then_add %-44s %s ms" % ("the first %d: one call" % nc, spread(one, 1e3)),
              "represented_then_add %-44s %s ms (equal records, keep flags and gate bytes)" % ("the first %d: composed, n = 1 then add" % nc, spread(comp, 1e3)),
              "not measured: the walker's occupancy (one workgroup of 256 threads on one CU, by construction), and the walker's share of an idle "
              "device — nothing else ran in this process, so what a concurrent batched call would gain beside it is not known from these figures."]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    g.destroy(); bf.destroy()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20_000,
         sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "represented_then_add_bench.txt"),
         int(sys.argv[3]) if len(sys.argv) > 3 else 50_000_000)
