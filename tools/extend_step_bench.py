#!/usr/bin/env python3
"""The paired-k-mer branch extension (rb_graph_extend_se, GraphUtils.extendRightSE) against the same step composed from the calls the library
had before it: rb_graph_kmers, rb_graph_neighbors, rb_graph_naive_extend mode 2 and rb_filter_lookup on the read-pair filter.
    python tools/extend_step_bench.py [sequences=20000] [out=profiles/extend_step_bench.txt]
Input: the isoform worlds of tests/test_extend_step_rules.py at d = 100 (k = 25, canonical, transcripts of 900 bases tiled every 25 bases with
250-base reads, inserted through addReads so that the read-pair filter is filled by the product path), and as sequences the ones that world
cuts so that they end at a fork or at the first of two forks in a row (the whole prefix, its last 5 to 7 k-mers, its last k-mer), repeated up
to the number asked for.  Floor 1 for every sequence, direction 0.
  new call: extendStepSEFlat end to end (host text in, records and bases out), and its kernels alone (profile entry "extend_se").
  composed: every stage holds all sequences in ONE call, as a careful host caller would batch them — tails' k-mers, the last k-mers'
  successors, a NoBackChecks walk per candidate, the walked k-mers, their pair look-ups, then for the unsupported first stretches the same four
  calls again (the walks one call per distinct gap: the bound d - gap is an argument of the call).  Two figures: the time spent inside the library's calls alone, and the whole step with the numpy / Python glue between them
  (index building, pair hashes, scoring).  The first is the floor of any host composition; a JNI caller pays its own glue instead.
Each figure is the best of 3 after one warm-up.  The composition must agree with the new call on every sequence (outcome, winner, length)
before anything is timed; otherwise the tool stops and writes no file.
The figures, their ratios and rb_build_id() go to the output file; no figure is promised in advance."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np

K, D, FLOOR = 25, 100, 1.0
ACGT = b"ACGT"


class Clock:
    """seconds spent inside the library's calls"""

    def __init__(self): self.t = 0.0

    def __call__(self, fn, *a, **kw):
        t0 = time.perf_counter(); out = fn(*a, **kw); self.t += time.perf_counter() - t0
        return out


def pair_hashes(lf, lr, rf, rr, stranded):
    from rnabloom.graphutils import _combine
    p = _combine(lf, rf)
    if not stranded:
        q = _combine(rr, lr)
        p = np.where(q.view(np.int64) < p.view(np.int64), q, p)
    return p


def median(c):
    c = np.sort(c); n = c.size
    return np.float32(np.float32(c[n // 2] + c[n // 2 - 1]) / np.float32(2)) if n % 2 == 0 else c[n // 2]


def count_pairs(g, T, owner, ef, er, eko, tf, tr, tko):
    """countKmerPairsSE (gap 0) for many extensions in one look-up: extension x belongs to sequence owner[x], its k-mers are
    e*[eko[x]:eko[x + 1]], the sequence's last min(n, d) k-mers t*[tko[i]:tko[i + 1]] -> (pairs[x], last[x])"""
    xs, js, ts = [], [], []
    for x in range(owner.size):
        i = owner[x]
        nt = int(tko[i + 1] - tko[i]); m = int(eko[x + 1] - eko[x])
        j = np.arange(min(D, m))
        t = nt - D + j
        ok = (t >= 0) & (t < nt)
        xs.append(np.full(int(ok.sum()), x)); js.append(j[ok]); ts.append(t[ok] + int(tko[i]))
    xs, js, ts = (np.concatenate(a) if a else np.zeros(0, np.int64) for a in (xs, js, ts))
    ei = eko[xs] + js
    hit = T(g.lookupReadKmerPair, pair_hashes(tf[ts], tr[ts], ef[ei], er[ei], g.stranded)) if xs.size else np.zeros(0, bool)
    pairs = np.bincount(xs[hit], minlength=owner.size)
    last = np.full(owner.size, -1, np.int64)
    np.maximum.at(last, xs[hit], js[hit])
    return pairs, last


def composed(g, seqs, T):
    """-> (outcome, winner, out_len) per sequence, 0 NONE 1 SINGLE 2 FIRST 3 SECOND as rb_extend_rec"""
    n = len(seqs)
    tails = [s[-(D + K - 1):] for s in seqs]
    tko, tf, tr, tc = T(g.getKmers, tails)
    li = tko[1:] - 1
    f4, r4, c4 = T(g.getNeighbors, tf[li], tr[li], np.array([t[-K] for t in tails], np.uint8), 0)
    si, bi = np.nonzero(c4 >= np.float32(1))
    ncand = np.bincount(si, minlength=n)
    seeds = [tails[i][-(K - 1):] + ACGT[b:b + 1] for i, b in zip(si, bi)]
    app, _ = T(g.naiveExtend, seeds, 0, 2, D - 2, FLOOR)
    ext = [s + a for s, a in zip(seeds, app)]
    eko, ef, er, ec = T(g.getKmers, ext)
    elen = np.diff(eko)
    outcome = np.zeros(n, np.int32); winner = np.full(n, -1, np.int32); out_len = np.zeros(n, np.int32)
    one = ncand[si] == 1
    outcome[si[one]] = 1; winner[si[one]] = bi[one]; out_len[si[one]] = elen[one]
    many = np.nonzero(~one)[0]
    # the look-ups of the forked sequences' candidates only (a single candidate is returned unscored)
    sub_ko = np.zeros(many.size + 1, np.int64); np.cumsum(elen[many], out=sub_ko[1:])
    idx = np.concatenate([np.arange(eko[x], eko[x + 1]) for x in many]) if many.size else np.zeros(0, np.int64)
    pairs, last = count_pairs(g, T, si[many], ef[idx], er[idx], sub_ko, tf, tr, tko)
    path_min = np.array([tc[tko[i]:tko[i + 1]].min() for i in range(n)], np.float32)
    offers = []                                                           # (sequence, first base, second base or -1, median, pairs, last, outcome)
    offer = lambda i, cov, p, l, oc, w: offers.append((int(i), int(w) & 3, int(w) >> 4 if oc == 3 else -1, cov, int(p), int(l), oc, int(w)))
    second = []
    for y, x in enumerate(many):
        if pairs[y] > 0:
            offer(si[x], median(ec[eko[x]:eko[x + 1]]), pairs[y], last[y], 2, bi[x])
        elif elen[x] < D - 1:
            second.append(x)
    if second:
        second = np.array(second)
        lk = eko[second + 1] - 1
        g4, _, d4 = T(g.getNeighbors, ef[lk], er[lk], np.array([ext[x][-K] for x in second], np.uint8), 0)
        xi, b2 = np.nonzero(d4 >= np.float32(1))
        px = second[xi]                                                   # the first stretch each second-level walk continues
        seeds2 = [ext[x][-(K - 1):] + ACGT[b:b + 1] for x, b in zip(px, b2)]
        app2 = [None] * px.size                                           # the call takes one bound: a call per distinct gap, bound d - gap
        for gap in np.unique(elen[px]):
            at = np.nonzero(elen[px] == gap)[0]
            got, _ = T(g.naiveExtend, [seeds2[y] for y in at], 0, 2, D - int(gap), FLOOR)
            for y, a in zip(at, got):
                app2[y] = a
        ext2 = [ext[x] + ACGT[b:b + 1] + a for x, b, a in zip(px, b2, app2)]
        ko2, f2, r2, c2 = T(g.getKmers, ext2)
        pairs2, last2 = count_pairs(g, T, si[px], f2, r2, ko2, tf, tr, tko)
        for y in range(px.size):
            if pairs2[y] > 0:
                offer(si[px[y]], median(c2[ko2[y]:ko2[y + 1]]), pairs2[y], last2[y], 3, bi[px[y]] | (b2[y] << 4))
    best = {}                                                             # sequence -> (score, median); offers compete in the reference's order
    for i, _, _, cov, p, l, oc, w in sorted(offers, key=lambda o: o[:3]):
        score = np.float32(np.float32(min(path_min[i], cov) * np.float32(p)) / np.float32(l + 1))
        b = best.get(i, (np.float32(0), np.float32(0)))
        if score > b[0] or (score == b[0] and cov > b[1]):
            best[i] = (score, cov)
            outcome[i], winner[i], out_len[i] = oc, w, l + 1
    return outcome, winner, out_len


def main(n_seq, out_path):
    import torch
    import test_extend_step_rules as R
    from rnabloom import _native as N
    from rnabloom.graph import BloomFilterDeBruijnGraph, _pack
    w = R.World(K, False, seed=900, d=D, n_iso=12, read_len=250, tile=25, tx_len=900)
    g = BloomFilterDeBruijnGraph(*w.sizes, 2, 2, 2, K, False, True, rngSeed=5)
    g.setReadPairedKmerDistance(D)
    g.addReads(*w.packed, 3, storeReadPairedKmers=True)
    at_fork = ("fork-0", "fork-short-0", "fork-one-kmer", "fork2", "fork2-short", "fork2-one-kmer")   # long, 7 k-mers, one k-mer
    pool = [s for kind, s, dd in w.queries if dd == 0 and kind in at_fork]
    seqs = [pool[i % len(pool)] for i in range(n_seq)]
    seq, off = _pack(seqs)
    new = lambda: g.extendStepSEFlat(seq, off, 0, FLOOR)
    bases, recs, _ = new()
    oc, wn, ln = composed(g, seqs, Clock())
    same = int(((oc == recs["outcome"]) & (wn == recs["winner"]) & (ln == recs["out_len"])).sum())
    if same != n_seq:
        raise SystemExit("extend step: the composition agrees with rb_graph_extend_se on %d of %d sequences only — nothing is timed" % (same, n_seq))
    tally = np.bincount(recs["outcome"], minlength=4)
    lines = ["build %s" % N.lib.rb_build_id().decode(),
             "extend step: %d sequences ending at forks, k = %d, d = %d, floor %g: none %d, single %d, first %d, second %d; the composition "
             "agrees on all %d (outcome, winner, length)" % (n_seq, K, D, FLOOR, *tally, same),
             "composed: one call a stage over all sequences; the second-level walks take one rb_graph_naive_extend call per distinct gap (its "
             "bound is per call), which favours the composition on this input (%d distinct sequences)" % len(pool)]
    ts = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter(); new(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    g.profileEnable(True); g.profileGet(reset=True)
    ks = []
    for _ in range(3):
        new(); ks.append(g.profileGet(reset=True)["extend_se"][0] / 1e3)
    g.profileEnable(False)
    cs, ws = [], []
    for _ in range(3):
        T = Clock(); torch.cuda.synchronize(); t0 = time.perf_counter(); composed(g, seqs, T); torch.cuda.synchronize()
        ws.append(time.perf_counter() - t0); cs.append(T.t)
    t_new, t_k, t_calls, t_all = min(ts), min(ks), min(cs), min(ws)
    for what, dt in (("rb_graph_extend_se (kernels)", t_k), ("rb_graph_extend_se (end to end)", t_new),
                     ("composed (inside the library's calls)", t_calls), ("composed (with the host glue)", t_all)):
        lines.append("extend step %-40s %9.2f ms = %8.3f M sequences/s" % (what, dt * 1e3, n_seq / dt / 1e6))
    lines.append("extend step ratio composed calls / new call end to end: %.2f" % (t_calls / t_new))
    lines.append("extend step ratio composed with glue / new call end to end: %.2f" % (t_all / t_new))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    g.destroy()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20_000,
         sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "extend_step_bench.txt"))
