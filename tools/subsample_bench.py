#!/usr/bin/env python3
"""Subsampling of long reads (rb_subsample_reads: the accept / reject loop of SeqSubsampler.strobemerBased on the device) timed on synthetic reads,
beside the composed route — the same loop over rb_strobemers, getCount and increment per read — in the same process.
    python tools/subsample_bench.py [reads=20000] [composed_prefix=1500] [out=profiles/subsample_bench.txt]
Input: corrected long reads of 1 800 - 2 200 letters (a whole transcript where it is shorter) drawn from 1 000 transcripts of 1 000 - 4 000 letters —
each letter of a transcript lies under about 14 reads, so with depth 3 most later reads are redundant — with 0.3 % substitutions, sorted by length, longest first, as RNABloom.main hands them over (R/RNABloom.java:7367); the worker's defaults
-lrsub 3,s,11,50: depth 3, strobemers of k = 11, wMin 12, wMax 61, two hash functions, a filter of 512 M counters.
Figures, one run each after a warm-up on a small input: the walker kernel (the call's own event time, summed over its launches) for both workgroup
sizes that were tried (RB_SUB_TPB), the route end to end (host reads in, kept indices out, the filter made and its FPR taken), the kept
fraction, and the walker's microseconds per kept and per dropped read — a least-squares fit of the walker time of calls of 500 reads to their
numbers of kept and dropped reads.  The composed route is slow (half a millisecond a read), so it runs on a prefix of the input — the longest reads — and the device route on the same
prefix beside it: kept lists and FPR must be equal, or the tool fails.  Nothing here is a criterion; occupancy and the walker's share of an idle device are not measured."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd")):
    sys.path.insert(0, p)

import numpy as np

K, INDEL, DEPTH, NUM_HASH, CLIP, BF_SIZE, N_TX = 11, 50, 3, 2, 0, 512 << 20, 1000
ACGT = np.frombuffer(b"ACGT", np.uint8)


def make_reads(n_reads, rng):
    tx = [ACGT[rng.integers(0, 4, int(n), dtype=np.uint8)] for n in rng.integers(1000, 4001, N_TX)]
    reads = []
    for _ in range(n_reads):
        t = tx[int(rng.integers(0, len(tx)))]
        ln = min(t.size, int(rng.integers(1800, 2201)))
        a = int(rng.integers(0, t.size - ln + 1))
        r = t[a:a + ln].copy()
        bad = rng.integers(0, ln, rng.binomial(ln, 0.003))
        r[bad] = ACGT[rng.integers(0, 4, bad.size)]
        reads.append(r.tobytes())
    reads.sort(key=len, reverse=True)
    return reads


def device_walk(reads, piece_reads):
    """the steps of subsampler.strobemerBased with the call's totals kept: (kept indices, [(kept, dropped, walker ns) per call])"""
    from rnabloom import subsampler
    from rnabloom.bloom import CountingBloomFilter
    cbf = CountingBloomFilter(BF_SIZE, NUM_HASH, K, device=0)
    order = subsampler.visiting_order(len(reads))
    seqs = [reads[i] for i in order]
    p = subsampler.strobemer_params(K, DEPTH, CLIP, INDEL)
    calls, kept = [], []
    for a in range(0, len(seqs), piece_reads):
        keep, _, t = subsampler.subsample_reads(cbf, p, seqs[a:a + piece_reads])
        calls.append((int(t[0]), keep.size - int(t[0]), int(t[3])))
        kept += [order[a + j] for j in np.flatnonzero(keep)]
    cbf.destroy()
    return kept, np.array(calls, np.float64)


def main(n_reads, prefix, out_path):
    import torch
    from rnabloom import _native as N
    from rnabloom import subsampler
    rng = np.random.default_rng(7355)
    reads = make_reads(n_reads, rng)
    letters = sum(len(r) for r in reads)
    args = (BF_SIZE, K, NUM_HASH, True, DEPTH, CLIP, INDEL)
    subsampler.strobemerBased(reads[:64], *args)                                  # warm-up: the library's first launches
    lines = ["build %s" % N.lib.rb_build_id().decode(), "one run, nothing tuned",
             "subsample: %d reads (%d letters) of %d transcripts, longest first; strobemers k = %d, wMin %d, wMax %d, depth %d, %d hash functions, "
             "%d M counters, maxEdgeClip %d" % (n_reads, letters, N_TX, K, K + 1, K + max(K, INDEL), DEPTH, NUM_HASH, BF_SIZE >> 20, CLIP)]
    walk = {}
    for tpb in (256, 1024):
        os.environ["RB_SUB_TPB"] = str(tpb)
        kept, calls = device_walk(reads, 500)
        walk[tpb] = (kept, calls)
        ns = calls[:, 2].sum()
        fit = np.linalg.lstsq(calls[:, :2], calls[:, 2], rcond=None)[0] / 1e3
        lines.append("subsample walker, workgroup of %4d: %9.2f ms in %d calls of 500 reads = %8.3f M reads/s; kept %d of %d (%.3f); fit: %.2f us per kept read, "
                     "%.2f us per dropped read" % (tpb, ns / 1e6, len(calls), n_reads / ns * 1e3, len(kept), n_reads, len(kept) / n_reads, fit[0], fit[1]))
    assert walk[256][0] == walk[1024][0], "the two workgroup sizes disagree"
    del os.environ["RB_SUB_TPB"]
    torch.cuda.synchronize(); t0 = time.perf_counter()
    kept, fpr = subsampler.strobemerBased(reads, *args)
    t_dev = time.perf_counter() - t0
    assert kept == walk[256][0]
    lines.append("subsample strobemerBased end to end (one call of the library per %d reads): %9.2f ms = %8.3f M reads/s; FPR %.3g"
                 % (subsampler.PIECE_READS, 1e3 * t_dev, n_reads / t_dev / 1e6, fpr))
    part = reads[:prefix]
    t0 = time.perf_counter(); kept_c, fpr_c = subsampler.strobemerBasedComposed(part, *args); t_comp = time.perf_counter() - t0
    t0 = time.perf_counter(); kept_d, fpr_d = subsampler.strobemerBased(part, *args); t_part = time.perf_counter() - t0
    equal = kept_c == kept_d and fpr_c == fpr_d
    lines += ["subsample composed route (rb_strobemers + getCount + increment per read) on the first %d reads: %9.2f ms = %8.4f M reads/s; kept %d"
              % (len(part), 1e3 * t_comp, len(part) / t_comp / 1e6, len(kept_c)),
              "subsample strobemerBased on the same %d reads: %9.2f ms = %8.4f M reads/s; kept %d; results %s; composed / device = %.1f"
              % (len(part), 1e3 * t_part, len(part) / t_part / 1e6, len(kept_d), "equal" if equal else "DIFFERENT", t_comp / t_part),
              "occupancy and the walker's share of an idle device (one workgroup on one compute unit): not measured"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    assert equal, "the two routes disagree"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20_000, int(sys.argv[2]) if len(sys.argv) > 2 else 1500,
         sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "subsample_bench.txt"))
