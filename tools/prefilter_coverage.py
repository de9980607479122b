"""Coverage of the prefilter's hot-k-mer cache on the input of tests/test_gpu_prefilter.py: of the distinct k-mers whose oracle counter
exponent is >= 1 after two passes over 2600 uniform 150-base reads (G = 4000), how many have an entry in the table an insert uses.  A
measurement of this code for later changes to be compared with, not a bound (tests assert none).  Usage: prefilter_coverage.py OUT.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rna-bloom_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import prefilter_ref as P          # noqa: E402
import test_gpu_prefilter as T     # noqa: E402


def coverage(k, geometry):
    from oracle import rbo
    from rnabloom.graph import BloomFilterDeBruijnGraph
    with T.env():                                    # (clears the switches, asks for the smallest tables)
        if geometry == "default":
            os.environ.pop("RB_MPF"); os.environ.pop("RB_NPF")
        og = rbo.Graph(*T.SIZES, 2, 2, 2, k, False, False, T.SEED)
        gg = BloomFilterDeBruijnGraph(*T.SIZES, 2, 2, 2, k, False, False, rngSeed=T.SEED, maxBatchKmers=15_000)
        r = T.reads_of("uniform", k)
        for _ in range(2):
            og.add_reads(r.seq, r.qual, r.off, 3, 0)
            st = gg.addReads(r.seq, r.qual, r.off, 3)
        tab, lg, m = T.cache_export(gg, P.MPF)
    ent = P.decode_mpf(tab, lg)
    known = P.Known(2).add(T.windows_of("uniform", k, False))
    filt = P.OracleFilters(og, T.SIZES[0], T.SIZES[1], 2, 2)
    P.check_entries(ent, known, filt)
    hot = P.cache_exp(filt.minimum(known.rows)) >= 1
    have = np.isin(known.h0, ent.h0)
    return lg, m, int(hot.sum()), int((hot & have).sum()), len(ent), ent.n_slots, st.sorted_kmers, st.kmers


def main(out):
    from rnabloom import _native as N
    lines = ["prefilter cache coverage (tools/prefilter_coverage.py), build id %s" % N.lib.rb_build_id().decode(),
             "input: synth.generate_pairs(2600, G=4000, L=150, err=0.002, n_rate=1e-3, seed=91, uniform_expr=True), left reads, inserted twice, sub-batches of 15 000 records",
             "filters: dbgbf %d bits, cbf %d bytes, 2 hashes each; canonical hashing; minimizer-bucketed table" % T.SIZES[:2],
             "geometry  k   log2(buckets) m   k-mers at exponent >= 1   with an entry   coverage   slots used / slots   second pass: sorted / windows"]
    for geometry in ("smallest", "default"):
        for k in (17, 25, 35, 63):
            lg, m, hot, cov, used, slots, srt, tot = coverage(k, geometry)
            lines.append("%-9s %-3d %-13d %-3d %-25d %-15d %-10.4f %d / %-12d %d / %d" % (geometry, k, lg, m, hot, cov, cov / max(hot, 1), used, slots, srt, tot))
    text = "\n".join(lines) + "\n"
    with open(out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main(sys.argv[1])
