"""The rules of rb_graph_correct_long restated in Python from the reference's Java, statement by statement over lists of k-mers, and checked
on hand-worked cases over a dictionary graph.  tests/test_gpu_long_correction.py applies the same restatement to the CPU oracle's filters.

  GraphUtils.correctLongSequenceWindowed (R/util/GraphUtils.java:3087-3185), getCoverageStats :1799-1848, correctInternalErrors :3402-3602,
  trimLowCoverageEdgeKmers :3187-3241, getMedianKmerCoverage :208-247; getMaxCoveragePath :1591-1675 and getPercentIdentity are
  tests/test_error_correction_rules.py's, the median and getAltNucleotides tests/test_mismatch_rules.py's.
A k-mer is the pair (its letters, its count); a list is a Python list of them — NOT a text: that every list the reference builds spells a text
whose getKmers list it is (what the device relies on) is not assumed here, so the comparison on the GPU tests it.
The graph is an object with counts(sequence) -> getKmers' counts, variants(k-mer, 0, "L") -> the counts of the four k-mers with A C G T in place of
its first letter, max_cov_path(left, right, bound, min_cov) -> k-mers or None.  The record keeps the branch counters of rb_long_rec.
The last part of the file checks that the feature exists at every layer."""
import os
import re

import numpy as np
import pytest

from test_error_correction_rules import FLOAT_MIN_VALUE, EGraph, percent_identity
from test_mismatch_rules import K, NORM, TRUE, alt_nucleotides, median, sub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NULL, UNCHANGED, CHANGED, NO_KMER = 0, 1, 2, 3
OVERFLOW, TRIMMED_TO_NOTHING = 1, 2
CTRS = ("snv_replaced", "snv_kept", "path_none", "zero_accepted", "zero_kept", "accepted_10x", "accepted_identity", "cov_kept", "short_skipped",
        "anchor_moved")
FIELDS = ("status", "passes", "out_len", "trim_begin", "trim_end") + CTRS + ("flags",)
DEFAULTS = dict(maxItr=2, maxCovGradient=0.5, lookahead=5, maxIndelSize=1, percentIdentity=0.9, minKmerCov=1, minNumSolidKmers=0,
                trimLowCovEdges=False, windowSize=500)


def get_kmers(seq, k, G):
    c = G.counts(seq)
    return [(bytes(seq[i:i + k]), F32(c[i])) for i in range(len(c))]


def assemble(kmers):
    return kmers[0][0] + b"".join(km[0][-1:] for km in kmers[1:]) if kmers else b""


def coverage_stats(counts, max_cov_gradient, lookahead):
    """getCoverageStats(kmers, maxCovGradient, lookahead, true) :1799-1848 -> (median, dropoff)"""
    covs = sorted(F32(c) for c in counts)
    n = len(covs)
    half = n // 2
    med = F32(F32(covs[half - 1] + covs[half]) / F32(2.0)) if n % 2 == 0 else covs[half]
    dropoff = F32(0)
    if n >= lookahead:
        last = covs[n - lookahead]
        for i in range(n - lookahead - 1, -1, -1):
            c = covs[i]
            if c < F32(last * F32(max_cov_gradient)):
                dropoff = last
                break
            last = c
    return med, dropoff


def windows(num_kmers, window_size, to_shift):
    """:3124-3135: the [i, end) of a pass"""
    shift, out, end, i = window_size // 2, [], 0, 0
    while i < num_kmers:
        end = min(i + shift + window_size, num_kmers) if i == 0 and to_shift else min(i + window_size, num_kmers)
        if end + shift >= num_kmers:
            end = num_kmers
        out.append((i, end))
        i = end
    return out


def correct_internal_errors(kmers, k, G, lookahead, max_indel, T, pid, min_cov, ctr):
    """:3402-3602 -> kmers2 or None.  ctr: the record's counters, added to."""
    corrected, n, expected = False, len(kmers), k - 1
    kmers2, nbad, zero = [], 0, False
    i = 0
    while i < n:                                                        # for (int i=0; i<numKmers; ++i), with its continue and its cursor jump
        kmer = kmers[i]
        if kmer[1] >= T:
            if nbad > 0:
                fill = lambda: kmers2.extend(kmers[i - nbad:i])
                if not kmers2:
                    kmers2.extend(kmers[:i])
                elif nbad == expected:                                  # a SNV bubble
                    left_edge, right_edge = kmers[i - nbad], kmers[i - 1]
                    prefix = left_edge[0][:k - 1]
                    best, best_cov = None, FLOAT_MIN_VALUE
                    vc = G.variants(right_edge[0], 0, "L")              # getLeftVariants(k, numHash, graph, minKmerCov)
                    for a in alt_nucleotides(right_edge[0][0]):
                        if F32(vc[b"ACGT".index(a)]) >= min_cov:
                            test = get_kmers(prefix + bytes([a]) + right_edge[0][1:], k, G)
                            if test:
                                cs = [c for _, c in test]
                                if min(cs) >= min_cov and median(cs) > best_cov:
                                    best_cov, best = median(cs), test
                    if best is not None and best_cov >= min_cov:
                        kmers2.extend(best)
                        corrected = True
                        ctr["snv_replaced"] += 1
                    else:
                        fill()
                        ctr["snv_kept"] += 1
                elif nbad < expected - max_indel:
                    nbad += 1
                    ctr["short_skipped"] += 1
                    i += 1
                    continue
                else:
                    mld = max_indel if pid < F32(1.0) else 0
                    size2 = len(kmers2)
                    bl = size2 - 1
                    stop = max(0, bl - lookahead)
                    best_left = kmers2[bl]
                    for j in range(size2 - 3, stop - 1, -1):           # bestLeftKmerIndex-2: index size - 2 is never looked at
                        if kmers2[j][1] > best_left[1]:
                            best_left, bl = kmers2[j], j
                    br = i
                    best_right = kmer
                    for j in range(i + 1, min(i + lookahead, n - 1) + 1):
                        if kmers[j][1] > best_right[1]:
                            best_right, br = kmers[j], j
                    if bl != size2 - 1 or br != i:
                        ctr["anchor_moved"] += 1
                    path = G.max_cov_path(best_left[0].translate(NORM), best_right[0].translate(NORM), nbad + mld, min_cov)
                    accept = False
                    if not path:                                        # null or empty
                        ctr["path_none"] += 1
                    else:
                        alt = [(bytes(p), F32(G.counts(bytes(p))[0])) for p in path]
                        left_adjust, right_adjust = size2 - 1 - bl, br - i
                        ori_len = nbad + left_adjust + right_adjust
                        len_ok = abs(ori_len - len(alt)) <= mld
                        if zero:
                            accept = len_ok
                            ctr["zero_accepted" if accept else "zero_kept"] += 1
                        else:
                            alt_cov = median([c for _, c in alt])
                            ori_cov = median([c for _, c in kmers[i - nbad:i]])
                            if F32(2 * ori_cov) <= alt_cov and len_ok:
                                if ori_cov < min_cov and alt_cov >= F32(10 * ori_cov):
                                    accept = True
                                    ctr["accepted_10x"] += 1
                                elif i - nbad - left_adjust >= 0:       # (a negative index: the reference throws; the run is kept)
                                    if percent_identity(assemble(alt), assemble(kmers[i - nbad - left_adjust:i + right_adjust])) >= pid:
                                        accept = True
                                        ctr["accepted_identity"] += 1
                            if not accept:
                                ctr["cov_kept"] += 1
                    if accept:
                        del kmers2[bl + 1:]
                        kmers2.extend(alt)
                        i, kmer = br, best_right
                        corrected = True
                    else:
                        fill()
                nbad, zero = 0, False
            kmers2.append(kmer)
        else:
            nbad += 1
            if kmer[1] == 0:
                zero = True
        i += 1
    if 0 < nbad < n:
        kmers2.extend(kmers[n - nbad:])
    return kmers2 if corrected else None


def trim_low_coverage_edge_kmers(kmers, threshold):
    """:3187-3241 -> (list or None, headIndex, tailIndex)"""
    n = len(kmers)
    head, tail, prev_good = 0, n, False
    for i in range(n):
        if kmers[i][1] >= threshold:
            if prev_good:
                head = i
                break
            prev_good = True
        else:
            prev_good = False
    prev_good = False
    for i in range(n - 1, head, -1):
        if kmers[i][1] >= threshold:
            if prev_good:
                tail = i + 2
                break
            prev_good = True
        else:
            prev_good = False
    if head > 0 or tail < n:
        return (kmers[head:tail] if tail - head > 1 else []), head, tail
    return None, head, tail


def correct_long(seq, k, G, **params):
    """correctLongSequenceWindowed on getKmers(seq) -> (the text the returned list spells, or None for null; the record as a dict)"""
    P = dict(DEFAULTS, **params)
    assert set(P) == set(DEFAULTS)
    seq = bytes(seq)
    rec = dict.fromkeys(FIELDS, 0)
    rec["trim_begin"] = rec["trim_end"] = -1
    kmers = get_kmers(seq, k, G)
    if not kmers:
        rec.update(status=NO_KMER, out_len=len(seq))
        return None, rec
    min_cov, pid = F32(P["minKmerCov"]), F32(P["percentIdentity"])
    needed = P["minNumSolidKmers"]
    if needed > 0:
        for km in kmers:
            if km[1] >= min_cov:
                needed -= 1
                if needed <= 0:
                    break
    if needed > 0:
        rec.update(status=NULL, out_len=len(seq))
        return None, rec
    test, to_shift = kmers, False
    for _ in range(P["maxItr"]):
        corrected, out = False, []
        for a, e in windows(len(test), P["windowSize"], to_shift):
            window, wc = test[a:e], None
            if e - a >= P["lookahead"]:
                med, dropoff = coverage_stats([c for _, c in window], P["maxCovGradient"], P["lookahead"])
                T = max(dropoff, min_cov) if dropoff > 0 else med
                wc = correct_internal_errors(window, k, G, P["lookahead"], P["maxIndelSize"], T, pid, min_cov, rec)
            if wc is None:
                out.extend(window)
            else:
                corrected = True
                out.extend(wc)
        if not corrected:
            break
        test, to_shift = out, not to_shift
        rec["passes"] += 1
    trimmed = False
    if P["trimLowCovEdges"] and median([c for _, c in test]) >= F32(P["minKmerCov"] * 2):
        t, head, tail = trim_low_coverage_edge_kmers(test, min_cov)
        if t is not None:
            test, trimmed = t, True
            rec.update(trim_begin=head, trim_end=tail)
            if not t:
                rec["flags"] |= TRIMMED_TO_NOTHING
    text = assemble(test)
    rec.update(status=CHANGED if rec["passes"] or trimmed else UNCHANGED, out_len=len(text))
    return text, rec


def assemble_valid_kmers(seq, k, G):
    """assembleValidKmers :3626-3654 of getKmers(seq)"""
    kmers, segs, start, end = get_kmers(seq, k, G), [], -1, -1
    for i, (km, c) in enumerate(kmers):
        if c > 0 or all(ch in b"ACGTUacgtu" for ch in km):
            if start < 0:
                start = i
            end = i
        elif start >= 0:
            segs.append(assemble(kmers[start:end + 1]))
            start = end = -1
    if start >= 0 and end == len(kmers) - 1:
        segs.append(assemble(kmers[start:]))
    return segs


# ---- hand-worked cases over the dictionary graph (k = 5).  TRUE is a 28-letter transcript whose 24 k-mers are all different.
def run(g, seq, **params):
    return correct_long(seq, K, g, **dict(dict(lookahead=2, windowSize=100, maxItr=1), **params))


def counters(rec):
    return {c: rec[c] for c in CTRS if rec[c]}


def test_coverage_stats_median_and_dropoff():
    # an even number of counts: the float32 mean of the middle two; no drop by half or more on the way down from sorted[len - lookahead]: no dropoff
    assert coverage_stats([10, 12, 9, 11], 0.5, 2) == (F32(10.5), F32(0))
    # sorted 1 1 10 12: the walk starts at sorted[4 - 2] = 10 and meets 1 < 10 * 0.5: dropoff 10 (the LAST value above the cliff)
    assert coverage_stats([12, 1, 10, 1], 0.5, 2) == (F32(5.5), F32(10))
    # the walk starts BELOW the cliff with lookahead 3 (sorted[1] = 1): nothing further down drops: no dropoff although the counts have a cliff
    assert coverage_stats([12, 1, 10, 1], 0.5, 3) == (F32(5.5), F32(0))
    # a gradient above 1 finds a "drop" between equal counts
    assert coverage_stats([4, 4, 4], 1.5, 1) == (F32(4), F32(4))
    # fewer counts than lookahead: no dropoff
    assert coverage_stats([1, 100], 0.5, 3) == (F32(50.5), F32(0))


def test_window_cuts():
    # no shift: windows of 10; the rest of 4 <= shift = 5 is merged into the last window (end + shift >= nk)
    assert windows(34, 10, False) == [(0, 10), (10, 20), (20, 34)]
    assert windows(36, 10, False) == [(0, 10), (10, 20), (20, 30), (30, 36)]
    # a shifted pass: the first window is shift longer
    assert windows(36, 10, True) == [(0, 15), (15, 25), (25, 36)]
    assert windows(12, 10, True) == [(0, 12)] and windows(10, 10, False) == [(0, 10)] and windows(0, 10, False) == []
    # window 1: shift 0, every k-mer its own window
    assert windows(3, 1, False) == [(0, 1), (1, 2), (2, 3)]


def test_substitution_with_absent_kmers_is_a_zero_coverage_path():
    g = EGraph([(TRUE, 10)])
    bad = sub(TRUE, 12, "T")                                             # k-mers 8 .. 12 hold the error: a run of k = 5, not an SNV bubble (k - 1)
    # counts 10 x 8, 0 x 5, 10 x 11: sorted[24 - 2] = 10, the walk down meets 0 < 5: dropoff 10, T = 10.  The run has count 0: only the lengths
    # are compared — the path from k-mer 7 to k-mer 13 has 5 k-mers for 5: accepted, the text is the transcript's again
    text, rec = run(g, bad)
    assert text == TRUE and rec["status"] == CHANGED and rec["passes"] == 1 and counters(rec) == dict(zero_accepted=1)
    assert rec["out_len"] == len(TRUE) and (rec["trim_begin"], rec["trim_end"], rec["flags"]) == (-1, -1, 0)
    # no pass: nothing happens
    text, rec = run(g, bad, maxItr=0)
    assert text == bad and rec["status"] == UNCHANGED and rec["passes"] == 0 and counters(rec) == {}


def test_deletion_is_an_snv_bubble_that_grows_by_one_letter():
    g = EGraph([(TRUE, 10)])
    dele = TRUE[:12] + TRUE[13:]                                         # the 4 = k - 1 k-mers over the junction are absent
    assert [int(c) for c in g.counts(dele)[7:13]] == [10, 0, 0, 0, 0, 10]
    # prefix = the first bad k-mer's 4 letters, var = a letter + the last bad k-mer's last 4: the deleted letter gives the transcript's 5 k-mers,
    # which stand for the 4 bad ones
    text, rec = run(g, dele)
    assert text == TRUE and len(text) == len(dele) + 1 and counters(rec) == dict(snv_replaced=1) and rec["status"] == CHANGED
    # two letters deleted: again 4 k-mers over the junction, but no single letter mends it: kept
    dele2 = TRUE[:12] + TRUE[14:]
    text, rec = run(g, dele2)
    assert text == dele2 and counters(rec) == dict(snv_kept=1) and rec["status"] == UNCHANGED and rec["passes"] == 0
    # the transcript's k-mers 8 .. 12 (the candidate's windows) below min_kmer_cov: no variant counts
    g2 = EGraph([(TRUE, 10)], extra={TRUE[i:i + K]: 2 for i in range(8, 13)})
    assert counters(run(g2, dele, minKmerCov=3)[1]) == dict(snv_kept=1) and counters(run(g2, dele, minKmerCov=2)[1]) == dict(snv_replaced=1)


def test_insertion_is_kept_for_its_length():
    g = EGraph([(TRUE, 10)])
    ins = TRUE[:12] + b"TT" + TRUE[12:]                                  # 6 k-mers over the insertion, the path between the anchors has 4
    assert [int(c) for c in g.counts(ins)[7:15]] == [10, 0, 0, 0, 0, 0, 0, 10]
    text, rec = run(g, ins, maxIndelSize=1)
    assert text == ins and counters(rec) == dict(zero_kept=1)
    text, rec = run(g, ins, maxIndelSize=2)                              # |6 - 4| <= 2
    assert text == TRUE and counters(rec) == dict(zero_accepted=1)
    # percent_identity 1.0 switches the length tolerance off
    assert counters(run(g, ins, maxIndelSize=2, percentIdentity=1.0)[1]) == dict(zero_kept=1)


def test_short_run_swallows_the_good_kmer_behind_it():
    # k-mers 8 and 9 thin (1 < T), k-mer 10 good, k-mers 11 .. 13 thin: with max_indel_size 1 a run of 2 < k - 1 - 1 is not closed: k-mer 10 is
    # counted as bad (:3468-3471) and the run goes on to 6 k-mers; all of them have a count above 0 and the path of 6 true k-mers is as
    # covered as they are (2 * 1 <= 1 fails): kept.  Whatever is kept is copied, k-mer 10 included: the text is unchanged.
    thin = {TRUE[i:i + K]: 1 for i in (8, 9, 11, 12, 13)}
    g = EGraph([(TRUE, 10)], extra=thin)
    text, rec = run(g, TRUE)
    assert text == TRUE and counters(rec) == dict(short_skipped=1, cov_kept=1) and rec["status"] == UNCHANGED
    # k-mer 9 alone thin, max_indel_size 0: runs of 1, 2 and 3 are < k - 1 = 4, so the good k-mers 10, 11 and 12 are swallowed one after the
    # other; at k-mer 13 the run has 4 = k - 1 k-mers and is taken for an SNV bubble, which no letter mends: kept
    g = EGraph([(TRUE, 10)], extra={TRUE[9:9 + K]: 1})
    text, rec = run(g, TRUE, maxIndelSize=0)
    assert text == TRUE and counters(rec) == dict(short_skipped=3, snv_kept=1)


def test_ten_times_rule_against_identity():
    # the erroneous k-mers are known thinly (count 1): not zero coverage
    bad = sub(TRUE, 12, "T")
    thin = {bad[i:i + K]: 1 for i in range(8, 13)}
    g = EGraph([(TRUE, 10)], extra=thin)
    # min_kmer_cov 2: oriCov 1 < 2 and altCov 10 >= 10 * 1: accepted without looking at the letters
    text, rec = run(g, bad, minKmerCov=2)
    assert text == TRUE and counters(rec) == dict(accepted_10x=1)
    # min_kmer_cov 1: the identity decides: path + anchors' overlap, 9 letters with one substitution: 8/9 >= 0.8
    text, rec = run(g, bad, minKmerCov=1, percentIdentity=0.8)
    assert text == TRUE and counters(rec) == dict(accepted_identity=1)
    assert percent_identity(TRUE[8:17], bad[8:17]) == F32(F32(8) / F32(9))
    text, rec = run(g, bad, minKmerCov=1, percentIdentity=0.95)
    assert text == bad and counters(rec) == dict(cov_kept=1)
    # the original as covered as half the path: 2 * 6 > 10: kept before any other test
    g6 = EGraph([(TRUE, 10)], extra={km: 6 for km in thin})
    assert counters(run(g6, bad, minKmerCov=7)[1]) == dict(cov_kept=1)


def test_left_anchor_search_skips_the_entry_before_the_last():
    bad = sub(TRUE, 14, "T")                                             # k-mers 10 .. 14 bad; kmers2 = k-mers 0 .. 9 when the run ends
    # k-mer 8 (entry last - 1) is the best covered by far, k-mer 7 (last - 2) better than the last: the anchor moves to k-mer 7, never to 8
    g = EGraph([(TRUE, 10)], extra={TRUE[8:8 + K]: 40, TRUE[7:7 + K]: 20})
    # oriPathLen = 5 + leftAdjust 2: the path from k-mer 7 to k-mer 15 has 7 k-mers.  The bound is run + maxLengthDifference, whatever the anchors
    # do, and the walk needs one step more than the path has k-mers to arrive: with max_indel_size 1 (bound 6) there is no path
    text, rec = run(g, bad, lookahead=3, maxIndelSize=1)
    assert text == bad and counters(rec) == dict(anchor_moved=1, path_none=1)
    text, rec = run(g, bad, lookahead=3, maxIndelSize=3)
    assert text == TRUE and counters(rec) == dict(anchor_moved=1, zero_accepted=1)
    assert g.max_cov_path(TRUE[7:12], TRUE[15:20], 8, 1.0) == [TRUE[i:i + K] for i in range(8, 15)]
    # only entry last - 1 stands out: the anchor stays
    g = EGraph([(TRUE, 10)], extra={TRUE[8:8 + K]: 40})
    assert counters(run(g, bad, lookahead=3, maxIndelSize=3)[1]) == dict(zero_accepted=1)


def test_cursor_jumps_over_a_following_gap():
    # two substitutions 7 apart: runs 8 .. 12 and 15 .. 19 with good k-mers 13 and 14 between.  k-mer 20 is the best covered within lookahead 7 of
    # k-mer 13: the right anchor of the FIRST run is k-mer 20, the path spans both runs, the cursor moves behind the second: one event
    bad = sub(sub(TRUE, 12, "T"), 19, "A")
    g = EGraph([(TRUE, 10)], extra={TRUE[20:20 + K]: 30})
    assert [int(c) for c in g.counts(bad)[7:21]] == [10, 0, 0, 0, 0, 0, 10, 10, 0, 0, 0, 0, 0, 30]
    # (oriPathLen = 5 + rightAdjust 7 = 12 = the path's k-mers 8 .. 19; the bound 5 + max_indel_size has to reach 13)
    text, rec = run(g, bad, lookahead=7, maxIndelSize=8)
    assert text == TRUE and counters(rec) == dict(zero_accepted=1, anchor_moved=1)
    # with lookahead 2 the anchors stay and the runs are two events
    text, rec = run(g, bad, lookahead=2)
    assert text == TRUE and counters(rec) == dict(zero_accepted=2)


def test_path_none_and_leading_and_trailing_runs():
    g = EGraph([(TRUE, 10)])
    # a run at the window's start is copied, one at its end too: nothing to count
    s = sub(sub(TRUE, 1, "T"), 26, "A")
    text, rec = run(g, s)
    assert text == s and counters(rec) == {} and rec["status"] == UNCHANGED
    # a better covered branch behind the left anchor and another before the right anchor, both dead ends: either walk leaves the transcript
    bad = sub(TRUE, 12, "T")
    g = EGraph([(TRUE, 10)], extra={TRUE[8:12] + b"C": 50, b"C" + TRUE[13:17]: 50})
    assert g.max_cov_path(TRUE[7:12], TRUE[13:18], 6, 1.0) is None
    text, rec = run(g, bad)
    assert text == bad and counters(rec) == dict(path_none=1) and rec["status"] == UNCHANGED


def test_second_pass_corrects_what_the_first_exposed():
    g = EGraph([(TRUE, 10)])
    dele = TRUE[:12] + TRUE[13:]
    text, rec = run(g, dele, maxItr=5)
    assert text == TRUE and rec["passes"] == 1                           # the second pass corrects nothing and ends the loop
    # two windows: the error lies across the cut of the first pass (windows of 8 k-mers: [0, 8), [8, 16), [16, 24)): the run 8 .. 12 starts its
    # window and is copied.  Nothing is corrected, so there is no second pass.
    bad = sub(TRUE, 12, "T")
    assert windows(24, 8, False) == [(0, 8), (8, 16), (16, 24)]
    text, rec = run(g, bad, windowSize=8, maxItr=5)
    assert text == bad and rec["passes"] == 0 and rec["status"] == UNCHANGED
    # the error one letter on: the run 9 .. 13 is inside [8, 16): corrected in pass 1
    bad = sub(TRUE, 13, "G")
    text, rec = run(g, bad, windowSize=8, maxItr=5)
    assert text == TRUE and rec["passes"] == 1
    # two errors: the one at 13 is mended by pass 1 ([8, 16)), the one at 20 (run 16 .. 20) starts the window [16, 24) of pass 1 and is inside
    # the window [12, 24) of the shifted pass 2, which only runs because pass 1 corrected something
    assert windows(24, 8, True) == [(0, 12), (12, 24)]
    bad = sub(sub(TRUE, 13, "G"), 20, "C")
    text, rec = run(g, bad, windowSize=8, maxItr=1)
    assert text == sub(TRUE, 20, "C") and rec["passes"] == 1
    text, rec = run(g, bad, windowSize=8, maxItr=5)
    assert text == TRUE and rec["passes"] == 2 and rec["zero_accepted"] == 2


def test_edge_trim_outcomes():
    g = EGraph([(TRUE, 10)])
    # headIndex is the SECOND k-mer of the first good pair, tailIndex = i + 2 one behind the last good pair: a clean sequence loses its first k-mer
    text, rec = run(g, TRUE, trimLowCovEdges=True, maxItr=0)
    assert text == TRUE[1:] and (rec["trim_begin"], rec["trim_end"], rec["status"], rec["flags"]) == (1, 24, CHANGED, 0)
    # two foreign letters at either end: k-mers 0, 1 and 24, 25 are absent
    s = b"TT" + TRUE + b"AA"
    text, rec = run(g, s, trimLowCovEdges=True, maxItr=0)
    assert text == s[3:-2] and (rec["trim_begin"], rec["trim_end"]) == (3, 26)
    # the median below 2 * min_kmer_cov: the trim is not tried
    text, rec = run(g, s, trimLowCovEdges=True, maxItr=0, minKmerCov=6)
    assert text == s and (rec["trim_begin"], rec["trim_end"], rec["status"]) == (-1, -1, UNCHANGED)
    # no two good k-mers side by side: null, nothing is trimmed
    g2 = EGraph([(TRUE[:K], 10), (TRUE[2:2 + K], 10)])
    assert [int(c) for c in g2.counts(TRUE[:K + 2])] == [10, 0, 10]
    text, rec = run(g2, TRUE[:K + 2], trimLowCovEdges=True, maxItr=0)
    assert text == TRUE[:K + 2] and (rec["trim_begin"], rec["trim_end"], rec["status"]) == (-1, -1, UNCHANGED)
    # the only good pair is the last two k-mers: headIndex = nk - 1, tailIndex = nk: trimmed to nothing
    s = b"T" + TRUE[:K + 1]
    assert [int(c) for c in g.counts(s)] == [0, 10, 10]
    text, rec = run(g, s, trimLowCovEdges=True, maxItr=0)
    assert text == b"" and (rec["trim_begin"], rec["trim_end"], rec["flags"], rec["out_len"], rec["status"]) == (2, 3, TRIMMED_TO_NOTHING, 0, CHANGED)


def test_solid_screen_and_sequences_without_kmers():
    g = EGraph([(TRUE, 10)])
    bad = sub(TRUE, 12, "T")                                             # 19 k-mers of count 10
    assert run(g, bad, minNumSolidKmers=19)[0] == TRUE
    text, rec = run(g, bad, minNumSolidKmers=20)
    assert text is None and rec["status"] == NULL and rec["out_len"] == len(bad)
    assert run(g, bad, minNumSolidKmers=19, minKmerCov=11)[1]["status"] == NULL
    text, rec = run(g, b"ACG")
    assert text is None and rec["status"] == NO_KMER and rec["out_len"] == 3
    # a window shorter than lookahead is copied
    text, rec = run(g, bad, lookahead=30)
    assert text == bad and rec["status"] == UNCHANGED


def test_assemble_valid_kmers():
    g = EGraph([(TRUE, 10)])
    assert assemble_valid_kmers(TRUE, K, g) == [TRUE]
    s = TRUE[:12] + b"N" + TRUE[13:]                                     # the 5 k-mers with the N are invalid: two segments
    assert assemble_valid_kmers(s, K, g) == [TRUE[:12], TRUE[13:]]
    assert assemble_valid_kmers(sub(TRUE, 12, "T"), K, g) == [sub(TRUE, 12, "T")]      # count 0 but letters of ACGT: valid
    assert assemble_valid_kmers(b"N" + TRUE[:6], K, g) == [TRUE[:6]] and assemble_valid_kmers(TRUE[:6] + b"N", K, g) == [TRUE[:6]]
    assert assemble_valid_kmers(b"ACG", K, g) == []


# ---- the feature exists at every layer (these fail before it does) ----
def test_header_declares_the_entry_point():
    src = open(os.path.join(ROOT, "include", "rb_capi.h")).read()
    assert re.search(r"typedef struct rb_long_params \{\s*int32_t max_itr, lookahead, max_indel_size, min_kmer_cov, min_num_solid, trim_low_cov_edges, "
                     r"window_size;\s*float max_cov_gradient, percent_identity;\s*\} rb_long_params;", src)
    rec = re.search(r"typedef struct rb_long_rec \{([^}]*)\} rb_long_rec;", src)
    assert rec and len(re.findall(r"\b[a-z_0-9]+\s*[,;]", re.sub(r"/\*.*?\*/", "", rec.group(1)))) == 16
    assert re.search(r"\bint rb_graph_correct_long\(rb_graph \*g, const char \*seq, const int64_t \*offsets, int64_t n, const rb_long_params \*p,\s*"
                     r"const int64_t \*out_offsets, char \*out_seq, rb_long_rec \*recs\);", src)
    for cite in ("GraphUtils.java:3087-3185", ":1799-1848", ":3402-3602", ":3187-3241", ":1591-1675"):
        assert cite in src, cite


def test_library_exports_and_python_binds_it():
    import ctypes as C
    from rnabloom import _native as N
    assert hasattr(C.CDLL(N.LIB_PATH), "rb_graph_correct_long")
    assert "rb_graph_correct_long" in {s[0] for s in N.SYMBOLS}
    assert C.sizeof(N.LongParams) == 36
    from rnabloom import graphutils
    from rnabloom.graph import BloomFilterDeBruijnGraph
    assert callable(getattr(BloomFilterDeBruijnGraph, "correctLongFlat", None)) and callable(getattr(BloomFilterDeBruijnGraph, "correctLong", None))
    assert BloomFilterDeBruijnGraph.LONG_DTYPE.itemsize == 64 and BloomFilterDeBruijnGraph.LONG_DTYPE.names == FIELDS
    assert set(BloomFilterDeBruijnGraph.LONG_DEFAULTS) == set(DEFAULTS)
    for f in ("correctLongSequenceWindowed", "correctLongReads", "assembleValidKmers"):
        assert callable(getattr(graphutils, f, None)), f


def test_java_and_jni_sides_exist():
    java = open(os.path.join(ROOT, "java", "rnabloom", "graph", "NativeGraph.java")).read()
    assert re.search(r"public static native void correctLong\(long h, ByteBuffer seq, long\[\] offsets, int n, int\[\] params, float maxCovGradient,", java)
    jni = open(os.path.join(ROOT, "jni", "rb_jni.c")).read()
    assert "FN(correctLong)" in jni and "rb_graph_correct_long(" in jni
    g = open(os.path.join(ROOT, "java", "rnabloom", "graph", "BloomFilterDeBruijnGraph.java")).read()
    assert "NativeGraph.correctLong(handle" in g
