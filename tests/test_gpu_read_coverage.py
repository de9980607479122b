"""rb_graph_read_coverage (BloomFilterDeBruijnGraph.coverageStats) against the restatement of the reference's rules in
tests/test_read_coverage_rules.py, applied to the CPU oracle's getKmers count rows: every field of every record bit-equal (floats compared
as their bits), for reads, windows and mates, host and device outputs, sub-ranges, many pieces, counters at their ceiling, and the
argument errors."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rnabloom import _native as N
from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch, pair_threshold
from test_gpu_parity import graph_pair, make_reads, ragged_reads
from test_gpu_queries import expected_rows
from test_read_coverage_rules import FIELDS, F, complex_windows, expected_records, windows
import test_read_coverage_rules as R

PARAMS = [  # (lookahead, maxCovGradient, covFPR, minKmerCov)
    (3, 0.5, 0.0, 1.0), (1, 0.1, 0.01, 2.0), (3, 1.0, 0.5, 1.0), (1000, 0.5, 0.01, 3.0), (1, 1.0, 0.0, 0.0)]


def as_bits(recs):
    """records (numpy structured array or restated dicts) -> uint32 matrix, floats as their bits"""
    if isinstance(recs, np.ndarray):
        return recs.view(np.uint32).reshape(len(recs), 12)
    out = np.zeros((len(recs), 12), np.uint32)
    for i, r in enumerate(recs):
        out[i, :4] = [r["n"], r["n_solid"], r["n_complex"], r["flags"]]
        out[i, 4:] = np.array([r[f] for f in FIELDS[4:]], np.float32).view(np.uint32)
    return out


def assert_records(got, want):
    g, w = as_bits(got), as_bits(want)
    assert g.shape == w.shape, (g.shape, w.shape)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert bad.size == 0, "%d records differ, first %d: got %s want %s" % (bad.size, bad[0], got[bad[0]], want[bad[0]])


def with_complex(recs, reads, k, cache):
    """the restated records of reads mode carry n_complex (computed once per read set and k: the slow part of the restatement)"""
    key = (hash(tuple(reads)), k)
    if key not in cache:
        cache[key] = [complex_windows(s, k) for s in reads]
    for r, c in zip(recs, cache[key]):
        r["n_complex"] = c
    return recs


def restated(rows, lookahead, g, fpr, mc, **kw):
    recs, so = [], [0]
    for i, row in enumerate(rows):
        if kw.get("window"):
            recs += [R.coverage_stats(row[a:b], lookahead, F(g), F(fpr), mc) for a, b in windows(len(row), kw["window"])]
        else:
            mn = len(kw["mate_rows"][i]) if "mate_rows" in kw else None
            recs.append(R.coverage_stats(row, lookahead, F(g), F(fpr), mc, mn))
        so.append(len(recs))
    return recs, np.array(so, np.int64)


def short_reads(k, seed):
    (ls, lq, off), _ = make_reads(1200, 12000, 0.003, 1e-3, seed=seed)
    reads = [bytes(ls[off[i]:off[i + 1]]) for i in range(120)]
    rag, _ = ragged_reads(seed, 60)
    rag += [reads[0][:40] + b"N" + reads[1][:80], b"", reads[2][:k - 1], reads[3][:k], b"A" * 60 + reads[4][:50], (b"CA" * 40)]
    return (ls, lq, off), reads + rag


_cache = {}


@pytest.mark.parametrize("k,stranded", [(25, False), (25, True), (31, False), (63, True)])
def test_reads_mode_matches_the_restated_rules(k, stranded):
    (ls, lq, off), reads = short_reads(k, 40 + k)
    og, gg = graph_pair(300_007, 2_000_003, 10_007, k=k, stranded=stranded, pairs=False)
    og.add_reads(ls, lq, off, 3, 0); gg.addReads(ls, lq, off, 3)
    rows = expected_rows(og, reads, k)
    b = ReadBatch.from_reads(reads, None)
    for la, g, fpr, mc in PARAMS:
        got, so = gg.coverageStats(b, lookahead=la, maxCovGradient=g, covFPR=fpr, minKmerCov=mc)
        want, wso = restated(rows, la, g, fpr, mc)
        assert (so == wso).all()
        assert_records(got, with_complex(want, reads, k, _cache))
    # device output = host output; a sub-range = the matching slice; many pieces = one
    dev, _ = gg.coverageStats(b, to_host=False)
    host, _ = gg.coverageStats(b)
    assert (dev.cpu().numpy().view(gg.COV_DTYPE) == host).all()
    sub, sso = gg.coverageStats(b, 17, 100)
    assert (as_bits(sub) == as_bits(host[17:117])).all() and (sso == np.arange(101)).all()
    gg.destroy()


def test_many_pieces_equal_one(monkeypatch):
    (ls, lq, off), reads = short_reads(25, 3)
    og, gg = graph_pair(300_007, 2_000_003, 10_007, pairs=False)
    gg.addReads(ls, lq, off, 3)
    b = ReadBatch.from_reads(reads * 4, None)
    whole, _ = gg.coverageStats(b, covFPR=0.01)
    for piece in ("1", "1000"):
        monkeypatch.setenv("RB_QUERY_PIECE", piece)
        assert (as_bits(gg.coverageStats(b, covFPR=0.01)[0]) == as_bits(whole)).all()
        dev, _ = gg.coverageStats(b, covFPR=0.01, to_host=False)
        assert (dev.cpu().numpy().view(np.uint32).reshape(-1, 12) == as_bits(whole)).all()
        l, r = b, ReadBatch.from_reads(reads[::-1] * 4, None)
        m1 = gg.coverageStats(l, mates=r, lookahead=1)
        monkeypatch.delenv("RB_QUERY_PIECE")
        m0 = gg.coverageStats(l, mates=r, lookahead=1)
        assert (as_bits(m1[0]) == as_bits(m0[0])).all() and (m1[2].view(np.uint32) == m0[2].view(np.uint32)).all()
    gg.destroy()


def long_reads(n, seed, lo=2000, hi=5000):
    rng = np.random.default_rng(seed)
    T = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 20000)]
    out = []
    for _ in range(n):
        L = int(rng.integers(lo, hi + 1)); s = int(rng.integers(0, T.size - L))
        r = T[s:s + L].copy()
        err = rng.random(L) < 0.01
        r[err] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(err.sum()))]
        out.append(r.tobytes())
    return out


def test_windows_mode_on_long_reads_k35():
    reads = long_reads(24, 5)
    reads[3] = reads[3][:1000] + b"N" + reads[3][1001:]
    seq = np.frombuffer(b"".join(reads * 3), np.uint8)
    off = np.zeros(len(reads) * 3 + 1, np.int64); np.cumsum([len(r) for r in reads * 3], out=off[1:])
    og, gg = graph_pair(4_000_037, 8_000_009, 10_007, k=35, pairs=False)
    og.add_reads(seq, None, off, 0, 0); gg.addReads(seq, None, off, 0)
    rows = expected_rows(og, reads, 35)
    b = ReadBatch.from_reads(reads, None)
    for W, (la, g, fpr, mc) in zip((1, 7, 50, 501, 10 ** 6), PARAMS):
        got, so = gg.coverageStats(b, window=W, lookahead=la, maxCovGradient=g, covFPR=fpr, minKmerCov=mc)
        want, wso = restated(rows, la, g, fpr, mc, window=W)
        assert (so == wso).all() and so[-1] == len(got)
        assert_records(got, want)
        dev, _ = gg.coverageStats(b, window=W, lookahead=la, to_host=False)
        assert dev.numel() == 48 * so[-1]
    # reads mode over reads longer than a wavefront's share (a workgroup per read), n_complex included
    few = reads[:3]
    got, _ = gg.coverageStats(ReadBatch.from_reads(few, None), lookahead=3)
    want, _ = restated(rows[:3], 3, 0.5, 0.0, 1.0)
    assert_records(got, with_complex(want, few, 35, _cache))
    gg.destroy()


def test_mates_mode_with_mates_of_different_lengths():
    k = 25
    (ls, lq, off), (rs, rq, _) = make_reads(1500, 12000, 0.003, 1e-3, seed=61)
    og, gg = graph_pair(300_007, 2_000_003, 10_007, pairs=False)
    og.add_reads(ls, lq, off, 3, 0); gg.addReads(ls, lq, off, 3)
    og.add_reads(rs, rq, off, 3, rbo_revcomp()); gg.addReads(rs, rq, off, 3, reverseComplement=True)
    left = [bytes(ls[off[i]:off[i + 1]]) for i in range(100)]
    right = [bytes(rs[off[i]:off[i + 1]])[:150 - (i % 7) * 15] for i in range(100)]
    right[5] = right[5][:k - 3]
    right[9] = b""
    lrows, rrows = expected_rows(og, left, k), expected_rows(og, right, k)
    lb, rb = ReadBatch.from_reads([b"ACGT" * 9] + left, None), ReadBatch.from_reads(right + [b"ACGT" * 9], None)
    for la, g, fpr, mc in PARAMS:
        got, so, pt = gg.coverageStats(lb, 1, 100, mates=rb, mate_first=0, lookahead=la, maxCovGradient=g, covFPR=fpr, minKmerCov=mc)
        want, _ = expected_records(lrows, left, k, la, F(g), F(fpr), mc, mate_rows=rrows, mate_reads=right)
        assert (so == np.arange(101)).all() and len(got) == 200
        assert_records(got, want)
        wpt = np.array([R.pair_threshold(want[i], want[100 + i]) for i in range(100)], np.float32)
        assert (pt.view(np.uint32) == wpt.view(np.uint32)).all()
        assert (pair_threshold(got[:100], got[100:]).view(np.uint32) == wpt.view(np.uint32)).all()
    dev, _, dpt = gg.coverageStats(lb, 1, 100, mates=rb, to_host=False, covFPR=0.01)
    host, _, hpt = gg.coverageStats(lb, 1, 100, mates=rb, covFPR=0.01)
    assert (dev.cpu().numpy().view(gg.COV_DTYPE) == host).all() and (dpt.view(np.uint32) == hpt.view(np.uint32)).all()
    gg.destroy()


def rbo_revcomp():
    from oracle import rbo
    return rbo.REVCOMP


def test_counters_at_the_ceiling_give_every_rank():
    """prefixes of three transcripts read at geometric depths: counts from 1 to MiniFloat.toFloat(127) + 1 = 245761, and absent k-mers"""
    k = 25
    rng = np.random.default_rng(77)
    reads = []
    Ts = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, k + 160)].tobytes() for _ in range(3)]
    for t, T in enumerate(Ts):
        depth = np.round(np.geomspace(330_000, 1, 160) * (1 + 0.3 * t)).astype(np.int64)
        add = np.maximum(depth - np.append(depth[1:], 0), 0)          # prefix j read add[j] times: k-mer i is read depth[i] times
        for j in range(160):
            reads += [T[:k + j]] * int(add[j])
    rng.shuffle(reads)
    seq = np.frombuffer(b"".join(reads), np.uint8)
    off = np.zeros(len(reads) + 1, np.int64); np.cumsum([len(r) for r in reads], out=off[1:])
    og, gg = graph_pair(2_000_003, 3_000_017, 10_007, k=k, pairs=False)
    og.add_reads(seq, None, off, 0, 0); gg.addReads(seq, None, off, 0)
    probe = Ts + [T[::-1] for T in Ts] + [Ts[0][:60] + b"N" + Ts[1][:90], Ts[2][:k - 1]]
    rows = expected_rows(og, probe, k)
    seen = set(np.concatenate(rows).tolist())
    val = {0.0} | {float(x if x <= 7 else ((x & 7) | 8) << ((x >> 3) - 1)) + 1.0 for x in range(128)}
    assert seen <= val and len(seen) >= 120 and 245761.0 in seen and 0.0 in seen, sorted(val - seen)
    b = ReadBatch.from_reads(probe, None)
    for la, g, fpr, mc in PARAMS:
        got, _ = gg.coverageStats(b, lookahead=la, maxCovGradient=g, covFPR=fpr, minKmerCov=mc)
        want, _ = restated(rows, la, g, fpr, mc)
        assert_records(got, with_complex(want, probe, k, _cache))
        for W in (1, 5, 40):
            got, _ = gg.coverageStats(b, window=W, lookahead=la, maxCovGradient=g, covFPR=fpr, minKmerCov=mc)
            assert_records(got, restated(rows, la, g, fpr, mc, window=W)[0])
    gg.destroy()


def test_argument_errors():
    og, gg = graph_pair(100_003, 100_003, 10_007, pairs=False)
    b = ReadBatch.from_reads([b"ACGT" * 20] * 4, None)
    m = ReadBatch.from_reads([b"ACGT" * 20] * 2, None)
    with pytest.raises(RuntimeError, match="read range outside the batch"):
        gg.coverageStats(b, 2, 5)
    with pytest.raises(RuntimeError, match="mate range outside the mate batch"):
        gg.coverageStats(b, 0, 3, mates=m)
    with pytest.raises(RuntimeError, match="mates are only available with RB_COV_READS"):
        gg.coverageStats(b, mates=b, window=10)
    with pytest.raises(RuntimeError, match="lookahead must be >= 1"):
        gg.coverageStats(b, lookahead=0)
    with pytest.raises(RuntimeError, match="window must be >= 1"):
        gg.coverageStats(b, window=-1)
    with pytest.raises(RuntimeError, match="cov_fpr must be in"):
        gg.coverageStats(b, covFPR=1.5)
    with pytest.raises(RuntimeError, match="max_cov_gradient must be finite"):
        gg.coverageStats(b, maxCovGradient=float("nan"))
    with pytest.raises(RuntimeError, match="min_kmer_cov must be finite"):
        gg.coverageStats(b, minKmerCov=float("inf"))
    import ctypes as C
    p = N.CovParams(N.COV_WINDOWS, 10, 3, 0.5, 0.0, 1.0)
    assert N.lib.rb_graph_read_coverage(gg.h, b.h, 0, 2, None, 0, C.byref(p), None, None, 0) != 0
    assert b"seg_offsets is required" in N.lib.rb_last_error()
    p = N.CovParams(2, 10, 3, 0.5, 0.0, 1.0)
    assert N.lib.rb_graph_read_coverage(gg.h, b.h, 0, 2, None, 0, C.byref(p), None, None, 0) != 0
    assert b"segments must be" in N.lib.rb_last_error()
    rec, so = gg.coverageStats(b, 0, 0)
    assert rec.size == 0 and list(so) == [0]
    gg.destroyCbf()
    with pytest.raises(RuntimeError, match="counting filter has been destroyed"):
        gg.coverageStats(b)
    from rnabloom.sharded import LoopbackCluster
    cl = LoopbackCluster(2, 100_003, 100_003, 10_007, 2, 2, 2, 25, False, False)
    with pytest.raises(RuntimeError, match="not available on a shard handle"):
        BloomFilterDeBruijnGraph.coverageStats(cl.ranks[0], b)
