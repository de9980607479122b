"""rb_graph_correct_pairs (GraphUtils.correctErrorsPE / correctErrorsSE with every round on the device) against the restatement of
tests/test_pair_correction_rules.py run on the CPU oracle's filters, a device graph and the oracle built from the same reads
(tests/pair_correction_worlds.py; tests/test_pair_correction_reach.py shows that the pairs ask something).  Compared exactly: every int of
every record — the thresholds as bits — and both texts byte for byte.  Then: graphutils.correctErrorsPEComposed on the same device graph (the
host loop over ReadBatch / coverageStats / correctErrors), the single form against correct_single and against coverageStats' se_threshold +
correctErrors, many pieces, capacities of the exact input length, 0 / 1 / 4 rounds, two threads on one handle, the refusals, the profile entry."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pair_correction_worlds as PW
from rnabloom import _native as N
from rnabloom import graphutils, sharded
from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch, _pack
from test_pair_correction_rules import NOT_JUDGED, REC_FIELDS

ERR_INVALID = 1


def kw_of(params):
    return dict(lookahead=params["lookahead"], maxIndelSize=params["max_indel"], maxCovGradient=params["gradient"], covFPR=params["fpr"],
                errorCorrectionIterations=params["iterations"], minCovThreshold=params["min_thr"], percentIdentity=params["pid"],
                minKmerCov=params["min_cov"])


KW = kw_of(PW.PARAMS)


def rec_tuple(r):
    return tuple(int(r[f]) for f in REC_FIELDS)


def compare(g, pairs, want, label, **over):
    res, recs = g.correctPairs([l for l, _ in pairs], [r for _, r in pairs], records=True, **dict(KW, **over))
    for i, ((rec, lo, ro), got) in enumerate(zip(want, res)):
        assert rec_tuple(recs[i]) == tuple(rec[f] for f in REC_FIELDS), (label, i, dict(zip(REC_FIELDS, rec_tuple(recs[i]))), rec)
        if rec["status"] == NOT_JUDGED:
            assert got is None, (label, i)
        else:
            assert got == (lo, ro, rec["status"] == N.PAIRC_CORRECTED), (label, i, rec)
    return res, recs


@pytest.mark.parametrize("case", PW.CASES, ids=PW.case_id)
def test_pairs_match_the_oracle_and_the_composed_route(case):
    w, pairs, _ = PW.pair_case(case)
    want = PW.gpu_calls(case)[PW.PARAMS["iterations"]]
    g = w.device()
    res, _ = compare(g, pairs, want, "4 rounds")
    lefts, rights = [l for l, _ in pairs], [r for _, r in pairs]
    args = (PW.PARAMS["lookahead"], PW.PARAMS["max_indel"], PW.PARAMS["gradient"], PW.PARAMS["fpr"], PW.PARAMS["iterations"], PW.PARAMS["min_thr"],
            PW.PARAMS["pid"], PW.PARAMS["min_cov"])
    assert graphutils.correctErrorsPE(g, lefts, rights, *args) == res
    assert graphutils.correctErrorsPEComposed(g, lefts, rights, *args) == res
    assert g.correctPairs([], []) == []


@pytest.mark.parametrize("case", PW.CASES, ids=PW.case_id)
@pytest.mark.parametrize("iterations", PW.ROUND_COUNTS)
def test_round_counts(case, iterations):
    w, pairs, _ = PW.pair_case(case)
    want = PW.gpu_calls(case)[iterations]
    compare(w.device(), pairs[:len(want)], want, "%d rounds" % iterations, errorCorrectionIterations=iterations)


@pytest.mark.parametrize("case", PW.CASES[:2], ids=PW.case_id)
def test_single_form(case):
    w, seqs, want = PW.single_case(case)
    g = w.device()
    res, recs = g.correctReads(seqs, records=True, **KW)
    for i, ((rec, text), got) in enumerate(zip(want, res)):
        assert rec_tuple(recs[i]) == tuple(rec[f] for f in REC_FIELDS), (i, dict(zip(REC_FIELDS, rec_tuple(recs[i]))), rec)
        assert got == (text if rec["status"] == N.PAIRC_CORRECTED else None), i
    assert graphutils.correctErrorsSE(g, seqs, KW["lookahead"], KW["maxIndelSize"], KW["maxCovGradient"], KW["covFPR"], KW["percentIdentity"], KW["minKmerCov"]) == res
    # the existing route: coverageStats' se_threshold, then correctErrors on the reads that have one
    have = [i for i, s in enumerate(seqs) if len(s) >= w.k]
    seq, off = _pack([seqs[i] for i in have])
    b = ReadBatch.from_ascii(seq, None, off, 0)
    st, _ = g.coverageStats(b, maxCovGradient=KW["maxCovGradient"], covFPR=KW["covFPR"])
    b.close()
    found = [j for j in range(len(have)) if int(st[j]["flags"]) & N.COV_SE_FOUND]
    out = g.correctErrors([seqs[have[j]] for j in found], [float(st[j]["se_threshold"]) for j in found], KW["lookahead"], KW["maxIndelSize"],
                          KW["percentIdentity"], KW["minKmerCov"])
    composed = [None] * len(seqs)
    for j, (text, ok) in zip(found, out):
        composed[have[j]] = text if ok else None
    assert composed == res
    # iterations is read as zero or not; min_cov_threshold is not read
    assert g.correctReads(seqs[:40], **dict(KW, errorCorrectionIterations=1, minCovThreshold=1e9)) == res[:40]
    assert g.correctReads(seqs[:40], **dict(KW, errorCorrectionIterations=0)) == [None] * 40


def flat(w, pairs, room=16, **over):
    lseq, lo = _pack([l for l, _ in pairs])
    rseq, ro = _pack([r for _, r in pairs])
    loo, roo = np.zeros(len(pairs) + 1, np.int64), np.zeros(len(pairs) + 1, np.int64)
    np.cumsum([len(l) + room for l, _ in pairs], out=loo[1:])
    np.cumsum([len(r) + room for _, r in pairs], out=roo[1:])
    return (loo, roo) + w.device().correctPairsFlat(lseq, lo, rseq, ro, loo, roo, **dict(KW, **over))


def same(a, b):
    return all((x == y).all() for x, y in zip(a, b))


def test_many_pieces_equal_one(monkeypatch):
    w, pairs, want = PW.pair_case(PW.CASES[0])
    whole = flat(w, pairs)
    assert (whole[4]["rounds_run"] >= 2).sum() >= 10
    for piece in ("1", "7", "5000"):
        monkeypatch.setenv("RB_QUERY_PIECE", piece)
        assert same(flat(w, pairs), whole), piece


def test_exact_capacity_overflows_and_a_second_call_has_the_text():
    w, pairs, want = PW.pair_case(PW.CASES[0])
    loo, roo, lout, rout, recs = flat(w, pairs, room=0)
    grown = 0
    for i, (rec, lo, ro) in enumerate(want):
        fl = int(recs[i]["flags"])
        assert bool(fl & N.PAIRC_LEFT_OVERFLOW) == (len(lo) > len(pairs[i][0])) and bool(fl & N.PAIRC_RIGHT_OVERFLOW) == (len(ro) > len(pairs[i][1])), i
        assert (int(recs[i]["left_len"]), int(recs[i]["right_len"])) == (len(lo), len(ro)), i
        assert fl & 3 == rec["flags"] and rec_tuple(recs[i])[:3] == (rec["status"], rec["end"], rec["rounds_run"])
        for out, oo, text, over in ((lout, loo, lo, fl & N.PAIRC_LEFT_OVERFLOW), (rout, roo, ro, fl & N.PAIRC_RIGHT_OVERFLOW)):
            if over:
                grown += 1
                assert not out[oo[i]:oo[i + 1]].any(), i                       # nothing written
            else:
                assert out[oo[i]:oo[i] + len(text)].tobytes() == text, i
    assert grown >= 20
    # the public form calls once more for the mates that overflow: slack 0 gives what slack 16 gives
    g = w.device()
    sub = pairs[:200]
    assert g.correctPairs([l for l, _ in sub], [r for _, r in sub], slack=0, **KW) == g.correctPairs([l for l, _ in sub], [r for _, r in sub], **KW)


def test_two_threads_on_one_handle():
    w, pairs, want = PW.pair_case(PW.CASES[1])
    a, b = pairs[:300], pairs[300:]
    ra, rb_ = flat(w, a), flat(w, b)
    res, errs = {}, []

    def work(name, prs):
        try:
            for _ in range(3):
                res[name] = flat(w, prs)
        except Exception as e:                     # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=("a", a)), threading.Thread(target=work, args=("b", b))]
    for t in ts: t.start()
    for t in ts: t.join()
    assert not errs, errs
    assert same(res["a"], ra) and same(res["b"], rb_)


def raw_call(g, lefts, rights, params=(2, 5, 1, 0.5, 0.01, 2.0, 0.9, 1.0), lseq=True, loff=True, rseq=True, roff=True, p=True, loo=True, lout=True,
             roo=True, rout=True, recs=True, loffsets=None, loo_values=None):
    ls, lo = _pack(lefts)
    n = len(lefts)
    if loffsets is not None:
        lo = np.asarray(loffsets, np.int64)
    a_loo = np.arange(n + 1, dtype=np.int64) * 400 if loo_values is None else np.asarray(loo_values, np.int64)
    a_lout = np.zeros(1 << 16, np.uint8)
    pr = N.PairCorrParams(*params)
    a_recs = np.zeros(n, BloomFilterDeBruijnGraph.PAIRC_DTYPE)
    ptr = lambda a, use: a.ctypes.data_as(C.c_void_p) if use and a is not None else None
    rs = ro = a_roo = a_rout = None
    if rights is not None:
        rs, ro = _pack(rights)
        a_roo = np.arange(n + 1, dtype=np.int64) * 400
        a_rout = np.zeros(1 << 16, np.uint8)
    return N.lib.rb_graph_correct_pairs(g, ptr(ls, lseq), ptr(lo, loff), ptr(rs, rseq), ptr(ro, roff), n, C.byref(pr) if p else None, ptr(a_loo, loo),
                                        ptr(a_lout, lout), ptr(a_roo, roo), ptr(a_rout, rout), ptr(a_recs, recs))


class launches_nothing:
    """every call made on handle h inside the block is refused before anything is launched: no piece of rb_graph_correct_pairs ran, so the
    profile has no "correct_pairs" entry"""

    def __init__(self, h):
        self.h = h

    def profile(self):
        p = N.Profile()
        assert N.lib.rb_graph_profile_get(self.h, C.byref(p), 1) == 0
        return {p.name[i].decode(): (p.ms[i], p.launches[i]) for i in range(p.n)}

    def __enter__(self):
        assert N.lib.rb_graph_profile_enable(self.h, 1) == 0
        self.profile()
        return self

    def __exit__(self, *exc):
        prof = self.profile()
        assert N.lib.rb_graph_profile_enable(self.h, 0) == 0
        if exc[0] is None:
            assert "correct_pairs" not in prof, "a refusal launched something: %s" % prof
        return False


def test_refusals():
    l, r = [b"ACGT" * 60, b"ACGTTGCA" * 20], [b"TTGCA" * 40, b"ACGT" * 50]
    good = (2, 5, 1, 0.5, 0.01, 2.0, 0.9, 1.0)
    g = BloomFilterDeBruijnGraph(100_003, 200_003, 30_011, 2, 2, 2, 25, False, True)
    # what is taken, and that a call that is taken shows in the profile (so its absence below means something)
    g.profileEnable(True)
    g.profileGet(reset=True)
    assert raw_call(g.h, l, r) == 0 and raw_call(g.h, l, None) == 0
    assert g.profileGet(reset=True)["correct_pairs"][1] == 2
    assert raw_call(g.h, l, r, params=(2, 5, 1, 0.0, 0.0, -3.0, 0.9, 1.0)) == 0 and raw_call(g.h, l, r, params=(2, 5, 1, 1.0, 1.0, 2.0, 0.9, 1.0)) == 0
    assert raw_call(g.h, l, r, params=(2, 1, 0, 0.5, 0.01, 2.0, 0.9, 1.0)) == 0 and raw_call(g.h, l, r, params=(2, 16, 4096, 0.5, 0.01, 2.0, 0.9, 1.0)) == 0
    assert g.profileGet(reset=True)["correct_pairs"][1] == 4
    assert raw_call(g.h, l, r, params=(0, 5, 1, 0.5, 0.01, 2.0, 0.9, 1.0)) == 0      # no rounds: nothing to launch
    assert "correct_pairs" not in g.profileGet(reset=True)
    g.profileEnable(False)
    # every refusal, and none launches anything
    assert raw_call(None, l, r) == ERR_INVALID
    with launches_nothing(g.h):
        for name in ("loff", "p", "loo", "lout", "recs", "lseq", "rseq", "roo", "rout"):
            assert raw_call(g.h, l, r, **{name: False}) == ERR_INVALID, name
        assert raw_call(g.h, l, r, roff=False) == ERR_INVALID                 # right text without offsets is no single form
        for at in range(3, 8):
            for bad in (np.nan, np.inf, -np.inf):
                assert raw_call(g.h, l, r, params=good[:at] + (bad,) + good[at + 1:]) == ERR_INVALID, (at, bad)
        assert raw_call(g.h, l, r, params=(2, 5, 1, -0.1, 0.01, 2.0, 0.9, 1.0)) == ERR_INVALID
        for fpr in (-0.01, 1.01):
            assert raw_call(g.h, l, r, params=(2, 5, 1, 0.5, fpr, 2.0, 0.9, 1.0)) == ERR_INVALID
        for la in (0, -1, 17):
            assert raw_call(g.h, l, r, params=(2, la, 1, 0.5, 0.01, 2.0, 0.9, 1.0)) == ERR_INVALID
        for indel in (-1, 4097):
            assert raw_call(g.h, l, r, params=(2, 5, indel, 0.5, 0.01, 2.0, 0.9, 1.0)) == ERR_INVALID
        assert raw_call(g.h, l, r, params=(-1, 5, 1, 0.5, 0.01, 2.0, 0.9, 1.0)) == ERR_INVALID
        assert raw_call(g.h, l, r, loffsets=[0, 240, 100]) == ERR_INVALID     # decreasing offsets
        assert raw_call(g.h, l, r, loo_values=[0, 400, 300]) == ERR_INVALID
        assert raw_call(g.h, l, None, params=(2, 0, 1, 0.5, 0.01, 2.0, 0.9, 1.0)) == ERR_INVALID      # the single form is refused alike
        with pytest.raises(N.NativeError):
            g.correctPairs(l, r, maxCovGradient=float("nan"))
    with launches_nothing(g.h):
        g.destroyCbf()
        assert raw_call(g.h, l, r) == ERR_INVALID
    g.destroy()
    g = BloomFilterDeBruijnGraph(100_003, 200_003, 30_011, 2, 2, 2, 25, False, True)
    with launches_nothing(g.h):
        g.destroyDbgbf()
        assert raw_call(g.h, l, r) == ERR_INVALID
    g.destroy()
    g = BloomFilterDeBruijnGraph(100_003, 200_003, 30_011, 2, 2, 2, 1, False, True)
    with launches_nothing(g.h):
        assert raw_call(g.h, l, r) == ERR_INVALID                             # k < 2
    g.destroy()
    rk = sharded.ShardRank((100_003, 200_003, 30_011, 2, 2, 2, 25, 0, 1, 0, 0, 9, 0), 0, 1, 0, "split")
    with launches_nothing(rk.h):
        assert raw_call(rk.h, l, r) == ERR_INVALID                            # a shard handle


def test_profile_entry():
    w, pairs, want = PW.pair_case(PW.CASES[0])
    g = w.device()
    g.profileEnable(True)
    g.profileGet(reset=True)
    flat(w, pairs)
    prof = g.profileGet()
    g.profileEnable(False)
    assert prof["correct_pairs"][0] > 0 and prof["correct_pairs"][1] == 1, prof
    assert not any(name.startswith("correct_errors") for name in prof), prof
