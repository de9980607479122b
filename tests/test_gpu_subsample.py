"""rb_subsample_reads against the restatement of tests/test_subsample_rules.py on the worlds of tests/subsample_worlds.py: out_keep, every int of
every record, the counting filter's bytes and the op ordinal — both modes, the stranded and the canonical pair form, one to four hash
functions, maxMultiplicity 1, 3 and 20, filters of 257 counters (where most increments of a read share counters and a look-up that saw a stale
counter would change a verdict) and of a realistic size.  The same input in one call, in three calls and in pieces of one read gives the
same bytes; rnabloom.subsampler's two routes agree; shard handles and bad arguments are refused."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import subsample_worlds as W
from rnabloom import _native as N
from rnabloom import sharded, subsampler
from rnabloom.bloom import CountingBloomFilter
from test_subsample_rules import FIELDS, Filter, NOT_JUDGED, strobemer_based

IDS = [W.world_id(w) for w in W.WORLDS]


def params_of(w):
    if w["mode"] == "strobemer":
        return subsampler.strobemer_params(W.K, w["M"], w["clip"], W.INDEL)
    return N.SubsampleParams(N.SUB_KMER, W.K, 0, 0, int(w["canonical"]), w["M"], w["clip"], 0)


def run(i, piece_reads=subsampler.PIECE_READS):
    w = W.WORLDS[i]
    cbf = CountingBloomFilter(w["size"], w["H"], W.K, device=0, rngSeed=w["seed"])
    keep, recs, totals = subsampler.subsample_reads(cbf, params_of(w), list(W.reads_of(i)), piece_reads, want_recs=True)
    return keep, recs, totals, cbf.toBytes(), cbf._g.getOpOrdinal()


def same_as_wanted(i, got):
    keep, recs, totals, data, ordinal = got
    wkeep, wrecs, wdata, wordinal = W.want(i)
    bad = np.flatnonzero((recs != wrecs).any(axis=1))
    assert bad.size == 0, "read %d: got %s, want %s (%s)" % (bad[0], recs[bad[0]].tolist(), wrecs[bad[0]].tolist(), ", ".join(FIELDS))
    assert (keep == wkeep).all()
    assert ordinal == wordinal
    diff = np.flatnonzero(data != wdata)
    assert diff.size == 0, "%d counters differ, the first at %d: %d for %d" % (diff.size, diff[0], data[diff[0]], wdata[diff[0]])
    assert totals[:3].tolist() == [int(wkeep.sum()), wordinal, int((wrecs[:, 0] == NOT_JUDGED).sum())] and totals[3] > 0


@pytest.mark.parametrize("i", range(len(W.WORLDS)), ids=IDS)
def test_keep_records_filter_and_ordinal_match_the_restatement(i):
    same_as_wanted(i, run(i))


@pytest.mark.parametrize("i", [1, 3, 6], ids=[IDS[1], IDS[3], IDS[6]])
def test_three_calls_and_pieces_of_one_read_give_the_bytes_of_one_call(i, monkeypatch):
    same_as_wanted(i, run(i, piece_reads=(len(W.reads_of(i)) + 2) // 3))
    monkeypatch.setenv("RB_QUERY_PIECE", "1")                       # the library's own pieces: one read each
    same_as_wanted(i, run(i))


def test_the_other_workgroup_size_gives_the_same(monkeypatch):
    monkeypatch.setenv("RB_SUB_TPB", "256")
    same_as_wanted(2, run(2))
    monkeypatch.setenv("RB_SUB_TPB", "64")
    same_as_wanted(6, run(6))


def test_the_two_routes_of_the_subsampler_agree():
    reads = list(W.reads_of(0))[:150]
    for size, H, M, clip in ((W.REAL, 2, 1, 0), (W.SMALL, 3, 3, 90)):
        args = (reads, size, W.K, H, True, M, clip, W.INDEL)
        kept, fpr = subsampler.strobemerBased(*args, device=0, rngSeed=5)
        kept_c, fpr_c, data_c, ordinal_c = subsampler.strobemerBasedComposed(*args, device=0, rngSeed=5, want_filter=True)
        assert kept == kept_c and fpr == fpr_c and 0 < len(kept) < len(reads)
        # ... and are the restatement in the reference's visiting order, on the filter's bytes too
        order = subsampler.visiting_order(len(reads))
        assert order[:3] == [0, 3, 6] and sorted(order) == list(range(len(reads)))
        f = Filter(size, H, W.K, seed=5)
        wkeep, _ = strobemer_based(f, [reads[j] for j in order], W.K, M, clip, W.INDEL)
        assert kept == [j for j, kp in zip(order, wkeep) if kp]
        assert (data_c == f.bytes()).all() and ordinal_c == f.ordinal()


def test_kmer_based_returns_the_kept_indices_and_raises_where_the_reference_throws():
    i = 4
    w = W.WORLDS[i]
    reads = list(W.reads_of(i))
    with pytest.raises(ValueError, match="negative range"):
        subsampler.kmerBased(reads, w["size"], W.K, w["H"], True, w["M"], w["clip"], device=0, rngSeed=w["seed"])
    wkeep, wrecs, _, _ = W.want(i)
    first_bad = int(np.flatnonzero(wrecs[:, 0] == NOT_JUDGED)[0])
    kept, fpr = subsampler.kmerBased(reads[:first_bad], w["size"], W.K, w["H"], True, w["M"], w["clip"], device=0, rngSeed=w["seed"])
    assert kept == np.flatnonzero(wkeep[:first_bad]).tolist() and 0 < fpr < 1


def test_refusals_leave_the_filter_alone():
    reads = list(W.reads_of(0))[:5]
    seq = np.frombuffer(b"".join(reads), np.uint8)
    off = np.zeros(6, np.int64); off[1:] = np.cumsum([len(r) for r in reads])
    keep = np.zeros(5, np.uint8)
    cbf = CountingBloomFilter(W.REAL, 2, W.K, device=0)

    def call(h, p, off=off, keep_ptr=keep.ctypes.data):
        return N.lib.rb_subsample_reads(h, C.byref(p) if p is not None else None, seq.ctypes.data, off.ctypes.data, 5, keep_ptr, None, None)

    good = subsampler.strobemer_params(W.K, 1, 0, W.INDEL)
    rk = sharded.ShardRank((100_003, 200_003, 30_011, 2, 2, 2, W.K, 0, 1, 0, 0, 9, 0), 0, 1, 0, "split")
    assert call(rk.h, good) != 0 and b"shard" in N.lib.rb_last_error()                    # a shard handle
    assert call(None, good) != 0 and call(cbf._g.h, None) != 0 and call(cbf._g.h, good, keep_ptr=None) != 0
    for field, value in (("mode", 2), ("k", W.K + 1), ("wmin", 0), ("wmax", 5), ("max_multiplicity", 0), ("max_edge_clip", -1)):
        p = subsampler.strobemer_params(W.K, 1, 0, W.INDEL)
        setattr(p, field, value)
        assert call(cbf._g.h, p) != 0, field
    down = off.copy(); down[2] = down[1] - 1
    assert call(cbf._g.h, good, off=down) != 0
    assert cbf._g.getOpOrdinal() == 0 and not cbf.toBytes().any() and not keep.any()
    f = Filter(W.REAL, 2, W.K)                                                           # ... and the good call works
    wkeep, _ = strobemer_based(f, reads, W.K, 1, 0, W.INDEL)
    assert call(cbf._g.h, good) == 0 and keep.tolist() == wkeep.tolist() and cbf._g.getOpOrdinal() == f.ordinal() > 0
    t = np.full(4, -1, np.int64)                                                         # no reads: nothing happens
    assert N.lib.rb_subsample_reads(cbf._g.h, C.byref(good), None, None, 0, None, None, t.ctypes.data) == 0 and t.tolist() == [0, 0, 0, 0]
