"""The table-driven emit pass (k_hash_windows_direct): after the prefilter one lane hashes one kept window from its own
k bases, four bases per table lookup, instead of rolling through the dropped windows before it.

  a  against the walkers: RB_EMIT_CHECK=1 runs the emit kernel the call would have used before (the sparse walker; the resuming one where
     states were saved) into scratch arrays beside the direct one and compares every key and every occurrence id on the device; the call
     fails on the first difference.  Every insert below runs with it.  That the check CAN fail is unverified: the library has no hook that
     makes one of the two kernels wrong, and none was added for it.  What is verified is that it ran (RB_EMIT_CHECK=2 reports the records
     it compared) and, by (b), that a wrong key or occurrence id would not pass anyway.
  b  against the oracle: dbgbf, the counting filter and rpkbf byte-equal to oracle/rbo's after each pass, and the same bytes with
     RB_EMIT_DIRECT=0 and =1.  Unlike a prefilter fault, a wrong hash or occurrence id changes filter bytes (the occurrence id feeds the
     draw of the counter increment).

k = 17, 24, 25, 31, 32 (k mod 4 = 1, 0, 1, 3, 0, and the window that fills all 64 bits of its codes) and k = 18 for k mod 4 = 2; forward,
canonical and reverse hashing, reverseComplement on and off; uniform 150-base reads and ragged reads of 0 .. 300 bases (shorter than k, ending
at word boundaries, masked stretches that leave whole 512-word blocks empty).  Each input is inserted twice in sub-batches of at most 15 000
records: the first sub-batches of the first pass meet a cold cache and keep every window (every start bit 0 .. 31 of a word, blocks of up to
16 384 records = many rounds), the second pass keeps few (sparse masks)."""
import contextlib
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (300_007, 400_009, 60_013)                   # dbgbf bits, cbf bytes, rpkbf bits: the prefilter test's sizes
SEED = 7
SWITCHES = ("RB_EMIT_DIRECT", "RB_EMIT_CHECK", "RB_EMIT_RESUME", "RB_SPARSE_EMIT", "RB_FILTER_CHECK", "RB_PF_SKIP", "RB_SERIAL")
KS = (17, 18, 24, 25, 31, 32)
HASHING = [(False, False), (False, True), (True, False), (True, True)]       # (stranded, reverseComplement): canonical x 2, forward, reverse
_hid = lambda h: ("stranded" if h[0] else "canonical") + ("-rc" if h[1] else "")


@contextlib.contextmanager
def env(**kw):
    """the library reads its switches from the environment on every call"""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def reads_of(shape, k):
    """(seq, qual, offsets) of about 3 000 reads of a 4 000-base text.  ragged: lengths 0 .. 300 with every edge (shorter than k, k, whole words),
    and 260 reads in a row whose every base is below the quality floor: 1 300 words that keep nothing, so whole 512-word blocks are empty"""
    from rnabloom import synth
    L, n = {"uniform": (150, 3000), "ragged": (300, 3000)}[shape]
    d = synth.generate_pairs(n, G=4000, L=L, err=0.002, n_rate=1e-3, seed=91, uniform_expr=True, frag_mean=450.0, frag_sd=30.0)
    reads, quals = d["left"], d["lqual"].copy()
    rng = np.random.default_rng(1000 * k + L)
    if shape == "uniform":
        lens = np.full(n, L)
    else:
        lens = np.where(rng.random(n) < 0.5, 150, rng.integers(1, 301, n))
        edges = [0, 1, k - 1, k, k + 1, 32, 33, 64, 65, 96, 128, 150, 160, 192, 256, 257, 288, 299, 300]
        lens[rng.integers(0, n, 300)] = rng.choice(edges, 300)
        lens[:len(edges)] = edges
        lens[1200:1460] = 150
        quals[1200:1460, :] = ord("!")
        for r in rng.integers(0, n, 400):                 # masked bases inside reads: words that keep nothing beside words that do
            a = int(rng.integers(0, L - 40))
            quals[r, a:a + int(rng.integers(1, 40))] = ord("!")
    keep = np.arange(L)[None, :] < lens[:, None]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return np.ascontiguousarray(reads[keep]), np.ascontiguousarray(quals[keep]), off


def insert_twice(k, stranded, rc, shape, direct, capfd):
    """both passes through the library under RB_EMIT_DIRECT=direct with the emit check on (it only exists beside the direct kernel);
    the filters after each pass and the records the check compared"""
    from rnabloom import _native as N
    from rnabloom.graph import BloomFilterDeBruijnGraph
    seq, qual, off = reads_of(shape, k)
    out, compared, kept = [], 0, []
    with env(RB_EMIT_DIRECT=direct, RB_EMIT_CHECK="2"):
        gg = BloomFilterDeBruijnGraph(*SIZES, 2, 2, 2, k, stranded, True, rngSeed=SEED, maxBatchKmers=15_000)
        gg.setReadPairedKmerDistance(40)
        for _ in range(2):
            capfd.readouterr()
            st = gg.addReads(seq, qual, off, 3, reverseComplement=rc, storeReadPairedKmers=True)
            err = capfd.readouterr().err
            compared += sum(int(m) for m in re.findall(r"emit check: (\d+) records, 0 differ", err))
            assert "differ" not in re.sub(r"emit check: \d+ records, 0 differ", "", err), err
            kept.append((st.sorted_kmers, st.kmers))
            out.append([gg.exportFilter(w).copy() for w in (N.DBGBF, N.CBF, N.RPKBF)])
        gg.destroy()
    return out, compared, kept


@functools.lru_cache(maxsize=None)
def oracle_twice(k, stranded, rc, shape):
    from oracle import rbo
    seq, qual, off = reads_of(shape, k)
    og = rbo.Graph(*SIZES, 2, 2, 2, k, stranded, True, SEED)
    og.set_read_pair_distance(40)
    out = []
    for _ in range(2):
        og.add_reads(seq, qual, off, 3, rbo.STORE_READ_PAIRS | (rbo.REVCOMP if rc else 0))
        out.append([og.dbgbf_bytes().copy(), og.cbf_bytes().copy(), og.rpkbf_bytes().copy()])
    return out


@pytest.mark.parametrize("shape", ["uniform", "ragged"])
@pytest.mark.parametrize("hashing", HASHING, ids=_hid)
@pytest.mark.parametrize("k", KS)
def test_direct_emit_equals_the_walkers_and_the_oracle(k, hashing, shape, capfd):
    stranded, rc = hashing
    want = oracle_twice(k, stranded, rc, shape)
    got, compared, kept = insert_twice(k, stranded, rc, shape, "1", capfd)
    old, compared_old, kept_old = insert_twice(k, stranded, rc, shape, "0", capfd)
    for p in range(2):
        for name, g, o, w in zip(("dbgbf", "cbf", "rpkbf"), got[p], old[p], want[p]):
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, "pass %d, %s: %d bytes differ from the oracle's (first %s)" % (p + 1, name, bad.size, bad[:5])
            assert (g == o).all(), "pass %d, %s differs between RB_EMIT_DIRECT=1 and =0" % (p + 1, name)
    # (a) ran on every record the direct kernel wrote, and only beside it
    assert compared == kept[0][0] + kept[1][0] and compared_old == 0, (compared, kept, compared_old)
    assert kept[0][1] == kept_old[0][1] and kept[1][1] == kept_old[1][1]      # (how many are KEPT depends on how far the consumer's cache updates got)
    # the warm pass kept less than the first and dropped most windows: dense and sparse masks were both emitted
    assert kept[0][0] > kept[1][0] > 0 and kept[1][0] < kept[1][1] // 2 and kept[0][1] > 100_000, kept


def test_sharded_engine_gets_the_direct_emit(capfd):
    """2 virtual ranks in split mode reach the same launcher (rb_shard.hip): the check runs there too and the filters are the oracle's"""
    from oracle import rbo
    from rnabloom import _native as N
    from rnabloom import synth
    from rnabloom.graph import ReadBatch
    from rnabloom.sharded import LoopbackCluster
    d = synth.generate_pairs(3000, G=4000, err=0.002, n_rate=1e-3, seed=5, uniform_expr=True)
    s, off = synth.flat(d["left"]); q, _ = synth.flat(d["lqual"])
    with env(RB_EMIT_CHECK="2"):
        og = rbo.Graph(*SIZES, 2, 2, 2, 25, False, True, 9)
        cl = LoopbackCluster(2, *SIZES, 2, 2, 2, 25, False, True, rngSeed=9, mode="split")
        og.set_read_pair_distance(115); cl.setReadPairedKmerDistance(115)
        compared = 0
        for _ in range(2):
            og.add_reads(s, q, off, 3, rbo.STORE_READ_PAIRS)
            capfd.readouterr()
            cl.addBatch(ReadBatch.from_ascii(s, q, off, 3), 150, storeReadPairedKmers=True, reads_per_substep=500)
            err = capfd.readouterr().err
            compared += sum(int(m) for m in re.findall(r"emit check: (\d+) records, 0 differ", err))
            assert "differ" not in re.sub(r"emit check: \d+ records, 0 differ", "", err), err
            assert (cl.exportFilter(N.DBGBF) == og.dbgbf_bytes()).all()
            assert (cl.exportFilter(N.CBF) == og.cbf_bytes()).all()
            assert (cl.exportFilter(N.RPKBF) == og.rpkbf_bytes()).all()
        kept, total = sum(r.stats["sorted_kmers"] for r in cl.ranks), sum(r.stats["kmers"] for r in cl.ranks)
        assert 0 < compared <= kept < total, (compared, kept, total)
        cl.destroy()
