"""The no-op prefilter and its hot-k-mer cache against the oracle, through rb_debug_cache_export / rb_debug_prefilter
and the plain reference of tests/prefilter_ref.py.

Whole inserts cannot see most faults here: a lookup that misses keeps the window, a cache that is off for one strand or one k range only
sorts more records, and a forged or overstated entry changes a filter byte only if an unlucky draw meets it.  So:

  A  after every insert call the table is dumped and every entry must be true of the oracle's filters (never forge, never overstate);
  B  with the cache hot, the keep mask of the window walk must be exactly what the dumped table and the shared generator imply, the entry
     being looked up by hash ANYWHERE in the table — over the reads the cache was built from, their reverse complements, a stranded graph,
     k = 17 .. 64, a read per lane / ragged reads with every length edge / reads too long for a lane, every walker (RB_FILTER_PIPE = 0, 1, 3)
     and the hash-bucketed table (RB_NO_MPF);
  C  what the debug call keeps is what a real insert of the same reads from the same state sorts;
  D  4096 copies of one clean read: every k-mer with an entry drops what its bound allows, and a k-mer seen before may not have two EMPTY
     candidate slots.

The tables are the smallest the library accepts (RB_MPF = RB_NPF = 8): buckets full, both cuckoo steps and the replacement by rank at work."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

import prefilter_ref as P

pytestmark = pytest.mark.gpu

SEED, ORD0, POSB = 7, (1 << 33) + 12345, 9           # one generator table for every case (tests/grouping_ref.py keeps it)
SIZES = (300_007, 400_009, 60_013)                   # dbgbf bits, cbf bytes, rpkbf bits: the neighbouring tests' sizes
NB = 600                                             # reads of a batch the window walk is checked on
SWITCHES = ("RB_FILTER_PIPE", "RB_READ_LANES", "RB_RAGGED_LANES", "RB_NO_MPF", "RB_WIDE_MPF", "RB_WIDE_PREFILTER", "RB_FILTER_CHECK", "RB_FILT_DBG",
            "RB_MPF", "RB_NPF", "RB_MPF_M", "RB_PF_SKIP", "RB_NO_RAMP", "RB_SERIAL", "RB_WINDOW_MUL")


@contextlib.contextmanager
def env(**kw):
    """the library reads its switches from the environment on every call"""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update({"RB_MPF": "8", "RB_NPF": "8"})
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def cache_export(gg, which):
    from rnabloom import _native as N
    lg, m = C.c_uint32(), C.c_uint32()
    N.check(N.lib.rb_debug_cache_export(gg.h, which, None, 0, C.byref(lg), C.byref(m)))
    tab = np.full((16 << lg.value) if which == P.MPF else (1 << lg.value), 0xEE, np.uint64)
    N.check(N.lib.rb_debug_cache_export(gg.h, which, _p(tab), tab.size, C.byref(lg), C.byref(m)))
    return tab, lg.value, m.value


def entries(gg, which):
    tab, lg, _ = cache_export(gg, which)
    return P.decode(which, tab, lg)


def prefilter(gg, batch, n_words, first_word=0, ordinal0=ORD0, pos_bits=POSB):
    from rnabloom import _native as N
    cnt, mask = np.full(n_words, 0xDDDDDDDD, np.uint32), np.full(n_words, 0xDDDDDDDD, np.uint32)
    N.check(N.lib.rb_debug_prefilter(gg.h, batch.h, first_word, n_words, ordinal0, pos_bits, _p(cnt), _p(mask)))
    return cnt, mask


# ---- reads ---------------------------------------------------------------------------------------------------------------------
class Reads:
    def __init__(self, seq, qual, lens):
        self.seq, self.qual, self.lens = np.ascontiguousarray(seq), np.ascontiguousarray(qual), np.asarray(lens, np.int64)
        self.off = np.zeros(self.lens.size + 1, np.int64)
        np.cumsum(self.lens, out=self.off[1:])

    def head(self, n):
        return Reads(self.seq[:self.off[n]], self.qual[:self.off[n]], self.lens[:n])

    def revcomp(self):
        from rnabloom import synth
        s, q = self.seq.copy(), self.qual.copy()
        for i in range(self.lens.size):
            a, e = self.off[i], self.off[i + 1]
            s[a:e], q[a:e] = synth.revcomp(self.seq[a:e]), self.qual[a:e][::-1]
        return Reads(s, q, self.lens)


@functools.lru_cache(maxsize=None)
def reads_of(shape, k):
    """the three batch shapes, all from one transcriptome (synth seeds its genome by `seed` alone): uniform 150-base reads (a read per lane);
    320-base reads trimmed to ragged lengths with every edge the parity test uses; reads of more than 32 * RB_READ_WORDS = 320 bases, which
    only the word-per-lane walker k_filter_windows_fast takes"""
    from rnabloom import synth
    L, n = {"uniform": (150, 2600), "ragged": (320, 2600), "long": (400, 300)}[shape]
    d = synth.generate_pairs(n, G=4000, L=L, err=0.002, n_rate=1e-3, seed=91, uniform_expr=True, frag_mean=450.0, frag_sd=30.0)
    reads, quals = d["left"], d["lqual"]
    rng = np.random.default_rng(1000 * k + L)
    if shape == "uniform":
        lens = np.full(n, L)
    elif shape == "ragged":
        lens = np.where(rng.random(n) < 0.6, 150, rng.integers(100, 151, n))
        lens[rng.integers(0, n, 200)] = rng.choice([0, 1, k - 1, k, k + 1, 32, 33, 64, 65, 150, 256, 257, 319, 320], 200)
        lens[:14] = [0, 1, k - 1, k, k + 1, 32, 33, 64, 65, 150, 256, 257, 319, 320]         # every edge among the reads case B walks
    else:
        lens = rng.choice([321, 352, 353, 384, 385, 400], n)
    keep = np.arange(L)[None, :] < lens[:, None]
    return Reads(reads[keep], quals[keep], lens)


@functools.lru_cache(maxsize=None)
def windows_of(shape, k, stranded, rc=False, n=None):
    r = reads_of(shape, k)
    r = r if n is None else r.head(n)
    r = r.revcomp() if rc else r
    return P.usable_windows(r.seq, r.qual, r.off, k, stranded, 2)


def table_of(k, shape, no_mpf, pipe):
    """which table an insert of such a batch looks its k-mers up in (csrc/rb_device.hpp): the minimizer-bucketed one for
    k <= 31; for 32 <= k <= 63 only where a lane takes a whole read (up to 320 bases) and the walker fetches ahead (RB_FILTER_PIPE 1 or 3);
    else — k = 64, RB_NO_MPF — the hash-bucketed one"""
    if no_mpf or k > 63:
        return P.NPF
    if k <= 31:
        return P.MPF
    return P.MPF if shape != "long" and pipe in ("1", "3") else P.NPF


# ---- a graph with a hot cache, checked against the oracle after every insert (case A) ---------------------------------------------------
class World:
    pass


@functools.lru_cache(maxsize=None)
def world(k, stranded, no_mpf):
    """the oracle and the library given the same reads: every shape twice (counters pass exponent 1, the cache is hot), sub-batches of
    15 000 records (many of them feed the cache); after each of the six insert calls both tables are dumped and every entry must be true"""
    from oracle import rbo
    from rnabloom.graph import BloomFilterDeBruijnGraph
    w = World()
    w.k, w.stranded, w.no_mpf = k, stranded, no_mpf
    w.env = {"RB_NO_MPF": "1"} if no_mpf else {}
    w.known, w.n_entries, w.floor_checked = P.Known(2), {P.MPF: 0, P.NPF: 0}, 0
    with env(**w.env):
        w.og = rbo.Graph(*SIZES, 2, 2, 2, k, stranded, False, SEED)
        w.gg = BloomFilterDeBruijnGraph(*SIZES, 2, 2, 2, k, stranded, False, rngSeed=SEED, maxBatchKmers=15_000)
        for shape in ("uniform", "ragged", "long"):
            r = reads_of(shape, k)
            w.known.add(windows_of(shape, k, stranded))
            for second in (False, True):
                hot = hot_kmers(w, shape) if second else None
                w.og.add_reads(r.seq, r.qual, r.off, 3, 0)
                w.gg.addReads(r.seq, r.qual, r.off, 3)
                check_tables(w)
                if second and table_of(k, shape, no_mpf, "3") == P.MPF:
                    w.floor_checked += check_floor(w, shape, hot)
    return w


def hot_kmers(w, shape):
    """the distinct k-mers of a shape's reads whose oracle exponent is >= 1 now: (base hash, a read and a window that hold it)"""
    win = windows_of(shape, w.k, w.stranded)
    h0, first = np.unique(win.h0, return_index=True)
    mn = P.OracleFilters(w.og, SIZES[0], SIZES[1], 2, 2).minimum(win.rows[first])
    sel = P.cache_exp(mn) >= 1
    return h0[sel], win.read[first][sel], win.pos[first][sel]


def check_floor(w, shape, hot):
    """the one coverage floor that needs no measurement: mpf_store takes an empty candidate slot unconditionally and slots are never cleared,
    so a k-mer that was at exponent >= 1 when a sub-batch holding it retired cannot have BOTH candidate slots empty afterwards.  Checked after
    the second insert of a shape for the k-mers that were at exponent >= 1 before that call began: every sub-batch of the call holds reads
    of the same transcriptome at ~5 occurrences per k-mer, so each of them retired in many sub-batches of this call.  Exempt are k-mers that
    reached exponent 1 only during the call — they may have done so in its last two sub-batches, which the producer prefilters one ahead of
    the consumer and which this test cannot tell from the others.  The k-mer's bucket is the reference's restatement of
    the store side's address (prefilter_ref.mpf_bucket_of): where it is wrong the candidates of an uncached k-mer are empty.  Returns the
    number of uncached k-mers that were checked."""
    tab, log2b, m = cache_export(w.gg, P.MPF)
    ent = P.decode_mpf(tab, log2b)
    h0, rd, ps = hot
    r = reads_of(shape, w.k)
    n = 0
    for i in np.flatnonzero(~np.isin(h0, ent.h0)):
        a = int(r.off[rd[i]] + ps[i])
        kmer = r.seq[a:a + w.k].tobytes().upper()
        b = P.mpf_bucket_of(kmer, log2b, m)
        sa, sb = P.mpf_candidates(h0[i])
        assert tab[16 * b + sa] != 0 or tab[16 * b + sb] != 0, \
            "%s reads: k-mer %s (hash %#x, bucket %d) was at exponent >= 1 before the last insert call, has no entry and both candidate slots are empty" % (shape, kmer, h0[i], b)
        n += 1
    # ... and the restated address is the store side's: the k-mers that DO have an entry lie in the bucket it names
    at = dict(zip(ent.h0.tolist(), ent.bucket.tolist()))
    for i in np.flatnonzero(np.isin(h0, ent.h0))[:200]:
        a = int(r.off[rd[i]] + ps[i])
        b = P.mpf_bucket_of(r.seq[a:a + w.k].tobytes().upper(), log2b, m)
        assert at[int(h0[i])] == b, "%s reads: k-mer with hash %#x lies in bucket %d, the reference's address is %d" % (shape, h0[i], at[int(h0[i])], b)
    return n


def check_tables(w):
    filt = P.OracleFilters(w.og, SIZES[0], SIZES[1], 2, 2)
    for which in (P.MPF, P.NPF):
        if which == P.MPF and w.k > 63:
            continue
        w.n_entries[which] = P.check_entries(entries(w.gg, which), w.known, filt)


WORLDS = [(k, False, False) for k in (17, 25, 31, 35, 47, 63, 64)] + [(k, True, False) for k in (17, 25, 31, 35, 47, 63, 64)] + \
         [(k, False, True) for k in (17, 25, 31, 35, 47, 63)]
_wid = lambda w: "k%d-%s-%s" % (w[0], "stranded" if w[1] else "canonical", "npf" if w[2] else "default")


@pytest.mark.parametrize("key", WORLDS, ids=_wid)
def test_every_cache_entry_is_true_of_the_oracle(key):
    """A: never forge, never overstate — decoded from the dump, every entry is the hash of an inserted k-mer that the oracle has in dbgbf
    with a counter exponent of at least the entry's bound; saturated means 127; no hash in two buckets.  Both tables, after every insert call
    (world() raises at the first false entry).  The table an insert of these reads uses must have filled: the check is not vacuous."""
    k, stranded, no_mpf = key
    w = world(*key)
    main = table_of(k, "uniform", no_mpf, "3")
    # (thousands of distinct k-mers at exponent >= 1 for 4096 / 256 slots, and an empty candidate slot is always taken)
    assert w.n_entries[main] >= (100 if main == P.NPF else 1000), w.n_entries
    assert w.og.cbf_bytes().max() >= 24
    if main == P.MPF:       # 4096 slots for more hot k-mers than fit two choices: the floor (check_floor) met uncached k-mers
        assert w.floor_checked > 0
    if k > 63:
        from rnabloom import _native as N
        with pytest.raises(N.NativeError):
            cache_export(w.gg, P.MPF)              # no such table at k = 64: the call fails, it does not hand out an empty dump


@pytest.mark.parametrize("shape", ["uniform", "ragged", "long"])
@pytest.mark.parametrize("key", WORLDS, ids=_wid)
def test_the_keep_mask_is_an_exact_function_of_the_table(key, shape):
    """B: rb_debug_prefilter, then the dump (nothing runs in between: the table is the one the kernel read).  Per window: unusable -> 0;
    usable -> 0 iff the table holds its hash anywhere with bound s and strength(ordinal, position) < s (saturated: always); count = popcount;
    words where no window starts 0 / 0.  Forward reads and their reverse complements (canonical hashing drops both strands alike — and the
    store side's bucket, found through window_min_order, must be the one the walkers roll to), every walker."""
    from rnabloom.graph import ReadBatch
    k, stranded, no_mpf = key
    w = world(*key)
    n = min(NB, reads_of(shape, k).lens.size)
    dropped = {}
    for rc in (False, True):
        r = reads_of(shape, k).head(n)
        r = r.revcomp() if rc else r
        win = windows_of(shape, k, stranded, rc, n)
        batch = ReadBatch.from_ascii(r.seq, r.qual, r.off, 3)
        n_words = int(P.words_of(r.lens)[-1])
        for pipe in ("3", "1", "0"):
            with env(RB_FILTER_PIPE=pipe, **w.env):
                cnt, mask = prefilter(w.gg, batch, n_words)
                which = table_of(k, shape, no_mpf, pipe)
                ent = entries(w.gg, which)
            kept, total = P.check_keep(cnt, mask, win, ent, SEED, ORD0, POSB, "%s, RB_FILTER_PIPE=%s, %s: " % ("revcomp" if rc else "forward", pipe, "Mpf" if which == P.MPF else "Npf"))
            dropped[(rc, pipe)] = total - kept
        batch.close()
    # the check is about something: the table the default walker uses drops windows of the reads it was built from, and on both strands
    assert dropped[(False, "3")] > 0, dropped
    if not stranded:
        assert dropped[(True, "3")] > 0, dropped


@pytest.mark.parametrize("pipe", ["3", "1", "0"])
@pytest.mark.parametrize("key", [(25, False, False), (47, True, False), (63, False, False), (64, False, False), (31, False, True)], ids=_wid)
def test_what_the_debug_call_keeps_is_what_an_insert_sorts(key, pipe):
    """C: one sub-batch (60 reads: 7 560 windows at most, under the 15 000-record bound) through rb_debug_prefilter with the handle's next op
    ordinal and add_range's pos_bits, then inserted for real from the same state: sorted_kmers = sum of the counts, kmers = usable windows.
    Under every RB_FILTER_PIPE: the debug call restates add_range's choice of table and walker, and this is what holds the two together"""
    from rnabloom.graph import ReadBatch
    k, stranded, no_mpf = key
    w = world(*key)
    r = reads_of("uniform", k).head(60)
    win = windows_of("uniform", k, stranded, False, 60)
    batch = ReadBatch.from_ascii(r.seq, r.qual, r.off, 3)
    pos_bits = max(1, int(150 - k).bit_length())                      # smallest b >= 1 with 2^b > max_len - k
    with env(RB_FILTER_PIPE=pipe, **w.env):
        ordinal = w.gg.getOpOrdinal()
        cnt, mask = prefilter(w.gg, batch, 60 * 5, ordinal0=ordinal, pos_bits=pos_bits)
        w.og.add_reads(r.seq, r.qual, r.off, 3, 0)
        st = w.gg.addBatch(batch)
        check_tables(w)
    batch.close()
    assert (cnt == P.popcount32(mask)).all()
    assert st.kmers == win.read.size and st.sorted_kmers == int(cnt.sum()), (st.kmers, win.read.size, st.sorted_kmers, int(cnt.sum()))
    assert 0 < st.sorted_kmers < st.kmers
    assert w.gg.getOpOrdinal() == ordinal + 60


def test_copies_of_one_read_are_dropped_as_far_as_their_entries_allow():
    """D: one clean 150-base read, 4096 copies as one batch, inserted three times at k = 25 (126 distinct k-mers, each at a count of
    thousands after the first pass).  Before the third pass the walk over the first 600 copies must drop exactly what the table allows (B).
    No coverage floor is asserted but the one that follows from mpf_store taking an empty candidate slot unconditionally: a k-mer whose
    exponent was >= 1 when a sub-batch that holds it retired cannot have both candidate slots EMPTY afterwards (slots are never cleared).
    Exempt would be the k-mers of the last two sub-batches of a call — the producer prefilters one sub-batch ahead of the consumer — ; here
    every pass is one sub-batch of its own call, the calls are synchronous, and both passes before the dump count."""
    from oracle import rbo
    from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch
    k, copies = 25, 4096
    rng = np.random.default_rng(2024)
    one = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 150)]
    r = Reads(np.tile(one, copies), np.full(150 * copies, ord("I"), np.uint8), np.full(copies, 150))
    win = P.usable_windows(r.seq[:150 * NB], r.qual[:150 * NB], r.off[:NB + 1], k, False, 2)
    kmers = P.Known(2).add(win)
    assert kmers.h0.size == 126
    with env():
        og = rbo.Graph(*SIZES, 2, 2, 2, k, False, False, SEED)
        gg = BloomFilterDeBruijnGraph(*SIZES, 2, 2, 2, k, False, False, rngSeed=SEED)
        batch = ReadBatch.from_ascii(r.seq, r.qual, r.off, 3)
        for _ in range(2):
            og.add_reads(r.seq, r.qual, r.off, 3, 0)
            st = gg.addBatch(batch)
            assert P.check_entries(entries(gg, P.MPF), kmers, P.OracleFilters(og, SIZES[0], SIZES[1], 2, 2)) <= 126
        assert P.cache_exp(P.OracleFilters(og, SIZES[0], SIZES[1], 2, 2).minimum(kmers.rows)).min() >= 7
        cnt, mask = prefilter(gg, batch, NB * 5)
        tab, log2b, m = cache_export(gg, P.MPF)
        ent = P.decode_mpf(tab, log2b)
        have = np.isin(kmers.h0, ent.h0)
        note = "%d of the 126 k-mers have an entry" % have.sum()
        kept, total = P.check_keep(cnt, mask, win, ent, SEED, ORD0, POSB, note + ": ")
        assert total == 126 * NB and kept < total, note
        for h0 in kmers.h0[~have]:
            p = int(win.pos[np.flatnonzero(win.h0 == h0)[0]])
            b = P.mpf_bucket_of(one[p:p + k].tobytes(), log2b, m)
            sa, sb = P.mpf_candidates(h0)
            assert tab[16 * b + sa] != 0 or tab[16 * b + sb] != 0, "k-mer %#x (window %d, bucket %d): no entry and both candidate slots empty; %s" % (h0, p, b, note)
        og.add_reads(r.seq, r.qual, r.off, 3, 0)
        st = gg.addBatch(batch)
        assert P.check_entries(entries(gg, P.MPF), kmers, P.OracleFilters(og, SIZES[0], SIZES[1], 2, 2)) <= 126
        assert st.kmers == 126 * copies and st.sorted_kmers < st.kmers, note
        assert (gg.exportFilter(1) == og.cbf_bytes()).all()
        batch.close()


def test_the_debug_calls_refuse_what_they_cannot_do():
    from rnabloom import _native as N
    from rnabloom.graph import BloomFilterDeBruijnGraph, ReadBatch
    r = reads_of("ragged", 25).head(40)
    with env():
        gg = BloomFilterDeBruijnGraph(*SIZES, 2, 2, 2, 25, False, False, rngSeed=SEED)
        batch = ReadBatch.from_ascii(r.seq, r.qual, r.off, 3)
        n_words = int(P.words_of(r.lens)[-1])
        woff = P.words_of(r.lens)
        mid = int(woff[np.flatnonzero(r.lens > 32)[0]]) + 1               # the second word of a read
        with pytest.raises(N.NativeError):
            prefilter(gg, batch, n_words - mid, first_word=mid)      # not whole reads
        with pytest.raises(N.NativeError):
            prefilter(gg, batch, n_words + 1)
        tab = np.zeros(16, np.uint64)
        lg, m = C.c_uint32(), C.c_uint32()
        with pytest.raises(N.NativeError):
            N.check(N.lib.rb_debug_cache_export(gg.h, 0, _p(tab), tab.size, C.byref(lg), C.byref(m)))      # too small an array
        assert cache_export(gg, P.MPF)[1:] == (8, 16) and cache_export(gg, P.NPF)[1:] == (8, 0)
        assert not cache_export(gg, P.MPF)[0].any()
        cnt, mask = prefilter(gg, batch, n_words)                    # a cold cache keeps every usable window
        win = P.usable_windows(r.seq, r.qual, r.off, 25, False, 2)
        assert int(cnt.sum()) == win.read.size
        batch.close()
    with env(RB_NPF="0", RB_MPF="0"):
        g0 = BloomFilterDeBruijnGraph(*SIZES, 2, 2, 2, 25, False, False, rngSeed=SEED)
        for which in (P.MPF, P.NPF):
            with pytest.raises(N.NativeError):
                cache_export(g0, which)
