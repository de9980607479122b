"""Plain numpy + oracle reference of the no-op prefilter's contract (the cache layout is the one the comments of
csrc/rb_device.hpp describe, restated here from those comments and not from its functions).

An entry of the hot-k-mer cache asserts "this k-mer is in dbgbf and the exponent of its counting-Bloom minimum is >= s".  Two things follow
and both are checked from a dump of the table (rb_debug_cache_export) and the oracle's filters:

  check_entries()   every entry is TRUE: its 64 bits are the base hash of a k-mer that was inserted, the oracle has that k-mer in dbgbf and
                    the exponent of its oracle minimum is at least the entry's bound ("never forge, never overstate"); no hash lives in two
                    buckets.
  expected_keep()   the keep mask of the window walk (rb_debug_prefilter) is an exact function of the table and the shared generator: a usable
                    window is dropped iff the table holds its hash ANYWHERE with bound s and the occurrence's draw strength is below s.  The
                    entry is looked up by hash alone — a walker that rolls to another bucket than the one the store side filed the k-mer
                    under does not find it, and the masks differ.

Strengths come from tests/grouping_ref.py (the oracle's generator), usable windows from the oracle's segmentation.  This file does not import
the library.  No GPU in this file."""
import numpy as np

import grouping_ref as G

MPF, NPF = 0, 1                 # `which` of rb_debug_cache_export
MPF_TOP_BOUND = 11              # exponent code 0 of the minimizer-bucketed table: "11 or more"
NPF_SATURATED = 15              # exponent field 15 of the hash-bucketed table: the minimum stands at 127
_U = np.uint64


class PrefilterError(AssertionError):
    def __init__(self, rule, msg):
        super().__init__("[%s] %s" % (rule, msg))
        self.rule = rule


def _fail(rule, msg, *args):
    raise PrefilterError(rule, msg % args)


class Entries:
    """the non-empty words of a table: bucket, slot inside the bucket, the hash the word stands for, the exponent bound it asserts
    (saturated: the entry says the minimum is 127 — its bound reads NPF_SATURATED)"""

    def __init__(self, which, bucket, slot, h0, bound, saturated, n_slots):
        self.which, self.bucket, self.slot, self.h0, self.bound, self.saturated, self.n_slots = which, bucket, slot, h0, bound, saturated, n_slots

    def __len__(self):
        return self.h0.size


# ---- table dump -> entries ---------------------------------------------------------------------------------------------------
def decode_mpf(tab, log2b):
    """minimizer-bucketed table: 2^log2b buckets of 16 words = 8 bins of an A slot (2 bin) and a B slot (2 bin + 1).
    A slot of bin b: entry = (h0 >> 3) << 3 | code, b = h0 & 7.  B slot of bin b: entry = (h0 >> 6) << 6 | (h0 & 7) << 3 | code,
    b = (h0 >> 3) & 7.  code 1..6 = that exponent, 7 = "7 to 10", 0 = "11 or more".  A zero word is empty."""
    tab = np.ascontiguousarray(tab, np.uint64)
    assert tab.size == 16 << log2b, "a dump of %d words is not 2^%d buckets of 16" % (tab.size, log2b)
    idx = np.flatnonzero(tab)
    e = tab[idx]
    bucket, slot = idx >> 4, idx & 15
    b = (slot >> 1).astype(np.uint64)
    h_a = ((e >> _U(3)) << _U(3)) | b
    h_b = ((((e >> _U(6)) << _U(3)) | b) << _U(3)) | ((e >> _U(3)) & _U(7))
    code = (e & _U(7)).astype(np.int64)
    bound = np.where(code == 0, MPF_TOP_BOUND, code)
    return Entries(MPF, bucket, slot, np.where((slot & 1) == 1, h_b, h_a), bound, np.zeros(idx.size, bool), tab.size)


def decode_npf(tab, log2n):
    """hash-bucketed table: 2^log2n words, 8 per bucket, bucket = low B = log2n - 3 bits of h0, entry = (h0 >> B) << 4 | exponent,
    exponent 1..14, or 15 = saturated.  A zero word is empty."""
    tab = np.ascontiguousarray(tab, np.uint64)
    assert tab.size == 1 << log2n and log2n >= 3
    B = _U(log2n - 3)
    idx = np.flatnonzero(tab)
    e = tab[idx]
    bucket, slot = idx >> 3, idx & 7
    h0 = ((e >> _U(4)) << B) | bucket.astype(np.uint64)
    bound = (e & _U(15)).astype(np.int64)
    return Entries(NPF, bucket, slot, h0, bound, bound == NPF_SATURATED, tab.size)


def decode(which, tab, log2):
    return decode_mpf(tab, log2) if which == MPF else decode_npf(tab, log2)


def bounds_for(ent, h0):
    """per queried hash: (largest bound of an entry with that hash anywhere in the table — 0: none —, whether one of them says saturated)"""
    h0 = np.asarray(h0, np.uint64)
    if len(ent) == 0 or h0.size == 0:
        return np.zeros(h0.size, np.int64), np.zeros(h0.size, bool)
    o = np.lexsort((ent.bound, ent.h0))
    h, b = ent.h0[o], ent.bound[o]
    last = np.append(h[1:] != h[:-1], True)
    hu, bu = h[last], b[last]
    sat_h = np.unique(ent.h0[ent.saturated])
    i = np.minimum(np.searchsorted(hu, h0), hu.size - 1)
    found = hu[i] == h0
    return np.where(found, bu[i], 0), np.isin(h0, sat_h)


# ---- the oracle's side ----------------------------------------------------------------------------------------------------------
def cache_exp(mn):
    """exponent of a counter minimum as an entry states it: (mn >> 3) - 1 (below 1: nothing an entry may say), 15 at the ceiling 127"""
    mn = np.asarray(mn, np.int64)
    return np.where(mn >= 127, NPF_SATURATED, (mn >> 3) - 1)


class Windows:
    """the usable windows of a batch, in read order: read index, window start, hashes [n, h] (column 0 = the base hash)"""

    def __init__(self, read, pos, rows, lens):
        self.read, self.pos, self.rows, self.lens = read, pos, rows, np.asarray(lens, np.int64)

    @property
    def h0(self):
        return self.rows[:, 0]


def usable_windows(seq, qual, off, k, stranded, h, min_q=3):
    """the oracle's notion (rbo.segments: quality threshold, letters outside ACGTU, segments shorter than k) and the oracle's hashes
    (forward hashing on a stranded graph, canonical otherwise)"""
    from oracle import rbo
    seq = np.ascontiguousarray(seq, np.uint8)
    n = len(off) - 1
    rd, ps, rows = [], [], []
    for i in range(n):
        a0, a1 = int(off[i]), int(off[i + 1])
        if a1 - a0 < k:
            continue
        s = seq[a0:a1].tobytes()
        q = None if qual is None else qual[a0:a1].tobytes()
        for a, e in rbo.segments(s, q, k, min_q):
            hh, _ = rbo.hash_region(s, k, h, 0 if stranded else 1, int(a), int(e))
            rows.append(hh)
            rd.append(np.full(len(hh), i, np.int64))
            ps.append(np.arange(a, a + len(hh), dtype=np.int64))
    cat = lambda x, dt, shape: np.concatenate(x) if x else np.zeros(shape, dt)
    return Windows(cat(rd, np.int64, 0), cat(ps, np.int64, 0), cat(rows, np.uint64, (0, h)), np.diff(np.asarray(off, np.int64)))


class OracleFilters:
    """a snapshot of the oracle's dbgbf and cbf"""

    def __init__(self, og, dbg_bits, cbf_bytes, dbg_h, cbf_h):
        self.dbg, self.cbf = og.dbgbf_bytes(), og.cbf_bytes()
        self.dbg_bits, self.cbf_size, self.dbg_h, self.cbf_h = dbg_bits, cbf_bytes, dbg_h, cbf_h

    def contains(self, rows):
        i = (rows[:, :self.dbg_h] >> _U(1)) % _U(self.dbg_bits)
        return (((self.dbg[(i >> _U(3)).astype(np.int64)] >> (i & _U(7)).astype(np.uint8)) & 1) == 1).all(axis=1)

    def minimum(self, rows):
        i = (rows[:, :self.cbf_h] >> _U(1)) % _U(self.cbf_size)
        return self.cbf[i.astype(np.int64)].min(axis=1).astype(np.int64)


class Known:
    """the distinct k-mers the oracle was given so far: base hash (sorted) and all hashes"""

    def __init__(self, h):
        self.h0, self.rows = np.zeros(0, np.uint64), np.zeros((0, h), np.uint64)

    def add(self, win):
        rows = np.concatenate([self.rows, win.rows])
        self.h0, first = np.unique(rows[:, 0], return_index=True)
        self.rows = rows[first]
        return self


# ---- A: every entry is true --------------------------------------------------------------------------------------------------
def check_entries(ent, known, filt):
    """raises PrefilterError on the first entry that is not true of the oracle's filters; returns the number of entries"""
    if len(ent) == 0:
        return 0
    where = lambda i: "bucket %d slot %d (hash %#x, bound %d)" % (ent.bucket[i], ent.slot[i], ent.h0[i], ent.bound[i])
    bad = (ent.bound < 1) | (ent.bound > (NPF_SATURATED if ent.which == NPF else MPF_TOP_BOUND))
    if bad.any():
        _fail("bound", "%s states no exponent an entry can state", where(int(np.flatnonzero(bad)[0])))
    o = np.lexsort((ent.bucket, ent.h0))
    two = (ent.h0[o][1:] == ent.h0[o][:-1]) & (ent.bucket[o][1:] != ent.bucket[o][:-1])
    if two.any():
        i = int(np.flatnonzero(two)[0])
        _fail("two-buckets", "%s and %s hold the same hash", where(int(o[i])), where(int(o[i + 1])))
    j = np.minimum(np.searchsorted(known.h0, ent.h0), max(known.h0.size - 1, 0))
    forged = np.ones(len(ent), bool) if known.h0.size == 0 else known.h0[j] != ent.h0
    if forged.any():
        _fail("forged", "%s is the hash of no k-mer that was inserted (%d such entries of %d)", where(int(np.flatnonzero(forged)[0])), forged.sum(), len(ent))
    rows = known.rows[j]
    absent = ~filt.contains(rows)
    if absent.any():
        _fail("not-in-dbgbf", "%s: the oracle's dbgbf does not hold this k-mer", where(int(np.flatnonzero(absent)[0])))
    mn = filt.minimum(rows)
    wrong = ent.saturated & (mn != 127)
    if wrong.any():
        i = int(np.flatnonzero(wrong)[0])
        _fail("saturated", "%s says saturated, the oracle's minimum is %d", where(i), mn[i])
    over = cache_exp(mn) < ent.bound
    if over.any():
        i = int(np.flatnonzero(over)[0])
        _fail("overstated", "%s: the oracle's minimum is %d, exponent %d", where(i), mn[i], cache_exp(mn)[i])
    return len(ent)


# ---- B: the keep mask is a function of the table -----------------------------------------------------------------------------------
def words_of(lens):
    """first packed word of every read (32 bases per word), and the total"""
    w = np.zeros(len(lens) + 1, np.int64)
    np.cumsum((np.asarray(lens, np.int64) + 31) >> 5, out=w[1:])
    return w


def expected_keep(win, ent, seed, ordinal0, pos_bits):
    """-> (cnt, mask) per packed word, as rb_debug_prefilter reports them: bit (p & 31) of word (p >> 5) of its read is set iff window p
    is usable and not provably a no-op; unusable windows and words in which no window starts read 0"""
    woff = words_of(win.lens)
    mask = np.zeros(int(woff[-1]), np.uint32)
    if win.read.size:
        assert int(win.pos.max()) < (1 << pos_bits) and (int(win.read.max()) + 1) << pos_bits <= 1 << 32, "occurrence ids do not fit"
    bound, sat = bounds_for(ent, win.h0)
    st = G.strengths(((win.read << pos_bits) | win.pos).astype(np.uint32), seed, ordinal0, pos_bits).astype(np.int64)
    keep = ~((bound > 0) & (sat | (st < bound)))
    np.bitwise_or.at(mask, woff[win.read[keep]] + (win.pos[keep] >> 5), (np.uint32(1) << (win.pos[keep] & 31).astype(np.uint32)))
    return popcount32(mask), mask


def popcount32(x):
    x = np.asarray(x, np.uint32)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1).astype(np.uint32)


def check_keep(cnt, mask, win, ent, seed, ordinal0, pos_bits, what=""):
    """raises PrefilterError on the first word whose count or mask is not what the table and the generator imply"""
    cnt, mask = np.asarray(cnt, np.uint32), np.asarray(mask, np.uint32)
    e_cnt, e_mask = expected_keep(win, ent, seed, ordinal0, pos_bits)
    if mask.size != e_mask.size:
        _fail("words", "%s%d words reported, the batch has %d", what, mask.size, e_mask.size)
    if (cnt != popcount32(mask)).any():
        i = int(np.flatnonzero(cnt != popcount32(mask))[0])
        _fail("count", "%sword %d: count %d, mask %08x", what, i, cnt[i], mask[i])
    if (mask != e_mask).any():
        bad = np.flatnonzero(mask != e_mask)
        i = int(bad[0])
        woff = words_of(win.lens)
        r = int(np.searchsorted(woff, i, side="right") - 1)
        extra, lost = int((mask[bad] & ~e_mask[bad]).any()), int((e_mask[bad] & ~mask[bad]).any())
        _fail("mask", "%s%d of %d words differ (kept where the table says drop: %d, dropped where it does not: %d); first: word %d (read %d, bases %d..), "
              "mask %08x, expected %08x", what, bad.size, mask.size, extra, lost, i, r, 32 * (i - int(woff[r])), mask[i], e_mask[i])
    return int(e_cnt.sum()), int(win.read.size)


# ---- where the store side files a k-mer (needed by one check only: the empty-candidate floor) --------------------------------------
def _mix_order(canon):
    x = (canon * 0x9E3779B1) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x85EBCA77) & 0xFFFFFFFF
    x ^= x >> 13
    return x


def mpf_bucket_of(kmer, log2b, m):
    """bucket of a k-mer (ACGT bytes) in the minimizer-bucketed table: the smallest mixed order among the canonical m-mers of its middle
    21 (k odd) / 20 (k even) bases — of the whole k-mer for k <= 21 —, mixed once more and masked (csrc/rb_device.hpp: mmer_order, mpf_kp,
    mpf_lag, window_min_order, mpf_bucket; restated: a k-mer WITHOUT an entry has no other way to its candidate slots)"""
    code = {65: 0, 67: 1, 71: 2, 84: 3, 85: 3}
    k = len(kmer)
    kp = k if k <= 21 else 21 - ((k & 1) ^ 1)
    lag = (k - kp) >> 1
    c = [code[x] for x in kmer[lag:lag + kp]]
    best = 0xFFFFFFFF
    for j in range(kp - m + 1):
        f = r = 0
        for t in range(m):
            f = (f << 2) | c[j + t]
            r = (r << 2) | (3 - c[j + m - 1 - t])
        best = min(best, _mix_order(min(f, r)))
    x = (best * 0xC2B2AE3D) & 0xFFFFFFFF
    x ^= x >> 16; x = (x * 0x27D4EB2F) & 0xFFFFFFFF
    x ^= x >> 15
    return x & ((1 << log2b) - 1)


def mpf_candidates(h0):
    """the two slots of a bucket a k-mer may live in: the A slot of bin (h0 & 7), the B slot of bin ((h0 >> 3) & 7)"""
    h0 = int(h0)
    return 2 * (h0 & 7), 2 * ((h0 >> 3) & 7) + 1
