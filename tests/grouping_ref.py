"""Plain numpy reference of the grouping stage's contract (csrc/rb_group.hip, its header comment and csrc/rb_internal.hpp "hand-written
grouping stage"): N (hash, occurrence) records -> occurrences in grouped order, their draw strengths, runs (hash, count, start).

check_grouping() takes the inputs, the outputs and the `info` block of rb_debug_group and raises GroupingError — with the rule that is
broken and the offending index — on the first violation.  Everything is derived from the INPUTS: the live set, the fine bucket of every
record, the order where the stage is deterministic, the keys that must come out as one run, the strengths (from the oracle's rbo_rng31,
not from the library).  reference_grouping() builds a correct grouping the same way (tests/test_grouping_rules.py mutates it).

No GPU in this file."""
import numpy as np

GR_KEY_TOP = 60            # the stage groups on hash bits below this one
GR_TILE = 4096             # records a bucket may have to be grouped in LDS; a larger one is "oversized"
GR_FLAG_DEAD = 1
DEAD_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
DEAD_VAL = np.uint32(0xFFFFFFFF)
FIX_LIST = 64              # hash changes inside groups a bucket's repair list holds
FIX_GROUP = 32             # records of the longest group the repair sorts
INFO_FIELDS = ("T", "t_hi", "t_lo", "l_hi", "l_lo", "fix", "idx_keyed", "n_runs", "n_main", "n_live", "n_big", "largest_big")


class GroupingError(AssertionError):
    def __init__(self, rule, msg):
        super().__init__("[%s] %s" % (rule, msg))
        self.rule = rule


class Info:
    def __init__(self, raw):
        raw = [int(x) for x in raw]
        assert len(raw) == len(INFO_FIELDS)
        for name, x in zip(INFO_FIELDS, raw):
            setattr(self, name, x)

    def raw(self):
        return np.array([getattr(self, f) for f in INFO_FIELDS], np.int64)


def _fail(rule, msg, *args):
    raise GroupingError(rule, msg % args)


def _first(mask):
    return int(np.flatnonzero(mask)[0])


# ---- the fine bucket of a record -------------------------------------------------------------------------------------------
def mulhi64(a, b):
    """floor(a * b / 2^64) for a uint64 array a and an integer 0 <= b < 2^64, in 32-bit limbs (no intermediate exceeds 64 bits)"""
    a = np.asarray(a, np.uint64)
    m, s = np.uint64(0xFFFFFFFF), np.uint64(32)
    b_lo, b_hi = np.uint64(b & 0xFFFFFFFF), np.uint64(b >> 32)
    a_lo, a_hi = a & m, a >> s
    p0, p1, p2, p3 = a_lo * b_lo, a_lo * b_hi, a_hi * b_lo, a_hi * b_hi
    carry = ((p0 >> s) + (p1 & m) + (p2 & m)) >> s
    return p3 + (p1 >> s) + (p2 >> s) + carry


def index_bucket_mul(T, span):
    assert span > (1 << T), "an index-keyed partition needs more indices than fine buckets"
    return (1 << (64 + T)) // span


def index_bucket(keys, T, size, lo, span):
    """min(((key >> 1) % size - lo) * floor(2^(64+T) / span) >> 64, 2^T - 1); an index outside [lo, lo + span) wraps and lands in the last bucket"""
    keys = np.asarray(keys, np.uint64)
    i = (keys >> np.uint64(1)) % np.uint64(size) - np.uint64(lo)
    return np.minimum(mulhi64(i, index_bucket_mul(T, span)), np.uint64((1 << T) - 1)).astype(np.int64)


def index_bucket_exact(key, T, size, lo, span):
    """the same in Python integers"""
    i = (((int(key) >> 1) % size) - lo) % (1 << 64)
    return min((i * ((1 << (64 + T)) // span)) >> 64, (1 << T) - 1)


def fine_bucket(keys, info, idx):
    keys = np.asarray(keys, np.uint64)
    if info.T == 0:
        return np.zeros(keys.size, np.int64)
    if info.idx_keyed:
        return index_bucket(keys, info.T, *idx)
    return ((keys >> np.uint64(GR_KEY_TOP - info.T)) & np.uint64((1 << info.T) - 1)).astype(np.int64)


def local_digits(keys, T, L):
    """the L hash bits right below the T partition bits (what a bucket is sorted on)"""
    keys = np.asarray(keys, np.uint64)
    if L == 0:
        return np.zeros(keys.size, np.int64)
    return ((keys >> np.uint64(GR_KEY_TOP - T - L)) & np.uint64((1 << L) - 1)).astype(np.int64)


# ---- strengths -------------------------------------------------------------------------------------------------------------
_TABLES = {}
_TABLE_MAX = 1 << 20


def _tz(r):
    r |= 0x8000
    return (r & -r).bit_length() - 1


def strengths(vals, seed, ordinal0, pos_bits):
    """ctz(rng31(seed, ordinal0 + (v >> pos_bits), v & (2^pos_bits - 1)) | 0x8000) from the oracle; small occurrence ids go through a
    table that is made once per (seed, ordinal0, pos_bits) and shared by every caller"""
    from oracle import rbo
    f = rbo.lib().rbo_rng31
    vals = np.asarray(vals, np.uint32)
    pm = (1 << pos_bits) - 1
    out = np.empty(vals.size, np.uint8)
    small = vals < _TABLE_MAX
    if small.any():
        need = int(vals[small].max()) + 1
        key = (int(seed), int(ordinal0), int(pos_bits))
        tab = _TABLES.get(key, np.empty(0, np.uint8))
        if tab.size < need:
            ext = [_tz(f(seed, ordinal0 + (v >> pos_bits), v & pm)) for v in range(tab.size, need)]
            tab = np.concatenate([tab, np.array(ext, np.uint8)])
            _TABLES[key] = tab
        out[small] = tab[vals[small]]
    for i in np.flatnonzero(~small):
        v = int(vals[i])
        out[i] = _tz(f(seed, ordinal0 + (v >> pos_bits), v & pm))
    return out


# ---- the order and the runs the inputs imply ---------------------------------------------------------------------------------
def live_mask(keys, vals, flags):
    if not (flags & GR_FLAG_DEAD):
        return np.ones(keys.size, bool)
    return ~((keys == DEAD_KEY) & (vals == DEAD_VAL))


def stable_order(bucket, digits, L, pos):
    """input positions `pos` in the stable order on (fine bucket, local digits)"""
    comp = (bucket[pos] << L) | digits[pos]
    return pos[np.argsort(comp, kind="stable")]


def runs_of(keys_in_order):
    """(start, count) of the maximal runs of equal keys"""
    n = keys_in_order.size
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    head = np.ones(n, bool)
    head[1:] = keys_in_order[1:] != keys_in_order[:-1]
    st = np.flatnonzero(head)
    return st, np.diff(np.append(st, n))


def _cell_stats(cell, k):
    """per record of an array ordered by cell: number of records and of distinct keys in the record's cell"""
    _, inv, size = np.unique(cell, return_inverse=True, return_counts=True)
    o = np.lexsort((k, inv))
    ko, co = k[o], inv[o]
    new = np.ones(k.size, bool)
    new[1:] = (ko[1:] != ko[:-1]) | (co[1:] != co[:-1])
    nkeys = np.bincount(co[new], minlength=size.size)
    return size[inv], nkeys[inv]


def _changes_per_bucket(cell, k, b, nb):
    """hash changes inside groups (neighbours of one cell with different keys), counted per fine bucket"""
    chg = np.zeros(k.size, bool)
    chg[1:] = (k[1:] != k[:-1]) & (cell[1:] == cell[:-1])
    return np.bincount(b[chg], minlength=nb)


def one_run_keys(keys, bucket, info, pos):
    """the keys that must come out as exactly one run (the no-needless-split rules), as {rule: sorted unique keys}"""
    T, L, nb = info.T, info.l_hi + info.l_lo, 1 << info.T
    bsize = np.bincount(bucket[pos], minlength=nb)
    out = {}
    dig = local_digits(keys, T, L)
    o = stable_order(bucket, dig, L, pos)
    k, b = keys[o], bucket[o]
    cell = (b << L) | dig[o]
    csize, ckeys = _cell_stats(cell, k)
    # a key that shares its (fine bucket, local digits) with no other key: at every fix level, in a bucket of any size
    out["one-run-alone"] = np.unique(k[ckeys == 1])
    if info.fix >= 1:
        chg = _changes_per_bucket(cell, k, b, nb)
        ok = (bsize[b] <= GR_TILE) & (chg[b] <= FIX_LIST) & (csize <= FIX_GROUP)
        out["one-run-repair"] = np.unique(k[ok])
    if info.fix >= 2:
        L2 = L + 8
        dig2 = local_digits(keys, T, L2)
        o2 = stable_order(bucket, dig2, L2, pos)
        k2, b2 = keys[o2], bucket[o2]
        cell2 = (b2 << L2) | dig2[o2]
        csize2, ckeys2 = _cell_stats(cell2, k2)
        chg2 = _changes_per_bucket(cell2, k2, b2, nb)
        # a bucket that level 1 could not finish (a full list, a group of more than 32) is sorted again on 8 more bits and repaired on those:
        # a hash alone in its (L + 8)-bit cell is one run either way (where level 1 finished, every hash of the bucket is), and so are the
        # hashes of the short groups that are left when the list holds all the changes of that order
        ok = (bsize[b2] <= GR_TILE) & ((ckeys2 == 1) | ((chg2[b2] <= FIX_LIST) & (csize2 <= FIX_GROUP)))
        out["one-run-repair2"] = np.unique(k2[ok])
    return out


# ---- the checker ---------------------------------------------------------------------------------------------------------
def check_grouping(keys, vals, out, info, *, flags=0, seed=0, ordinal0=0, pos_bits=8, idx=None, ordered=False):
    """keys / vals: the inputs (the live values are distinct).  out: dict with vals_out, tz_out, uniq, counts, starts and, for the export,
    brun, bnr.  info: Info or the 12 integers of rb_debug_group.  idx: (size, lo, span) of an index-keyed call.  ordered: RB_GROUP_ORDERED=1."""
    if not isinstance(info, Info):
        info = Info(info)
    keys = np.ascontiguousarray(keys, np.uint64)
    vals = np.ascontiguousarray(vals, np.uint32)
    n = keys.size
    T, L, nb = info.T, info.l_hi + info.l_lo, 1 << info.T
    if info.T != info.t_hi + info.t_lo or (info.idx_keyed and idx is None):
        _fail("plan", "T = %d, passes of %d + %d bits, index-keyed %d", info.T, info.t_hi, info.t_lo, info.idx_keyed)

    # live set
    live = live_mask(keys, vals, flags)
    pos = np.flatnonzero(live)
    n_live = pos.size
    if info.n_live != n_live:
        _fail("live-count", "the stage reports %d live records, the inputs hold %d of %d", info.n_live, n_live, n)
    lv = vals[pos]
    lo_ = np.argsort(lv, kind="stable")
    lv_sorted = lv[lo_]
    assert n_live < 2 or (lv_sorted[1:] != lv_sorted[:-1]).all(), "the checker needs distinct occurrence ids"
    vout = np.asarray(out["vals_out"], np.uint32)[:n_live]
    vs = np.sort(vout)
    if not np.array_equal(vs, lv_sorted):
        i = _first(vs != lv_sorted)
        _fail("permutation", "the grouped occurrences are not the live ones: sorted position %d holds %d, expected %d", i, vs[i], lv_sorted[i])
    ipos = pos[lo_[np.searchsorted(lv_sorted, vout)]]          # input position of the record at every output position
    kout = keys[ipos]

    # runs
    R = info.n_runs
    if not (0 <= R <= n_live) or (R == 0) != (n_live == 0):
        _fail("run-count", "%d runs for %d live records", R, n_live)
    uniq = np.asarray(out["uniq"], np.uint64)[:R]
    counts = np.asarray(out["counts"], np.uint32)[:R].astype(np.int64)
    starts = np.asarray(out["starts"], np.uint32)[:R].astype(np.int64)
    ro = np.argsort(starts, kind="stable")
    s_, c_, u_ = starts[ro], counts[ro], uniq[ro]
    if R:
        if (c_ < 1).any():
            i = _first(c_ < 1)
            _fail("run-tiling", "run slot %d (start %d) has count %d", ro[i], s_[i], c_[i])
        ends = s_ + c_
        bad = np.concatenate([[s_[0] != 0], s_[1:] != ends[:-1]])
        if bad.any():
            i = _first(bad)
            _fail("run-tiling", "run slot %d starts at %d, the run before it ends at %d", ro[i], s_[i], ends[i - 1] if i else 0)
        if ends[-1] != n_live:
            _fail("run-tiling", "the last run (slot %d) ends at %d of %d live records", ro[-1], ends[-1], n_live)
        rid = np.repeat(np.arange(R), c_)                       # run (in position order) of every output position
        if (kout != u_[rid]).any():
            i = _first(kout != u_[rid])
            _fail("run-key", "position %d (occurrence %d, input %d) has hash %#x in a run of %#x (slot %d)", i, vout[i], ipos[i], kout[i], u_[rid[i]], ro[rid[i]])
        if (u_[1:] == u_[:-1]).any():
            i = _first(u_[1:] == u_[:-1])
            _fail("run-adjacent", "runs at %d and %d are neighbours with the same hash %#x", s_[i], s_[i + 1], u_[i])
        # stability: inside a run the input positions increase
        inside = np.ones(n_live, bool)
        inside[s_] = False
        bad = inside & np.concatenate([[False], ipos[1:] <= ipos[:-1]])
        if bad.any():
            i = _first(bad)
            _fail("stability", "position %d holds input %d behind input %d of the same run", i, ipos[i], ipos[i - 1])

    # bucket order
    bucket = fine_bucket(keys, info, idx)
    bout = bucket[ipos]
    if (bout[1:] < bout[:-1]).any():
        i = _first(bout[1:] < bout[:-1]) + 1
        _fail("bucket-order", "position %d is of fine bucket %d behind one of bucket %d", i, bout[i], bout[i - 1])
    bsize = np.bincount(bucket[pos], minlength=nb)
    n_big, largest = int((bsize > GR_TILE).sum()), int(bsize.max()) if n_live else 0
    if info.n_big != n_big or (n_big and info.largest_big != largest):
        _fail("oversized", "the stage reports %d oversized buckets (largest %d), the inputs give %d (largest %d)", info.n_big, info.largest_big, n_big, largest)

    # exact order where the stage is deterministic: without repair everywhere, and always inside oversized buckets
    dig = local_digits(keys, T, L)
    ref = stable_order(bucket, dig, L, pos)
    exact = np.ones(n_live, bool) if info.fix == 0 else bsize[bout] > GR_TILE
    if exact.any():
        bad = exact & (ipos != ref)
        if bad.any():
            i = _first(bad)
            _fail("exact-order", "position %d holds input %d, the stable order on (bucket, %d local bits) puts input %d there", i, ipos[i], L, ref[i])
        rs, rc = runs_of(keys[ref])
        want = np.stack([rs, rc], 1)[exact[rs]]
        got = np.stack([s_, c_], 1)[exact[s_]]
        if want.shape != got.shape or (want != got).any():
            m = min(len(want), len(got))
            d = np.flatnonzero((want[:m] != got[:m]).any(1))
            i = int(d[0]) if d.size else m
            _fail("exact-runs", "run %d of the deterministic part: expected (start, count) %s, found %s", i,
                  tuple(want[i]) if i < len(want) else None, tuple(got[i]) if i < len(got) else None)

    # no needless split
    if R:
        ku, kc = np.unique(uniq, return_counts=True)
        for rule, must in one_run_keys(keys, bucket, info, pos).items():
            split = must[kc[np.searchsorted(ku, must)] != 1]
            if split.size:
                k0 = split[0]
                _fail(rule, "hash %#x must be one run, it came out as %d (starts %s)", k0, kc[np.searchsorted(ku, k0)], s_[u_ == k0][:8].tolist())

    # strengths
    tz = np.asarray(out["tz_out"], np.uint8)[:n_live]
    want = strengths(vout, seed, ordinal0, pos_bits)
    if (tz != want).any():
        i = _first(tz != want)
        _fail("strength", "position %d (occurrence %d): strength %d, expected %d", i, vout[i], tz[i], want[i])

    # export for the swept stage
    if out.get("brun") is not None:
        brun = np.asarray(out["brun"], np.uint32)[:nb].astype(np.int64)
        bnr = np.asarray(out["bnr"], np.uint32)[:nb].astype(np.int64)
        big = bsize > GR_TILE
        rb = fine_bucket(uniq, info, idx)                       # fine bucket of every run slot
        per = np.bincount(rb, minlength=nb)
        if (bnr[big] != 0).any():
            c = int(np.flatnonzero(big)[_first(bnr[big] != 0)])
            _fail("export", "oversized bucket %d has bnr = %d", c, bnr[c])
        bad = ~big & (bnr != per)
        if bad.any():
            c = _first(bad)
            _fail("export", "bucket %d: bnr = %d, it has %d runs", c, bnr[c], per[c])
        if info.n_main != int(bnr.sum()):
            _fail("export", "n_main = %d, sum(bnr) = %d", info.n_main, int(bnr.sum()))
        sl = ~big & (bnr > 0)
        if ((brun[sl] < 0) | (brun[sl] + bnr[sl] > info.n_main)).any():
            c = int(np.flatnonzero(sl)[_first((brun[sl] + bnr[sl] > info.n_main))])
            _fail("export", "bucket %d: slots [%d, %d) reach beyond n_main = %d", c, brun[c], brun[c] + bnr[c], info.n_main)
        owner = np.repeat(np.flatnonzero(sl), bnr[sl])
        slot = np.repeat(brun[sl], bnr[sl]) + (np.arange(owner.size) - np.repeat(np.cumsum(bnr[sl]) - bnr[sl], bnr[sl]))
        if (rb[slot] != owner).any():
            i = _first(rb[slot] != owner)
            _fail("export", "run slot %d (hash %#x, bucket %d) lies in the slots of bucket %d", slot[i], uniq[slot[i]], rb[slot[i]], owner[i])
        if (~big[rb[info.n_main:]]).any():
            i = info.n_main + _first(~big[rb[info.n_main:]])
            _fail("export", "run slot %d, behind n_main = %d, is of bucket %d, which is not oversized", i, info.n_main, rb[i])
        if ordered and (np.diff(starts[:info.n_main]) <= 0).any():
            i = _first(np.diff(starts[:info.n_main]) <= 0) + 1
            _fail("export-ordered", "run slot %d starts at %d, the slot before it at %d", i, starts[i], starts[i - 1])
    return info


# ---- a correct grouping, built from the inputs --------------------------------------------------------------------------
def reference_grouping(keys, vals, *, T, L, fix=0, flags=0, seed=0, ordinal0=0, pos_bits=8, idx=None, repaired=False):
    """-> (out, info) as rb_debug_group would leave them for a plan of T partition and L local bits: stable order on (fine bucket, local
    digits) — repaired: and on the full hash in the buckets that fit LDS, which is valid at every fix level —, runs in bucket order, those of
    oversized buckets behind all others"""
    keys = np.ascontiguousarray(keys, np.uint64)
    vals = np.ascontiguousarray(vals, np.uint32)
    n = keys.size
    t_hi = T if T <= 10 else (T + 1) // 2
    info = Info([T, t_hi, T - t_hi, (L + 1) // 2, L // 2, fix, int(idx is not None and T > 0), 0, 0, 0, 0, 0])
    pos = np.flatnonzero(live_mask(keys, vals, flags))
    bucket = fine_bucket(keys, info, idx)
    nb = 1 << T
    bsize = np.bincount(bucket[pos], minlength=nb)
    order = stable_order(bucket, local_digits(keys, T, L), L, pos)
    if repaired:
        b = bucket[order]
        cell = (b << L) | local_digits(keys[order], T, L)
        tie = np.where(bsize[b] <= GR_TILE, keys[order], np.uint64(0))
        order = order[np.lexsort((np.arange(order.size), tie, cell))]
    st, cn = runs_of(keys[order])
    rb = bucket[order[st]]
    big = bsize[rb] > GR_TILE
    slot_order = np.concatenate([np.flatnonzero(~big), np.flatnonzero(big)])
    st, cn, rb = st[slot_order], cn[slot_order], rb[slot_order]
    n_main = int((~big).sum())
    bnr = np.bincount(rb[:n_main], minlength=nb)
    brun = np.cumsum(bnr) - bnr
    pad = lambda a, dt: np.concatenate([a.astype(dt), np.zeros(n - a.size, dt)])
    out = {"vals_out": pad(vals[order], np.uint32), "tz_out": pad(strengths(vals[order], seed, ordinal0, pos_bits), np.uint8),
           "uniq": pad(keys[order[st]], np.uint64), "counts": pad(cn, np.uint32), "starts": pad(st, np.uint32),
           "brun": brun.astype(np.uint32), "bnr": bnr.astype(np.uint32)}
    info.n_runs, info.n_main, info.n_live = int(st.size), n_main, int(pos.size)
    info.n_big = int((bsize > GR_TILE).sum())
    info.largest_big = int(bsize.max()) if info.n_big else 0
    return out, info
