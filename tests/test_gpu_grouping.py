"""The grouping stage of the insert pipeline (csrc/rb_group.hip: group_records_device) run directly on host arrays through
rb_debug_group and checked against the plain numpy reference of its contract (tests/grouping_ref.py): live set, runs, stability, bucket
order, the exact order where the stage is deterministic, no needless split, strengths (from the oracle), the export for the swept stage.
The shapes are the smallest at which each mechanism engages: a bucket of 4096 / 4097 records, runs against the 4096-record pieces of an
oversized bucket, groups of 32 / 33 records that agree in every sorted bit, 64 / 65 hash changes in a bucket, a tile of cancelled
records, empty first-pass buckets.  Whole inserts tolerate split runs by design, so none of this shows in the filter comparisons."""
import ctypes as C

import numpy as np
import pytest

import grouping_ref as G

pytestmark = pytest.mark.gpu

SEED, ORD0, POSB = 0x5EED5EED5EED, (1 << 33) + 12345, 8      # (an ordinal beyond 32 bits)
ENV = ("T", "FIX", "TPB", "ORDERED", "PREFETCH", "CLASSES", "WIDE_LDS", "XCD", "GRID", "TARGET")
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for e in ENV:
        monkeypatch.delenv("RB_GROUP_" + e, raising=False)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run_group(keys, vals, *, group_bits=64, bucket_target=0, flags=0, idx=None, export=False):
    from rnabloom import _native as N
    keys = np.ascontiguousarray(keys, np.uint64)
    vals = np.ascontiguousarray(vals, np.uint32)
    n = keys.size
    out = {"vals_out": np.empty(n, np.uint32), "tz_out": np.empty(n, np.uint8), "uniq": np.empty(n, np.uint64),
           "counts": np.empty(n, np.uint32), "starts": np.empty(n, np.uint32),
           "brun": np.empty(1 << 20, np.uint32) if export else None, "bnr": np.empty(1 << 20, np.uint32) if export else None}
    info = np.zeros(12, np.int64)
    size, lo, span = idx if idx else (0, 0, 0)
    N.check(N.lib.rb_debug_group(0, _p(keys), _p(vals), n, group_bits, bucket_target, flags, SEED, ORD0, POSB, size, lo, span,
                                 _p(out["vals_out"]), _p(out["tz_out"]), _p(out["uniq"]), _p(out["counts"]), _p(out["starts"]),
                                 _p(out["brun"]), _p(out["bnr"]), _p(info)))
    return out, G.Info(info)


def group_and_check(keys, vals, *, ordered=False, **kw):
    out, info = run_group(keys, vals, **kw)
    G.check_grouping(keys, vals, out, info, flags=kw.get("flags", 0), seed=SEED, ordinal0=ORD0, pos_bits=POSB, idx=kw.get("idx"), ordered=ordered)
    return out, info


def _vals(rng, n):
    return rng.permutation(n).astype(np.uint32)          # a permutation, not arange: value order and input order differ


def _rand64(rng, n):
    return rng.integers(0, 2**64, n, dtype=np.uint64)


def _dups(rng, n):
    """random 64-bit hashes, a third of the records duplicates of others"""
    k = _rand64(rng, n)
    if n >= 3:
        k[rng.integers(0, n, n // 3)] = k[rng.integers(0, n, n // 3)]
    return k


def _zipf(rng, n):
    """run lengths of every class the bucket kernel orders by (1, 2, 3-4, 5-8, ... 65+), shuffled"""
    lens = np.array([1] * 30 + [2] * 10 + [3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130])
    reps = lens[rng.integers(0, lens.size, n // 4 + 1)]
    k = np.repeat(_rand64(rng, reps.size), reps)
    k = np.concatenate([k, _rand64(rng, max(0, n - k.size))])[:n]
    return k[rng.permutation(n)]


def _runs_of_key(out, info, key):
    m = out["uniq"][:info.n_runs] == np.uint64(key)
    return out["starts"][:info.n_runs][m], out["counts"][:info.n_runs][m]


# ---- one bucket: 4096 is the last size that fits LDS, 4097 the smallest oversized bucket ------------------------------------
@pytest.mark.parametrize("mix", ["random", "distinct", "equal", "half"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4095, 4096, 4097, 8192, 8193, 12289])
def test_single_bucket(monkeypatch, n, mix):
    monkeypatch.setenv("RB_GROUP_T", "0")
    rng = np.random.default_rng(n * 7 + len(mix))
    if mix == "random":
        keys = _rand64(rng, n // 3 + 1)[rng.integers(0, n // 3 + 1, n)]
    elif mix == "distinct":
        keys = np.unique(_rand64(rng, 2 * n + 8))[:n][rng.permutation(n)]
    elif mix == "equal":
        keys = np.full(n, 0x0123456789ABCDEF, np.uint64)
    else:
        keys = _rand64(rng, n)
        keys[rng.permutation(n)[: (n + 1) // 2]] = np.uint64(0x0FEDCBA987654321)
    out, info = group_and_check(keys, _vals(rng, n))
    assert info.T == 0 and info.l_hi + info.l_lo == 16 and info.fix == 1
    assert info.n_big == (1 if n > 4096 else 0) and info.largest_big == (n if n > 4096 else 0)
    if mix == "equal":
        assert info.n_runs == 1
    if mix == "half":
        assert _runs_of_key(out, info, 0x0FEDCBA987654321)[1].tolist() == [(n + 1) // 2]


# ---- an oversized bucket: a hot hash against the 4096-record pieces ---------------------------------------------------------
@pytest.mark.parametrize("start,length,behind", [(4096, 4096, 1000), (4095, 4098, 500), (4097, 4094, 700), (3000, 20000, 1577), (100, 5000, 3093)])
def test_hot_run_against_piece_boundaries(monkeypatch, start, length, behind):
    """the hot hash occupies sorted positions [start, start + length) of the one bucket: exactly one run, wherever the pieces cut
    ((100, 5000, 3093): 8193 records, the last piece holds one)"""
    monkeypatch.setenv("RB_GROUP_T", "0")
    rng = np.random.default_rng(start + length)
    d = 0x7000                                               # the hot hash's 16 local bits (bits 44 .. 59)
    low = lambda m: rng.integers(0, 1 << 44, m, dtype=np.uint64)
    hot = (np.uint64(d) << np.uint64(44)) | np.uint64(0xABCDE)
    keys = np.concatenate([(rng.integers(0, d, start).astype(np.uint64) << np.uint64(44)) | low(start), np.full(length, hot, np.uint64),
                           (rng.integers(d + 1, 1 << 16, behind).astype(np.uint64) << np.uint64(44)) | low(behind)])
    n = keys.size
    keys = keys[rng.permutation(n)]
    out, info = group_and_check(keys, _vals(rng, n))
    assert info.n_big == 1 and info.largest_big == n
    st, cn = _runs_of_key(out, info, hot)
    assert st.tolist() == [start] and cn.tolist() == [length]


# ---- the plan an insert gets ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", ["dups", "zipf"])
@pytest.mark.parametrize("n", [3072, 3073, 4096, 50_001, 300_007])
def test_default_plan(n, mix):
    rng = np.random.default_rng(n + len(mix))
    keys = _dups(rng, n) if mix == "dups" else _zipf(rng, n)
    out, info = group_and_check(keys, _vals(rng, n))
    assert info.T == max(0, int(np.ceil(np.log2(n / 3072)))) and info.fix == 1 and not info.idx_keyed
    if mix == "zipf" and n >= 50_001:                        # the by-class run ordering engages: buckets of more than 64 runs of mixed lengths
        assert info.n_runs / (1 << info.T) > 64 and info.n_runs < n


@pytest.mark.parametrize("switch", ["CLASSES=0", "PREFETCH=0", "ORDERED=1", "TPB=256"])
def test_default_plan_with_a_switch(monkeypatch, switch):
    name, value = switch.split("=")
    monkeypatch.setenv("RB_GROUP_" + name, value)
    rng = np.random.default_rng(50_001 + len("zipf"))
    keys = _zipf(rng, 50_001)
    out, info = group_and_check(keys, _vals(rng, 50_001), export=True, ordered=name == "ORDERED")
    assert info.n_main == info.n_runs and info.n_big == 0


# ---- partition widths -----------------------------------------------------------------------------------------------------
N_WIDTH = 200_003


@pytest.fixture(scope="module")
def width_inputs():
    rng = np.random.default_rng(200_003)
    return _dups(rng, N_WIDTH), _vals(rng, N_WIDTH)


@pytest.mark.parametrize("wide", [None, "0"])
@pytest.mark.parametrize("T", [1, 8, 9, 10, 11, 18, 20])
def test_partition_widths(monkeypatch, width_inputs, T, wide):
    """9 and 10 bits: the wide rank path; 11: the smallest two-pass plan; 18 and 20: most fine buckets, and some first-pass buckets, are empty"""
    monkeypatch.setenv("RB_GROUP_T", str(T))
    if wide is not None:
        monkeypatch.setenv("RB_GROUP_WIDE_LDS", wide)
    keys, vals = width_inputs
    out, info = group_and_check(keys, vals)
    assert info.T == T and (info.t_hi, info.t_lo) == ((T, 0) if T <= 10 else ((T + 1) // 2, T // 2))
    assert info.n_big == (2 if T == 1 else 0)


@pytest.mark.parametrize("T", [11, 18])
@pytest.mark.parametrize("skew", ["one-segment", "two-buckets", "outside-bits"])
def test_partition_skew(monkeypatch, T, skew):
    monkeypatch.setenv("RB_GROUP_T", str(T))
    rng = np.random.default_rng(T + len(skew))
    n = 30_011
    t_hi = (T + 1) // 2
    keys = _dups(rng, n)
    below = np.uint64((1 << (60 - T)) - 1)
    if skew == "one-segment":        # every hash has the same top t_hi partition bits: the second pass has one segment, every other one is empty
        keys = (keys & np.uint64(~(((1 << t_hi) - 1) << (60 - t_hi)) & (2**64 - 1))) | (np.uint64(5) << np.uint64(60 - t_hi))
    elif skew == "two-buckets":      # two fine buckets, 3000 records and the rest (oversized)
        b = np.where(np.arange(n) < 3000, 77, (1 << T) - 3).astype(np.uint64)
        keys = (keys & below) | (b[rng.permutation(n)] << np.uint64(60 - T))
    else:
        # hashes that differ only in bits 60-63 and bit 0 — outside every sorted bit — are still different hashes: 16 of them, two records
        # each (a group of 32: repaired), and a pair of 100 records each (too long a group to repair: it may stay split, but never merged)
        base = np.uint64(0x0123456789ABCDE0)
        g32 = base | (np.arange(16, dtype=np.uint64) >> np.uint64(1) << np.uint64(61)) | (np.arange(16, dtype=np.uint64) & np.uint64(1))
        g32 = np.tile(g32, 2)
        base2 = np.uint64(0x0765432101234560)
        pair = np.tile(np.array([base2, base2 | np.uint64(1) | (np.uint64(9) << np.uint64(60))], np.uint64), 100)
        keys[rng.permutation(n)[:232]] = np.concatenate([g32, pair])
    out, info = group_and_check(keys, _vals(rng, n))
    assert info.T == T and info.t_lo > 0 and info.fix == 1
    if skew == "two-buckets":
        assert info.n_big == 1 and info.largest_big == n - 3000
    if skew == "outside-bits":
        for k in g32[:16]:
            assert _runs_of_key(out, info, k)[1].tolist() == [2]
        assert sum(_runs_of_key(out, info, k)[1].sum() for k in np.unique(pair)) == 200


# ---- repair of interleaved hashes -------------------------------------------------------------------------------------------
def _repair_inputs(variant):
    """4 fine buckets (RB_GROUP_T=2, 16 local bits: 42 .. 57) of hashes with distinct local digits, plus groups of 2-4 hashes that agree in
    every sorted bit, interleaved: bucket 0 groups of 2, 31 and 32 records; bucket 1 groups of 33, 200 and 4; bucket 2 exactly 64 hash changes
    inside groups (what the repair list holds); bucket 3 exactly 65.  variant "next8": the hashes of a group differ in the 8 bits below the
    sorted ones (level 2 sorts on them); "below": only below those."""
    rng = np.random.default_rng(len(variant))
    sh = np.uint64(34 if variant == "next8" else 3)
    keys, groups, expect = [], [], {}
    used = [set() for _ in range(4)]

    def group(bucket, name, n_keys, size, pattern):
        d = int(rng.integers(0, 1 << 16))
        while d in used[bucket]:
            d = int(rng.integers(0, 1 << 16))
        used[bucket].add(d)
        base = (np.uint64(bucket) << np.uint64(58)) | (np.uint64(d) << np.uint64(42)) | np.uint64(int(rng.integers(0, 1 << 34)) & ~(0xFF << 3))
        ks = base | ((np.arange(n_keys, dtype=np.uint64) + np.uint64(1)) << sh)
        g = ks[np.array([pattern(i) % n_keys for i in range(size)])]
        groups.append((len(keys), g))
        keys.append(g)
        expect.setdefault(name, []).extend(np.unique(g).tolist())

    group(0, "g2", 2, 2, lambda i: i)
    group(0, "g31", 3, 31, lambda i: i // 4)
    group(0, "g32", 4, 32, lambda i: i // 3)
    group(1, "g33", 3, 33, lambda i: i // 5)
    group(1, "g200", 2, 200, lambda i: i // 40)
    group(1, "g4", 2, 4, lambda i: i)                        # (a short group in a bucket that level 2 sorts again: it stays repaired)
    for _ in range(32):
        group(2, "c64", 2, 3, lambda i: i)                   # A B A: two changes each
    for _ in range(32):
        group(3, "c65", 2, 3, lambda i: i)
    group(3, "c65", 2, 2, lambda i: i)                       # the 65th
    n_bg = 1800
    for b in range(4):
        free = np.array(sorted(set(range(1 << 16)) - used[b]))
        d = rng.choice(free, n_bg, replace=False).astype(np.uint64)
        keys.append((np.uint64(b) << np.uint64(58)) | (d << np.uint64(42)) | rng.integers(0, 1 << 42, n_bg, dtype=np.uint64))
    sizes = [k.size for k in keys]
    keys = np.concatenate(keys)
    # a random input order that keeps every group's own order (the interleaving is the point)
    r = rng.random(keys.size)
    o = 0
    for s in sizes[:len(groups)]:
        r[o:o + s] = np.sort(r[o:o + s])
        o += s
    order = np.argsort(r, kind="stable")
    return keys[order], _vals(rng, keys.size), expect


@pytest.mark.parametrize("variant", ["next8", "below"])
@pytest.mark.parametrize("fix", [0, 1, 2])
def test_repair_levels(monkeypatch, fix, variant):
    monkeypatch.setenv("RB_GROUP_T", "2")
    monkeypatch.setenv("RB_GROUP_FIX", str(fix))
    keys, vals, expect = _repair_inputs(variant)
    out, info = group_and_check(keys, vals, group_bits=64)
    assert (info.T, info.l_hi + info.l_lo, info.fix, info.n_big) == (2, 16, fix, 0)
    # the scenario is what it claims to be: which groups the reference holds to one run per hash at this level
    must = G.one_run_keys(keys, G.fine_bucket(keys, info, None), info, np.arange(keys.size))
    held = set().union(*(set(v.tolist()) for name, v in must.items() if name != "one-run-alone"))
    small = ["g2", "g31", "g32", "g4", "c64"]
    want = {0: [], 1: small, 2: small + (["g33", "g200", "c65"] if variant == "next8" else [])}[fix]
    for name, ks in expect.items():
        assert set(ks) <= held if name in want else not (set(ks) & held), (name, fix, variant)
    if fix == 0:                     # nothing is repaired: every interleaved group is as split as the stable order leaves it
        for name in ("g31", "g32", "g33", "g200", "c64", "c65"):
            assert all(len(_runs_of_key(out, info, k)[0]) > 1 for k in expect[name][:1]), name


@pytest.mark.parametrize("group_bits", [1, 8, 20])
def test_fewer_grouping_bits_give_the_stable_order(width_inputs, group_bits):
    keys, vals = width_inputs
    out, info = group_and_check(keys, vals, group_bits=group_bits)
    assert info.fix == 0 and info.T == min(7, group_bits) and info.l_hi + info.l_lo == min(16, group_bits - info.T)
    assert info.n_big == (2 if group_bits == 1 else 0)


# ---- cancelled records -------------------------------------------------------------------------------------------------------
# A sub-batch with NO live record does not reach the stage today: no caller passes GR_FLAG_DEAD yet (group_enqueue's callers in rb_graph.hip
# and rb_shard.hip leave flags at 0, and rb_batch.hip's emit pass writes no cancelled record), group_enqueue returns before the stage for
# N == 0, and group_records_device refuses N == 0.  So there is no all-cancelled case here; the closest the flag's contract reaches is one
# live record.
@pytest.mark.parametrize("plan", ["default", "T=0", "T=11"])
@pytest.mark.parametrize("layout", ["edges-tile-ones", "all-but-one", "none", "first", "last"])
def test_cancelled_records(monkeypatch, plan, layout):
    if plan != "default":
        monkeypatch.setenv("RB_GROUP_T", plan[2:])
    rng = np.random.default_rng(len(plan) * 10 + len(layout))
    n = 20_011
    keys, vals = _dups(rng, n), _vals(rng, n)
    dead = np.zeros(n, bool)
    if layout == "edges-tile-ones":
        dead[0] = dead[-1] = True
        dead[4096:8192] = True                               # a whole tile of the first partition pass
        keys[[1, 4095, 8192, n - 2]] = ONES                  # live all-ones hashes next to cancelled records
        keys[9000] = ONES; vals[9001] = 0xFFFFFFFF           # ... and an all-ones occurrence id under an ordinary hash: live as well
    elif layout == "all-but-one":
        dead[:] = True
        dead[12_345] = False
    elif layout == "first":
        dead[0] = True
    elif layout == "last":
        dead[-1] = True
    keys[dead] = ONES
    vals[dead] = 0xFFFFFFFF
    out, info = group_and_check(keys, vals, flags=G.GR_FLAG_DEAD)
    assert info.n_live == n - dead.sum()
    assert info.T == {"default": 3, "T=0": 1, "T=11": 11}[plan]        # (cancelled records leave in a partition pass: T = 0 becomes 1)
    if layout == "edges-tile-ones":
        assert _runs_of_key(out, info, ONES)[1].tolist() == [5]
    if layout == "all-but-one":
        assert info.n_runs == 1 and out["vals_out"][0] == vals[12_345]


# ---- index-keyed partition and the export for the swept stage -----------------------------------------------------------------
SIZE = 1_000_003


def _keys_with_index(rng, idx):
    idx = np.asarray(idx, np.uint64)
    return (idx + np.uint64(SIZE) * rng.integers(0, 2**62 // SIZE, idx.size).astype(np.uint64)) * np.uint64(2) + rng.integers(0, 2, idx.size).astype(np.uint64)


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("T", [3, 10, 11, 18])
def test_index_keyed_whole_filter(monkeypatch, T, ordered):
    monkeypatch.setenv("RB_GROUP_T", str(T))
    if ordered:
        monkeypatch.setenv("RB_GROUP_ORDERED", "1")
    rng = np.random.default_rng(T)
    n = 50_001
    keys = _keys_with_index(rng, rng.integers(0, SIZE, n))
    keys[rng.integers(0, n, n // 3)] = keys[rng.integers(0, n, n // 3)]
    if T >= 10:                      # one oversized index range: 5000 records of indices inside fine bucket 2^T / 3
        c = (1 << T) // 3
        first = -(-c * SIZE >> T) + 1
        keys[rng.permutation(n)[:5000]] = _keys_with_index(rng, first + rng.integers(0, max(1, (SIZE >> T) - 2), 5000))
    out, info = group_and_check(keys, _vals(rng, n), idx=(SIZE, 0, SIZE), export=True, ordered=ordered)
    assert info.T == T and info.idx_keyed == 1
    assert info.n_big == (8 if T == 3 else 1) and 0 <= info.n_main < info.n_runs
    if T >= 10:
        assert info.largest_big >= 5000


def test_index_keyed_shard_range_and_hash_keyed_fallback(monkeypatch):
    monkeypatch.setenv("RB_GROUP_T", "10")
    rng = np.random.default_rng(10)
    n = 50_001
    lo, span = SIZE // 3, SIZE // 4
    keys = _keys_with_index(rng, lo + rng.integers(0, span, n))
    keys[[0, 1, 2, 3]] = _keys_with_index(rng, [lo, lo, lo + span - 1, lo + span - 1])      # the range's first and last index
    vals = _vals(rng, n)
    out, info = group_and_check(keys, vals, idx=(SIZE, lo, span), export=True)
    assert info.idx_keyed == 1 and info.n_big == 0 and info.n_main == info.n_runs
    assert (out["bnr"][: 1 << 10] > 0).all()
    # no more indices than fine buckets: the partition goes by the hash bits
    out, info = group_and_check(keys, vals, idx=(SIZE, lo, 1 << 10), export=True)
    assert info.idx_keyed == 0 and info.T == 10
    out, info = group_and_check(keys, vals, idx=(SIZE, lo, (1 << 10) + 1))
    assert info.idx_keyed == 1 and info.n_big >= 1           # (nearly every index lies behind the range: the last bucket takes them)
