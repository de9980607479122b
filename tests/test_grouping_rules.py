"""The grouping checker (tests/grouping_ref.py) against itself, without a GPU: a grouping built by the reference passes, and every
way a subtly wrong grouping kernel could come out — one mutation at a time — is rejected, by the rule that is meant to catch it.
Plus the 128-bit-safe numpy form of the index-bucket formula against Python integers."""
import copy

import numpy as np
import pytest

import grouping_ref as G

SEED, ORD0, POSB = 5, 1000, 7
T, L = 3, 16
ONES = 0xFFFFFFFFFFFFFFFF


def _key(bucket, local, rest):
    return (np.uint64(bucket) << np.uint64(60 - T)) | (np.uint64(local) << np.uint64(60 - T - L)) | np.uint64(rest)


def _inputs():
    """8 fine buckets: 0-4 and 6 ordinary (duplicated hashes, a third of the records), 5 oversized with a hot hash, 7 with interleaved
    hashes that agree in every sorted bit, live all-ones hashes and cancelled records"""
    rng = np.random.default_rng(11)
    keys = []
    for b in (0, 1, 2, 3, 4, 6):
        pool = _key(b, rng.integers(0, 1 << L, 700), rng.integers(0, 1 << 41, 700))
        keys.append(pool[rng.integers(0, 700, 2100)])
    pool = _key(5, rng.integers(0, 1 << L, 900), rng.integers(0, 1 << 41, 900))
    keys.append(np.concatenate([pool[rng.integers(0, 900, 3000)], np.repeat(_key(5, 0x8000, 77), 2500)]))
    grp = [_key(7, 0x1234, r) for r in (1, 2, 3)]                       # a group of 3 hashes x 8 records, interleaved
    keys.append(np.array(grp * 8, np.uint64))
    keys.append(_key(7, rng.integers(0, 1 << 15, 500), rng.integers(0, 1 << 41, 500)))
    keys.append(np.full(6, ONES, np.uint64))                            # 3 live all-ones hashes and 3 cancelled records (values below)
    keys = np.concatenate(keys)
    n = keys.size
    sh = rng.permutation(n)
    keys = keys[sh]
    vals = rng.permutation(n).astype(np.uint32)
    ones = np.flatnonzero(keys == np.uint64(ONES))
    vals[ones[:3]] = 0xFFFFFFFF
    return keys, vals


KEYS, VALS = _inputs()
KW = dict(flags=G.GR_FLAG_DEAD, seed=SEED, ordinal0=ORD0, pos_bits=POSB)


@pytest.fixture(scope="module")
def good():
    """a correct grouping that is valid at every fix level, claimed at level 1 (the exact-order rule then binds in the oversized bucket only)"""
    out, info = G.reference_grouping(KEYS, VALS, T=T, L=L, fix=1, repaired=True, **KW)
    G.check_grouping(KEYS, VALS, out, info, **KW)
    return out, info


def _mutant(good):
    out, info = good
    return {k: v.copy() for k, v in out.items()}, copy.copy(info)


def _rejected(out, info, *rules):
    with pytest.raises(G.GroupingError) as e:
        G.check_grouping(KEYS, VALS, out, info, **KW)
    assert e.value.rule in rules, str(e.value)


def _run_of(out, info, pred):
    """first run slot with pred(hash, start, count)"""
    for r in range(info.n_runs):
        if pred(int(out["uniq"][r]), int(out["starts"][r]), int(out["counts"][r])):
            return r
    raise AssertionError("the fixture has no such run")


def _swap(out, i, j):
    for name in ("vals_out", "tz_out"):
        out[name][[i, j]] = out[name][[j, i]]


def test_reference_grouping_passes_at_every_fix_level():
    assert (KEYS == np.uint64(ONES)).sum() == 6 and G.live_mask(KEYS, VALS, G.GR_FLAG_DEAD).sum() == KEYS.size - 3
    for fix, repaired in ((0, False), (1, True), (2, True)):
        out, info = G.reference_grouping(KEYS, VALS, T=T, L=L, fix=fix, repaired=repaired, **KW)
        assert info.n_big == 1 and info.largest_big == 5500 and info.n_live == KEYS.size - 3
        G.check_grouping(KEYS, VALS, out, info, **KW)
        G.check_grouping(KEYS, VALS, out, info, ordered=True, **KW)
    # the unrepaired order is what level 0 must give — and it is not good enough at level 1: the interleaved group of bucket 7 is split
    out, info = G.reference_grouping(KEYS, VALS, T=T, L=L, fix=1, repaired=False, **KW)
    _rejected(out, info, "one-run-repair")
    # ... and the repaired order is not what level 0 gives
    out, info = G.reference_grouping(KEYS, VALS, T=T, L=L, fix=0, repaired=True, **KW)
    _rejected(out, info, "exact-order")


def test_two_records_of_one_run_swapped(good):
    out, info = _mutant(good)
    r = _run_of(out, info, lambda u, s, c: c >= 3)
    s = int(out["starts"][r])
    _swap(out, s, s + 1)
    _rejected(out, info, "stability")
    # inside the hot run of the oversized bucket the exact order binds as well
    out, info = _mutant(good)
    r = _run_of(out, info, lambda u, s, c: c == 2500)
    s = int(out["starts"][r])
    _swap(out, s + 1000, s + 1001)
    _rejected(out, info, "stability", "exact-order")


def test_two_records_of_different_runs_swapped(good):
    out, info = _mutant(good)
    r = _run_of(out, info, lambda u, s, c: c >= 2 and s > 0)
    s = int(out["starts"][r])
    _swap(out, s - 1, s)
    _rejected(out, info, "run-key")


def test_run_boundary_moved_by_one(good):
    out, info = _mutant(good)
    r = _run_of(out, info, lambda u, s, c: c >= 2 and s > 0)
    prev = int(np.flatnonzero(out["starts"][:info.n_runs] + out["counts"][:info.n_runs] == out["starts"][r])[0])
    out["starts"][r] += 1; out["counts"][r] -= 1; out["counts"][prev] += 1
    _rejected(out, info, "run-key")
    out, info = _mutant(good)
    out["counts"][r] -= 1                                               # a gap instead
    _rejected(out, info, "run-tiling")


def _split(out, info, r, at):
    """run slot r cut `at` records behind its start; the second half gets a new slot at the end"""
    R = info.n_runs
    out["uniq"][R] = out["uniq"][r]
    out["starts"][R] = out["starts"][r] + at
    out["counts"][R] = out["counts"][r] - at
    out["counts"][r] = at
    info.n_runs += 1


def test_run_split_where_the_no_split_rule_applies(good):
    # a hash alone in its cell, its run cut in two with another cell's records in between: every run is well-formed, only the rule objects
    out, info = _mutant(good)
    alone = G.one_run_keys(KEYS, G.fine_bucket(KEYS, info, None), info, np.flatnonzero(G.live_mask(KEYS, VALS, G.GR_FLAG_DEAD)))["one-run-alone"]
    st, cn, un = out["starts"], out["counts"], out["uniq"]
    r = _run_of(out, info, lambda u, s, c: c >= 2 and u in alone and (u >> 57) & 7 == 0 and s > 0)
    nxt = int(np.flatnonzero(st[:info.n_runs] == st[r] + cn[r])[0])     # the run behind it, of the same bucket
    assert (int(un[nxt]) >> 57) & 7 == 0
    a, m, e = int(st[r]), int(st[r]) + int(cn[r]), int(st[nxt]) + int(cn[nxt])
    new = np.concatenate([np.arange(a, a + 1), np.arange(m, e), np.arange(a + 1, m)])     # [first record][next run][the rest]
    for name in ("vals_out", "tz_out"):
        out[name][a:e] = out[name][new]
    st[nxt] = a + 1
    _split(out, info, r, 1)
    st[info.n_runs - 1] = a + 1 + cn[nxt]
    _rejected(out, info, "one-run-alone")
    # the hot hash of the oversized bucket cut at a piece boundary: neighbours with one hash
    out, info = _mutant(good)
    r = _run_of(out, info, lambda u, s, c: c == 2500)
    _split(out, info, r, 4096 - int(out["starts"][r]) % 4096)
    _rejected(out, info, "run-adjacent")
    # the interleaved group of bucket 7 left as the counting sort gives it (level 1 must repair it: 24 records, 23 changes)
    out, info = G.reference_grouping(KEYS, VALS, T=T, L=L, fix=1, repaired=False, **KW)
    _rejected(out, info, "one-run-repair")
    out, info = G.reference_grouping(KEYS, VALS, T=T, L=L, fix=2, repaired=False, **KW)
    _rejected(out, info, "one-run-repair", "one-run-repair2")


def test_adjacent_equal_key_runs_left_unmerged(good):
    out, info = _mutant(good)
    r = _run_of(out, info, lambda u, s, c: c >= 2)
    _split(out, info, r, 1)
    _rejected(out, info, "run-adjacent")


def test_one_record_dropped_and_another_duplicated(good):
    out, info = _mutant(good)
    out["vals_out"][10] = out["vals_out"][11]
    _rejected(out, info, "permutation")


def test_dead_record_kept(good):
    out, info = _mutant(good)
    L_ = info.n_live
    r = _run_of(out, info, lambda u, s, c: u == ONES)
    # the cancelled record joins the run of its all-ones hash at the end of the array (bucket 7 is the last one)
    assert int(out["starts"][r]) + int(out["counts"][r]) == L_
    out["vals_out"][L_] = 0xFFFFFFFF; out["counts"][r] += 1; info.n_live += 1
    _rejected(out, info, "live-count")


def test_live_all_ones_key_dropped(good):
    out, info = _mutant(good)
    r = _run_of(out, info, lambda u, s, c: u == ONES)
    assert int(out["counts"][r]) == 3 and int(out["starts"][r]) + 3 == info.n_live
    out["counts"][r] -= 1; info.n_live -= 1
    _rejected(out, info, "live-count")


def test_one_strength_off_by_one(good):
    for i in (0, 777, good[1].n_live - 1):
        out, info = _mutant(good)
        out["tz_out"][i] += 1
        _rejected(out, info, "strength")
        out["tz_out"][i] = (int(out["tz_out"][i]) - 2) & 31
        _rejected(out, info, "strength")


def test_two_buckets_record_ranges_exchanged(good):
    out, info = _mutant(good)
    b = G.fine_bucket(out["uniq"][:info.n_runs], info, None)
    st, cn = out["starts"].astype(np.int64), out["counts"].astype(np.int64)
    lo1, lo2, lo3 = (int(st[:info.n_runs][b == c].min()) for c in (1, 2, 3))
    n1, n2 = lo2 - lo1, lo3 - lo2
    new = np.concatenate([np.arange(lo2, lo3), np.arange(lo1, lo2)])
    for name in ("vals_out", "tz_out"):
        out[name][lo1:lo3] = out[name][new]
    R = info.n_runs
    out["starts"][:R] = np.where(b == 1, st[:R] + n2, np.where(b == 2, st[:R] - n1, st[:R]))
    _rejected(out, info, "bucket-order")


def test_brun_entry_shifted_by_one(good):
    for d in (1, -1):
        out, info = _mutant(good)
        out["brun"][2] = int(out["brun"][2]) + d
        _rejected(out, info, "export")
    out, info = _mutant(good)
    out["bnr"][2] -= 1
    _rejected(out, info, "export")
    out, info = _mutant(good)
    assert out["bnr"][5] == 0
    out["bnr"][5] = 1                                                   # the oversized bucket
    _rejected(out, info, "export")
    out, info = _mutant(good)
    s = out["starts"]
    s[[3, 4]] = s[[4, 3]]; out["counts"][[3, 4]] = out["counts"][[4, 3]]; out["uniq"][[3, 4]] = out["uniq"][[4, 3]]
    G.check_grouping(KEYS, VALS, out, info, **KW)                       # the order of a bucket's runs is free ...
    _check = pytest.raises(G.GroupingError)
    with _check as e:
        G.check_grouping(KEYS, VALS, out, info, ordered=True, **KW)     # ... unless the call asked for bucket order
    assert e.value.rule == "export-ordered"


def test_oversized_bucket_order_is_exact_at_every_fix_level(good):
    # two records of different cells of the oversized bucket exchanged together with their runs: well-formed, but not the stable order
    out, info = _mutant(good)
    b = G.fine_bucket(out["uniq"][:info.n_runs], info, None)
    r = [i for i in range(info.n_main, info.n_runs) if out["counts"][i] == 1]
    a = next(i for i in r if any(out["starts"][j] == out["starts"][i] + 1 for j in r))
    c = next(j for j in r if out["starts"][j] == out["starts"][a] + 1)
    assert b[a] == 5 and b[c] == 5
    _swap(out, int(out["starts"][a]), int(out["starts"][c]))
    out["uniq"][[a, c]] = out["uniq"][[c, a]]
    _rejected(out, info, "exact-order")


# ---- the index-bucket formula -------------------------------------------------------------------------------------------
def _edge(c, T_, span, mul):
    """first index of fine bucket c (what the swept stage's sw_first finds), in Python integers"""
    dig = lambda x: min((x * mul) >> 64, (1 << T_) - 1)
    e = (c * span) >> T_
    while e > 0 and dig(e - 1) >= c: e -= 1
    while e < span and dig(e) < c: e += 1
    return e


@pytest.mark.parametrize("size,T_", [(1_000_003, 3), (1_000_003, 10), (1_000_003, 11), (1_000_003, 18), (2**33 + 9, 3), (2**33 + 9, 11), (2**33 + 9, 20)])
def test_index_bucket_formula_matches_python_integers(size, T_):
    rng = np.random.default_rng(size % 1000 + T_)
    for lo, span in ((0, size), (size // 3, size // 4 if size // 4 > (1 << T_) else size - size // 3)):    # (a shard's range; more indices than buckets)
        mul = G.index_bucket_mul(T_, span)
        cs = np.arange(1, 1 << T_) if T_ <= 11 else np.unique(np.concatenate([np.array([1, 2, (1 << T_) - 2, (1 << T_) - 1]), rng.integers(1, 1 << T_, 3000)]))
        edges = np.array([_edge(int(c), T_, span, mul) for c in cs], np.uint64)
        rel = np.unique(np.concatenate([edges - np.uint64(1), edges[edges < span], rng.integers(0, span, 20000).astype(np.uint64), np.array([0, span - 1], np.uint64)]))
        # keys whose index is lo + rel: (key >> 1) % size == lo + rel, with and without the low bit and a multiple of size on top
        idx = rel + np.uint64(lo)
        keys = (idx + np.uint64(size) * rng.integers(0, (2**62) // size, idx.size).astype(np.uint64)) * np.uint64(2) + rng.integers(0, 2, idx.size).astype(np.uint64)
        got = G.index_bucket(keys, T_, size, lo, span)
        want = np.array([G.index_bucket_exact(int(k), T_, size, lo, span) for k in keys])
        assert np.array_equal(got, want)
        # the formula is floor(i * 2^T / span) or one less (the reciprocal is rounded down: i * mul / 2^64 > i * 2^T / span - i / 2^64), never decreasing
        true = np.array([(int(r) << T_) // span for r in rel])
        assert ((got == true) | (got == true - 1)).all() and (np.diff(got) >= 0).all()
        # both neighbours of every edge lie in different buckets, the upper one in bucket c or beyond (c itself unless the bucket is empty)
        below = G.index_bucket((edges - np.uint64(1) + np.uint64(lo)) * np.uint64(2), T_, size, lo, span)
        assert (below < cs).all()
        inside = edges < span
        at = G.index_bucket((edges[inside] + np.uint64(lo)) * np.uint64(2), T_, size, lo, span)
        assert (at >= cs[inside]).all()
    # an index outside [lo, lo + span) lands in the last bucket, as on the device (the subtraction wraps)
    assert G.index_bucket(np.array([2 * 5], np.uint64), T_, size, 1000, size // 2)[0] == (1 << T_) - 1


def test_mulhi64_and_strengths_match_python():
    rng = np.random.default_rng(2)
    a = np.concatenate([rng.integers(0, 2**64, 5000, dtype=np.uint64), np.array([0, 1, 2**64 - 1, 2**32, 2**32 - 1], np.uint64)])
    for b in (0, 1, 2**64 - 1, 2**32, 0x9E3779B97F4A7C15, int(rng.integers(0, 2**63))):
        assert [int(x) for x in G.mulhi64(a, b)] == [(int(x) * b) >> 64 for x in a]
    from oracle import rbo
    f = rbo.lib().rbo_rng31
    v = np.concatenate([rng.integers(G._TABLE_MAX, 2**32, 300, dtype=np.uint64), np.array([0, 1, 4097, 2**32 - 1, G._TABLE_MAX], np.uint64)]).astype(np.uint32)
    for pb in (0, 7, 31):
        want = []
        for x in v:
            r = f(SEED, ORD0 + (int(x) >> pb), int(x) & ((1 << pb) - 1)) | 0x8000
            want.append(next(i for i in range(32) if (r >> i) & 1))
        assert G.strengths(v, SEED, ORD0, pb).tolist() == want
    assert set(G.strengths(np.arange(5000, dtype=np.uint32), SEED, ORD0, POSB).tolist()) <= set(range(16))
