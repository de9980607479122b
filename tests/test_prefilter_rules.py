"""tests/prefilter_ref.py against itself, without a GPU: tables packed here word by word from the layout (Python integers, not the reference's
own expressions) must decode to the records they were packed from; a true table passes check_entries and each kind of lie is named; the
keep mask follows the table and the oracle's generator.  The reference is what tests/test_gpu_prefilter.py holds the library to, so a
decoder that reads a bit wrong would either fail every GPU test or — worse — excuse a real fault."""
import numpy as np
import pytest

import grouping_ref as G
import prefilter_ref as P

M64 = (1 << 64) - 1


def pack_mpf(log2b, items):
    """items: (bucket, 'A' | 'B', h0, code) -> table words, written as the layout's sentences say"""
    tab = np.zeros(16 << log2b, np.uint64)
    for bucket, ab, h0, code in items:
        if ab == "A":
            slot, word = 2 * (h0 % 8), (h0 // 8) * 8 + code
        else:
            slot, word = 2 * ((h0 // 8) % 8) + 1, (h0 // 64) * 64 + (h0 % 8) * 8 + code
        tab[16 * bucket + slot] = word
    return tab


def pack_npf(log2n, items):
    """items: (slot, h0, exponent)"""
    tab = np.zeros(1 << log2n, np.uint64)
    nb = 1 << (log2n - 3)
    for slot, h0, exp in items:
        tab[8 * (h0 % nb) + slot] = (h0 // nb) * 16 + exp
    return tab


def _hashes(rng, n):
    return [int(x) for x in rng.integers(0, 1 << 64, n, dtype=np.uint64)]


@pytest.mark.parametrize("log2b", [8, 12])
def test_minimizer_bucketed_table_round_trip(log2b):
    rng = np.random.default_rng(log2b)
    hs = _hashes(rng, 400) + [M64, M64 - 7, 8, 64 + 5, 1 << 63]          # (all ones, low bits all set / clear, the top bit alone)
    items, seen = [], set()
    for h0 in hs:
        bucket, ab, code = int(rng.integers(0, 1 << log2b)), "AB"[int(rng.integers(0, 2))], int(rng.integers(0, 8))
        slot = 2 * (h0 % 8) if ab == "A" else 2 * ((h0 // 8) % 8) + 1
        if (bucket, slot) in seen or (ab == "A" and h0 // 8 == 0 and code == 0):
            continue
        seen.add((bucket, slot)); items.append((bucket, ab, h0, code))
    ent = P.decode_mpf(pack_mpf(log2b, items), log2b)
    assert len(ent) == len(items)
    want = sorted((b, 2 * (h % 8) if ab == "A" else 2 * ((h // 8) % 8) + 1, h, {0: 11, 7: 7}.get(c, c)) for b, ab, h, c in items)
    got = sorted(zip(ent.bucket.tolist(), ent.slot.tolist(), [int(x) for x in ent.h0], ent.bound.tolist()))
    assert got == want
    assert not ent.saturated.any()
    for _, _, h, _ in items[:50]:
        assert P.mpf_candidates(h) == (2 * (h % 8), 2 * ((h // 8) % 8) + 1)


@pytest.mark.parametrize("log2n", [8, 16])
def test_hash_bucketed_table_round_trip(log2n):
    rng = np.random.default_rng(log2n)
    items, seen = [], set()
    for h0 in _hashes(rng, 300) + [M64, 1 << 63, (1 << (log2n - 3)) + 1]:
        slot, exp = int(rng.integers(0, 8)), int(rng.integers(1, 16))
        if (h0 % (1 << (log2n - 3)), slot) in seen:
            continue
        seen.add((h0 % (1 << (log2n - 3)), slot)); items.append((slot, h0, exp))
    ent = P.decode_npf(pack_npf(log2n, items), log2n)
    want = sorted((h % (1 << (log2n - 3)), s, h, e) for s, h, e in items)
    assert sorted(zip(ent.bucket.tolist(), ent.slot.tolist(), [int(x) for x in ent.h0], ent.bound.tolist())) == want
    assert (ent.saturated == (ent.bound == 15)).all() and ent.saturated.sum() == sum(e == 15 for _, _, e in items)


def test_the_largest_bound_of_a_hash_wherever_it_lies():
    h = [0x1234567890ABCDEF, 0x0FEDCBA987654321, 77]
    ent = P.decode_mpf(pack_mpf(8, [(3, "A", h[0], 2), (3, "B", h[0], 5), (9, "B", h[1], 0), (200, "A", h[2], 7)]), 8)
    b, sat = P.bounds_for(ent, np.array(h + [78], np.uint64))
    assert b.tolist() == [5, 11, 7, 0] and not sat.any()
    ent = P.decode_npf(pack_npf(8, [(0, h[0], 15), (1, h[0], 3), (5, h[1], 14)]), 8)
    b, sat = P.bounds_for(ent, np.array(h, np.uint64))
    assert b.tolist() == [15, 14, 0] and sat.tolist() == [True, False, False]


class _Filters:
    """stands in for the oracle's filters: membership and minimum by base hash"""

    def __init__(self, mn):
        self.mn = mn

    def contains(self, rows):
        return np.array([self.mn.get(int(h), -1) >= 0 for h in rows[:, 0]])

    def minimum(self, rows):
        return np.array([max(self.mn.get(int(h), 0), 0) for h in rows[:, 0]], np.int64)


def _known(hs):
    k = P.Known(1)
    k.h0 = np.sort(np.array(hs, np.uint64)); k.rows = k.h0[:, None].copy()
    return k


def test_a_true_table_passes_and_every_lie_is_named():
    rng = np.random.default_rng(5)
    hs = _hashes(rng, 6)
    mn = {hs[0]: 16, hs[1]: 63, hs[2]: 64, hs[3]: 126, hs[4]: 127, hs[5]: 15}      # exponents 1, 6, 7, 14, saturated, 0
    known, filt = _known(hs), _Filters(mn)
    true_m = [(1, "A", hs[0], 1), (1, "B", hs[1], 6), (2, "A", hs[2], 7), (2, "B", hs[3], 0), (7, "A", hs[4], 0), (2, "A", hs[3], 7)]
    assert P.check_entries(P.decode_mpf(pack_mpf(8, true_m), 8), known, filt) == 6
    true_n = [(0, hs[0], 1), (1, hs[3], 14), (2, hs[4], 15), (3, hs[4], 9)]
    assert P.check_entries(P.decode_npf(pack_npf(8, true_n), 8), known, filt) == 4

    def rule(items, which=P.MPF):
        tab = pack_mpf(8, items) if which == P.MPF else pack_npf(8, items)
        with pytest.raises(P.PrefilterError) as e:
            P.check_entries(P.decode(which, tab, 8), known, filt)
        return e.value.rule
    assert rule([(1, "A", hs[0], 2)]) == "overstated"                   # exponent 1, the entry says 2
    assert rule([(1, "B", hs[2], 0)]) == "overstated"                   # exponent 7 is not "11 or more"
    assert rule([(1, "A", hs[5], 1)]) == "overstated"                   # below exponent 1 nothing may be said
    assert rule([(1, "A", hs[0] ^ 8, 1)]) == "forged"                   # one bit of the tag
    assert rule([(1, "A", hs[0] ^ 1, 1)]) == "forged"                   # ... of the slot
    assert rule([(1, "A", hs[0], 1), (2, "B", hs[0], 1)]) == "two-buckets"
    filt.mn[hs[1]] = -1
    assert rule([(1, "B", hs[1], 1)]) == "not-in-dbgbf"
    assert rule([(0, hs[3], 15)], P.NPF) == "saturated"                 # 126 is not the ceiling
    assert rule([(0, hs[2], 8)], P.NPF) == "overstated"
    tab = pack_npf(8, [(0, hs[0], 1)]); tab[np.flatnonzero(tab)[0]] &= np.uint64(~15 & M64)
    with pytest.raises(P.PrefilterError) as e:
        P.check_entries(P.decode_npf(tab, 8), known, filt)
    assert e.value.rule == "bound"


def test_the_keep_mask_follows_the_table_and_the_generator():
    """three reads of 70, 40 and 0 bases at k = 8 with a gap of unusable windows: a window is dropped iff its hash has an entry and the draw is
    weaker than the bound; bit p & 31 of word p >> 5 of the read; words where nothing starts read 0"""
    seed, ord0, posb, k = 99, (1 << 33) + 5, 7, 8
    lens = [70, 40, 0]
    read = np.concatenate([np.zeros(40, np.int64), np.ones(33, np.int64)])
    pos = np.concatenate([np.arange(0, 20), np.arange(43, 63), np.arange(0, 33)]).astype(np.int64)     # read 0: windows 20..42 are unusable
    rng = np.random.default_rng(1)
    h0 = rng.integers(0, 1 << 64, read.size, dtype=np.uint64)
    h0[50:] = h0[5]                                                       # one k-mer many times: draws of every strength
    win = P.Windows(read, pos, h0[:, None], lens)
    st = G.strengths(((read << posb) | pos).astype(np.uint32), seed, ord0, posb).astype(int)
    ent = P.decode_mpf(pack_mpf(8, [(4, "B", int(h0[5]), 2), (9, "A", int(h0[7]), 0)]), 8)
    cnt, mask = P.expected_keep(win, ent, seed, ord0, posb)
    assert mask.size == 3 + 2 + 0 and cnt.tolist() == P.popcount32(mask).tolist()
    for i in range(read.size):
        bound = 2 if h0[i] == h0[5] else 11 if i == 7 else 0
        kept = not (bound and st[i] < bound)
        w = (0 if read[i] == 0 else 3) + pos[i] // 32
        assert bool((int(mask[w]) >> (pos[i] % 32)) & 1) == kept, i
    assert int(cnt.sum()) == sum(1 for i in range(read.size) if not ((h0[i] == h0[5] and st[i] < 2) or (i == 7 and st[i] < 11)))
    assert mask[0] >> 20 == 0 and mask[2] >> 31 == 0 and (st[50:] < 2).any() and (st[50:] >= 2).any()
    P.check_keep(cnt, mask, win, ent, seed, ord0, posb)
    for flip, rule in (("mask", "mask"), ("cnt", "count")):
        c2, m2 = cnt.copy(), mask.copy()
        if flip == "mask":
            m2[1] ^= 1 << 12; c2 = P.popcount32(m2)
        else:
            c2[3] += 1
        with pytest.raises(P.PrefilterError) as e:
            P.check_keep(c2, m2, win, ent, seed, ord0, posb)
        assert e.value.rule == rule
    # a saturated entry drops every occurrence, whatever the draw
    ent = P.decode_npf(pack_npf(8, [(2, int(h0[5]), 15)]), 8)
    _, m3 = P.expected_keep(win, ent, seed, ord0, posb)
    assert int(P.popcount32(m3).sum()) == int((h0 != h0[5]).sum())


def test_usable_windows_are_the_oracles_segments():
    from oracle import rbo
    k = 5
    reads = [b"ACGTACGTNACGTAC", b"ACG", b"", b"ACGTUacgtACGTA", b"ACGTACGTACGT"]
    quals = [b"IIIIIIIIIIIIIII", b"III", b"", b"IIIIIIIIIIIIII", b"IIII#IIIIIII"]
    seq, qual = np.frombuffer(b"".join(reads), np.uint8), np.frombuffer(b"".join(quals), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    win = P.usable_windows(seq, qual, off, k, False, 2)
    assert win.lens.tolist() == [15, 3, 0, 14, 12]
    assert win.pos[win.read == 0].tolist() == [0, 1, 2, 3, 9, 10] and not (win.read == 1).any() and not (win.read == 2).any()
    assert win.pos[win.read == 3].tolist() == list(range(10))                      # U and lower case are bases
    assert win.pos[win.read == 4].tolist() == [5, 6, 7]                            # the '#' (PHRED 2 < 3) cuts the read
    h, _ = rbo.hash_region(reads[4], k, 2, 1, 5, 12)
    assert (win.rows[win.read == 4] == h).all()
    fwd = P.usable_windows(seq, qual, off, k, True, 1)
    assert (fwd.h0[fwd.read == 4] == rbo.hash_region(reads[4], k, 1, 0, 5, 12)[0][:, 0]).all()


def test_the_bucket_of_a_kmer_is_the_same_for_both_strands():
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    rng = np.random.default_rng(3)
    for k in (17, 21, 22, 25, 31, 35, 48, 63):
        s = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, k)])
        m = min(16, k)
        assert P.mpf_bucket_of(s, 12, m) == P.mpf_bucket_of(s.translate(comp)[::-1], 12, m)
        assert 0 <= P.mpf_bucket_of(s, 8, m) < 256
