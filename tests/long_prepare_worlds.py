"""The worlds of tests/test_long_prepare_reach.py (CPU) and tests/test_gpu_long_prepare.py: seeded raw long reads for rb_long_prepare, a few
hundred in all, and what the restatement of tests/test_long_prepare_rules.py makes of them — computed once per case and shared.
A case is a set of rb_prep_params.  Its reads are random letters at the lengths where the call takes another path (0, min_len - 1 and min_len,
6 and 7, 199 and 200, 5 lc_window - 1 and 5 lc_window, lengths with every remainder that matters), the same lengths filled with repeats, reads
with a poly-A tail, a poly-T head, both, with and without letters outside them (5 % foreign letters inside), reads laid out window by window
from complex and low blocks (a run from window 0, a run open at the end, several segments, one to four low windows that do not make the
cut fire), the same with a tail (several segments clear hasPolyA), copies with lower case, N, U and bytes above 127, all A and all T, and — in
two cases — one read of 70 000 and one of 300 001 letters with low stretches at both ends and in the middle."""
import functools

import numpy as np

from test_long_prepare_rules import FIELDS, Finder, params, prepare

ACGT = np.frombuffer(b"ACGT", np.uint8)

CASES = [
    # the worker's own values (k = 25)
    dict(big=True, P=params()),
    # a short seed in a window no wider than it needs, every window cut: lc_min_length 0
    dict(big=True, P=params(min_len=0, seed_length=4, window=5, max_gap=1, lc_window=37, lc_min_length=0)),
    # a window wider than any read but the big ones, stranded
    dict(big=False, P=params(min_len=31, seed_length=10, window=4000, strand_specific=1)),
    # no finder, the read turned first, odd windows that never add up to the cut
    dict(big=False, P=params(min_len=16, polya=0, reverse_complement=1, lc_window=37)),
    # identity 0.5: seeds of two A in three, joins that only percentA allows
    dict(big=False, P=params(min_len=0, seed_length=3, min_identity=0.5, max_gap=1, window=5, lc_min_length=300)),
    # the read turned first and then searched: a head in the input is a tail, and a tail is a head that turns it back
    dict(big=False, P=params(reverse_complement=1, lc_min_length=200)),
    # stranded and turned
    dict(big=False, P=params(reverse_complement=1, strand_specific=1, seed_length=12, window=100, lc_window=100, lc_min_length=0)),
]


def case_id(c):
    P = c["P"]
    return "k%d-rc%d-ss%d-polya%d-seed%d-id%g-gap%d-w%d-lc%d-%d%s" % (P["min_len"], P["reverse_complement"], P["strand_specific"], P["polya"],
                                                                       P["seed_length"], P["min_identity"], P["max_gap"], P["window"],
                                                                       P["lc_window"], P["lc_min_length"], "-big" if c["big"] else "")


def rand(rng, n):
    return ACGT[rng.integers(0, 4, int(n))].tobytes()


def low(rng, n):
    """n letters of a repeat of one, two or three letters"""
    m = int(rng.integers(1, 4))
    unit = bytes(rng.permutation(ACGT)[:m].tolist())
    return (unit * (int(n) // m + 1))[:int(n)]


def rich(rng, n, letter):
    """n letters, 5 % of them foreign"""
    b = bytearray(letter * int(n))
    for p in rng.choice(int(n), max(1, int(n) // 20), replace=False):
        b[int(p)] = int(rng.choice([x for x in b"ACGT" if x != letter[0]]))
    return bytes(b)


def laid_out(rng, pattern, ws, edge):
    """a read of len(pattern) windows of ws letters — c: complex, L: low — behind edge // 2 letters and before edge - edge // 2 (edge < ws)"""
    return rand(rng, edge // 2) + b"".join(rand(rng, ws) if ch == "c" else low(rng, ws) for ch in pattern) + rand(rng, edge - edge // 2)


def reads_of(i):
    c = CASES[i]
    P, rng = c["P"], np.random.default_rng(4200 + i)
    ws, k = P["lc_window"], P["min_len"]
    out = []
    lengths = sorted({0, max(0, k - 1), k, 6, 7, 199, 200, 201, 249, 250, 5 * ws - 1, 5 * ws, 5 * ws + 1, 7 * ws, 7 * ws + 1, 8 * ws - 1, 6 * ws + ws // 2})
    out += [rand(rng, n) for n in lengths]
    out += [low(rng, n) for n in (7, 8, 50, 199, 200, 260, 5 * ws - 1, 5 * ws, 6 * ws + 1)]
    out += [b"A" * 30, b"T" * 30, b"A" * (5 * ws + 3), b"T" * (5 * ws + 3), b"A" * 6, b"a" * 40, b"t" * 40]
    out += [b"CGCGCGCGCG" + b"AACCACAAAAA", b"CG" * 10 + b"AAAACGCGAAAACGCGAAAA", b"TTTTGCGCTTTT" + b"CG" * 10, b"TTTTAAAA", b"TATATATATA" * 3]
    for j in range(18):                                              # tails and heads
        body, t, h = rand(rng, rng.integers(150, 900)), rich(rng, rng.integers(15, 61), b"A"), rich(rng, rng.integers(15, 61), b"T")
        junk = rand(rng, rng.integers(1, 9))
        out.append([body + t, body + t + junk, h + body, junk + h + body, h + body + t, junk + h + body + t + junk][j % 6])
    patterns = ["cLcLLLLc", "LccLLLLLc", "ccccc", "cLccc", "ccLLc", "cLLLcc", "cLLLLc", "LLLLLL", "cLcLcLcLcLc", "ccccccL", "Lcccccc", "cLLLLLc"]
    for j, pat in enumerate(patterns):
        edge = int(rng.integers(0, ws))
        out.append(laid_out(rng, pat, ws, edge))
        if j % 2 == 0:                                               # ... with a tail, a head, or letters before the head
            out.append(laid_out(rng, pat, ws, edge) + rich(rng, 20 + j, b"A"))
            out.append(rand(rng, j % 3) + rich(rng, 20 + j, b"T") + laid_out(rng, pat, ws, edge))
    for j, s in enumerate(list(out[-30::3])):                        # other letters: lower case, N, U, bytes above 127
        b = bytearray(s)
        for p in rng.choice(len(b), max(1, len(b) // 15), replace=False):
            p = int(p)
            b[p] = [b[p] | 0x20, ord("N"), ord("U") if b[p] == ord("T") else ord("u"), b[p] | 0x80, 200][(p + j) % 5]
        out.append(bytes(b))
    if c["big"]:
        for n in (70_000, 300_001):
            a, m, z = low(rng, 650), low(rng, 900), low(rng, 730)
            half = (n - len(a) - len(m) - len(z) - 40) // 2
            s = a + rand(rng, half) + m + rand(rng, n - len(a) - len(m) - len(z) - 40 - half) + z + rich(rng, 40, b"A")
            assert len(s) == n
            out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def want(i):
    """the reads of CASES[i], what prepare makes of each — (record, segments, transformed read) — and the joins only percentA / percentT made"""
    reads = reads_of(i)
    f = Finder(CASES[i]["P"])
    return reads, [prepare(r, CASES[i]["P"], f) for r in reads], f.bridged


F = {f: j for j, f in enumerate(FIELDS)}
