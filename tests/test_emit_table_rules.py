"""The arithmetic of the table-driven emit kernel (csrc/rb_batch.hip k_hash_windows_direct) restated in Python and held against the oracle's
from-scratch ntHash: the 256-entry table of four-base contributions, the window's bytes folded in ascending order with a rotation by four
per byte, the bases past the window's end masked to code 0 and taken out again, one final rotation per strand.  No device: this checks the
identities the kernel rests on (for every k it serves, k mod 4 = 0 .. 3, and the k = 32 window that fills its 64 bits); the kernel itself is
compared with the walkers and the oracle in tests/test_gpu_emit_direct.py."""
import numpy as np
import pytest

from oracle import rbo

M64 = (1 << 64) - 1
SEED = (0x3c8bfbb395c60474, 0x3193c18562a02b4c, 0x20323ed082572324, 0x295549f54be24456)       # A C G T (R/bloom/hash/NTHash.java:39-43)


def rotl(v, s):
    s &= 63
    return ((v << s) | (v >> (64 - s))) & M64 if s else v


def table():
    f, r = [0] * 256, [0] * 256
    for b in range(256):
        for t in range(4):
            c = (b >> (2 * t)) & 3
            f[b] ^= rotl(SEED[c], 3 - t)
            r[b] ^= rotl(SEED[3 - c], t)
    return f, r


T4F, T4R = table()


def direct(codes, k):
    """(f, r) of the window whose k 2-bit codes are `codes`, as a lane of the kernel computes them"""
    w = sum(int(c) << (2 * i) for i, c in enumerate(codes))                 # already masked to 2k bits
    n = (k + 3) // 4
    pad = 4 * n - k
    fx = rx = 0
    for t in range(4 - pad, 4):
        fx ^= rotl(SEED[0], 3 - t)
        rx ^= rotl(SEED[3], t)
    f = r = 0
    for q in range(n):
        b = (w >> (8 * q)) & 0xFF
        f = rotl(f, 4) ^ T4F[b]
        r = rotl(r, 60) ^ T4R[b]
    return rotl(f ^ fx, (k - 4 * n) & 63), rotl(r ^ rx, 4 * (n - 1))


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 16, 17, 18, 24, 25, 27, 31, 32])
def test_table_hash_equals_the_from_scratch_hash(k):
    rng = np.random.default_rng(k)
    codes = rng.integers(0, 4, 400)
    codes[:40] = 0; codes[40:80] = 3                                      # homopolymers: every byte 0x00 / 0xFF
    seq = bytes(b"ACGT"[c] for c in codes)
    _, fr = rbo.hash_region(seq, k, 1, 1)
    assert fr.shape == (len(seq) - k + 1, 2)
    for p in range(fr.shape[0]):
        assert direct(codes[p:p + k], k) == (int(fr[p, 0]), int(fr[p, 1])), (k, p)
