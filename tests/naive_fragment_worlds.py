"""Worlds, fragments and the restatement for rb_graph_naive_extend_fragments — GraphUtils.naiveExtend(kmers, graph, maxTipLength, minKmerCov)
(R/util/GraphUtils.java:6935-6957) — shared by test_naive_fragment_reach.py (CPU: what the worlds reach) and test_gpu_naive_fragments.py.

The restatement is the reference's two statements over rbo.naive_extend, the statement-by-statement oracle of naiveExtendLeft / Right: the left
walk from kmers[0] with the fragment as terminators, then the right walk from kmers[last] with the left extension + the fragment as terminators.
A call's `room` is the oracle's cap (its reason 6).

Random worlds (traversal_worlds.World: reads with substitutions over a random genome, a tandem repeat, a fork) reach NO_NEIGHBOUR, BACK_BRANCH and
SEVERAL on both sides, and MEMBER only through the tandem repeat's fragment.  Ring worlds — a random circle read twice, so that every k-mer counts
2 — give MEMBER on chosen k-mers and the long walks; a spur is a single k-mer that counts 1: a back branch where a walk stands on the k-mer it
varies, a second neighbour only below min_kmer_cov 2."""
import functools

import numpy as np
from oracle import rbo

import traversal_worlds as tw
from traversal_worlds import ACGT, World

DONE, ROOM, NOT_JUDGED = range(3)
WHY_NONE, WHY_NO_KMER, WHY_LETTER = range(3)
END_NOT_RUN, END_NO_NEIGHBOUR, END_BACK_BRANCH, END_SEVERAL, END_MEMBER, END_ROOM = range(6)
END_OF_REASON = {0: END_NO_NEIGHBOUR, 1: END_BACK_BRANCH, 2: END_SEVERAL, 5: END_MEMBER, 6: END_ROOM}     # rbo.naive_extend's reasons
FIELDS = ("status", "why", "left_ext", "right_ext", "out_len", "left_end", "right_end", "left_hit", "right_hit")

AMPLE = 4096                  # a room no walk of these worlds fills
MIN_COVS = (1.0, 2.0)
K_MAIN = 25
K_MATRIX = tuple(k for k in tw.KS if k in (16, 32, 33, 64, 65, 143))
assert len(K_MATRIX) == 6


def restate(og, k, text, min_cov, room=AMPLE, phase=0):
    """one call for one sequence: the dict of FIELDS and "text" """
    text = bytes(text)
    if len(text) < k or any(c not in b"ACGT" for c in text):
        return dict(status=NOT_JUDGED, why=WHY_NO_KMER if len(text) < k else WHY_LETTER, left_ext=0, right_ext=0, out_len=len(text), left_end=0,
                    right_end=0, left_hit=-1, right_hit=-1, text=text)

    def count(km):
        return float(og.get_kmers(km)[2][0])

    def candidate(km, direction):       # the only neighbour with count >= min_cov of the k-mer a walk ended on with reason 5
        c = [nb for nb in ((km[1:] + bytes([x]) if direction == 0 else bytes([x]) + km[:-1]) for x in b"ACGT") if count(nb) >= min_cov]
        assert len(c) == 1
        return c[0]

    lext, lend, lcand = b"", END_NOT_RUN, None
    if phase == 0:
        walked, reason = rbo.naive_extend(og, text[:k], 1, 0, min_cov=min_cov, terminators=text, k=k, cap=room)
        lext, lend = walked[::-1], END_OF_REASON[reason]             # (the oracle returns a left walk's bases in walking order)
        if lend == END_MEMBER: lcand = candidate((lext + text)[:k], 1)
    rext, rend, rcand = b"", END_NOT_RUN, None
    if lend != END_ROOM:
        rext, reason = rbo.naive_extend(og, text[-k:], 0, 0, min_cov=min_cov, terminators=lext + text, k=k, cap=room)
        rend = END_OF_REASON[reason]
        if rend == END_MEMBER: rcand = candidate((text + rext)[-k:], 0)
    out = lext + text + rext
    first = {}
    for p in range(len(out) - k + 1): first.setdefault(out[p:p + k], p)
    return dict(status=ROOM if END_ROOM in (lend, rend) else DONE, why=WHY_NONE, left_ext=len(lext), right_ext=len(rext), out_len=len(out),
                left_end=lend, right_end=rend, left_hit=first[lcand] if lcand else -1, right_hit=first[rcand] if rcand else -1, text=out)


def restate_chain(og, k, text, min_cov, room):
    """the calls a caller chains until the status is DONE: (the final text, left_ext and right_ext summed, the last call's record, calls made)"""
    phase, left, right, calls = 0, 0, 0, 0
    while True:
        a = restate(og, k, text, min_cov, room, phase)
        calls += 1
        text, left, right = a["text"], left + a["left_ext"], right + a["right_ext"]
        if a["status"] != ROOM: return text, left, right, a, calls
        phase = 0 if a["left_end"] == END_ROOM else 1


# ---- random worlds ----
def _rng(k, stranded, salt):
    return np.random.default_rng(7919 * k + (31 if stranded else 0) + salt)


def random_fragments(w, n, seed):
    """n substrings of the world's genome reads, 1 .. about 150 k-mers (the first has exactly one), and the tandem repeat's first 30 k-mers: a
    fragment whose k-mers repeat with the period 12"""
    rng, k = _rng(w.k, w.stranded, seed), w.k
    out = []
    for i in range(n):
        rd = w.genome_reads[int(rng.integers(0, len(w.genome_reads)))]
        nk = 1 if i == 0 else int(rng.integers(1, min(150, len(rd) - k + 1) + 1))
        p = int(rng.integers(0, len(rd) - k + 1 - nk + 1))
        out.append(rd[p:p + nk + k - 1])
    out.append(w.repeat_read[:30 + k - 1])
    return out


# (k, stranded, hashes, branchy): the four k = 25 worlds, then one world per k of the matrix with the strandedness, hash counts and noise alternating
RANDOM_CASES = tuple((K_MAIN, s, (2, 2), b) for s in (True, False) for b in (False, True)) + \
    tuple((k, i % 2 == 0, tw.HASHES[i % 5], i % 3 == 0) for i, k in enumerate(K_MATRIX))
N_RANDOM = {K_MAIN: 30}       # fragments per world (the k = 25 worlds have the issue's 120 together); the matrix's worlds have 10 each


def random_world(case, device=False):
    return World(*case, device=device)


def random_case_fragments(w):
    return random_fragments(w, N_RANDOM.get(w.k, 10), 1)


# ---- ring worlds ----
BIG = (tw._prime_above(4_000_000), tw._prime_above(2_000_000))      # filters in which a 550-step walk meets no false neighbour (about 1e-7 a look-up)
RING_SPURS = ("none", "far", "first")


def ring_shape(k):
    """(letters of the circle, the fragment's first and last + 1 circle k-mer, the circle k-mer the far spur varies): the issue's ring at k = 25,
    a shorter one for the matrix"""
    return (700, 300, 450, 100) if k == K_MAIN else (300, 100, 160, 40)


def ring_world(k, stranded, spur, device=False):
    """a random circle c read twice as c + c[:k - 1]; spur "far": the k-mer Y[:-1] + x once, Y the circle k-mer ring_shape names; "first": the
    same on the fragment's first k-mer.  w.fragment is the fragment, w.circle the circle."""
    n, f0, f1, far = ring_shape(k)
    rng = _rng(k, stranded, 1000 + RING_SPURS.index(spur))
    c = bytes(ACGT[rng.integers(0, 4, n)])
    cc = c + c + c
    reads = [c + c[:k - 1]] * 2
    if spur != "none":
        y = cc[(far if spur == "far" else f0):][:k]
        reads.append(y[:-1] + bytes([b"ACGT"[(b"ACGT".index(y[-1]) + 1) % 4]]))
    w = World.__new__(World)
    w.k, w.stranded, w.hashes, w.branchy, w.reads, w.sizes = k, stranded, (2, 2), False, reads, BIG
    w._build(device)
    w.circle, w.fragment, w.spur = c, cc[f0:f1 + k - 1], spur
    return w


RING_CASES = tuple((K_MAIN, s, sp) for s in (True, False) for sp in RING_SPURS) + \
    tuple((k, i % 2 == 1 or k == 64, RING_SPURS[i % 3]) for i, k in enumerate(K_MATRIX))
RING_ROOMS = (AMPLE, 64)      # a call with ample room (the table in device scratch) and one that runs out of it (the table in LDS)


def hash_equal_fragments():
    """tw.hash_equal_world (k = 64, the read (AC) x 50): (AC)^32 and (CA)^32 hash alike, so the fragment (AC)^32 meets a candidate whose hash
    hit must fail on the bases (it is added), and the next candidate is the fragment's own k-mer"""
    return [b"AC" * 32, b"CA" * 32 + b"C", b"AC" * 40]


def answers(og, k, frags, min_cov, room=AMPLE, phases=None):
    return [restate(og, k, f, min_cov, room, 0 if phases is None else int(phases[i])) for i, f in enumerate(frags)]


@functools.lru_cache(maxsize=None)
def cpu_random(case):
    w = random_world(case)
    return w, random_case_fragments(w)


@functools.lru_cache(maxsize=None)
def cpu_ring(case):
    return ring_world(*case)


# ---- the worker's rules after overlapAndConnect (R/RNABloom.java:2182-2268), restated; graphutils.finishFragments is the batched form ----
KEPT, INCONSISTENT, SPURIOUS, EMPTY, NO_COMPLEX_KMER, TOO_SHORT = range(6)


def finish_restated(F, left_nk, right_nk, *, k, d, lookahead, min_num_kmer_pairs, extend, trim, support, trim_fn, extend_fn, counts_fn, is_repeat):
    """one connected fragment: (text or None, preExtensionFragLen, minCov, outcome, adopted).  support(text) -> a bool per k-mer i of
    lookupReadKmerPair(kmers[i], kmers[i + d]); trim_fn(text) -> the string the TRIM_EDGE overload's k-mers spell; extend_fn(text) -> the string
    naiveExtend's list spells; counts_fn(text) -> the k-mers' counts (float32)."""
    from test_paired_segment_rules import break_read
    cut = lambda t, r: t[r[0]:r[1] + k - 1]
    nk = len(F) - k + 1
    if d < nk:                                                                      # :2186
        ranges = break_read(support(F), nk, d, lookahead)                           # :2187 numPairsRequired = lookahead
        if len(ranges) != 1:
            return None, -1, None, INCONSISTENT, False
        r = ranges[0]
        if r[0] >= left_nk or r[1] < nk - right_nk:                                 # :2194
            return None, -1, None, SPURIOUS, False
        F = cut(F, r)
    if trim:                                                                        # :2205
        F = trim_fn(F)
        if len(F) < k:
            return None, -1, None, EMPTY, False
    pre = len(F) - k + 1 + k - 1                                                    # :2211
    adopted = False
    if extend:
        E = extend_fn(F)
        nk_e = len(E) - k + 1
        if nk_e != pre:                                                             # :2216 a k-mer count against a letter count, as written
            ranges = break_read(support(E), nk_e, d, min_num_kmer_pairs)            # :2218 the whole-list form
            if len(ranges) == 1:
                F, adopted = cut(E, ranges[0]), True
    nk = len(F) - k + 1
    if nk + k - 1 >= k + lookahead:                                                 # :2238
        min_cov = np.float32(min(counts_fn(F)))
        if any(not is_repeat(F[p:p + k]) for p in range(nk)):
            return F, pre, min_cov, KEPT, adopted
        return None, pre, min_cov, NO_COMPLEX_KMER, adopted
    return None, pre, None, TOO_SHORT, adopted


FINISH = dict(lookahead=7, minNumKmerPairs=10, maxTipLength=5, minKmerCov=1.0)
FINISH_SWITCHES = ((True, True), (False, False), (True, False))      # (extendFragments, trimArtifact)


def finish_world(stranded):
    """test_extend_step_rules.World at k = 25, d = 30: transcripts tiled with reads, read pairs stored"""
    import test_extend_step_rules as R
    return R.world(25, stranded)


def finish_fragments(w):
    """(fragment, leftNk, rightNk): stretches of one transcript of 1 .. 250 k-mers (some end where their transcript ends), chimeras of two
    transcripts with both parts long, with a short head and with a short tail, short fragments, runs of one letter"""
    rng, k = np.random.default_rng(55 + w.stranded), w.k
    tx = [t for t, _ in w.tx if len(t) >= 400 and len(set(t)) == 4]
    pick = lambda: tx[int(rng.integers(0, len(tx)))]
    out = []
    for i in range(40):
        t = pick()
        nk = int(rng.integers(1, 251))
        a = (0, len(t) - nk - k + 1)[i % 2] if i < 8 else int(rng.integers(0, len(t) - nk - k + 2))
        out.append((t[a:a + nk + k - 1], min(nk, 16), min(nk, 16)))
    for i in range(18):
        t1, t2 = pick(), pick()
        a, b = int(rng.integers(0, len(t1) - 120)), int(rng.integers(0, len(t2) - 120))
        n1, n2 = ((100, 100), (k + 8, 100), (100, k + 8))[i % 3]
        out.append((t1[a:a + n1] + t2[b:b + n2], 16, 16))
    for i in range(8):
        t = pick()
        a = int(rng.integers(50, len(t) - 100))
        out.append((t[a:a + k + i], 1 + i, 1 + i))
    out += [(b"C" * (k + 12), 5, 5), (b"A" * (k + 40), 16, 16)]
    return out


def finish_answers(w, extend, trim):
    import test_trim_artifact_rules as T
    from test_read_coverage_rules import is_repeat
    k, d, og, o = w.k, w.d, w.og, w.o
    P = FINISH

    def support(t):
        nk = len(t) - k + 1
        return [i + d < nk and o.lookup_read_pair(t[i:i + k], t[i + d:i + d + k]) for i in range(nk)]

    return [finish_restated(F, ln, rn, k=k, d=d, lookahead=P["lookahead"], min_num_kmer_pairs=P["minNumKmerPairs"], extend=extend, trim=trim, support=support,
                            trim_fn=lambda t: T.judge(og, k, w.stranded, t, T.EDGE, clip=P["maxTipLength"])[1],
                            extend_fn=lambda t: restate_chain(og, k, t, P["minKmerCov"], AMPLE)[0],
                            counts_fn=lambda t: og.get_kmers(t)[2], is_repeat=is_repeat)
            for F, ln, rn in finish_fragments(w)]
