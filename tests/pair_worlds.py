"""The worlds of tests/test_gpu_pair_matrix.py and tests/test_pair_reach.py: graphs for rb_graph_overlap_pairs, rb_graph_extend_se,
rb_graph_extend_pe and rb_graph_join_pairs at k = 16 ... 256, stranded and canonical, with hash counts other than (2, 2, 2), from the World
classes of tests/test_gpu_overlap.py, tests/test_extend_step_rules.py, tests/test_extend_pe_rules.py and tests/test_join_rules.py.  Those
classes were written at k = 25 and hold lengths in letters (flanks, repeat counts, homopolymer runs, read lengths); here every such length is
derived from k so that a world looks in K-MERS as the k = 25 world does: a length of n letters becomes n + (k - 25), a unit repeated r times is
repeated often enough to cover as many k-mers as before.  Below k = 25 the lengths stay what they are.  Around the slot boundaries of the
kernels k takes both neighbours, as tests/correction_worlds.py has them, and 255 beside 256: ex_one packs the last k-mer four bases to a lane
and k = 253 ... 256 reach lane 63, 255 with a partial last byte.

On top of what the classes hold, the overlap worlds get pairs that only exist at large k (overlap_extras) and the extension worlds get queries
whose bad letter sits at the packing boundaries of ex_one (seed_queries).  Two kinds that the spanning loop's code suggests cannot exist and
are not here: a spanned pair
whose only spanning k-mer that is no homopolymer has index >= 64, and one whose only such k-mer has index < 64.  EVERY spanning k-mer holds
all shared letters, the letter in front of them on the left read and the letter behind them on the right read; were it a homopolymer the
reads would agree one shift earlier and share one letter more (tests/test_overlap_rules.py::test_a_valid_span_is_always_complex).  The reach
file asserts that on every record with a span.

The CPU file proves that the worlds ask something, the GPU file compares; a world holds its restatement's answers, computed once.  (Only the
last two worlds of a call are kept: one has filters of up to 48 MB.)"""
import collections
import functools
import hashlib

import numpy as np

import correction_worlds as CW
import test_extend_pe_rules as P
import test_extend_step_rules as R
import test_gpu_overlap as OV
import test_join_rules as J
from traversal_worlds import _prime_above

ACGT = np.frombuffer(b"ACGT", np.uint8)
KS = tuple(sorted(CW.KS + (255,)))
# (dbgbf, cbf, pair filters): (2, 2, 3) is the graph's fast path with the generic pair probe, (3, 1, 2) the reverse
TRIPLES = ((1, 1, 1), (3, 4, 3), (2, 2, 3), (3, 1, 2), (2, 2, 2))
D_READ, D_FRAG = 30, 80                                           # the walk rows stay in LDS; the distances' edges are tested at k = 25

# k, stranded, (dbgbf, cbf, pair) hash counts, read-pair and fragment distance, join's (bound, gradient, tip, min_kmer_cov), overlap's
# (min_overlap, min_kmer_cov).  Case number i = 2 * (index of k) + (0 stranded, 1 canonical); the hash counts go round in i, so each triple
# occurs six or seven times, on both strandednesses, at k >= 64 as well.  The extension's floors are the worlds' own (1 / 2 / 5 / 1e6 by query).
Case = collections.namedtuple("Case", "k stranded hashes d_r d_f join overlap")
CASES = tuple(Case(k, i % 2 == 0, TRIPLES[i % 5], D_READ, D_FRAG, (J.JoinWorld.BOUND, J.JoinWorld.GRAD, J.JoinWorld.TIP, J.JoinWorld.MIN_COV), (OV.MO, 1.0))
              for i, k in ((2 * j + s, k) for j, k in enumerate(KS) for s in (0, 1)))
N_JOIN_PAIRS = 700                                                # as at k = 25: REACHED_LEFT and the step's rarer ends come up once or twice in 700 pairs
SPAN_ROUND = 64                                                   # windows a round of the spanning loop and of ov_any_singleton takes
WRAP = 142                                                        # the shortest overlap whose isRepeat threshold round(0.9 n) a signed byte cannot hold

# What a world's assert_every_branch_is_reached asks for and cannot exist at that k: {(call, k): {branch: why}}.  Nothing for k <= 33, no
# outcome value, nothing of overlap_extras.
EXCUSED = {
    # a first stretch with fragment pairs and no read pair.  Chain k-mer i is asked with the path's k-mers n - 30 + i (read) and n - 80 + i
    # (fragment).  From k = 80 on the k-mers n - 80 + i and the chain's i overlap, so whatever holds them 80 apart holds every path k-mer in
    # between, and a fragment stores its pairs at the read distance too (FragmentsToGraphWorker; WorldPE does as it does): a read pair is
    # there.  And a letter that is no base inside path k-mer n - 30 + i and outside n - 80 + i lies at n + i or behind: in the last k-mer, which
    # the call then refuses.  No transcript, fragment or query places it; a world has it where the fragment-pair filter gives a false positive
    # to a branch without read pairs.  (Up to k = 50 an N does it: pe_case's fork2-n-frag.)
    ("pe", k): {"frag_only_first_stretch": "no fragment holds a pair at the fragment distance without the read pairs between, from k = 80 on"}
    for k in KS if k >= 80
}


def case_id(case):
    return "k%d-%s-h%d%d%d" % ((case.k, "stranded" if case.stranded else "canonical") + case.hashes)


# Which of the rarer branches a world of random transcripts reaches is luck (the k = 25 worlds have their seeds for the same reason): a
# (call, k, stranded) listed here takes the n-th seed behind its own, the first with which its assert_every_branch_is_reached holds
RESEED = {("join", 31, False): 2, ("join", 33, True): 1, ("join", 64, True): 1, ("join", 128, False): 1, ("join", 192, False): 1}     # (no step there overshot the bound)


CALLS = dict(step=1, join=2, pe=3, overlap=5)


def seed_of(case, call):
    return 10_000_000 * RESEED.get((call, case.k, case.stranded), 0) + 1_000_000 * CALLS[call] + 1000 * case.k + 100 * case.hashes[0] + 10 * case.hashes[1] + 2 * case.hashes[2] + (1 if case.stranded else 0)


def grow(k):
    """letters a length of the k = 25 worlds gains"""
    return max(k - 25, 0)


def more_reps(k, unit):
    """repeats of a unit of `unit` letters that cover grow(k) letters"""
    return -(-grow(k) // unit)


def sizes_of(hashes):
    """(dbgbf, cbf, pair filter, fragment-pair filter) slots.  A filter with one function gets eight times the room, or false positives of a
    few per cent open forks everywhere and support branches no read holds; dbgbf and cbf differ in size, or with one function each a false
    positive of dbgbf would read the count of the very k-mer it collides with (tests/correction_worlds.py)"""
    room = lambda h, slots: _prime_above(slots * (8 if h == 1 else 1))
    return room(hashes[0], 6_000_000), room(hashes[1], 5_000_000), room(hashes[2], 5_000_000), room(hashes[2], 3_000_000)


def digest(*parts):
    """SHA-256 over lists of reads, queries, pairs and floors (their repr) and packed reads (the arrays' bytes)"""
    h = hashlib.sha256()
    for p in parts:
        if isinstance(p, tuple) and p and isinstance(p[0], np.ndarray):
            for a in p:
                h.update(np.ascontiguousarray(a).tobytes())
        else:
            h.update(repr(p).encode())
        h.update(b"|")
    return h.hexdigest()


def digest_of(w):
    """of everything a world is made of that goes into a graph or a call"""
    if isinstance(w, P.WorldPE):
        return digest(w.w.reads, w.extra_packed, w.queries, w.floors, w.frags)
    if isinstance(w, J.JoinWorld):
        return digest(w.w.reads, w.w.queries, w.w.floors, w.pairs)
    if isinstance(w, OV.World):
        return digest(w.reads, w.pairs, w.kind)
    return digest(w.reads, w.queries, w.floors)


# ---- the extension worlds (extend_se, join, extend_pe share the transcripts' recipe) ----
def step_kw(case, call):
    """R.World's keywords at the case's k: reads of k + 75 letters every 10 (a k-mer in 7 or 8 reads, a pair d apart in 4 or 5, as at k = 25),
    transcripts with 226 k-mers before and after the fork"""
    k, g = case.k, grow(case.k)
    r14 = more_reps(k, 14)
    lengths = dict(flank=100 + g, unit_reps=12 + r14, tandem_query_reps=2 + r14, circle_reps=4 + r14, poly_run=60 + g,
                   poly_tx=max(120 + g, 3 * (k + 15)), poly_query=30 + g)
    return dict(d=case.d_r, read_len=100 + g, tile=10, tx_len=500 + 2 * g, hashes=case.hashes, sizes=sizes_of(case.hashes)[:3], lengths=lengths,
                extra_tx=tuple(extra_transcripts(k, case.d_r, seed_of(case, call) + 7)))


def extra_transcripts(k, d, seed):
    """(transcript, multiplicity, queries) on top of R.World's own, for two branches that its transcripts reach by luck or not at all:
    - a walk that meets its start again.  R.World has it from C x (k + 3), whose only successor is itself; but at k = 0 and 1 mod 64 ntHash
      gives every homopolymer of 64 letters one hash, A^k (or A^64 z) of another transcript answers for C^k's neighbours and the walk forks.
      Its `circle` is left through the reversed tandem transcript after a few steps.  Here: a circle of 20 k-mers (< d - 2) that is nothing else;
    - a tie of two scores decided by coverage: a fork of coverage 1 : 3 whose heavier branch begins with the later base, asked with an N
      among the last d k-mers (the path's minimum count is 0 and both scores are)"""
    rng = np.random.default_rng(seed)
    rnd = lambda n: ACGT[rng.integers(0, 4, n)].tobytes()
    c = rnd(min(20, d - 3))
    reps = -(-(k + d + 80) // len(c))
    out = [(c * reps, 1, [("circle-alone", (c * reps)[5:5 + k + 10])])]
    p, a, b = rnd(k + 150), rnd(k + 100), rnd(k + 100)
    a, b = b"A" + a[1:], b"G" + b[1:]
    return out + [(p + a, 1, [("tie-fork", R.put(p, len(p) - k - 4, "N"))]), (p + b, 3, [])]


def seed_queries(w, n_iso=6):
    """[(kind, sequence)] for ex_one's packing of the last k-mer (four bases to a lane): the sequence up to each fork with a letter that is no
    base (N: the seed is refused) or a lower-case one (read as its upper case) at the last base, at base k - 1 - (k - 1) % 4 of the last
    k-mer — the first of its last packed byte —, and an N one letter before the last k-mer, which is valid"""
    k, out = w.k, []
    forks = [i for i in range(n_iso) if w.tx[2 * i][0][len(w.tx[2 * i][0]) // 2] != w.tx[2 * i + 1][0][len(w.tx[2 * i][0]) // 2]]
    assert len(forks) >= 2                                        # (the others fork one base on: their branches begin alike)
    for j, i in enumerate(forks):
        t = w.tx[2 * i][0]
        p = t[:len(t) // 2]
        bad = (lambda s, at: R.put(s, at, "N")) if j % 2 == 0 else (lambda s, at: s[:at] + s[at:at + 1].lower() + s[at + 1:])
        first = len(p) - k
        out += [("seed-last-base", bad(p, len(p) - 1)), ("seed-last-byte", bad(p, first + k - 1 - (k - 1) % 4)), ("seed-n-before", R.put(p, first - 1, "N"))]
    return out


def add_seed_queries(w):
    """appended to a world's queries in both directions, floor 1"""
    for kind, s in seed_queries(w):
        w.queries += [(kind, s, 0), (kind, s[::-1], 1)]
        w.floors += [1.0, 1.0]


@functools.lru_cache(maxsize=2)
def step_case(case):
    w = R.World(case.k, case.stranded, seed_of(case, "step"), **step_kw(case, "step"))
    add_seed_queries(w)
    return w


@functools.lru_cache(maxsize=2)
def join_case(case):
    k, g = case.k, grow(case.k)
    kw = step_kw(case, "join")
    kw["world_read_len"] = kw.pop("read_len")
    lengths = kw["lengths"]
    # the left read of a run's first pair ends k - 20 letters into the run: its walk meets the homopolymer k-mer inside the bound of 20
    pl = dict(fork_tx=2 * lengths["flank"] + lengths["poly_run"], a_run=40 + g, c_run=100 + g, run_left=max(5, k - 20), run_right=55 + g, run_second=20)
    tx, pairs = join_extras(k, k + 15, seed_of(case, "join") + 8)
    kw["extra_tx"] += tuple(tx)
    return J.JoinWorld(case.k, case.stranded, seed_of(case, "join"), n_pairs=N_JOIN_PAIRS, pair_lengths=pl, extra_pairs=pairs, **kw)


def join_extras(k, L, seed):
    """(transcripts for R.World's extra_tx, pairs): the ends of a walk that random pairs reach once in some hundreds, made on purpose, each
    for the left walk and — with the reversed transcripts, which R.World inserts too — for the right walk.  Both need a threshold that
    keeps two neighbours: the reads begin at a transcript's first letter, where one read covers a k-mer.
    - a fork the step cannot decide (STEP_NONE; from the left, the right walk then comes back to left's last k-mer: REACHED_LEFT): one
      transcript ends with the k-mer X, two begin with its last k - 1 letters, and no read holds a k-mer of both sides;
    - a step whose extension is a homopolymer (EXT_HOMOPOLYMER): a transcript of 32 letters and a run of G, which ends it.  The walk comes to
      C G^(k-1) after 16 k-mers; its successors are G^k and G^(k-1) C (the reversed transcript leaves the run there), and only G^k has a
      read pair with the path, k-mer 2 of the transcript.  No other transcript has a run of G"""
    rng = np.random.default_rng(seed)
    rnd = lambda n: ACGT[rng.integers(0, 4, n)].tobytes()
    x, p, s2, s3 = rnd(k), rnd(150), b"C" + rnd(k + 120), b"G" + rnd(k + 120)
    t1, t2, t3 = p + x, x[1:] + s2, x[1:] + s3
    tx = [(t1, 1, []), (t2, 1, []), (t3, 1, [])]
    pairs = [(t1[-L:], t2[5:5 + L]), (t2[::-1][:L], t1[::-1][:L])]
    t4 = rnd(31) + b"C" + b"G" * (100 + grow(k))
    tx += [(t4, 1, [])]
    pairs += [(t4[:L], t2[-L:]), (t2[::-1][:L], t4[::-1][-L:])]
    return tx, pairs


@functools.lru_cache(maxsize=2)
def pe_case(case):
    k, g = case.k, grow(case.k)
    kw = step_kw(case, "pe")
    d_r = kw.pop("d")
    extras = P.extras(k, case.d_f, seed_of(case, "pe") + 4, lengths=dict(flank=150 + g, circle_reps=8 + more_reps(k, 40)))
    # the tie decided by coverage, as extra_transcripts has it, with both branches fragments as a whole: the letter replaced 4 in front of
    # the last k-mer takes k k-mers off the path, and a branch is scored only with a read pair (chain k-mers 26 ...) AND a fragment pair (76 ...)
    rng = np.random.default_rng(seed_of(case, "pe") + 5)
    rnd = lambda n: ACGT[rng.integers(0, 4, n)].tobytes()
    p, a, b = rnd(k + case.d_f + 100), b"A" + rnd(k + case.d_f + 50), b"G" + rnd(k + case.d_f + 50)
    extras += [(p + a, 1, [("tie-fork-pe", R.put(p, len(p) - k - 4, "N"))], p + a), (p + b, 3, [], p + b)]
    # a third of the transcripts are fragments up to 50 k-mers behind the fork, as at k = 25 (0.6 of 500 letters): walks of d_f - 1 k-mers
    # lose their fragment pairs there and are trimmed
    part = 0.6 if k <= 25 else (275 + k) / kw["tx_len"]
    w = P.WorldPE(k, case.stranded, seed_of(case, "pe"), d_r, case.d_f, extra=extras, fsize=sizes_of(case.hashes)[3],
                  second_level_lengths=dict(prefix=100 + g, branch=50 + g), frag_part=part, **kw)
    if k <= 50:
        # a first stretch with fragment pairs and no read pair (see EXCUSED): before the second forks 5 and 12 k-mers on, an N inside all
        # the path k-mers the stretch is asked with at the read distance (n - 30 ...) and none of those at the fragment distance (n - 80 ...)
        for i, g2 in ((0, 5), (5, 12)):
            t = w.tx[2 * 6 + 3 * i][0]
            s = t[:len(t) // 2]
            s = R.put(s, len(s) - k + 1 - d_r + min(k, g2) - 1, "N")
            w.queries += [("fork2-n-frag", s, 0), ("fork2-n-frag", s[::-1], 1)]
            w.floors += [1.0, 1.0]
    add_seed_queries(w)
    return w


# ---- the overlap worlds ----
def overlap_lengths(k):
    g = grow(k)
    # (the singleton reads grow by 2 g: the pair with an N among k - 5 shared letters needs left k-mers in front of the N's, 2 k - 6 letters;
    # a dovetail below k needs min(ll, rl) * 3 / 4 - 1 <= k - 1, which k + 7 letters break below k = 19)
    return dict(tx=500 + 2 * g, read=100 + g, single_tx=300 + 4 * g, single_read=(60 + 2 * g, 110 + 2 * g), dovetail_span=min(7, (4 * k + 3) // 3 - k), pair_read=(40 + g, 150 + g), inside_left=150 + g,
                inside_end=110 + g, contained=60 + g, long_merge=30 + g, long_span=min(15, k - 1), long_read=100 + g)


def wrap_text(n):
    """n letters A with a C at 5, 16, 27, ...: ten A in eleven letters reach round(0.9 n), and no dinucleotide or trinucleotide phase reaches
    its threshold (tests/test_extend_pe_rules.py::test_is_repeat_is_the_reference_s has the same text at 143)"""
    t = bytearray(b"A" * n)
    for p in range(5, n, 11):
        t[p] = ord("C")
    return bytes(t)


def has_long_spans(k, min_overlap):
    """can an overlap below k have 65 spanning k-mers?  k - 1 - overlap of them, the overlap at least min_overlap"""
    return k - 1 - min_overlap > SPAN_ROUND


def overlap_extras(k, min_overlap, seed):
    """(reads, [(kind, left, right)]): the pairs that need more than 64 spanning k-mers or an overlap of more than 64 letters below k.
    `Single` pairs are the two reads of a transcript nothing else covers, inserted once: their k-mers count 1 and the spanning k-mers are
    absent, unless a read is added that holds some of them."""
    rng = np.random.default_rng(seed)
    rnd = lambda n: ACGT[rng.integers(0, 4, n)].tobytes()
    reads, pairs = [], []
    if not has_long_spans(k, min_overlap):
        return reads, pairs
    o_max = k - 2 - SPAN_ROUND                                    # 65 spanning k-mers
    # spanned, 65 spanning k-mers and the most there can be: a transcript tiled with reads
    t = rnd(3 * k + 200)
    reads += [t[a:a + k + 75] for a in range(0, len(t) - k - 74, 10)]
    for o in (o_max, min_overlap):
        pairs.append(("span-65", t[20:k + 100], t[k + 100 - o:2 * k + 180 - o]))
    # rescued: the spanning k-mers 0 .. first_bad - 1 are in a read of their own, the next one is in none
    o = max(min_overlap, min(20, o_max))
    for first_bad in (SPAN_ROUND, k - 2 - o):
        t = rnd(2 * k + 200)
        ll = k + 60
        reads += [t[:ll], t[ll - o:ll - o + k + 60], t[ll - k + 1:ll + first_bad]]
        pairs.append(("rescue-bad-64", t[:ll], t[ll - o:ll - o + k + 60]))
    # rescued, an overlap of 65: the right read's k-mers 0 .. 63 are in a second read (they count 2) and only k-mer 64 of the 65 asked counts
    # 1; the same for the left read's k-mers nka - 65 .. nka - 2.  And the same pairs with the second read one k-mer longer: no singleton
    o = SPAN_ROUND + 1
    for side in ("right", "left"):
        for n_twice, kind in ((SPAN_ROUND, "rescue-%s-64" % side), (o, "none-%s-64" % side)):
            t = rnd(3 * k + 300)
            ll = k + o + 20
            left, right = t[:ll], t[ll - o:ll + k + 30]
            twice = right[:k - 1 + n_twice] if side == "right" else left[ll - k + 1 - o:ll - o + n_twice]
            reads += [left, right, twice]
            pairs.append((kind, left, right))
    # isRepeat's signed-byte counter: 142 shared letters (threshold 128: the A counter wraps at 128 and never gets there) against 141 (127)
    if k - 2 >= WRAP:
        for o in (WRAP, WRAP - 1):
            w, m, z = rnd(k + 20), wrap_text(o), rnd(k + 20)
            reads += [w + m, m + z]
            pairs.append(("repeat-wrap-%d" % o, w + m, m + z))
    return reads, pairs


@functools.lru_cache(maxsize=2)
def overlap_case(case):
    k = case.k
    assert case.overlap[0] == OV.MO
    reads, pairs = overlap_extras(k, case.overlap[0], seed_of(case, "overlap") + 1)
    h = case.hashes
    sizes = sizes_of(h)[:2] + (_prime_above(400_000),)
    return OV.World(k, case.stranded, seed_of(case, "overlap"), hashes=h, sizes=sizes, lengths=overlap_lengths(k), extra_reads=reads, extra_pairs=pairs)


def span_counts(w, i, min_kmer_cov=1.0):
    """of pair i of an overlap world, from its record: the counts of its spanning k-mers"""
    rec, text = w.want(min_kmer_cov)[i]
    return [float(c) for c in w.o.counts(text)[rec[5]:rec[5] + rec[6]]]


def outcome_counts(records):
    out = collections.Counter(records)
    return sorted(out.items())
