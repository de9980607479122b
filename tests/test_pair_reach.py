"""On the CPU oracle alone: the proof that the worlds of tests/pair_worlds.py ask something.  tests/test_gpu_pair_matrix.py compares
rb_graph_overlap_pairs, rb_graph_extend_se, rb_graph_extend_pe and rb_graph_join_pairs with their restatements on these worlds at k = 16 ... 256;
a world that lost its forks, its walks or its rescued pairs when k grew would let a wrong kernel pass.  Each world asserts the reach check of
its class (assert_every_branch_is_reached, as the k = 25 worlds do), the overlap worlds also the pairs that exist only with more than 64
spanning k-mers or more than 64 shared letters, the extension worlds the queries at ex_one's packing boundaries.  A branch that cannot exist at
some k is excused in pair_worlds.EXCUSED, with its reason, and shown here to be absent indeed.  Each test prints the counts it rests on (-s
shows them).

The world classes got keyword parameters for their lengths to make this possible; the worlds the other tests build must not have changed by a
byte, and the first test holds their reads, queries or pairs, floors and fragments to SHA-256 digests recorded before that edit."""
import collections

import numpy as np
import pytest

import pair_worlds as PW
import test_extend_pe_rules as P
import test_extend_step_rules as R
import test_gpu_extend_pe as GP
import test_gpu_extend_step as EX
import test_gpu_join as GJ
import test_gpu_overlap as OV
import test_hash_counts_reach as HC
import test_join_rules as J
import test_overlap_rules as OR

IDS = [PW.case_id(c) for c in PW.CASES]


# ---- the worlds of the existing tests are what they were ----
def k143_world():
    """as tests/test_gpu_extend_pe.py::test_k_143_and_the_byte_counters builds it"""
    rng = np.random.default_rng(77)
    rnd = lambda n: np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()
    p = rnd(200) + GP.tail_143()
    extra = [(p + rnd(300), 1, [("tail-fork", p), ("tail-fork-short", p[-(143 + 20):])]), (p + rnd(300), 2, [])]
    return P.WorldPE(143, False, 1430, 30, 40, extra=extra, n_iso=2, read_len=400, tx_len=800)


OLD_WORLDS = {
    "step-25-0": (lambda: R.world(25, False), "e803070b7313fb5953f54c40fb3ad1633f024ba74a02bf61e43702b69ba8d316"),
    "step-25-1": (lambda: R.world(25, True), "72500ca05eb36db27d060bfcf15847399ca6b1a05738cbba51a981b27aa7cf5c"),
    "join-25-0": (lambda: J.world(25, False), "ee7a806374e01a0dd89f294da9b9f8326fc2e7c0800f94776e68ffdac345eaba"),
    "join-25-1": (lambda: J.world(25, True), "6f84f056b939a00c62bf0eb1890a647cbd0e9d73191497e6e5d5522ae1eff4b1"),
    "pe-25-0": (lambda: P.world(25, False), "e6817d62fafcf14d549a4f44edcb4df17f923692e2c1342c8481bf2f432b783d"),
    "pe-25-1": (lambda: P.world(25, True), "7e76f35e727aff4b167d483b0e0aacf7cafc16b822f62e7c706416a71ebbc970"),
    "step-d2": (lambda: EX.small_world(2), "1a5a0dfac41598bc34fb245b7de70d957db05a5d3f4385fee85cb68023cc9138"),
    "step-d3": (lambda: EX.small_world(3), "f9a34f0254a225c5394d448b5bd509802b98ed9007f6aae5b3798cb73ff9f26f"),
    "step-d256": (lambda: EX.small_world(256), "c00df2645430c47559068f9584859ff678290802aa32e13999676e22c76c3966"),
    "step-d300": (lambda: EX.small_world(300), "c1762775c73b1e5380eabe6a51261686c0628d8e3bca223347bf84c67da2e4ae"),
    "join-d2": (lambda: GJ.small_world(2), "ebae014e09265cc3ac5d34efa7ec722fa357d456e7bf1b6884867590bbe664ef"),
    "join-d3": (lambda: GJ.small_world(3), "7ebc686d1500b622b3d3b9fd6eea78aa2a920ff50b5a6e45a9330b5f02b29bad"),
    "join-d256": (lambda: GJ.small_world(256), "7c4d636fe48cbef6174644bc19eb9b0e2b45759cd51824166cb3fd3b9ef67762"),
    "join-d300": (lambda: GJ.small_world(300), "d3a9c0bcaf947279ba50622770f2f54f7447265af3a729c74b843d01aa0de66c"),
    "pe-d2-2": (lambda: GP.small_world(2, 2), "d3a96ad6975f8a253d48389c3650b600b59ccbcbbf07a71005297c520bbd20a1"),
    "pe-d2-3": (lambda: GP.small_world(2, 3), "22b494bd1f23b8842600a196d366e2044c86a8a49b7bdf246be6e1a953ef8a39"),
    "pe-d30-20": (lambda: GP.small_world(30, 20), "c422f5f0bfa23fd2fe8cbc5defe2632aad4ae2bc0114a7c45a9df2f762bed8fc"),
    "pe-d30-256": (lambda: GP.small_world(30, 256), "63a1f05c86d8f145256cff2f3e36793bcd3f8c0fce23b8a542c0dfaac2d44ef6"),
    "pe-d30-300": (lambda: GP.small_world(30, 300), "11d3e8a489244bddfd4497d9c50eee01ad7ebe05ba9647045bcea94c32dfbe7a"),
    "pe-k143": (k143_world, "55d877eb17909c4fe20b6713e8c3f50943af864afd5eb9d02c187fca5acc0e5d"),
    "step-h111": (lambda: HC.extend_case((1, 1, 1))[0], "6620c7413a15def89f3a725206b4af03aa87b70f298201382c09e852e13ebb0a"),
    "step-h333": (lambda: HC.extend_case((3, 3, 3))[0], "939dbfb9de8dcd2c203b0d30d419904b23b1a9cd0bb00679a0ea06a0087e0833"),
    "step-h231": (lambda: HC.extend_case((2, 3, 1))[0], "d179bc5ae17a0fd19a18d646835e6c58f32e71f4f1619f9fe1ddc22ea379b66d"),
    "overlap-h111": (lambda: HC.overlap_case((1, 1, 1))[0], "aad7b7b2e4af57f4df78c8583cc8305c93d6ae081e649423f6a5f60f47916860"),
    "overlap-h333": (lambda: HC.overlap_case((3, 3, 3))[0], "4defc9d5ff1911e6c4c1985b1c9aacc2c4565be56b59f2720e6a478039082605"),
    "overlap-h231": (lambda: HC.overlap_case((2, 3, 1))[0], "de5f7cae602bd9edffa5105c5da4a8cbe9db7d076db9ccbdfc5d558ac7653f1e"),
    "overlap-25-0": (lambda: OV.world(25, False), "6b548a22abff6211413b361191f080df10c22124563ed94d4cf1126511b18508"),
    "overlap-25-1": (lambda: OV.world(25, True), "0216cd064f487fe5d18ed9b3373c385c70b0ee8a75feeb2e17da370ad11c16a9"),
    "overlap-21-0": (lambda: OV.world(21, False), "5cf23fa12710245671ee41f6738b1e0fc209853367acd9a47f56941e8b705e61"),
    "overlap-rescue": (lambda: OV.World(25, False, seed=77, n_tx=8, n_single=16), "1e27a404288686da300a89109d71bf87de31e9d74c547f54fd4905876ce1bc6d"),
}


def test_old_worlds_cover_every_hash_count_world():
    assert {(1, 1, 1), (3, 3, 3), (2, 3, 1)} == set(HC.HASHES)


@pytest.mark.parametrize("name", sorted(OLD_WORLDS))
def test_existing_worlds_are_unchanged_byte_for_byte(name):
    make, want = OLD_WORLDS[name]
    assert PW.digest_of(make()) == want


# ---- the matrix ----
def test_matrix_spreads_the_axes():
    assert PW.KS == (16, 31, 32, 33, 62, 63, 64, 65, 127, 128, 129, 143, 192, 193, 255, 256)
    assert len({(c.k, c.stranded) for c in PW.CASES}) == len(PW.CASES) == 32
    for k in PW.KS:
        assert {c.stranded for c in PW.CASES if c.k == k} == {False, True}
    for h in PW.TRIPLES:
        mine = [c for c in PW.CASES if c.hashes == h]
        assert len(mine) >= 6 and any(c.k >= 64 for c in mine) and {c.stranded for c in mine} == {False, True}, h
    # every k that has an overlap below k with more than 64 spanning k-mers also has one of more than 64 letters, and the other way round
    for k in PW.KS:
        assert PW.has_long_spans(k, OV.MO) == (k >= 66)
    assert sum(k - 2 >= PW.WRAP for k in PW.KS) >= 2


def test_the_excuse_table_is_small_and_says_why():
    outcome_names = {"NONE", "SINGLE", "FIRST", "SECOND", "JOINED", "LEFT", "RIGHT", "MERGED", "SPANNED", "RESCUE"}
    for (call, k), entries in PW.EXCUSED.items():
        assert call in PW.CALLS and call != "overlap" and k in PW.KS and k > 33, (call, k)
        for branch, why in entries.items():
            assert isinstance(branch, str) and branch.upper() not in outcome_names and why, (call, k, branch)


ABSENT = collections.defaultdict(set)          # {(call, k, branch): the strandednesses of the worlds that lack it}, filled by the tests below


def lacking(w):
    """the tags that the steps of one direction or the other do not have"""
    by_direction = [set().union(*(st.tags for st, q in zip(w.want(), w.queries) if q[2] == direction)) for direction in (0, 1)]
    return (P.NEED_TAGS | by_direction[0] | by_direction[1]) - (by_direction[0] & by_direction[1])


def excused(case, call, w):
    """the branches excused at the case's k; an entry is used if one of the two worlds of that k lacks the branch in a direction"""
    ex = set(PW.EXCUSED.get((call, case.k), {}))
    for branch in ex & (lacking(w) if ex else set()):
        ABSENT[(call, case.k, branch)].add(case.stranded)
    return ex


def check_seed_queries(w, k):
    """ex_one's packing: an N at the last base and at the first base of the last packed byte refuses the seed, a lower-case letter there
    does not and the fork is seen, an N one letter in front of the last k-mer does no harm; from k = 253 on extended sequences whose last base
    — base 252 ... of the row, the last lane's — is no A"""
    got = collections.defaultdict(list)
    for st, (kind, s, direction) in zip(w.want(), w.queries):
        if kind.startswith("seed-"):
            last = s[-k:] if direction == 0 else s[:k]
            got[(kind, direction, R.is_acgtu(last))].append((st, last))
    for direction in (0, 1):
        for kind in ("seed-last-base", "seed-last-byte"):
            assert len(got[(kind, direction, False)]) >= 1 and all(st.why == R.WHY_INVALID_SEED for st, _ in got[(kind, direction, False)])
            valid = got[(kind, direction, True)]
            assert len(valid) >= 1 and all(st.n_cand >= 2 for st, _ in valid), (kind, direction)
            assert all(last != last.upper() for _, last in valid)
        before = got[("seed-n-before", direction, True)]
        assert len(before) >= 2 and all(st.n_cand >= 2 for st, _ in before)
        assert not got[("seed-n-before", direction, False)]
        if k >= 253:
            ends = [(s[-1:] if direction == 0 else s[:1]) for st, (_, s, dd) in zip(w.want(), w.queries) if dd == direction and st.outcome != R.NONE]
            assert sum(e not in b"Aa" for e in ends) >= 20


@pytest.mark.parametrize("case", PW.CASES, ids=IDS)
def test_extension_world(case):
    w = PW.step_case(case)
    assert excused(case, "step", w) == set()
    w.assert_every_branch_is_reached()
    check_seed_queries(w, case.k)
    for direction in (0, 1):
        steps = [st for st, q in zip(w.want(), w.queries) if q[2] == direction]
        print("extend_se %s direction %d: %d queries, (outcome, why) %s" % (PW.case_id(case), direction, len(steps), PW.outcome_counts((st.outcome, st.why) for st in steps)))
    assert len(w.queries) <= 340


@pytest.mark.parametrize("case", PW.CASES, ids=IDS)
def test_extension_pe_world(case, monkeypatch):
    w = PW.pe_case(case)
    ex = excused(case, "pe", w)
    monkeypatch.setattr(P, "NEED_TAGS", P.NEED_TAGS - ex)
    w.assert_every_branch_is_reached()
    check_seed_queries(w, case.k)
    for direction in (0, 1):
        steps = [st for st, q in zip(w.want(), w.queries) if q[2] == direction]
        print("extend_pe %s direction %d: %d queries, (outcome, why) %s, excused %s" % (
            PW.case_id(case), direction, len(steps), PW.outcome_counts((st.outcome, st.why) for st in steps), sorted(ex)))
    assert len(w.queries) <= 420


@pytest.mark.parametrize("case", PW.CASES, ids=IDS)
def test_join_world(case):
    w = PW.join_case(case)
    assert (w.BOUND, w.GRAD, w.TIP, w.MIN_COV) == case.join
    assert (("join", case.k) in PW.EXCUSED) is False
    w.assert_every_branch_is_reached()                          # (at most 2 % of the pairs NOT_JUDGED among its conditions)
    want = w.want()
    print("join %s: %d pairs, (outcome, why) %s, l_end %s, r_end %s" % (PW.case_id(case), len(want), PW.outcome_counts((r.outcome, r.why) for r in want),
                                                                   PW.outcome_counts(r.l_end for r in want), PW.outcome_counts(r.r_end for r in want)))
    # the pairs made on purpose end as they were made to
    made = [(r.why, r.l_end, r.r_end) for r in want[-4:]]
    assert made[0][1] == J.STEP_NONE and made[1][2] == J.STEP_NONE, made
    if case.k % 64 > 1:       # (at k = 0 and 1 mod 64 ntHash gives all runs of 64 equal letters one hash: the runs of A lend their exits to the run of G)
        assert made[2][1] == J.EXT_HOMOPOLYMER and made[3][2] == J.EXT_HOMOPOLYMER, made


@pytest.mark.parametrize("case", PW.CASES, ids=IDS)
def test_overlap_world(case):
    k, (mo, mincov) = case.k, case.overlap
    w = PW.overlap_case(case)
    want = w.want(mincov)
    w.assert_every_branch_is_reached()
    print("overlap %s: %d pairs, (outcome, why, swapped) %s" % (PW.case_id(case), len(want), PW.outcome_counts(rec[:3] for rec, _ in want)))
    # no spanning k-mer is a homopolymer, whatever the pair (pair_worlds' docstring)
    spans = 0
    for rec, text in want:
        for i in range(rec[5], rec[5] + rec[6]):
            assert not OR.is_homopolymer(text[i:i + k])
        spans += rec[6] > 0
    assert spans >= 20
    by_kind = collections.defaultdict(list)
    for i, kind in enumerate(w.kind):
        by_kind[kind].append(i)
    if not PW.has_long_spans(k, mo):
        assert not [kind for kind in by_kind if kind.endswith(("-64", "-65")) or kind.startswith("repeat-wrap")]
        return
    R64 = PW.SPAN_ROUND
    recs = lambda kind: [want[i][0] for i in by_kind[kind]]
    # spanned with 65 spanning k-mers and more: a second round of the spanning loop, every k-mer of it good
    assert [(r[0], r[6] > R64) for r in recs("span-65")] == [(OR.SPANNED, True)] * 2 and recs("span-65")[0][6] == R64 + 1
    # rescued, the first spanning k-mer below min_kmer_cov at index 64, and the last one of all
    firsts = []
    for i in by_kind["rescue-bad-64"]:
        counts = PW.span_counts(w, i, mincov)
        assert want[i][0][:2] == (OR.RESCUE, OR.FOUND) and len(counts) > R64
        firsts.append((next(j for j, c in enumerate(counts) if c < mincov), len(counts)))
    assert firsts[0][0] == R64 and firsts[1][0] == firsts[1][1] - 1 >= R64, firsts
    # rescued by a singleton that is the 65th k-mer asked on its read, and refused when that k-mer counts 2 as the 64 before it do
    for side, why in (("right", OR.NO_RIGHT_SINGLETON), ("left", OR.NO_LEFT_SINGLETON)):
        (i,), (j,) = by_kind["rescue-%s-64" % side], by_kind["none-%s-64" % side]
        assert want[i][0][:4] == (OR.RESCUE, OR.FOUND, 0, R64 + 1) and want[j][0][:4] == (OR.NONE, why, 0, R64 + 1), (side, want[i][0], want[j][0])
        for x, last_is_single in ((i, True), (j, False)):
            left, right = w.pairs[x]
            c = [float(v) for v in (w.o.counts(right)[:R64 + 1] if side == "right" else w.o.counts(left)[-(R64 + 1):])]
            assert all(v >= 2.0 for v in c[:R64]) and (c[R64] == 1.0) == last_is_single, (side, c)      # (2, or more where the counting filter collides)
    # isRepeat's signed byte
    if k - 2 >= PW.WRAP:
        (i,), (j,) = by_kind["repeat-wrap-%d" % PW.WRAP], by_kind["repeat-wrap-%d" % (PW.WRAP - 1)]
        assert want[i][0][:4] == (OR.RESCUE, OR.FOUND, 0, PW.WRAP) and want[j][0][:4] == (OR.NONE, OR.REPEAT, 0, PW.WRAP - 1)
        shared = w.pairs[i][1][:PW.WRAP]
        assert not OR.is_repeat(shared) and P.is_repeat(shared, byte_counters=False)       # counters that do not wrap would refuse the pair
    else:
        assert not [kind for kind in by_kind if kind.startswith("repeat-wrap")]


def test_no_excuse_is_unused():
    """behind the worlds' tests, whose findings it takes (a world they have not built is built here): each entry of the table names a branch
    that a world of its k lacks"""
    for (call, k), entries in PW.EXCUSED.items():
        for branch in entries:
            if not ABSENT[(call, k, branch)]:
                for case in (c for c in PW.CASES if c.k == k):
                    if branch in lacking(getattr(PW, call + "_case")(case)):
                        ABSENT[(call, k, branch)].add(case.stranded)
            assert ABSENT[(call, k, branch)], (call, k, branch)
