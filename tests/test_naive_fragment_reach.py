"""What the worlds of tests/naive_fragment_worlds.py reach on the CPU oracle — so that tests/test_gpu_naive_fragments.py, which compares the device
with the same restatement, is known to pass through every end of GraphUtils.naiveExtend's two walks — and the literal restatement of the
FragmentAssembler's rules after overlapAndConnect (R/RNABloom.java:2182-2268) against hand-worked cases."""
import collections

import numpy as np
import pytest

import naive_fragment_worlds as NW
import traversal_worlds as tw
from rnabloom import _native as N
from test_paired_segment_rules import pattern

ENDS = (NW.END_NO_NEIGHBOUR, NW.END_BACK_BRANCH, NW.END_SEVERAL, NW.END_MEMBER, NW.END_ROOM)


@pytest.fixture(scope="module")
def reached():
    """every (world, fragment, min_cov, room) of the device test with its restated record"""
    out = []
    for case in NW.RANDOM_CASES:
        w, frags = NW.cpu_random(case)
        for mc in NW.MIN_COVS:
            for room in (256, NW.AMPLE):
                out += [("random", case, f, mc, room, a) for f, a in zip(frags, NW.answers(w.og, w.k, frags, mc, room))]
    for case in NW.RING_CASES:
        w = NW.cpu_ring(case)
        for mc in NW.MIN_COVS:
            for room in NW.RING_ROOMS:
                out.append(("ring", case, w.fragment, mc, room, NW.restate(w.og, w.k, w.fragment, mc, room)))
    w = tw.hash_equal_world(True)
    out += [("hash_equal", (64, True), f, 1.0, 64, a) for f, a in zip(NW.hash_equal_fragments(), NW.answers(w.og, 64, NW.hash_equal_fragments(), 1.0, 64))]
    return out


def test_every_end_occurs_on_each_side_at_least_three_times(reached):
    left, right = collections.Counter(r[5]["left_end"] for r in reached), collections.Counter(r[5]["right_end"] for r in reached)
    for e in ENDS:
        assert left[e] >= 3 and right[e] >= 3, (e, left, right)
    assert right[NW.END_NOT_RUN] >= 3                                    # behind a left walk that ran out of room
    # the k = 25 random worlds alone: the three ends a random world gives, on both sides, and extensions of some length in a clean world
    k25 = [r[5] for r in reached if r[0] == "random" and r[1][0] == NW.K_MAIN]
    assert len(k25) == 4 * 31 * 2 * 2
    for e in ENDS[:3]:
        assert sum(a["left_end"] == e for a in k25) >= 3 and sum(a["right_end"] == e for a in k25) >= 3, e
    assert max(max(a["left_ext"], a["right_ext"]) for a in k25) >= 20


def test_member_is_met_in_the_fragment_and_in_the_left_extension(reached):
    in_fragment = in_left_ext = last_added = 0
    for _, _, f, _, _, a in reached:
        for side in ("left", "right"):
            if a[side + "_end"] != NW.END_MEMBER: continue
            hit = a[side + "_hit"]
            assert 0 <= hit < a["out_len"]
            if hit < a["left_ext"]: in_left_ext += 1
            else: in_fragment += 1
            if side == "right" and a["left_ext"] and hit == 0: last_added += 1             # the k-mer the left walk added last
    assert in_fragment >= 3 and in_left_ext >= 3 and last_added >= 1


def test_the_issues_ring_table(reached):
    """k = 25, both strandednesses, ample room: (left_ext, left_end, left_hit, right_ext, right_end, right_hit)"""
    M, B, S = NW.END_MEMBER, NW.END_BACK_BRANCH, NW.END_SEVERAL
    table = {("none", 1.0): (550, M, 699, 0, M, 0), ("none", 2.0): (550, M, 699, 0, M, 0),
             ("far", 2.0): (200, B, -1, 350, M, 0), ("far", 1.0): (200, B, -1, 350, S, -1),
             ("first", 2.0): (0, B, -1, 550, M, 0), ("first", 1.0): (0, B, -1, 550, S, -1)}
    seen = 0
    for kind, case, _, mc, room, a in reached:
        if kind == "ring" and case[0] == NW.K_MAIN and room == NW.AMPLE:
            assert tuple(a[f] for f in ("left_ext", "left_end", "left_hit", "right_ext", "right_end", "right_hit")) == table[(case[2], mc)], (case, mc)
            seen += 1
        if kind == "ring" and case[0] == NW.K_MAIN and room == 64 and case[2] == "none":
            assert (a["status"], a["left_ext"], a["left_end"], a["right_end"]) == (NW.ROOM, 64, NW.END_ROOM, NW.END_NOT_RUN)
    assert seen == 12
    assert any(max(r[5]["left_ext"], r[5]["right_ext"]) >= 500 for r in reached)


def test_every_k_of_the_matrix_reaches_member_and_a_long_walk(reached):
    for k in NW.K_MATRIX:
        mine = [r[5] for r in reached if r[0] == "ring" and r[1][0] == k and r[4] == NW.AMPLE]
        assert any(NW.END_MEMBER in (a["left_end"], a["right_end"]) for a in mine), k
        assert max(a["left_ext"] + a["right_ext"] for a in mine) == 240, k
    assert any(r[1][:2] == (64, True) for r in reached if r[0] == "ring")          # stranded k = 64: k-mers may hash alike


def test_both_homes_of_the_table_one_kmer_and_repeated_kmers(reached):
    """the kernel keeps the table in LDS while the fragment's k-mers + 2 room are at most NAIVE_FRAG_LDS_ENTRIES, else in device scratch"""
    assert N.NAIVE_FRAG_LDS_ENTRIES == 1024
    need = lambda r: len(r[2]) - r[1][0] + 1 + 2 * r[4]
    assert any(need(r) <= N.NAIVE_FRAG_LDS_ENTRIES for r in reached) and any(need(r) > N.NAIVE_FRAG_LDS_ENTRIES for r in reached)
    long_walks = [r for r in reached if r[5]["left_ext"] + r[5]["right_ext"] >= 500]
    assert long_walks and all(need(r) > N.NAIVE_FRAG_LDS_ENTRIES for r in long_walks)
    assert any(r[5]["status"] == NW.ROOM and need(r) <= N.NAIVE_FRAG_LDS_ENTRIES for r in reached)
    assert sum(len(r[2]) == r[1][0] for r in reached if r[0] == "random") >= len(NW.RANDOM_CASES)      # a fragment of exactly one k-mer
    # the tandem repeat's fragment: 30 k-mers of period 12, so the candidate before k-mer 0 is k-mers 11 and 23 and the one behind k-mer 29 is
    # k-mers 6 and 18: the LOWEST index is reported
    lowest = 0
    for kind, case, f, mc, room, a in reached:
        if kind == "random" and not case[3] and f == NW.cpu_random(case)[0].repeat_read[:30 + case[0] - 1]:
            k = case[0]
            kmers = [f[p:p + k] for p in range(30)]
            assert len(set(kmers)) == 12
            if (a["left_end"], a["right_end"]) == (NW.END_MEMBER, NW.END_MEMBER) and a["left_ext"] == 0:
                assert (a["left_hit"], a["right_hit"]) == (11, 6)
                lowest += 1
    assert lowest >= 4


def test_a_hash_hit_must_fail_on_the_bases(reached):
    """k = 64 stranded: the fragment (AC)^32; its left candidate (CA)^32 hashes as the fragment's only k-mer does and is a different k-mer: it is
    added, and the next candidate is the fragment's k-mer, at index 1 of the returned text"""
    w = tw.hash_equal_world(True)
    f, r, _ = w.og.get_kmers(b"AC" * 32 + b"A")
    assert f[0] == f[1]
    a = [r for r in reached if r[0] == "hash_equal"][0][5]
    assert (a["left_ext"], a["left_end"], a["left_hit"]) == (1, NW.END_MEMBER, 1)


def test_chained_calls_equal_one_call():
    """why the device call may be resumed: the restatement itself, chained with room 64, 7 and 1, returns what one call with ample room returns"""
    for case in NW.RING_CASES[:3]:
        w = NW.cpu_ring(case)
        for mc in NW.MIN_COVS:
            one = NW.restate(w.og, w.k, w.fragment, mc)
            for room in (64, 7) if case[2] != "far" else (64, 1):
                text, left, right, last, calls = NW.restate_chain(w.og, w.k, w.fragment, mc, room)
                assert text == one["text"] and (left, right) == (one["left_ext"], one["right_ext"]) and calls > 1
                assert (last["right_end"], last["right_hit"]) == (one["right_end"], one["right_hit"])


# ---- the finishing rules, hand-worked: k = 4, d = 3; a text of n letters has n - 3 k-mers ----
def finish(F, left_nk=2, right_nk=2, *, lookahead=1, mnp=1, extend=False, trim=False, sup=None, trim_fn=None, extend_fn=None, counts=None, repeat=False):
    sup = sup if sup is not None else (lambda t: [True] * (len(t) - 3))
    return NW.finish_restated(F, left_nk, right_nk, k=4, d=3, lookahead=lookahead, min_num_kmer_pairs=mnp, extend=extend, trim=trim, support=sup,
                              trim_fn=trim_fn or (lambda t: t), extend_fn=extend_fn or (lambda t: t),
                              counts_fn=counts or (lambda t: [np.float32(3.0)] * (len(t) - 3)), is_repeat=lambda km: repeat)


T13 = b"ACGTTGCATAGCC"      # 13 letters, 10 k-mers


def padded(s):
    return lambda t: pattern(s) + [False] * (len(t) - 3 - len(s))


def test_rule_1_the_consistency_check():
    # nk = 2 <= d: no check at all, whatever the support says
    assert finish(b"ACGTA", sup=lambda t: [False] * 2) == (b"ACGTA", 5, np.float32(3.0), NW.KEPT, False)
    # one range [0, 7) (tests/test_paired_segment_rules.py): kept and cut while it reaches the right read's k-mers
    assert finish(T13, right_nk=3, sup=padded("1001000")) == (T13[:10], 10, np.float32(3.0), NW.KEPT, False)
    assert finish(T13, right_nk=2, sup=padded("1001000"))[3] == NW.SPURIOUS                       # 7 < 10 - 2
    # one range [3, 10): it must begin inside the left read's k-mers
    assert finish(T13, left_nk=4, sup=padded("0001111")) == (T13[3:], 10, np.float32(3.0), NW.KEPT, False)
    assert finish(T13, left_nk=3, sup=padded("0001111"))[3] == NW.SPURIOUS                        # 3 >= 3
    # two ranges, [0, 4) and [6, 10), and none
    assert finish(T13, sup=padded("1000001"))[3] == NW.INCONSISTENT
    assert finish(T13, sup=padded("0000000")) == (None, -1, None, NW.INCONSISTENT, False)
    # numPairsRequired is `lookahead` here, not minNumKmerPairs: isolated pairs make a range for 1 and none for 2
    assert finish(T13, left_nk=9, right_nk=9, lookahead=1, mnp=9, sup=padded("1010101"))[3] == NW.KEPT
    assert finish(T13, left_nk=9, right_nk=9, lookahead=2, mnp=1, sup=padded("1010101"))[3] == NW.INCONSISTENT


def test_rule_2_the_trim():
    assert finish(T13, trim=True, trim_fn=lambda t: t[2:9]) == (T13[2:9], 7, np.float32(3.0), NW.KEPT, False)
    assert finish(T13, trim=True, trim_fn=lambda t: b"") == (None, -1, None, NW.EMPTY, False)     # the reference would throw in kmers.get(0)
    assert finish(T13, trim=False, trim_fn=lambda t: b"")[3] == NW.KEPT


def test_rule_3_the_extension_and_its_odd_test():
    F = b"ACGTTGCA"                                                                             # 5 k-mers, preExtensionFragLen 8
    grow = lambda left, right: (lambda t: b"G" * left + t + b"C" * right)
    # two k-mers added: 7 != 8, one range: adopted whole
    assert finish(F, extend=True, extend_fn=grow(1, 1)) == (b"G" + F + b"C", 8, np.float32(3.0), NW.KEPT, True)
    # exactly k - 1 = 3 k-mers added: 8 k-mers against 8 letters — "not extended", the extension is dropped unseen
    assert finish(F, extend=True, extend_fn=grow(2, 1)) == (F, 8, np.float32(3.0), NW.KEPT, False)
    assert finish(F, extend=True, extend_fn=grow(0, 3)) == (F, 8, np.float32(3.0), NW.KEPT, False)
    # nothing added: 5 != 8, so the unextended list goes through the whole-list check too and is cut to its one range — [0, 4) where only the
    # first pair is found (the support rule 1 saw, asked first, is complete)
    asked = []
    twice = lambda t: (asked.append(t), [True] * 5 if len(asked) == 1 else pattern("10000"))[1]
    assert finish(F, extend=True, sup=twice) == (F[:7], 8, np.float32(3.0), NW.KEPT, True) and asked == [F, F]
    # no range or two: the fragment stays as it was before the extension (F itself passes rule 1: `extended` is the support of longer texts only)
    extended = lambda s: (lambda t: [True] * 5 if t == F else padded(s)(t))
    assert finish(F, extend=True, extend_fn=grow(4, 4), sup=extended("0" * 10)) == (F, 8, np.float32(3.0), NW.KEPT, False)
    assert finish(F, extend=True, extend_fn=grow(3, 4), sup=extended("100000001")) == (F, 8, np.float32(3.0), NW.KEPT, False)
    # the second check takes minNumKmerPairs
    assert finish(F, extend=True, mnp=2, extend_fn=grow(1, 1), sup=extended("1010"))[4] is False
    assert finish(F, extend=True, mnp=1, extend_fn=grow(1, 1), sup=extended("1010"))[4] is True


def test_rule_4_the_final_screen():
    T6 = T13[:6]                                                                                  # 3 k-mers <= d: rule 1 does not run
    three = np.float32(3.0)
    assert finish(T6, lookahead=2) == (T6, 6, three, NW.KEPT, False)                              # 6 >= 4 + 2
    assert finish(T6, lookahead=3) == (None, 6, None, NW.TOO_SHORT, False)
    assert finish(T6, repeat=True) == (None, 6, three, NW.NO_COMPLEX_KMER, False)
    got = finish(T13, counts=lambda t: [np.float32(c) for c in (5, 2.5, 9, 3, 3, 3, 3, 3, 3, 7)])
    assert got[2] == np.float32(2.5) and got[2].dtype == np.float32
    # a longer fragment meets `lookahead` twice: as rule 1's numPairsRequired and as rule 4's length
    assert finish(T13, lookahead=7)[3] == NW.KEPT and finish(T13, lookahead=8)[3] == NW.INCONSISTENT


@pytest.mark.parametrize("stranded", [False, True])
def test_the_finish_world_reaches_every_outcome_but_empty(stranded):
    w = NW.finish_world(stranded)
    seen, adopted, chained = set(), 0, 0
    for extend, trim in NW.FINISH_SWITCHES:
        for (f, _, _), a in zip(NW.finish_fragments(w), NW.finish_answers(w, extend, trim)):
            seen.add(a[3]); adopted += a[4]
            chained += a[0] is not None and len(a[0]) > len(f) + 512          # an extension that room 256 cannot hold in one call
    assert seen == {NW.KEPT, NW.INCONSISTENT, NW.SPURIOUS, NW.NO_COMPLEX_KMER, NW.TOO_SHORT} and adopted >= 20
    assert chained >= 1 or not stranded
