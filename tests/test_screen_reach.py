"""On the CPU oracle alone: the proof that the worlds of tests/screen_worlds.py ask something.  tests/test_gpu_screen_matrix.py compares
rb_graph_screen_fragments, rb_graph_represented and rb_graph_trim_rc_artifacts with their restatements on these worlds at k = 16 ... 256; a
world that lost its gaps, its tails or its hairpins when k grew would let a wrong kernel pass.  Each world asserts the reach check of its
class (assert_every_branch_is_reached, as the k = 25 worlds do), the screen worlds also the gaps that only k decides (gaps of 2 k and 2 k + 1
k-mers, a path that arrives after k steps, a splice at entry k - 1 and 2 k - 1 of the left walk) and every chim_why and blunt_why under both
settings of the device test.  A branch that cannot exist at some k is excused in screen_worlds.EXCUSED, with its reason.  Each test prints
the counts it rests on (-s shows them).

The world classes got keyword parameters and offsets in terms of k to make this possible; the worlds the other tests build must not have
changed by a byte, and the first test holds their reads, gate sequences, queries and expected records under the existing settings to
SHA-256 digests recorded before that edit."""
import pytest

import screen_worlds as SW
import test_represented_rules as RR
import test_screen_rules as S
import test_trim_artifact_rules as T

IDS = [SW.case_id(c) for c in SW.CASES]
S25 = [(3, 2), (5, 1), (3, SW.DEEP), (5, 0)]
T3 = ((T.HASHES, 0, 0.0), (T.EDGE, 60, 0.0), (T.LONG, 30, 0.5))

# ---- the worlds of the existing tests are what they were ----
OLD_WORLDS = {
    "screen-25-0": (lambda: SW.screen_digest(S.world(25, False), S25), "06d6a79ad21701bde9772b08edaf559465454ccecf0216dd6c31860588e73d27"),
    "screen-25-1": (lambda: SW.screen_digest(S.world(25, True), S25), "7c06af75e859dc0fc4d05bb3ad39db347660e14d7bbd0f9de7068957ab25712a"),
    "screen-143": (lambda: SW.screen_digest(S.world_143(), [(3, 2)]), "c4197d6aa27ef9b206525a3f832bacf733c79ede7f2d315e7dd652ba38d7ef58"),
    "screen-hashes": (lambda: SW.screen_digest(S.world_hashes(), [(3, 2), (5, SW.DEEP)]), "c945b8498d91fa81df8977e0e27ec0b58c7740dbd272adfcee9e109f4b6296e2"),
    "repr-25-0": (lambda: SW.repr_digest(RR.world(25, False), RR.SETTINGS), "1e04c15c2b34501bd3669748bf354df85fc367cb5c0a284678efac1dae20aeab"),
    "repr-25-1": (lambda: SW.repr_digest(RR.world(25, True), RR.SETTINGS), "a601e964870087d93a9bd201092f762a68f5fe602adbfff11bb26a36bf28a4db"),
    "repr-143": (lambda: SW.repr_digest(RR.world_143(), [(3, 1, 10, 0.9)]), "25b56a90533f459da50adbaec0a971fc86eee811255f53f5426fd976fd88f225"),
    "repr-hashes": (lambda: SW.repr_digest(RR.world_hashes(), [(3, 1, 40, 0.9)]), "b9ca0638a654495742a69734d49a197975a63c1ba29a6fdf7796aa4038e10280"),
    "trim-25-0": (lambda: SW.trim_digest(T.world(25, False), T.K25_SETTINGS), "719416f46e21d643313c370edd3b7c0209244acb9ba0aae9bf4120cbcf8ec543"),
    "trim-25-1": (lambda: SW.trim_digest(T.world(25, True), T.K25_SETTINGS), "7741524f9a850a18571cfc91f69053786a5d85726ebfdc1319baeef272975537"),
    "trim-143-0": (lambda: SW.trim_digest(T.world(143, False), T.world(143, False).settings), "f4224edf649a70191337d7bbb493b2a33e043af1eb252774104af4b353dba569"),
    "trim-143-1": (lambda: SW.trim_digest(T.world(143, True), T.world(143, True).settings), "65e33cc58d8186f610970188673a1d8d85727fba190a638c54b5e6290dbfc839"),
    "trim-hashes": (lambda: SW.trim_digest(T.world(25, False, (1, 3, 3)), T3), "5b2ed125f169f59d6b1d7bb1f67f85a3bcf402def47566b18e81f63acff9a0f1"),
}


@pytest.mark.parametrize("name", sorted(OLD_WORLDS))
def test_existing_worlds_are_unchanged_byte_for_byte(name):
    make, want = OLD_WORLDS[name]
    assert make() == want


# ---- the matrix ----
def test_matrix_spreads_the_axes():
    assert SW.KS == (16, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256)
    assert len({(c.k, c.stranded) for c in SW.CASES}) == len(SW.CASES) == 28
    for k in SW.KS:
        assert {c.stranded for c in SW.CASES if c.k == k} == {False, True}
    for pick, values in ((lambda c: c.hashes, SW.TRIPLES), (lambda c: c.gate_h, SW.GATES)):
        for v in set(values):
            mine = [c for c in SW.CASES if pick(c) == v]
            assert {c.stranded for c in mine} == {False, True} and any(c.k < 64 for c in mine) and any(c.k > 64 for c in mine), v
    assert {c.clip for c in SW.CASES if c.stranded} == {c.clip for c in SW.CASES if not c.stranded} == {10, 40}
    assert sorted((c.k, c.stranded) for c in SW.CASES if c.identity == 1.0) == sorted(SW.IDENTITY_ONE) and {s for _, s in SW.IDENTITY_ONE} == {False, True}
    for case in SW.CASES:                                         # no filter larger than the largest of the k = 25 and k = 143 worlds: 4 800 011 counters
        sizes, gate = SW.sizes_of(case)
        assert max(sizes[0] // 8, sizes[1], sizes[2] // 8, gate // 8) <= 4_800_011
        low, mid, high = (st[1] for st in SW.trim_settings(case.k) if st[0] == T.LONG)
        assert low < case.k < mid < 11 * case.k + 51 < high and len(SW.trim_settings(case.k)) == 7 and SW.trim_settings(case.k)[1][:2] == (T.EDGE, 1)


def test_the_excuse_and_reseed_tables_are_small_and_say_why():
    for (call, k), entries in SW.EXCUSED.items():
        assert (call == "repr" and k >= 127 or call == "trim" and k % 2 == 0) and k in SW.KS, (call, k)
        for branch, why in entries.items():
            assert not branch.startswith(("why_", "chim_why", "blunt_why")) and why         # no `why` value of any record
            assert branch not in ("left_walk_arrives_after_64_steps", "spliced_at_entry_64_or_beyond")
    assert all(call in SW.CALLS and k in SW.KS and 0 < n < 10 for (call, k, _), n in SW.RESEED.items())


@pytest.mark.parametrize("case", SW.CASES, ids=IDS)
def test_screen_and_represented_world(case):
    SW.check_case(case, "screen")
    w = SW.screen_case(case)
    for setting in SW.SCREEN_SETTINGS:
        got = w.want(*setting)
        print("screens %s %s: %d queries, (chim_why, blunt_why) %s, most visits %d" % (
            SW.case_id(case), setting, len(got), SW.outcome_counts((st.record[1], st.record[6]) for st in got), w.largest_visit_count(*setting)))
    got = w.judged(3, 1, case.clip, case.identity)
    print("represented %s clip %d identity %.1f: (why, path_form) %s, excused %s" % (
        SW.case_id(case), case.clip, case.identity, SW.outcome_counts((st.record[1], st.record[10]) for st in got), sorted(SW.EXCUSED.get(("repr", case.k), {}))))
    assert {st.record[1] for st in got} >= {0, 1, 2, 4, 5, 6, 8} and {st.record[10] for st in got} == {0, 1, 2, 3}       # under the device test's own setting
    assert {3, 9} <= {st.record[1] for st in got}                                                                       # (edge-a-quarter-off)


@pytest.mark.parametrize("case", SW.CASES, ids=IDS)
def test_trim_world(case):
    SW.check_case(case, "trim")
    w = SW.trim_case(case)
    assert w.settings == SW.trim_settings(case.k) and {"tile-%d" % n for n in (1, 64, 65, T.LDS_LIST, T.LDS_LIST + 1)} <= set(w.names)
    for setting in w.settings:
        recs = [rec for rec, _ in w.judged(*setting)]
        print("trim %s %s: %d queries, (flags, pass 0 why, pass 1 why) %s" % (SW.case_id(case), setting, len(recs), SW.outcome_counts((r[0], r[4], r[9]) for r in recs)))
        assert any(not r[0] & T.FOUND for r in recs) and (setting[1] < case.k or any(r[0] & T.FOUND for r in recs))
