"""GraphUtils.represented(kmers, graph, bf, lookahead, maxIndelSize, maxEdgeClipLength, percentIdentity) (R/util/GraphUtils.java:711-824) — the
transcript assembler's screen between isBranchFree and isChimera — restated line by line in Python over the CPU oracle.  What it calls is
restated elsewhere and reused: the gated walks, getMaxCoveragePath and the static hasDepth* (tests/test_screen_rules.py), SeqUtils.getDistance
and getPercentIdentity (tests/test_error_correction_rules.py).  The restatement returns the 12 ints of rb_repr_rec, the call count of every
hasDepth* search and the names of the branches it took.
The world of tests/test_gpu_represented.py is tests/test_screen_rules.ScreenWorld with more queries and a few more k-mers in its gate; every
`why` and every branch the device test relies on is shown here to be reached by a named query.  No device is needed."""
import pytest

import test_screen_rules as S
from test_error_correction_rules import distance, distance_literal, percent_identity
from test_extend_step_rules import F32, ACGT
from test_screen_rules import OverBudget, Side, has_depth, max_coverage_path

REPRESENTED, BAD_LETTER, NO_KMER, OVER_BUDGET = 1, 8, 16, 32
WHY_TRUE, WHY_NO_RUN, WHY_LEFT_LENGTH, WHY_LEFT_IDENTITY, WHY_WIDE_GAP, WHY_NO_PATH, WHY_PATH_LENGTH, WHY_PATH_IDENTITY, WHY_RIGHT_LENGTH, \
    WHY_RIGHT_IDENTITY = range(10)
PATH_NONE, PATH_LEFT, PATH_RIGHT, PATH_SPLICED = range(4)
FIELDS = ("flags", "why", "left", "right", "expected_len", "found_len", "distance", "tests_passed", "distance_sum", "tips_skipped", "path_form",
          "reserved")
DEFAULT_VISITS = S.DEFAULT_VISITS


def blank(flags):
    return [flags, -1, -1, -1, -1, -1, -1, 0, 0, 0, 0, 0]


def assemble(kmers):
    """graph.assemble(ArrayDeque<Kmer>) (R/graph/BloomFilterDeBruijnGraph.java:1236-1252): "" for no k-mer"""
    return kmers[0] + b"".join(km[-1:] for km in kmers[1:]) if kmers else b""


def represented(s, seq, lookahead, max_indel, clip, pid, d, budget=None, visits=None, tags=None):
    """:711-824 -> the record.  seq: upper-case ACGT.  Raises OverBudget out of a hasDepth* search."""
    k = s.k
    kmers = [seq[p:p + k] for p in range(len(seq) - k + 1)]
    n = len(kmers)
    max_index = n - 1
    max_bubble = d + k
    pid = F32(pid)
    visits = [] if visits is None else visits
    tags = set() if tags is None else tags
    acc = [0, 0, 0, PATH_NONE]                                   # tests passed, the sum of their distances, tips skipped, the last path's form

    def out(why, left=-1, right=-1, expected=-1, found=-1, dist=-1):
        tags.add("why_%d" % why)
        return [REPRESENTED if why == WHY_TRUE else 0, why, left, right, expected, found, dist] + acc + [0]

    def depth(source, direction, dep):
        ans, calls = has_depth(s, source, direction, dep, False, budget)
        visits.append(calls)
        return ans

    def identity_below(text, own):
        """getPercentIdentity(graph.assemble(path), graph.assemble(kmers, ...)) < percentIdentity, and the distance"""
        return bool(percent_identity(text, own) < pid), distance(text, own)

    last = -1
    i = 0
    while i < n:
        if s.gate(kmers[i]):
            start = end = i
            for j in range(i + 1, n):
                if s.gate(kmers[j]):
                    end = j
                else:
                    break
            if end - start + 1 >= lookahead:
                if start > 0:
                    if last < 0:
                        if start >= clip or depth(kmers[0], 1, clip - start):
                            if start < clip: tags.add("left_edge_tested_after_depth")
                            walk = s.greedy_walk(kmers[start], 1, lookahead, start)        # walking order: right to left
                            if len(walk) != start:
                                return out(WHY_LEFT_LENGTH, 0, start, start, len(walk))
                            below, dist = identity_below(assemble(walk[::-1]), seq[0:start + k - 1])
                            if below:
                                return out(WHY_LEFT_IDENTITY, 0, start, start, len(walk), dist)
                            acc[0] += 1; acc[1] += dist
                            tags.add("left_edge_passed")
                        else:
                            acc[2] += 1
                            tags.add("left_tip_skipped")
                    else:
                        expected = start - last - 1
                        if expected > max_bubble:
                            return out(WHY_WIDE_GAP)
                        missing = k - expected
                        left, right = last, start
                        if missing > 0:
                            tags.add("gap_widened")
                            for j in range(missing):
                                if left == 0:
                                    tags.add("widening_stops_at_index_0")
                                    break
                                left -= 1                                                   # --left comes before the lookup
                                if not s.gate(kmers[left]):
                                    tags.add("widening_stops_on_an_unassembled_kmer_left")
                                    break
                            else:
                                tags.add("widening_runs_its_length_left")
                            for j in range(missing):
                                if right == max_index:
                                    tags.add("widening_stops_at_max_index")
                                    break
                                right += 1
                                if not s.gate(kmers[right]):
                                    tags.add("widening_stops_on_an_unassembled_kmer_right")
                                    break
                            else:
                                tags.add("widening_runs_its_length_right")
                            expected = right - left - 1
                        ptags = set()
                        path = max_coverage_path(s, kmers[left], kmers[right], expected + max_indel, lookahead, ptags)
                        tags |= ptags
                        acc[3] = PATH_NONE if path is None else PATH_LEFT if "path_from_the_left" in ptags else PATH_RIGHT if "path_from_the_right" in ptags else PATH_SPLICED
                        if path is None:
                            return out(WHY_NO_PATH, left, right, expected)
                        if not path: tags.add("empty_path")
                        if len(path) < expected - max_indel or len(path) > expected + max_indel:
                            return out(WHY_PATH_LENGTH, left, right, expected, len(path))
                        below, dist = identity_below(assemble(path), seq[left + 1:right + k - 1])
                        if below:
                            return out(WHY_PATH_IDENTITY, left, right, expected, len(path), dist)
                        acc[0] += 1; acc[1] += dist
                        tags.add("gap_passed")
                last = end
            else:
                tags.add("short_run")
            i = end
        i += 1
    if last >= 0:
        if last < max_index:
            expected = n - last - 1
            if expected >= clip or depth(kmers[max_index], 0, clip - expected):
                if expected < clip: tags.add("right_edge_tested_after_depth")
                walk = s.greedy_walk(kmers[last], 0, lookahead, expected)
                if len(walk) != expected:
                    return out(WHY_RIGHT_LENGTH, last, max_index, expected, len(walk))
                below, dist = identity_below(assemble(walk), seq[last + 1:])
                if below:
                    return out(WHY_RIGHT_IDENTITY, last, max_index, expected, len(walk), dist)
                acc[0] += 1; acc[1] += dist
                tags.add("right_edge_passed")
            else:
                acc[2] += 1
                tags.add("right_tip_skipped")
    else:
        return out(WHY_NO_RUN)
    return out(WHY_TRUE)


def judge(s, seq, lookahead, max_indel, clip, pid, d, max_visits=0):
    """what rb_graph_represented reports for one sequence"""
    if len(seq) < s.k:
        return S.Screened(blank(NO_KMER))
    if not S.is_acgtu(seq):
        return S.Screened(blank(BAD_LETTER))
    seq = seq.upper().replace(b"U", b"T")
    visits, tags = [], set()
    try:
        rec = represented(s, seq, lookahead, max_indel, clip, pid, d, max_visits or DEFAULT_VISITS, visits, tags)
    except OverBudget:
        rec = blank(OVER_BUDGET)                                 # not judged: nothing is guessed
        tags.add("over_budget")
    return S.Screened(rec, visits, tags)


# ---- hand-worked toy cases: an unbranched graph, every k-mer with count 1, a chosen set of them in the gate ----
class Toy(S.ToySide):
    def gate(self, kmer):
        return kmer in self.gated

    def greedy_once(self, kmer, direction, lookahead):
        nb = self.neighbours(kmer, direction, True)
        assert len(nb) <= 1                                      # the toys have no fork
        return nb[0] if nb else None

    def greedy_walk(self, kmer, direction, lookahead, bound):
        out = []
        for _ in range(bound):
            kmer = self.greedy_once(kmer, direction, lookahead)
            if kmer is None:
                break
            out.append(kmer)
        return out


def toy(text, k, gated_idx, extra=()):
    kmers = [text[p:p + k] for p in range(len(text) - k + 1)]
    return Toy(k, set(kmers) | set(extra), {kmers[i] for i in gated_idx} | set(extra)), kmers


TOY = b"ACGGTCATTGCAAGCTTAGGCATCGA"                              # 26 letters, 22 different 5-mers


def test_the_toy_text_has_no_repeated_kmer():
    assert len({TOY[p:p + 5] for p in range(22)}) == 22 and len({TOY[p:p + 4] for p in range(23)}) == 23     # no k-mer twice, no fork


def test_widening_moves_the_index_before_it_looks():
    # k = 5: k-mers 0..7 in the gate, 8 and 9 not, 10 and 11 in, 12 not, 13.. in.  The second run (10..11) has a gap of 2 behind it: numMissing = 3.
    # --left looks at 6, 5, 4: all in the gate, left = 4.  ++right looks at 11 (in), 12 (not): the loop breaks with right ON 12 (:776).
    t, km = toy(TOY, 5, [0, 1, 2, 3, 4, 5, 6, 7, 10, 11] + list(range(13, 22)))
    tags = set()
    rec = represented(t, TOY, 1, 0, 0, 0.0, 30, tags=tags)
    assert "widening_stops_on_an_unassembled_kmer_right" in tags and "widening_runs_its_length_left" in tags
    # the gated walk from k-mer 4 never takes k-mer 8 (outside the gate): no path, with the widened indices on record
    assert rec == [0, WHY_NO_PATH, 4, 12, 7, -1, -1, 0, 0, 0, PATH_NONE, 0]
    # every gap k-mer in the gate's graph: widening then ends on a k-mer in the gate after numMissing steps, and at the ends of the list
    t, km = toy(TOY, 5, [0, 1, 4, 5] + list(range(6, 22)))
    tags = set()
    rec = represented(t, TOY, 1, 0, 0, 0.0, 30, tags=tags)
    assert "widening_stops_at_index_0" in tags and "widening_runs_its_length_right" in tags
    assert rec[:6] == [0, WHY_NO_PATH, 0, 7, 6, -1]


def test_a_run_shorter_than_lookahead_is_ignored_but_skipped_over():
    # k-mers 0..5 in the gate, 6..8 not, 9 and 10 in (a run of 2 < lookahead 3), 11.. not: the run 9..10 neither tests its gap nor moves
    # lastRepresentedKmerFoundIndex, and the scan goes on behind it (i = endIndex): the right edge is 16 k-mers from k-mer 5 on, not 11
    t, km = toy(TOY, 5, [0, 1, 2, 3, 4, 5, 9, 10])
    tags = set()
    rec = represented(t, TOY, 3, 0, 0, 0.0, 30, tags=tags)
    assert "short_run" in tags and "gap_widened" not in tags
    assert rec == [0, WHY_RIGHT_LENGTH, 5, 21, 16, 0, -1, 0, 0, 0, PATH_NONE, 0]       # the gated walk from k-mer 5 finds k-mer 6 outside the gate
    # with lookahead 2 the run counts: its gap of 3 is tested (widened, no path through k-mers outside the gate)
    rec = represented(t, TOY, 2, 0, 0, 0.0, 30)
    assert rec[:5] == [0, WHY_NO_PATH, 3, 11, 7]                  # ++right stops ON k-mer 11


def test_an_empty_path_assembles_to_nothing():
    # TOY[:12] + "C" + TOY[8:] repeats four letters behind an inserted one: the 5 k-mers that hold the C are nowhere, so the gap is 5 k-mers
    # wide (no widening at k = 5), left = k-mer 7 of the query = TOY[7:12], right = k-mer 13 = TOY[8:13]: in the graph right is left's successor,
    # so getMaxCoveragePath returns the EMPTY leftPath (:1710-1711), not null.  Length 0 is outside 5 +- 1 ...
    q = TOY[:12] + b"C" + TOY[8:]
    graph = [TOY[p:p + 5] for p in range(22)]
    t = Toy(5, set(graph), set(graph))
    tags = set()
    rec = represented(t, q, 1, 1, 0, 0.0, 30, tags=tags)
    assert "empty_path" in tags and rec == [0, WHY_PATH_LENGTH, 7, 13, 5, 0, -1, 0, 0, 0, PATH_LEFT, 0]
    # ... and inside 5 +- 5: "" against the gap's 9 letters is distance 9 (:196), identity (9 - 9) / 9 = 0: below 0.5, not below 0.0
    rec = represented(t, q, 1, 5, 0, 0.5, 30)
    assert rec == [0, WHY_PATH_IDENTITY, 7, 13, 5, 0, 9, 0, 0, 0, PATH_LEFT, 0]
    rec = represented(t, q, 1, 5, 0, 0.0, 30)
    assert rec == [REPRESENTED, WHY_TRUE, -1, -1, -1, -1, -1, 1, 9, 0, PATH_LEFT, 0]


def test_distance_is_neither_symmetric_nor_reversal_invariant():
    """v0[tLen] is never refreshed (System.arraycopy copies tLen entries), so the last column is not Levenshtein's: the operands' order and
    orientation matter, and the device must be given s = the assembled path left to right, t = the sequence's letters"""
    s, t = b"ACGTTT", b"ACG"
    assert distance_literal(s, t) == distance(s, t) == 4          # Levenshtein says 3: the stale v0[3] = 3 gives v1[3] = min(v1[2] + 1, 3 + 1, ...) = 4
    assert distance_literal(t, s) == distance(t, s) == 3          # swapped
    assert distance_literal(s[::-1], t[::-1]) == distance(s[::-1], t[::-1]) == 3      # both read right to left
    s, t = b"AAAAC", b"C"
    assert (distance(s, t), distance(t, s)) == (distance_literal(s, t), distance_literal(t, s)) == (2, 4)      # ... and below Levenshtein's 4


# ---- the world of the device test ----
SETTINGS = [(3, 1, 10, 0.9), (3, 1, 40, 0.9), (3, 1, 10, 1.0), (5, 2, 1, 0.9), (0, 0, 0, 0.0)]     # lookahead, max_indel, clip, identity
TILING = (63, 64, 65, 128, 129)                                  # letters of an edge's assembled text around the wavefront's 64 columns
LONG_EDGE = 1021                                                 # k-mers of the edge that leaves LDS (1024 columns) and passes 1000 k-mers


def snvs_every(seq, last, step):
    """a letter changed at `last`, last - step, ...: with step < k every k-mer up to index `last` carries one, k-mer last + 1 none"""
    for p in range(last, -1, -step):
        seq = S.put(seq, p, chr(S.other(seq[p])[0]))
    return seq


class ReprWorld(S.ScreenWorld):
    """ScreenWorld's graph, gate and queries; more queries (each mirrored) and, in the gate alone, eight k-mers of one of them"""

    def __init__(self, k, stranded, seed, seg=150, **kw):
        super().__init__(k, stranded, seed, seg=seg, **kw)
        from oracle import rbo
        a1, b1, c1, c2, big = (self.tx[i][0] for i in (0, 2, 4, 5, 6))
        q = []
        # an SNV 15 k-mers from the end of an assembled stretch: an edge of 15 k-mers with one mismatch
        base = a1[40:2 * seg + 60]
        q.append(("snv-near-end", S.put(base, len(base) - 15, chr(S.other(base[len(base) - 15])[0]))))
        # three letters inserted (a gap of k + 2 k-mers over a path of k - 1), one letter left out (a gap of k - 1: widened by one on each side)
        ins = S.other(base[seg])                                 # neither neighbour's letter: k + 2 k-mers hold an inserted one
        if ins[0] == base[seg - 1]: ins = S.other(ins[0])
        q.append(("insertion-3", base[:seg] + bytes(ins * 3) + base[seg:]))
        q.append(("deletion-1", base[:seg] + base[seg + 1:]))
        # gene C forks 3 : 1 behind its first exon.  The light isoform with its first own letter changed to one neither isoform has: the walk from
        # the left takes the heavy branch, the walk from the right comes back to `left` alone.  Changed 5 letters before the fork: the walk from
        # the right meets the left walk on the shared exon.
        fork = seg
        while c1[fork] == c2[fork]: fork += 1                   # (where the two second exons begin alike)
        third = [ch for ch in ACGT if ch not in (c1[fork], c2[fork])][0]
        fl = k + 45
        q.append(("fork-snv-on-the-light-branch", S.put(c2[fork - fl:fork + fl], fl, chr(third))))
        q.append(("fork-snv-before-it", S.put(c2[fork - fl:fork + fl], fl - 5, chr(S.other(c2[fork - 5])[0]))))
        # a run of 8 k-mers that the gate holds (and the graph does not) inside an SNV's gap: two short gaps whose widening meets k-mers outside
        # the gate; the same 5 k-mers from the start of the query
        p, w = max(600, 4 * k + 20), 4 * k
        if (LONG_EDGE - 1 - p) % (k - 1) == 0: p += 1          # (edge-long changes that letter too, and would meet the run that the gate alone holds)
        wide = S.put(big[p - w:p + w], w, chr(S.other(big[p])[0]))
        # the run's k-mers io .. io + il - 1 before the changed letter's last k-mer all carry that letter, and so do k-mers in front of them
        # and behind: 16 and 8 from k = 25 on, two thirds and one third of k below
        io, il = self.island = (16, 8) if k >= 25 else (2 * k // 3, k // 3)
        island = wide[w - io:w - io + k + il - 1]                # k-mers w - 16 .. w - 9 of `wide`: all carry the changed letter
        q.append(("widening-meets-unassembled", wide))
        q.append(("widening-meets-the-end", wide[w - k + 1 - 5:]))
        # ... the query starts 3 k-mers before the run (an excused tip at a clip of 10 or more), or ends on the run's 4th k-mer
        q.append(("widening-meets-unassembled-behind", wide[w - io - 3:]))
        q.append(("widening-meets-the-last-kmer", wide[:w - io + 3 + k]))
        # an edge that is in the graph but not in the gate, shorter than the clip of 40: hasDepth* answers true and the edge is tested
        a2 = self.tx[1][0]
        q.append(("edge-in-the-graph", a2[seg - k - 35:seg + 15]))
        # edges whose assembled text is 63 .. 129 letters, and one of 1021 k-mers: a changed letter every k - 1 letters
        for letters in TILING:
            nk = letters - k + 1
            if nk > 0:
                q.append(("edge-%d-letters" % letters, snvs_every(big[300:300 + nk + k + 35], nk - 1, k - 1)))
        q.append(("edge-long", snvs_every(big[:LONG_EDGE + k + 55], LONG_EDGE - 1, k - 1)))
        more = [(name, s_) for name, s_ in q] + [(name + "~", s_[::-1]) for name, s_ in q]
        more.append(("edge-in-the-graph-deepest", a2[seg - k - 35:seg + 12]))      # not mirrored: the one query with the longest depth search
        self.queries = self.queries + more
        self.names = [name for name, _ in self.queries]
        mode = rbo.FWD if stranded else rbo.CANON
        extra = [island, island[::-1]]
        for t in extra:
            hv, _ = rbo.hash_region(t, k, self.gate_og.h, mode)
            for row in hv:
                self.gate_og.add_dbg_only(row)
        self.gate_seqs = self.gate_seqs + extra
        self.s = Side(self.og, self.gate_og)                    # nothing memoised from before the gate grew
        self._repr = {}

    def judged(self, lookahead, max_indel, clip, pid, max_visits=0):
        """the restatement's records for every query, computed once per setting"""
        key = (lookahead, max_indel, clip, float(pid), max_visits)
        if key not in self._repr:
            self._repr[key] = [judge(self.s, s_, lookahead, max_indel, clip, pid, self.d, max_visits) for _, s_ in self.queries]
        return self._repr[key]

    def most_visits(self, lookahead, max_indel, clip, pid):
        return max((max(st.visits) for st in self.judged(lookahead, max_indel, clip, pid) if st.visits), default=0)

    def named(self, *setting):
        return dict(zip(self.names, self.judged(*setting)))


WORLDS = {}


def world(k, stranded):
    if (k, stranded) not in WORLDS:
        WORLDS[(k, stranded)] = ReprWorld(k, stranded, seed=900 + stranded)
    return WORLDS[(k, stranded)]


def world_143():
    if 143 not in WORLDS:
        WORLDS[143] = ReprWorld(143, False, seed=943, read_len=400, tile=40, seg=500, long_len=1400)
    return WORLDS[143]


def world_hashes():
    if "h" not in WORLDS:
        WORLDS["h"] = ReprWorld(25, False, seed=977, hashes=(1, 3, 2), gate_h=3)
    return WORLDS["h"]


def assert_every_branch_is_reached(w, excused=()):
    """every `why`, every path form and every branch of the widening, the edges and the scan, each by a query named for it; (3, 1, 10, 0.9) unless said.
    excused: "short_edges_fail_identity" where k is so large that an edge of 15 or 20 k-mers cannot differ in a tenth of its letters"""
    base, clip40, exact = w.named(3, 1, 10, 0.9), w.named(3, 1, 40, 0.9), w.named(3, 1, 10, 1.0)
    rec = lambda got, name: got[name].record
    short_edges_fail = "short_edges_fail_identity" not in excused
    # what the screens' own queries reach: every why but 3, 6 and 7 unmirrored, 3 in a mirror
    for name, why in (("assembled", WHY_TRUE), ("assembled-long", WHY_TRUE), ("ends-not-assembled", WHY_NO_RUN), ("first-not-assembled", WHY_LEFT_LENGTH),
                      ("wide-gap", WHY_WIDE_GAP), ("skipped-exon", WHY_NO_PATH), ("chimera", WHY_NO_PATH), ("blunt-assembled-path-short", WHY_RIGHT_LENGTH),
                      ("blunt-artifact", WHY_RIGHT_IDENTITY), ("blunt-artifact~", WHY_LEFT_IDENTITY), ("first-not-assembled~", WHY_RIGHT_LENGTH),
                      ("blunt-assembled-path-short~", WHY_LEFT_LENGTH)):
        if name.startswith("blunt-artifact") and not short_edges_fail:
            assert rec(base, name)[1] in (why, WHY_TRUE) and rec(base, name)[7] == (rec(base, name)[1] == WHY_TRUE), (name, rec(base, name))
            continue
        assert rec(base, name)[1] == why and bool(rec(base, name)[0] & REPRESENTED) == (why == WHY_TRUE), (name, rec(base, name))
    assert rec(base, "wide-gap")[2:7] == (-1,) * 5 and rec(base, "ends-not-assembled")[2:7] == (-1,) * 5 and rec(base, "assembled")[2:7] == (-1,) * 5
    for name in ("one-kmer-assembled", "two-kmers-assembled"):    # a run below the lookahead of 3 does not count
        assert "short_run" in base[name].tags and rec(base, name)[1] == WHY_NO_RUN
    assert "short_run" not in base["three-kmers-assembled"].tags and rec(base, "three-kmers-assembled")[0] == REPRESENTED
    assert "path_from_the_left" in base["snv-bridged"].tags and rec(base, "snv-bridged")[7:11] == (1, 1, 0, PATH_LEFT)
    for name, tag in (("blunt-artifact", "right_tip_skipped"), ("blunt-artifact~", "left_tip_skipped")):      # a tail of 20 k-mers below the clip of 40
        assert tag in clip40[name].tags and rec(clip40, name) == (REPRESENTED, WHY_TRUE, -1, -1, -1, -1, -1, 0, 0, 1, PATH_NONE, 0)
    # an edge with one mismatch passes at 0.9 and fails at 1.0
    assert rec(base, "snv-near-end") == (REPRESENTED, WHY_TRUE, -1, -1, -1, -1, -1, 1, 1, 0, PATH_NONE, 0) and "right_edge_passed" in base["snv-near-end"].tags
    assert "left_edge_passed" in base["snv-near-end~"].tags
    assert rec(exact, "snv-near-end")[1:] == (WHY_RIGHT_IDENTITY, rec(exact, "snv-near-end")[2], rec(exact, "snv-near-end")[2] + 15, 15, 15, 1, 0, 0, 0, PATH_NONE, 0)
    assert rec(exact, "snv-near-end~")[:7] == (0, WHY_LEFT_IDENTITY, 0, 15, 15, 15, 1)
    # gaps: an insertion's path is too short; a deletion's gap is widened and bridged by a spliced path; the fork's light branch is reached from the right
    for nm in ("insertion-3", "insertion-3~"):
        assert rec(base, nm)[1] == WHY_PATH_LENGTH and rec(base, nm)[4:7] == (w.k + 2, w.k - 1, -1) and rec(base, nm)[10] == PATH_LEFT, rec(base, nm)
    for nm in ("deletion-1", "deletion-1~"):
        assert {"gap_widened", "paths_spliced", "gap_passed"} <= base[nm].tags and rec(base, nm)[7:11] == (1, 1, 0, PATH_SPLICED), rec(base, nm)
        assert rec(exact, nm)[1] == WHY_PATH_IDENTITY and rec(exact, nm)[6] == 1 and rec(exact, nm)[10] == PATH_SPLICED
        assert rec(exact, nm)[3] - rec(exact, nm)[2] - 1 == rec(exact, nm)[4] >= w.k + 1      # g <= k - 1 missing k-mers widen to 2 k - g
    assert rec(base, "fork-snv-on-the-light-branch")[7:11] == (1, 1, 0, PATH_RIGHT) and "path_from_the_right" in base["fork-snv-on-the-light-branch"].tags
    assert rec(base, "fork-snv-before-it")[7:11] == (1, 1, 0, PATH_SPLICED) and "gap_widened" not in base["fork-snv-before-it"].tags
    assert rec(exact, "fork-snv-on-the-light-branch")[1] == WHY_PATH_IDENTITY and rec(exact, "fork-snv-on-the-light-branch")[10] == PATH_RIGHT
    # the widening's four ways to stop, besides running its length (the deletion)
    for name, tag, got in (("widening-meets-unassembled", "widening_stops_on_an_unassembled_kmer_right", base),
                           ("widening-meets-unassembled-behind", "widening_stops_on_an_unassembled_kmer_left", base),
                           ("widening-meets-unassembled-behind", "widening_stops_on_an_unassembled_kmer_left", clip40),
                           ("widening-meets-the-end", "widening_stops_at_index_0", base), ("widening-meets-the-last-kmer", "widening_stops_at_max_index", base)):
        assert tag in got[name].tags and rec(got, name)[1] == WHY_NO_PATH, (name, got[name].tags, rec(got, name))
    r = rec(base, "widening-meets-unassembled")                   # `right` stands ON the first k-mer behind the run of 8
    assert r[3] == 4 * w.k - w.island[0] + w.island[1] and not w.s.gate(w.queries[w.names.index("widening-meets-unassembled")][1][r[3]:r[3] + w.k])
    r = rec(base, "widening-meets-unassembled-behind")            # `left` ON the last of the 3 k-mers before it; the tip before that was excused
    assert r[2] == 2 and r[9] == 1 and "left_tip_skipped" in base["widening-meets-unassembled-behind"].tags
    assert rec(base, "widening-meets-the-end")[2] == 0
    r = rec(base, "widening-meets-the-last-kmer")
    assert r[3] == len(w.queries[w.names.index("widening-meets-the-last-kmer")][1]) - w.k
    # an edge shorter than the clip whose k-mers go on in the graph: hasDepth* answers true and the edge is tested
    passes = () if short_edges_fail else (WHY_TRUE,)
    assert "right_edge_tested_after_depth" in clip40["edge-in-the-graph"].tags and rec(clip40, "edge-in-the-graph")[1] in (WHY_RIGHT_IDENTITY,) + passes
    assert "left_edge_tested_after_depth" in clip40["edge-in-the-graph~"].tags and rec(clip40, "edge-in-the-graph~")[1] in (WHY_LEFT_IDENTITY,) + passes
    assert clip40["edge-in-the-graph"].visits in ([40 - 15], [40 - 14]) and not base["edge-in-the-graph"].visits      # (14 where the exons e2 and e3 begin alike)
    # the tiling edges and the long one pass at 0.9 with a distance of one per changed letter
    for letters in TILING:
        nk = letters - w.k + 1                                    # (an edge's text has k letters at the least: no such edge from k = letters + 1 on)
        for nm, tag in (("edge-%d-letters" % letters, "left_edge_passed"), ("edge-%d-letters~" % letters, "right_edge_passed")) if nk >= 10 else ():         # (shorter than the clip of 10: a tip)
            assert tag in base[nm].tags and rec(base, nm)[7:9] == (1, (nk - 1) // (w.k - 1) + 1), (nm, rec(base, nm))
            assert rec(exact, nm)[4:6] == (nk, nk), (nm, rec(exact, nm))
    for nm in ("edge-long", "edge-long~"):
        assert rec(base, nm)[0] == REPRESENTED and rec(base, nm)[7:9] == (1, (LONG_EDGE - 1) // (w.k - 1) + 1)
        assert rec(exact, nm)[4:7] == (LONG_EDGE, LONG_EDGE, (LONG_EDGE - 1) // (w.k - 1) + 1) and LONG_EDGE > 1000 and LONG_EDGE + w.k - 1 > 1024
    # all in all: every why, every form, and the not-judged records
    everything = [st for setting in SETTINGS for st in w.judged(*setting)]
    assert {st.record[1] for st in everything} == set(range(10)) | {-1}
    assert {st.record[10] for st in everything} == {PATH_NONE, PATH_LEFT, PATH_RIGHT, PATH_SPLICED}
    for name in ("too-short", "empty", "too-short~"):
        assert rec(base, name) == tuple(blank(NO_KMER))
    for name in ("bad-letter", "bad-letter-short", "bad-letter~"):
        assert rec(base, name) == tuple(blank(BAD_LETTER))
    assert rec(base, "lower-case-and-u") == rec(base, "assembled")
    assert all(st.record[11] == 0 and not st.record[0] & OVER_BUDGET for st in everything)
    assert all(0 < max(w.most_visits(*setting), 1) < DEFAULT_VISITS // 4 for setting in SETTINGS)


@pytest.mark.parametrize("stranded", [False, True])
def test_the_world_reaches_every_branch_on_the_oracle(stranded):
    assert_every_branch_is_reached(world(25, stranded))


def test_lookahead_zero_counts_every_run_and_a_clip_of_zero_tests_every_edge():
    w = world(25, False)
    loose = w.named(0, 0, 0, 0.0)
    assert not any(st.visits for st in loose.values())            # no edge is below a clip of 0: no depth search
    assert loose["one-kmer-assembled"].record[0] == REPRESENTED and "short_run" not in loose["one-kmer-assembled"].tags
    assert loose["blunt-artifact"].record[:2] == (REPRESENTED, WHY_TRUE) and loose["blunt-artifact"].record[8] > 0     # an identity of 0.0 passes whatever the distance
    assert loose["insertion-3"].record[1] == WHY_PATH_LENGTH and loose["deletion-1"].record[1] == WHY_PATH_LENGTH       # no indel allowed
    five = w.named(5, 2, 1, 0.9)
    assert "short_run" in five["three-kmers-assembled"].tags and five["deletion-1"].record[0] == REPRESENTED


def test_the_budget_flips_exactly_the_query_with_the_most_calls():
    w = world(25, False)
    setting = (3, 1, 40, 0.9)
    base = w.judged(*setting)
    most = w.most_visits(*setting)
    who = [i for i, st in enumerate(base) if st.visits and max(st.visits) == most]
    assert [w.names[i] for i in who] == ["edge-in-the-graph-deepest"] and most == 40 - 12
    at, below = w.judged(*setting, max_visits=most), w.judged(*setting, max_visits=most - 1)
    assert [st.record for st in at] == [st.record for st in base]
    assert [i for i, (x, y) in enumerate(zip(below, base)) if x.record != y.record] == who
    assert below[who[0]].record == tuple(blank(OVER_BUDGET)) and "over_budget" in below[who[0]].tags
    assert most < DEFAULT_VISITS // 4


def test_the_other_worlds_reach_their_branches():
    for w in (world_143(), world_hashes()):
        got = w.named(3, 1, 10, 0.9)
        assert {st.record[1] for st in got.values()} >= {0, 1, 2, 3, 4, 5, 6, 8, 9}
        assert {st.record[10] for st in got.values()} == {PATH_NONE, PATH_LEFT, PATH_RIGHT, PATH_SPLICED}
        assert got["edge-long"].record[0] == REPRESENTED and "widening_stops_on_an_unassembled_kmer_right" in got["widening-meets-unassembled"].tags
