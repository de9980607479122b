"""rb_graph_extend_loop restated — the CALL, not only the loop: GraphUtils.extendSE / extendPE (R/util/GraphUtils.java:6454-6678) with what the call
adds to them (include/rb_capi.h): the letters it judges, `room` with whole rounds only, `phase`, and every field of rb_extend_loop_rec.  Built
over the step functions of tests/test_extend_step_rules.py and tests/test_extend_pe_rules.py and run on the CPU oracle:
 (a) with room 4096 the restated call gives the text and range of extend_se / extend_pe for every seed, status DONE;
 (b) chained calls with room D + 2 and with room 256, resumed as rb_capi.h says, give the same texts and summed extensions;
 (c) the seeds of every world tests/test_gpu_extend_loop.py uses reach every ending on both sides;
and graphutils.extendSEOnDevice / extendPEOnDevice chain and fall back as they should, over a stand-in graph whose call is the restatement."""
import functools

import numpy as np
import pytest

import pair_worlds as PW
import test_extend_pe_rules as P
import test_extend_step_rules as R

F32 = np.float32
SE, PE = 0, 1
DONE, ROOM, NOT_JUDGED = range(3)
WHY_NONE, WHY_NO_KMER, WHY_LETTER = range(3)
END_NOT_RUN, END_NOTHING, END_USED_SHORT, END_USED_PAIR, END_ROOM = range(5)
FIELDS = ("status", "why", "left_ext", "right_ext", "out_len", "left_end", "right_end", "left_rounds", "right_rounds", "steps", "floor_drops",
          "used_passed", "left_floor", "right_floor")
AMPLE = 4096


def blank(seq):
    rec = dict.fromkeys(FIELDS, 0)
    rec["left_floor"] = rec["right_floor"] = F32(0)
    rec["out_len"] = len(seq)
    return rec


def restated_call(g, seq, min_cov, D, k, step, room, phase=0, trace=None):
    """rb_graph_extend_loop of one sequence: (text, record as a dict of FIELDS).  step(g, text, direction, floor, D, k) is extend_step or the PE
    step.  trace (a dict) gets what the record does not hold: per side the rounds that were used and went on, and whether an outer iteration
    saw the floor fall twice."""
    rec = blank(seq)
    if len(seq) < k or any(ch not in b"ACGT" for ch in seq):
        rec["status"], rec["why"] = NOT_JUDGED, WHY_NO_KMER if len(seq) < k else WHY_LETTER
        return seq, rec
    n0 = len(seq) - k + 1
    kmers = [seq[i:i + k] for i in range(n0)]
    cnts = [F32(c) for c in g.counts(seq)]
    used = set(kmers)
    text = seq
    for direction, side in ((1, "left"), (0, "right")):
        if direction == 1:
            kmers.reverse(); cnts.reverse()                                                    # :6465
        run = phase == 0 if direction == 1 else rec["left_end"] != END_ROOM
        added, end = 0, END_NOT_RUN
        while run:
            thr = min(cnts[max(0, len(kmers) - D):])                                            # :6468
            drops = 0
            while True:                                                                         # :6472-6480
                thr = max(F32(min_cov), F32(thr * F32(0.1)))
                e = step(g, text, direction, thr, D, k).ext
                rec["steps"] += 1
                rec[side + "_floor"] = thr
                if e or thr == F32(min_cov):
                    break
                drops += 1
            rec["floor_drops"] += drops
            if trace is not None:
                trace[side + "_most_drops"] = max(trace.get(side + "_most_drops", 0), drops)
                if drops >= 2:
                    trace[side + "_drops_twice"] = True
            if not e:
                end = END_NOTHING                                                               # :6482
                break
            if len(e) > room - added:
                end = END_ROOM                                                                  # only whole rounds
                break
            if all(km in used for km, _, _ in e):                                               # :6486-6495 (:6497-6504 cannot clear the flag)
                if len(kmers) < D:
                    end = END_USED_SHORT
                    break
                if R.has_duplicated_kmer_pair(kmers, e[-1][0], D, len(kmers) - 1 - D + len(e)):
                    end = END_USED_PAIR
                    break
                rec["used_passed"] += 1
                if trace is not None:
                    trace[side + "_used_passed"] = trace.get(side + "_used_passed", 0) + 1
            kmers += [km for km, _, _ in e]                                                     # :6510-6511
            cnts += [c for _, c, _ in e]
            used.update(km for km, _, _ in e)
            add = bytes(R.ACGT[b] for _, _, b in e)
            text = add[::-1] + text if direction == 1 else text + add
            added += len(e)
            rec[side + "_rounds"] += 1
        rec[side + "_ext"], rec[side + "_end"] = added, end
        if direction == 1:
            kmers.reverse(); cnts.reverse()
    rec["status"] = ROOM if END_ROOM in (rec["left_end"], rec["right_end"]) else DONE
    rec["out_len"] = len(text)
    return text, rec


def chained(call, seq, room):
    """calls resumed as rb_capi.h says until the status is no longer ROOM: (text, the summed left extension, records)"""
    text, rec = call(seq, room, 0)
    left, recs = rec["left_ext"], [rec]
    while rec["status"] == ROOM:
        text, rec = call(text, room, 0 if rec["left_end"] == END_ROOM else 1)
        left += rec["left_ext"]
        recs.append(rec)
    return text, left, recs


# ---- the worlds: k = 25 (SE d 30; PE d_r 30, d_f 80), and the matrix over pair_worlds.CASES ----
MATRIX_KS = (16, 32, 33, 64, 65, 128, 255, 256)


def seeds_of(w, hot, mirror, n=200):
    """R.driver_seeds with random pieces of k .. k + 54 letters (its own rule, k .. 79, has no length to draw from k = 80 on; at k = 25 these ARE
    its 200 seeds): the special seeds first.  mirror: every special seed reversed as well, behind them."""
    rng = np.random.default_rng(9)
    seeds = list(hot) + [s[::-1] for s in hot]
    seeds += [s if dd == 0 else s[::-1] for kind, s, dd in w.queries if kind in ("circle", "poly-only", "tandem", "fork2-short", "junction-2")]
    if mirror:                                                # the worlds are mirrored: what ends one side of a seed ends the other side of its reverse
        seeds += [s[::-1] for s in seeds[2 * len(hot):]]
    while len(seeds) < n:
        t = w.tx[int(rng.integers(0, len(w.tx)))][0]
        a = int(rng.integers(0, max(1, len(t) - (w.k + 55))))
        seeds.append(t[a:a + int(rng.integers(w.k, w.k + 55))])
    return [s for s in seeds if len(s) >= w.k and all(ch in b"ACGT" for ch in s)][:n]


class Side:
    """one world and one of the two loops over it: the oracle side, the distances, the step, the seeds, the reference loop"""

    def __init__(self, w, which, mirror=False):
        self.w, self.which, self.k, self.o = w, which, w.k, w.o
        if which == PE:
            self.d_r, self.D = w.d_r, w.d_f
            self.step = lambda g, text, direction, thr, d, k: P.extend_step_pe(g, text, direction, thr, w.d_r, w.d_f, k)
            self.seeds = seeds_of(w, w.w.hot, mirror)
        else:
            self.d_r = self.D = w.d
            self.step = R.extend_step
            self.seeds = seeds_of(w, w.hot, mirror)
        self._calls = {}

    def call(self, seq, room, phase=0, trace=None, min_cov=1.0):
        return restated_call(self.o, seq, min_cov, self.D, self.k, self.step, room, phase, trace)

    def ample(self, i):
        """the restated call of seed i with room 4096 and its trace, computed once and shared"""
        if i not in self._calls:
            trace = {}
            self._calls[i] = self.call(self.seeds[i], AMPLE, trace=trace) + (trace,)
        return self._calls[i]

    def reference(self, seq):
        return R.extend_se(self.o, seq, 1.0, self.D, self.k, step=self.step)

    def chain(self, seq, room):
        text, left, recs = chained(lambda s, r, ph: self.call(s, r, ph), seq, room)
        return text, [left, left + len(seq) - self.k + 1], recs

    def assert_reach(self):
        """(c): the 200 seeds reach, on both sides, END_NOTHING, END_USED_SHORT, END_USED_PAIR and a round that was used and went on"""
        assert len(self.seeds) == 200
        got = [self.ample(i) for i in range(200)]
        for side in ("left", "right"):
            ends = {rec[side + "_end"] for _, rec, _ in got}
            assert {END_NOTHING, END_USED_SHORT, END_USED_PAIR} <= ends, (side, ends)
            assert any(tr.get(side + "_used_passed", 0) > 0 for _, _, tr in got), side
        assert all(rec["status"] == DONE for _, rec, _ in got)

    def most_drops(self):
        """the most steps that returned nothing above the lowest floor in ONE outer iteration, over the 200 seeds and both sides"""
        return max(max(self.ample(i)[2].get("left_most_drops", 0), self.ample(i)[2].get("right_most_drops", 0)) for i in range(200))

    def picks(self, n=20):
        """n seeds for the chained calls: the longest grower, one of each ending on each side, the rest from the front"""
        grown = [self.ample(i)[1]["left_ext"] + self.ample(i)[1]["right_ext"] for i in range(len(self.seeds))]
        idx = [int(np.argmax(grown))]
        for side in ("left", "right"):
            for end in (END_NOTHING, END_USED_SHORT, END_USED_PAIR):
                idx += [i for i in range(len(self.seeds)) if self.ample(i)[1][side + "_end"] == end][:1]
        for i in range(len(self.seeds)):
            if len(set(idx)) >= n:
                break
            idx.append(i)
        return sorted(set(idx))


@functools.lru_cache(maxsize=None)
def side25(which, stranded):
    return Side(P.world(25, stranded) if which == PE else R.world(25, stranded), which)


@functools.lru_cache(maxsize=2)
def side_of_case(which, case):
    return Side(PW.pe_case(case) if which == PE else PW.step_case(case), which, mirror=True)


MATRIX = [c for c in PW.CASES if c.k in MATRIX_KS]
K25 = [(which, stranded) for which in (SE, PE) for stranded in (False, True)]
k25_id = lambda p: "%s-%s" % ("pe" if p[0] else "se", "stranded" if p[1] else "canonical")


# ---- the restatement by hand: room, whole rounds, phase, the not-judged ----
def test_the_restated_call_on_the_toy_graph():
    k, d = 4, 3
    g = R.Toy(k, [R.T_A, R.T_B], [1, 3]).build(d)
    call = lambda s, room, phase=0: restated_call(g, s, 1.0, d, k, R.extend_step, room, phase)
    for s in (R.T_A[4:10], R.T_B[8:14], R.T_A[:5]):
        want = R.extend_se(g, s, 1.0, d, k)
        text, rec = call(s, 64)
        assert (text, [rec["left_ext"], rec["left_ext"] + len(s) - k + 1]) == want and rec["status"] == DONE
        assert rec["out_len"] == len(text) == len(s) + rec["left_ext"] + rec["right_ext"] and rec["steps"] >= 2
        # room d + 2: every call adds whole rounds only, at most 5 letters a side, and the chain arrives where the ample call does
        ctext, cleft, recs = chained(call, s, d + 2)
        assert (ctext, [cleft, cleft + len(s) - k + 1]) == want
        assert all(r["left_ext"] <= d + 2 and r["right_ext"] <= d + 2 for r in recs)
        for r in recs[:-1]:
            assert r["status"] == ROOM and (r["right_end"] == END_NOT_RUN if r["left_end"] == END_ROOM else r["right_end"] == END_ROOM)
        # phase 1: the left side is taken as ended
        ptext, prec = call(s, 64, 1)
        assert prec["left_ext"] == 0 and prec["left_end"] == END_NOT_RUN and prec["left_floor"] == 0 and ptext.startswith(s)
    for s, why in ((b"ACG", WHY_NO_KMER), (b"", WHY_NO_KMER), (b"ACGNT", WHY_LETTER), (b"ACgTT", WHY_LETTER), (b"ACGUT", WHY_LETTER)):
        text, rec = call(s, 64)
        assert text == s and rec == dict(blank(s), status=NOT_JUDGED, why=why)
    unit = b"ACGGTCA"                                         # a circle: the loop ends by usedKmers + hasDuplicatedKmerPair
    circ = R.Toy(k, [unit * 8]).build(d)
    text, rec = restated_call(circ, (unit * 3)[:10], 1.0, d, k, R.extend_step, 64)
    assert (text, [rec["left_ext"], rec["left_ext"] + 7]) == R.extend_se(circ, (unit * 3)[:10], 1.0, d, k)
    assert END_USED_PAIR in (rec["left_end"], rec["right_end"]) and rec["used_passed"] > 0


# ---- (a) (b) (c) on the k = 25 worlds ----
@pytest.mark.parametrize("p", K25, ids=k25_id)
def test_ample_room_equals_the_reference_loop_and_reaches_every_ending(p):
    sd = side25(*p)
    assert len(sd.seeds) == 200
    for i, s in enumerate(sd.seeds):
        text, rec, _ = sd.ample(i)
        assert (text, [rec["left_ext"], rec["left_ext"] + len(s) - sd.k + 1]) == sd.reference(s), i
        assert rec["status"] == DONE and max(rec["left_ext"], rec["right_ext"]) < AMPLE
    sd.assert_reach()
    assert sd.most_drops() >= 2                               # an outer iteration in which the floor fell twice


@pytest.mark.parametrize("p", K25, ids=k25_id)
def test_chained_calls_equal_the_ample_call(p):
    sd = side25(*p)
    picks = sd.picks()
    assert len(picks) >= 20
    for room in (sd.D + 2, 256):
        resumed = 0
        for i in picks:
            text, rec, _ = sd.ample(i)
            ctext, crng, recs = sd.chain(sd.seeds[i], room)
            assert ctext == text and crng[0] == rec["left_ext"] and sum(r["right_ext"] for r in recs) == rec["right_ext"], (room, i)
            assert sum(r["left_rounds"] for r in recs) == rec["left_rounds"] and sum(r["right_rounds"] for r in recs) == rec["right_rounds"]
            assert (recs[-1]["left_end"] or rec["left_end"], recs[-1]["right_end"]) == (rec["left_end"], rec["right_end"]), (room, i)
            resumed += len(recs) > 1
        assert resumed > 0, room


# ---- (c) on the matrix worlds ----
@pytest.mark.parametrize("case", MATRIX, ids=PW.case_id)
def test_matrix_worlds_reach_every_ending(case):
    """Every ending on both sides in the SE and in the PE world of the case.  The floor falls twice in one outer iteration somewhere in the case:
    in every PE world (three times), and in the SE worlds at k = 16, 64, 65, 128 and the canonical one at 256; in the SE worlds at k = 32, 33,
    255 and the stranded one at 256 it falls once at the most (the stretches covered 150 times more give one drop: 158 -> 15.8 -> 1.58 finds
    the branches), which the walks of those worlds happen not to exceed."""
    drops = []
    for which in (SE, PE):
        sd = side_of_case(which, case)
        sd.assert_reach()
        drops.append(sd.most_drops())
    assert max(drops) >= 2 and drops[1] >= 2, drops


# ---- the package's wrappers without a device: a stand-in whose extendLoop is the restated call ----
class LoopStandIn(P.StepStandInPE):
    EXTL_SE, EXTL_PE, EXTL_DONE, EXTL_ROOM, EXTL_NOT_JUDGED = SE, PE, DONE, ROOM, NOT_JUDGED

    def __init__(self, sd):
        P.StepStandInPE.__init__(self, sd.o, sd.k, sd.d_r, sd.D)
        self.sd, self.loops = sd, []

    def extendLoop(self, seqs, which, minKmerCov, room, phase=None):
        assert which == self.sd.which
        self.loops.append((len(seqs), room, None if phase is None else list(phase)))
        got = [self.sd.call(s, room, 0 if phase is None else phase[i], min_cov=minKmerCov) for i, s in enumerate(seqs)]
        recs = np.zeros(len(seqs), [(f, "<f4" if f.endswith("floor") else "<i4") for f in FIELDS])
        for i, (_, rec) in enumerate(got):
            for f in FIELDS:
                recs[i][f] = rec[f]
        return [t for t, _ in got], recs


@pytest.mark.parametrize("which", [SE, PE], ids=["se", "pe"])
def test_the_package_s_device_route_chains_and_falls_back(which):
    from rnabloom import graphutils
    sd = side25(which, False)
    picks = sd.picks()
    fork = next(s for kind, s, dd in sd.w.queries if kind == "fork-0" and dd == 0)
    odd = [fork[:-1] + b"N", fork[:40].lower() + fork[40:], fork.replace(b"T", b"U"), fork[:sd.k - 1], b""]
    seeds = [sd.seeds[i] for i in picks] + odd
    dev = LoopStandIn(sd)
    on_device = graphutils.extendPEOnDevice if which == PE else graphutils.extendSEOnDevice
    host_loop = graphutils.extendPE if which == PE else graphutils.extendSE
    texts, ranges = on_device(dev, seeds, 1.0, room=sd.D + 2)
    for j, i in enumerate(picks):
        text, rec, _ = sd.ample(i)
        assert (texts[j], ranges[j]) == (text, [rec["left_ext"], rec["left_ext"] + len(seeds[j]) - sd.k + 1]), i
    want = host_loop(LoopStandIn(sd), odd, 1.0)
    assert (texts[len(picks):], ranges[len(picks):]) == (want[0], want[1])
    # one call for all, then only the sequences out of room, their room doubled and their phase from their records
    assert dev.loops[0] == (len(seeds), sd.D + 2, None) and len(dev.loops) > 1
    for (n1, r1, _), (n2, r2, ph) in zip(dev.loops, dev.loops[1:]):
        assert n2 <= n1 - (len(odd) if n1 == len(seeds) else 0) and r2 == 2 * r1 and len(ph) == n2 and set(ph) <= {0, 1}
    assert dev.calls > 0 and dev.most == sum(len(s) >= sd.k for s in odd)                       # the host loop ran for the not-judged only
