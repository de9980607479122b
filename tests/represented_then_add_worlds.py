"""The in-order represented-then-add loop — TranscriptWriter.write (R/RNABloom.java:1639-1720), GraphUtils.reduceRedundancy
(R/util/GraphUtils.java:652-699) — restated over the CPU oracle: what rb_graph_represented_then_add must report for a list of sequences and
leave in the gate.  The verdict is tests/test_represented_rules.judge, asked of a FRESH Side for every sequence (a Side memoises the gate's
answers, and the gate grows); a kept sequence's hash rows go into the oracle gate through add_dbg_only; its median is
getMedianKmerCoverage (R/util/GraphUtils.java:229-247) of the oracle's counts; the walk stops at the first sequence that is over its budget.
Not collected: a helper of tests/test_represented_then_add_reach.py (CPU) and tests/test_gpu_represented_then_add.py (device), which share
the walks computed here."""
import numpy as np

import test_represented_rules as R
import test_screen_rules as S
from test_extend_step_rules import F32

NOT_REACHED = 64                                                 # RB_SCREEN_NOT_REACHED
BASE, CLIP40 = (3, 1, 10, 0.9), (3, 1, 40, 0.9)                  # lookahead, max_indel, clip, identity


def fresh_gate(w, gate_seqs=()):
    """a new oracle gate of the world's size and hash count, empty or holding the k-mers of gate_seqs"""
    from oracle import rbo
    gate = rbo.Graph(w.gate_size, 64, 0, w.gate_h, 1, 1, w.k, True, False, 0)
    for t in gate_seqs:
        add_kmers(w, gate, t)
    return gate


def add_kmers(w, gate, seq):
    """screeningBf.add(kmer.getHash()) for every k-mer of seq (upper-case ACGT)"""
    from oracle import rbo
    hv, _ = rbo.hash_region(seq, w.k, gate.h, rbo.FWD if w.stranded else rbo.CANON)
    for row in hv:
        gate.add_dbg_only(row)


def median_coverage(counts):
    """getMedianKmerCoverage: the middle count, or the float32 mean of the two middle ones"""
    c = sorted(counts)
    n = len(c)
    return F32(c[n // 2]) if n % 2 else F32(F32(c[n // 2] + c[n // 2 - 1]) / F32(2))


class Walked:
    """records (12 ints each), keep, median (float32), n_done, the Screened of every sequence that was judged, and the gate afterwards"""

    def __init__(self, records, keep, median, n_done, judged, gate):
        self.records, self.keep, self.median, self.n_done, self.judged, self.gate = records, keep, np.asarray(median, np.float32), n_done, judged, gate

    def gate_bytes(self):
        return self.gate.dbgbf_bytes()


def walk(w, gate_og, seqs, setting, max_visits=0, before=None):
    """the reference's loop over seqs in list order against gate_og, which is written; before(i, fresh Side): a look at the gate as sequence i meets it"""
    records, keep, median, judged = [], [], [], []
    n_done = len(seqs)
    counts = {}                                                  # (the graph is read-only: its counts may be remembered across sequences)
    for i, seq in enumerate(seqs):
        if before is not None:
            probe = S.Side(w.og, gate_og)
            probe._c = counts
            before(i, probe)
        side = S.Side(w.og, gate_og)
        side._c = counts
        st = R.judge(side, seq, *setting, w.d, max_visits)
        judged.append(st)
        records.append(st.record)
        kept = st.record[0] == 0
        keep.append(1 if kept else 0)
        median.append(F32(0))
        if st.record[0] & R.OVER_BUDGET:
            n_done = i
            break
        if kept:
            text = seq.upper().replace(b"U", b"T")
            add_kmers(w, gate_og, text)
            median[-1] = median_coverage(side.counts(text))
    behind = len(seqs) - len(records)
    records += [tuple(R.blank(NOT_REACHED))] * behind
    keep += [0] * behind
    median += [F32(0)] * behind
    return Walked(records, keep, median, n_done, judged, gate_og)


def ordered(seqs, order):
    """list order, reverse order, or the stable sort by length, longest first (BitSequence.compareTo under Collections.sort)"""
    if order == "list":
        return list(seqs)
    if order == "reverse":
        return list(seqs)[::-1]
    assert order == "length"
    return sorted(seqs, key=lambda s: -len(s))


WALKS = {}


def walked(w, start, order, setting, max_visits=0, seqs=None, tag=None):
    """walk() once per (world, `world` gate or `empty` gate, order, setting, budget[, a named list]) for all tests of the session"""
    key = (id(w), start, order, setting, max_visits, tag)
    if key not in WALKS:
        assert start in ("world", "empty") and (seqs is None) == (tag is None)
        gate = fresh_gate(w, w.gate_seqs if start == "world" else ())
        if start == "world":
            assert (gate.dbgbf_bytes() == w.gate_og.dbgbf_bytes()).all()
        WALKS[key] = walk(w, gate, ordered([s for _, s in w.queries] if seqs is None else seqs, order), setting, max_visits)
    return WALKS[key]


def hand_made(w):
    """(what it is, sequence, expected flags, expected why or None) from an empty gate: a transcript, its copies and variants, two isoforms"""
    k = w.k
    full, iso1, iso2, unassembled = (w.tx[i][0] for i in (0, 4, 5, 3))
    snv = S.put(full, len(full) // 2, chr(S.other(full[len(full) // 2])[0]))
    return [("a full transcript", full, 0, None),
            ("the same transcript again", full, R.REPRESENTED, R.WHY_TRUE),
            ("the transcript with one changed letter", snv, R.REPRESENTED, None),
            ("an inner piece of it", full[50:300], R.REPRESENTED, None),
            ("the first isoform", iso1, 0, None),
            ("the second isoform", iso2, 0, R.WHY_RIGHT_IDENTITY),
            ("the second isoform again", iso2, R.REPRESENTED, None),
            ("exactly k letters", unassembled[70:70 + k], 0, R.WHY_NO_RUN),
            ("k - 1 letters", full[:k - 1], R.NO_KMER, None),
            ("a letter N", S.put(full[40:140], 30, "N"), R.BAD_LETTER, None)]


STOPS = {}


def stop_case(w):
    """(sequences, budget, stop index) at CLIP40 from the world's gate: the world's queries with `edge-in-the-graph-deepest` moved forward
    from the end of the list to the last place at which it still reaches its depth search under the in-order gate and makes more calls
    than every sequence before it; the budget is one call short of that, so the walk stops there and nowhere before"""
    if id(w) not in STOPS:
        at = w.names.index("edge-in-the-graph-deepest")
        rest = [s for i, (_, s) in enumerate(w.queries) if i != at]
        deepest = w.queries[at][1]
        # one walk over the rest, asking before every sequence how many calls the deepest query would make against the gate as it stands there
        there = {}
        free = walk(w, fresh_gate(w, w.gate_seqs), rest, CLIP40,
                    before=lambda i, side: there.__setitem__(i, max(R.judge(side, deepest, *CLIP40, w.d).visits, default=0)))
        calls = [max(st.visits, default=0) for st in free.judged]
        for p in range(len(rest) - 1, 0, -1):
            if there[p] > 1 and there[p] > max(calls[:p]):
                STOPS[id(w)] = (rest[:p] + [deepest] + rest[p:], there[p] - 1, p)
                break
        assert id(w) in STOPS, "no place in the list at which the deepest query reaches its depth search"
    return STOPS[id(w)]
