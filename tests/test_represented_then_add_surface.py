"""What of rb_graph_represented_then_add can be held without a GPU: the walker kernel's resources beside those of the two kernels it shares its
body with, read from the code objects inside librb_hip.so; the symbol, its binding and the new not-judged bit; the refusals that come before
any device call; and the host logic of graphutils.writeTranscripts / reduceRedundancy — the stable sort by length, cid / l= / c=, and the
resumption behind an over-budget stop — over a stand-in graph whose representedThenAdd IS the restated loop on the CPU oracle
(tests/represented_then_add_worlds.py).  Every test here fails on a tree without the call."""
import ctypes as C
import os
import re

import numpy as np

import represented_then_add_worlds as W
import test_represented_rules as R
from test_capi_symbols import ROOT, _kernel_resources


def kernel(fragment):
    found = {name: v for name, v in _kernel_resources().items() if fragment in name}
    assert len(found) == 1, (fragment, sorted(found))
    return next(iter(found.values()))


DFS, ROW = 4 * 17 * 24, 1024 * 4                                 # a wavefront's lookahead stacks and its alignment row in LDS


def test_the_walker_spills_nothing_and_holds_one_wavefronts_rows_in_lds():
    vgprs, spilled, lds = kernel("k_represented_walk")
    assert spilled == 0 and vgprs <= 256, (vgprs, spilled)
    assert DFS + ROW < lds <= DFS + ROW + 16, lds                 # ... and the verdict's flags


def test_the_kernels_that_share_the_body_keep_their_lds_and_spill_nothing():
    vgprs, spilled, lds = kernel("13k_representedE")
    assert spilled == 0 and vgprs <= 256 and lds == 4 * (DFS + ROW), (vgprs, spilled, lds)
    vgprs, spilled, lds = kernel("k_screen")
    assert spilled == 0 and vgprs <= 256 and lds == 4 * DFS, (vgprs, spilled, lds)


def test_the_symbol_its_binding_and_the_new_bit():
    from rnabloom import _native as N
    from rnabloom.graph import BloomFilterDeBruijnGraph as G
    assert "rb_graph_represented_then_add" in {s[0] for s in N.SYMBOLS} and hasattr(N.lib, "rb_graph_represented_then_add")
    header = open(os.path.join(ROOT, "include", "rb_capi.h")).read()
    assert re.search(r"RB_SCREEN_NOT_REACHED\s*=\s*64\b", header) and N.SCREEN_NOT_REACHED == G.SCREEN_NOT_REACHED == 64
    # the next free bit of the not-judged set: above every bit a record's flags could carry before
    assert N.SCREEN_NOT_REACHED == 2 * N.SCREEN_OVER_BUDGET and not N.SCREEN_NOT_REACHED & (G.SCREEN_NOT_JUDGED | N.REPR_REPRESENTED)
    assert callable(G.representedThenAdd) and callable(G.representedThenAddFlat)


def test_refusals_that_need_no_device_write_nothing():
    from rnabloom import _native as N
    seq = np.frombuffer(b"ACGT" * 20, np.uint8).copy()
    off = np.array([0, 80], np.int64)
    rec, keep, med, done = np.full(12, 7, np.int32), np.full(1, 7, np.uint8), np.full(1, 7, np.float32), np.full(1, 7, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                   # noqa: E731
    fake = C.c_void_p(0)
    for g, gate in ((None, None), (None, fake), (fake, None)):   # a null graph, a null gate: refused before either is looked into
        rc = N.lib.rb_graph_represented_then_add(g, gate, p(seq), p(off), 1, 3, 1, 10, 0.9, 0, p(rec), p(keep), p(med), p(done))
        assert rc == 1 and b"rb_graph_represented_then_add" in N.lib.rb_last_error()
        assert (rec == 7).all() and keep[0] == 7 and med[0] == 7 and done[0] == 7


def test_the_median_is_the_references():
    from rnabloom import graphutils
    for counts in ([3.0], [1.0, 2.0], [5.0, 1.0, 3.0], [1.0, 2.0, 4.0, 8.0], [16777216.0, 16777218.0], [0.0] * 6):
        assert np.float32(graphutils._median_f32(counts)).view(np.uint32) == W.median_coverage([np.float32(c) for c in counts]).view(np.uint32)


class OracleGate:
    """a screeningBf over an oracle gate: add(h0) as rnabloom.bloom.BloomFilter.add takes it"""

    def __init__(self, w, gate):
        self.w, self.gate = w, gate

    def add(self, h0):
        from oracle import rbo
        for h in np.asarray(h0, np.uint64):
            self.gate.add_dbg_only(rbo.ntm64(int(h), self.w.k, self.gate.h))


class OracleGraph:
    """what graphutils asks of a graph, answered by the restated loop on the CPU oracle"""

    def __init__(self, w):
        from rnabloom.graph import BloomFilterDeBruijnGraph as G
        self.w, self.k, self.stranded, self.REPR_DTYPE = w, w.k, w.stranded, G.REPR_DTYPE
        self.calls = []

    def representedThenAdd(self, seqs, bf, lookahead, max_indel, clip, identity, max_visits=0):
        got = W.walk(self.w, bf.gate, list(seqs), (lookahead, max_indel, clip, identity), max_visits)
        self.calls.append(len(seqs))
        recs = np.array([tuple(r) for r in got.records], self.REPR_DTYPE) if got.records else np.zeros(0, self.REPR_DTYPE)
        return recs, np.array(got.keep, np.uint8), got.median, got.n_done

    def getKmers(self, seqs):
        f, r, c = self.w.og.get_kmers(seqs[0])
        return None, f, r, c


def records(recs):
    return [tuple(int(rc[f]) for f in R.FIELDS) for rc in recs]


def test_reduce_redundancy_sorts_stably_by_length_and_numbers_what_it_keeps():
    from rnabloom import graphutils
    w = R.world(25, False)
    seqs = [s for _, s in w.queries]
    shuffled = [seqs[i] for i in np.random.default_rng(7).permutation(len(seqs))]
    want = W.walked(w, "world", "length", W.BASE, seqs=shuffled, tag="shuffled")
    by_length = W.ordered(shuffled, "length")
    g, bf = OracleGraph(w), OracleGate(w, W.fresh_gate(w, w.gate_seqs))
    kept, removed = graphutils.reduceRedundancy(g, bf, shuffled, *W.BASE)
    exp = [by_length[i] for i in np.flatnonzero(want.keep)]
    assert [s for _, _, s in kept] == exp and [(cid, l) for cid, l, _ in kept] == [(j + 1, len(s)) for j, s in enumerate(exp)]
    assert removed == len(seqs) - len(exp) and g.calls == [len(seqs)]
    assert (bf.gate.dbgbf_bytes() == want.gate_bytes()).all()


def test_write_transcripts_resumes_behind_a_stop_either_way():
    from rnabloom import graphutils
    w = R.world(25, False)
    seqs, budget, p = W.stop_case(w)
    # the default decision and an explicit "no": the stopped sequence is left out, the rest is what the walk without it gives
    left_out = W.walked(w, "world", "list", W.CLIP40, seqs=seqs[:p] + seqs[p + 1:], tag="stop-left-out")
    g, bf = OracleGraph(w), OracleGate(w, W.fresh_gate(w, w.gate_seqs))
    kept, recs = graphutils.writeTranscripts(g, bf, seqs, *W.CLIP40, maxVisits=budget, decide=lambda i, s: False)
    want_idx = [int(i) + (i >= p) for i in np.flatnonzero(left_out.keep)]
    assert kept == [(i, len(seqs[i]), "%.1f" % float(left_out.median[i - (i > p)])) for i in want_idx]
    assert records(recs) == left_out.records[:p] + [tuple(R.blank(R.OVER_BUDGET))] + left_out.records[p:]
    assert g.calls == [len(seqs), len(seqs) - p - 1] and (bf.gate.dbgbf_bytes() == left_out.gate_bytes()).all()
    # "yes": its k-mers go into the filter before the walk goes on, and it is written with its own median
    gate = W.fresh_gate(w, w.gate_seqs)
    head = W.walk(w, gate, seqs[:p], W.CLIP40, budget)
    W.add_kmers(w, gate, seqs[p].upper().replace(b"U", b"T"))
    tail = W.walk(w, gate, seqs[p + 1:], W.CLIP40, budget)
    assert head.n_done == p and tail.n_done == len(seqs) - p - 1
    asked = []
    g, bf = OracleGraph(w), OracleGate(w, W.fresh_gate(w, w.gate_seqs))
    kept, recs = graphutils.writeTranscripts(g, bf, seqs, *W.CLIP40, maxVisits=budget, decide=lambda i, s: asked.append((i, s)) or True)
    assert asked == [(p, seqs[p])]
    want_idx = [int(i) for i in np.flatnonzero(head.keep)] + [p] + [p + 1 + int(i) for i in np.flatnonzero(tail.keep)]
    assert [i for i, _, _ in kept] == want_idx and all(l == len(seqs[i]) for i, l, _ in kept)
    mid = W.median_coverage([np.float32(c) for c in w.og.get_kmers(seqs[p])[2]])
    assert dict((i, c) for i, _, c in kept)[p] == "%.1f" % float(mid)
    assert records(recs) == head.records + [tuple(R.blank(R.OVER_BUDGET))] + tail.records
    assert (bf.gate.dbgbf_bytes() == gate.dbgbf_bytes()).all()
