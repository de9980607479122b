"""The transcript worker's per-fragment calls beyond k = 25 and two hash functions: rb_graph_screen_fragments and rb_graph_represented
(csrc/rb_screen.hip) and rb_graph_trim_rc_artifacts (csrc/rb_trim.hip) on the worlds of tests/screen_worlds.py: k = 16 ... 256 on both sides of
64, 128 and 192, and 255 beside 256; stranded and canonical; hash counts (1, 1, 1), (3, 4, 3), (2, 2, 3), (3, 1, 2) and (2, 2, 2) with a gate
of 1, 3, 2, 4 and 2 functions.  What only runs there: the second to fourth round of the loops that spread a k-mer's letters over the lanes
(sc_walk_begin, sc_equals_seq, sc_equals_chain, tr_matches) and their last full round at k = 64, 128, 192 and 256; the rotations by 0, 31, 32
and 63 bits; getMaxCoveragePath with bounds of up to 2 k = 512 entries, a left walk that arrives at its 65th step and later and a splice at
entry 64 and beyond (wave_find's later rounds); isChimera's gap tests at exactly 2 k and 2 k + 1; represented's row capacity where read_d + k
wins (k = 16); alignments of more than 256 columns for every edge and gap at k = 256; HASHES' `numMatch >= k` and LONG's match length of
2 k at every k.  Every expected value is the restatements' (tests/test_screen_rules.py, tests/test_represented_rules.py,
tests/test_trim_artifact_rules.py) on the CPU oracle's filters; tests/test_screen_reach.py proves on the CPU that the worlds ask something.
The device graph and the gate are filled through the product's insert path and are the oracle's byte for byte before anything is compared;
every comparison is exact, every int of every record, through compare() of the calls' own device test files; the filters' folds are what
they were afterwards."""
import pytest

pytestmark = pytest.mark.gpu

from rnabloom import _native as N
from rnabloom.graph import _pack

import screen_worlds as SW
import test_gpu_represented as GR
import test_gpu_screen as GS
import test_gpu_trim_artifacts as GT

IDS = [SW.case_id(c) for c in SW.CASES]
PIECE_CASE = next(c for c in SW.CASES if c.k == 193 and c.stranded)


@pytest.fixture(scope="module", params=SW.CASES, ids=IDS)
def case(request):
    """module-scoped, so that the three tests of a case run one after the other and share its worlds"""
    return request.param


def gated_device(mod, w):
    """the device twins through the call's own device test file: filled by the product's insert path, every filter equal to the oracle's"""
    g, bf = mod.device(w)
    assert (g.exportFilter(N.DBGBF) == w.og.dbgbf_bytes()).all(), "dbgbf"
    assert (g.exportFilter(N.CBF) == w.og.cbf_bytes()).all(), "cbf"
    assert (g.exportFilter(N.RPKBF) == w.og.rpkbf_bytes()).all(), "rpkbf"
    assert (bf.toBytes() == w.gate_og.dbgbf_bytes()).all(), "gate"
    return g, bf


def release(mod, w):
    held = mod.DEVICES.pop(id(w), None)
    for h in (held if isinstance(held, tuple) else (held,)):
        if h is not None:
            h.destroy()


def test_screens(case):
    w = SW.screen_case(case)
    try:
        g, bf = gated_device(GS, w)
        before = GS.folds(g, bf)
        for lookahead, max_depth in SW.SCREEN_SETTINGS:
            got = GS.compare(w, (SW.case_id(case), lookahead, max_depth), lookahead, max_depth)
            assert not any(r[0] & GS.S.OVER_BUDGET for r in got)
            print("screens %s (%d, %d): %d queries, (chim_why, blunt_why) %s" % (SW.case_id(case), lookahead, max_depth, len(got), SW.outcome_counts((r[1], r[6]) for r in got)))
        assert GS.folds(g, bf) == before
    finally:
        release(GS, w)


def test_represented(case):
    w = SW.screen_case(case)
    try:
        g, bf = gated_device(GR, w)
        before = GR.folds(g, bf)
        got = GR.compare(w, SW.case_id(case), (3, 1, case.clip, case.identity))
        assert not any(r[0] & GR.R.OVER_BUDGET for r in got)
        print("represented %s clip %d identity %.1f: %d queries, (why, path_form) %s" % (SW.case_id(case), case.clip, case.identity, len(got), SW.outcome_counts((r[1], r[10]) for r in got)))
        assert GR.folds(g, bf) == before
    finally:
        release(GR, w)


def test_trim(case):
    w = SW.trim_case(case)
    try:
        g = GT.device(w)
        assert (g.exportFilter(N.DBGBF) == w.og.dbgbf_bytes()).all() and (g.exportFilter(N.CBF) == w.og.cbf_bytes()).all()
        before = GT.digests(g.h)
        for setting in w.settings:
            got = GT.compare(w, setting)
            print("trim %s %s: %d queries, (flags, pass 0 why, pass 1 why) %s" % (SW.case_id(case), setting, len(got), SW.outcome_counts((r[0], r[4], r[9]) for r in got)))
        assert GT.digests(g.h) == before
    finally:
        release(GT, w)


# ---- RB_QUERY_PIECE = 1: every sequence alone in its piece, its rows at offset 0 — against the whole call, byte for byte ----
def test_screens_a_sequence_a_piece(monkeypatch):
    w = SW.screen_case(PIECE_CASE)
    seq, off = _pack([s for _, s in w.queries])
    try:
        g, bf = gated_device(GS, w)
        whole = g.screenFragmentsFlat(seq, off, bf, 7, 3, 2)
        assert GS.records(whole) == [st.record for st in w.want(3, 2)]
        monkeypatch.setenv("RB_QUERY_PIECE", "1")
        assert g.screenFragmentsFlat(seq, off, bf, 7, 3, 2).tobytes() == whole.tobytes()
    finally:
        release(GS, w)


def test_represented_a_sequence_a_piece(monkeypatch):
    w = SW.screen_case(PIECE_CASE)
    setting = (3, 1, PIECE_CASE.clip, PIECE_CASE.identity)
    seq, off = _pack([s for _, s in w.queries])
    try:
        g, bf = gated_device(GR, w)
        whole = g.representedFlat(seq, off, bf, *setting)
        assert GR.records(whole) == [st.record for st in w.judged(*setting)]
        monkeypatch.setenv("RB_QUERY_PIECE", "1")
        assert g.representedFlat(seq, off, bf, *setting).tobytes() == whole.tobytes()
    finally:
        release(GR, w)


def test_trim_a_sequence_a_piece(monkeypatch):
    w = SW.trim_case(PIECE_CASE)
    seq, off = _pack([s for _, s in w.queries])
    try:
        g = GT.device(w)
        for setting in w.settings[:1] + w.settings[2:3] + w.settings[5:6]:        # HASHES, EDGE and LONG under their middle clips
            whole = g.trimArtifactsFlat(seq, off, *setting)
            assert GT.records(whole) == [rec for rec, _ in w.judged(*setting)]
            monkeypatch.setenv("RB_QUERY_PIECE", "1")
            assert g.trimArtifactsFlat(seq, off, *setting).tobytes() == whole.tobytes(), setting
            monkeypatch.delenv("RB_QUERY_PIECE")
    finally:
        release(GT, w)
