"""The in-order represented-then-add loop on the CPU oracle alone (tests/represented_then_add_worlds.py): the existing represented worlds are a
test bed on which ORDER MATTERS — a batched call against a snapshot of the gate cannot stand in for the loop — and the hand-made list, the
orders and the over-budget stop that tests/test_gpu_represented_then_add.py relies on are reached.  No device is needed."""
import represented_then_add_worlds as W
import test_represented_rules as R


def test_order_matters_on_the_world():
    w = R.world(25, False)
    in_order = W.walked(w, "world", "list", W.BASE)
    snapshot = [st.record for st in w.judged(*W.BASE)]
    differ = sum(x != y for x, y in zip(in_order.records, snapshot))
    assert differ >= 15, differ                                   # measured: 20 of 114
    assert {r[1] for r in in_order.records} >= {0, 1, 2, 3, 4, 5, 6, 8, 9}
    assert in_order.n_done == len(w.queries) and 0 < sum(in_order.keep) < len(w.queries)
    # a kept sequence is judged and false, and only a kept one has a median
    for rec, keep, med in zip(in_order.records, in_order.keep, in_order.median):
        assert keep == (rec[0] == 0) and (keep or med == 0)
    assert sum(med > 0 for med in in_order.median) >= 15


def test_other_orders_keep_other_sequences():
    w = R.world(25, False)
    seqs = [s for _, s in w.queries]
    kept = {}
    for order in ("list", "reverse", "length"):
        got = W.walked(w, "world", order, W.BASE)
        kept[order] = {i for i, s in enumerate(seqs) for j, t in enumerate(W.ordered(seqs, order)) if got.keep[j] and t is s}
    assert kept["reverse"] != kept["list"] and kept["length"] != kept["list"]
    lens = [len(s) for s in W.ordered(seqs, "length")]
    assert lens == sorted(lens, reverse=True) and len(set(lens)) < len(lens)          # ties: the sort must be stable to be the reference's


def test_the_hand_made_list_from_an_empty_gate():
    w = R.world(25, False)
    hm = W.hand_made(w)
    got = W.walked(w, "empty", "list", W.BASE, seqs=[s for _, s, _, _ in hm], tag="hand-made")
    for (what, _, flags, why), rec, keep in zip(hm, got.records, got.keep):
        assert rec[0] == flags and (why is None or rec[1] == why) and keep == (flags == 0), (what, rec)
    assert got.n_done == len(hm)


def test_a_budget_stops_the_walk_strictly_inside_the_list():
    w = R.world(25, False)
    seqs, budget, p = W.stop_case(w)
    assert 0 < p < len(seqs) - 1
    free = W.walked(w, "world", "list", W.CLIP40, seqs=seqs, tag="stop-free")
    stopped = W.walked(w, "world", "list", W.CLIP40, max_visits=budget, seqs=seqs, tag="stop")
    assert free.n_done == len(seqs) and not any(r[0] & (R.OVER_BUDGET | W.NOT_REACHED) for r in free.records)
    assert stopped.n_done == p and stopped.records[p] == tuple(R.blank(R.OVER_BUDGET))
    assert stopped.records[:p] == free.records[:p] and stopped.keep[:p] == free.keep[:p]
    assert all(r == tuple(R.blank(W.NOT_REACHED)) for r in stopped.records[p + 1:]) and not any(stopped.keep[p:])
    assert (stopped.median[p:] == 0).all()


def test_the_other_worlds_behave_alike():
    for w, setting in ((R.world(25, True), W.BASE), (R.world_hashes(), W.CLIP40), (R.world_143(), W.BASE)):
        in_order = W.walked(w, "world", "list", setting)
        snapshot = [st.record for st in w.judged(*setting)]
        assert sum(x != y for x, y in zip(in_order.records, snapshot)) >= 15
