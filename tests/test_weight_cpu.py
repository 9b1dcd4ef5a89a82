"""The weighted-sweep table (tests/weight_cases.py) without a GPU: the numpy restatement of the sweep equals the oracle on
every shot that reached OSD, and the inputs of tests/test_gpu_weight_edges.py, decoded on the oracle, decide what that test
is about -- shots reach OSD, the search moves away from OSD-0, the weights matter (the Hamming-weight search picks another
candidate), and for the two-valued vector the winner depends on the order of the additions and on the tie rule.  A drift of
the inputs fails here, so the GPU test cannot go vacuous.

Shots on which BP converged (the all-zero syndrome among them) do not reach the sweep: the oracle returns BP's decoding for
them, and the restatement has nothing to say.  The "rows" kind is the same oracle computation as "select" and "flat-rows"
the same as the uniform decode (tests/weight_cases.reference), so each pair is checked once."""
import functools

import numpy as np
import pytest

from tests import weight_cases as wc
from tests.edge_codes import EDGE_BY_ID, kprime, osd_words

IDS = [r["id"] for r in wc.WEIGHT_EDGES]


@functools.lru_cache(maxsize=None)
def report(row_id):
    """Per checked kind of a row: shots, osd (shots BP did not converge on), moved (osdw != osd0), hamming (the search with unit
    weights picks another candidate), order / tie (vector only: the sum_descending / last_wins mutant changes osdw), mismatch
    (shots on which the restatement differs from the oracle: must stay empty)."""
    row, inp = wc.ROW_BY_ID[row_id], wc.inputs(row_id)
    Hd, S = wc.dense(row["edge"]), inp["S"]
    ones = np.ones(Hd.shape[1])
    kinds = ["vector", "select", "flat-rows"] + (["continuous"] if row["continuous"] else []) + (["extreme"] if row_id == wc.EXTREME_ROW else [])
    out = {}
    for kind in kinds:
        ref = wc.reference(row_id, kind)
        c = dict(shots=len(S), osd=0, moved=0, hamming=0, order=0, tie=0, mismatch=[])
        for b in np.flatnonzero(ref["converged"] == 0):
            cost = wc.kind_cost(row_id, kind, b)
            sw = wc.Sweep(Hd, S[b], ref["llr"][b], row["method"], row["order"], row.get("bit_order") or 0)
            specs = [(cost, False)] + ([(ones, False)] if kind != "flat-rows" else []) + ([(cost, True)] if kind == "vector" else [])
            ws = sw.weights(specs)
            win = sw.pick(ws[0])
            if not ((sw.candidate(0) == ref["osd0"][b]).all() and (sw.candidate(win) == ref["osdw"][b]).all()):
                c["mismatch"].append(int(b))
            c["osd"] += 1
            c["moved"] += win != 0
            if kind != "flat-rows":
                c["hamming"] += sw.pick(ws[1]) != win
            if kind == "vector":
                c["order"] += sw.pick(ws[2]) != win
                c["tie"] += sw.pick(ws[0], last_wins=True) != win
        out[kind] = c
    return out


@pytest.mark.parametrize("row_id", IDS)
def test_restatement_equals_oracle_and_the_inputs_decide(row_id):
    row = wc.ROW_BY_ID[row_id]
    rep = report(row_id)
    print(row_id, {k: {x: v[x] for x in ("shots", "osd", "moved", "hamming", "order", "tie")} for k, v in rep.items()})
    cap = 2 * (11 if row["hbm"] else (48 if EDGE_BY_ID[row["edge"]]["n"] <= 1023 else 24))
    assert row["shots"] <= cap
    for kind, c in rep.items():
        assert not c["mismatch"], f"{kind}: the restatement differs from the oracle on shots {c['mismatch']}"
        assert 2 * c["osd"] > c["shots"], f"{kind}: only {c['osd']} of {c['shots']} shots reach OSD"
        assert c["moved"] >= 1, f"{kind}: osdw == osd0 on every shot"
        if kind != "flat-rows":
            assert c["hamming"] >= 1, f"{kind}: the weights never decide"
    v = rep["vector"]
    assert v["tie"] >= 1, "no tie-rule-sensitive shot"
    if row["method"] == "osd_e" or EDGE_BY_ID[row["edge"]]["n"] <= 255:
        assert v["order"] >= 1, "no order-sensitive shot"
    sel, uni = wc.reference(row_id, "select"), wc.reference(row_id, "uniform")
    assert any((sel[k] != uni[k]).any() for k in ("osdw", "bp", "iters")), "the select kind equals the uniform decode"


def test_joint_order_sensitivity():
    small = sum(report(r["id"])["vector"]["order"] for r in wc.WEIGHT_EDGES if not r["hbm"])
    hbm = sum(report(r["id"])["vector"]["order"] for r in wc.WEIGHT_EDGES if r["hbm"])
    print("order-sensitive shots: small path", small, "HBM path", hbm)
    assert small >= 20 and hbm >= 2


def test_table_instances_and_inputs():
    assert len(set(IDS)) == len(IDS) == 24
    for row in wc.WEIGHT_EDGES:
        e = EDGE_BY_ID[row["edge"]]
        m, n = e["m"], e["n"]
        assert row["order"] <= kprime(e) and row["osd_variant"] == e["osd_variant"]
        if m <= 1024 and n <= 2047:
            assert not row["hbm"] and row["osd"] == ("osd_kernel", (osd_words(n),)), row["id"]
            if e["osd"][0] == "osd_kernel":
                assert row["osd"] == e["osd"]
            else:  # the dispatch rows: the EDGES row asks for (and without weights gets) a wave kernel
                assert e["osd_variant"] == 2 and e["osd"][0] in ("osd_wave_kernel", "osd_mw_kernel")
        else:
            assert row["hbm"] and row["osd"] == e["osd"] and e["osd"][0] == "osd_large_kernel", row["id"]
        inp = wc.inputs(row["id"])
        share, hi, lo = wc.MIXES[row["mix"]]
        assert inp["S"].shape == (row["shots"], m) and not inp["S"][-1].any() and inp["S"][:-1].any(axis=1).all()
        assert set(np.unique(inp["vec"])) == {hi, lo} and inp["q"] == lo
        assert (inp["rows"] == np.where(inp["sel"] != 0, hi, lo)).all() and (inp["flat"] == lo).all()
        assert all(not a.flags.writeable for a in inp.values() if isinstance(a, np.ndarray))
    widths = {r["osd"][1][0] for r in wc.WEIGHT_EDGES if not r["hbm"]}
    assert widths == {1, 2, 4, 8, 16, 24, 31, 32}
    assert {r["osd"][1][0] for r in wc.WEIGHT_EDGES if r["hbm"]} == {2, 4, 8}
    assert {wc.ROW_BY_ID[i]["hbm"] for i in wc.UPDATE_ROWS} == {False, True}


def test_extreme_probabilities_leave_no_nan():
    """Entries of exactly 1.0 and 0.0 on bits that pairwise share no check: prior LLRs of -inf / +inf and costs of 0 / +inf go
    through BP and the sweep without a NaN, and the restatement (checked with the table) follows the oracle."""
    vec, picked = wc.extreme_vector()
    H = wc.matrix(wc.ROW_BY_ID[wc.EXTREME_ROW]["edge"])
    assert (vec[list(picked[:3])] == 1.0).all() and (vec[list(picked[3:])] == 0.0).all() and ((vec == 0) | (vec == 1)).sum() == 6
    sub = H[:, list(picked)]
    assert (np.asarray(sub.sum(axis=1)).ravel() <= 1).all(), "two of the bits share a check"
    cost = wc.cost_of(vec)
    assert (cost[list(picked[:3])] == 0.0).all() and np.isinf(cost[list(picked[3:])]).all()
    ref = wc.reference(wc.EXTREME_ROW, "extreme")
    assert not np.isnan(ref["llr"]).any()
    assert np.isinf(ref["llr"][:, list(picked)]).all()
    assert (ref["osdw"][:, list(picked[3:])] == 0).all(), "a bit that cannot be in error is set"


def test_unit_weights_restate_the_hamming_search():
    """The "hamming" counts weigh with unit costs; on one row that is held against the oracle's weight_fn = 1 search."""
    from oracle import OracleDecoder

    row_id = "osd_kernel_W1_n63-osd_cs6"
    row, inp = wc.ROW_BY_ID[row_id], wc.inputs(row_id)
    H = wc.matrix(row["edge"])
    ref = wc.reference(row_id, "vector")
    o = OracleDecoder(H, channel_probs=inp["vec"], weight_fn=1, **wc.settings(row))
    for b in np.flatnonzero(ref["converged"] == 0):
        r = o.osd(inp["S"][b], ref["llr"][b])
        osd0, osdw = wc.sweep_restatement(H, inp["S"][b], ref["llr"][b], np.ones(H.shape[1]), row["method"], row["order"])
        assert (osd0 == r["osd0"]).all() and (osdw == r["osdw"]).all(), b


@pytest.mark.parametrize("row_id", ["osd_kernel_W1_n63-osd_cs6", "osd_kernel_W2_n64-osd_e5"])
def test_mutants_are_the_restatement_with_one_thing_changed(row_id):
    """sweep_restatement on the smallest row of either method: without a flag it equals tests/ref_numpy.osd_decode (plain
    Python), each flag changes osdw on as many shots as the table counts, and the bit-by-bit sums are ``np.cumsum``'s, in
    either direction."""
    from tests import ref_numpy

    row, inp = wc.ROW_BY_ID[row_id], wc.inputs(row_id)
    H = wc.dense(row["edge"])
    ref = wc.reference(row_id, "vector")
    cost = wc.cost_of(inp["vec"])
    changed = {"sum_descending": 0, "last_wins": 0}
    for b in np.flatnonzero(ref["converged"] == 0):
        s, llr = inp["S"][b], ref["llr"][b]
        got0, gotw = wc.sweep_restatement(H, s, llr, cost, row["method"], row["order"])
        if b < 12:
            osd0, osdw, _, _ = ref_numpy.osd_decode(H, s, llr, inp["vec"], row["method"], row["order"])
            assert (got0 == osd0).all() and (gotw == osdw).all(), b
        for flag in changed:
            changed[flag] += (wc.sweep_restatement(H, s, llr, cost, row["method"], row["order"], **{flag: True})[1] != gotw).any()
        sw = wc.Sweep(H, s, llr, row["method"], row["order"])
        up, down = sw.weights([(cost, False), (cost, True)])
        assert (up.view(np.uint64) == sw.weights_by_cumsum(cost).view(np.uint64)).all()
        assert (down.view(np.uint64) == sw.weights_by_cumsum(cost, descending=True).view(np.uint64)).all()
    rep = report(row_id)["vector"]
    assert changed == {"sum_descending": rep["order"], "last_wins": rep["tie"]} and min(changed.values()) >= 1, changed
