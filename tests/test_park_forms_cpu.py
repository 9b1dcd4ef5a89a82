"""The plan of tests/test_gpu_park_forms.py (tests/park_forms_cases.py) without a GPU, on the oracle alone: what keeps the
device table from being trivial."""
import numpy as np
import pytest

from tests import park_forms_cases as pf
from tests.local_park_cases import CH, PARK_ROWS, batch_index, crosses

IDS = [c["id"] for c in pf.CASES]


@pytest.mark.parametrize("case", pf.CASES, ids=IDS)
def test_pool_has_its_edge_shots_under_its_own_setting(case):
    """Under the setting's own channels and scaling factor the pool holds the zero syndrome, a shot the oracle converges in
    exactly CH - 1, CH and CH + 1 iterations and one it gives up on; at max_iter CH nothing of the batch crosses a boundary,
    at every larger max_iter the CH, CH + 1, stuck and late shots do and the CH - 1 shot and the zero syndrome do not."""
    row_id, setting = case["row"], case["setting"]
    p = pf.plan(row_id, setting)
    assert p["pool"].shape[0] == pf.N_POOL == len(p["rows"]) and not p["pool"][0].any()
    K = len(pf.channel(row_id, setting)["R"])
    assert K == (pf.N_ROWS if setting in ("rows", "sel") else 1)
    assert len(set(p["rows"].tolist())) >= min(K, 4), "the pool draws on few of the setting's rows"
    assert set(batch_index(case["B"])) == set(range(pf.N_POOL))
    top = pf.reference(row_id, setting, pf.MAX_ITERS[-1])
    for k, i in p["edge"].items():
        assert top["converged"][i] and top["iters"][i] == k, (case["id"], k)
    assert top["iters"][0] == 0 and top["converged"][0]
    for mi in pf.MAX_ITERS:
        ref = pf.reference(row_id, setting, mi)
        assert not ref["converged"][p["stuck"]] and ref["iters"][p["stuck"]] == mi
        c = crosses(ref["iters"], mi)
        for nb in (case["B"], pf.B_EXACT):
            n = pf.planned_parks(row_id, setting, nb, mi)
            print(case["id"], "max_iter", mi, "B", nb, "pool rows that cross", np.flatnonzero(c).tolist(), "of the batch", n)
            if mi <= CH:
                assert n == 0 and not c.any()
            else:
                assert n >= nb // pf.N_POOL * int(c.sum()) > 0
        if mi > CH:
            assert c[p["edge"][CH]] and c[p["edge"][CH + 1]] and c[p["stuck"]] and c[p["late"]].all() and not c[p["edge"][CH - 1]] and not c[0]
    at = pf.reference(row_id, setting, CH)
    assert at["converged"][p["edge"][CH]] and at["iters"][p["edge"][CH]] == CH and not at["converged"][p["edge"][CH + 1]]
    assert pf.reference(row_id, setting, CH + 1)["converged"][p["edge"][CH + 1]]  # restored straight into the LLR body, converges there


@pytest.mark.parametrize("case", [c for c in pf.CASES if c["setting"] != "varscale"], ids=[i for i in IDS if not i.endswith("varscale")])
def test_parked_shots_are_sensitive_to_their_priors(case):
    """At least three of the shots that park decode differently (iters, bp or osd0) under the channel a continuation with
    the wrong source of priors would use -- the handle's own channel for rows and select bytes, the scalar prior q for the
    per-bit form -- than under their own.  This is necessary for the device test to notice a wrong prior; it is not
    sufficient: a continuation decodes with the wrong prior only from the restored iteration on, which this oracle run
    (wrong from iteration 1) does not restate."""
    row_id, setting = case["row"], case["setting"]
    ch = pf.channel(row_id, setting)
    assert (ch["R"] == 0.5).sum(axis=1).min() >= (2 if setting != "sel" else 0)
    if setting in ("rows", "sel"):  # the rows differ from each other and from the handle's channel
        assert len({r.tobytes() for r in ch["R"]}) == pf.N_ROWS and all((r != ch["other"]).any() for r in ch["R"])
    for mi in pf.MAX_ITERS:
        if mi > CH:
            s = pf.sensitive_rows(row_id, setting, mi)
            print(case["id"], "max_iter", mi, "parked pool rows", pf.parked_pool_rows(row_id, setting, mi).tolist(), "sensitive", s.tolist())
            assert s.size >= 3, (case["id"], mi, s)


def test_table_reaches_every_instance():
    """By the dispatch of launch_bp_local restated (``expected_instance``), not by the device: the per-bit form reaches
    all four UPRIOR = false shapes -- <1,1024,8>, <2,1024,6> plain and with a PAIRKEY, <2,2048,4> -- in byte and packed
    form, the rows form the three it can be given within the size limit, the select form the pair instance, and the
    variable factor runs UPRIOR = true on a one-check-per-thread call and on the pair instance (MINW 8 there)."""
    reach = {}
    for c in pf.CASES:
        for packed in c["forms"]:
            for nb in (c["B"], pf.B_EXACT):
                (name, shape, pk), pair, up = pf.expected_instance(c["row"], c["setting"], nb, packed)
                assert name == "bp_local_kernel"
                reach.setdefault(c["setting"], set()).add((shape, pair, up, pk))
    shapes = [((1, 1024, 8, 0), False), ((2, 1024, 6, 0), False), ((2, 1024, 6, 0), True), ((2, 2048, 4, 0), True)]
    for shape, pair in shapes:
        for packed in (False, True):
            assert (shape, pair, False, packed) in reach["bit"], (shape, pair, packed)
    for shape, pair in (shapes[0], shapes[1], shapes[3]):
        assert (shape, pair, False, False) in reach["rows"], (shape, pair)
    assert (shapes[0] + (False, False)) in reach["sel"] and (shapes[2] + (False, False)) in reach["sel"]
    assert reach["varscale"] == {((1, 1024, 8, 0), False, True, False), ((2, 1024, 8, 0), True, True, False)}
    # the rows are those of the existing park table, and no input array of a case exceeds about 100 MB
    park_rows = {r for r, _ in PARK_ROWS}
    for c in pf.CASES:
        assert c["row"] in park_rows
        n = 2 * pf.row_by_id(c["row"])["m"]
        largest = {"rows": 8 * n, "sel": n}.get(c["setting"], n // 2)  # bytes per shot: an fp64 row, select bytes, the syndrome
        assert c["B"] * largest <= 100e6, (c["id"], c["B"] * largest)
    assert pf.row_by_id(pf.PAIR_ROW)["pairkey"] >= 0 and pf.row_by_id("reg128_s1")["pairkey"] < 0


@pytest.mark.parametrize("stage", pf.STAGES, ids=[s["id"] for s in pf.STAGES])
def test_stages_see_parked_shots(stage):
    """Behind BP every stage has work that parked: shots BP gives up on among those that cross a boundary -- for LSD some of
    them with status 0 (solved by lsd_kernel from the LLR rows the continuation wrote) --, and the weighted sweep changes
    some parked shot's row (osdw != osd0), so that its weights matter."""
    row_id, setting = stage["row"], stage["setting"]
    assert pf.row_by_id(row_id)["m"] <= 1024 and pf.STAGE_B <= pf.SMALL_CALL
    changed = 0
    for mi in pf.STAGE_ITERS:
        ref = pf.stage_reference(stage, mi)
        plain = pf.reference(row_id, setting, mi)
        for k in ("bp", "converged", "iters"):
            assert (np.asarray(ref[k]) == np.asarray(plain[k])).all(), (stage["id"], k)
        parked = crosses(ref["iters"], mi)
        open_ = parked & (np.asarray(ref["converged"]) == 0)
        assert open_.sum() >= 3, (stage["id"], mi)
        if stage["lsd"] is not None:
            assert (np.asarray(ref["status"])[open_] == 0).any(), (stage["id"], mi)
            assert (np.asarray(ref["status"])[np.asarray(ref["converged"]) != 0] == -1).all()
        changed += int((np.asarray(ref["osdw"])[open_] != np.asarray(ref["osd0"])[open_]).any(axis=1).sum())
    if stage["osd"][0] == "osd_cs" and stage["lsd"] is None or (stage["lsd"] or ("", 0))[0] == "lsd_cs":
        assert changed > 0, (stage["id"], "no sweep improves on a parked shot")


def test_observables_and_dem_plans():
    """Two observable words; the engine's batch, decoded by engine="numpy" around the oracle, holds shots that cross a
    boundary, converged and not, on a call size that takes one check per thread."""
    L = pf.observable_matrix(128)
    assert L.shape == (65, 128) and pf.observables_packed(np.eye(128, dtype=np.uint8), L).shape == (128, 2)
    assert (pf.observables_packed(np.eye(128, dtype=np.uint8)[:1], L)[0, 1] == L[64, 0])
    H, Lm, priors = pf.dem_model()
    assert H.shape == (64, 128) and Lm.shape == (65, 128) and len(set(priors.tolist())) > 100
    ref = pf.dem_reference()
    it, conv = ref.last_batch("iters"), ref.last_batch("converged")
    c = crosses(it, pf.DEM_KW["max_iter"])
    print("dem shots", len(it), "cross", int(c.sum()), "of them converged", int((conv[c] != 0).sum()))
    assert len(it) == pf.DEM_B <= pf.SMALL_CALL and (conv[c] != 0).any() and (conv[c] == 0).any()
    assert 0 < ref.osdw_success_count < ref.run_count
