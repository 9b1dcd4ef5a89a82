"""The harvest of failing shots without a GPU: ``engine="numpy"`` on the CPU oracle -- the figures the GPU
tests of tests/test_gpu_harvest.py are held against, recomputed and pinned here so that those cannot pass on a degenerate
batch -- every residual against rows the test keeps itself, the cap, batch splits, the log-weights of a tilted run, what is
refused, and the kernel cases' own rows."""
import json
import os

import numpy as np
import pytest

from bp_osd_amd import _lib
from bp_osd_amd._dem_base import harvest_batch
from tests import dem_cases as dc
from tests import harvest_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_harvest_calls_are_declared_and_listed_for_export():
    public = open(os.path.join(ROOT, "include", "bposd_mi355x.h")).read()
    debug = open(os.path.join(ROOT, "include", "bposd_mi355x_debug.h")).read()
    for name in ("bposd_dem_set_harvest", "bposd_dem_harvest_info", "bposd_window_set_harvest", "bposd_window_harvest_info"):
        assert name in _lib.EXPORTED_SYMBOLS and f"int {name}(" in public, name
    assert "bposd_debug_dem_harvest" in _lib.DEBUG_SYMBOLS and "int bposd_debug_dem_harvest(" in debug
    for engine, items, first in (("DEM", _lib.DEM_ITEMS, 11), ("WINDOW", _lib.WINDOW_ITEMS, 8)):
        for i, item in enumerate(hc.ITEMS):
            assert items[item][0] == first + i and f"BPOSD_{engine}_{item.upper()} = {first + i}" in public, (engine, item)


@pytest.mark.parametrize("case", hc.RUN_CASES, ids=[c["id"] for c in hc.RUN_CASES])
def test_oracle_harvest_is_what_the_gpu_tests_expect(case):
    """The figures of the case, and every harvested residual against faults ^ correction from rows this test keeps."""
    H, L, priors, _ = hc.model(case)
    B, N = case["B"], H.shape[1]
    factory, kept = hc.keeping_oracle()
    sim = hc.sim(case, "numpy", B, factory=factory)
    ref = hc.run_reference(case["id"])
    flags, faults = sim.last_batch("flags"), dc.unpack(sim.last_batch("faults"), N)
    if case["kind"] == "dem":
        assert len(kept) == 1
        corr, failing = kept[0] & 1, (flags & 4) != 0
    else:
        corr, failing = dc.unpack(sim.last_batch("correction"), N), (flags & 3) == 1
        assert sim.residual_count == 0
        # the committed correction is the windows' kept rows at their committed faults
        again = np.zeros_like(corr)
        assert len(kept) == len(sim.plan.windows)
        for win, rows in zip(sim.plan.windows, kept):
            sel = np.flatnonzero(win.commit)
            again[:, win.fault[sel]] = rows[:, sel] & 1
        assert (again == corr).all()
    residual = faults ^ corr
    assert not dc.mod2(H, residual).any(), "H (f ^ c) = 0 on every shot of the case"
    rows = np.flatnonzero(failing)
    weight = residual[rows].sum(axis=1)
    F = sim.failures
    print(case["id"], "failures", rows.size, "rows", rows[:10], "weights", weight[:10], "min", sim.min_logical_weight, sim.min_logical_shot)
    # the issue's figures
    assert rows.size == case["failures"] and 0 < rows.size < B
    if case["first"] is not None:
        assert tuple(rows[:len(case["first"])]) == case["first"]
    if case["weights"] is not None:
        assert tuple(np.sort(weight)[:len(case["weights"])]) == case["weights"]
    lightest = rows[weight == weight.min()]
    if case["lightest"] is not None:
        assert lightest.size == case["lightest"]
    assert weight.min() == case["min_weight"] and tuple(lightest[:len(case["tied"])]) == case["tied"]
    # the harvest
    assert (F["shot"] == rows).all() and F["shot"].dtype == np.uint64 and (F["weight"] == weight).all() and F["weight"].dtype == np.int32
    assert (F["residual"] == dc.pack(residual[rows])).all() and (F["faults"] == dc.pack(faults[rows])).all()
    assert dc.mod2(L, residual[rows]).any(axis=1).all(), "L r != 0 on every harvested row"
    assert sim.min_logical_weight == case["min_weight"] and sim.min_logical_shot == case["tied"][0]
    assert sim.min_logical_fault.dtype == np.uint8 and (sim.min_logical_fault == residual[case["tied"][0]]).all()
    counts = sim.failure_weight_counts
    assert counts.shape == (N + 1,) and counts.dtype == np.int64 and counts.sum() == rows.size
    assert (counts == np.bincount(weight, minlength=N + 1)).all()
    assert (sim.last_batch("fail_rows") == rows).all() and (sim.last_batch("fail_weight") == weight).all()
    assert (sim.last_batch("min_residual") == dc.pack(residual[[case["tied"][0]]])[0]).all()
    assert json.loads(sim.output_dict())["min_logical_weight"] == case["min_weight"]
    # and the shared reference of the GPU tests is this run
    assert (ref["failures"]["residual"] == F["residual"]).all() and ref["min_logical_shot"] == sim.min_logical_shot


def test_a_cap_of_two_keeps_two_rows_and_still_finds_the_lightest():
    case = hc.RUN_BY_ID["surface13-R3"]
    ref = hc.run_reference("surface13-R3")
    sim = hc.sim(case, "numpy", 2)
    assert sim.failures["shot"].tolist() == [5, 6] and sim.failures["residual"].shape == (2, 2)
    assert (sim.failures["residual"] == ref["failures"]["residual"][:2]).all() and (sim.failures["faults"] == ref["failures"]["faults"][:2]).all()
    assert sim.min_logical_shot == 17 and sim.min_logical_weight == 3
    assert (sim.min_logical_fault == ref["min_logical_fault"]).all() and (sim.last_batch("min_residual") == ref["items"]["min_residual"]).all()
    assert sim.failure_weight_counts.sum() == 44 and (sim.failure_weight_counts == ref["failure_weight_counts"]).all()
    assert sim.last_batch("fail_rows").size == 44 and sim.last_batch("fail_residual").shape == (2, 2)


@pytest.mark.parametrize("kind,case_id", [("dem", "surface13-R3"), ("window", "surface13-R3-w21")])
@pytest.mark.parametrize("split", [(64, 64, 128), (100, 100, 56)], ids=["64+64+128", "100s"])
def test_batch_splits_give_the_attributes_of_one_batch(kind, case_id, split):
    case = hc.RUN_BY_ID[case_id]
    ref = hc.run_reference(case_id)
    sim = hc.sim(case, "numpy", case["B"], batch_size=max(split), run_sim=False)
    for B in split:
        sim._run_batch_numpy(B)
    assert sim.run_count == 256
    for key in hc.RESULTS:
        assert np.array_equal(getattr(sim, key), ref[key]), key
    for key, v in ref["failures"].items():
        assert np.array_equal(sim.failures[key], v) and sim.failures[key].dtype == v.dtype, key
    assert json.loads(sim.output_dict())["min_logical_weight"] == json.loads(ref["output"])["min_logical_weight"]
    # a cap below the failures of the first batch: later batches are asked for nothing they could add
    capped = hc.sim(case, "numpy", 3, batch_size=64)
    assert np.array_equal(capped.failures["shot"], ref["failures"]["shot"][:3]) and capped.min_logical_shot == ref["min_logical_shot"]
    assert (capped.failure_weight_counts == ref["failure_weight_counts"]).all()


def test_a_tilted_run_keeps_the_log_weights_of_its_failures():
    case = hc.RUN_BY_ID["surface13-R3"]
    sim = hc.sim(case, "numpy", 256, sample_scale=4)
    F = sim.failures
    rows = np.flatnonzero(sim.last_batch("flags") & 4)
    assert rows.size > 44 and (F["shot"] == rows).all()  # a harsher draw fails more often
    assert F["logw"].dtype == np.int64 and (F["logw"] == sim.last_batch("logw")[rows]).all() and len(set(F["logw"].tolist())) > 1
    assert "logw" not in hc.run_reference("surface13-R3")["failures"]


def test_harvest_off_changes_nothing():
    case = hc.RUN_BY_ID["surface13-R3"]
    off = hc.sim(case, "numpy", 0)
    plain = dc.oracle_sim(*dc.run_model("surface13-R3"), 256)
    assert off.output_dict() == plain.output_dict() and "min_logical_weight" not in json.loads(off.output_dict())
    for key in hc.RESULTS + ("failures",):
        assert getattr(off, key, None) is None, key
    with pytest.raises(ValueError, match="harvest"):
        off.last_batch("fail_rows")
    on = json.loads(hc.run_reference("surface13-R3")["output"])
    assert set(on) == set(json.loads(plain.output_dict())) | {"min_logical_weight"}
    w = hc.RUN_BY_ID["surface13-R3-w21"]
    off = hc.sim(w, "numpy", 0)
    assert off.failures is None and off.min_logical_weight is None
    assert set(json.loads(hc.run_reference("surface13-R3-w21")["output"])) == set(json.loads(off.output_dict())) | {"min_logical_weight"}
    with pytest.raises(ValueError, match="harvest"):
        off.last_batch("min_residual")


@pytest.mark.parametrize("bad", [-1, 1.5, "2", None, True])
def test_harvest_must_be_a_count(bad):
    for case_id in ("surface13-R3", "surface13-R3-w21"):
        with pytest.raises(ValueError, match="harvest"):
            hc.sim(hc.RUN_BY_ID[case_id], "numpy", bad, run_sim=False)


def test_nothing_failed_leaves_none():
    """p = 0: no fault fires, nothing fails; the attributes say so and the items are empty."""
    H, L, priors = dc.run_model("surface13-R3")
    from bp_osd_amd.dem import dem_decode_sim
    from oracle import OracleDecoder

    sim = dem_decode_sim(H, L, priors * 0, batch_size=32, engine="numpy", seed=1, target_runs=32, decoder_factory=OracleDecoder, harvest=4, **dc.DECODER)
    assert sim.min_logical_weight is None and sim.min_logical_shot is None and sim.min_logical_fault is None
    assert sim.failure_weight_counts.sum() == 0 and sim.failures["shot"].size == 0 and sim.failures["residual"].shape == (0, 2)
    assert sim.last_batch("fail_rows").size == 0 and not sim.last_batch("min_residual").any()
    assert json.loads(sim.output_dict())["min_logical_weight"] is None


@pytest.mark.parametrize("case", hc.KERNEL_CASES, ids=[c["id"] for c in hc.KERNEL_CASES])
def test_kernel_cases_show_what_they_are_for(case):
    """The rows of the kernel cases on the reference alone, and the two host restatements against each other."""
    faults, corr, select = hc.kernel_rows(case["id"])
    ref = hc.kernel_reference(case["id"])
    N, B, K = case["N"], case["B"], case["K"]
    assert faults.shape == corr.shape == (B, N) and select.shape == (B,)
    count, min_w, min_row = ref["info"]
    if case["select"] == "none":
        assert ref["info"] == (0, -1, -1) and not ref["min_residual"].any() and ref["fail_residual"].shape == (0, 2)
    elif case["select"] == "all":
        assert count == B and ref["fail_residual"].shape[0] == min(B, K)
    else:
        assert 0 < count < B and (select > 1).any()
    if case["special"] == "ends":
        assert ref["fail_rows"][0] == 0 and ref["fail_rows"][-1] == B - 1
    w, rows = ref["fail_weight"], ref["fail_rows"]
    if case["special"] == "tie":
        tied = rows[w == min_w]
        assert tied.size == 3 and min_row == tied.min() and list(w).index(min_w) > 0
        assert np.flatnonzero(w == min_w)[0] == 7  # and the slots were not made in row order
    if case["special"] == "last":
        assert (w == min_w).sum() == 1 and min_row == rows[-1] and w[-1] == min_w
    if case["special"] == "beyond":
        assert (w == min_w).sum() == 1 and list(rows).index(min_row) >= K and ref["min_residual"].any()
        assert not (ref["fail_residual"] == ref["min_residual"]).all(axis=1).any()
    own = harvest_batch(faults, corr, select, K)
    assert (own["fail_count"], own["min_weight"], own["min_row"]) == ref["info"]
    for item in hc.ITEMS:
        assert own[item].dtype == ref[item].dtype and np.array_equal(own[item], ref[item]), item
