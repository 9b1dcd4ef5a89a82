"""Sliding-window decoding without a GPU: the plan against its definition, ``windowed_dem_decode_sim(engine="numpy")`` on the
CPU oracle -- the oracle's figures of the whole-run cases of tests/test_gpu_window.py, so that those cannot pass on a
degenerate batch -- and what construction refuses."""
import json

import numpy as np
import pytest

from bp_osd_amd import _lib, phenomenological_detector_times, window_plan
from bp_osd_amd.window import windowed_dem_decode_sim
from oracle import OracleDecoder
from tests import dem_cases as dc
from tests import window_cases as wc

PLANS = sorted({(c["model"], c["window"]) for c in wc.RUN_CASES})


def test_the_window_calls_are_listed_for_export():
    for name in ("bposd_window_create", "bposd_window_decode_device", "bposd_window_synchronize", "bposd_window_decode", "bposd_window_run",
                 "bposd_window_fetch", "bposd_window_device_bytes", "bposd_window_last_error", "bposd_window_destroy"):
        assert name in _lib.EXPORTED_SYMBOLS, name
    for name in ("bposd_debug_window_step", "bposd_debug_window_timing"):
        assert name in _lib.DEBUG_SYMBOLS, name


def test_phenomenological_detector_times():
    assert phenomenological_detector_times(3, 2).tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2]


@pytest.mark.parametrize("name,window", PLANS, ids=[f"{n}-{w[0]}{w[1]}" for n, w in PLANS])
def test_plan_follows_the_definition(name, window):
    H, L, priors, times = wc.model(name)
    plan = window_plan(H, times, window, priors=priors)
    W, C = window
    Hd = H.toarray()
    M, N = Hd.shape
    T = int(times.max()) + 1
    tau = np.array([times[Hd[:, i] != 0].min() if Hd[:, i].any() else -1 for i in range(N)])
    assert plan.T == T and (plan.tau == tau).all()
    # the last window is the first one whose hi reaches T
    assert [w.lo for w in plan.windows] == [i * C for i in range(len(plan.windows))]
    assert plan.windows[-1].hi >= T and all(w.hi < T for w in plan.windows[:-1])
    committed = np.zeros(N, int)
    for i, w in enumerate(plan.windows):
        assert w.hi == w.lo + W
        assert w.det.tolist() == [d for d in range(M) if w.lo <= times[d] < w.hi]
        assert w.fault.tolist() == [f for f in range(N) if w.lo <= tau[f] < w.hi]
        want = np.ones(w.fault.size, bool) if i == len(plan.windows) - 1 else tau[w.fault] < w.lo + C
        assert (w.commit.astype(bool) == want).all()
        assert (w.H.toarray() == Hd[np.ix_(w.det, w.fault)]).all()
        committed[w.fault[w.commit != 0]] += 1
    # every fault with a non-empty column is committed exactly once, an empty one never
    assert (committed == (tau >= 0)).all()
    # the dedup map: windows share a handle exactly when (H_w, priors_w) are equal
    for a in plan.windows:
        for b in plan.windows:
            same = (a.H.shape == b.H.shape and (a.H.toarray() == b.H.toarray()).all() and (priors[a.fault] == priors[b.fault]).all())
            assert same == (a.handle == b.handle), (a.index, b.index)
    assert [plan.windows[u].handle for u in plan.unique] == list(range(len(plan.unique)))
    # a step's word range covers what its commit touches and its gather reads
    assert len(plan.step_words) == len(plan.windows) + 1
    for s, (lo, hi) in enumerate(plan.step_words):
        bits = set()
        if s > 0:
            p = plan.windows[s - 1]
            bits |= set(np.flatnonzero(Hd[:, p.fault[p.commit != 0]].any(axis=1)).tolist())
        if s < len(plan.windows):
            bits |= set(plan.windows[s].det.tolist())
        assert (lo, hi) == (min(bits) >> 6, (max(bits) >> 6) + 1)


def test_time_invariant_models_need_few_handles():
    H, L, priors, times = wc.model("surface13-R5")
    plan = window_plan(H, times, (2, 1), priors=priors)
    assert len(plan.windows) == 5 and len(plan.unique) == 2
    H, L, priors, times = wc.model("hgp400-R3")
    plan = window_plan(H, times, (2, 1), priors=priors)
    assert [w.H.shape for w in plan.windows] == [(384, 1184), (384, 1184), (384, 992)]
    assert plan.step_words[2][0] > 0  # a step whose staged range does not start at word 0
    H, L, priors, times = wc.model("random-520-129-65")
    assert len(window_plan(H, times, (2, 1)).windows) == 4


@pytest.mark.parametrize("case", wc.RUN_CASES, ids=[c["id"] for c in wc.RUN_CASES])
def test_oracle_figures_of_the_run_cases(case):
    ref = wc.run_reference(case["id"])
    B, o = case["B"], case["oracle"]
    assert ref["run_count"] == B
    assert ref["bp_converge_count"] == o["converged"]
    assert B - ref["osdw_success_count"] == o["wrong"]
    assert ref["trivial_count"] == o["quiet"]
    # full-rank windows: the residual is zero on every shot
    assert ref["residual_count"] == 0 and not ref["residual"].any()
    assert not (ref["flags"] & 2).any()
    # the correction explains the detectors and gives the observables
    H, L, priors, times = wc.model(case["model"])
    corr = dc.unpack(ref["correction"], H.shape[1])
    assert (dc.pack(dc.mod2(H, corr)) == ref["detectors"]).all()
    empty = np.flatnonzero(np.diff(H.tocsc().indptr) == 0)
    assert not corr[:, empty].any()
    Lz = L.tolil()
    Lz[:, empty] = 0
    assert (dc.pack(dc.mod2(Lz, corr)) == ref["obs_osdw"]).all()
    assert int(((ref["flags"] & 1) != 0).sum()) == o["wrong"]


@pytest.mark.parametrize("name", sorted(wc.SINGLE_WINDOW))
def test_a_single_window_is_the_unwindowed_engine(name):
    ref = wc.single_window_reference(name)
    whole = dc.run_reference(wc.SINGLE_WINDOW[name])
    assert ref["run_count"] == whole["run_count"]
    assert ref["osdw_success_count"] == whole["osdw_success_count"]
    assert ref["bp_converge_count"] == whole["bp_converge_count"]
    assert ref["trivial_count"] == whole["trivial_count"]
    for item, other in (("obs_osdw", "obs_osdw"), ("observables", "observables"), ("detectors", "detectors"), ("converged", "converged"),
                        ("iters", "iters")):
        assert (ref[item] == whole[other]).all(), item


def test_batches_of_100_give_the_counters_of_one_batch():
    c = wc.RUN_BY_ID["surface13-R3-w21"]
    ref = wc.run_reference(c["id"])
    sim = wc.oracle_sim(c["model"], c["window"], c["B"], batch_size=100)
    for key in wc.COUNTS:
        assert getattr(sim, key) == ref[key], key
    assert (sim.osdw_observable_error_rates == ref["osdw_observable_error_rates"]).all()
    assert sim.last_batch("flags").shape == (56,)
    assert (sim.last_batch("obs_osdw") == ref["obs_osdw"][200:]).all()
    out = json.loads(sim.output_dict())
    assert out["run_count"] == 256 and out["windows"] == 3 and out["window"] == [2, 1]
    assert out["osdw_logical_error_rate"] == pytest.approx(45 / 256)


def test_refusals():
    H, L, priors, times = wc.toric_model()
    with pytest.raises(ValueError, match=r"window 1 .*18 x 45 with rank 17"):
        window_plan(H, times, (2, 1))
    with pytest.raises(ValueError, match="window 1"):
        windowed_dem_decode_sim(H, L, priors, times, (2, 1), engine="numpy", decoder_factory=OracleDecoder, run_sim=False, **wc.DECODER)
    H, L, priors, times = wc.model("surface13-R3")
    with pytest.raises(ValueError, match="1 <= C <= W"):
        window_plan(H, times, (2, 3))
    with pytest.raises(ValueError, match="1 <= C <= W"):
        window_plan(H, times, (2, 0))
    with pytest.raises(ValueError, match="length 24"):
        window_plan(H, times[:-1], (2, 1))
    gap = np.array(times) * 2  # no detector has an odd time: window 1 of (1, 1) is empty
    with pytest.raises(ValueError, match="window 1 .*holds 0 detectors"):
        window_plan(H, gap, (1, 1))
    # what the decoder's own constructor refuses comes back naming the window
    opts = dict(wc.DECODER, osd_order=60)
    with pytest.raises(ValueError, match="window 0"):
        windowed_dem_decode_sim(H, L, priors, times, (2, 1), engine="numpy", decoder_factory=OracleDecoder, run_sim=False, **opts)
