"""Importance sampling of detector error models without a GPU: ``importance_table`` and what it refuses, and
``dem_decode_sim(engine="numpy", sample_priors=... / sample_scale=...)`` on the CPU oracle -- neutral when q = p, within its
own error bar of the exact logical error rate of a model small enough to enumerate, and independent of the batch size.
Models and references: tests/dem_weight_cases.py."""
import functools
import json
import math

import numpy as np
import pytest

from bp_osd_amd import _lib, dem_decode_sim, importance_table
from tests import dem_cases as dc
from tests import dem_weight_cases as wc


def test_library_declares_the_sampling_call():
    assert "bposd_dem_set_sampling" in _lib.EXPORTED_SYMBOLS and _lib.DEM_ITEMS["logw"] == (10, "<i8", None)


# --------------------------------------------------------------------------------------------------- importance_table
def test_table_of_equal_rows_is_zero():
    p = np.array([0.0, 1.0, 1e-3, 0.03, 0.5, 0.999, 0.0, 1.0])
    incr, c0 = importance_table(p, p.copy())
    assert incr.dtype == np.int64 and incr.shape == p.shape and not incr.any()
    assert c0 == 0.0 and isinstance(c0, float)


def test_table_of_three_faults_by_hand():
    """p = (1/4, 1/100, 3/10), q = (1/2, 1/25, 3/10): a_0 = log(1/2) - log(3/2) = -log 3, a_1 = log(1/4) - log(99/96) = -log(33/8),
    a_2 = 0, c0 = log(3/2) + log(33/32) = log(99/64); the integers are round(a 2^32) from a 50-digit evaluation."""
    incr, c0 = importance_table([0.25, 0.01, 0.3], [0.5, 0.04, 0.3])
    assert incr.tolist() == [-4718503851, -6086252211, 0]
    assert c0 == pytest.approx(0.43623676677491807, rel=1e-15)
    # a fired fault 0 and a quiet fault 1: w = (p0 / q0) (1 - p1) / (1 - q1), up to 2^-33 relative per fired fault
    w = math.exp(c0 + int(incr[0]) / 2 ** 32)
    assert w == pytest.approx(0.5 * (0.99 / 0.96), rel=2.0 ** -32)


@pytest.mark.parametrize("what,p_i,q_i", [("q = 0 where p > 0", 0.2, 0.0), ("q = 1 where p < 1", 0.2, 1.0), ("NaN", 0.2, float("nan")),
                                          ("q < 0", 0.2, -0.1), ("q > 1", 0.2, 1.5), ("beyond e^64", 1e-40, 0.5), ("p = 0 where q > 0", 0.0, 0.5),
                                          ("p = 1 where q < 1", 1.0, 0.5)])
def test_table_refusals_name_the_fault(what, p_i, q_i):
    p = np.full(7, 0.1)
    q = np.full(7, 0.2)
    p[4], q[4] = p_i, q_i
    with pytest.raises(ValueError, match="fault 4"):
        importance_table(p, q)
    H, L, _ = dc.run_model("surface13-R3")
    pr = np.full(H.shape[1], 0.1)
    qr = np.full(H.shape[1], 0.2)
    pr[4], qr[4] = p_i, q_i
    with pytest.raises(ValueError, match="fault 4"):  # the front end refuses before it builds anything
        dem_decode_sim(H, L, pr, engine="numpy", sample_priors=qr, decoder_factory=lambda *a, **k: None, run_sim=False)


def test_table_wants_rows_of_one_length():
    # (the refusal of sum |incr| >= 2^62 needs 2^24 faults at |a| <= 64: the library's own check is tested on the device)
    with pytest.raises(ValueError, match="one length"):
        importance_table([0.1, 0.2], [0.1])


def test_front_end_arguments():
    H, L, p = dc.run_model("surface13-R3")
    make = lambda **kw: dem_decode_sim(H, L, p, engine="numpy", decoder_factory=lambda *a, **k: None, run_sim=False, **kw)
    with pytest.raises(ValueError, match="not both"):
        make(sample_priors=p, sample_scale=2)
    for bad in (0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sample_scale"):
            make(sample_scale=bad)
    with pytest.raises(ValueError, match="length"):
        make(sample_priors=p[:-1])
    pp = np.array([0.0, 1.0, 0.6, 0.5, 0.2, 0.01])
    sim = dem_decode_sim(np.ones((1, 6), np.uint8), np.ones((1, 6), np.uint8), pp, engine="numpy", decoder_factory=lambda *a, **k: None,
                         run_sim=False, sample_scale=4)
    assert sim._sample_priors.tolist() == [0.0, 1.0, 0.6, 0.5, 0.5, 0.04]
    with pytest.raises(ValueError, match="importance sampling"):
        make().last_batch("logw")


# --------------------------------------------------------------------------------------------------- runs on the oracle
def test_sampling_from_the_priors_is_neutral():
    """sample_priors = priors: the shots, counters and rates of the plain run, log-weights 0 and weights exactly 1."""
    case = dc.RUN_BY_ID["surface13-R3"]
    ref = dc.run_reference(case["id"])
    H, L, priors = dc.run_model(case["id"])
    plain = dc.oracle_sim(H, L, priors, case["B"])
    sim = wc.oracle_sim(H, L, priors, case["B"], sample_priors=priors.copy())
    for c in dc.COUNTS:
        assert getattr(sim, c) == ref[c], c
    for item in dc.ITEMS:
        assert (sim.last_batch(item) == ref[item]).all(), item
    logw = sim.last_batch("logw")
    assert logw.dtype == np.int64 and logw.shape == (case["B"],) and not logw.any()
    assert sim.weight_mean == 1.0 and sim.effective_sample_fraction == 1.0
    for x in ("bp", "osd0", "osdw"):
        assert getattr(sim, f"{x}_logical_error_rate") == getattr(plain, f"{x}_logical_error_rate"), x
        assert getattr(sim, f"{x}_logical_error_rate_eb") == pytest.approx(getattr(plain, f"{x}_logical_error_rate_eb"), rel=1e-12), x
    assert 0 < sim.osdw_logical_error_rate < 1
    a, b = json.loads(plain.output_dict()), json.loads(sim.output_dict())
    assert set(b) - set(a) == {"sample_scale", "weight_mean", "effective_sample_fraction"} and b["sample_scale"] is None
    assert all(a[k] == b[k] for k in a if not k.endswith("_eb"))


def test_plain_run_is_untouched():
    """Without the keywords: no new attribute or key, and the formulas of css_decode_sim."""
    case = dc.RUN_BY_ID["surface13-R3"]
    H, L, priors = dc.run_model(case["id"])
    plain = dc.oracle_sim(H, L, priors, case["B"])
    out = json.loads(plain.output_dict())
    assert not {"sample_scale", "weight_mean", "effective_sample_fraction"} & set(out) and not hasattr(plain, "weight_mean")
    ler = 1 - plain.osdw_success_count / case["B"]
    assert out["osdw_logical_error_rate"] == ler and out["osdw_logical_error_rate_eb"] == float(np.sqrt((1 - ler) * ler / case["B"]))


def test_exact_rate_is_the_one_enumerated_before():
    assert wc.exact_osdw_rate() == pytest.approx(9.468253753472913e-4, rel=1e-12)


@functools.lru_cache(maxsize=None)
def _plain(seed):
    H, L, p = wc.exact_model()
    return wc.oracle_sim(H, L, p, wc.EXACT_SHOTS, seed=seed)


@pytest.mark.parametrize("scale", wc.EXACT_SCALES)
@pytest.mark.parametrize("seed", wc.EXACT_SEEDS)
def test_tilted_estimate_meets_the_exact_rate(seed, scale):
    """[[13,1,3]] at R = 0, p = 0.01 / 0.004: the estimate of 16384 tilted shots lies within 4 of its own error bars of the exact
    osdw logical error rate, which is the sum over all 2^13 fault rows.

    Measured (exact 9.468254e-04; plain sampling at the same shots: eb 2.20e-04, 2.36e-04, 2.36e-04 on seeds 5, 6, 7):
        seed 5: scale 4  8.602e-04 +- 0.632e-04 (1.37 eb)   scale 8  8.872e-04 +- 0.379e-04 (1.57 eb)
        seed 6: scale 4  9.240e-04 +- 0.658e-04 (0.35 eb)   scale 8  9.586e-04 +- 0.394e-04 (0.30 eb)
        seed 7: scale 4 10.147e-04 +- 0.686e-04 (0.99 eb)   scale 8  9.671e-04 +- 0.396e-04 (0.51 eb)
    effective sample fraction 0.79-0.80 at scale 4 and 0.53 at scale 8, weight_mean within 0.8 % of 1."""
    H, L, p = wc.exact_model()
    exact = wc.exact_osdw_rate()
    plain = _plain(seed)
    sim = wc.oracle_sim(H, L, p, wc.EXACT_SHOTS, seed=seed, sample_scale=scale)
    rate, eb = sim.osdw_logical_error_rate, sim.osdw_logical_error_rate_eb
    print(f"seed {seed} scale {scale}: {rate:.6e} +- {eb:.3e} ({abs(rate - exact) / eb:.2f} eb of exact {exact:.6e}); plain "
          f"{plain.osdw_logical_error_rate:.3e} +- {plain.osdw_logical_error_rate_eb:.3e}; weight_mean {sim.weight_mean:.4f}, effective "
          f"sample fraction {sim.effective_sample_fraction:.3f}")
    assert eb > 0 and abs(rate - exact) <= 4 * eb
    assert abs(sim.weight_mean - 1) < 0.05 and 0 < sim.effective_sample_fraction < 1  # (the mean of 16384 weights of variance < 1)
    assert sim.run_count == wc.EXACT_SHOTS and sim.osdw_success_count < plain.osdw_success_count  # harsher shots, unweighted counts


def test_tilted_run_is_batch_size_independent():
    """16384 shots in one batch and in batches of 1000: the same per-shot log-weights and flags, the same counters; the float
    sums are added in another order."""
    H, L, p = wc.exact_model()
    parts = {"logw": [], "flags": []}
    small = wc.oracle_sim(H, L, p, wc.EXACT_SHOTS, seed=5, batch_size=1000, sample_scale=4, run_sim=False)
    while small.run_count < small.target_runs:
        small._run_batch_numpy(min(1000, small.target_runs - small.run_count))
        for k in parts:
            parts[k].append(small.last_batch(k))
    one = wc.oracle_sim(H, L, p, wc.EXACT_SHOTS, seed=5, sample_scale=4)
    for k, rows in parts.items():
        assert (np.concatenate(rows) == one.last_batch(k)).all(), k
    assert one.last_batch("logw").any()
    for c in dc.COUNTS:
        assert getattr(one, c) == getattr(small, c), c
    for k in wc.WEIGHT_RESULTS:
        assert getattr(small, k) == pytest.approx(getattr(one, k), rel=1e-12), k
    for k, v in one._wsum.items():
        assert small._wsum[k] == pytest.approx(v, rel=1e-12), k
