"""Importance sampling in the library's detector-error-model engine on the MI355X (bposd_dem_set_sampling, item
BPOSD_DEM_LOGW, dem_decode_sim(engine="native", sample_priors=... / sample_scale=...)): the weighted sampler against the
host draw and the integer product ``faults @ incr`` bit for bit, whole runs against engine="numpy" on the CPU oracle, the
neutral case, and what the C-ABI refuses.  Tables and references: tests/dem_weight_cases.py."""
import numpy as np
import pytest

from tests import dem_cases as dc
from tests import dem_weight_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


def _rows_equal(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    bad = np.flatnonzero((got != ref).reshape(len(got), -1).any(axis=1))
    assert bad.size == 0, f"{what} differs from the host in {bad.size} shots, first {bad[:5]}"


@pytest.mark.parametrize("case", dc.SAMPLER_CASES, ids=[c["id"] for c in dc.SAMPLER_CASES])
def test_weighted_sampler_equals_host_draw(gpu_ready, case):
    """dem_sample_kernel<true> alone: the rows are those of the host draw against q, logw = fault_bits @ incr exactly -- with
    the table of importance_table, and with increments chosen so that sums carry across the 32-bit halves and go negative.
    Switched off again, the engine gives the plain reference and refuses the item."""
    from bp_osd_amd import _lib

    H, L, priors = dc.random_model(case["N"], case["M"], case["k"])
    B, first = case["B"], case["first_shot"]
    q, incr, arbitrary = wc.tilted_tables(case["id"])
    ref = wc.tilted_sampler_reference(case["id"])
    if case["N"] >= 4:  # the reference is not degenerate: q differs from p, and the arbitrary sums need their high words
        assert (q != priors).any() and incr.any() and (ref["fault_bits"] != dc.sampler_reference(case["id"])["fault_bits"]).any()
        assert (ref["logw_arbitrary"] < 0).any() and (ref["logw_arbitrary"] > 2 ** 32).any()
        assert ((ref["logw_arbitrary"] & (2 ** 32 - 1)) != 0).any()

    eng = wc.Engine(gpu_ready, H, L, priors, capacity=B + 3, seed=dc.SAMPLER_SEED)
    before = eng.device_bytes()
    assert eng.set_sampling(q, incr) == 0, eng.error()
    assert eng.device_bytes() >= before + 8 * (B + 3) + 16 * case["N"]
    grown = eng.device_bytes()
    assert eng.sample(first, B) == 0, eng.error()
    for k in ("faults", "detectors", "observables", "logw"):
        _rows_equal(eng.fetch(k), ref[k], k)

    assert eng.set_sampling(q, arbitrary) == 0, eng.error()
    assert eng.device_bytes() == grown  # allocated once
    assert eng.fetch_rc("logw")[0] == _lib.BPOSD_ERR_INVALID  # the batch at hand was summed from the other table
    assert eng.sample(first, B) == 0, eng.error()
    _rows_equal(eng.fetch("logw"), ref["logw_arbitrary"], "logw of the arbitrary table")
    _rows_equal(eng.fetch("faults"), ref["faults"], "faults")

    assert eng.set_sampling(None, None) == 0, eng.error()
    assert eng.sample(first, B) == 0, eng.error()
    plain = dc.sampler_reference(case["id"])
    for k in ("faults", "detectors", "observables"):
        _rows_equal(eng.fetch(k), plain[k], k + " (plain again)")
    rc, _ = eng.fetch_rc("logw")
    assert rc == _lib.BPOSD_ERR_INVALID and "weighted sampling" in eng.error()
    eng.close()


def _native(H, L, priors, B, **kw):
    from bp_osd_amd import dem_decode_sim

    return dem_decode_sim(H, L, priors, batch_size=B, engine="native", seed=dc.RUN_SEED, target_runs=B, **dict(dc.DECODER, **kw))


@pytest.mark.parametrize("case_id", ["surface13-R3", "hgp400-R1"])
def test_tilted_native_run_equals_oracle_run(gpu_ready, case_id):
    """sample_scale = 3, one batch, the same seed: counters, per-shot flags, convergence and log-weights, the weighted sums and
    every reported figure equal those of engine="numpy" on the CPU oracle -- exactly, since one helper sums equal arrays."""
    B = dc.RUN_BY_ID[case_id]["B"]
    ref = wc.tilted_run_reference(case_id)
    plain = dc.run_reference(case_id)
    # the reference is a tilted one: other shots than the plain run's, more of them wrong, weights that differ
    assert np.unique(ref["logw"]).size > 4 and ref["osdw_success_count"] < plain["osdw_success_count"]
    assert 0 < ref["osdw_logical_error_rate"] < 1 - ref["osdw_success_count"] / B and 0 < ref["effective_sample_fraction"] < 1

    H, L, priors = dc.run_model(case_id)
    got = wc.snapshot(_native(H, L, priors, B, sample_scale=wc.RUN_SCALE))
    print(case_id, {k: got[k] for k in dc.COUNTS + wc.WEIGHT_RESULTS})
    for k in dc.COUNTS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in wc.WEIGHT_ITEMS:
        _rows_equal(got[k], ref[k], k)
    assert got["wsum"] == ref["wsum"]
    for k in wc.WEIGHT_RESULTS:
        assert got[k] == ref[k], (k, got[k], ref[k])


def test_native_sampling_from_the_priors_is_neutral(gpu_ready):
    """sample_priors = priors on the device: the counters and flags of the plain native run, log-weights all zero."""
    case = dc.RUN_BY_ID["surface13-R3"]
    H, L, priors = dc.run_model(case["id"])
    plain = _native(H, L, priors, case["B"])
    sim = _native(H, L, priors, case["B"], sample_priors=priors.copy())
    for k in dc.COUNTS:
        assert getattr(sim, k) == getattr(plain, k) == dc.run_reference(case["id"])[k], k
    assert (sim.last_batch("flags") == plain.last_batch("flags")).all()
    logw = sim.last_batch("logw")
    assert logw.shape == (case["B"],) and logw.dtype == np.int64 and not logw.any()
    assert sim.weight_mean == 1.0 and sim.osdw_logical_error_rate == plain.osdw_logical_error_rate
    with pytest.raises(ValueError, match="importance sampling"):
        plain.last_batch("logw")


def test_set_sampling_refusals_leave_the_engine_as_it_was(gpu_ready):
    """Through the raw C-ABI: q outside [0, 1] or NaN, one NULL pointer, sum |incr| >= 2^62 -- BPOSD_ERR_INVALID with a message,
    and the engine samples on in the mode it was in: plain before the first switch, weighted with the table it had after it."""
    from bp_osd_amd import _lib
    from bp_osd_amd.sim import philox_uniforms

    c = dc.SAMPLER_BY_ID["127-63-1"]
    H, L, priors = dc.random_model(c["N"], c["M"], c["k"])
    q, incr, _ = wc.tilted_tables(c["id"])
    B, N = 300, c["N"]
    u = philox_uniforms(dc.SAMPLER_SEED, 0, B, N)
    eng = wc.Engine(gpu_ready, H, L, priors, capacity=B, seed=dc.SAMPLER_SEED)
    two = np.flatnonzero((q > 0.2) & (q < 0.8))[:2]  # two faults that fire in some shots and not in others

    def refusals():
        for bad in (-0.1, 1.5, float("nan")):
            qq = q.copy()
            qq[9] = bad
            assert eng.set_sampling(qq, incr) == _lib.BPOSD_ERR_INVALID and "fault 9" in eng.error()
        assert eng.set_sampling(q, None) == _lib.BPOSD_ERR_INVALID and "both" in eng.error()
        assert eng.set_sampling(None, incr) == _lib.BPOSD_ERR_INVALID and "both" in eng.error()
        for big in ([2 ** 61, -2 ** 61], [2 ** 62, 0], [-2 ** 63, 0], [2 ** 63 - 1, 2 ** 63 - 1]):
            ii = incr.copy()
            ii[two] = big
            assert eng.set_sampling(q, ii) == _lib.BPOSD_ERR_INVALID and "2^62" in eng.error()
        ii = np.zeros(N, np.int64)
        ii[two] = [2 ** 61, -(2 ** 61 - 1)]  # sum |incr| = 2^62 - 1: the largest table that passes
        return ii

    refusals()  # in plain mode
    assert eng.sample(0, B) == 0, eng.error()
    assert (eng.fetch("faults") == dc.pack((u < priors).astype(np.uint8))).all()
    assert eng.fetch_rc("logw")[0] == _lib.BPOSD_ERR_INVALID

    assert eng.set_sampling(q, incr) == 0, eng.error()
    largest = refusals()  # in weighted mode
    assert eng.sample(0, B) == 0, eng.error()
    faults = (u < q).astype(np.uint8)
    assert (eng.fetch("faults") == dc.pack(faults)).all() and (eng.fetch("logw") == faults.astype(np.int64) @ incr).all()

    assert eng.set_sampling(q, largest) == 0, eng.error()
    assert eng.sample(0, B) == 0, eng.error()
    want = faults.astype(np.int64) @ largest
    assert {0, 1, 2 ** 61, -(2 ** 61 - 1)} == set(want.tolist())
    assert (eng.fetch("logw") == want).all()
    eng.close()
