"""Fault sets of a fixed weight in the library's detector-error-model engine on the MI355X (bposd_dem_set_subset,
dem_subset_kernel, dem_decode_sim(engine="native", fault_weight=..., subset=...)): the sampler alone against the host
definition ``fault_subsets`` bit for bit -- items 0-2 and the integer log-weights -- at the shapes where it can go wrong,
whole runs against engine="numpy" on the CPU oracle, and what the C-ABI refuses.  Tables and references:
tests/subset_cases.py."""
import math

import numpy as np
import pytest

from tests import dem_cases as dc
from tests import dem_weight_cases as wc
from tests import subset_cases as sc

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


def _check(eng, ref, what=""):
    for k in ("faults", "detectors", "observables") + (("logw",) if "logw" in ref else ()):
        _rows_equal(eng.fetch(k), ref[k], f"{k} {what}")


def _sample_and_check(eng, H, L, support, mode, w, first, B, incr):
    assert eng.set_subset(mode, w, support, incr) == 0, eng.error()
    assert eng.sample(first, B) == 0, eng.error()
    ref = sc.reference(H, L, support, mode, w, first, B, incr)
    _check(eng, ref, f"({mode}, w = {w}, first shot {first})")
    return ref


def test_smallest_model(gpu_ready):
    """N = 1: the empty set and the one fault, in both modes."""
    H, L, p = dc.random_model(1, 1, 1)
    eng = sc.Engine(gpu_ready, H, L, p, capacity=70, seed=sc.SEED)
    for mode in sc.MODES:
        ref = _sample_and_check(eng, H, L, None, mode, 0, 0, 1 if mode == "enumerate" else 70, [-5])
        assert not ref["fault_bits"].any() and not ref["logw"].any()
        ref = _sample_and_check(eng, H, L, None, mode, 1, 0, 1 if mode == "enumerate" else 70, [-5])
        assert ref["fault_bits"].all() and (ref["logw"] == -5).all()
    eng.close()


def test_every_fault_at_once(gpu_ready):
    """N = 64, w = 64: one set, all 64 lanes hold an element, in both modes."""
    H, L, p = dc.random_model(64, 33, 2)
    incr = sc.increments(64)
    eng = sc.Engine(gpu_ready, H, L, p, capacity=300, seed=sc.SEED)
    ref = _sample_and_check(eng, H, L, None, "enumerate", 64, 0, 1, incr)
    assert ref["fault_bits"].all() and ref["logw"][0] == int(incr.sum())
    assert eng.sample(1, 1) == -1 and "only 1 sets" in eng.error()
    ref = _sample_and_check(eng, H, L, None, "random", 64, 2 ** 33, 300, incr)
    assert ref["fault_bits"].all()
    eng.close()


def test_all_pairs_in_one_call(gpu_ready):
    """N = 129, M = 65, k = 65, w = 2 enumerated whole: B = 8256 is 2064 workgroups of four shots, more than the grid of 2048 --
    a grid-stride with a tail -- and the fault, detector and observable rows all cross a word boundary.  Every pair appears
    exactly once."""
    H, L, p = dc.random_model(129, 65, 65)
    B = math.comb(129, 2)
    assert B == 8256
    incr = sc.increments(129)
    eng = sc.Engine(gpu_ready, H, L, p, capacity=B, seed=sc.SEED)
    ref = _sample_and_check(eng, H, L, None, "enumerate", 2, 0, B, incr)
    assert (ref["logw"] < 0).any() and (ref["logw"] > 2 ** 32).any() and ((ref["logw"] & (2 ** 32 - 1)) != 0).any()
    f = dc.unpack(eng.fetch("faults"), 129)
    assert (f.sum(axis=1) == 2).all() and np.unique(f, axis=0).shape[0] == B
    assert ref["fault_bits"][:, 128].any() and ref["detectors"][:, 1].any() and ref["observables"][:, 1].any()
    eng.close()


def test_ranks_beyond_32_bits_and_the_end_of_a_stratum(gpu_ready):
    """N = 1031, w = 4, C = 4.7e10: ranks from 2^32 + 12345 on, the last B ranks ending at C - 1, and a batch that ends past C - 1
    refused."""
    from bp_osd_amd import _lib

    H, L, p = dc.random_model(1031, 130, 3)
    B, C = 8209, math.comb(1031, 4)
    assert C > 2 ** 35
    incr = sc.increments(1031)
    eng = sc.Engine(gpu_ready, H, L, p, capacity=B, seed=sc.SEED)
    _sample_and_check(eng, H, L, None, "enumerate", 4, 2 ** 32 + 12345, B, incr)
    last = _sample_and_check(eng, H, L, None, "enumerate", 4, C - B, B, incr)
    assert np.flatnonzero(last["fault_bits"][-1]).tolist() == [1027, 1028, 1029, 1030]
    for first, rows in ((C - B + 1, B), (C, 1), (2 ** 64 - 1, 2)):
        assert eng.sample(first, rows) == _lib.BPOSD_ERR_INVALID and "sets of weight 4" in eng.error(), (first, rows)
    assert eng.sample(C - 1, 1) == 0, eng.error()
    _rows_equal(eng.fetch("faults"), last["faults"][-1:], "the last rank alone")
    eng.close()


def test_sixty_four_of_128_drawn(gpu_ready):
    """N = 128, w = 64 drawn, B = 8209: every lane busy in Floyd's resolve, two fault words, sums of 64 increments."""
    H, L, p = dc.random_model(128, 64, 64)
    eng = sc.Engine(gpu_ready, H, L, p, capacity=8209, seed=sc.SEED)
    ref = _sample_and_check(eng, H, L, None, "random", 64, 2 ** 32 - 100, 8209, sc.increments(128))
    assert np.unique(ref["logw"]).size > 1000 and (ref["logw"] < 0).any() and (ref["logw"] > 0).any()
    eng.close()


def test_collisions(gpu_ready):
    """N = 8, w = 7 drawn: nearly every step of Floyd's algorithm meets an element it has already taken."""
    H, L, p = dc.random_model(8, 5, 2)
    eng = sc.Engine(gpu_ready, H, L, p, capacity=1000, seed=sc.SEED)
    ref = _sample_and_check(eng, H, L, None, "random", 7, 0, 1000, sc.increments(8))
    assert np.unique(ref["faults"]).size == 8  # every one of the 8 sets is drawn
    eng.close()


@pytest.mark.parametrize("mode", list(sc.MODES))
def test_support_maps_positions_to_faults(gpu_ready, mode):
    """A support that skips the 0- and 1-priors of random_model (n < N), with the empty, the observable-only and the heavy
    column in it; w = 3; without increments item 10 is refused."""
    from bp_osd_amd import _lib

    H, L, p = dc.random_model(129, 65, 65)
    sup = sc.interior_support(129, 65, 65)
    B = 4099
    eng = sc.Engine(gpu_ready, H, L, p, capacity=B, seed=sc.SEED)
    ref = _sample_and_check(eng, H, L, sup, mode, 3, 5, B, sc.increments(129))
    outside = np.setdiff1d(np.arange(129), sup)
    assert outside.size and not ref["fault_bits"][:, outside].any()
    for special in (dc.EMPTY_FAULT, dc.OBS_ONLY_FAULT, dc.HEAVY_FAULT):
        assert ref["fault_bits"][:, special].any()
    assert eng.set_subset(mode, 3, sup, None) == 0, eng.error()
    assert eng.sample(5, B) == 0, eng.error()
    _check(eng, {k: ref[k] for k in ("faults", "detectors", "observables")}, "without increments")
    rc, _ = eng.fetch_rc("logw")
    assert rc == _lib.BPOSD_ERR_INVALID and "increment" in eng.error()
    eng.close()


@pytest.mark.parametrize("mode", list(sc.MODES))
def test_batch_independence(gpu_ready, mode):
    """One call against the same shots in three unequal calls."""
    H, L, p = dc.random_model(129, 65, 65)
    incr = sc.increments(129)
    B = 3000
    first = 2 ** 32 - 1000 if mode == "random" else math.comb(129, 3) - B - 17  # (across 2^32; near the end of the stratum)
    eng = sc.Engine(gpu_ready, H, L, p, capacity=B, seed=sc.SEED)
    ref = _sample_and_check(eng, H, L, None, mode, 3, first, B, incr)
    at = 0
    for part in (1, 2047, 952):
        assert eng.sample(first + at, part) == 0, eng.error()
        _check(eng, {k: v[at:at + part] for k, v in ref.items()}, f"rows {at} .. {at + part}")
        at += part
    assert at == B
    eng.close()


def test_refusals_leave_the_engine_as_it_was(gpu_ready):
    """Every refusal of bposd_dem_set_subset: BPOSD_ERR_INVALID with a message that names the culprit, and the engine samples
    on in the mode it was in -- Bernoulli rows before the first switch, the stratum it had after it."""
    from bp_osd_amd import _lib

    c = dc.SAMPLER_BY_ID["127-63-1"]
    H, L, p = dc.random_model(c["N"], c["M"], c["k"])
    N, B = c["N"], 300
    incr = sc.increments(N)
    q, tilt, _ = wc.tilted_tables(c["id"])
    eng = sc.Engine(gpu_ready, H, L, p, capacity=B, seed=sc.SEED)
    INV = _lib.BPOSD_ERR_INVALID

    def refusals():
        for mode in (3, -1, 99):
            assert eng.set_subset(mode, 2, None, incr) == INV and f"mode = {mode}" in eng.error()
        for w in (-1, 65, 128):
            assert eng.set_subset("random", w, None, incr) == INV and f"weight = {w}" in eng.error()
        assert eng.set_subset("random", 5, [1, 2, 3, 4], incr) == INV and "weight = 5" in eng.error()  # w > n
        for sup, word in (([0, 5, 5, 9], "support[2] = 5"), ([0, 7, 6, 9], "support[2] = 6"), ([0, 5, 127], "support[2] = 127"), ([-1, 5, 9], "support[0] = -1")):
            assert eng.set_subset("random", 2, sup, incr) == INV and word in eng.error(), sup
        assert eng.set_subset("random", 2, [0, 1], incr, n_support=-1) == INV and "n_support" in eng.error()
        assert eng.set_subset("random", 2, [0, 1], incr, n_support=N + 1) == INV and "n_support" in eng.error()
        assert eng.set_subset("enumerate", 60, None, incr) == INV and "C(127, 60)" in eng.error()  # 1.2e37
        for big, w in ((2 ** 62, 1), (-2 ** 63, 1), (2 ** 61, 2), (-2 ** 61, 2), (2 ** 56, 64)):
            ii = incr.copy()
            ii[9] = big
            assert eng.set_subset("random", w, None, ii) == INV and "fault 9" in eng.error() and "2^62" in eng.error(), (big, w)
        ii = incr.copy()
        ii[9] = 2 ** 61 - 1  # 2 (2^61 - 1) < 2^62: the largest that passes at w = 2; and a fault outside the support is not held against it
        return ii

    refusals()  # in plain mode
    assert eng.sample(0, B) == 0, eng.error()
    from bp_osd_amd.sim import philox_uniforms

    plain = dc.pack((philox_uniforms(sc.SEED, 0, B, N) < p).astype(np.uint8))
    assert (eng.fetch("faults") == plain).all() and eng.fetch_rc("logw")[0] == INV

    before = eng.device_bytes()
    sup = np.arange(3, 120, dtype=np.int32)
    assert eng.set_subset("enumerate", 3, sup, incr) == 0, eng.error()
    grown = eng.device_bytes()
    assert grown >= before + 8 * 3 * (sup.size + 1) + 8 * N + 4 * sup.size + 8 * B  # binomials, increments, support, log-weights
    largest = refusals()  # in subset mode
    assert eng.set_sampling(q, tilt) == INV and "bposd_dem_set_subset" in eng.error()  # one off first
    assert eng.set_sampling(None, None) == 0
    assert eng.sample(7, B) == 0, eng.error()
    _check(eng, sc.reference(H, L, sup, "enumerate", 3, 7, B, incr), "after the refusals")

    assert eng.set_subset("random", 2, None, largest) == 0, eng.error()
    assert eng.fetch_rc("logw")[0] == INV  # the batch at hand was summed from the table that went
    assert eng.sample(0, B) == 0, eng.error()
    _check(eng, sc.reference(H, L, None, "random", 2, 0, B, largest), "the largest increment")
    big = np.zeros(N, np.int64)
    big[9] = 2 ** 62
    assert eng.set_subset("random", 2, [0, 1, 2], big) == 0, eng.error()  # fault 9 is outside the support
    assert eng.device_bytes() < grown  # the block was replaced, not added to

    # and the other way round: weighted sampling on refuses the subset switch
    assert eng.set_subset(None, 0) == 0
    assert eng.set_sampling(q, tilt) == 0, eng.error()
    assert eng.set_subset("random", 2, None, incr) == INV and "bposd_dem_set_sampling" in eng.error()
    assert eng.sample(0, B) == 0, eng.error()
    assert (eng.fetch("faults") == dc.pack((philox_uniforms(sc.SEED, 0, B, N) < q).astype(np.uint8))).all()
    eng.close()


def test_switching_off_restores_the_bernoulli_rows(gpu_ready):
    from bp_osd_amd import _lib

    c = dc.SAMPLER_BY_ID["127-63-1"]
    H, L, p = dc.random_model(c["N"], c["M"], c["k"])
    eng = sc.Engine(gpu_ready, H, L, p, capacity=c["B"], seed=sc.SEED)
    _sample_and_check(eng, H, L, None, "random", 5, c["first_shot"], c["B"], sc.increments(c["N"]))
    assert eng.set_subset(None, 0) == 0, eng.error()
    rc, _ = eng.fetch_rc("logw")
    assert rc == _lib.BPOSD_ERR_INVALID
    assert eng.sample(c["first_shot"], c["B"]) == 0, eng.error()
    ref = dc.sampler_reference(c["id"])
    for k in ("faults", "detectors", "observables"):
        _rows_equal(eng.fetch(k), ref[k], k + " (Bernoulli again)")
    rc, _ = eng.fetch_rc("logw")
    assert rc == _lib.BPOSD_ERR_INVALID and "weighted sampling" in eng.error()
    eng.close()


# --------------------------------------------------------------------------------------------------- whole runs
def _native(H, L, priors, w, subset, batch_size=4096, **kw):
    from bp_osd_amd import dem_decode_sim

    return dem_decode_sim(H, L, priors, batch_size=batch_size, engine="native", seed=dc.RUN_SEED, fault_weight=w, subset=subset, **dict(dc.DECODER, **kw))


def test_native_strata_of_the_exact_model_equal_the_oracle(gpu_ready):
    """exact_model, every stratum enumerated on the device: counters, per-shot items, sums and failure masses equal those of
    engine="numpy" on the CPU oracle exactly, and so their sum meets exact_osdw_rate(); dem_failure_spectrum on top."""
    from bp_osd_amd import dem_failure_spectrum

    H, L, p = wc.exact_model()
    ref = sc.exact_strata()
    total = 0.0
    for w in range(14):
        got = sc.snapshot(_native(H, L, p, w, "enumerate", batch_size=500))
        sc.assert_same_run(got, ref[w])
        total += got["osdw_failure_mass"]
    exact = wc.exact_osdw_rate()
    print("sum of the strata on the device", total, "exact", exact)
    assert abs(total - exact) <= sc.EXACT_REL * exact
    sp = dem_failure_spectrum(H, L, p, 4, 300, engine="native", seed=dc.RUN_SEED, **dc.DECODER)
    assert sp["corrected_weight"] == 1 and sp["min_failing_weight"] == 2
    assert [r["osdw_failures"] for r in sp["strata"][:4]] == list(sc.EXACT_FAILING)
    assert [r["osdw_failure_mass"] for r in sp["strata"][:4]] == [s["osdw_failure_mass"] for s in ref[:4]]


@pytest.mark.parametrize("batch_size", [4096, 1000])
def test_native_pairs_of_surface13_equal_the_oracle(gpu_ready, batch_size):
    """surface13-R3 (24 x 70), all 2415 pairs: as one batch, and as batches of 1000 with a clamped last one."""
    H, L, p = dc.run_model("surface13-R3")
    ref = sc.surface_pairs(batch_size)
    assert ref["run_count"] == 2415 and 0 < ref["osdw_success_count"] and ref["osdw_failure_mass_eb"] == 0.0
    got = sc.snapshot(_native(H, L, p, 2, "enumerate", batch_size=batch_size))
    print(batch_size, {k: got[k] for k in dc.COUNTS + sc.STRATUM_RESULTS})
    sc.assert_same_run(got, ref)


@pytest.mark.parametrize("w", [6, 30])
def test_native_drawn_sets_with_a_harvest_equal_the_oracle(gpu_ready, w):
    """hgp400-R1 (384 x 992, k = 16), sets of weight 6 and 30 drawn, one batch of 128, harvest = 8: the harvest composes
    unchanged.  All 128 sets of weight 6 are corrected; of weight 30, bp fails on most and osdw on three, which the harvest
    keeps with their log-weights."""
    H, L, p = dc.run_model("hgp400-R1")
    ref = sc.hgp_random(w)
    assert ref["run_count"] == 128 and ref["failures_logw"].size == ref["failures_shot"].size
    if w == 30:
        assert ref["failures_shot"].size == 3 and ref["osdw_failure_mass_eb"] > 0 and ref["bp_success_count"] < 64
    got = sc.snapshot(_native(H, L, p, w, "random", batch_size=128, target_runs=128, harvest=8))
    print(w, {k: got[k] for k in dc.COUNTS + sc.STRATUM_RESULTS})
    sc.assert_same_run(got, ref)
