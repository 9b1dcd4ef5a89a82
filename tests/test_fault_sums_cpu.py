"""Per-fault sums over selected shots and the cross-entropy fit of a sampling row on the host: the package's
restatement against dense integer arithmetic on every kernel case, the multipliers, the refusals, ``fault_stats`` on the
oracle engine against the fetched rows, and the fit on the model whose logical error rate is known exactly.  No GPU: the
harness runs ``engine="numpy"`` around the CPU oracle.  Shapes, rows and references: tests/fault_sums_cases.py."""
import os
import re

import numpy as np
import pytest

from tests import dem_cases as dc
from tests import dem_weight_cases as wc
from tests import fault_sums_cases as fc


def _oracle_sim(**kw):
    from bp_osd_amd.dem import dem_decode_sim
    from oracle import OracleDecoder

    H, L, p = wc.exact_model()
    opts = dict(batch_size=64, engine="numpy", seed=1, target_runs=64, decoder_factory=OracleDecoder, run_sim=False)
    opts.update(dc.DECODER)
    opts.update(kw)
    return dem_decode_sim(H, L, p, **opts)


# ------------------------------------------------------------------------------------------------------------ the statistic
def test_the_tile_constant_is_the_kernels():
    src = open(os.path.join(dc.ROOT, "bp_osd_amd", "csrc", "fault_sums_kernel.hip.h")).read()
    words = int(re.search(r"constexpr int FS_TILE_WORDS = (\d+);", src).group(1))
    assert re.search(r"constexpr int FS_TILE_COLS = 64 \* FS_TILE_WORDS;", src) and 64 * words == fc.TILE_COLS
    lds = 4 * fc.TILE_COLS + 8 * fc.TILE_COLS  # 32-bit counts and 64-bit sums
    assert lds <= 64 * 1024


@pytest.mark.parametrize("form", ["listed", "all"])
@pytest.mark.parametrize("case", fc.KERNEL_CASES, ids=[c["id"] for c in fc.KERNEL_CASES])
def test_restatement_equals_dense_integer_sums(case, form):
    from bp_osd_amd._dem_base import fault_sums_batch

    faults, select, mult = fc.kernel_rows(case["id"])
    rows, counts, sums = fc.kernel_reference(case["id"], form)
    _case_shows_what_it_is_for(case, form, rows, counts, sums)
    got_c, got_s = fault_sums_batch(dc.pack(faults), rows, mult[rows], case["N"])
    assert got_c.dtype == got_s.dtype == np.uint64 and got_c.shape == got_s.shape == (case["N"],)
    assert (got_c == counts).all() and (got_s == sums).all()
    only_c, none = fault_sums_batch(dc.pack(faults), rows, None, case["N"])
    assert none is None and (only_c == counts).all()
    # every split of the row list adds up to the same arrays
    cut = rows.size // 3
    a, b = fault_sums_batch(dc.pack(faults), rows[:cut], mult[rows[:cut]], case["N"]), fault_sums_batch(dc.pack(faults), rows[cut:], mult[rows[cut:]], case["N"])
    assert (a[0] + b[0] == counts).all() and (a[1] + b[1] == sums).all()


def _case_shows_what_it_is_for(case, form, rows, counts, sums):
    """Each case's condition on the reference alone."""
    faults, select, mult = fc.kernel_rows(case["id"])
    B = case["B"]
    if form == "all" or case["select"] == "all":
        assert rows.size == B
    elif case["select"] == "none":
        assert rows.size == 0 and not counts.any() and not sums.any()
    elif case["select"] == "one":
        assert rows.size == 1
    else:
        assert 1 < rows.size < B
    if case.get("ends") and form == "listed":
        assert rows[0] == 0 and rows[-1] == B - 1
    if rows.size >= fc.ONES_ROWS:
        full = faults[rows].all(axis=1)
        assert (mult[rows][full] == fc.MULT_MAX).sum() >= 5 and int(sums.max()) > 2 ** 32  # a column sum crosses 2^32
        if case["rows"] == "sparse":
            assert (~faults[rows].any(axis=1)).sum() >= 3 and set(fc.MULT_VALUES) <= set(mult[rows].tolist())
    if case["rows"] == "ones" and rows.size:
        assert (counts == rows.size).all() and (sums == rows.size * fc.MULT_MAX).all()
    assert int(sums.max(initial=0)) < 2 ** 63


def test_restatement_refuses_what_it_cannot_sum():
    from bp_osd_amd._dem_base import fault_sums_batch

    words = np.zeros((4, 2), np.uint64)
    for rows in ([2, 1], [1, 1], [-1], [4]):
        with pytest.raises(ValueError, match="ascend"):
            fault_sums_batch(words, rows)
    with pytest.raises(ValueError, match="multipliers"):
        fault_sums_batch(words, [0, 1], [1])
    with pytest.raises(ValueError, match="multipliers"):
        fault_sums_batch(words, [0], [2 ** 32])
    with pytest.raises(ValueError, match="multipliers"):
        fault_sums_batch(words, [0], [0.5])
    with pytest.raises(ValueError, match="N = 64"):
        fault_sums_batch(words, [0], None, 64)


def test_weight_multipliers():
    from bp_osd_amd.dem import LOGW_ONE, weight_multipliers

    lw = np.array([-3 * LOGW_ONE, 5 * LOGW_ONE, 5 * LOGW_ONE - 1, 4 * LOGW_ONE, -40 * LOGW_ONE], np.int64)
    v = weight_multipliers(lw)
    assert v.dtype == np.uint32 and v.shape == (5,)
    assert v[1] == 2 ** 31 - 1 == v.max()  # the largest log-weight
    assert v[3] == int(np.rint(np.exp(-1.0) * (2 ** 31 - 1))) and v[4] == 0
    assert v[0] == int(np.rint(np.exp(-8.0) * (2 ** 31 - 1)))
    assert (weight_multipliers(lw + 7 * LOGW_ONE) == v).all()  # only differences count
    one = weight_multipliers(np.array([-(2 ** 61)], np.int64))
    assert one.dtype == np.uint32 and one.tolist() == [2 ** 31 - 1]
    none = weight_multipliers(np.zeros(0, np.int64))
    assert none.dtype == np.uint32 and none.shape == (0,)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_fault_stats_needs_the_harvest():
    with pytest.raises(ValueError, match="harvest"):
        _oracle_sim(fault_stats=True)
    off = _oracle_sim(harvest=2)
    assert off.fault_counts is None and off.failure_fault_counts is None
    on = _oracle_sim(harvest=2, fault_stats=True)
    assert on.fault_counts.dtype == on.failure_fault_counts.dtype == np.int64 and not on.fault_counts.any()


def test_fault_sums_refusals():
    sim = _oracle_sim(harvest=2)
    with pytest.raises(RuntimeError, match="batch"):
        sim.fault_sums("all")
    sim.run_decode_sim()
    with pytest.raises(ValueError, match="select"):
        sim.fault_sums("some")
    with pytest.raises(ValueError, match="multipliers"):
        sim.fault_sums("all", np.ones(63, np.uint32))
    with pytest.raises(ValueError, match="2\\^32"):
        sim.fault_sums("all", np.full(64, 2 ** 32, np.uint64))
    with pytest.raises(ValueError, match="2\\^32"):
        sim.fault_sums("all", np.full(64, 0.5))
    with pytest.raises(ValueError, match="harvest"):
        _oracle_sim().fault_sums("failing")
    counts, sums = sim.fault_sums("all", np.full(64, 3, np.uint32))
    assert sums is not None and (sums == 3 * counts).all()
    assert (counts.astype(np.int64) == dc.unpack(sim.last_batch("faults"), sim.N).sum(axis=0)).all()


def test_set_sampling_refusals_and_reset():
    H, L, p = wc.exact_model()
    sim = _oracle_sim(harvest=2, fault_stats=True, sample_scale=4)
    sim.run_decode_sim()
    assert sim.run_count == 64 and sim.fault_counts.any()
    was = (sim._sample_priors.copy(), sim._incr.copy(), sim._c0, sim.run_count)
    for bad, why in ((dict(sample_priors=np.full(12, 0.1)), "length 13"), (dict(sample_priors=np.full(13, 0.1), nominal=np.full(3, 0.1)), "length 13"),
                     (dict(sample_priors=np.full(13, 0.1), first_shot=-1), "first_shot"), (dict(sample_priors=np.full(13, 1.5)), "not a probability"),
                     (dict(sample_priors=np.zeros(13)), "unbounded")):
        with pytest.raises(ValueError, match=why):
            sim.set_sampling(**bad)
    assert (sim._sample_priors == was[0]).all() and (sim._incr == was[1]).all() and (sim._c0, sim.run_count) == was[2:]  # a refusal changes nothing
    q, nominal = np.minimum(6 * p, 0.5), np.minimum(2 * p, 0.5)
    sim.set_sampling(q, nominal=nominal, target_runs=32, first_shot=5 << 40)
    from bp_osd_amd.dem import importance_table

    incr, c0 = importance_table(nominal, q)
    assert (sim._incr == incr).all() and sim._c0 == c0 and sim.sample_scale is None
    assert sim.run_count == 0 and sim.target_runs == 32 and not sim.fault_counts.any() and sim.failures["shot"].size == 0 and sim._wsum["w"] == 0.0
    sim.run_decode_sim()
    from bp_osd_amd.sim import philox_uniforms

    drawn = (philox_uniforms(sim.seed, 5 << 40, 32, 13) < q).astype(np.uint8)
    assert (dc.unpack(sim.last_batch("faults"), 13) == drawn).all() and (sim.last_batch("logw") == drawn.astype(np.int64) @ incr).all()
    # an untilted sim can be tilted; a sim of fault sets of a fixed weight cannot
    plain = _oracle_sim(harvest=1)
    plain.set_sampling(q)
    plain.run_decode_sim()
    assert "logw" in plain.failures and plain.weight_mean > 0
    with pytest.raises(ValueError, match="fixed weight"):
        _oracle_sim(fault_weight=1, subset="enumerate", target_runs=13).set_sampling(q)


def test_fit_sample_priors_refusals():
    from bp_osd_amd.dem import fit_sample_priors
    from oracle import OracleDecoder

    H, L, p = wc.exact_model()
    fit = lambda **kw: fit_sample_priors(H, L, p, **dict(dict(engine="numpy", decoder_factory=OracleDecoder, shots_per_level=256, batch_size=256, **dc.DECODER), **kw))
    for bad, why in ((dict(levels=(8.0, 2.0)), "last level must be 1"), (dict(levels=()), "non-empty"), (dict(levels=(0.5, 1.0)), ">= 1"),
                     (dict(smoothing=0.0), "smoothing"), (dict(smoothing=1.5), "smoothing"), (dict(shots_per_level=0), "shots_per_level"),
                     (dict(min_failures=0), "min_failures"), (dict(harvest=3), "sets harvest itself"), (dict(sample_scale=2), "sets sample_scale itself")):
        with pytest.raises(ValueError, match=why):
            fit(**bad)
    with pytest.raises(ValueError, match=r"level 0 \(scale 1\).*larger first scale") as e:  # too few failures at the true priors
        fit(levels=(1.0,))
    assert "min_failures = 32" in str(e.value)
    with pytest.raises(ValueError, match="not a probability"):
        fit_sample_priors(H, L, np.full(13, 1.5), engine="numpy", decoder_factory=OracleDecoder)


# ------------------------------------------------------------------------------------------------------------ fault_stats
@pytest.mark.parametrize("case_id", [c["id"] for c in dc.RUN_CASES])
def test_fault_stats_equal_the_column_sums_of_the_fetched_rows(case_id):
    ref = fc.stats_reference(case_id)
    assert ref["failures"] == dc.RUN_BY_ID[case_id]["oracle"]["wrong"][2] > 0
    assert (ref["fault_counts"] == ref["from_rows"]).all() and (ref["failure_fault_counts"] == ref["from_failing_rows"]).all()
    assert ref["fault_counts"].dtype == np.int64 and 0 < ref["failure_fault_counts"].sum() < ref["fault_counts"].sum()


@pytest.mark.parametrize("case_id", ["surface13-R3", "hgp400-R1"])
def test_fault_stats_do_not_depend_on_the_batch_size(case_id):
    ref = fc.stats_reference(case_id)
    sim = fc.stats_sim(case_id, "numpy", run_sim=False)
    out = sim.output_dict()
    for B in fc.split_sizes(dc.RUN_BY_ID[case_id]["B"]):
        sim._run_batch_numpy(B)
    assert sim.run_count == dc.RUN_BY_ID[case_id]["B"]
    assert (sim.fault_counts == ref["fault_counts"]).all() and (sim.failure_fault_counts == ref["failure_fault_counts"]).all()
    assert "fault_counts" not in out and "fault_counts" not in sim.output_dict()  # output_dict is unchanged


# ---------------------------------------------------------------------------------------------------------------- the fit
@pytest.mark.parametrize("seed", wc.EXACT_SEEDS)
def test_fitted_row_on_the_exact_model(seed):
    """fit_sample_priors with its default arguments on exact_model(), oracle engine, then EXACT_SHOTS shots with the fitted
    row: the estimate lies within 4 of its own error bars of the exact rate, its error bar is no larger than that of
    sample_scale=8 on the same seed, and weight_mean is within 5 % of 1."""
    H, L, p = wc.exact_model()
    exact = wc.exact_osdw_rate()
    q, report = fc.oracle_fit(seed)
    assert q.shape == (13,) and ((q >= p) & (q <= 0.5)).all()  # a legal sample_priors, never below the model
    assert [r["level"] for r in report] == [0, 1, 2] and [r["scale"] for r in report] == [8.0, 1.0, 1.0]
    assert all(r["failures"] >= 32 and r["shots"] == 4096 and 0 < r["effective_sample_fraction"] <= 1 for r in report)
    assert (report[-1]["sample_priors"] == q).all()
    fitted = wc.oracle_sim(H, L, p, wc.EXACT_SHOTS, seed=seed, batch_size=4096, sample_priors=q)
    scale8 = wc.oracle_sim(H, L, p, wc.EXACT_SHOTS, seed=seed, batch_size=4096, sample_scale=8)
    rate, eb = fitted.osdw_logical_error_rate, fitted.osdw_logical_error_rate_eb
    print(f"seed {seed}: fitted {rate:.6e} +- {eb:.3e} ({(rate - exact) / eb:+.2f} eb from exact {exact:.6e}), sample_scale=8 eb "
          f"{scale8.osdw_logical_error_rate_eb:.3e}, weight_mean {fitted.weight_mean:.4f}, effective sample fraction "
          f"{fitted.effective_sample_fraction:.3f}, q {np.round(q, 3).tolist()}")
    assert abs(rate - exact) <= 4 * eb
    assert eb <= scale8.osdw_logical_error_rate_eb
    assert abs(fitted.weight_mean - 1) <= 0.05


def test_the_fit_does_not_touch_faults_outside_0_to_half():
    from bp_osd_amd.dem import fit_sample_priors
    from oracle import OracleDecoder

    H, L, p = wc.exact_model()
    p = p.copy()
    p[9], p[11] = 0.0, 0.6
    q, _ = fit_sample_priors(H, L, p, levels=(8.0, 1.0), shots_per_level=1024, batch_size=512, engine="numpy", seed=3, smoothing=0.5,
                             decoder_factory=OracleDecoder, **dc.DECODER)
    assert q[9] == 0.0 and q[11] == 0.6 and ((q >= p) & (q <= np.maximum(p, 0.5))).all()
