"""The relay mode without a GPU: the numpy reference (bp_osd_amd/relay.py) against a scalar restatement of the definition
written here, the degenerate setting against the C oracle's min-sum, the coverage the GPU test relies on, and every refusal
of ``RelayConfig``."""
import math

import numpy as np
import pytest

from tests import relay_cases as rc

DBL_MAX = float(np.finfo(np.float64).max)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def relay_scalar(H, syndrome, probs, gammas, leg_iters, stop_after, leg_init, ms):
    """One shot, dict of edges, plain Python floats (in the manner of tests/ref_numpy.bp_decode)."""
    H = np.asarray(H, dtype=np.uint8)
    m, n = H.shape
    rows = [list(np.nonzero(H[c])[0]) for c in range(m)]
    cols = [list(np.nonzero(H[:, j])[0]) for j in range(n)]
    l0 = [math.log((1 - probs[j]) / probs[j]) for j in range(n)]
    W = [int(np.rint(min(max(l0[j], -32768.0), 32768.0) * 4294967296.0)) for j in range(n)]
    M, dec = list(l0), [0] * n
    if not any(int(x) & 1 for x in syndrome):
        return dict(bp=dec, converged=True, iters=0, solutions=0, best_leg=-1, weight=0, llr=M)
    b2c = {(c, j): l0[j] for c in range(m) for j in rows[c]}
    c2b = {}
    t = found = 0
    best, best_w, best_leg = None, 0, -1
    for r in range(len(leg_iters)):
        g = [float(x) for x in gammas[r]]
        if r > 0 and leg_init == 0:
            b2c = {(c, j): l0[j] for c in range(m) for j in rows[c]}
        for _ in range(int(leg_iters[r])):
            t += 1
            alpha = ms if ms != 0 else 1.0 - 2.0 ** (-t)
            for c in range(m):
                total = int(syndrome[c]) & 1
                low, fwd = DBL_MAX, []
                for j in rows[c]:
                    v = b2c[(c, j)]
                    total += 1 if v <= 0 else 0
                    fwd.append(low)
                    if abs(v) < low:
                        low = abs(v)
                low = DBL_MAX
                for k in range(len(rows[c]) - 1, -1, -1):
                    j = rows[c][k]
                    v = b2c[(c, j)]
                    mag = low if low < fwd[k] else fwd[k]
                    val = mag * alpha
                    c2b[(c, j)] = -val if (total + (1 if v <= 0 else 0)) % 2 else val
                    if abs(v) < low:
                        low = abs(v)
            for j in range(n):
                a = (1.0 - g[j]) * l0[j]
                b = g[j] * M[j]
                acc = a + b
                for c in cols[j]:
                    b2c[(c, j)] = acc
                    acc = acc + c2b[(c, j)]
                M[j] = acc
                dec[j] = 1 if acc <= 0 else 0
                suf = 0.0
                for c in reversed(cols[j]):
                    b2c[(c, j)] = b2c[(c, j)] + suf
                    suf = suf + c2b[(c, j)]
            if all(sum(dec[j] for j in rows[c]) % 2 == (int(syndrome[c]) & 1) for c in range(m)):
                found += 1
                w = sum(W[j] for j in range(n) if dec[j])
                if best is None or w < best_w:
                    best, best_w, best_leg = list(dec), w, r
                break
        if found == stop_after:
            break
    return dict(bp=best if found else dec, converged=found > 0, iters=t, solutions=found, best_leg=best_leg, weight=best_w if found else 0,
                llr=M)


@pytest.mark.parametrize("case", rc.CASES, ids=[c["id"] for c in rc.CASES])
def test_reference_equals_scalar_restatement(case):
    H = rc.matrix(case["code"]).toarray()
    S, p, cfg, ref = rc.syndromes(case["id"]), rc.priors_of(case), rc.config_of(case), rc.reference(case["id"])
    assert len(S) == rc.NONTRIVIAL + 1 and not S[-1].any() and S[:-1].any(axis=1).all()
    for b in range(len(S)):
        one = relay_scalar(H, S[b], p, cfg.gammas, cfg.leg_iters, cfg.stop_after, cfg.leg_init, case["ms"])
        for key in ("bp", "osd0", "osdw"):
            assert (ref[key][b] == np.array(one["bp"], np.uint8)).all(), (b, key)
        for key in ("converged", "iters", "solutions", "best_leg", "weight"):
            assert int(ref[key][b]) == int(one[key]), (b, key, ref[key][b], one[key])
        assert (_bits(ref["llr"][b]) == _bits(one["llr"])).all(), b
    assert ref["solutions"][-1] == 0 and ref["best_leg"][-1] == -1 and ref["weight"][-1] == 0 and ref["converged"][-1] and ref["iters"][-1] == 0


def test_per_shot_channels_in_the_reference():
    """The [B, n] form and the two-valued form give every shot the prior LLRs -- and the weights -- of its own channel."""
    from bp_osd_amd import relay_decode_reference

    case = rc.CASE_BY_ID["hgp_p06_r6_s3"]
    H, S, cfg = rc.matrix(case["code"]), rc.syndromes(case["id"])[:6], rc.config_of(case)
    n = H.shape[1]
    rng = np.random.default_rng(5)
    P = np.clip(0.06 * np.exp(rng.uniform(-1, 1, (6, n))), 1e-3, 0.4)
    rows = relay_decode_reference(H, S, P, cfg, 0.625)
    for b in range(6):
        one = relay_scalar(H.toarray(), S[b], P[b], cfg.gammas, cfg.leg_iters, cfg.stop_after, cfg.leg_init, 0.625)
        assert (rows["bp"][b] == np.array(one["bp"], np.uint8)).all() and rows["weight"][b] == one["weight"]
        assert (_bits(rows["llr"][b]) == _bits(one["llr"])).all()
    sel = (rng.random((6, n)) < 0.3).astype(np.uint8)
    alt = rng.uniform(0.02, 0.3, n)
    two = relay_decode_reference(H, S, np.full(n, 0.06), cfg, 0.625, prior_select=sel, alt_priors=alt)
    same = relay_decode_reference(H, S, np.where(sel != 0, alt, 0.06), cfg, 0.625)
    for key in two:
        assert (np.asarray(two[key]) == np.asarray(same[key])).all() or key == "llr"
    assert (_bits(two["llr"]) == _bits(same["llr"])).all()


@pytest.mark.parametrize("code", ["surface13_hz", "hgp_ham3_hz"])
@pytest.mark.parametrize("ms", [0.0, 0.625])
def test_degenerate_relay_is_the_oracles_min_sum(code, ms):
    from bp_osd_amd import RelayConfig, relay_decode_reference
    from oracle import OracleDecoder

    H = rc.matrix(code)
    n = H.shape[1]
    rng = np.random.default_rng(9)
    p = np.clip(0.08 * np.exp(rng.uniform(-1, 1, n) * np.log(3)), 1e-3, 0.4)
    S = rc.draw_syndromes(H, p, 13, 30)
    max_iter = 12
    ref = relay_decode_reference(H, S, p, RelayConfig(np.zeros((1, n)), [max_iter]), ms)
    o = OracleDecoder(H, channel_probs=p, max_iter=max_iter, bp_method="ms", ms_scaling_factor=ms, osd_method="osd0").decode_batch(S)
    assert (ref["bp"] == o["bp"]).all() and (ref["converged"] == o["converged"].astype(bool)).all() and (ref["iters"] == o["iters"]).all()
    assert (_bits(ref["llr"]) == _bits(o["llr"])).all()
    if code == "hgp_ham3_hz":  # (surface13's six checks leave nothing open)
        assert 0 < ref["converged"][:-1].sum() < len(S) - 1, "the shots should mix converged and non-converged"
    assert (ref["solutions"] == ref["converged"] & S.any(axis=1)).all() and (ref["best_leg"][ref["solutions"] == 0] == -1).all()


# The issue's table of counts -- (10, 3, 0), (4, 0, 23), (11, 0, 16) -- comes from a prototype whose memory strengths and shots it
# does not give, so no choice of seed here can reproduce it: the strengths are `relay_gammas` defaults at the case's seed and
# the shots numpy's default_rng at the same seed.  What the counts are for holds: all four coverage conditions, with both
# `leg_init` values, and at p = 0.10 close to half the shots stay open as in the issue's table.  The lower bounds asserted below
# guard the conditions; the exact counts of this table are frozen next to them, so a change of the reference or of the
# generators shows.
# what the reference yields on the table, frozen: (first solution from a leg >= 1, best solution not the first, no solution)
COVERAGE = {
    "hgp_p06_r6_s3": (7, 2, 3),
    "hgp_p10_r4_s2": (5, 0, 20),
    "hgp_p10_r4_s2_keep": (5, 2, 20),
    "hgp_nonuniform_negative": (5, 2, 14),
    "surface13_r3": (4, 0, 0),
}


def test_coverage_conditions():
    cov = {c["id"]: rc.coverage(c["id"]) for c in rc.CASES}
    print(cov)
    assert sum(v["later"] for v in cov.values()) >= 1, cov
    assert sum(v["best_not_first"] for v in cov.values()) >= 1, cov  # (= two solutions of different weight in one shot)
    assert sum(v["none"] for v in cov.values()) >= 1, cov
    for leg_init in (0, 1):
        assert sum(cov[c["id"]]["later"] for c in rc.CASES if c["init"] == leg_init) >= 1, (leg_init, cov)
    # the settings of the issue's table: shots rescued by a later leg at p = 0.06, shots left open at p = 0.10
    assert cov["hgp_p06_r6_s3"]["later"] >= 4 and cov["hgp_p06_r6_s3"]["best_not_first"] >= 1, cov
    assert cov["hgp_p10_r4_s2"]["later"] >= 2 and cov["hgp_p10_r4_s2"]["none"] >= 8, cov
    assert cov["hgp_p10_r4_s2_keep"]["later"] >= 2 and cov["hgp_p10_r4_s2_keep"]["none"] >= 8, cov
    assert {k: (v["later"], v["best_not_first"], v["none"]) for k, v in cov.items()} == COVERAGE
    neg = rc.config_of(rc.CASE_BY_ID["hgp_nonuniform_negative"]).gammas[1]
    assert (neg < 0).mean() > 0.6 and len(set(rc.priors_of(rc.CASE_BY_ID["hgp_nonuniform_negative"]))) > 10


def test_shape_cases_sit_where_they_should():
    a, b, d = (rc.matrix(rc.SHAPE_BY_ID[k]["code"]) for k in ("lds_last_fit", "ws_first", "degrees_20_9"))
    assert rc.LDS_PER_CU - 128 < rc.bp_relay_lds_bytes(a.shape[0], a.shape[1], a.nnz) <= rc.LDS_PER_CU and rc.expected_instance(a) == 1
    assert rc.LDS_PER_CU < rc.bp_relay_lds_bytes(b.shape[0], b.shape[1], b.nnz) <= rc.LDS_PER_CU + 128 and rc.expected_instance(b) == 2
    assert np.diff(d.indptr).max() == 20 and np.bincount(d.indices).max() == 9
    for H in (a, b, d):
        assert H.shape[0] % 64 and H.shape[1] % 64
    r3, r4 = (rc.matrix(rc.SHAPE_BY_ID[k]["code"]) for k in ("dem_rounds3_lds", "dem_rounds4_ws"))
    assert r3.shape == (768, 2176) and rc.bp_relay_lds_bytes(768, 2176, r3.nnz) == 161824 and rc.expected_instance(r3) == 1
    assert r4.shape == (960, 2768) and rc.bp_relay_lds_bytes(960, 2768, r4.nnz) == 205056 and rc.expected_instance(r4) == 2
    for H in (r3, r4):  # irregular: bit degrees 2 .. 4, check degrees up to 9
        assert sorted(set(np.bincount(H.indices))) == [2, 3, 4] and np.diff(H.indptr).max() == 9 and np.diff(H.indptr).min() < 9
    from bp_osd_amd import codes

    h = codes.h1922(compute_logicals=False).hz
    assert h.nnz == 5766 and rc.bp_relay_lds_bytes(h.shape[0], h.shape[1], h.nnz) <= rc.LDS_PER_CU
    for k in rc.SHAPE_BY_ID:
        ref = rc.shape_reference(k)
        assert 0 < (ref["solutions"] > 0).sum(), k


def test_relay_gammas():
    from bp_osd_amd import relay_gammas

    g = relay_gammas(58, 4, seed=3)
    assert g.shape == (4, 58) and g.dtype == np.float64 and (g[0] == 0.125).all()
    assert (g[1:] == -0.24 + (0.66 - -0.24) * np.random.default_rng(3).random((3, 58))).all()
    assert (relay_gammas(5, 1, gamma0=-0.5) == -0.5).all()
    assert (relay_gammas(58, 4, seed=3) == g).all() and (relay_gammas(58, 4, seed=4)[1:] != g[1:]).any()


@pytest.mark.parametrize("kw,word", [
    (dict(gammas=[[0.1, np.nan]], leg_iters=[3]), "gammas[0][1]"),
    (dict(gammas=[[0.1, 0.2], [np.inf, 0.0]], leg_iters=[3, 3]), "gammas[1][0]"),
    (dict(gammas=[[0.1, 0.2]], leg_iters=[0]), "leg_iters[0]"),
    (dict(gammas=[[0.1, 0.2], [0.1, 0.2]], leg_iters=[3, -1]), "leg_iters[1]"),
    (dict(gammas=[[0.1, 0.2], [0.1, 0.2]], leg_iters=[3]), "leg_iters"),
    (dict(gammas=[[0.1, 0.2]], leg_iters=[2.5]), "leg_iters"),
    (dict(gammas=[[0.1, 0.2]], leg_iters=[3], stop_after=0), "stop_after"),
    (dict(gammas=[[0.1, 0.2]], leg_iters=[3], leg_init=2), "leg_init"),
    (dict(gammas=[0.1, 0.2], leg_iters=[3]), "gammas"),
    (dict(gammas=np.zeros((0, 4)), leg_iters=[]), "gammas"),
])
def test_relay_config_refusals(kw, word):
    from bp_osd_amd import RelayConfig

    with pytest.raises(ValueError) as e:
        RelayConfig(**kw)
    assert word in str(e.value), str(e.value)


def test_relay_config_keeps_a_copy():
    from bp_osd_amd import RelayConfig

    g = np.full((2, 3), 0.25)
    cfg = RelayConfig(g, [4, 5], stop_after=2, leg_init=1)
    g[:] = 9
    assert (cfg.gammas == 0.25).all() and cfg.legs == 2 and cfg.n == 3 and cfg.total_iters == 9 and cfg.stop_after == 2 and cfg.leg_init == 1
    with pytest.raises(ValueError):
        cfg.gammas[0, 0] = 1.0


def test_c_abi_is_declared():
    import os
    from bp_osd_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    public = open(os.path.join(root, "include", "bposd_mi355x.h")).read()
    debug = open(os.path.join(root, "include", "bposd_mi355x_debug.h")).read()
    lib = _lib.load()
    for name in ("bposd_set_relay", "bposd_relay_stats"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and f"int {name}(" in public, name
    assert "BPOSD_BP_KERNEL_RELAY 6" in debug
    from bp_osd_amd import BpOsdDecoder

    assert BpOsdDecoder.BP_KERNEL_NAMES[6] == "bp_relay_kernel"


def _window_setting():
    """surface13 at 5 rounds, window (3, 1): windows of 57 and 51 faults; strengths for all 325 faults of the model."""
    from bp_osd_amd import RelayConfig, relay_gammas
    from tests import window_cases as wc

    H, L, priors, times = wc.model("surface13-R5")
    cfg = RelayConfig(relay_gammas(H.shape[1], 3, seed=12), [6, 5, 5], stop_after=2)
    return H, L, priors, times, cfg


def test_window_engine_slices_a_model_wide_configuration():
    """``windowed_dem_decode_sim(..., relay=cfg)`` with cfg over all N faults: every window runs with its own columns of the
    strengths, windows share a decoder only where those agree, and the host loop equals the reference window by window."""
    from bp_osd_amd import RelayConfig, RelayReferenceDecoder, relay_decode_reference, window_plan, windowed_dem_decode_sim

    H, L, priors, times, cfg = _window_setting()
    N = H.shape[1]
    kw = dict(engine="numpy", decoder_factory=RelayReferenceDecoder, seed=5, target_runs=96, batch_size=96, bp_method="ms",
              ms_scaling_factor=0.625, osd_method="osd_off")
    sim = windowed_dem_decode_sim(H, L, priors, times, (3, 1), relay=cfg, **kw)
    plan = sim.plan
    widths = sorted({w.fault.size for w in plan.windows})
    assert len(widths) > 1 and widths[-1] < N, widths  # no single width: one configuration per window is what it takes
    assert len(plan.unique) == len(plan.windows)  # random strengths differ from window to window
    assert len(window_plan(H, times, (3, 1), priors=priors).unique) < len(plan.windows)
    for w, dec in zip(plan.unique, sim.decoders):
        assert (dec._cfg.gammas == cfg.gammas[:, plan.windows[w].fault]).all() and dec._cfg.stop_after == 2
        assert (dec._cfg.leg_iters == cfg.leg_iters).all()
    assert 0 < sim.bp_converge_count < 96 and 0 < sim.osdw_success_count < 96
    # window 0 of the host loop is the reference on the window's matrix, priors and strengths
    from tests.dem_cases import unpack

    det = unpack(sim.last_batch("detectors"), H.shape[0])
    w0 = plan.windows[0]
    ref = relay_decode_reference(w0.H, det[:, w0.det], priors[w0.fault], cfg.restrict(w0.fault), 0.625)
    sel = w0.fault[w0.commit != 0]
    corr = unpack(sim.last_batch("correction"), N)
    assert (corr[:, sel] == ref["osdw"][:, w0.commit != 0]).all()
    # strengths that repeat from round to round keep the shared decoders of a time-invariant model
    flat = RelayConfig(np.tile([[0.125], [-0.1], [0.4]], (1, N)), [6, 5, 5], stop_after=2)
    again = windowed_dem_decode_sim(H, L, priors, times, (3, 1), relay=flat, run_sim=False, **kw)
    assert len(again.plan.unique) == len(window_plan(H, times, (3, 1), priors=priors).unique) < len(plan.windows)
    # a configuration of another width goes to every window as it is, and the refusal names the window
    with pytest.raises(ValueError, match=r"window \d+ .*relay configuration is for 57 bits"):
        windowed_dem_decode_sim(H, L, priors, times, (3, 1), relay=cfg.restrict(np.arange(57)), run_sim=False, **kw)


def test_reference_decoder_takes_per_shot_channels_or_refuses():
    from bp_osd_amd import RelayReferenceDecoder, relay_decode_reference

    case = rc.CASE_BY_ID["hgp_p10_r4_s2"]
    H, S, cfg = rc.matrix(case["code"]), rc.syndromes(case["id"])[:8], rc.config_of(case)
    n = H.shape[1]
    rng = np.random.default_rng(2)
    P = rng.uniform(0.03, 0.2, (8, n))
    sel, alt = (rng.random((8, n)) < 0.3).astype(np.uint8), rng.uniform(0.02, 0.3, n)
    d = RelayReferenceDecoder(H, channel_probs=np.full(n, 0.1), relay=cfg, ms_scaling_factor=0.625)
    for got, want in ((d.decode_batch(S, channel_probs_rows=P, want_llr=True), relay_decode_reference(H, S, P, cfg, 0.625)),
                      (d.decode_batch(S, prior_select=sel, alt_channel_probs=alt),
                       relay_decode_reference(H, S, np.full(n, 0.1), cfg, 0.625, prior_select=sel, alt_priors=alt))):
        assert (got["bp"] == want["bp"]).all() and (got["weight"] == want["weight"]).all() and (_bits(got["llr"]) == _bits(want["llr"])).all()
    assert (d.decode_batch(S, channel_probs_rows=P)["weight"] != d.decode_batch(S)["weight"]).any()
    for bad in (dict(packed=True), dict(prior_select=sel), dict(channel_probs_rows=P, prior_select=sel, alt_channel_probs=alt)):
        with pytest.raises(ValueError):
            d.decode_batch(S, **bad)


def test_restrict():
    from bp_osd_amd import RelayConfig

    cfg = RelayConfig(np.arange(12.0).reshape(3, 4) / 20, [2, 3, 4], stop_after=2, leg_init=1)
    sub = cfg.restrict([3, 1])
    assert (sub.gammas == cfg.gammas[:, [3, 1]]).all() and sub.n == 2 and sub.legs == 3
    assert (sub.leg_iters == cfg.leg_iters).all() and sub.stop_after == 2 and sub.leg_init == 1
