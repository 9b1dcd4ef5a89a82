"""The models, tables and references of tests/test_window_cpu.py and tests/test_gpu_window.py.

Every reference comes from ``windowed_dem_decode_sim(engine="numpy")`` around the CPU oracle -- the per-shot definition of
DESIGN.md 4.12 as a host loop -- and never from rows a GPU produced.  Each is computed once per process (lru_cache) and
handed out read-only.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

from tests import dem_cases

DECODER = dem_cases.DECODER
RUN_SEED = dem_cases.RUN_SEED

# Whole runs: seed 5, first shot 0, one batch.  `oracle`: BP converged in every window, shots whose observables are wrong,
# shots with no detector fired -- computed on the CPU oracle; tests/test_window_cpu.py recomputes them.
RUN_CASES = [
    dict(id="surface13-R3-w21", model="surface13-R3", window=(2, 1), B=256, oracle=dict(converged=89, wrong=45, quiet=15)),
    dict(id="surface13-R3-w32", model="surface13-R3", window=(3, 2), B=256, oracle=dict(converged=127, wrong=45, quiet=15)),
    dict(id="surface13-R5-w21", model="surface13-R5", window=(2, 1), B=256, oracle=dict(converged=28, wrong=67, quiet=2)),  # five windows, two handles
    dict(id="hgp400-R3-w21", model="hgp400-R3", window=(2, 1), B=64, oracle=dict(converged=1, wrong=3, quiet=0)),  # windows 384 x 1184 / 384 x 992
    dict(id="hgp400-R3-w32", model="hgp400-R3", window=(3, 2), B=64, oracle=dict(converged=0, wrong=2, quiet=0)),
    dict(id="random-520-w21", model="random-520-129-65", window=(2, 1), B=200, oracle=dict(converged=2, wrong=171, quiet=0)),  # four windows, two observable words
    dict(id="random-1031-w32", model="random-1031-130-3", window=(3, 2), B=200, oracle=dict(converged=0, wrong=172, quiet=0)),
]
RUN_BY_ID = {c["id"]: c for c in RUN_CASES}

# name -> (code, rounds, p = q) of the phenomenological models
PHENOMENOLOGICAL = {"surface13-R3": ("surface13", 3, 0.04), "surface13-R5": ("surface13", 5, 0.04), "hgp400-R3": ("hgp400", 3, 0.02)}
RANDOM = {"random-520-129-65": (520, 129, 65), "random-1031-130-3": (1031, 130, 3)}
# the unwindowed cases of dem_cases that a single window (W >= T) must reproduce
SINGLE_WINDOW = {"surface13-R3": "surface13-R3", "hgp400-R3": "hgp400-R3"}

ITEMS = ("faults", "detectors", "observables", "obs_osdw", "correction", "residual", "flags", "converged", "iters", "obs_fail")
COUNTS = ("run_count", "bp_converge_count", "osdw_success_count", "residual_count", "trivial_count")


@functools.lru_cache(maxsize=None)
def model(name):
    """(H, L, priors, detector_time) of a model above."""
    from bp_osd_amd.dem import phenomenological_dem, phenomenological_detector_times

    if name in PHENOMENOLOGICAL:
        code, R, p = PHENOMENOLOGICAL[name]
        cd = dem_cases.code(code)
        H, L, priors = phenomenological_dem(cd.hz, cd.lz, R, p, p)
        times = phenomenological_detector_times(cd.hz.shape[0], R)
    else:
        N, M, k = RANDOM[name]
        H0, L0, _ = dem_cases.random_model(N, M, k)
        rng = np.random.default_rng(3)
        H = sp.hstack([H0, sp.identity(M, dtype=np.uint8)], format="csr")
        L = sp.hstack([L0, sp.csr_matrix((k, M), dtype=np.uint8)], format="csr")
        priors = rng.choice([0.002, 0.01, 0.03], size=N + M)
        times = rng.integers(0, 5, size=M)
    priors = np.array(priors, dtype=np.float64)
    times = np.array(times, dtype=np.int64)
    priors.setflags(write=False)
    times.setflags(write=False)
    return H, L, priors, times


def toric_model():
    """hgp(ring_code(3)) at R = 2: with window (2, 1) its last window is 18 x 45 with rank 17 -- the refusal case."""
    from bp_osd_amd.codes import hgp, ring_code
    from bp_osd_amd.dem import phenomenological_dem, phenomenological_detector_times

    cd = hgp(ring_code(3))
    H, L, priors = phenomenological_dem(cd.hz, cd.lz, 2, 0.02, 0.02)
    return H, L, priors, phenomenological_detector_times(cd.hz.shape[0], 2)


def oracle_sim(name, window, B, batch_size=None, **kw):
    """windowed_dem_decode_sim on the host around the CPU oracle."""
    from bp_osd_amd.window import windowed_dem_decode_sim
    from oracle import OracleDecoder

    H, L, priors, times = model(name)
    opts = dict(DECODER)
    opts.update(kw)
    return windowed_dem_decode_sim(H, L, priors, times, window, batch_size=batch_size or B, engine="numpy", seed=RUN_SEED, target_runs=B,
                                   decoder_factory=OracleDecoder, **opts)


def snapshot(sim):
    """Counters and every last_batch item of a finished run, read-only."""
    out = {k: getattr(sim, k) for k in COUNTS}
    for item in ITEMS:
        a = np.array(sim.last_batch(item))
        a.setflags(write=False)
        out[item] = a
    out["osdw_observable_error_rates"] = np.array(sim.osdw_observable_error_rates)
    return out


@functools.lru_cache(maxsize=None)
def run_reference(case_id):
    """Counters and every last_batch item of the case on the oracle, one batch."""
    c = RUN_BY_ID[case_id]
    return snapshot(oracle_sim(c["model"], c["window"], c["B"]))


@functools.lru_cache(maxsize=None)
def single_window_reference(name):
    """The model decoded as one window (W = C = T) on the oracle."""
    H, L, priors, times = model(name)
    T = int(times.max()) + 1
    return snapshot(oracle_sim(name, (T, T), dem_cases.RUN_BY_ID[SINGLE_WINDOW[name]]["B"]))


# --------------------------------------------------------------------------------------------------- window_step_kernel alone
def numpy_step(plan, H, L, s, running, obs, corr, decoded, prev_conv, prev_iters, conv_all, iters):
    """Step s of the plan restated on unpacked uint8 rows: commit window s - 1 from `decoded` ([B, |F_{s-1}|]) into copies of
    running [B, M], obs [B, k] and corr [B, N], fold prev_conv / prev_iters, gather window s.  Returns (running, obs, corr,
    next syndrome [B, |D_s|] or None, conv_all, iters)."""
    running, obs, corr = running.copy(), obs.copy(), corr.copy()
    conv_all, iters = conv_all.copy(), iters.copy()
    if s > 0:
        win = plan.windows[s - 1]
        sel = np.flatnonzero(win.commit)
        cols = win.fault[sel]
        c = decoded[:, sel] & 1
        running ^= dem_cases.mod2(sp.csc_matrix(H)[:, cols], c)
        obs ^= dem_cases.mod2(sp.csc_matrix(L)[:, cols], c)
        corr[:, cols] |= c
        conv_all &= (prev_conv != 0).astype(np.uint8)
        iters = iters + prev_iters
    synd = running[:, plan.windows[s].det].copy() if s < len(plan.windows) else None
    return running, obs, corr, synd, conv_all, iters
