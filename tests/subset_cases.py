"""The models, tables and references of tests/test_subset_cpu.py and tests/test_gpu_subset.py: fault sets of a fixed weight,
enumerated or drawn uniformly (bposd_dem_set_subset, dem_decode_sim(fault_weight=..., subset=...), dem_failure_spectrum).
Models and the decoder come from tests/dem_cases.py and tests/dem_weight_cases.py; every reference is computed on the host
(``bp_osd_amd.fault_subsets`` and the CPU oracle), once per process, and handed out read-only -- never from a GPU row.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import dem_cases as dc
from tests import dem_weight_cases as wc

SEED = dc.SAMPLER_SEED
MODES = {"enumerate": 1, "random": 2}

# the exact answer (tests/dem_weight_cases.exact_model under dem_cases.DECODER on the oracle): failing osdw sets of weight 0 .. 3
EXACT_FAILING = (0, 0, 21, 152)
EXACT_REL = 1e-8  # sum of the failure masses against exact_osdw_rate(): the integer log-weights round by 13 * 2^-33 = 1.5e-9


@functools.lru_cache(maxsize=None)
def increments(N):
    """int64 [N] drawn from +-dem_weight_cases.ARBITRARY_INCREMENTS: sums carry across the 32-bit halves and go negative."""
    rng = np.random.default_rng(900 + N)
    a = rng.choice(wc.ARBITRARY_INCREMENTS, size=N).astype(np.int64) * rng.choice((-1, 1), size=N)
    a.setflags(write=False)
    return a


def interior_support(N, M, k):
    """The faults of dem_cases.random_model with a prior inside (0, 1) -- the 0- and 1-priors are skipped, so n < N and position
    and fault index differ -- and the empty column (whose prior is 1) put back: with the heavy and the observable-only fault,
    which have prior 0.5, every special column is in the support."""
    _, _, p = dc.random_model(N, M, k)
    keep = (p > 0) & (p < 1)
    keep[dc.EMPTY_FAULT] = True
    sup = np.flatnonzero(keep).astype(np.int32)
    assert sup.size < N and {dc.EMPTY_FAULT, dc.OBS_ONLY_FAULT, dc.HEAVY_FAULT} <= set(sup.tolist())
    return sup


def rows_of(H, L, support, positions, incr=None):
    """The items of the shots whose sets are ``positions`` [B, w] of ``support`` (None: all faults): packed faults, detectors
    and observables, the 0/1 fault rows, and with ``incr`` the integer sums."""
    N = H.shape[1]
    sup = np.arange(N) if support is None else np.asarray(support, dtype=np.int64)
    B = positions.shape[0]
    f = np.zeros((B, N), np.uint8)
    f[np.arange(B)[:, None], sup[positions]] = 1
    assert (f.sum(axis=1) == positions.shape[1]).all()
    out = dict(faults=dc.pack(f), detectors=dc.pack(dc.mod2(H, f)), observables=dc.pack(dc.mod2(L, f)), fault_bits=f)
    if incr is not None:
        out["logw"] = f.astype(np.int64) @ np.asarray(incr, dtype=np.int64)
    return out


def reference(H, L, support, mode, w, first_shot, B, incr=None, seed=SEED):
    from bp_osd_amd import fault_subsets

    n = H.shape[1] if support is None else len(support)
    return rows_of(H, L, support, fault_subsets(seed, first_shot, B, n, w, mode), incr)


class Engine(wc.Engine):
    """dem_weight_cases.Engine with the subset switch."""

    def set_subset(self, mode, w, support=None, incr=None, n_support=None):
        """The return code of bposd_dem_set_subset; ``mode`` a name of MODES, None (off) or a raw int; None arrays are NULL."""
        m = 0 if mode is None else MODES.get(mode, mode)
        sup = None if support is None else np.ascontiguousarray(support, dtype=np.int32)
        inc = None if incr is None else np.ascontiguousarray(incr, dtype=np.int64)
        n = n_support if n_support is not None else (0 if sup is None else sup.size)
        return self.lib.bposd_dem_set_subset(self.h, m, w, None if sup is None else sup.ctypes.data, n, None if inc is None else inc.ctypes.data)


# --------------------------------------------------------------------------------------------------- whole runs
STRATUM_RESULTS = ("stratum_size", "stratum_mass") + tuple(f"{x}_failure_mass{e}" for x in ("bp", "osd0", "osdw") for e in ("", "_eb"))
STRATUM_ITEMS = ("faults", "flags", "converged", "logw")


def oracle_sim(H, L, priors, w, subset, batch_size=4096, seed=dc.RUN_SEED, **kw):
    from bp_osd_amd import dem_decode_sim
    from oracle import OracleDecoder

    return dem_decode_sim(H, L, priors, batch_size=batch_size, engine="numpy", seed=seed, decoder_factory=OracleDecoder, fault_weight=w,
                          subset=subset, **dict(dc.DECODER, **kw))


def snapshot(sim):
    """Counters, the stratum's results, its sums and the per-shot items of the last batch; with a harvest its results too."""
    out = {k: getattr(sim, k) for k in dc.COUNTS + STRATUM_RESULTS}
    out["ssum"] = dict(sim._ssum)
    for item in STRATUM_ITEMS:
        out[item] = np.array(sim.last_batch(item))
    if sim.harvest:
        out["min_logical_weight"], out["min_logical_shot"] = sim.min_logical_weight, sim.min_logical_shot
        out["min_logical_fault"] = None if sim.min_logical_fault is None else np.array(sim.min_logical_fault)
        out["failure_weight_counts"] = np.array(sim.failure_weight_counts)
        for k, v in sim.failures.items():
            out["failures_" + k] = np.array(v)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def assert_same_run(got, ref):
    for k in ref:
        if isinstance(ref[k], np.ndarray):
            assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype and (got[k] == ref[k]).all(), k
        else:
            assert got[k] == ref[k], (k, got[k], ref[k])


@functools.lru_cache(maxsize=None)
def exact_strata():
    """snapshot of every stratum w = 0 .. 13 of exact_model, enumerated whole on the oracle."""
    H, L, p = wc.exact_model()
    return tuple(snapshot(oracle_sim(H, L, p, w, "enumerate", batch_size=500)) for w in range(H.shape[1] + 1))


@functools.lru_cache(maxsize=None)
def surface_pairs(batch_size):
    """snapshot of surface13-R3 (24 x 70), w = 2 enumerated whole: all 2415 pairs, in batches of ``batch_size``."""
    H, L, p = dc.run_model("surface13-R3")
    return snapshot(oracle_sim(H, L, p, 2, "enumerate", batch_size=batch_size))


@functools.lru_cache(maxsize=None)
def hgp_random(w):
    """snapshot of hgp400-R1 (384 x 992, k = 16), sets of weight w drawn, one batch of 128, harvest = 8.  At w = 6 (this code's
    distance) the oracle corrects all 128; at w = 30 three shots fail under osdw, so the harvest has rows to compare."""
    H, L, p = dc.run_model("hgp400-R1")
    return snapshot(oracle_sim(H, L, p, w, "random", batch_size=128, target_runs=128, harvest=8))
