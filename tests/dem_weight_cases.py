"""The models, tables and references of tests/test_dem_weight_cpu.py and tests/test_gpu_dem_weight.py: importance sampling of
detector error models.  Shapes, models and the decoder come from tests/dem_cases.py; every reference is computed on the host
(``sim.philox_uniforms < q`` and the CPU oracle), once per process, and handed out read-only.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from tests import dem_cases as dc

ARBITRARY_INCREMENTS = (1, 2 ** 31, 2 ** 32, 2 ** 38 - 1)  # and their negatives: carries across the 32-bit halves, negative sums


# --------------------------------------------------------------------------------------------------- the sampler alone
@functools.lru_cache(maxsize=None)
def tilted_tables(case_id):
    """(q, incr, arbitrary) of a SAMPLER_CASES shape: q drawn per fault from {p, min(4 p, 0.5), 0.5 p} of random_model's priors
    with 0 and 1 kept, the increments of importance_table(p, q), and a second table drawn from +-ARBITRARY_INCREMENTS."""
    from bp_osd_amd import importance_table

    c = dc.SAMPLER_BY_ID[case_id]
    _, _, p = dc.random_model(c["N"], c["M"], c["k"])
    rng = np.random.default_rng(70 + c["N"])  # (a seed at which the arbitrary sums of every shape go both ways)
    pick = rng.integers(0, 3, size=c["N"])
    q = np.where(pick == 0, p, np.where(pick == 1, np.minimum(4 * p, 0.5), 0.5 * p))
    q = np.where((p == 0) | (p == 1), p, q)
    incr, _ = importance_table(p, q)
    arbitrary = rng.choice(ARBITRARY_INCREMENTS, size=c["N"]).astype(np.int64) * rng.choice((-1, 1), size=c["N"])
    for a in (q, incr, arbitrary):
        a.setflags(write=False)
    return q, incr, arbitrary


@functools.lru_cache(maxsize=None)
def tilted_sampler_reference(case_id):
    """dem_cases.sampler_reference with the draw against q, and the two log-weight rows."""
    from bp_osd_amd.sim import philox_uniforms

    c = dc.SAMPLER_BY_ID[case_id]
    H, L, _ = dc.random_model(c["N"], c["M"], c["k"])
    q, incr, arbitrary = tilted_tables(case_id)
    faults = (philox_uniforms(dc.SAMPLER_SEED, c["first_shot"], c["B"], c["N"]) < q).astype(np.uint8)
    out = dict(faults=dc.pack(faults), detectors=dc.pack(dc.mod2(H, faults)), observables=dc.pack(dc.mod2(L, faults)), fault_bits=faults,
               logw=faults.astype(np.int64) @ incr, logw_arbitrary=faults.astype(np.int64) @ arbitrary)
    for v in out.values():
        v.setflags(write=False)
    return out


class Engine:
    """bposd_dem_* through ctypes on a model (H, L, priors) with the sampling switch; dec = None: the sample-only engine."""

    def __init__(self, lib, H, L, priors, capacity, seed, dec=None):
        from bp_osd_amd import _lib

        self.lib, self._lib, self.h = lib, _lib, None
        self.M, self.N = H.shape
        self.k = L.shape[0]
        cfg = _lib.BposdDemConfig(device=0, seed=seed, capacity=capacity)
        a = [np.ascontiguousarray(v, dtype=np.int32) for v in (H.indptr, H.indices, L.indptr, L.indices)]
        p = np.ascontiguousarray(priors, dtype=np.float64)
        h = C.c_void_p()
        rc = lib.bposd_dem_create(C.byref(cfg), dec._h if dec is not None else None, a[0].ctypes.data, a[1].ctypes.data, self.M, a[2].ctypes.data,
                                  a[3].ctypes.data, self.k, self.N, p.ctypes.data, C.byref(h))
        _lib.check_dem(lib, None, rc)
        self.h = h

    def set_sampling(self, q, incr):
        """The return code of bposd_dem_set_sampling; None stands for a NULL pointer."""
        q = None if q is None else np.ascontiguousarray(q, dtype=np.float64)
        incr = None if incr is None else np.ascontiguousarray(incr, dtype=np.int64)
        return self.lib.bposd_dem_set_sampling(self.h, None if q is None else q.ctypes.data, None if incr is None else incr.ctypes.data)

    def error(self):
        return self.lib.bposd_dem_last_error(self.h).decode()

    def sample(self, first_shot, B):
        self.B = B
        return self.lib.bposd_dem_sample(self.h, first_shot, B)

    def fetch_rc(self, what):
        """(return code, array) of bposd_dem_fetch."""
        item, dtype, cols = self._lib.DEM_ITEMS[what]
        width = {"N": self.N, "M": self.M, "k": self.k}
        shape = (self.B,) if cols is None else (self.k,) if cols == "k32" else (self.B, (width[cols] + 63) // 64)
        out = np.empty(shape, np.dtype(dtype))
        return self.lib.bposd_dem_fetch(self.h, item, out.ctypes.data, out.nbytes), out

    def fetch(self, what):
        rc, out = self.fetch_rc(what)
        self._lib.check_dem(self.lib, self.h, rc)
        return out

    def device_bytes(self):
        return int(self.lib.bposd_dem_device_bytes(self.h))

    def close(self):
        if getattr(self, "h", None) is not None:
            self.lib.bposd_dem_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


# --------------------------------------------------------------------------------------------------- whole runs
WEIGHT_ITEMS = ("flags", "converged", "logw")
WEIGHT_RESULTS = ("weight_mean", "effective_sample_fraction") + tuple(
    f"{x}_logical_error_rate{e}" for x in ("bp", "osd0", "osdw") for e in ("", "_eb"))
RUN_SCALE = 3.0  # sample_scale of the whole-run comparisons


def oracle_sim(H, L, priors, B, seed=dc.RUN_SEED, batch_size=None, **kw):
    """dem_decode_sim on the host around the CPU oracle (dem_cases.oracle_sim with a seed and the sampling keywords)."""
    from bp_osd_amd.dem import dem_decode_sim
    from oracle import OracleDecoder

    return dem_decode_sim(H, L, priors, batch_size=batch_size or B, engine="numpy", seed=seed, target_runs=B, decoder_factory=OracleDecoder,
                          **dict(dc.DECODER, **kw))


def snapshot(sim):
    """Counters, weighted sums, reported results and the per-shot items of the last batch of a tilted run."""
    out = {k: getattr(sim, k) for k in dc.COUNTS + WEIGHT_RESULTS}
    out["wsum"] = dict(sim._wsum)
    for item in WEIGHT_ITEMS:
        a = np.array(sim.last_batch(item))
        a.setflags(write=False)
        out[item] = a
    return out


@functools.lru_cache(maxsize=None)
def tilted_run_reference(case_id):
    """snapshot of the RUN_CASES case on the oracle with sample_scale = RUN_SCALE, one batch."""
    c = dc.RUN_BY_ID[case_id]
    H, L, priors = dc.run_model(case_id)
    return snapshot(oracle_sim(H, L, priors, c["B"], sample_scale=RUN_SCALE))


# --------------------------------------------------------------------------------------------------- the exact answer
EXACT_SHOTS = 16384
EXACT_SEEDS = (5, 6, 7)
EXACT_SCALES = (4, 8)


@functools.lru_cache(maxsize=None)
def exact_model():
    """(H, L, priors): [[13,1,3]] hz and lz at R = 0 (N = 13), p = 0.01 with p[::3] = 0.004."""
    from bp_osd_amd.dem import phenomenological_dem

    cd = dc.code("surface13")
    H, L, p = phenomenological_dem(cd.hz, cd.lz, 0, 0.01, 0.0)
    p = p.copy()
    p[::3] = 0.004
    p.setflags(write=False)
    return H, L, p


@functools.lru_cache(maxsize=None)
def exact_osdw_rate():
    """The osdw logical error rate of exact_model under dem_cases.DECODER on the oracle, from all 2^13 fault rows:
    sum over f of P(f) [L c(H f) != L f]."""
    import math

    from oracle import OracleDecoder

    H, L, p = exact_model()
    N = H.shape[1]
    f = ((np.arange(2 ** N)[:, None] >> np.arange(N)) & 1).astype(np.uint8)
    r = OracleDecoder(H, channel_probs=p, **dc.DECODER).decode_batch(dc.mod2(H, f))
    wrong = (dc.mod2(L, np.asarray(r["osdw"], dtype=np.uint8) & 1) != dc.mod2(L, f)).any(axis=1)
    prob = np.where(f == 1, p, 1 - p).prod(axis=1)
    assert abs(math.fsum(prob) - 1) < 1e-12
    return math.fsum(prob[wrong])
