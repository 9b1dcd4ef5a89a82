"""The models, tables and numpy references of tests/test_dem_cpu.py and tests/test_gpu_dem.py.

References are computed from host draws of the Philox stream (``sim.philox_uniforms < priors``) and from rows the CPU oracle
decoded -- never from rows a GPU produced.  Every reference is computed once per process (lru_cache) and handed out
read-only.
"""
from __future__ import annotations

import functools
import os

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIOR_VALUES = (0.0, 1.0, 1e-3, 0.03, 0.5)
SAMPLER_SEED = 11


def pack(bits):
    """uint8 [B, c] -> uint64 [B, ceil(c/64)], bit (j & 63) of word (j >> 6) = entry j, padding zero."""
    bits = np.ascontiguousarray(bits, dtype=np.uint8)
    by = np.packbits(bits, axis=1, bitorder="little")
    out = np.zeros((bits.shape[0], 8 * ((bits.shape[1] + 63) // 64)), np.uint8)
    out[:, :by.shape[1]] = by
    return out.view("<u8")


def unpack(words, c):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")[:, :c]


def mod2(A, X):
    """(A X^T)^T over GF(2) for uint8 rows X [B, N] and a sparse or dense A [r, N] -> uint8 [B, r]."""
    A = sp.csr_matrix(A).astype(np.int64)
    return np.ascontiguousarray((np.asarray(A @ np.asarray(X, dtype=np.int64).T) & 1).T.astype(np.uint8))


# --------------------------------------------------------------------------------------------------- random sparse models
# (N, M, k, B, first_shot): the shapes at which dem_sample_kernel can go wrong.  A workgroup is 4 waves and a wave step
# covers 128 faults (a chunk).  The grid is min(B, 8 workgroups per CU = 2048 on an MI355X): every B is above 2048 and no
# multiple of it, so every case has a grid-stride with a tail, and a B above 4096 gives some workgroups a third shot -- the
# second use of an accumulator row, written out, cleared and flipped again.
SAMPLER_CASES = [
    dict(id="1-1-1", N=1, M=1, k=1, B=4101, first_shot=0),               # smallest shape
    dict(id="127-63-1", N=127, M=63, k=1, B=6247, first_shot=0),         # odd tail of the pair draw; one chunk, fewer chunks than waves; 3-4 shots per workgroup
    dict(id="128-64-64", N=128, M=64, k=64, B=4099, first_shot=0),       # exact words; 2-3 shots per workgroup
    dict(id="129-65-65", N=129, M=65, k=65, B=4173, first_shot=2 ** 32 + 12345),  # one bit into the next word everywhere; two observable words; 2-3 shots per workgroup
    dict(id="1031-130-3", N=1031, M=130, k=3, B=4109, first_shot=7),     # 9 chunks on 4 waves; 2-3 shots per workgroup
]
SAMPLER_BY_ID = {c["id"]: c for c in SAMPLER_CASES}
EMPTY_FAULT, OBS_ONLY_FAULT, HEAVY_FAULT = 1, 2, 3  # the special columns of random_model, where the shape has room for them


@functools.lru_cache(maxsize=None)
def random_model(N, M, k, seed=SAMPLER_SEED):
    """(H, L, priors): random sparse H [M, N] and L [k, N] (scipy CSR, uint8) and priors drawn from PRIOR_VALUES so that 0
    and 1 are hit exactly.  Where the shape has room (N >= 4), fault 1 has an empty column, fault 2 touches one observable and
    no detector, and fault 3 touches every detector and observable up to 48 of them (>= 40 where M + k >= 40); faults 2 and 3
    fire in about half of the shots."""
    rng = np.random.default_rng(seed + 1000 * N + M)
    H = (rng.random((M, N)) < min(0.5, 6.0 / M)).astype(np.uint8)
    L = (rng.random((k, N)) < min(0.5, 3.0 / k)).astype(np.uint8)
    priors = rng.choice(PRIOR_VALUES, size=N)
    if N >= 4:
        H[:, EMPTY_FAULT] = 0
        L[:, EMPTY_FAULT] = 0
        H[:, OBS_ONLY_FAULT] = 0
        L[:, OBS_ONLY_FAULT] = 0
        L[k - 1, OBS_ONLY_FAULT] = 1
        H[:, HEAVY_FAULT] = 0
        L[:, HEAVY_FAULT] = 0
        H[:min(M, 48), HEAVY_FAULT] = 1
        L[:max(0, min(k, 48 - M)), HEAVY_FAULT] = 1
        priors[EMPTY_FAULT] = 1.0  # fires in every shot and must change nothing
        priors[OBS_ONLY_FAULT] = priors[HEAVY_FAULT] = 0.5
    else:
        H[:], L[:], priors[:] = 1, 1, 0.5
    priors.setflags(write=False)
    return sp.csr_matrix(H), sp.csr_matrix(L), priors


@functools.lru_cache(maxsize=None)
def sampler_reference(case_id, first_shot=None):
    """Packed faults, detectors and observables of the case's shots from the host draw."""
    from bp_osd_amd.sim import philox_uniforms

    c = SAMPLER_BY_ID[case_id]
    H, L, priors = random_model(c["N"], c["M"], c["k"])
    first = c["first_shot"] if first_shot is None else first_shot
    faults = (philox_uniforms(SAMPLER_SEED, first, c["B"], c["N"]) < priors).astype(np.uint8)
    out = dict(faults=pack(faults), detectors=pack(mod2(H, faults)), observables=pack(mod2(L, faults)), fault_bits=faults)
    for v in out.values():
        v.setflags(write=False)
    return out


# --------------------------------------------------------------------------------------------------- phenomenological models
DECODER = dict(max_iter=4, bp_method="ms", ms_scaling_factor=0.625, osd_method="osd_cs", osd_order=2)
RUN_SEED = 5

# Whole runs: seed 5, first shot 0, one batch.  `oracle` holds what the CPU oracle gives on that stream (computed on the
# CPU, tests/test_dem_cpu.py recomputes them): shots with no detector fired, bp converged, shots whose bp / osd0 / osdw
# observables are wrong.
RUN_CASES = [
    dict(id="surface13-R3", code="surface13", R=3, p=0.04, q=0.04, B=256, shape=(24, 70), k=1,
         oracle=dict(trivial=15, converged=171, wrong=(57, 44, 44))),
    dict(id="hgp400-R1", code="hgp400", R=1, p=0.03, q=0.03, B=128, shape=(384, 992), k=16,
         oracle=dict(trivial=None, converged=23, wrong=(58, 15, 5))),
    dict(id="hgp400-R3", code="hgp400", R=3, p=0.02, q=0.02, B=64, shape=(768, 2176), k=16,
         oracle=dict(trivial=None, converged=11, wrong=(26, 5, 2))),
]
RUN_BY_ID = {c["id"]: c for c in RUN_CASES}


@functools.lru_cache(maxsize=None)
def code(name):
    from bp_osd_amd.codes import hgp, surface13

    if name == "surface13":
        return surface13()
    seed = np.loadtxt(os.path.join(ROOT, "tests", "golden", "mkmn_16_4_6.txt")).astype(np.uint8)
    return hgp(seed)


@functools.lru_cache(maxsize=None)
def run_model(case_id):
    from bp_osd_amd.dem import phenomenological_dem

    c = RUN_BY_ID[case_id]
    cd = code(c["code"])
    return phenomenological_dem(cd.hz, cd.lz, c["R"], c["p"], c["q"])


@functools.lru_cache(maxsize=None)
def random_L70():
    """A random L of k = 70 on the [[13,1,3]] R = 3 model (density 0.3, seed 11): the scorer's second observable word."""
    L = (np.random.default_rng(11).random((70, 70)) < 0.3).astype(np.uint8)
    return sp.csr_matrix(L)


def oracle_sim(H, L, priors, B, batch_size=None, **kw):
    """dem_decode_sim on the host around the CPU oracle."""
    from bp_osd_amd.dem import dem_decode_sim
    from oracle import OracleDecoder

    opts = dict(DECODER)
    opts.update(kw)
    return dem_decode_sim(H, L, priors, batch_size=batch_size or B, engine="numpy", seed=RUN_SEED, target_runs=B,
                          decoder_factory=OracleDecoder, **opts)


ITEMS = ("faults", "detectors", "observables", "obs_bp", "obs_osd0", "obs_osdw", "flags", "converged", "iters", "obs_fail")
COUNTS = ("run_count", "bp_converge_count", "bp_success_count", "osd0_success_count", "osdw_success_count", "trivial_count")


@functools.lru_cache(maxsize=None)
def run_reference(case_id):
    """Counters and every last_batch item of the case on the oracle, one batch."""
    c = RUN_BY_ID[case_id]
    H, L, priors = run_model(case_id)
    sim = oracle_sim(H, L, priors, c["B"])
    out = {k: getattr(sim, k) for k in COUNTS}
    for item in ITEMS:
        a = np.array(sim.last_batch(item))
        a.setflags(write=False)
        out[item] = a
    out["osdw_observable_error_rates"] = np.array(sim.osdw_observable_error_rates)
    return out


def numpy_score(truth, obs_bp, obs_osd0, obs_osdw, converged, detectors, k):
    """flags [B], the five counters and obs_fail [k] from packed rows: what dem_score_kernel computes, restated."""
    wrong = [(np.asarray(o) != np.asarray(truth)).any(axis=1) for o in (obs_bp, obs_osd0, obs_osdw)]
    conv = np.asarray(converged) != 0
    quiet = ~np.asarray(detectors).any(axis=1)
    flags = wrong[0].astype(np.uint8) | (wrong[1].astype(np.uint8) << 1) | (wrong[2].astype(np.uint8) << 2) | (quiet.astype(np.uint8) << 3)
    counters = [int(conv.sum()), int((conv & ~wrong[0]).sum()), int((~wrong[1]).sum()), int((~wrong[2]).sum()), int(quiet.sum())]
    obs_fail = (unpack(obs_osdw, k) != unpack(truth, k)).sum(axis=0).astype(np.int32)
    return flags, counters, obs_fail
