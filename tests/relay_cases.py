"""Cases of the relay mode (``BpOsdDecoder(..., relay=RelayConfig(...))``): matrices, channels, syndromes and the reference.

``CASES`` is the table tests/test_relay_cpu.py keeps honest on the CPU (reference against a scalar restatement, coverage
conditions) and tests/test_gpu_relay.py runs on the device bit for bit.  ``SHAPE_CASES`` are the matrices that pin the two
kernel instances and the shapes a kernel can go wrong at; ``bp_relay_lds_bytes`` restates the library's LDS budget.
The reference of a case is computed once per process and never written to.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

LDS_PER_CU = 160 * 1024  # MI355X: LDS of one CU
NONTRIVIAL = 44          # shots with a non-zero syndrome per case; one all-zero shot follows them


def bp_relay_lds_bytes(m, n, E):
    """csrc/bp_relay_kernel.hip.h: messages | prefixes (E doubles each), M | A | G (n doubles each), decision bytes, best
    solution, syndrome bytes (padded to 16), 32 control bytes."""
    pad = lambda x: (x + 15) & ~15
    return 8 * (2 * E + 3 * n) + 2 * pad(n) + pad(m) + 32


def expected_instance(H):
    m, n = H.shape
    return 1 if bp_relay_lds_bytes(m, n, H.nnz) <= LDS_PER_CU else 2


# id, matrix, p (None: the non-uniform channel), scaling, legs, iterations per leg, stop_after, leg_init, seed (shots, gammas)
CASES = [
    dict(id="hgp_p06_r6_s3", code="hgp_ham3_hz", p=0.06, ms=0.625, legs=6, iters=10, stop=3, init=0, seed=1),
    dict(id="hgp_p10_r4_s2", code="hgp_ham3_hz", p=0.10, ms=0.625, legs=4, iters=6, stop=2, init=0, seed=2),
    dict(id="hgp_p10_r4_s2_keep", code="hgp_ham3_hz", p=0.10, ms=0.625, legs=4, iters=6, stop=2, init=1, seed=2),
    # non-uniform priors (two exact ties at p = 0.5), the variable scaling factor, a leg whose strengths are mostly negative
    dict(id="hgp_nonuniform_negative", code="hgp_ham3_hz", p=None, ms=0.0, legs=3, iters=8, stop=2, init=0, seed=3, negative_leg=1),
    dict(id="surface13_r3", code="surface13_hz", p=0.08, ms=0.625, legs=3, iters=5, stop=2, init=1, seed=4),
]
CASE_BY_ID = {c["id"]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def matrix(code):
    from bp_osd_amd import codes

    if code == "hgp_ham3_hz":
        H = codes.hgp(codes.hamming_code(3)).hz
    elif code == "surface13_hz":
        H = codes.surface13().hz
    elif code.startswith("circ3_"):  # n x n circulant of weight 3: E = 3 n exactly
        H = codes.circulant(int(code.split("_")[1]), [0, 1, 3])
    elif code.startswith("mkmn_dem_"):  # phenomenological model of the [[400,16,6]] code's hz: irregular (bit degrees 2 .. 4, checks up to 9)
        import os

        from bp_osd_amd.dem import phenomenological_dem

        seed = np.loadtxt(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mkmn_16_4_6.txt")).astype(np.uint8)
        cd = codes.hgp(seed)
        H = phenomenological_dem(cd.hz, cd.lz, int(code.split("_")[2]), 0.02, 0.02)[0]
    elif code == "dense_dc20_dv9":
        from tests.edge_codes import edge_pcm

        H = edge_pcm(70, 150, 20, 9, seed=5)
    else:
        raise KeyError(code)
    H = sp.csr_matrix(H, dtype=np.uint8)
    H.sort_indices()
    return H


def priors_of(case):
    n = matrix(case["code"]).shape[1]
    if case["p"] is not None:
        return np.full(n, case["p"])
    rng = np.random.default_rng(100 + case["seed"])
    p = np.clip(0.07 * np.exp(rng.uniform(-1, 1, n) * np.log(3)), 1e-3, 0.4)
    p[rng.permutation(n)[:2]] = 0.5  # prior LLR exactly 0
    return p


def config_of(case, stop=None):
    from bp_osd_amd import RelayConfig, relay_gammas

    n = matrix(case["code"]).shape[1]
    g = relay_gammas(n, case["legs"], seed=case["seed"])
    if "negative_leg" in case:
        rng = np.random.default_rng(200 + case["seed"])
        g[case["negative_leg"]] = np.where(rng.random(n) < 0.8, rng.uniform(-0.35, -0.05, n), rng.uniform(0.0, 0.3, n))
    return RelayConfig(g, np.full(case["legs"], case["iters"], np.int32), stop_after=case["stop"] if stop is None else stop,
                       leg_init=case["init"])


def draw_syndromes(H, p, seed, count=NONTRIVIAL):
    """``count`` non-zero syndromes of errors drawn with probabilities p, then one all-zero syndrome."""
    rng = np.random.default_rng(seed)
    m, n = H.shape
    Hi = sp.csr_matrix(H, dtype=np.int32)
    rows = []
    while len(rows) < count:
        err = (rng.random((count, n)) < p).astype(np.int32)
        S = (np.asarray(Hi @ err.T) % 2).T
        rows.extend(S[S.any(axis=1)][:count - len(rows)])
    S = np.ascontiguousarray(np.vstack(rows + [np.zeros(m, np.int64)]), dtype=np.uint8)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def syndromes(case_id):
    case = CASE_BY_ID[case_id]
    return draw_syndromes(matrix(case["code"]), priors_of(case), case["seed"])


def _frozen(ref):
    for v in ref.values():
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(case_id, stop=None):
    """The numpy reference of a case (``stop``: another stop_after, e.g. 1 for the first solution of every shot)."""
    from bp_osd_amd import relay_decode_reference

    case = CASE_BY_ID[case_id]
    return _frozen(relay_decode_reference(matrix(case["code"]), syndromes(case_id), priors_of(case), config_of(case, stop), case["ms"]))


def coverage(case_id):
    """Per case: shots whose first solution comes from a leg >= 1, shots whose best solution is not their first (so two
    solutions of different weight were found), shots without a solution."""
    first, full = reference(case_id, 1), reference(case_id)
    nz = syndromes(case_id).any(axis=1)
    later = int((nz & (first["best_leg"] >= 1)).sum())
    moved = nz & (full["solutions"] >= 2) & (full["best_leg"] != first["best_leg"])
    assert (full["weight"][moved] < first["weight"][moved]).all()
    return dict(later=later, best_not_first=int(moved.sum()), none=int((nz & (full["solutions"] == 0)).sum()))


# ---- shapes: the two instances at the LDS threshold, degrees beyond the tuned kernels, sizes that are no multiple of 64
# mkmn_dem_3 (768 x 2176, 6528 edges) needs 161 824 bytes, 2 016 under the CU's 160 KB; one more round, mkmn_dem_4 (960 x 2768, 8256
# edges, 205 056 bytes), is past it: the irregular pair.  The circulants pin the threshold itself:
# circ3_2183 needs 56 bytes less than the CU's 160 KB (the last shape of instance 1), circ3_2184 is the first shape of instance 2
SHAPE_CASES = [
    dict(id="lds_last_fit", code="circ3_2183", p=0.02, shots=5, instance=1),
    dict(id="ws_first", code="circ3_2184", p=0.02, shots=5, instance=2),
    dict(id="dem_rounds3_lds", code="mkmn_dem_3", p=0.02, shots=5, instance=1),
    dict(id="dem_rounds4_ws", code="mkmn_dem_4", p=0.02, shots=5, instance=2),
    dict(id="degrees_20_9", code="dense_dc20_dv9", p=0.03, shots=12, instance=1),
]
SHAPE_BY_ID = {c["id"]: c for c in SHAPE_CASES}


def shape_config(case, legs=3, iters=6, stop=2, init=0):
    from bp_osd_amd import RelayConfig, relay_gammas

    n = matrix(case["code"]).shape[1]
    return RelayConfig(relay_gammas(n, legs, seed=11), np.full(legs, iters, np.int32), stop_after=stop, leg_init=init)


@functools.lru_cache(maxsize=None)
def shape_syndromes(case_id):
    case = SHAPE_BY_ID[case_id]
    H = matrix(case["code"])
    return draw_syndromes(H, np.full(H.shape[1], case["p"]), 21, case["shots"])


@functools.lru_cache(maxsize=None)
def shape_reference(case_id):
    from bp_osd_amd import relay_decode_reference

    case = SHAPE_BY_ID[case_id]
    H = matrix(case["code"])
    return _frozen(relay_decode_reference(H, shape_syndromes(case_id), np.full(H.shape[1], case["p"]), shape_config(case), 0.625))
