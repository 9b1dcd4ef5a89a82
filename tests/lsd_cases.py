"""Cases of the LSD mode (``BpOsdDecoder(..., lsd=LsdConfig(...))``): matrices, syndromes, settings and the reference.

``CASES`` is the table tests/test_lsd_cpu.py keeps honest on the CPU (the reference against a scalar restatement, coverage
conditions) and tests/test_gpu_lsd.py runs on the device bit for bit.  ``RUNS`` are the settings every case is decoded
with; ``EDGE_RUNS`` put a cap on a cluster size that occurs, and one below it, at the kernel's internal ceilings (64 and 65
checks: a second row per lane; 64 / 65 and 128 / 129 bits: another word per row; 256 / 257: the ceilings themselves).
The reference of a (case, run) pair is computed once per process and never written to.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

LSD_MAX = 256  # csrc/lsd_kernel.hip.h: LSD_MAXB == LSD_MAXC

# id, matrix, error rate of the shots and of the decoder, BP iterations (few: BP must leave shots open), shots drawn, seed of
# the generator, pick (the shots kept, all when absent); an all-zero syndrome follows the kept shots
CASES = [
    dict(id="surface13", code="surface13_hz", p=0.08, max_iter=3, shots=300, rng=901),
    dict(id="hgp_rep5", code="hgp_rep5_hz", p=0.08, max_iter=5, shots=300, rng=902),             # degree-class BP
    dict(id="reg1000", code="reg1000_s14", p=0.045, max_iter=6, shots=120, rng=903),             # (3,6)-regular: bp_local_kernel
    dict(id="dense_dc20_dv9", code="dense_dc20_dv9", p=0.03, max_iter=4, shots=200, rng=904),    # any-degree BP; clusters up to 73 of 150 bits
    dict(id="hbm_m1025", code="bp_shape8_m1025_dc6", p=0.01, max_iter=4, shots=96, rng=905),     # HBM-resident OSD (m > 1024)
    # weak BP on a (3,6)-regular 300 x 600 code: clusters of hundreds of bits, for the ceilings.  Kept: clusters of 129 and 130
    # bits (shots 30, 2), of 129 and 130 checks (28, 83), of 125 bits (53: two words per row, the others three), of 64 and 66
    # bits (24, 52), of 252 bits and checks (35), of 254 checks (56) and of 257 checks (6: one past the ceiling)
    dict(id="reg300_weak", code="reg300_s1", p=0.05, max_iter=2, shots=150, rng=7, pick=(2, 6, 24, 28, 30, 35, 52, 53, 56, 83)),
]
# Deterministic sizes: the bidiagonal chain of N checks (check i holds bits i and i + 1; the last check holds bit N - 1 and
# eight spare bits N .. N + 7, so that n - rank = 8 admits osd_cs 7) with the syndrome e_0.  Bit 0 has the largest prior LLR
# and keeps the largest posterior, so it is the last in bit order: bits 1, 2, ... join one per round, each with the next
# check; the cluster turns valid with the first bit that joins after bit N - 1 has brought the last check: exactly N bits and
# N checks.  128 / 129 and 192 / 193: a third and a fourth word per row and row per lane; 256: the last
# slot of every array of the elimination, status 0 exactly at both ceilings; 257: one past both, status 1.
CHAIN_SIZES = (128, 129, 192, 193, 256, 257)
CASES += [dict(id=f"chain_{N}", code=f"chain_{N}", chain=N, p=0.1, max_iter=2, shots=1, rng=0) for N in CHAIN_SIZES]
# ... and more bits than checks: the same chain with 100 further copies of bit 1's column (checks 0 and 1) at the lowest LLRs.
# They join first, one per round, bring no check and never make the cluster valid, so it ends with N + 100 bits on N checks:
# 256 bits exactly (status 0), and 257 bits on 157 checks (status 1 by bits: a bit past the ceiling is counted, not stored).
CHAIN_COPIES = 100
CHAIN_OVERFLOWS = ("chain_257", "chaindup_157")
CASES += [dict(id=f"chaindup_{N}", code=f"chaindup_{N}", chain=N, copies=CHAIN_COPIES, p=0.1, max_iter=2, shots=1, rng=0) for N in (156, 157)]
CASE_BY_ID = {c["id"]: c for c in CASES}
BP_KERNEL = {"surface13": "bp_class_kernel", "hgp_rep5": "bp_class_kernel", "reg1000": "bp_local_kernel", "dense_dc20_dv9": "bp_anydeg_kernel",
             "hbm_m1025": "bp_kernel"}
OSD_KERNEL = {"hbm_m1025": "osd_large_kernel"}

# (max_cluster_bits, max_cluster_checks, osd_method, osd_order, sort_tie_policy)
RUNS = [
    (LSD_MAX, LSD_MAX, "osd_cs", 7, 0),
    (LSD_MAX, LSD_MAX, "osd_off", 0, 1),
    (4, LSD_MAX, "osd_off", 0, 0),   # overflow by bits
    (LSD_MAX, 4, "osd_cs", 7, 1),    # overflow by checks
]
# (case, cap on bits, cap on checks): the CPU test asserts that each cap is met exactly by some shot of the case and
# exceeded by one by another (so cap and cap + 1 both occur)
EDGE_RUNS = [
    ("dense_dc20_dv9", 64, LSD_MAX), ("dense_dc20_dv9", LSD_MAX, 64),
    ("reg300_weak", LSD_MAX, LSD_MAX), ("reg300_weak", 129, LSD_MAX), ("reg300_weak", LSD_MAX, 129),
]


def edge_run(edge):
    """The run of one EDGE_RUNS row: OSD-0 behind the clusters, ties by ascending index."""
    return (edge[1], edge[2], "osd_0", 0, 0)


def run_id(run):
    return f"b{run[0]}_c{run[1]}_{run[2]}{run[3]}_tie{run[4]}"


@functools.lru_cache(maxsize=None)
def matrix(code):
    from bp_osd_amd import codes

    if code == "surface13_hz":
        H = codes.surface13().hz
    elif code == "hgp_rep5_hz":
        H = codes.hgp(codes.rep_code(5)).hz
    elif code == "reg1000_s14":
        from tests.local_codes import matrix_of, row_by_id

        H = matrix_of(row_by_id(code))
    elif code == "reg300_s1":
        H = codes.regular_ldpc_seed(300, 600, 3, 6, seed=1)
    elif code.startswith("chain"):
        N = int(code.split("_")[1])
        H = np.zeros((N, N + 8 + (CHAIN_COPIES if code.startswith("chaindup") else 0)), np.uint8)
        H[:2, N + 8:] = 1
        H[np.arange(N), np.arange(N)] = 1
        H[np.arange(N - 1), np.arange(1, N)] = 1
        H[N - 1, N:N + 8] = 1
    elif code == "dense_dc20_dv9":
        from tests.edge_codes import edge_pcm

        H = edge_pcm(70, 150, 20, 9, seed=5)
    elif code == "bp_shape8_m1025_dc6":
        from tests.edge_codes import EDGE_BY_ID, pcm_for

        H = pcm_for(EDGE_BY_ID[code])
    else:
        raise KeyError(code)
    H = sp.csr_matrix(H, dtype=np.uint8)
    H.sort_indices()
    return H


@functools.lru_cache(maxsize=None)
def syndromes(case_id):
    """uint8 [kept shots + 1, m]: H e for random e of the case's rate; the last shot is the all-zero syndrome."""
    case = CASE_BY_ID[case_id]
    H = matrix(case["code"])
    if "chain" in case:
        S = np.zeros((2, H.shape[0]), np.uint8)
        S[0, 0] = 1
        S.setflags(write=False)
        return S
    rng = np.random.default_rng(case["rng"])
    e = (rng.random((case["shots"], H.shape[1])) < case["p"]).astype(np.int32)
    if "pick" in case:
        e = e[list(case["pick"])]
    e = np.concatenate([e, np.zeros((1, H.shape[1]), np.int32)])
    S = np.ascontiguousarray((np.asarray(H.astype(np.int32) @ e.T) % 2).T.astype(np.uint8))
    S.setflags(write=False)
    return S


def settings(case, run):
    """Keyword arguments of ``BpOsdDecoder`` and of ``LsdReferenceDecoder`` alike (without ``lsd=``)."""
    kw = dict(max_iter=case["max_iter"], bp_method="ms", ms_scaling_factor=0.625, osd_method=run[2], osd_order=run[3], sort_tie_policy=run[4])
    if "chain" in case:  # bit 0 all but certainly clean: the largest LLR
        kw["channel_probs"] = np.concatenate([[1e-6], np.full(case["chain"] + 7, case["p"]), np.full(case.get("copies", 0), 0.4)])
    else:
        kw["error_rate"] = case["p"]
    return kw


def config_of(run):
    from bp_osd_amd import LsdConfig

    return LsdConfig(run[0], run[1])


def reference_decoder(pcm, **kw):
    """``LsdReferenceDecoder`` around the CPU oracle (also a ``decoder_factory=`` for ``engine="numpy"``)."""
    from bp_osd_amd import LsdReferenceDecoder
    from oracle import OracleDecoder

    return LsdReferenceDecoder(pcm, base_factory=OracleDecoder, **kw)


@functools.lru_cache(maxsize=None)
def reference(case_id, run):
    case = CASE_BY_ID[case_id]
    ref = reference_decoder(matrix(case["code"]), lsd=config_of(run), **settings(case, run)).decode_batch(syndromes(case_id))
    for v in ref.values():
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def uncapped(case_id, tie=0):
    """The definition without caps on the shots BP leaves open: dict of lsd_decode_reference plus ``open`` (shot indices)."""
    from bp_osd_amd import lsd_decode_reference
    from oracle import OracleDecoder

    case = CASE_BY_ID[case_id]
    H, S = matrix(case["code"]), syndromes(case_id)
    kw = settings(case, (0, 0, "osd_off", 0, tie))
    bp = OracleDecoder(H, **kw).decode_batch(S)
    open_ = np.flatnonzero(bp["converged"] == 0)
    out = lsd_decode_reference(H, S[open_], bp["llr"][open_], None, tie)
    out["open"], out["llr"] = open_, bp["llr"][open_]
    return out


@functools.lru_cache(maxsize=None)
def sizes_at_the_ceilings(case_id):
    """``max_bits`` and ``max_checks`` of the shots BP leaves open under the ceilings as caps (a shot of status 1 reports the
    sizes it ended with), plus ``open``."""
    from bp_osd_amd import LsdConfig, lsd_decode_reference

    ref = reference(case_id, (LSD_MAX, LSD_MAX, "osd_off", 0, 0))
    open_ = np.flatnonzero(ref["status"] >= 0)
    case = CASE_BY_ID[case_id]
    out = lsd_decode_reference(matrix(case["code"]), syndromes(case_id)[open_], ref["llr"][open_], LsdConfig(), 0)
    out["open"] = open_
    return out
