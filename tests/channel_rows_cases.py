"""Cases, inputs and the shot-by-shot oracle reference of the per-shot channel rows (``decode_batch(channel_probs_rows=P)``).

One row of ``CASES`` per kernel family the rows must reach: matrices of tests/edge_codes.py (every bp_kernel degree pair
class, the any-degree, serial, class and HBM-resident BP kernels, osd_kernel and osd_large_kernel) and of
tests/local_codes.py (bp_local_kernel at both strides).  The reference is the oracle used the documented way:
``update_channel_probs(P[b])``, then decode ``S[b]``, shot by shot (tests/sim_util.OracleAdapter's decoder).
tests/test_channel_rows_cpu.py keeps the table honest without a GPU, tests/test_gpu_channel_rows.py runs it.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

from tests.edge_codes import EDGE_BY_ID, osd_words, pcm_for
from tests.local_codes import matrix_of, row_by_id

EDGE_IDS = ("bp_pair_4_2", "bp_pair_8_4", "bp_pair_16_8", "bp_anydeg_dc17", "bp_serial_dv8", "bp_class_mp256_m170",
            "bp_hbm_m1025_dc9", "bp_shape8_m1025_dc8", "large_n2048_m1000")
LOCAL_IDS = ("reg64_s1", "reg128_s1", "random31_s3_hz", "reg1025_s1")
EDGE_Q = 0.03

# id, q and the settings that differ from the default (osd_cs 6): the table of the issue, reg1025_s1 once more at q = 0.03
# (local kernel, stride 2048, converged shots) and two more orders on bp_pair_8_4
CASES = [dict(id=i, code=i, q=EDGE_Q) for i in EDGE_IDS] + [dict(id=i, code=i, q=None) for i in LOCAL_IDS]
TABLE_IDS = tuple(c["id"] for c in CASES)
CASES.append(dict(id="reg1025_s1_q0.03", code="reg1025_s1", q=EDGE_Q))
CASES.append(dict(id="bp_pair_8_4_osd_e5", code="bp_pair_8_4", q=EDGE_Q, osd=("osd_e", 5)))
CASES.append(dict(id="bp_pair_8_4_osd0", code="bp_pair_8_4", q=EDGE_Q, osd=("osd0", 0)))
CASE_BY_ID = {c["id"]: c for c in CASES}


def is_local(case):
    return case["code"] in LOCAL_IDS


@functools.lru_cache(maxsize=None)
def matrix(code):
    H = matrix_of(row_by_id(code)) if code in LOCAL_IDS else pcm_for(EDGE_BY_ID[code])
    H = sp.csr_matrix(H, dtype=np.uint8)
    H.sort_indices()
    return H


def case_q(case):
    return case["q"] if case["q"] is not None else row_by_id(case["code"])["q"]


def settings(case, **over):
    """Decoder keywords of a case: min-sum 0.625, max_iter 12, osd_cs 6, the ctor channel uniform q."""
    method, order = case.get("osd", ("osd_cs", 6))
    kw = dict(error_rate=case_q(case), max_iter=12, bp_method="ms", ms_scaling_factor=0.625, osd_method=method, osd_order=order)
    if not is_local(case) and EDGE_BY_ID[case["code"]].get("schedule"):
        kw["schedule"] = EDGE_BY_ID[case["code"]]["schedule"]
    kw.update(over)
    return kw


def expected_instances(case):
    """(bp, osd) as ``last_instance()`` must report them for a rows call of the case's 48 or 11 shots."""
    H = matrix(case["code"])
    m, n = H.shape
    if is_local(case):
        # rows keep the prior per bit: the plain (non-scalar-prior) instances; a call this small takes one check per thread
        bp = ("bp_local_kernel", (1, 1024, 8, 0) if m <= 1024 else (2, 2048, 4, 0))
        osd = ("osd_kernel", (osd_words(n),)) if (m <= 1024 and n < 2048) else ("osd_large_kernel", (2,))
        return bp + (False,), osd + (False,)
    e = EDGE_BY_ID[case["code"]]
    return e["bp"] + (False,), e["osd"] + (False,)


def osd_variant(case):
    return 0 if is_local(case) else EDGE_BY_ID[case["code"]]["osd_variant"]


@functools.lru_cache(maxsize=None)
def inputs(code, q):
    """(P [B, n] float64, S [B, m] uint8): every shot's channel and its syndrome."""
    H = matrix(code)
    m, n = H.shape
    B = 48 if (m <= 1024 and n < 2048) else 11
    rng = np.random.default_rng(7)
    P = np.clip(q * np.exp(rng.uniform(-1, 1, (B, n)) * np.log(4)), 1e-3, 0.4)
    P[rng.random((B, n)) < 0.01] = 0.5  # prior LLR exactly 0: the `<= 0` tie of the hard decision
    err = rng.random((B, n)) < P
    S = (np.asarray(sp.csr_matrix(H, dtype=np.int32) @ err.T.astype(np.int32)) % 2).T
    P.setflags(write=False)
    S = np.ascontiguousarray(S, dtype=np.uint8)
    S.setflags(write=False)
    return P, S


def case_inputs(case):
    return inputs(case["code"], case_q(case))


def oracle_rows(H, kw, P, S, want_llr=True):
    """The reference: update_channel_probs(P[b]), decode S[b], shot by shot."""
    from tests.sim_util import OracleAdapter

    kw = dict(kw)
    if "error_rate" in kw:  # (the adapter takes the ctor channel as a vector)
        kw["channel_probs"] = np.full(H.shape[1], kw.pop("error_rate"))
    o = OracleAdapter(H, **kw).dec
    outs = []
    for b in range(len(S)):
        o.update_channel_probs(P[b])
        outs.append(o.decode_batch(S[b:b + 1], want_llr=want_llr))
    keys = [k for k in ("osdw", "osd0", "bp", "converged", "iters", "llr") if outs[0].get(k) is not None]
    ref = {k: np.concatenate([r[k] for r in outs]) for k in keys}
    for v in ref.values():
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """The oracle's rows decode of a case, computed once per process and never written to."""
    case = CASE_BY_ID[case_id]
    P, S = case_inputs(case)
    return oracle_rows(matrix(case["code"]), settings(case), P, S)


@functools.lru_cache(maxsize=None)
def uniform_reference(case_id):
    """The oracle's decode of the same syndromes on the ctor channel (uniform q)."""
    from oracle import OracleDecoder

    case = CASE_BY_ID[case_id]
    _, S = case_inputs(case)
    return OracleDecoder(matrix(case["code"]), **settings(case)).decode_batch(S, want_llr=False)
