"""Cases of the higher LSD orders (``LsdConfig(method=..., order=..., min_free_bits=..., grow_bits_limit=...)``).

``TABLE`` pairs cases of tests/lsd_cases.py -- and two more chains, 248 and 249 checks -- with order settings; each row meets
a condition tests/test_lsd_order_cpu.py asserts on the reference (``EXPECT``), so that the device table of
tests/test_gpu_lsd_order.py cannot be trivial.  ``RUNS`` are the OSD settings and tie policies every row is decoded with.
The two fp64 cases give ``dense_dc20_dv9`` a two-valued per-shot channel and ``hgp_rep5`` a channel row per shot; their
seeds were searched on the CPU so that on some shot the sweep's choice differs from the one Hamming weights would make.
The reference of a (row, run) pair is computed once per process and never written to.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import lsd_cases as lc

# the chain of tests/lsd_cases.py with N checks and N + 8 bits: grown for 8 free bits it ends with min(N + 8, 256) bits
CASE_BY_ID = dict(lc.CASE_BY_ID)
for _N in (248, 249):
    CASE_BY_ID[f"chain_{_N}"] = dict(id=f"chain_{_N}", code=f"chain_{_N}", chain=_N, p=0.1, max_iter=2, shots=1, rng=0)


def order_kw(method="lsd_0", order=0, min_free_bits=0, grow_bits_limit=256):
    return (("method", method), ("order", order), ("min_free_bits", min_free_bits), ("grow_bits_limit", grow_bits_limit))


# (case, order settings)
TABLE = [
    ("hgp_rep5", order_kw("lsd_cs", 4, 4)),
    ("hgp_rep5", order_kw("lsd_cs", 7, 8)),
    ("hgp_rep5", order_kw("lsd_cs", 7, 0)),
    ("hgp_rep5", order_kw("lsd_e", 5, 4)),
    ("dense_dc20_dv9", order_kw("lsd_cs", 7, 0)),
    ("dense_dc20_dv9", order_kw("lsd_cs", 7, 8)),
    ("reg300_weak", order_kw("lsd_cs", 7, 0)),
    ("chain_248", order_kw("lsd_cs", 7, 8)),
    ("chain_248", order_kw("lsd_e", 8, 8)),
    ("chain_249", order_kw("lsd_cs", 7, 8)),
    ("chain_249", order_kw("lsd_e", 8, 8)),
    ("chain_192", order_kw("lsd_0", 0, 8)),
    ("chain_192", order_kw("lsd_0", 0, 8, 196)),
    ("chaindup_156", order_kw("lsd_cs", 7, 0)),
    ("reg1000", order_kw("lsd_0", 0, 4, 24)),
]
# what the reference gives on the open shots of a row, tie policy 0, LSD uncapped (None: not asserted); `exact` rows are
# asserted as equalities under both tie policies (the chains have no tied LLRs among the bits that matter), the others as
# equalities under tie policy 0 and as "at least one" / "at most" under tie policy 1
EXPECT = {
    0: dict(open=142, improved=3, max_free=8),
    1: dict(open=142, improved=3, max_free=13),
    2: dict(open=142, improved=0, max_free_at_most=2),
    4: dict(open=85, improved=3, max_free=9),
    5: dict(open=85, improved=10),
    6: dict(improved=1, four_words=True, tie0_only=True),  # (a single shot: nothing is claimed under the other tie policy)
    7: dict(exact=True, status=0, max_bits=256, max_free=8, w0=248, ww=1),
    8: dict(exact=True, status=0, max_bits=256, max_free=8, w0=248, ww=1),
    9: dict(exact=True, status=0, max_bits=256, max_free=7, improved=0),
    10: dict(exact=True, status=0, max_bits=256, max_free=7, improved=0),
    11: dict(exact=True, status=0, max_bits=200, max_free=8),
    12: dict(exact=True, status=0),
    13: dict(exact=True, status=0, max_bits=256, max_free=100, improved=0),
    14: dict(open=63, status1=58),
}
# (osd_method, osd_order, sort_tie_policy)
RUNS = [("osd_cs", 7, 0), ("osd_off", 0, 1), ("osd_cs", 7, 1), ("osd_off", 0, 0)]

# ---- the fp64 cases
# dense_dc20_dv9 with a two-valued channel: bit i of shot b has probability ALT_P where sel[b, i] is set, the case's p
# elsewhere (decode_batch(prior_select=, alt_channel_probs=))
TWO_VALUED = dict(case="dense_dc20_dv9", order=order_kw("lsd_cs", 7, 8), alt_p=0.2, density=0.3, seed=1)
# hgp_rep5 with a channel row per shot (decode_batch(channel_probs_rows=)): p * 3^u, u uniform in [-1, 1]
ROWS = dict(case="hgp_rep5", order=order_kw("lsd_cs", 7, 8), seed=1)


def row_id(row):
    k = dict(row[1])
    return f"{row[0]}_{k['method']}{k['order']}_free{k['min_free_bits']}_grow{k['grow_bits_limit']}"


def run_id(run):
    return f"{run[0]}{run[1]}_tie{run[2]}"


def config_of(order, bits=lc.LSD_MAX, checks=lc.LSD_MAX):
    from bp_osd_amd import LsdConfig

    return LsdConfig(bits, checks, **dict(order))


def matrix(case_id):
    return lc.matrix(CASE_BY_ID[case_id]["code"])


@functools.lru_cache(maxsize=None)
def syndromes(case_id):
    if case_id in lc.CASE_BY_ID:
        return lc.syndromes(case_id)
    S = np.zeros((2, matrix(case_id).shape[0]), np.uint8)  # a chain: e_0, then the all-zero syndrome
    S[0, 0] = 1
    S.setflags(write=False)
    return S


def settings(case_id, run):
    return lc.settings(CASE_BY_ID[case_id], (0, 0) + tuple(run))


def cost_of(kw):
    """log(1/p) of the channel of ``settings`` where the OSD stage sums it, None where it counts bits."""
    import math

    if "channel_probs" not in kw:
        return None
    return np.array([math.log(1 / float(p)) for p in kw["channel_probs"]])


@functools.lru_cache(maxsize=None)
def reference(case_id, order, run):
    """``LsdReferenceDecoder`` around the CPU oracle on the case's syndromes."""
    ref = lc.reference_decoder(matrix(case_id), lsd=config_of(order), **settings(case_id, run)).decode_batch(syndromes(case_id))
    for v in ref.values():
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def open_shots(case_id, tie=0):
    """(open shot indices, their syndromes, their LLRs) after the oracle's BP."""
    from oracle import OracleDecoder

    S = syndromes(case_id)
    bp = OracleDecoder(matrix(case_id), **settings(case_id, ("osd_off", 0, tie))).decode_batch(S)
    open_ = np.flatnonzero(bp["converged"] == 0)
    return open_, S[open_], bp["llr"][open_]


@functools.lru_cache(maxsize=None)
def uncapped(case_id, order, tie=0):
    """The definition under the ceilings as caps on the shots BP leaves open (dict of lsd_decode_reference)."""
    from bp_osd_amd import lsd_decode_reference

    _, S, llr = open_shots(case_id, tie)
    return lsd_decode_reference(matrix(case_id), S, llr, config_of(order), tie, cost=cost_of(settings(case_id, ("osd_off", 0, tie))))


@functools.lru_cache(maxsize=None)
def two_valued_channel():
    """(sel uint8 [B, n], alt float64 [n]) of TWO_VALUED."""
    c = TWO_VALUED
    H = matrix(c["case"])
    B = len(syndromes(c["case"]))
    sel = (np.random.default_rng(c["seed"]).random((B, H.shape[1])) < c["density"]).astype(np.uint8)
    sel.setflags(write=False)
    return sel, np.full(H.shape[1], c["alt_p"])


@functools.lru_cache(maxsize=None)
def channel_rows():
    """float64 [B, n] of ROWS."""
    c = ROWS
    H = matrix(c["case"])
    B = len(syndromes(c["case"]))
    p = CASE_BY_ID[c["case"]]["p"]
    P = np.clip(p * np.exp(np.random.default_rng(c["seed"]).uniform(-1, 1, (B, H.shape[1])) * np.log(3)), 1e-3, 0.4)
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def per_shot_reference(which, run=RUNS[0]):
    """The reference of an fp64 case, a decoder per shot (the oracle has one channel per handle): ``which`` is "two_valued"
    or "rows".  Returns (reference dict, the channel [B, n])."""
    c = TWO_VALUED if which == "two_valued" else ROWS
    H, S = matrix(c["case"]), syndromes(c["case"])
    if which == "two_valued":
        sel, alt = two_valued_channel()
        P = np.where(sel != 0, alt[None, :], CASE_BY_ID[c["case"]]["p"])
    else:
        P = channel_rows()
    kw = {k: v for k, v in settings(c["case"], run).items() if k != "error_rate"}
    keys = None
    want = {}
    for b in range(len(S)):
        r = lc.reference_decoder(H, lsd=config_of(c["order"]), channel_probs=P[b], **kw).decode_batch(S[b:b + 1])
        keys = keys or [k for k in r if r[k] is not None]
        for k in keys:
            want.setdefault(k, []).append(r[k])
    want = {k: np.concatenate(v) for k, v in want.items()}
    for v in want.values():
        v.setflags(write=False)
    return want, P
