"""The plan of tests/test_gpu_park_forms.py, shared with tests/test_park_forms_cpu.py (which asserts it without a GPU).

tests/local_park_cases.py parks shots of one kind of call: a uniform channel, a constant scaling factor, OSD-0 behind BP.
The continuation of a parked shot reads three things that are not in its record -- the priors (from ``llr0[bit]``, from
row ``s`` of ``llr0_rows`` or through ``sel[s]``, with ``s`` the shot index the record holds), the scaling factor (from the
iteration the record holds) and, behind both launches, whatever stage consumes BP's list and LLR rows -- and this plan
parks shots under every one of them.

A *setting* says how the channel reaches the kernel:

    bit       ``channel_probs=`` non-uniform (q 4^u, u uniform in [-1, 1], two entries exactly 0.5): UPRIOR = false, the
              prior comes from ``llr0[bit]``; byte and packed calls
    rows      ``d_prior_llr_rows`` + ``d_cost_rows`` on a handle whose own channel is uniform q: row ``s`` of the caller's
    sel       ``d_prior_select`` + ``alt_channel_probs`` on a handle whose own channel is the per-bit one
    varscale  uniform q with ``ms_scaling_factor=0.0`` (1 - 2^-iteration): UPRIOR = true, the factor is recomputed from
              the restored iteration

Under every setting a shot's *effective channel* is one of at most N_ROWS distinct probability rows ``R[k]`` (one row for
bit and varscale; eight drawn rows for rows; ``where(sel_k, alt, base)`` for eight drawn select rows), so the oracle
decodes one batch per row: ``update_channel_probs(R[k])``, then the shots of that row -- the documented way to decode a
shot with a channel of its own, as tests/channel_rows_cases.py does it shot by shot.

The pool of a (matrix, setting) pair (``plan``): N_POOL (syndrome, row) pairs -- candidate c of the seeded ``H e``
syndromes of tests/local_codes.py goes with row c mod N_ROWS -- scanned by the oracle at max_iter 2 CH + 8: the zero
syndrome, the first candidates the oracle converges in exactly CH - 1, CH and CH + 1 iterations under their row, the first
it gives up on, up to N_LATE further candidates that cross the first chunk boundary (iters >= CH: they are what parks, and
what the sensitivity condition counts), and ordinary candidates up to N_POOL.  The batch repeats the pool with period
N_POOL and so do its channel rows: batch row b has syndrome and channel of pool row b mod N_POOL.

``reference`` decodes the pool at one max_iter with one OSD / LSD stage behind BP; it is computed once per process and
handed out read-only.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

from tests.local_codes import matrix_of, row_by_id, syndrome_seed, syndromes
from tests.local_park_cases import B_2048, B_ONE, B_TWO, CH, N_POOL, _row_pair_and_generic, batch_index, crosses

MAX_ITERS = (CH, CH + 1, 2 * CH, 2 * CH + 8)  # CH: the control, nothing may park
SCAN = 2 * CH + 8
N_ROWS = 8
N_LATE = 8
B_EXACT = 128  # at most one shot per workgroup of any grid
SETTINGS = ("bit", "rows", "sel", "varscale")
PAIR_ROW = _row_pair_and_generic()
SMALL_CALL = 40000  # launch_bp_local: at most this many shots take one check per thread at 1024 positions


# ------------------------------------------------------------------------------------------------ channels
def per_bit_probs(q, n, seed):
    """q 4^u with u uniform in [-1, 1], two entries exactly 0.5 (prior LLR exactly 0: the `<= 0` tie of the decision)."""
    rng = np.random.default_rng(seed)
    p = q * np.exp(rng.uniform(-1, 1, n) * np.log(4))
    p[rng.choice(n, 2, replace=False)] = 0.5
    return p


@functools.lru_cache(maxsize=None)
def channel(row_id, setting):
    """dict(ctor: the channel keywords of the handle, ms: its scaling factor, R float64 [K, n]: the effective rows,
    sel uint8 [K, n] and alt float64 [n] (sel only), other float64 [n]: the channel a continuation that took the
    handle's own priors -- for ``bit``, the scalar prior of a uniform channel -- would decode with)."""
    row = row_by_id(row_id)
    q, n = row["q"], 2 * row["m"]
    base = per_bit_probs(q, n, 21)
    out = dict(ms=0.625, sel=None, alt=None)
    if setting == "bit":
        out.update(ctor=dict(channel_probs=base), R=base[None], other=np.full(n, q))
    elif setting == "rows":
        out.update(ctor=dict(error_rate=q), R=np.stack([per_bit_probs(q, n, 30 + k) for k in range(N_ROWS)]), other=np.full(n, q))
    elif setting == "sel":
        rng = np.random.default_rng(22)
        sel = (rng.random((N_ROWS, n)) < 0.25).astype(np.uint8)
        alt = rng.uniform(0.02, 0.3, n)
        out.update(ctor=dict(channel_probs=base), R=np.where(sel != 0, alt, base), sel=sel, alt=alt, other=base)
    elif setting == "varscale":
        out.update(ctor=dict(error_rate=q), ms=0.0, R=np.full((1, n), q), other=None)
    else:
        raise ValueError(setting)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def uprior(setting):
    """launch_bp_local: one finite positive prior below 0.5 for every bit, no select bytes and no rows."""
    return setting == "varscale"


def settings(row_id, setting, max_iter, osd=("osd0", 0), tie=0):
    """Keywords of ``BpOsdDecoder`` and of the oracle alike."""
    ch = channel(row_id, setting)
    return dict(max_iter=max_iter, bp_method="ms", ms_scaling_factor=ch["ms"], osd_method=osd[0], osd_order=osd[1], sort_tie_policy=tie, **ch["ctor"])


def _by_row(dec, R, S, rows_of, **kw):
    """The reference decode: per distinct row k, ``update_channel_probs(R[k])`` then the shots that go with it."""
    out = None
    for k in range(len(R)):
        at = np.flatnonzero(rows_of == k)
        if at.size == 0:
            continue
        dec.update_channel_probs(R[k])
        r = dec.decode_batch(S[at], **kw)
        if out is None:
            out = {key: np.zeros((len(S),) + np.asarray(v).shape[1:], np.asarray(v).dtype) for key, v in r.items() if v is not None}
        for key in out:
            out[key][at] = r[key]
    return out


# ------------------------------------------------------------------------------------------------ the pool
@functools.lru_cache(maxsize=None)
def plan(row_id, setting):
    """dict(H, q, pool uint8 [N_POOL, m], rows int [N_POOL]: the effective row of every pool shot, edge {CH - 1, CH, CH + 1:
    pool row}, stuck (pool row), late [pool rows])."""
    from oracle import OracleDecoder

    row = row_by_id(row_id)
    H, q = matrix_of(row), row["q"]
    ch = channel(row_id, setting)
    K = len(ch["R"])
    # (shots of exactly CH - 1, CH and CH + 1 iterations are a few per thousand)
    cand = syndromes(H, q, 4096, syndrome_seed(row))
    cand_row = np.arange(len(cand)) % K
    scan = _by_row(OracleDecoder(H, **settings(row_id, setting, SCAN)), ch["R"], cand, cand_row, want_llr=False)
    conv, it = scan["converged"] != 0, scan["iters"]
    he = np.arange(len(cand)) >= 34  # (the candidates in front are the all-ones and uniformly random syndromes)
    picks = [0]
    edge = {}
    for k in (CH - 1, CH, CH + 1):
        hit = np.flatnonzero(he & conv & (it == k))
        assert hit.size, (row_id, setting, "no candidate converges in exactly", k, "iterations")
        edge[k] = len(picks)
        picks.append(int(hit[0]))
    hit = np.flatnonzero(he & ~conv)
    assert hit.size, (row_id, setting, "every candidate converges")
    stuck = len(picks)
    picks.append(int(hit[0]))
    # further shots that cross the boundary: late convergers first, then whatever else crosses
    late_conv = [i for i in np.flatnonzero(he & conv & (it >= CH)) if i not in picks][:N_LATE // 2]
    late_any = [i for i in np.flatnonzero(he & (it >= CH)) if i not in picks and i not in late_conv][:N_LATE - len(late_conv)]
    late = list(range(len(picks), len(picks) + len(late_conv) + len(late_any)))
    picks += [int(i) for i in late_conv + late_any]
    picks += [int(i) for i in np.flatnonzero(he & (it < CH)) if i not in picks][:N_POOL - len(picks)]
    assert len(picks) == N_POOL
    pool = np.ascontiguousarray(cand[picks])
    pool.setflags(write=False)
    rows = cand_row[picks]
    rows.setflags(write=False)
    return dict(H=H, q=q, pool=pool, rows=rows, edge=edge, stuck=stuck, late=late)


def lsd_config(spec):
    """None, or (method, order) of an ``LsdConfig`` with the default caps."""
    from bp_osd_amd import LsdConfig

    return None if spec is None else LsdConfig(method=spec[0], order=spec[1])


@functools.lru_cache(maxsize=None)
def reference(row_id, setting, max_iter, osd=("osd0", 0), tie=0, lsd=None, other=False):
    """The oracle's rows of the pool (``LsdReferenceDecoder`` around it with ``lsd``).  ``other``: every shot under
    ``channel(...)["other"]`` instead of its own row -- what a continuation with the wrong priors is near to."""
    from oracle import OracleDecoder

    p, ch = plan(row_id, setting), channel(row_id, setting)
    kw = settings(row_id, setting, max_iter, osd, tie)
    if lsd is not None:
        from bp_osd_amd import LsdReferenceDecoder

        dec = LsdReferenceDecoder(p["H"], lsd=lsd_config(lsd), base_factory=OracleDecoder, **kw)
        more = {}
    else:
        dec = OracleDecoder(p["H"], **kw)
        more = dict(want_llr=False)
    if other:
        ref = _by_row(dec, ch["other"][None], p["pool"], np.zeros(N_POOL, int), **more)
    else:
        ref = _by_row(dec, ch["R"], p["pool"], p["rows"], **more)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def planned_parks(row_id, setting, B, max_iter):
    """Shots of the batch that cross a boundary, by the oracle alone."""
    return int(crosses(reference(row_id, setting, max_iter)["iters"][batch_index(B)], max_iter).sum())


def parked_pool_rows(row_id, setting, max_iter):
    return np.flatnonzero(crosses(reference(row_id, setting, max_iter)["iters"], max_iter))


def sensitive_rows(row_id, setting, max_iter):
    """Pool rows that park at ``max_iter`` and whose iters, bp or osd0 differ under the other channel."""
    own, oth = reference(row_id, setting, max_iter), reference(row_id, setting, max_iter, other=True)
    differ = (own["iters"] != oth["iters"]) | (own["bp"] != oth["bp"]).any(axis=1) | (own["osd0"] != oth["osd0"]).any(axis=1)
    return np.flatnonzero(differ & crosses(own["iters"], max_iter))


# ------------------------------------------------------------------------------------------------ the device table
def expected_instance(row_id, setting, B, packed):
    """(("bp_local_kernel", (CPT, MP, MINW, EARLY), packed), pair body wanted, UPRIOR): the dispatch of launch_bp_local for
    bp_variant 0, restated -- 2048 positions have one shape; at 1024 a call of at most 40000 shots takes one check per
    thread, a larger one two with MINW 8 under the scalar prior and 6 without; the PAIRKEY instance where the layout has
    a (uniform key, mixed) wave and the call is not a small one."""
    row = row_by_id(row_id)
    up = uprior(setting)
    if row["MP"] == 2048:
        shape, pair = (2, 2048, 4, 0), row["pairkey"] >= 0
    elif B <= SMALL_CALL:
        shape, pair = (1, 1024, 8, 0), False
    else:
        shape, pair = (2, 1024, 8 if up else 6, 0), row["pairkey"] >= 0
    return ("bp_local_kernel", shape, bool(packed)), pair, up


# id, row of tests/local_codes.py, setting, the batch size that selects the shape, packed forms
CASES = [
    dict(row="reg64_s1", setting="bit", B=B_ONE, forms=(False, True)),
    dict(row="reg64_s1", setting="sel", B=B_ONE, forms=(False,)),
    dict(row="reg64_s1", setting="varscale", B=B_ONE, forms=(False,)),
    dict(row="reg65_s1", setting="rows", B=B_ONE, forms=(False,)),
    dict(row="reg128_s1", setting="bit", B=B_TWO, forms=(False, True)),
    dict(row="reg128_s1", setting="rows", B=B_TWO, forms=(False,)),
    dict(row=PAIR_ROW, setting="bit", B=B_TWO, forms=(False, True)),
    dict(row=PAIR_ROW, setting="sel", B=B_TWO, forms=(False,)),
    dict(row=PAIR_ROW, setting="varscale", B=B_TWO, forms=(False,)),
    dict(row="reg1900_s3", setting="bit", B=B_2048, forms=(False, True)),
    dict(row="reg1900_s3", setting="rows", B=B_2048, forms=(False,)),
]
for _c in CASES:
    _c["id"] = f"{_c['row']}-{_c['setting']}"
CASE_BY_ID = {c["id"]: c for c in CASES}

# Stages behind a parked BP, on one-check-per-thread call sizes: (id, row, setting, osd, tie, lsd, max_iters)
STAGE_ITERS = (CH + 1, 2 * CH + 8)  # restored straight into the LLR body; a second chunk and more
STAGES = [
    dict(id="osd_cs6-tie0", row="reg128_s1", setting="bit", osd=("osd_cs", 6), tie=0, lsd=None),
    dict(id="osd_cs6-tie1", row="reg128_s1", setting="bit", osd=("osd_cs", 6), tie=1, lsd=None),
    dict(id="osd_cs6-rows", row="reg128_s1", setting="rows", osd=("osd_cs", 6), tie=0, lsd=None),
    dict(id="lsd0-osd_cs7", row="reg128_s1", setting="bit", osd=("osd_cs", 7), tie=0, lsd=("lsd_0", 0)),
    dict(id="lsd0-osd_off", row="reg128_s1", setting="bit", osd=("osd_off", 0), tie=0, lsd=("lsd_0", 0)),
    dict(id="lsd_cs4-osd_cs7", row="reg128_s1", setting="bit", osd=("osd_cs", 7), tie=0, lsd=("lsd_cs", 4)),
]
STAGE_BY_ID = {s["id"]: s for s in STAGES}
STAGE_B = B_ONE
OBS_ROW, OBS_K = "reg64_s1", 65
REFUSAL_ROW = "reg64_s1"


def stage_reference(stage, max_iter):
    return reference(stage["row"], stage["setting"], max_iter, stage["osd"], stage["tie"], stage["lsd"])


@functools.lru_cache(maxsize=None)
def observable_matrix(n, k=OBS_K):
    """L uint8 [k, n], density 0.5 from default_rng(12): 65 rows are two observable words."""
    L = (np.random.default_rng(12).random((k, n)) < 0.5).astype(np.uint8)
    L.setflags(write=False)
    return L


def observables_packed(rows, L):
    """uint64 [B, ceil(k/64)]: (rows L^T) mod 2, bit (j & 63) of word (j >> 6) = observable j."""
    bits = ((np.asarray(rows).astype(np.int64) @ L.T.astype(np.int64)) & 1).astype(np.uint8)
    by = np.packbits(bits, axis=1, bitorder="little")
    out = np.zeros((bits.shape[0], 8 * ((bits.shape[1] + 63) // 64)), np.uint8)
    out[:, :by.shape[1]] = by
    return out.view("<u8")


# ------------------------------------------------------------------------------------------------ the DEM engine
DEM_B = B_ONE
DEM_KW = dict(batch_size=DEM_B, seed=5, target_runs=DEM_B, bp_method="ms", ms_scaling_factor=0.625, max_iter=2 * CH + 8, osd_method="osd_cs", osd_order=6)


@functools.lru_cache(maxsize=None)
def dem_model():
    """(H, L, priors): a local-kernel check matrix as the detector matrix, 65 seeded observables, non-uniform priors."""
    row = row_by_id("reg64_s1")
    H = matrix_of(row)
    return H, sp.csr_matrix(observable_matrix(H.shape[1])), channel("reg64_s1", "bit")["R"][0]


@functools.lru_cache(maxsize=None)
def dem_reference():
    """``dem_decode_sim(engine="numpy")`` around the CPU oracle, one batch."""
    from bp_osd_amd import dem_decode_sim
    from oracle import OracleDecoder

    H, L, priors = dem_model()
    return dem_decode_sim(H, L, priors, engine="numpy", decoder_factory=OracleDecoder, **DEM_KW)
