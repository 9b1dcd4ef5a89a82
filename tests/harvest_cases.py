"""The shapes, rows and numpy references of tests/test_harvest_cpu.py and tests/test_gpu_harvest.py: the harvest of failing
shots of the detector-error-model engines.

``numpy_harvest`` restates the definition on packed words, independently of the package's own ``harvest_batch``.  Whole-run
references come from ``engine="numpy"`` around the CPU oracle, with a decoder subclass that remembers what it decoded so
that a residual can be recomputed from rows the test keeps -- never from rows a GPU produced.  Every reference is computed
once per process (lru_cache) and handed out read-only.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import dem_cases as dc
from tests import window_cases as wc

LIST_TILE = 16384  # rows of one tile of harvest_list_kernel: 1024 threads x 16 flag bytes
ITEMS = ("fail_rows", "fail_weight", "fail_residual", "fail_faults", "min_residual")
RESULTS = ("min_logical_weight", "min_logical_shot", "min_logical_fault", "failure_weight_counts")

# ------------------------------------------------------------------------------------------------------- the kernels alone
# (N, B, K, select, special): the shapes at which the three kernels can go wrong.  harvest_list_kernel is one workgroup that
# walks tiles of 16384 flag bytes, 16 per thread, and takes the bytes of a thread's group one by one where the group
# crosses B; harvest_rows_kernel gives a wave to a listed shot (4 per workgroup, grid-stride beyond 8 workgroups per CU =
# 8192 listed shots on an MI355X) and a lane the words l, l + 64, ...; a byte row is packed 8 bytes at a time with a tail.
# `select`: a density, "none" or "all".  `special` builds rows for one property of the minimum (see kernel_rows).
KERNEL_CASES = [
    dict(id="n1-b1", N=1, B=1, K=1, select="all", special=None),             # the smallest shape: one bit, one row, a group of one byte
    dict(id="n63", N=63, B=4101, K=50, select=0.3, special=None),            # one word, one bit short; byte rows end in a 7-byte tail; B is no multiple of 16
    dict(id="n64", N=64, B=4101, K=50, select=0.3, special=None),            # exactly one word, no tail
    dict(id="n65", N=65, B=4101, K=50, select=0.3, special=None),            # one bit into the second word; byte rows start at odd addresses
    dict(id="n4097-b300", N=4097, B=300, K=300, select=0.5, special=None),   # 65 words: lane 0 takes a second word, and the last word holds one bit
    dict(id="tile-1", N=65, B=LIST_TILE - 1, K=8, select=0.01, special="ends"),  # one row short of a tile: the last thread's group crosses B
    dict(id="tile", N=65, B=LIST_TILE, K=8, select=0.01, special="ends"),        # exactly one tile
    dict(id="tile+1", N=65, B=LIST_TILE + 1, K=8, select=0.01, special="ends"),  # a second tile of one row: the running base, the other LDS row
    dict(id="none", N=65, B=4101, K=5, select="none", special=None),         # nothing selected: (0, -1, -1), zeros
    dict(id="all-K4101", N=65, B=4101, K=4101, select="all", special=None),  # every row listed and kept
    dict(id="all-K7", N=65, B=4101, K=7, select="all", special=None),        # ... kept up to slot 7 only, weights for all
    dict(id="all-K1", N=65, B=4101, K=1, select="all", special=None),        # ... the smallest cap
    dict(id="all-9000", N=130, B=9000, K=3, select="all", special=None),     # more listed shots than waves in the grid: the grid-stride of harvest_rows_kernel
    dict(id="tie", N=130, B=4101, K=50, select=0.3, special="tie"),          # the least weight at three rows: the lowest wins
    dict(id="last", N=130, B=4101, K=50, select=0.3, special="last"),        # the least weight only at the last selected row
    dict(id="beyond", N=130, B=4101, K=3, select=0.3, special="beyond"),     # the least weight at a slot beyond K
]
KERNEL_BY_ID = {c["id"]: c for c in KERNEL_CASES}
KERNEL_NS = sorted({c["N"] for c in KERNEL_CASES})
LIGHT = 2  # weight of the rows that `special` makes the lightest; every other selected row is made heavier


@functools.lru_cache(maxsize=None)
def kernel_rows(case_id):
    """(fault bits, correction bits, select) of a case, uint8 [B, N], [B, N], [B], seeded by the case."""
    c = KERNEL_BY_ID[case_id]
    N, B = c["N"], c["B"]
    rng = np.random.default_rng(1000 + KERNEL_CASES.index(c))
    faults = (rng.random((B, N)) < 0.1).astype(np.uint8)
    diff = (rng.random((B, N)) < 0.3).astype(np.uint8)
    if c["select"] == "none":
        select = np.zeros(B, np.uint8)
    elif c["select"] == "all":
        select = np.ones(B, np.uint8)
    else:
        select = (rng.random(B) < c["select"]).astype(np.uint8) * rng.integers(1, 256, size=B).astype(np.uint8)  # any non-zero byte selects
    if c["special"] == "ends":
        select[0] = select[B - 1] = 1
    if c["special"] in ("tie", "last", "beyond"):
        heavy = np.flatnonzero(diff.sum(axis=1) <= LIGHT)
        diff[heavy, :LIGHT + 1] = 1  # nobody else is as light
        rows = np.flatnonzero(select)
        at = {"tie": rows[[40, 7, 90]], "last": rows[-1:], "beyond": rows[[c["K"] + 4]]}[c["special"]]
        diff[at] = 0
        for i, b in enumerate(at):
            diff[b, [3 + i, 70 + i]] = 1
    for a in (faults, diff, select):
        a.setflags(write=False)
    return faults, faults ^ diff, select


def numpy_harvest(fault_words, corr_words, select, K):
    """The harvest restated on packed rows (uint64 [B, fw] each): a dict of the five items and ``info`` = (count, min weight,
    min row).  Python integers and a loop for the minimum: nothing shared with the package's restatement."""
    f, c = np.asarray(fault_words, dtype="<u8"), np.asarray(corr_words, dtype="<u8")
    rows = [b for b in range(len(select)) if select[b]]
    res = [f[b] ^ c[b] for b in rows]
    weight = [sum(bin(int(w)).count("1") for w in r) for r in res]
    fw = f.shape[1]
    keep = min(len(rows), K)
    best = None
    for slot, w in enumerate(weight):
        if best is None or w < weight[best]:
            best = slot
    return {"fail_rows": np.array(rows, np.int32), "fail_weight": np.array(weight, np.int32),
            "fail_residual": np.array(res[:keep], "<u8").reshape(keep, fw), "fail_faults": np.array([f[b] for b in rows[:keep]], "<u8").reshape(keep, fw),
            "min_residual": np.zeros(fw, "<u8") if best is None else res[best],
            "info": (len(rows), -1 if best is None else weight[best], -1 if best is None else rows[best])}


@functools.lru_cache(maxsize=None)
def kernel_reference(case_id):
    c = KERNEL_BY_ID[case_id]
    faults, corr, select = kernel_rows(case_id)
    out = numpy_harvest(dc.pack(faults), dc.pack(corr), select, c["K"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def chain_model(N):
    """(H, L, priors) with N faults for an engine the kernels alone run on: checks on neighbouring faults, one observable."""
    import scipy.sparse as sp

    M = max(1, min(N - 1, 12))
    H = np.zeros((M, N), np.uint8)
    for i in range(M):
        H[i, i] = H[i, min(i + 1, N - 1)] = 1
    L = np.ones((1, N), np.uint8)
    return sp.csr_matrix(H), sp.csr_matrix(L), np.full(N, 0.05)


# ------------------------------------------------------------------------------------------------------------- whole runs
# The figures of the issue, computed on the CPU oracle (seed 5, one batch); tests/test_harvest_cpu.py recomputes them.
#   kind "dem": dem_decode_sim on dem_cases' model `model`; "window": windowed_dem_decode_sim on window_cases' model.
#   failures, the first failing rows, the lightest weights in ascending order (None: not pinned), the least weight, the rows
#   that have it (a prefix of them) and how many have it (None: not pinned).
RUN_CASES = [
    dict(id="surface13-R3", kind="dem", model="surface13-R3", B=256, kw={}, failures=44, first=(5, 6, 17, 20, 28, 38, 42, 77, 78, 79),
         weights=(3,) * 10, min_weight=3, tied=(17, 94, 98, 106, 153), lightest=10),
    dict(id="hgp400-R1", kind="dem", model="hgp400-R1", B=128, kw={}, failures=5, first=(5, 69, 78, 102, 125), weights=(8, 8, 8, 22, 26),
         min_weight=8, tied=(5, 69, 125), lightest=3),
    dict(id="hgp400-R3", kind="dem", model="hgp400-R3", B=64, kw={}, failures=2, first=(55, 60), weights=(18, 36), min_weight=18, tied=(55,), lightest=1),
    dict(id="surface13-R3-serial", kind="dem", model="surface13-R3", B=256, kw=dict(schedule="serial"), failures=46, first=None, weights=None,
         min_weight=3, tied=(17,), lightest=None),
    dict(id="random-520", kind="dem", model="random-520-129-65", B=200, kw={}, failures=37, first=None, weights=None, min_weight=2,
         tied=(26, 44, 124), lightest=3),
    dict(id="surface13-R3-w21", kind="window", model="surface13-R3", window=(2, 1), B=256, kw={}, failures=45, first=None, weights=None,
         min_weight=3, tied=(17,), lightest=None),
    dict(id="hgp400-R3-w21", kind="window", model="hgp400-R3", window=(2, 1), B=64, kw={}, failures=3, first=None, weights=(13, 15, 18),
         min_weight=13, tied=(23,), lightest=1),
    dict(id="random-520-w21", kind="window", model="random-520-129-65", window=(2, 1), B=200, kw={}, failures=171, first=None, weights=None,
         min_weight=2, tied=(44, 124), lightest=2),
]
RUN_BY_ID = {c["id"]: c for c in RUN_CASES}


def model(case):
    """(H, L, priors, detector times or None) of a run case."""
    if case["kind"] == "window" or case["model"] not in dc.RUN_BY_ID:
        return wc.model(case["model"])
    return dc.run_model(case["model"]) + (None,)


def keeping_oracle():
    """(factory, kept): an OracleDecoder factory whose decoders append every ``decode_batch`` result (the osdw rows) to
    ``kept``, in call order."""
    from oracle import OracleDecoder

    kept = []

    class Keeping(OracleDecoder):
        def decode_batch(self, syndromes):
            rows = super().decode_batch(syndromes)
            kept.append(np.array(rows["osdw"] if isinstance(rows, dict) else rows, dtype=np.uint8))
            return rows

    return Keeping, kept


def sim(case, engine, harvest, batch_size=None, run_sim=True, factory=None, **more):
    """The harness of a run case on ``engine`` ("numpy": around the CPU oracle, or ``factory``)."""
    from bp_osd_amd.dem import dem_decode_sim
    from bp_osd_amd.window import windowed_dem_decode_sim
    from oracle import OracleDecoder

    H, L, priors, times = model(case)
    opts = dict(dc.DECODER)
    opts.update(case["kw"])
    opts.update(more)
    if engine == "numpy":
        opts["decoder_factory"] = factory or OracleDecoder
    common = dict(batch_size=batch_size or case["B"], engine=engine, seed=dc.RUN_SEED, target_runs=case["B"], run_sim=run_sim, harvest=harvest)
    if case["kind"] == "window":
        return windowed_dem_decode_sim(H, L, priors, times, case["window"], **common, **opts)
    return dem_decode_sim(H, L, priors, **common, **opts)


def snapshot(s):
    """The results of a harvest and the items of the last batch, copied and read-only."""
    out = {k: getattr(s, k) for k in RESULTS}
    out["failures"] = {k: np.array(v) for k, v in s.failures.items()}
    out["items"] = {k: np.array(s.last_batch(k)) for k in ITEMS}
    out["flags"] = np.array(s.last_batch("flags"))
    out["faults"] = np.array(s.last_batch("faults"))
    out["output"] = s.output_dict()
    for v in list(out["failures"].values()) + list(out["items"].values()) + [out["flags"], out["faults"], out["min_logical_fault"],
                                                                           out["failure_weight_counts"]]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def run_reference(case_id):
    """The case in one batch on the oracle with every failing row kept (harvest = B)."""
    case = RUN_BY_ID[case_id]
    return snapshot(sim(case, "numpy", case["B"]))
