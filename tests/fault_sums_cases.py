"""The shapes, rows and references of tests/test_fault_sums_cpu.py and tests/test_gpu_fault_sums.py: the per-fault sums over
selected shots of the detector-error-model engine and the cross-entropy fit built on them.

``dense_sums`` restates the definition on unpacked rows with Python integers, independently of the package's own
``fault_sums_batch``.  Whole-run references come from ``engine="numpy"`` around the CPU oracle -- never from rows a GPU
produced.  Every reference is computed once per process (lru_cache) and handed out read-only.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import dem_cases as dc
from tests import dem_weight_cases as wc
from tests import harvest_cases as hc

TILE_COLS = 4096  # faults of one column tile of fault_sums_kernel (FS_TILE_COLS: 64 words, one per lane); the CPU test reads the header
LIST_TILE = hc.LIST_TILE  # rows of one tile of harvest_list_kernel
MULT_VALUES = (0, 1, 2 ** 31, 2 ** 32 - 1)
MULT_MAX = 2 ** 32 - 1
ONES_ROWS = 6  # all-ones rows with the largest multiplier among the selected: five already carry a column sum past 2^32

# ------------------------------------------------------------------------------------------------------- the kernel alone
# (N, B, select, rows): the shapes at which fault_sums_kernel can go wrong.  A workgroup is 4 waves, a selected row each;
# lane l reads word tile + l of a row, so N decides which lanes read and how many column tiles (grid x) there are.  The
# row list is cut into chunks (grid y) of at least 64 rows, at most 2 per CU = 512 on an MI355X: a case with F <= 64 runs in
# one chunk, one with 64 < F <= 32768 in ceil(F / 64) chunks of 64 and a shorter last one, and beyond that in 512 chunks of
# more than 64 rows.  `select`: a density, "none", "one" or "all" -- the bytes the list is made from ("ends" adds the first
# and the last row); the implicit form of the kernel takes every row whatever the bytes say.  `rows`: "sparse" (3 % set,
# with ONES_ROWS all-ones rows at multiplier 2^32 - 1 and three zero rows among the selected) or "ones" (every row all-ones:
# every lane of every wave adds to the same LDS words).
KERNEL_CASES = [
    dict(id="n1-b1", N=1, B=1, select="all", rows="sparse"),                  # the smallest shape: one bit, one row, one lane reads
    dict(id="n63", N=63, B=1000, select=0.3, rows="sparse"),                  # one word, one bit short
    dict(id="n64", N=64, B=1000, select=0.3, rows="sparse"),                  # exactly one word
    dict(id="n65", N=65, B=1000, select=0.3, rows="sparse"),                  # one bit into the second word: lane 1 reads one bit
    dict(id="n129", N=129, B=1000, select=0.3, rows="sparse"),                # three words, the last holds one bit
    dict(id="tile", N=TILE_COLS, B=300, select=0.5, rows="sparse"),           # exactly one column tile: all 64 lanes read
    dict(id="tile+1", N=TILE_COLS + 1, B=300, select=0.5, rows="sparse"),     # a second column tile of one bit: grid x = 2
    dict(id="b1", N=65, B=1, select="all", rows="ones"),                      # one row, all ones
    dict(id="list-1", N=65, B=LIST_TILE - 1, select=0.01, rows="sparse", ends=True),  # one row short of a list tile
    dict(id="list", N=65, B=LIST_TILE, select=0.01, rows="sparse", ends=True),        # exactly one list tile
    dict(id="list+1", N=65, B=LIST_TILE + 1, select=0.01, rows="sparse", ends=True),  # a second list tile of one row
    dict(id="none", N=65, B=1000, select="none", rows="sparse"),              # F = 0: nothing is launched, zeros come down
    dict(id="one", N=65, B=1000, select="one", rows="sparse"),                # F = 1
    dict(id="all-16385", N=65, B=LIST_TILE + 1, select="all", rows="sparse"), # F = B: 257 chunks, the last of one row
    dict(id="all-40000", N=65, B=40000, select="all", rows="sparse"),         # more rows than 512 chunks of 64: chunks of 79, the last shorter
    dict(id="ones", N=129, B=300, select="all", rows="ones"),                 # every lane of every wave hits the same LDS words; sums of 300 (2^32 - 1)
]
KERNEL_BY_ID = {c["id"]: c for c in KERNEL_CASES}
KERNEL_NS = sorted({c["N"] for c in KERNEL_CASES})


@functools.lru_cache(maxsize=None)
def kernel_rows(case_id):
    """(fault bits uint8 [B, N], select bytes uint8 [B], multipliers uint32 [B]) of a case, seeded by the case.  The
    multiplier of a row goes with the row: the listed form passes ``mult[select != 0]``, the implicit form all of it."""
    c = KERNEL_BY_ID[case_id]
    N, B = c["N"], c["B"]
    rng = np.random.default_rng(4000 + KERNEL_CASES.index(c))
    if c["select"] == "none":
        select = np.zeros(B, np.uint8)
    elif c["select"] == "all":
        select = rng.integers(1, 256, size=B).astype(np.uint8)  # any non-zero byte selects
    elif c["select"] == "one":
        select = np.zeros(B, np.uint8)
        select[B // 3] = 7
    else:
        select = (rng.random(B) < c["select"]).astype(np.uint8) * rng.integers(1, 256, size=B).astype(np.uint8)
    if c.get("ends"):
        select[0] = select[B - 1] = 1
    mult = rng.choice(MULT_VALUES + (12345, 2 ** 31 - 1), size=B).astype(np.uint64)
    if c["rows"] == "ones":
        faults = np.ones((B, N), np.uint8)
        mult[:] = MULT_MAX
    else:
        faults = (rng.random((B, N)) < 0.03).astype(np.uint8)
        picked = np.flatnonzero(select) if np.count_nonzero(select) >= ONES_ROWS + 3 else np.arange(B)  # ("none", "one": among all rows)
        picked = picked[rng.permutation(picked.size)]
        ones, zeros = picked[:ONES_ROWS], picked[ONES_ROWS:ONES_ROWS + 3]
        faults[ones] = 1
        mult[ones] = MULT_MAX
        faults[zeros] = 0
    mult = mult.astype(np.uint32)
    for a in (faults, select, mult):
        a.setflags(write=False)
    return faults, select, mult


def dense_sums(bits, mult):
    """(counts, sums) of unpacked rows ``bits`` uint8 [F, N] and multipliers [F] as ``bits.T @ mult``: int64 products of the
    16-bit halves of the multipliers (each below 2^47 for F < 2^31), put together in Python integers.  Nothing shared with
    the package's restatement."""
    b = np.asarray(bits, dtype=np.int64)
    m = np.asarray(mult, dtype=np.uint64).astype(np.int64)
    lo, hi = b.T @ (m & 0xFFFF), b.T @ (m >> 16)
    sums = [int(a) + (int(h) << 16) for a, h in zip(lo.tolist(), hi.tolist())]
    counts = [int(v) for v in b.sum(axis=0).tolist()]
    return np.array(counts, dtype=np.uint64), np.array(sums, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def kernel_reference(case_id, form):
    """(rows, counts, sums) of the case: ``form`` "listed" takes the rows the select bytes name, "all" every row."""
    faults, select, mult = kernel_rows(case_id)
    rows = np.flatnonzero(select).astype(np.int32) if form == "listed" else np.arange(faults.shape[0], dtype=np.int32)
    counts, sums = dense_sums(faults[rows], mult[rows])
    for a in (rows, counts, sums):
        a.setflags(write=False)
    return rows, counts, sums


# ------------------------------------------------------------------------------------------------------------- whole runs
STATS_HARVEST = 4
SPLIT = (0.25, 0.25, 0.5)  # a run in three batches


def split_sizes(B):
    a, b = int(B * SPLIT[0]), int(B * SPLIT[1])
    return a, b, B - a - b


def stats_sim(case_id, engine, batch_size=None, run_sim=True, **more):
    """dem_decode_sim on a dem_cases.RUN_CASES model with fault_stats on ("numpy": around the CPU oracle)."""
    from bp_osd_amd.dem import dem_decode_sim
    from oracle import OracleDecoder

    c = dc.RUN_BY_ID[case_id]
    H, L, priors = dc.run_model(case_id)
    opts = dict(dc.DECODER)
    if engine == "numpy":
        opts["decoder_factory"] = OracleDecoder
    opts.update(more)
    return dem_decode_sim(H, L, priors, batch_size=batch_size or c["B"], engine=engine, seed=dc.RUN_SEED, target_runs=c["B"], run_sim=run_sim,
                          harvest=STATS_HARVEST, fault_stats=True, **opts)


@functools.lru_cache(maxsize=None)
def stats_reference(case_id):
    """(fault_counts, failure_fault_counts) of the case in one batch on the oracle, and the same two from the fetched rows
    -- the column sums of item "faults" over all shots and over the shots flagged as osdw failures."""
    sim = stats_sim(case_id, "numpy")
    N = sim.N
    bits = dc.unpack(sim.last_batch("faults"), N)
    fail = (sim.last_batch("flags") & 4) != 0
    out = dict(fault_counts=np.array(sim.fault_counts), failure_fault_counts=np.array(sim.failure_fault_counts),
               from_rows=bits.sum(axis=0, dtype=np.int64), from_failing_rows=bits[fail].sum(axis=0, dtype=np.int64), failures=int(fail.sum()))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tilted_reference(case_id):
    """(multipliers, counts, sums, rows) of fault_sums("failing", v) after one batch of the case with
    sample_scale = dem_weight_cases.RUN_SCALE on the oracle, v the multipliers of the failing shots' log-weights."""
    from bp_osd_amd.dem import weight_multipliers

    sim = stats_sim(case_id, "numpy", sample_scale=wc.RUN_SCALE)
    rows = np.array(sim.last_batch("fail_rows"))
    v = weight_multipliers(sim.last_batch("logw")[rows])
    counts, sums = sim.fault_sums("failing", v)
    for a in (v, counts, sums, rows):
        a.setflags(write=False)
    return v, counts, sums, rows


# ------------------------------------------------------------------------------------------------------------------ the fit
@functools.lru_cache(maxsize=None)
def oracle_fit(seed, batch_size=4096):
    """fit_sample_priors with its default arguments on dem_weight_cases.exact_model(), oracle engine."""
    from bp_osd_amd.dem import fit_sample_priors
    from oracle import OracleDecoder

    H, L, p = wc.exact_model()
    q, report = fit_sample_priors(H, L, p, engine="numpy", seed=seed, batch_size=batch_size, decoder_factory=OracleDecoder, **dc.DECODER)
    q.setflags(write=False)
    return q, report
