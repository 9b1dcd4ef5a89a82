"""Per-fault sums over selected shots on the MI355X (bposd_dem_fault_sums, ``fault_sums`` / ``fault_stats`` /
``fit_sample_priors`` of bp_osd_amd.dem): fault_sums_kernel alone on seeded rows against dense integer
arithmetic, whole runs and the cross-entropy fit against the CPU oracle, and switching, byte counts and refusals.  Shapes,
rows and references: tests/fault_sums_cases.py; tests/test_fault_sums_cpu.py holds the host side."""
import ctypes as C

import numpy as np
import pytest

from tests import dem_cases as dc
from tests import dem_weight_cases as wc
from tests import fault_sums_cases as fc
from tests import harvest_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


class Engine:
    """A bposd_dem with a decoder on hc.chain_model(N) and the harvest on (the list lives in its block), for the kernel alone."""

    def __init__(self, lib, N, capacity):
        from bp_osd_amd import BpOsdDecoder, _lib

        self.lib, self._lib, self.h, self.N = lib, _lib, None, N
        H, L, priors = hc.chain_model(N)
        self.dec = BpOsdDecoder(H, channel_probs=priors, max_iter=4, bp_method="ms", osd_method="osd0")  # (it never decodes)
        cfg = _lib.BposdDemConfig(device=0, seed=1, capacity=capacity)
        a = [np.ascontiguousarray(v, dtype=np.int32) for v in (H.indptr, H.indices, L.indptr, L.indices)]
        self.h = C.c_void_p()
        rc = lib.bposd_dem_create(C.byref(cfg), self.dec._h, a[0].ctypes.data, a[1].ctypes.data, H.shape[0], a[2].ctypes.data, a[3].ctypes.data, 1, N,
                                  priors.ctypes.data, C.byref(self.h))
        if rc != 0:
            self.h = None
            _lib.check_dem(lib, None, rc)
        _lib.check_dem(lib, self.h, lib.bposd_dem_set_harvest(self.h, 1))

    def sums(self, fault_words, select, mult):
        """bposd_debug_dem_fault_sums -> (counts, sums); select None: the implicit form, mult None: counts only."""
        f = np.ascontiguousarray(fault_words)
        s = None if select is None else np.ascontiguousarray(select, dtype=np.uint8)
        m = None if mult is None else np.ascontiguousarray(mult, dtype=np.uint32)
        counts = np.full(self.N, 0x5A5A5A5A5A5A5A5A, np.uint64)
        sums = None if m is None else np.full(self.N, 0x5A5A5A5A5A5A5A5A, np.uint64)
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
        mult_ptr = None if m is None else (m if m.size else np.zeros(1, np.uint32)).ctypes.data  # (F = 0 still asks for sums)
        rc = self.lib.bposd_debug_dem_fault_sums(self.h, f.ctypes.data, ptr(s), mult_ptr, f.shape[0], counts.ctypes.data, ptr(sums))
        self._lib.check_dem(self.lib, self.h, rc)
        return counts, sums

    def close(self):
        if getattr(self, "h", None) is not None:
            self.lib.bposd_dem_destroy(self.h)
            self.h = None

    __del__ = close


@pytest.fixture(scope="module")
def engines(gpu_ready):
    """One engine per N of the kernel cases, as large as that N's largest case."""
    made = {}

    def get(N):
        if N not in made:
            made[N] = Engine(gpu_ready, N, max(c["B"] for c in fc.KERNEL_CASES if c["N"] == N) + 3)
        return made[N]

    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "counts"])
@pytest.mark.parametrize("form", ["listed", "all"])
@pytest.mark.parametrize("case", fc.KERNEL_CASES, ids=[c["id"] for c in fc.KERNEL_CASES])
def test_kernel_alone_equals_dense_integer_sums(engines, case, form, weighted):
    """fault_sums_kernel through bposd_debug_dem_fault_sums, no decode: both instances, on the list harvest_list_kernel makes
    of the select bytes and on the implicit list of every row, equal ``rows.T @ mult`` in integers -- and the package's
    restatement, which tests/test_fault_sums_cpu.py holds against the same reference."""
    faults, select, mult = fc.kernel_rows(case["id"])
    rows, counts, sums = fc.kernel_reference(case["id"], form)
    got_c, got_s = engines(case["N"]).sums(dc.pack(faults), select if form == "listed" else None, mult[rows] if weighted else None)
    print(case["id"], form, "F", rows.size, "largest count", int(counts.max(initial=0)), "largest sum", int(sums.max(initial=0)))
    assert got_c.dtype == np.uint64 and (got_c == counts).all(), np.flatnonzero(got_c != counts)[:10]
    if weighted:
        assert (got_s == sums).all(), np.flatnonzero(got_s != sums)[:10]
    else:
        assert got_s is None


# ---------------------------------------------------------------------------------------------------------------- whole runs
@pytest.mark.parametrize("case_id", [c["id"] for c in dc.RUN_CASES])
def test_native_fault_stats_equal_the_oracle_engines(gpu_ready, case_id):
    """fault_stats=True, harvest=4 on the native engine against engine="numpy" around the CPU oracle: as one batch, and as
    the same run split in three."""
    ref = fc.stats_reference(case_id)
    B = dc.RUN_BY_ID[case_id]["B"]
    sim = fc.stats_sim(case_id, "native")
    print(case_id, "failures", ref["failures"], "faults fired", int(ref["fault_counts"].sum()), "in failing shots", int(ref["failure_fault_counts"].sum()))
    assert sim.run_count == B and sim.fault_counts.dtype == np.int64
    assert (sim.fault_counts == ref["fault_counts"]).all() and (sim.failure_fault_counts == ref["failure_fault_counts"]).all()
    split = fc.stats_sim(case_id, "native", run_sim=False)
    for part in fc.split_sizes(B):
        split._run_batch_native(part)
    assert split.run_count == B
    assert (split.fault_counts == ref["fault_counts"]).all() and (split.failure_fault_counts == ref["failure_fault_counts"]).all()


@pytest.mark.parametrize("case_id", ["surface13-R3", "hgp400-R1"])
def test_weighted_sums_of_a_tilted_batch_equal_the_oracle_engines(gpu_ready, case_id):
    from bp_osd_amd.dem import weight_multipliers

    v, counts, sums, rows = fc.tilted_reference(case_id)
    assert rows.size > 4 and v.max() == 2 ** 31 - 1 and np.unique(v).size > 1
    sim = fc.stats_sim(case_id, "native", sample_scale=wc.RUN_SCALE)
    assert (sim.last_batch("fail_rows") == rows).all()
    mine = weight_multipliers(sim.last_batch("logw")[rows])
    assert mine.dtype == np.uint32 and (mine == v).all()
    got_c, got_s = sim.fault_sums("failing", mine)
    assert (got_c == counts).all() and (got_s == sums).all() and sums.any()
    only_c, none = sim.fault_sums("failing")
    assert none is None and (only_c == counts).all()
    every_c, every_s = sim.fault_sums("all", np.full(sim.run_count, 3, np.uint32))
    assert (every_c.astype(np.int64) == dc.unpack(sim.last_batch("faults"), sim.N).sum(axis=0)).all() and (every_s == 3 * every_c).all()
    assert sim.fault_sums_ms() > 0


def test_native_fit_equals_the_oracle_engines(gpu_ready):
    """fit_sample_priors(engine="native") on exact_model() returns exactly the array engine="numpy" around the oracle
    returns, with the same batch size."""
    from bp_osd_amd.dem import fit_sample_priors

    H, L, p = wc.exact_model()
    ref_q, ref_report = fc.oracle_fit(wc.EXACT_SEEDS[0])
    q, report = fit_sample_priors(H, L, p, engine="native", seed=wc.EXACT_SEEDS[0], **dc.DECODER)
    print("fitted", np.round(q, 4).tolist(), "failures per level", [r["failures"] for r in report])
    assert q.dtype == np.float64 and (q == ref_q).all()
    for mine, ref in zip(report, ref_report):
        assert mine["failures"] == ref["failures"] and mine["effective_sample_fraction"] == ref["effective_sample_fraction"]
        assert (mine["sample_priors"] == ref["sample_priors"]).all()


# ------------------------------------------------------------------------------------------------------ switching and refusals
def test_switching_bytes_and_refusals(gpu_ready):
    from bp_osd_amd import _lib
    from tests.test_gpu_dem import Engine as SampleOnly

    lib = gpu_ready
    INVALID = _lib.BPOSD_ERR_INVALID
    H, L, priors = dc.run_model("surface13-R3")
    N, cap = H.shape[1], 128
    mk = lambda **kw: fc.stats_sim("surface13-R3", "native", batch_size=cap, run_sim=False, **kw)
    sim, plain = mk(), mk()  # (neither runs a batch of its own: the engine is driven by hand below)
    dem = sim._dem
    counts, sums, mult = np.zeros(N, np.uint64), np.zeros(N, np.uint64), np.ones(cap, np.uint32)
    call = lambda select, m, n, c, s: lib.bposd_dem_fault_sums(dem, select, None if m is None else m.ctypes.data, n, None if c is None else c.ctypes.data,
                                                              None if s is None else s.ctypes.data)
    err = lambda: lib.bposd_dem_last_error(dem)
    before = sim.device_bytes()
    assert before == plain.device_bytes()
    assert call(1, None, 0, counts, None) == INVALID and b"no batch" in err()
    # a batch with the harvest off, before any call has run: what every later run of the same shots must give again
    ref_c = (C.c_int64 * 5)()
    assert lib.bposd_dem_run(dem, 0, cap, ref_c) == 0
    sim._last_B = cap
    ref_flags, ref_obs = np.array(sim.last_batch("flags")), np.array(sim.last_batch("obs_osdw"))
    assert sim.device_bytes() == before
    refusals = [(lambda: call(2, None, 0, counts, None), b"select = 2"), (lambda: call(-1, None, 0, counts, None), b"select = -1"),
                (lambda: call(1, None, 0, counts, None), b"harvest on"), (lambda: call(0, mult, cap - 1, counts, sums), b"n_mult = 127"),
                (lambda: call(0, None, 0, None, None), b"counts is NULL"), (lambda: call(0, mult, cap, counts, None), b"go together"),
                (lambda: call(0, None, 0, counts, sums), b"go together")]

    def refused_and_nothing_changed(which):
        for attempt, why in which:
            assert attempt() == INVALID and why in err(), why
            assert sim.device_bytes() == bytes_now[0], why
            c = (C.c_int64 * 5)()
            assert lib.bposd_dem_run(dem, 0, cap, c) == 0 and list(c) == list(ref_c), why  # the next run and its outputs are as they were
            sim._last_B = cap
            assert (sim.last_batch("flags") == ref_flags).all() and (sim.last_batch("obs_osdw") == ref_obs).all(), why

    bytes_now = [before]
    refused_and_nothing_changed(refusals)  # (before anything was allocated)
    assert call(0, None, 0, counts, None) == 0
    grown = 16 * N + 4 * cap
    assert sim.device_bytes() == before + grown  # the first call that runs, and only that one
    bits = dc.unpack(sim.last_batch("faults"), N)
    assert (counts.astype(np.int64) == bits.sum(axis=0)).all()
    assert call(0, mult, cap, counts, sums) == 0 and (sums == counts).all() and sim.device_bytes() == before + grown

    # the harvest on: "failing" reads the list of the batch
    assert lib.bposd_dem_set_harvest(dem, 2) == 0
    bytes_now = [sim.device_bytes()]
    c_on = (C.c_int64 * 5)()
    assert lib.bposd_dem_run(dem, 0, cap, c_on) == 0 and list(c_on) == list(ref_c)
    rows = np.flatnonzero(ref_flags & 4)
    assert rows.size > 2
    assert call(1, None, 0, counts, None) == 0 and (counts.astype(np.int64) == bits[rows].sum(axis=0)).all()
    m3 = np.full(rows.size, 3, np.uint32)
    assert call(1, m3, rows.size, counts, sums) == 0 and (sums == 3 * counts).all()
    assert sim.device_bytes() == bytes_now[0]
    refused_and_nothing_changed(refusals[:2] + [(lambda: call(1, mult, rows.size + 1, counts, sums), b"failing shots")] + refusals[4:])
    # ... and after a batch with the harvest off again, its list is gone
    assert lib.bposd_dem_set_harvest(dem, 0) == 0 and lib.bposd_dem_run(dem, 0, cap, c_on) == 0
    assert call(1, None, 0, counts, None) == INVALID and b"harvest on" in err()
    assert lib.bposd_dem_fault_sums(None, 0, None, 0, counts.ctypes.data, None) == INVALID

    # a sample-only engine: "all" after bposd_dem_sample, nothing to fail
    eng = SampleOnly(lib, H, L, priors, capacity=32, seed=dc.RUN_SEED)
    b0 = lib.bposd_dem_device_bytes(eng.h)
    assert lib.bposd_dem_fault_sums(eng.h, 0, None, 0, counts.ctypes.data, None) == INVALID and lib.bposd_dem_device_bytes(eng.h) == b0
    assert lib.bposd_dem_sample(eng.h, 0, 32) == 0
    assert lib.bposd_dem_fault_sums(eng.h, 1, None, 0, counts.ctypes.data, None) == INVALID
    assert lib.bposd_dem_fault_sums(eng.h, 0, None, 0, counts.ctypes.data, None) == 0
    assert lib.bposd_dem_device_bytes(eng.h) == b0 + 16 * N + 4 * 32
    assert (counts.astype(np.int64) == bits[:32].sum(axis=0)).all()  # the same stream, the same first shots
    eng.close()
