"""The harvest of failing shots on the MI355X (bposd_*_set_harvest, harvest=K of the two DEM harnesses): the
three kernels alone on seeded rows against the numpy restatement of tests/harvest_cases.py, whole runs against the CPU
oracle item for item, and switching, byte counts and refusals.  Shapes, rows and references: tests/harvest_cases.py;
tests/test_harvest_cpu.py pins the oracle's figures."""
import ctypes as C
import json

import numpy as np
import pytest

from tests import dem_cases as dc
from tests import harvest_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


class Engine:
    """A bposd_dem with a decoder on hc.chain_model(N), for the kernels alone."""

    def __init__(self, lib, N, capacity):
        from bp_osd_amd import BpOsdDecoder, _lib

        self.lib, self._lib, self.h, self.N, self.fw = lib, _lib, None, N, (N + 63) // 64
        H, L, priors = hc.chain_model(N)
        self.dec = BpOsdDecoder(H, channel_probs=priors, max_iter=4, bp_method="ms", osd_method="osd0")  # (it never decodes: N = 1 has no column to search)
        cfg = _lib.BposdDemConfig(device=0, seed=1, capacity=capacity)
        a = [np.ascontiguousarray(v, dtype=np.int32) for v in (H.indptr, H.indices, L.indptr, L.indices)]
        self.h = C.c_void_p()
        rc = lib.bposd_dem_create(C.byref(cfg), self.dec._h, a[0].ctypes.data, a[1].ctypes.data, H.shape[0], a[2].ctypes.data, a[3].ctypes.data, 1, N,
                                  priors.ctypes.data, C.byref(self.h))
        if rc != 0:
            self.h = None
            _lib.check_dem(lib, None, rc)

    def harvest(self, fault_words, corr, packed, select, K):
        """bposd_debug_dem_harvest -> (info, the five items)."""
        chk = lambda rc: self._lib.check_dem(self.lib, self.h, rc)
        chk(self.lib.bposd_dem_set_harvest(self.h, K))
        f, c, s = np.ascontiguousarray(fault_words), np.ascontiguousarray(corr), np.ascontiguousarray(select, dtype=np.uint8)
        chk(self.lib.bposd_debug_dem_harvest(self.h, f.ctypes.data, c.ctypes.data, 1 if packed else 0, s.ctypes.data, len(s)))
        t = (C.c_int64 * 3)()
        chk(self.lib.bposd_dem_harvest_info(self.h, t))
        count, kept = int(t[0]), min(int(t[0]), K)
        shapes = {"fail_rows": (count,), "fail_weight": (count,), "fail_residual": (kept, self.fw), "fail_faults": (kept, self.fw),
                  "min_residual": (self.fw,)}
        out = {}
        for item, shape in shapes.items():
            out[item] = np.full(shape, 0x5A, dtype=np.dtype(self._lib.DEM_ITEMS[item][1]))
            dst = out[item] if out[item].nbytes else np.zeros(1, np.uint64)  # (an item of no rows is fetched too: 0 bytes)
            chk(self.lib.bposd_dem_fetch(self.h, self._lib.DEM_ITEMS[item][0], dst.ctypes.data, out[item].nbytes))
        return tuple(int(v) for v in t), out

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
            made[N] = Engine(gpu_ready, N, max(c["B"] for c in hc.KERNEL_CASES if c["N"] == N) + 3)
        return made[N]

    yield get
    for e in made.values():
        e.close()


def _reference_shows_the_case(case, ref):
    """Each case's condition on the numpy reference alone, before the device is asked."""
    count, min_w, min_row = ref["info"]
    rows, w, B, K = ref["fail_rows"], ref["fail_weight"], case["B"], case["K"]
    assert (np.diff(rows) > 0).all() and ref["fail_residual"].shape[0] == min(count, K)
    if case["select"] == "none":
        assert ref["info"] == (0, -1, -1) and not ref["min_residual"].any()
    elif case["select"] == "all":
        assert count == B and (rows == np.arange(B)).all()
    else:
        assert 0 < count < B
    if case["special"] == "ends":
        assert rows[0] == 0 and rows[-1] == B - 1
    if case["special"] == "tie":
        assert (w == min_w).sum() == 3 and min_row == rows[w == min_w].min()
    if case["special"] == "last":
        assert (w == min_w).sum() == 1 and min_row == rows[-1]
    if case["special"] == "beyond":
        assert (w == min_w).sum() == 1 and list(rows).index(min_row) >= K
    if count:
        assert min_w == w.min() and 0 <= min_w <= case["N"]


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "bytes"])
@pytest.mark.parametrize("case", hc.KERNEL_CASES, ids=[c["id"] for c in hc.KERNEL_CASES])
def test_kernels_alone_equal_numpy(engines, case, packed):
    """harvest_list_kernel, harvest_rows_kernel and harvest_min_kernel through bposd_debug_dem_harvest, no decode: every item
    and the triple equal the numpy restatement, in both forms a decoder leaves its correction rows in."""
    ref = hc.kernel_reference(case["id"])
    _reference_shows_the_case(case, ref)
    faults, corr, select = hc.kernel_rows(case["id"])
    if packed:
        rows = dc.pack(corr)
    else:  # of a byte row bit 0 counts
        rows = corr | (np.random.default_rng(7).integers(0, 128, size=corr.shape).astype(np.uint8) << 1)
        assert (corr.size < 64 or (rows > 1).any()) and ((rows & 1) == corr).all()
    info, got = engines(case["N"]).harvest(dc.pack(faults), rows, packed, select, case["K"])
    print(case["id"], "packed" if packed else "bytes", "info", info, "reference", ref["info"])
    assert info == ref["info"]
    for item in hc.ITEMS:
        assert got[item].shape == ref[item].shape and got[item].dtype == ref[item].dtype, item
        diff = got[item] != ref[item]  # (an item of no rows has nothing to differ in)
        bad = np.flatnonzero(diff.reshape(diff.shape[0], -1).any(axis=1)) if diff.size else np.zeros(0, np.int64)
        assert bad.size == 0, (item, bad[:10])


# ---------------------------------------------------------------------------------------------------------------- whole runs
def _equal(sim, ref):
    for key in hc.RESULTS:
        assert np.array_equal(getattr(sim, key), ref[key]), (key, getattr(sim, key), ref[key])
    assert set(sim.failures) == set(ref["failures"])
    for key, v in ref["failures"].items():
        assert sim.failures[key].dtype == v.dtype and np.array_equal(sim.failures[key], v), key


@pytest.mark.parametrize("case", hc.RUN_CASES, ids=[c["id"] for c in hc.RUN_CASES])
def test_native_harvest_equals_oracle_harvest(gpu_ready, case):
    """A whole batch with every failing row kept against engine="numpy" on the CPU oracle: the run's attributes, `failures`,
    the five items and output_dict; and the form the decoder left its rows in is the one the case is about."""
    ref = hc.run_reference(case["id"])
    count = ref["items"]["fail_rows"].size
    assert count == case["failures"] and ref["min_logical_weight"] == case["min_weight"] and ref["min_logical_shot"] == case["tied"][0]
    sim = hc.sim(case, "native", case["B"])
    print(case["id"], "failures", sim.last_batch("fail_rows").size, "min", sim.min_logical_weight, sim.min_logical_shot)
    assert (sim.last_batch("flags") == ref["flags"]).all() and (sim.last_batch("faults") == ref["faults"]).all()
    _equal(sim, ref)
    for item in hc.ITEMS:
        got = sim.last_batch(item)
        assert got.shape == ref["items"][item].shape and got.dtype == ref["items"][item].dtype and (got == ref["items"][item]).all(), item
    assert json.loads(sim.output_dict()) == dict(json.loads(ref["output"]), engine="native")
    if case["kind"] == "dem":
        bp, osd = sim.decoder.last_instance()["bp"], sim.decoder.last_osd_kernel()
        want = {"surface13-R3": (True, None), "hgp400-R1": (True, None), "hgp400-R3": (True, "osd_large_kernel"),
                "surface13-R3-serial": (False, None), "random-520": (False, None)}[case["id"]]
        assert bp[2] == want[0], bp
        if case["id"] == "surface13-R3-serial":
            assert bp[0] == "bp_serial_kernel"
        if case["id"] == "random-520":
            assert bp[0] == "bp_anydeg_kernel"
        if want[1]:
            assert osd == want[1]


@pytest.mark.parametrize("case_id", ["surface13-R3", "surface13-R3-w21"])
def test_native_harvest_is_batch_size_independent(gpu_ready, case_id):
    """64 + 64 + 128 shots equal one batch of 256."""
    case, ref = hc.RUN_BY_ID[case_id], hc.run_reference(case_id)
    sim = hc.sim(case, "native", 256, batch_size=128, run_sim=False)
    for B in (64, 64, 128):
        sim._run_batch_native(B)
    assert sim.run_count == 256
    _equal(sim, ref)
    assert json.loads(sim.output_dict())["min_logical_weight"] == case["min_weight"]


def test_a_cap_of_two_with_the_lightest_row_beyond_it(gpu_ready):
    case, ref = hc.RUN_BY_ID["surface13-R3"], hc.run_reference("surface13-R3")
    sim = hc.sim(case, "native", 2)
    assert sim.failures["shot"].tolist() == [5, 6]
    for key in ("weight", "residual", "faults"):
        assert np.array_equal(sim.failures[key], ref["failures"][key][:2]), key
    assert sim.min_logical_shot == 17 and sim.min_logical_weight == 3 and (sim.min_logical_fault == ref["min_logical_fault"]).all()
    assert (sim.failure_weight_counts == ref["failure_weight_counts"]).all() and sim.failure_weight_counts.sum() == 44
    assert sim.last_batch("fail_residual").shape == (2, 2) and (sim.last_batch("fail_weight") == ref["items"]["fail_weight"]).all()
    assert (sim.last_batch("min_residual") == ref["items"]["min_residual"]).all()


def test_a_tilted_run_keeps_the_log_weights_of_its_failures(gpu_ready):
    case = hc.RUN_BY_ID["surface13-R3"]
    host = hc.sim(case, "numpy", 256, sample_scale=4)
    sim = hc.sim(case, "native", 256, sample_scale=4)
    rows = np.flatnonzero(sim.last_batch("flags") & 4)
    assert rows.size > 44 and (sim.failures["logw"] == sim.last_batch("logw")[rows]).all()
    for key, v in host.failures.items():
        assert sim.failures[key].dtype == v.dtype and np.array_equal(sim.failures[key], v), key
    assert sim.min_logical_shot == host.min_logical_shot and (sim.min_logical_fault == host.min_logical_fault).all()


# ------------------------------------------------------------------------------------------------------ switching and refusals
def _blocks(*sizes):
    return sum(max(256, int(s)) for s in sizes)


def test_dem_switching_bytes_and_refusals(gpu_ready):
    from bp_osd_amd import _lib

    lib = gpu_ready
    case = hc.RUN_BY_ID["surface13-R3"]
    H, L, priors, _ = hc.model(case)
    (M, N), k, cap = H.shape, L.shape[0], 128
    fw, dw, ow = (N + 63) // 64, (M + 63) // 64, (k + 63) // 64
    plain = hc.sim(case, "native", 0, batch_size=cap, run_sim=False)
    sim = hc.sim(case, "native", 0, batch_size=cap, run_sim=False)
    dem = sim._dem
    # an engine that never switched it on: the sum of its blocks as before
    before = _blocks(8 * N, 4 * (N + 1), 4 * (H.nnz + L.nnz), 8 * cap * fw, 8 * cap * dw, 8 * cap * ow, 8 * cap * ow, 8 * cap * ow, 8 * cap * ow,
                     cap, cap, 4 * cap, 32, 4 * k)
    assert plain.device_bytes() == sim.device_bytes() == before
    t, buf = (C.c_int64 * 3)(), np.zeros(64, np.uint64)
    c_on, c_off = (C.c_int64 * 5)(), (C.c_int64 * 5)()
    # refusals leave the mode as it was: off
    assert lib.bposd_dem_set_harvest(dem, -1) == _lib.BPOSD_ERR_INVALID and b"negative" in lib.bposd_dem_last_error(dem)
    assert sim.device_bytes() == before
    assert lib.bposd_dem_run(dem, 0, cap, c_off) == 0
    assert lib.bposd_dem_harvest_info(dem, t) == _lib.BPOSD_ERR_INVALID and b"harvest off" in lib.bposd_dem_last_error(dem)
    for item in hc.ITEMS:
        assert lib.bposd_dem_fetch(dem, _lib.DEM_ITEMS[item][0], buf.ctypes.data, 8 * fw) == _lib.BPOSD_ERR_INVALID, item
    assert lib.bposd_debug_dem_harvest(dem, buf.ctypes.data, buf.ctypes.data, 1, buf.ctypes.data, 1) == _lib.BPOSD_ERR_INVALID
    # on: exactly the stated bytes, once
    K = 5
    assert lib.bposd_dem_set_harvest(dem, K) == 0
    grown = 8 * cap + (2 * K + 1) * 8 * fw + 256
    assert sim.device_bytes() == before + grown
    assert lib.bposd_dem_set_harvest(dem, 3) == 0 and sim.device_bytes() == before + grown  # a smaller cap keeps the block
    assert lib.bposd_dem_set_harvest(dem, -7) == _lib.BPOSD_ERR_INVALID  # ... and a refusal the mode: on, 3 rows
    assert lib.bposd_dem_run(dem, 0, cap, c_on) == 0
    assert lib.bposd_dem_harvest_info(dem, t) == 0
    ref = hc.run_reference("surface13-R3")
    rows = ref["items"]["fail_rows"][ref["items"]["fail_rows"] < cap]
    assert t[0] == rows.size > 3 and list(c_on) == list(c_off)
    got = np.zeros((3, fw), "<u8")
    assert lib.bposd_dem_fetch(dem, _lib.DEM_ITEMS["fail_residual"][0], got.ctypes.data, got.nbytes) == 0
    assert (got == ref["items"]["fail_residual"][:3]).all()
    assert lib.bposd_dem_fetch(dem, _lib.DEM_ITEMS["fail_residual"][0], got.ctypes.data, got.nbytes + 8 * fw) == _lib.BPOSD_ERR_INVALID
    # a larger cap replaces the block
    assert lib.bposd_dem_set_harvest(dem, 9) == 0 and sim.device_bytes() == before + 8 * cap + 19 * 8 * fw + 256
    # off again, then a batch: a plain engine's counters, and the harvest's items are gone
    assert lib.bposd_dem_set_harvest(dem, 0) == 0 and sim.device_bytes() == before + 8 * cap + 19 * 8 * fw + 256
    c_plain = (C.c_int64 * 5)()
    assert lib.bposd_dem_run(dem, 0, cap, c_off) == 0 and lib.bposd_dem_run(plain._dem, 0, cap, c_plain) == 0
    assert list(c_off) == list(c_plain) == list(c_on)
    assert lib.bposd_dem_harvest_info(dem, t) == _lib.BPOSD_ERR_INVALID
    assert lib.bposd_dem_fetch(dem, _lib.DEM_ITEMS["fail_rows"][0], buf.ctypes.data, 4 * rows.size) == _lib.BPOSD_ERR_INVALID
    # a sample-only engine has nothing to harvest
    from tests.test_gpu_dem import Engine as SampleOnly

    eng = SampleOnly(lib, H, L, priors, capacity=32, seed=1)
    b0 = lib.bposd_dem_device_bytes(eng.h)
    assert lib.bposd_dem_set_harvest(eng.h, 4) == _lib.BPOSD_ERR_INVALID and b"without a decoder" in lib.bposd_dem_last_error(eng.h)
    assert lib.bposd_dem_device_bytes(eng.h) == b0
    eng.close()
    assert lib.bposd_dem_set_harvest(None, 1) == _lib.BPOSD_ERR_INVALID


def test_window_switching_bytes_and_refusals(gpu_ready):
    from bp_osd_amd import _lib

    lib = gpu_ready
    case = hc.RUN_BY_ID["surface13-R3-w21"]
    cap, fw = 128, 2
    plain = hc.sim(case, "native", 0, batch_size=cap, run_sim=False)
    sim = hc.sim(case, "native", 0, batch_size=cap, run_sim=False)
    win, before = sim._win, plain.device_bytes()
    assert sim.device_bytes() == before
    t, buf = (C.c_int64 * 3)(), np.zeros(64, np.uint64)
    c_on, c_off, c_plain = (C.c_int64 * 4)(), (C.c_int64 * 4)(), (C.c_int64 * 4)()
    assert lib.bposd_window_set_harvest(win, -1) == _lib.BPOSD_ERR_INVALID and sim.device_bytes() == before
    assert lib.bposd_window_run(win, sim._sampler, 0, cap, c_off) == 0
    assert lib.bposd_window_harvest_info(win, t) == _lib.BPOSD_ERR_INVALID
    # an engine that never switched it on: the blocks include/bposd_mi355x.h documents at bposd_window_create, as before
    H, L, _, _ = hc.model(case)
    (M, N), k, plan = H.shape, L.shape[0], sim.plan
    dw, ow = (M + 63) // 64, (k + 63) // 64
    assert fw == (N + 63) // 64
    packed = [d.bp_kernel_info()["kernel"] not in ("bp_anydeg_kernel", "bp_serial_kernel") for d in sim.decoders]  # (they have decoded by now)
    row = lambda cols, p: 8 * ((cols + 63) // 64) if p else cols
    nc = sum(int(w.commit.sum()) for w in plan.windows)
    ncw = sum(len(set((w.fault[w.commit != 0] >> 6).tolist())) for w in plan.windows)
    synd = max(row(w.det.size, packed[w.handle]) for w in plan.windows)
    decd = max(row(w.fault.size, packed[w.handle]) for w in plan.windows)
    assert before == _blocks(4 * (N + 1), 4 * (H.nnz + L.nnz), 4 * nc, 4 * nc, 4 * nc, 4 * ncw, 4 * sum(w.det.size for w in plan.windows),
                             8 * cap * dw, 8 * cap * ow, 8 * cap * ow, 8 * cap * fw, cap * synd, cap * decd, cap, 4 * cap, cap, 4 * cap, cap, 32, 4 * k)
    assert sim.device_bytes() == before
    for item in hc.ITEMS:
        assert lib.bposd_window_fetch(win, _lib.WINDOW_ITEMS[item][0], buf.ctypes.data, 8 * fw) == _lib.BPOSD_ERR_INVALID, item
    assert lib.bposd_window_set_harvest(win, 4) == 0 and sim.device_bytes() == before + 8 * cap + 9 * 8 * fw + 256
    assert lib.bposd_window_set_harvest(win, -2) == _lib.BPOSD_ERR_INVALID
    assert lib.bposd_window_run(win, sim._sampler, 0, cap, c_on) == 0 and lib.bposd_window_harvest_info(win, t) == 0
    ref = hc.run_reference("surface13-R3-w21")
    rows = ref["items"]["fail_rows"][ref["items"]["fail_rows"] < cap]
    assert t[0] == rows.size > 4 and list(c_on) == list(c_off)
    got = np.zeros(rows.size, np.int32)
    assert lib.bposd_window_fetch(win, _lib.WINDOW_ITEMS["fail_rows"][0], got.ctypes.data, got.nbytes) == 0 and (got == rows).all()
    assert lib.bposd_window_set_harvest(win, 0) == 0
    assert lib.bposd_window_run(win, sim._sampler, 0, cap, c_off) == 0 and lib.bposd_window_run(plain._win, plain._sampler, 0, cap, c_plain) == 0
    assert list(c_off) == list(c_plain) == list(c_on)
    assert lib.bposd_window_harvest_info(win, t) == _lib.BPOSD_ERR_INVALID
    assert lib.bposd_window_fetch(win, _lib.WINDOW_ITEMS["fail_rows"][0], got.ctypes.data, got.nbytes) == _lib.BPOSD_ERR_INVALID
