"""The detector-error-model engine of the library (bposd_dem_*, dem_decode_sim(engine="native")) on the MI355X: the sampler
against the host restatement of the Philox stream bit for bit, the scorer against a numpy score of the same decoder
object's outputs, whole runs against the CPU oracle driven by the same stream, and the absence of torch.  Tables and
references: tests/dem_cases.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dem_cases as dc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


class Engine:
    """bposd_dem_* through ctypes on a model (H, L, priors); dec = None makes the sample-only engine."""

    def __init__(self, lib, H, L, priors, capacity, seed, dec=None):
        from bp_osd_amd import _lib

        self.lib, self._lib, self.h = lib, _lib, None
        self.M, self.N = H.shape
        self.k = L.shape[0]
        cfg = _lib.BposdDemConfig(device=0, seed=seed, capacity=capacity)
        a = [np.ascontiguousarray(v, dtype=np.int32) for v in (H.indptr, H.indices, L.indptr, L.indices)]
        p = np.ascontiguousarray(priors, dtype=np.float64)
        self.h = C.c_void_p()
        rc = lib.bposd_dem_create(C.byref(cfg), dec._h if dec is not None else None, a[0].ctypes.data, a[1].ctypes.data, self.M, a[2].ctypes.data,
                                  a[3].ctypes.data, self.k, self.N, p.ctypes.data, C.byref(self.h))
        if rc != 0:
            self.h = None
            _lib.check_dem(lib, None, rc)

    def sample(self, first_shot, B):
        self.B = B
        return self.lib.bposd_dem_sample(self.h, first_shot, B)

    def fetch(self, what):
        item, dtype, cols = self._lib.DEM_ITEMS[what]
        width = {"N": self.N, "M": self.M, "k": self.k}
        shape = (self.B,) if cols is None else (self.k,) if cols == "k32" else (self.B, (width[cols] + 63) // 64)
        out = np.empty(shape, np.dtype(dtype))
        self._lib.check_dem(self.lib, self.h, self.lib.bposd_dem_fetch(self.h, item, out.ctypes.data, out.nbytes))
        return out

    def close(self):
        if getattr(self, "h", None) is not None:
            self.lib.bposd_dem_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


@pytest.mark.parametrize("case", dc.SAMPLER_CASES, ids=[c["id"] for c in dc.SAMPLER_CASES])
def test_sampler_equals_host_stream(gpu_ready, case):
    """dem_sample_kernel alone: packed fault rows = np.packbits of the host draw; detectors and observables = its products
    with H and L, padding bits zero."""
    H, L, priors = dc.random_model(case["N"], case["M"], case["k"])
    B, first = case["B"], case["first_shot"]
    eng = Engine(gpu_ready, H, L, priors, capacity=B + 3, seed=dc.SAMPLER_SEED)
    assert eng.sample(first, B) == 0, gpu_ready.bposd_dem_last_error(eng.h)
    ref = dc.sampler_reference(case["id"])
    got = {k: eng.fetch(k) for k in ("faults", "detectors", "observables")}
    assert got["faults"].shape == (B, (case["N"] + 63) // 64) and got["faults"].dtype == np.dtype("<u8")
    for k, v in got.items():
        assert v.shape == ref[k].shape
        bad = np.flatnonzero((v != ref[k]).any(axis=1))
        assert bad.size == 0, f"{k} differs from the host stream in {bad.size} shots, first {bad[:5]}"
    if first >= 2 ** 32:  # the high counter word matters: the same rows of shot 12345 .. differ
        assert not (dc.sampler_reference(case["id"], first - 2 ** 32)["faults"] == got["faults"]).all()
    assert gpu_ready.bposd_dem_device_bytes(eng.h) >= 8 * (B + 3) * got["faults"].shape[1]
    eng.close()


def _native(H, L, priors, B, batch_size=None, run_sim=True):
    from bp_osd_amd import dem_decode_sim

    return dem_decode_sim(H, L, priors, batch_size=batch_size or B, engine="native", seed=dc.RUN_SEED, target_runs=B, run_sim=run_sim,
                          **dc.DECODER)


def _scorer_models():
    out = [(c["id"], c["id"], None) for c in dc.RUN_CASES]
    return out + [("surface13-R3-k70", "surface13-R3", "L70")]


@pytest.mark.parametrize("name,case_id,other_l", _scorer_models(), ids=[m[0] for m in _scorer_models()])
def test_scorer_equals_numpy_score(gpu_ready, name, case_id, other_l):
    """dem_score_kernel: flags, the five counters and obs_fail are the numpy score of the fetched true observables against the
    observables of the same decoder object's decode_batch_observables on the fetched detectors."""
    H, L, priors = dc.run_model(case_id)
    if other_l:
        L = dc.random_L70()
    B, k = dc.RUN_BY_ID[case_id]["B"], L.shape[0]
    sim = _native(H, L, priors, B)
    assert sim.run_count == B
    det, truth = sim.last_batch("detectors"), sim.last_batch("observables")
    faults = dc.unpack(sim.last_batch("faults"), H.shape[1])
    assert (dc.pack(dc.mod2(L, faults)) == truth).all() and (dc.pack(dc.mod2(H, faults)) == det).all()
    got = {item: sim.last_batch(item) for item in dc.ITEMS}
    counters = [sim.bp_converge_count, sim.bp_success_count, sim.osd0_success_count, sim.osdw_success_count, sim.trivial_count]
    dec = sim.decoder
    ow = dec.decode_batch_observables(det, want_osd0=True, want_bp=True, packed=True)
    assert ow.shape == (B, (k + 63) // 64)
    assert (got["obs_osdw"] == ow).all() and (got["obs_osd0"] == dec.batch_obs_osd0).all() and (got["obs_bp"] == dec.batch_obs_bp).all()
    assert (got["converged"].astype(bool) == dec.batch_converge).all() and (got["iters"] == dec.batch_iter).all()
    flags, want, obs_fail = dc.numpy_score(truth, dec.batch_obs_bp, dec.batch_obs_osd0, ow, dec.batch_converge, det, k)
    print(name, "counters", counters, "numpy", want)
    assert (got["flags"] == flags).all(), np.flatnonzero(got["flags"] != flags)[:10]
    assert counters == want
    assert (got["obs_fail"] == obs_fail).all() and (sim.osdw_observable_error_rates == obs_fail / B).all()
    assert 0 < want[3] < B, "no osdw failure (or nothing but failures) in the batch"
    if k > 64:  # the second observable word takes part: some shot is wrong there only / also there
        x = got["obs_osdw"] ^ truth
        assert x[:, 1].any() and obs_fail[64:].any()


@pytest.mark.parametrize("case", dc.RUN_CASES, ids=[c["id"] for c in dc.RUN_CASES])
def test_native_run_equals_oracle_run(gpu_ready, case):
    """A whole batch against engine="numpy" on the CPU oracle and the same stream (min-sum: bit-exact): counters, flags,
    converged, iters and all three observable sets."""
    ref = dc.run_reference(case["id"])
    B, want = case["B"], case["oracle"]
    # the case is not degenerate on the reference alone
    wrong = tuple(int(((ref["flags"] >> i) & 1).sum()) for i in range(3))
    assert ref["bp_converge_count"] == want["converged"] and wrong == want["wrong"]
    assert 0 < wrong[2] < B and 0 < ref["bp_converge_count"] < B
    assert (ref["obs_bp"] != ref["obs_osdw"]).any() and (ref["obs_bp"] != ref["obs_osd0"]).any()
    if want["trivial"] is not None:
        assert ref["trivial_count"] == want["trivial"]

    H, L, priors = dc.run_model(case["id"])
    sim = _native(H, L, priors, B)
    print(case["id"], {c: getattr(sim, c) for c in dc.COUNTS}, sim.decoder.bp_kernel_info()["kernel"], sim.decoder.last_osd_kernel())
    for c in dc.COUNTS:
        assert getattr(sim, c) == ref[c], (c, getattr(sim, c), ref[c])
    for item in dc.ITEMS:
        got = sim.last_batch(item)
        assert got.shape == ref[item].shape and got.dtype == ref[item].dtype, item
        assert (got == ref[item]).all(), (item, np.flatnonzero((got != ref[item]).reshape(len(got), -1).any(axis=1))[:10])
    assert (sim.osdw_observable_error_rates == ref["osdw_observable_error_rates"]).all()
    # N > 2047 runs on the HBM-resident OSD kernel, the smaller models on the register-resident ones
    assert (sim.decoder.last_osd_kernel() == "osd_large_kernel") == (H.shape[1] > 2047)
    assert sim.device_bytes() > 8 * B * ((H.shape[1] + 63) // 64)


def test_native_run_is_batch_size_independent(gpu_ready):
    """64 + 64 + 128 shots equal one batch of 256."""
    import json

    ref = dc.run_reference("surface13-R3")
    H, L, priors = dc.run_model("surface13-R3")
    sim = _native(H, L, priors, 256, batch_size=128, run_sim=False)
    parts = {item: [] for item in dc.ITEMS[:-1]}
    fails = np.zeros(1, np.int64)
    for B in (64, 64, 128):
        sim._run_batch_native(B)
        for item in parts:
            parts[item].append(sim.last_batch(item))
        fails += sim.last_batch("obs_fail")
    assert sim.run_count == 256
    for c in dc.COUNTS:
        assert getattr(sim, c) == ref[c], c
    for item, rows in parts.items():
        assert (np.concatenate(rows) == ref[item]).all(), item
    assert (fails == ref["obs_fail"]).all()
    one = _native(H, L, priors, 256)
    a, b = json.loads(one.output_dict()), json.loads(sim.output_dict())
    assert a == b and a["osdw_success_count"] == ref["osdw_success_count"]


def test_native_engine_imports_no_torch(gpu_ready):
    """A device-resident DEM run in a fresh process (this session's conftest imports torch) never loads torch."""
    child = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from bp_osd_amd.codes import surface13\n"
        "from bp_osd_amd import dem_decode_sim, phenomenological_dem\n"
        "c = surface13()\n"
        "H, L, p = phenomenological_dem(c.hz, c.lz, 3, 0.04, 0.04)\n"
        "sim = dem_decode_sim(H, L, p, batch_size=128, engine='native', seed=5, target_runs=300, max_iter=4, bp_method='ms',\n"
        "                     ms_scaling_factor=0.625, osd_method='osd_cs', osd_order=2)\n"
        "assert sim.run_count == 300 and 0 < sim.osdw_success_count < 300, sim.output_dict()\n"
        "assert sim.last_batch('flags').shape == (300 - 256,)\n"
        "assert 'torch' not in sys.modules, 'torch was imported'\n"
        "print('native ok', sim.osdw_success_count)\n")
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "native ok" in r.stdout, r.stdout + r.stderr


def test_engine_arguments_are_checked_by_the_library(gpu_ready):
    """B beyond the capacity, a fetch of a decoded item after sample only, run on a sample-only engine, a decoder of another
    shape, priors that are no probabilities: BPOSD_ERR_INVALID with a message."""
    from bp_osd_amd import BpOsdDecoder, _lib

    lib = gpu_ready
    H, L, priors = dc.run_model("surface13-R3")
    counters = (C.c_int64 * 5)()
    # sample-only engine
    eng = Engine(lib, H, L, priors, capacity=64, seed=1)
    out = np.empty((64, 1), np.uint64)
    assert lib.bposd_dem_fetch(eng.h, 0, out.ctypes.data, out.nbytes) == _lib.BPOSD_ERR_INVALID  # nothing has run
    assert lib.bposd_dem_sample(eng.h, 0, 65) == _lib.BPOSD_ERR_INVALID and b"capacity" in lib.bposd_dem_last_error(eng.h)
    assert lib.bposd_dem_sample(eng.h, 0, 0) == _lib.BPOSD_ERR_INVALID
    assert lib.bposd_dem_run(eng.h, 0, 64, counters) == _lib.BPOSD_ERR_INVALID and b"without a decoder" in lib.bposd_dem_last_error(eng.h)
    assert eng.sample(0, 64) == 0
    assert eng.fetch("detectors").shape == (64, 1)
    assert lib.bposd_dem_fetch(eng.h, 5, out.ctypes.data, out.nbytes) == _lib.BPOSD_ERR_INVALID and b"bposd_dem_run" in lib.bposd_dem_last_error(eng.h)
    assert lib.bposd_dem_fetch(eng.h, 1, out.ctypes.data, out.nbytes - 8) == _lib.BPOSD_ERR_INVALID and b"bytes" in lib.bposd_dem_last_error(eng.h)
    assert lib.bposd_dem_fetch(eng.h, 10, out.ctypes.data, out.nbytes) == _lib.BPOSD_ERR_INVALID
    eng.close()
    # with a decoder
    dec = BpOsdDecoder(H, channel_probs=priors, **dc.DECODER)
    eng = Engine(lib, H, L, priors, capacity=32, seed=1, dec=dec)
    assert lib.bposd_dem_run(eng.h, 0, 33, counters) == _lib.BPOSD_ERR_INVALID and b"capacity" in lib.bposd_dem_last_error(eng.h)
    assert lib.bposd_dem_run(eng.h, 0, 32, counters) == 0, lib.bposd_dem_last_error(eng.h)
    eng.B = 32
    assert eng.fetch("obs_osdw").shape == (32, 1) and eng.fetch("obs_fail").shape == (1,)
    assert eng.sample(100, 16) == 0  # a sample-only batch afterwards: the decoded items are gone again
    assert lib.bposd_dem_fetch(eng.h, 6, out.ctypes.data, 16) == _lib.BPOSD_ERR_INVALID
    eng.close()
    # a decoder of another shape
    other = BpOsdDecoder(dc.code("surface13").hz, error_rate=0.1)
    with pytest.raises(ValueError, match="does not match"):
        Engine(lib, H, L, priors, capacity=32, seed=1, dec=other)
    for bad in (-0.1, 1.5, float("nan")):
        p = priors.copy()
        p[9] = bad
        with pytest.raises(ValueError, match="fault 9"):
            Engine(lib, H, L, p, capacity=32, seed=1)
    h = C.c_void_p()
    assert lib.bposd_dem_create(None, None, None, None, 0, None, None, 0, 0, None, C.byref(h)) == _lib.BPOSD_ERR_INVALID
    assert not h.value and lib.bposd_dem_last_error(None)
