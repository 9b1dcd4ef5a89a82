"""The detector-error-model engine without a GPU: ``bposd_dem_tables`` against scipy's CSC of H stacked on L and what it
refuses, ``phenomenological_dem`` against a round-by-round simulation, and ``dem_decode_sim(engine="numpy")`` on the CPU
oracle -- including the oracle's figures of the whole-run cases of tests/test_gpu_dem.py, so that those cannot pass on a
degenerate batch."""
import json

import numpy as np
import pytest
import scipy.sparse as sp

from bp_osd_amd import _lib, dem_decode_sim, phenomenological_dem
from bp_osd_amd.build import build_library
from oracle import OracleDecoder
from tests import dem_cases as dc

POISON = 0x5A5A5A5A


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _lib.load()


def test_library_exports_the_dem_calls(lib):
    for name in ("bposd_dem_tables", "bposd_dem_create", "bposd_dem_sample", "bposd_dem_run", "bposd_dem_fetch", "bposd_dem_device_bytes",
                 "bposd_dem_last_error", "bposd_dem_destroy"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name


def _tables(lib, H, L, N=None, M=None, k=None):
    """(rc, col_ptr, col_bits, message) of the C call on scipy CSR operands; the outputs start poisoned."""
    H, L = sp.csr_matrix(H), sp.csr_matrix(L)
    return _tables_raw(lib, H.indptr, H.indices, H.shape[0] if M is None else M, L.indptr, L.indices, L.shape[0] if k is None else k,
                       H.shape[1] if N is None else N)


def _tables_raw(lib, h_rp, h_ci, M, l_rp, l_ci, k, N):
    a = [np.ascontiguousarray(v, dtype=np.int32) for v in (h_rp, h_ci, l_rp, l_ci)]
    col_ptr = np.full(max(N, 0) + 1, POISON, np.int32)
    col_bits = np.full(len(a[1]) + len(a[3]) + 1, POISON, np.int32)
    rc = lib.bposd_dem_tables(a[0].ctypes.data, a[1].ctypes.data, M, a[2].ctypes.data, a[3].ctypes.data, k, N, col_ptr.ctypes.data,
                              col_bits.ctypes.data)
    return rc, col_ptr, col_bits, lib.bposd_dem_last_error(None).decode()


@pytest.mark.parametrize("M", [1, 63, 64, 65])
@pytest.mark.parametrize("k", [1, 64, 65])
def test_dem_tables_is_the_csc_of_h_stacked_on_l(lib, M, k):
    N = 37
    rng = np.random.default_rng(100 * M + k)
    H = (rng.random((M, N)) < 0.3).astype(np.uint8)
    L = (rng.random((k, N)) < 0.3).astype(np.uint8)
    H[:, 5] = 0
    L[:, 5] = 0  # an empty column
    H[:, 9] = 0
    L[:, 9] = 0
    L[k - 1, 9] = 1  # a column with an observable entry only
    rc, col_ptr, col_bits, _ = _tables(lib, H, L)
    assert rc == 0
    want = sp.vstack([sp.csr_matrix(H), sp.csr_matrix(L)]).tocsc()
    want.sort_indices()
    assert (col_ptr == want.indptr).all()
    base = 64 * ((M + 63) // 64)
    want_bits = np.where(want.indices < M, want.indices, want.indices - M + base)  # stacked row -> bit of the accumulator row
    assert (col_bits[:-1] == want_bits).all() and col_bits[-1] == POISON
    assert col_ptr[6] == col_ptr[5] and col_ptr[10] - col_ptr[9] == 1 and col_bits[col_ptr[9]] == base + k - 1
    for i in range(N):  # entries ascend within a column
        assert (np.diff(col_bits[col_ptr[i]:col_ptr[i + 1]]) > 0).all()


H_OK = ([0, 2, 3], [1, 4, 0])  # 2 x 5
L_OK = ([0, 1], [3])           # 1 x 5


@pytest.mark.parametrize("what,h,M,l,k,N", [
    ("H column N", ([0, 2, 3], [1, 5, 0]), 2, L_OK, 1, 5),
    ("H column -1", ([0, 2, 3], [-1, 4, 0]), 2, L_OK, 1, 5),
    ("L column N", H_OK, 2, ([0, 1], [5]), 1, 5),
    ("H not ascending", ([0, 2, 3], [4, 4, 0]), 2, L_OK, 1, 5),
    ("H descending", ([0, 2, 3], [4, 1, 0]), 2, L_OK, 1, 5),
    ("L descending", H_OK, 2, ([0, 2], [3, 2]), 1, 5),
    ("k = 0", H_OK, 2, ([0], []), 0, 5),
    ("k = 4097", H_OK, 2, ([0] * 4098, []), 4097, 5),
    ("M = 0", ([0], []), 0, L_OK, 1, 5),
    ("N = 0", ([0, 0, 0], []), 2, ([0, 0], []), 1, 0),
])
def test_dem_tables_refusals_write_nothing(lib, what, h, M, l, k, N):
    rc, col_ptr, col_bits, msg = _tables_raw(lib, h[0], h[1], M, l[0], l[1], k, N)
    assert rc == _lib.BPOSD_ERR_INVALID and "bposd_dem_tables" in msg, (what, rc, msg)
    assert (col_ptr == POISON).all() and (col_bits == POISON).all(), "written in spite of the error"


def test_dem_tables_accepts_the_valid_neighbours(lib):
    rc, col_ptr, col_bits, _ = _tables_raw(lib, H_OK[0], H_OK[1], 2, L_OK[0], L_OK[1], 1, 5)
    assert rc == 0 and col_ptr.tolist() == [0, 1, 2, 2, 3, 4] and col_bits[:4].tolist() == [1, 0, 64, 0]
    assert _tables(lib, sp.csr_matrix((3, 7), dtype=np.uint8), sp.csr_matrix((4096, 7), dtype=np.uint8))[0] == 0  # the cap; no entry at all


# --------------------------------------------------------------------------------------------------- phenomenological_dem
def _round_by_round(h, faults, R):
    """Detector rows of fault rows [B, (R+1) n + R m] by direct simulation: data flips accumulate, measurement flips are
    XORed into their round's outcomes, consecutive rounds are differenced; round R is perfect."""
    m, n = h.shape
    B = len(faults)
    data = faults[:, :(R + 1) * n].reshape(B, R + 1, n)
    meas = faults[:, (R + 1) * n:].reshape(B, R, m)
    state = np.zeros((B, n), np.uint8)
    prev = np.zeros((B, m), np.uint8)
    det = np.zeros((B, R + 1, m), np.uint8)
    for t in range(R + 1):
        state ^= data[:, t]
        outcome = dc.mod2(h, state)
        if t < R:
            outcome ^= meas[:, t]
        det[:, t] = outcome ^ prev
        prev = outcome
    return det.reshape(B, (R + 1) * m), state


def test_phenomenological_dem_of_surface13():
    code = dc.code("surface13")
    h, l = code.hz, code.lz
    assert h.shape == (6, 13) and l.shape == (1, 13)
    H, L, priors = phenomenological_dem(h, l, 3, 0.04, 0.01)
    assert sp.isspmatrix_csr(H) and sp.isspmatrix_csr(L) and priors.dtype == np.float64
    assert H.shape == (24, 70) and L.shape == (1, 70) and priors.shape == (70,)
    assert (priors[:52] == 0.04).all() and (priors[52:] == 0.01).all()
    rows, cols = np.diff(H.indptr), np.diff(H.tocsc().indptr)
    assert rows.min() == 4 and rows.max() == 6 and cols.min() == 1 and cols.max() == 2
    assert not L[:, 52:].nnz
    faults = (np.random.default_rng(3).random((200, 70)) < 0.2).astype(np.uint8)
    det, final = _round_by_round(h, faults, 3)
    assert det.any() and (dc.mod2(H, faults) == det).all()
    assert (dc.mod2(L, faults) == dc.mod2(l, final)).all()  # the observable is that of the accumulated data error


def test_phenomenological_dem_without_rounds_is_code_capacity():
    code = dc.code("surface13")
    H, L, priors = phenomenological_dem(code.hz, code.lz, 0, 0.07, 0.5)
    assert (H != sp.csr_matrix(code.hz)).nnz == 0 and (L != sp.csr_matrix(code.lz)).nnz == 0
    assert priors.shape == (13,) and (priors == 0.07).all()
    with pytest.raises(ValueError):
        phenomenological_dem(code.hz, code.lz, -1, 0.1, 0.1)


# --------------------------------------------------------------------------------------------------- dem_decode_sim on the oracle
@pytest.mark.parametrize("case", dc.RUN_CASES, ids=[c["id"] for c in dc.RUN_CASES])
def test_oracle_run_is_what_the_gpu_tests_expect(case):
    """Shapes and the oracle's figures of the whole-run cases; counters equal a recount from the last_batch arrays."""
    H, L, priors = dc.run_model(case["id"])
    assert H.shape == case["shape"] and L.shape == (case["k"], case["shape"][1])
    r = dc.run_reference(case["id"])
    B, k, want = case["B"], case["k"], case["oracle"]
    assert r["run_count"] == B
    flags = r["flags"]
    wrong = tuple(int(((flags >> i) & 1).sum()) for i in range(3))
    print(case["id"], "trivial", r["trivial_count"], "converged", r["bp_converge_count"], "wrong", wrong)
    assert r["bp_converge_count"] == want["converged"] and wrong == want["wrong"]
    if want["trivial"] is not None:
        assert r["trivial_count"] == want["trivial"]
    # recount
    f2, counters, obs_fail = dc.numpy_score(r["observables"], r["obs_bp"], r["obs_osd0"], r["obs_osdw"], r["converged"], r["detectors"], k)
    assert (f2 == flags).all() and (obs_fail == r["obs_fail"]).all()
    assert counters == [r[c] for c in dc.COUNTS[1:]]
    assert r["osd0_success_count"] == B - wrong[1] and r["osdw_success_count"] == B - wrong[2]
    assert (r["osdw_observable_error_rates"] == r["obs_fail"] / B).all()
    # from the definitions, on unpacked rows
    faults = dc.unpack(r["faults"], H.shape[1])
    assert (dc.pack(dc.mod2(H, faults)) == r["detectors"]).all() and (dc.pack(dc.mod2(L, faults)) == r["observables"]).all()
    assert r["trivial_count"] == int((~dc.mod2(H, faults).any(axis=1)).sum())
    # not degenerate: the three outputs differ from each other somewhere, successes and failures both occur
    assert 0 < wrong[2] < B and 0 < r["bp_converge_count"] < B
    assert (r["obs_bp"] != r["obs_osdw"]).any() and (r["obs_bp"] != r["obs_osd0"]).any()
    if case["id"] != "surface13-R3":  # (one observable and 24 detectors: osd_cs of order 2 changes no observable there)
        assert (r["obs_osd0"] != r["obs_osdw"]).any()


def test_numpy_engine_is_batch_size_independent():
    H, L, priors = dc.run_model("surface13-R3")
    one = dc.oracle_sim(H, L, priors, 64, batch_size=64)
    four = dc.oracle_sim(H, L, priors, 64, batch_size=16)
    assert one.run_count == four.run_count == 64
    assert one.output_dict() == four.output_dict()
    out = json.loads(one.output_dict())
    assert out["run_count"] == 64 and 0 < out["osdw_success_count"] < 64 and len(out["osdw_observable_error_rates"]) == 1
    L_ = out["osdw_logical_error_rate"]
    assert L_ == 1 - out["osdw_success_count"] / 64 and out["osdw_logical_error_rate_eb"] == float(np.sqrt((1 - L_) * L_ / 64))
    assert four.last_batch("flags").shape == (16,) and one.last_batch("faults").shape == (64, 2)
    ref = dc.run_reference("surface13-R3")  # the first 64 shots of the 256-shot batch are the same shots
    assert (one.last_batch("faults") == ref["faults"][:64]).all() and (one.last_batch("flags") == ref["flags"][:64]).all()


def test_arguments_are_checked():
    H, L, priors = dc.run_model("surface13-R3")
    with pytest.raises(ValueError, match="decoder_factory"):
        dem_decode_sim(H, L, priors, engine="native", decoder_factory=OracleDecoder)
    for bad in (-0.1, 1.5, float("nan")):
        p = priors.copy()
        p[7] = bad
        with pytest.raises(ValueError, match="fault 7"):
            dem_decode_sim(H, L, p, engine="numpy", decoder_factory=OracleDecoder, **dc.DECODER)
    with pytest.raises(ValueError):
        dem_decode_sim(H, L, priors[:-1], engine="numpy", decoder_factory=OracleDecoder)
    with pytest.raises(ValueError):
        dem_decode_sim(H, L[:, :-1], priors, engine="numpy", decoder_factory=OracleDecoder)
    with pytest.raises(ValueError):
        dem_decode_sim(H, L, priors, engine="torch")
    sim = dem_decode_sim(H, L, priors, engine="numpy", decoder_factory=OracleDecoder, run_sim=False, **dc.DECODER)
    with pytest.raises(RuntimeError):
        sim.last_batch("flags")
    with pytest.raises(ValueError):
        sim.last_batch("nothing")


def test_sampler_models_have_the_columns_the_gpu_test_is_about():
    for c in dc.SAMPLER_CASES:
        H, L, priors = dc.random_model(c["N"], c["M"], c["k"])
        assert H.shape == (c["M"], c["N"]) and L.shape == (c["k"], c["N"])
        ref = dc.sampler_reference(c["id"])
        assert ref["detectors"].any() and ref["observables"].any()
        if c["N"] < 4:
            continue
        stacked = sp.vstack([H, L]).tocsc()
        w = np.diff(stacked.indptr)
        assert w[dc.EMPTY_FAULT] == 0 and w[dc.HEAVY_FAULT] >= 40
        assert H[:, dc.OBS_ONLY_FAULT].nnz == 0 and L[:, dc.OBS_ONLY_FAULT].nnz == 1
        assert set(priors) == set(dc.PRIOR_VALUES)
        fired = ref["fault_bits"]
        assert fired[:, dc.EMPTY_FAULT].all() and 0 < fired[:, dc.HEAVY_FAULT].sum() < len(fired) and 0 < fired[:, dc.OBS_ONLY_FAULT].sum() < len(fired)
        assert not fired[:, priors == 0].any() and fired[:, priors == 1].all()
