"""Logical observables without a GPU: ``bposd_observable_table`` against a numpy packing, what it refuses, and the oracle's
view of the inputs of tests/test_gpu_observables.py -- so that a kernel that mixes up its three row sets, or reads BP's rows
where OSD rewrote them, cannot pass there."""
import numpy as np
import pytest
import scipy.sparse as sp

from bp_osd_amd import _lib, BpOsdDecoder
from bp_osd_amd.build import build_library
from tests import channel_rows_cases as cr
from tests import observables_cases as oc


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _lib.load()


def test_library_exports_the_observables_calls(lib):
    for name in ("bposd_observable_table", "bposd_set_observables", "bposd_observables_device_lane", "bposd_decode_batch_observables_device",
                 "bposd_decode_batch_observables", "bposd_decode_batch_observables_packed", "bposd_decode_batch_observables_async",
                 "bposd_decode_batch_observables_packed_async"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name


def _numpy_table(L):
    """[ceil(n/64)][k]: bit (c & 63) of word (c >> 6) of column j = L[j][c]."""
    k, n = L.shape
    words = (n + 63) // 64
    padded = np.zeros((k, 64 * words), np.uint8)
    padded[:, :n] = L
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little").view("<u8").T)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 620])
@pytest.mark.parametrize("k", [1, 64, 65])
def test_observable_table_is_the_numpy_packing(lib, n, k):
    L = oc.edge_matrix(n, k)
    want = _numpy_table(L)
    assert want.shape == ((n + 63) // 64, k) and want.dtype == np.uint64
    for form in (L, np.array(L, dtype=np.int64), sp.csr_matrix(L), sp.coo_matrix(L)):
        got = BpOsdDecoder.observable_table(form, n)
        assert got.dtype == np.uint64 and got.shape == want.shape and got.flags.c_contiguous
        assert (got == want).all()
    assert (BpOsdDecoder.observable_table(L) == want).all()  # n from the matrix


def _c_call(lib, indptr, indices, k, n, words_rows):
    out = np.full((words_rows, max(k, 1)), 0x5A5A5A5A5A5A5A5A, np.uint64)
    ip, ix = np.asarray(indptr, np.int32), np.asarray(indices, np.int32)
    rc = lib.bposd_observable_table(ip.ctypes.data, ix.ctypes.data, k, n, out.ctypes.data)
    return rc, out, lib.bposd_last_error(None).decode()


@pytest.mark.parametrize("what,indptr,indices,k,n", [
    ("k = 0", [0], [], 0, 70),
    ("k = 4097", [0] * 4098, [], 4097, 70),
    ("column n", [0, 1, 3], [5, 2, 70], 2, 70),
    ("column -1", [0, 1, 3], [5, -1, 7], 2, 70),
    ("not ascending", [0, 1, 3], [5, 9, 9], 2, 70),
    ("descending", [0, 1, 3], [5, 9, 8], 2, 70),
])
def test_observable_table_refusals_write_nothing(lib, what, indptr, indices, k, n):
    rc, out, msg = _c_call(lib, indptr, indices, k, n, 2)
    assert rc == _lib.BPOSD_ERR_INVALID and "bposd_observable_table" in msg, (what, rc, msg)
    assert (out == 0x5A5A5A5A5A5A5A5A).all(), "written in spite of the error"


def test_observable_table_python_refusals(lib):
    with pytest.raises(ValueError, match="outside 1"):
        BpOsdDecoder.observable_table(np.zeros((0, 70), np.uint8), 70)
    with pytest.raises(ValueError, match="outside 1"):
        BpOsdDecoder.observable_table(sp.csr_matrix((4097, 70), dtype=np.uint8), 70)
    with pytest.raises(ValueError, match="shape"):
        BpOsdDecoder.observable_table(np.zeros((3, 70), np.uint8), 71)
    # the cap itself and an all-zero matrix are fine; the valid C call overwrites the whole table
    assert BpOsdDecoder.observable_table(sp.csr_matrix((4096, 70), dtype=np.uint8), 70).shape == (2, 4096)
    rc, out, _ = _c_call(lib, [0, 1, 3], [5, 2, 69], 2, 70, 2)
    assert rc == 0 and out.tolist() == [[1 << 5, 1 << 2], [0, 1 << 5]]


# shots whose bp observables differ from the osdw observables / whose osd0 observables do, per table case, for the plain
# random L (seed 11, k = 65) on the oracle
def _differing(case_id, L_of):
    n = cr.matrix(cr.CASE_BY_ID[case_id]["code"]).shape[1]
    r = oc.reference(case_id, L_of(n, 65))
    return int((r["bp"] != r["osdw"]).any(axis=1).sum()), int((r["osd0"] != r["osdw"]).any(axis=1).sum())


@pytest.mark.parametrize("L_of", [oc.plain_matrix, oc.edge_matrix], ids=["plain", "edge_rows"])
def test_oracle_table_keeps_the_gpu_test_honest(L_of):
    assert len(cr.TABLE_IDS) == 13
    got = {i: _differing(i, L_of) for i in cr.TABLE_IDS}
    print(got)
    for i, (bp_differs, _) in got.items():
        assert bp_differs >= 1, f"{i}: no shot whose bp observables differ from the osdw observables"
    with_osd0 = [i for i, (_, osd0_differs) in got.items() if osd0_differs >= 1]
    assert len(with_osd0) >= 5, with_osd0


def test_edge_matrix_rows():
    for n, k in ((620, 65), (2050, 65), (64, 5)):
        L = oc.edge_matrix(n, k)
        assert L[1].all() and L[2].sum() == 1 and L[2, n - 1] and L[3].sum() == 1 and L[3, 0]
        assert L[k - 1].sum() == 1 and L[k - 1, (n - 1) & ~63]
        assert not L[0].any() or k - 1 == 0
