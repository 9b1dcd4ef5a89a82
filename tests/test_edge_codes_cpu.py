"""The edge table of tests/test_gpu_edges.py, checked without a GPU: every row's matrix has the exact shape, degrees and rank
the row asks for, and its window arithmetic (osd_kernel width, wave / mw / large-path windows, BP degree pair, shape and
LDS fit) agrees with the instance the row expects."""
import numpy as np
import pytest

from tests.edge_codes import (BP_PAIRS, EDGES, LDS_PER_CU, bp_lds_bytes, class_pcm, class_shape, edge_pcm, kprime,
                              order_of, osd_words, pcm_for)


def _bp_window(m, n, dc, dv, bp_variant=0):
    """bposd_create + pick_shape for a non-regular, non-class matrix: (kernel, template integers) of bp_kernel /
    bp_large_kernel / bp_anydeg_kernel."""
    pair = next(((a, b) for a, b in BP_PAIRS if a >= dc and b >= dv), None)
    if pair is None:
        return ("bp_anydeg_kernel", ())
    p2 = lambda x: 1 << max(6, (x - 1).bit_length())
    if bp_variant == 2 and p2(max(-(-m // 2), -(-n // 4))) <= 512:  # shape 2 on request
        assert bp_lds_bytes(pair[0], 2 * p2(max(-(-m // 2), -(-n // 4)))) <= LDS_PER_CU
        return ("bp_kernel", pair + (2, 512))
    if p2(max(m, -(-n // 2))) <= 1024:
        shape, mp = (1, 1024), p2(max(m, -(-n // 2)))
    elif p2(max(-(-m // 2), -(-n // 4))) <= 1024:
        shape, mp = (2, 1024), 2 * p2(max(-(-m // 2), -(-n // 4)))
    else:
        shape, mp = None, 0
    if shape and bp_lds_bytes(pair[0], mp) <= LDS_PER_CU:
        return ("bp_kernel", pair + shape)
    return ("bp_large_kernel", ((12, 6) if dc <= 12 and dv <= 6 else (16, 8)) + (2,))


def _class_stride(H):
    """The LDS stride the class layout search settles on (host only: the same search bposd_create runs)."""
    from bp_osd_amd import _lib

    lib = _lib.load()
    m, n = H.shape
    ip, ix = np.ascontiguousarray(H.indptr, np.int32), np.ascontiguousarray(H.indices, np.int32)
    info = np.zeros(11, np.int64)
    assert lib.bposd_debug_class_layout(ip.ctypes.data, ix.ctypes.data, m, n, None, None, None, None, None,
                                        info.ctypes.data) == 0
    return int(info[4])


@pytest.mark.parametrize("case", EDGES, ids=[c["id"] for c in EDGES])
def test_edge_matrix(case):
    from bp_osd_amd.codes import gf2_rank
    from oracle import OracleDecoder

    H = pcm_for(case)
    m, n = case["m"], case["n"]
    assert H.shape == (m, n) and H.dtype == np.uint8 and (H.data == 1).all()
    rdeg, cdeg = np.diff(H.indptr), np.bincount(H.indices, minlength=n)
    assert rdeg.min() >= 1 and cdeg.min() >= 1, "empty row or column"
    assert rdeg.max() == case["dc"] and cdeg.max() == case["dv"]
    assert not (rdeg.min() == rdeg.max() and cdeg.min() == cdeg.max()), "regular"
    rank = gf2_rank(H.toarray())
    assert rank == OracleDecoder(H, error_rate=0.05).rank == m - case["deficit"]
    assert n - rank == kprime(case) >= order_of(case)
    large = m > 1024 or osd_words(n) == 0 or case["bp"][0] == "bp_large_kernel"
    if case["order"] == "kprime":
        assert kprime(case) <= (64 if case["method"] == "osd_cs" else (16 if large else 20))
    if case.get("family") == "class":
        assert class_shape(H) == (3, 4, 1, 2)
        assert case["bp"][1][:3] == (3, 4, 2)
        assert _class_stride(H) == case["bp"][1][3]
        return
    assert class_shape(H) is None
    if case.get("schedule") != "serial":
        assert case["bp"] == _bp_window(m, n, case["dc"], case["dv"], case.get("bp_variant", 0))
    name, t = case["osd"]
    if large:
        assert name == "osd_large_kernel" and t == (next(r for r in (2, 4, 8, 16) if m <= 1024 * r),)
    elif name == "osd_kernel":
        assert t == (osd_words(n),)
        assert case["osd_variant"] == 1 or case["method"] == "osd_e" and order_of(case) > 12
    elif name == "osd_wave_kernel":
        assert case["osd_variant"] == 2 and m <= 320 and n + 1 <= 640
    else:
        assert name == "osd_mw_kernel" and not (m <= 320 and n + 1 <= 640)
        assert t == {1: (2, 4, 15, 3), 2: (4, 3, 20, 2), 3: (8, 2, 31, 2)}[1 if m <= 512 and n < 960 else (2 if m <= 768 and n < 1280 else 3)]


def test_edge_table_covers_every_window_edge():
    """The osd_kernel widths at both sides of every width edge, the osd_rowbuf_extra switch, the wave and mw corners, the
    RPT switches of the HBM path, every bp_kernel pair and the LDS edge of BP shape 8 (check degree 8 fits, 9 does not)."""
    ids = {c["id"] for c in EDGES}
    seen = {(c["osd"][0], c["osd"][1]) for c in EDGES}
    for W in (1, 2, 4, 8, 16, 24, 31, 32):
        assert ("osd_kernel", (W,)) in seen
        assert f"osd_kernel_W{W}_n{64 * W - 1}" in ids
    for t in ((1, 2), (2, 4), (3, 7), (5, 10)):
        assert ("osd_wave_kernel", t) in seen
    for t in ((2, 4, 15, 3), (4, 3, 20, 2), (8, 2, 31, 2)):
        assert ("osd_mw_kernel", t) in seen
    for r in (2, 4, 8):
        assert ("osd_large_kernel", (r,)) in seen
    bps = {c["bp"] for c in EDGES}
    for dc, dv in BP_PAIRS:
        assert ("bp_kernel", (dc, dv, 1, 1024)) in bps
    assert bp_lds_bytes(8, 2048) <= LDS_PER_CU < bp_lds_bytes(12, 2048)
    assert {"bp_shape8_m1025_dc8", "bp_hbm_m1025_dc9", "bp_shape8_m2048_dc6", "bp_hbm_m2049_dv6", "bp_hbm_m2049_dv7"} <= ids
    for name in ("bp_anydeg_kernel", "bp_serial_kernel"):
        assert (name, ()) in bps
    assert {c["bp"][1][3] for c in EDGES if c["bp"][0] == "bp_class_kernel"} == {256, 512, 1024}
    assert ("bp_kernel", (8, 4, 2, 512)) in bps and ("bp_kernel", (8, 4, 2, 1024)) in bps


def test_edge_pcm_is_deterministic_and_checks_its_arguments():
    a = edge_pcm(100, 210, 8, 4, rank_deficit=2, seed=3)
    b = edge_pcm(100, 210, 8, 4, rank_deficit=2, seed=3)
    assert (a != b).nnz == 0
    assert (a != edge_pcm(100, 210, 8, 4, rank_deficit=2, seed=4)).nnz > 0
    c = class_pcm(60, 160, rank_deficit=2, seed=1)
    assert class_shape(c) == (3, 4, 1, 2)
    with pytest.raises(ValueError):
        edge_pcm(100, 50, 8, 4, rank_deficit=1)  # more independent rows than columns
