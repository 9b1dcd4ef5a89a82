"""The product-sum table of tests/test_gpu_ps_edges.py, checked without a GPU: every PS_EDGES row's matrix builds with the
check degrees the table states, the class rows land on their LDS stride, the table names every BP instance the issue lists,
and the CPU oracle ALONE -- both evaluation orders, every run of the row -- meets the conditions the GPU module rests on:
the share of shots it has to exclude (LLRs that mix numbers and NaN) stays within the cap, clipped runs are finite,
unclipped ones saturate where the table says so, short runs leave most shots to OSD."""
import numpy as np
import pytest

from tests.edge_codes import (BP_PAIRS, EDGE_BY_ID, PS_EDGES, class_shape, ps_case_id, ps_cases, ps_oracle_conditions,
                              ps_oracle_select, ps_pcm, ps_select, ps_settings)
from tests.test_edge_codes_cpu import _class_stride
from tests.test_gpu_edges import _syndromes

_IDS = [r["id"] for r in PS_EDGES]


@pytest.mark.parametrize("row", PS_EDGES, ids=_IDS)
def test_ps_row_matrix(row):
    H = ps_pcm(row)
    m, n = H.shape
    assert H.dtype == np.uint8 and (H.data == 1).all()
    rdeg, cdeg = np.diff(H.indptr), np.bincount(H.indices, minlength=n)
    assert rdeg.min() >= 1 and cdeg.min() >= 1
    assert (int((rdeg == 1).sum()), int((rdeg == 2).sum())) == (row["deg1"], row["deg2"])
    if row["edge"]:
        e = EDGE_BY_ID[row["edge"]]
        assert (m, n, rdeg.max(), cdeg.max()) == (e["m"], e["n"], e["dc"], e["dv"])
        assert row["bp"][0] == e["bp"][0] and row["bp"][1][:2] == e["bp"][1][:2]
        assert row["shots"] == (e.get("shots") or (38, 8)) and (m <= 1024 or row["shots"] == (7, 2))
    name, t = row["bp"]
    if name == "bp_class_kernel":
        s = class_shape(H)
        assert s is not None and (s[0], s[1], s[3]) == t[:3]
        assert _class_stride(H) == t[3] == row["stride"]
    elif name == "bp_kernel" and row.get("code") == "h1922_hz":
        # (3,6)-regular with stride 1024: the class kernel would take it (it does for min-sum batches the local-edge kernel
        # leaves), product-sum goes to bp_kernel<6, 3, REG> -- launch_bp_class.hip class_preferred
        assert class_shape(H) == (6, 6, 3, 3) and _class_stride(H) == 1024 and t[:2] == (6, 3)
    else:
        assert class_shape(H) is None
    if name == "bp_large_kernel":
        assert t[2] == 0
    assert row["sat12"] or name in ("bp_class_kernel",)


@pytest.mark.parametrize("row", PS_EDGES, ids=_IDS)
def test_ps_row_oracle_alone(row):
    """Every run of the row on the oracle: the exclusion cap and the non-triviality conditions (ps_oracle_conditions)."""
    from oracle import OracleDecoder

    H = ps_pcm(row)
    n = H.shape[1]
    syn, c = _syndromes(H, row)
    assert c == row["shots"][0] + 1 and len(syn) == sum(row["shots"]) + 2
    for case in ps_cases(row):
        if case["kind"] == "packed":  # the same decode as the uniform run, other host interface
            continue
        o = OracleDecoder(H, ps_math=2 - case["form"], **ps_settings(row, case, n))
        if case["kind"] == "select":
            ref = ps_oracle_select(o, syn, *ps_select(row, len(syn), n))
        else:
            ref = o.decode_batch(syn)
        try:
            ps_oracle_conditions(row, case, ref, syn)
        except AssertionError as e:
            raise AssertionError(f"{ps_case_id(case)}: {e}") from None


def test_ps_table_covers_every_bp_instance():
    bps = {r["bp"] for r in PS_EDGES}
    ids = set(_IDS)
    for dc, dv in BP_PAIRS:
        assert ("bp_kernel", (dc, dv, 1, 1024)) in bps and f"bp_pair_{dc}_{dv}" in ids
    assert {"bp_shape1_m1024_n2048_dc16", "bp_shape2_m1024_n2048_variant2", "bp_shape8_m1025_dc6", "bp_shape8_m1025_dc8",
            "bp_shape8_m2048_dc6", "bp_hbm_m1025_dc9", "bp_hbm_m2049_dv6", "bp_hbm_m1024_n2049_dc16", "bp_hbm_m2049_dv7",
            "bp_serial_dv8", "bp_anydeg_dc17", "bp_anydeg_dv9"} <= ids
    assert ("bp_kernel", (8, 4, 2, 512)) in bps
    assert {("bp_kernel", (6, 3, 2, 1024)), ("bp_kernel", (8, 4, 2, 1024))} <= bps  # shape 8
    reg = {r["bp"][1][2:]: r["bp_variant"] for r in PS_EDGES if r.get("code") == "h1922_hz"}
    assert reg == {(1, 1024): 1, (2, 512): 0, (4, 256): 4}
    cls = [r["bp"][1] for r in PS_EDGES if r["bp"][0] == "bp_class_kernel"]
    assert {t for t in cls if t[:3] == (3, 4, 2)} == {(3, 4, 2, 256), (3, 4, 2, 512), (3, 4, 2, 1024)}
    assert {t[:3] for t in cls} == {(3, 4, 2), (7, 7, 4), (6, 6, 3), (4, 4, 2), (8, 8, 4)}
    assert any(t[:3] == (6, 6, 3) and t[3] < 1024 for t in cls)
    assert {("bp_large_kernel", (12, 6, 0)), ("bp_large_kernel", (16, 8, 0)), ("bp_serial_kernel", ()),
            ("bp_anydeg_kernel", ())} <= bps
    # each family runs the per-bit channel, the per-shot channel and the packed host API on at least one row (the serial and
    # the any-degree kernel have no packed instance: unpack / pack kernels surround them, internal.h native_packed)
    fam = lambda r: "bp_kernel_reg" if r.get("code") == "h1922_hz" else r["bp"][0]
    for f in ("bp_kernel", "bp_kernel_reg", "bp_class_kernel", "bp_large_kernel", "bp_serial_kernel", "bp_anydeg_kernel"):
        have = set().union(*[set(r["extras"]) for r in PS_EDGES if fam(r) == f])
        assert {"channel", "select"} <= have, f
        assert "packed" in have or f in ("bp_serial_kernel", "bp_anydeg_kernel"), f
    assert any(r["deg1"] for r in PS_EDGES if fam(r) == "bp_kernel") and any(r["deg1"] for r in PS_EDGES if fam(r) == "bp_large_kernel")
