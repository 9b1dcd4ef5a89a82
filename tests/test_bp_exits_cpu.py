"""The row table of tests/test_gpu_bp_exits.py, checked without a GPU: every EXIT_ROWS matrix has the shape and degrees that
put the dispatch on the row's instance (class rows: the LDS stride the layout search settles on), the oracle ALONE yields
every required case of the min-sum plan, a row still unconverged after 56 iterations of the adaptive factor and every case of
the product-sum plan, every batch holds every pool row, and the table names every instance the other BP families have."""
import numpy as np
import pytest

from tests.bp_exit_cases import (B_CLASS, B_CLASS_QUEUE, B_GENERIC, CASES, CASES_WITHOUT_MAX_ITER_1, EXIT_ROWS, N_POOL, _occurred,
                                 batch_index, exit_matrix, exit_plan, has_ps, select_reference)
from tests.edge_codes import BP_PAIRS, CLASS_SHAPES, _deg_pair, class_shape, osd_words
from tests.test_edge_codes_cpu import _bp_window, _class_stride

_IDS = [r["id"] for r in EXIT_ROWS]


@pytest.mark.parametrize("row", EXIT_ROWS, ids=_IDS)
def test_exit_row_matrix(row):
    H = exit_matrix(row)
    m, n = H.shape
    assert H.dtype == np.uint8 and (H.data == 1).all()
    rdeg, cdeg = np.diff(H.indptr), np.bincount(H.indices, minlength=n)
    assert rdeg.min() >= 1 and cdeg.min() >= 1
    dc, dv = int(rdeg.max()), int(cdeg.max())
    regular = rdeg.min() == dc and cdeg.min() == dv
    name, t = row["bp"]
    fam = row["family"]
    assert name == (fam if fam != "bp_kernel_reg" else "bp_kernel")
    assert row["large_osd"] == (m > 1024 or osd_words(n) == 0 or name == "bp_large_kernel")
    if fam == "bp_class_kernel":
        s = class_shape(H)
        assert s in CLASS_SHAPES and (s[0], s[1], s[3]) == t[:3]
        assert _class_stride(H) == t[3] == row["stride"]
        # a (3,6)-regular code goes to the local-edge kernel unless the class kernel is asked for
        assert (row.get("bp_variant") == 32) == (regular and (dc, dv) == (6, 3)) == (row.get("env") == {"BPOSD_CLASS_ALWAYS": "1"})
        # m <= 160: eight shots per queue atomic (launch_bp_class.hip); one such row also runs the batch where that count falls
        assert row["batches"] in ((B_CLASS, B_CLASS_QUEUE), (B_CLASS,)) and (m <= 160 or row["batches"] == (B_CLASS,))
        if t[:3] == (3, 4, 2) and t[3] == 256:
            assert m in (150, 161)
        return
    assert row["batches"] == (B_GENERIC,)
    if fam == "bp_kernel_reg":  # bp_kernel<6, 3, REG>: compiled for stride 1024, shape on request
        assert regular and (dc, dv) == (6, 3) and n == 2 * m and m <= 1024 // 4
        assert t == (6, 3, row["bp_variant"], 1024 // row["bp_variant"])
        return
    if fam == "bp_serial_kernel":
        assert row["schedule"] == "serial" and dv == 8 and t == ()
        return
    assert not regular and "schedule" not in row
    if fam == "bp_anydeg_kernel":
        assert _deg_pair(dc, dv) is None and t == ()
        return
    # bp_kernel / bp_large_kernel: no degree class takes the matrix, or the row asks for shape 1 by number
    assert class_shape(H) is None or row.get("bp_variant") == 1
    assert row["bp"] == _bp_window(m, n, dc, dv, row.get("bp_variant", 0))
    if name == "bp_kernel":
        assert _deg_pair(dc, dv) == t[:2] and t[:2] in BP_PAIRS


@pytest.mark.parametrize("row", EXIT_ROWS, ids=_IDS)
def test_exit_row_oracle_alone(row):
    """The three plans of the row on the oracle (exit_plan asserts their cases), and the batches."""
    p = exit_plan(row["id"], "ms")
    assert 3 <= p["k"] < 30 and p["max_iters"] == (p["k"] + 1, p["k"], p["k"] - 1, 1) and p["cases"] == CASES
    seen = set().union(*[_occurred(p["refs"][mi], p["target"], p["k"], mi) for mi in p["max_iters"]])
    assert seen == set(CASES)
    assert p["kw"]["ms_scaling_factor"] == row["factor"] and p["kw"]["osd_method"] == ("osd_off" if row["large_osd"] else "osd0")
    assert ("refs_osd0" in p) == row["large_osd"]
    f = exit_plan(row["id"], "f56")
    left = f["ref"]["converged"] == 0
    assert f["kw"]["ms_scaling_factor"] == 0.0 and left[f["target"]] and (f["ref"]["iters"][left] == 56).all()
    assert np.isfinite(f["ref"]["llr"]).all()
    targets = [p["target"], f["target"]]
    if has_ps(row):
        s = exit_plan(row["id"], "ps")
        assert 3 <= s["k"] < 30 and s["max_iters"] == (s["k"] + 1, s["k"], s["k"] - 1) and s["cases"] == CASES_WITHOUT_MAX_ITER_1
        assert s["kw"]["ps_clip"] > 0 and all(np.isfinite(r["llr"]).all() for r in s["refs"].values())
        targets.append(s["target"])
    else:
        assert isinstance(row["ps"], str) and row["ps"]
    sel, alt, ref = select_reference(row, p)
    assert sel.shape == (N_POOL, p["H"].shape[1]) and 0 < sel.mean() < 1 and len(ref["iters"]) == N_POOL
    for B in row["batches"]:
        for t in targets:
            idx = batch_index(B, t)
            assert len(idx) == B and idx[0] == idx[-1] == t and set(idx) == set(range(N_POOL))
            assert tuple(idx[1:3]) == (0, 1) and tuple(idx[-3:-1]) == (1, 0)


def test_batches_exceed_twice_the_largest_grid():
    """256 CUs; a kernel of at least 256 threads fits 8 workgroups per CU (32 waves), bp_class_kernel caps at 16: a batch above
    twice the grid gives some workgroup a third shot."""
    assert B_GENERIC > 2 * 256 * 8 and B_CLASS > 2 * 256 * 16 and B_CLASS_QUEUE > 8 * 2 * 256 * 16
    assert B_GENERIC % 2 and B_CLASS % 2 and B_CLASS_QUEUE % 2


def test_table_covers_every_instance():
    bps = {(r["bp"], r.get("bp_variant", 0)) for r in EXIT_ROWS}
    inst = {r["bp"] for r in EXIT_ROWS}
    for dc, dv in BP_PAIRS:  # predicated, one check per thread
        assert ("bp_kernel", (dc, dv, 1, 1024)) in {r["bp"] for r in EXIT_ROWS if r["family"] == "bp_kernel"}
    reg = {r["bp"][1] for r in EXIT_ROWS if r["family"] == "bp_kernel_reg"}
    assert reg == {(6, 3, 1, 1024), (6, 3, 2, 512), (6, 3, 4, 256)}
    assert (("bp_kernel", (8, 4, 2, 512)), 2) in bps  # shape 2 on request
    assert {("bp_kernel", (8, 4, 2, 1024)), ("bp_kernel", (6, 3, 2, 1024))} <= inst  # shape 8 at two degree pairs
    cls = [r["bp"][1] for r in EXIT_ROWS if r["family"] == "bp_class_kernel"]
    assert {t for t in cls if t[:3] == (3, 4, 2)} == {(3, 4, 2, 256), (3, 4, 2, 512), (3, 4, 2, 1024)}
    assert {t[:3] for t in cls} == {(s[0], s[1], s[3]) for s in CLASS_SHAPES}
    assert any(B_CLASS_QUEUE in r["batches"] for r in EXIT_ROWS) and sum(r["bp"][1] == (3, 4, 2, 256) for r in EXIT_ROWS) == 2
    assert {("bp_large_kernel", (12, 6, 2)), ("bp_large_kernel", (16, 8, 2)), ("bp_anydeg_kernel", ()),
            ("bp_serial_kernel", ())} <= inst
    for i, r in enumerate(EXIT_ROWS):
        assert r["factor"] == (0.625, 0.0)[i % 2], r["id"]
    for fam in ("bp_kernel", "bp_kernel_reg", "bp_class_kernel", "bp_large_kernel", "bp_anydeg_kernel", "bp_serial_kernel"):
        rows = [r for r in EXIT_ROWS if r["family"] == fam]
        assert {r["probs"] for r in rows} == {"uniform", "channel"}, fam
        assert any(has_ps(r) for r in rows), fam
    assert {r["ps"]["form"] for r in EXIT_ROWS if has_ps(r)} == {0, 1}
