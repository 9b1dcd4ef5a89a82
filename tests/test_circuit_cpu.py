"""Circuit-level noise on the host (bp_osd_amd/circuit.py): the numpy engine against an independent
per-fault reference, the memory-experiment builder against ``phenomenological_dem``, the depolarising formulas against an
enumeration, hand-derived columns, annotations, merging, and the text writer.  tests/test_gpu_circuit.py holds the device
engine to the numpy engine."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from bp_osd_amd import _lib, phenomenological_dem, phenomenological_detector_times
from bp_osd_amd.build import build_library
from bp_osd_amd.circuit import (Circuit, check_annotations, circuit_dem, dem_text, depolarize1_mechanism, depolarize2_mechanism, fault_columns,
                                greedy_edge_colouring, make_faults)
from tests import circuit_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def numpy_columns(circuit, faults=None, max_words=0):
    return cc.engine_columns(fault_columns(circuit, faults, engine="numpy", max_words=max_words))


# ------------------------------------------------------------------------------------------- numpy engine == reference
@pytest.mark.parametrize("F", [1, 63, 64, 65, 129, 300])
def test_numpy_engine_equals_the_reference_on_every_opcode(F):
    c = cc.opcode_circuit()
    fa = cc.random_faults(c, F, seed=F)
    assert numpy_columns(c, fa) == cc.reference_columns(c, fa)


@pytest.mark.parametrize("max_words", [1, 3, 9])
def test_numpy_engine_chunks_give_the_same_columns(max_words):
    c = cc.opcode_circuit()
    fa = cc.random_faults(c, 64 * 7 + 5, seed=3)
    assert numpy_columns(c, fa, max_words) == cc.reference_columns(c, fa)


@pytest.mark.parametrize("kind", cc.ANNOTATION_KINDS)
def test_numpy_engine_equals_the_reference_on_annotation_shapes(kind):
    c, F = cc.annotation_circuit(kind)
    fa = cc.random_faults(c, F, seed=11)
    got = numpy_columns(c, fa)
    assert got == cc.reference_columns(c, fa)
    assert any(h or l for h, l in got)  # (the case is not empty)


@pytest.mark.parametrize("positions", [[None], [0, None], [3]], ids=["all_at_T", "0_and_T", "one_position"])
def test_numpy_engine_equals_the_reference_at_position_edges(positions):
    c = cc.opcode_circuit()
    fa = cc.random_faults(c, 70, seed=2, positions=[c.T if p is None else p for p in positions])
    assert numpy_columns(c, fa) == cc.reference_columns(c, fa)


@pytest.mark.parametrize("name,basis", cc.BUILDER_CASES)
def test_numpy_engine_equals_the_reference_on_builder_circuits(name, basis):
    c = cc.builder_circuit(name, basis, 2, cc.FULL_NOISE)
    assert numpy_columns(c) == cc.reference_columns(c)


# ------------------------------------------------------------------------------------------- phenomenological yardstick
def model_columns(H, L, priors):
    Hc, Lc = H.tocsc(), L.tocsc()
    Hc.sort_indices()
    Lc.sort_indices()
    return sorted((tuple(Hc.indices[Hc.indptr[i]:Hc.indptr[i + 1]].tolist()), tuple(Lc.indices[Lc.indptr[i]:Lc.indptr[i + 1]].tolist()), float(priors[i]))
                  for i in range(Hc.shape[1]))


@pytest.mark.parametrize("rounds", cc.BUILDER_ROUNDS)
@pytest.mark.parametrize("name,basis", cc.BUILDER_CASES)
def test_builder_with_data_and_measurement_noise_is_the_phenomenological_model(name, basis, rounds):
    """Only ``data = p`` and ``meas = q``: the reduced model is ``phenomenological_dem`` as a multiset of columns.

    The columns that merge are the n data columns of the last layer (t = rounds): the data fault in front of the
    transversal measurement and the flip of that measurement have the same column, so the mechanism's prior is
    p (1 - q) + q (1 - p), which is held to 4 ulp of p + q - 2 p q.  Every other column is one elementary fault (flips of
    the other basis' ancilla outcomes have empty columns and are dropped) and its prior is p or q to the last bit."""
    p, q = 0.01, 0.003
    hx, hz, lx, lz = cc.builder_code(name)
    h, l = (hz, lz) if basis == "z" else (hx, lx)
    m, n = h.shape
    c = cc.builder_circuit(name, basis, rounds, {"data": p, "meas": q})
    H, L, priors, detector_time, origin = circuit_dem(c, engine="numpy")
    He, Le, pe = phenomenological_dem(h, l, rounds, p, q)
    assert H.shape == He.shape and L.shape == Le.shape
    assert np.array_equal(detector_time, phenomenological_detector_times(m, rounds))
    last = np.arange(rounds * n, (rounds + 1) * n)
    exact = pe.copy()
    exact[last] = p + q - 2 * p * q
    got, want = model_columns(H, L, priors), model_columns(He, Le, exact)
    assert [g[:2] for g in got] == [w[:2] for w in want]
    merged = {w[:2] for w in model_columns(He[:, last], Le[:, last], exact[last])}
    sizes = np.diff(origin[0])
    assert sorted(sizes.tolist()) == [1] * (He.shape[1] - n) + [2] * n
    for g, w in zip(got, want):
        if g[:2] in merged:
            assert abs(g[2] - w[2]) <= 4 * np.spacing(w[2]), (g, w)
        else:
            assert g[2] == w[2], (g, w)


def test_greedy_edge_colouring_layers_are_disjoint_and_cover_every_edge():
    hx, hz, _, _ = cc.builder_code("surface13")
    for h in (hx, hz):
        layers = greedy_edge_colouring(h)
        edges = sorted(e for layer in layers for e in layer)
        assert edges == sorted(zip(*[a.tolist() for a in h.nonzero()]))
        for layer in layers:
            assert len({c for c, _ in layer}) == len(layer) == len({b for _, b in layer})


# ------------------------------------------------------------------------------------------------ depolarising formulas
@pytest.mark.parametrize("p", [1e-3, 0.1, 0.5])
@pytest.mark.parametrize("n_mech", [3, 15])
def test_depolarising_mechanisms_compose_to_equal_net_probabilities(n_mech, p):
    """All 2^3 / 2^15 firing patterns of the independent mechanisms, summed per net Pauli: p/3 resp. p/15 each.

    Tolerance, from the enumeration's own fp64 error with u = 2^-53: a pattern's probability is a product of n_mech factors,
    each either e or the rounded 1 - e: at most 2 n_mech roundings, relative error (2 n_mech + 2) u to first order.  The sum
    per class is math.fsum, exact but for one rounding.  The mechanism probability e carries an absolute error of at most
    2 u (one rounding in the root, one in the subtraction), and a net probability moves by at most one per unit of each of the
    n_mech mechanisms.  So |net - exact| <= ((2 n_mech + 3) S + 2 n_mech) u with S the class sum (S <= 1)."""
    e = depolarize1_mechanism(p) if n_mech == 3 else depolarize2_mechanism(p)
    patterns = np.arange(1 << n_mech)
    fired = (patterns[:, None] >> np.arange(n_mech)) & 1
    prob = np.prod(np.where(fired, e, 1.0 - e), axis=1)
    net = np.bitwise_xor.reduce(fired * (np.arange(n_mech) + 1), axis=1)
    u = 2.0 ** -53
    for pauli in range(1, n_mech + 1):
        s = math.fsum(prob[net == pauli].tolist())
        tol = ((2 * n_mech + 3) * s + 2 * n_mech) * u
        assert abs(s - p / n_mech) <= tol, (pauli, s, p / n_mech, tol)


def test_channels_expand_into_independent_faults_and_refuse_large_p():
    c = Circuit(2)
    c.depolarize1(0.3, 0)
    c.depolarize2(0.3, 0, 1)
    c.x_error(0.0, 0)  # nothing
    fa = c.faults
    assert len(fa) == 18 and (fa.pa != 0).all()
    pairs = {(int(a), int(pa), int(b), int(pb)) for a, pa, b, pb in zip(fa.qa[3:], fa.pa[3:], fa.qb[3:], fa.pb[3:])}
    want = {(0, a, 1, b) for a in (1, 2, 3) for b in (1, 2, 3)} | {(0, a, -1, 0) for a in (1, 2, 3)} | {(1, b, -1, 0) for b in (1, 2, 3)}
    assert pairs == want
    with pytest.raises(ValueError):
        c.depolarize1(0.76, 0)
    with pytest.raises(ValueError):
        c.depolarize2(0.94, 0, 1)


def test_faults_are_sorted_by_position_then_insertion():
    c = Circuit(2)
    c.h(0)
    c.h(1)
    c.fault(0.1, 0, 1)            # pos 2
    c.fault(0.2, 1, 2, pos=0)
    c.fault(0.3, 0, 3, pos=2)
    c.fault(0.4, 1, 1, pos=0)
    assert c.faults.prob.tolist() == [0.2, 0.4, 0.1, 0.3] and c.faults.pos.tolist() == [0, 0, 2, 2]


# -------------------------------------------------------------------------------------------------- hand-derived columns
def single(c, *fault):
    """The column of one fault (prob, qa, pa[, qb, pb, pos]) of circuit c, by the numpy engine and by the reference."""
    c.fault(*fault[:5], pos=fault[5])
    got = numpy_columns(c)
    assert got == cc.reference_columns(c)
    return got[0]


def test_x_on_a_cx_control_flips_both_later_z_measurements():
    c = Circuit(2)
    c.cx(0, 1)
    c.detector([c.m(0)])
    c.detector([c.m(1)])
    assert single(c, 0.1, 0, 1, -1, 0, 0) == ((0, 1), ())


def test_z_on_a_cx_target_reaches_only_an_mx_of_the_control():
    c = Circuit(2)
    c.cx(0, 1)
    c.detector([c.mx(0)])
    c.detector([c.m(1)])
    c.detector([c.m(0)])
    assert single(c, 0.1, 1, 2, -1, 0, 0) == ((0,), ())


def test_y_before_s_then_h_is_a_z():
    c = Circuit(1)
    c.s(0)
    c.h(0)
    c.detector([c.m(0)])
    c.detector([c.mx(0)])
    assert single(c, 0.1, 0, 3, -1, 0, 0) == ((1,), ())


def test_a_fault_behind_the_last_op_has_an_empty_column():
    c = Circuit(1)
    c.detector([c.m(0)])
    c.observable([0])
    assert single(c, 0.1, 0, 3, -1, 0, 1) == ((), ())


def test_a_fault_directly_before_a_reset_has_an_empty_column():
    c = Circuit(2)
    c.h(0)
    c.r(0)
    c.cx(0, 1)
    c.detector([c.m(0)])
    c.detector([c.m(1)])
    assert single(c, 0.1, 0, 3, -1, 0, 1) == ((), ())


# ----------------------------------------------------------------------------------------------------------- annotations
@pytest.mark.parametrize("name,basis", cc.BUILDER_CASES)
def test_builder_annotations_are_deterministic_under_full_noise(name, basis):
    check_annotations(cc.builder_circuit(name, basis, 3, cc.FULL_NOISE), engine="numpy")


def test_an_x_check_outcome_is_no_detector_of_a_basis_z_memory():
    hx, hz, _, _ = cc.builder_code("surface13")
    c = cc.builder_circuit("surface13", "z", 2, cc.FULL_NOISE)
    bad = c.detector([hz.shape[0]], 0)  # round 0: the Z outcomes come first, then X check 0
    with pytest.raises(ValueError, match=rf"detector {bad} is not deterministic"):
        check_annotations(c, engine="numpy")


def test_gauge_faults_sit_behind_resets_and_measurements():
    c = cc.opcode_circuit()
    g = c.gauge_faults()
    ops = c.ops
    assert (np.diff(g.pos) >= 0).all() and (g.qb == -1).all()
    want = sorted([(0, q, 2) for q in range(c.Q)] + [(t + 1, int(a), 2 if op in (0, 2, 4) else 1) for t, (op, a, _) in enumerate(ops) if op < 6])
    assert sorted(zip(g.pos.tolist(), g.qa.tolist(), g.pa.tolist())) == want


def test_annotations_refuse_a_measurement_out_of_range():
    c = Circuit(1)
    c.m(0)
    with pytest.raises(ValueError, match="measurement 1"):
        c.detector([0, 1])


# --------------------------------------------------------------------------------------------------------------- merging
def merging_circuit():
    c = Circuit(2)
    c.fault(0.01, 0, 1)          # 0: X0, becomes X0 X1
    c.fault(0.5, 0, 2)           # 1: Z0: empty column
    c.cx(0, 1)
    c.fault(0.02, 0, 1, 1, 1)    # 2: X0 X1
    c.fault(0.04, 0, 1)          # 3: X0 alone: the observable only
    c.fault(0.03, 1, 1, 0, 1)    # 4: X1 X0
    m0, m1 = c.m(0), c.m(1)
    c.detector([m1], 0)
    c.observable([m0])
    return c


def test_equal_columns_merge_in_ascending_fault_order():
    H, L, priors, _, (optr, oidx) = circuit_dem(merging_circuit(), engine="numpy")
    fold = lambda a, b: a * (1 - b) + b * (1 - a)
    assert H.toarray().tolist() == [[1, 0]] and L.toarray().tolist() == [[1, 1]]
    assert priors.tolist() == [fold(fold(0.01, 0.02), 0.03), 0.04]
    assert optr.tolist() == [0, 3, 4] and oidx.tolist() == [0, 2, 4, 3]
    assert H.dtype == np.uint8 and L.dtype == np.uint8 and H.format == "csr" and L.format == "csr"


def test_without_merging_every_non_empty_column_stays():
    H, L, priors, _, (optr, oidx) = circuit_dem(merging_circuit(), engine="numpy", merge=False)
    assert H.toarray().tolist() == [[1, 1, 0, 1]] and L.toarray().tolist() == [[1, 1, 1, 1]]
    assert priors.tolist() == [0.01, 0.02, 0.04, 0.03] and oidx.tolist() == [0, 2, 3, 4] and optr.tolist() == [0, 1, 2, 3, 4]


def test_merged_builder_model_keeps_every_fault_once():
    c = cc.builder_circuit("surface13", "z", 2, cc.FULL_NOISE)
    H, L, priors, _, (optr, oidx) = circuit_dem(c, engine="numpy")
    cols = numpy_columns(c)
    assert sorted(oidx.tolist()) == [i for i, col in enumerate(cols) if col[0] or col[1]]
    first = oidx[optr[:-1]]
    assert (np.diff(first) > 0).all()  # mechanisms in the order of their first fault
    Hc, Lc = H.tocsc(), L.tocsc()
    for j in range(H.shape[1]):
        col = (tuple(Hc.indices[Hc.indptr[j]:Hc.indptr[j + 1]].tolist()), tuple(Lc.indices[Lc.indptr[j]:Lc.indptr[j + 1]].tolist()))
        members = oidx[optr[j]:optr[j + 1]]
        assert (np.diff(members) > 0).all() and all(cols[i] == col for i in members)
        want = 0.0
        for i in members:
            want = want * (1 - c.faults.prob[i]) + c.faults.prob[i] * (1 - want)
        assert priors[j] == want
    assert len({(tuple(Hc.indices[Hc.indptr[j]:Hc.indptr[j + 1]]), tuple(Lc.indices[Lc.indptr[j]:Lc.indptr[j + 1]])) for j in range(H.shape[1])}) == H.shape[1]


# ------------------------------------------------------------------------------------------------------------------ text
def read_dem_text(text):
    """The ten-line reader of the round trip: error(p) D.. L.. and detector(t) Dd lines."""
    errors, times = [], {}
    for line in text.splitlines():
        head, *targets = line.split()
        kind, arg = head[:-1].split("(")
        if kind == "error":
            errors.append((float(arg), [int(t[1:]) for t in targets if t[0] == "D"], [int(t[1:]) for t in targets if t[0] == "L"]))
        else:
            assert kind == "detector" and len(targets) == 1
            times[int(targets[0][1:])] = int(arg)
    return errors, times


def test_dem_text_round_trips():
    c = cc.builder_circuit("surface13", "x", 2, cc.FULL_NOISE)
    H, L, priors, detector_time, _ = circuit_dem(c, engine="numpy")
    errors, times = read_dem_text(dem_text(H, L, priors, detector_time))
    assert [e[0] for e in errors] == priors.tolist()
    Hd, Ld = np.zeros(H.shape, np.uint8), np.zeros(L.shape, np.uint8)
    for i, (_, dets, obs) in enumerate(errors):
        Hd[dets, i] = 1
        Ld[obs, i] = 1
    assert np.array_equal(Hd, H.toarray()) and np.array_equal(Ld, L.toarray())
    assert [times[d] for d in range(H.shape[0])] == detector_time.tolist()
    assert "detector" not in dem_text(H, L, priors)


# ----------------------------------------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def lib():
    build_library()
    return _lib.load()


def test_the_frame_calls_are_declared_and_listed_for_export(lib):
    public = open(os.path.join(ROOT, "include", "bposd_mi355x.h")).read()
    debug = open(os.path.join(ROOT, "include", "bposd_mi355x_debug.h")).read()
    for name in ("bposd_frame_create", "bposd_frame_columns", "bposd_frame_fetch", "bposd_frame_device_bytes", "bposd_frame_last_error",
                 "bposd_frame_destroy"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and f"{name}(" in public, name
    assert "bposd_debug_frame_timing" in _lib.DEBUG_SYMBOLS and "int bposd_debug_frame_timing(" in debug
    from bp_osd_amd.circuit import OPCODES

    for name, value in OPCODES.items():
        assert f"BPOSD_FRAME_OP_{name} = {value}" in public, name


def frame_create(lib, ops, Q, n_meas, md, mo, M, k):
    ops = np.ascontiguousarray(ops, np.int32).reshape(-1, 3)
    a = [np.ascontiguousarray(v, np.int32) for v in (md[0], md[1], mo[0], mo[1])]
    cfg = _lib.BposdFrameConfig(device=0, layered=0, max_words=0, workspace_bytes=0)
    h = C.c_void_p()
    rc = lib.bposd_frame_create(C.byref(cfg), ops.ctypes.data, ops.shape[0], Q, n_meas, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data,
                                a[3].ctypes.data, M, k, C.byref(h))
    return rc, h, (lib.bposd_frame_last_error(None) or b"").decode()


@pytest.mark.parametrize("what,ops,n_meas,md,match", [
    ("qubit", [[6, 2, 0], [2, 0, 0]], 1, ([0, 1], [0]), "qubit a = 2"),
    ("qubit_b", [[8, 0, 5], [2, 0, 0]], 1, ([0, 1], [0]), "qubit b = 5"),
    ("same", [[9, 1, 1], [2, 0, 0]], 1, ([0, 1], [0]), "a == b == 1"),
    ("opcode", [[10, 0, 0], [2, 0, 0]], 1, ([0, 1], [0]), "opcode 10"),
    ("measurements", [[2, 0, 0]], 2, ([0, 1, 1], [0]), "measurement index is out of range"),
    ("detector", [[2, 0, 0]], 1, ([0, 1], [1]), "outside"),
])
def test_create_refuses_before_it_touches_a_device(lib, what, ops, n_meas, md, match):
    rc, h, msg = frame_create(lib, ops, 2, n_meas, md, ([0] * (n_meas + 1), []), 1, 0)
    assert rc == _lib.BPOSD_ERR_INVALID and not h.value and match in msg, msg
