"""Frame propagation on the MI355X (bposd_frame_*, ``circuit_dem(engine="native")``): the CSC columns of H and
L over the elementary faults are exactly those of ``engine="numpy"`` -- integers, no tolerance -- at the fault counts, chunk
sizes, fault positions and annotation shapes at which the kernels can go wrong; then the whole path into the DEM engines, and
the refusals.  The outputs are pre-filled with a sentinel (``prefill``).  Circuits and fault lists:
tests/circuit_cases.py; tests/test_circuit_cpu.py holds the numpy engine to an independent reference."""
import functools

import numpy as np
import pytest

from tests import circuit_cases as cc
from tests import dem_cases as dc

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A

@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


@functools.lru_cache(maxsize=None)
def opcode_case(F, positions=None):
    """(circuit, faults, numpy columns) on the five-qubit circuit; computed once and shared."""
    from bp_osd_amd.circuit import fault_columns

    c = cc.opcode_circuit()
    fa = cc.random_faults(c, F, seed=F, positions=None if positions is None else [c.T if p == "T" else p for p in positions])
    return c, fa, fault_columns(c, fa, engine="numpy")


def assert_same(got, want):
    for g, w, name in zip(got, want, ("h_indptr", "h_indices", "l_indptr", "l_indices")):
        assert g.shape == w.shape, name
        assert np.array_equal(g, w), name


LAYERED = pytest.mark.parametrize("layered", [False, True], ids=["op_by_op", "groups"])


def native(circuit, faults, max_words=0, layered=None):
    from bp_osd_amd.circuit import FramePropagator

    prop = FramePropagator(circuit, max_words=max_words, layered=layered)
    try:
        out = prop.columns(faults, prefill=SENTINEL)
        return out, prop.timing()
    finally:
        prop.close()


@LAYERED
@pytest.mark.parametrize("F", cc.FAULT_COUNTS)
def test_columns_equal_numpy_at_word_wave_and_workgroup_edges(gpu_ready, F, layered):
    """F at the edges of a word (64), a wave (64 words) and a workgroup (256 words); the last word is ragged, and its padding
    bits give no entry: the arrays have F + 1 pointers and exactly numpy's entries."""
    c, fa, want = opcode_case(F)
    got, (_, _, _, chunks, _) = native(c, fa, layered=layered)
    assert chunks == 1
    assert_same(got, want)
    assert want[1].size and want[3].size  # (the case is not empty)


@pytest.mark.parametrize("max_words", [1, 3, 9], ids=["1", "3", "one_more_than_needed"])
@LAYERED
def test_every_split_into_chunks_gives_the_same_columns(gpu_ready, max_words, layered):
    F = 64 * 7 + 5  # 8 words, the last one ragged
    c, fa, want = opcode_case(F)
    got, (_, _, _, chunks, _) = native(c, fa, max_words, layered)
    assert chunks == -(-8 // max_words)
    assert_same(got, want)


@pytest.mark.parametrize("F,positions", [(64, ("T",)), (64, (0, "T")), (128, (4,)), (70, (9,))],
                         ids=["word_at_T", "0_and_T_mixed", "one_position", "70_at_one_position"])
@LAYERED
def test_fault_positions_at_the_edges(gpu_ready, F, positions, layered):
    c, fa, want = opcode_case(F, positions)
    got, _ = native(c, fa, layered=layered)
    assert_same(got, want)
    if positions == ("T",):
        assert got[1].size == 0 and got[3].size == 0 and not got[0].any() and not got[2].any()


@pytest.mark.parametrize("kind", cc.ANNOTATION_KINDS)
@LAYERED
def test_annotation_shapes(gpu_ready, kind, layered):
    """A measurement in nothing, one in two detectors and an observable, a detector over 40 measurements, M = 1 with k = 0, 65
    observables, and one qubit."""
    from bp_osd_amd.circuit import fault_columns

    c, F = cc.annotation_circuit(kind)
    fa = cc.random_faults(c, F, seed=11)
    want = fault_columns(c, fa, engine="numpy")
    got, _ = native(c, fa, max_words=2, layered=layered)
    assert_same(got, want)
    if kind == "k65":
        assert (got[3] >= 64).any()  # the second observable word is reached


def test_a_second_call_does_not_see_the_first_calls_frames(gpu_ready):
    from bp_osd_amd.circuit import FramePropagator

    c, fa_big, want_big = opcode_case(64 * 7 + 5)
    _, fa_small, want_small = opcode_case(129)
    prop = FramePropagator(c, max_words=3)
    try:
        assert_same(prop.columns(fa_big, prefill=SENTINEL), want_big)
        assert_same(prop.columns(fa_small, prefill=SENTINEL), want_small)
        assert_same(prop.columns(fa_big, prefill=SENTINEL), want_big)
        assert prop.device_bytes() > 0
    finally:
        prop.close()


# ------------------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def surface_models():
    from bp_osd_amd.circuit import circuit_dem

    c = cc.builder_circuit("surface13", "z", 3, cc.FULL_NOISE)
    return c, circuit_dem(c, engine="native"), circuit_dem(c, engine="numpy")


@LAYERED
def test_builder_circuit_columns_equal_numpy_in_layers_and_op_by_op(gpu_ready, layered):
    """The memory experiment with full noise is what the groups are made for: CX layers with a channel behind every gate."""
    from bp_osd_amd.circuit import fault_columns

    c, _, _ = surface_models()
    got, _ = native(c, c.faults, max_words=5, layered=layered)
    assert_same(got, fault_columns(c, engine="numpy"))


def test_native_and_numpy_models_of_the_surface_code_are_identical(gpu_ready):
    from bp_osd_amd.circuit import check_annotations

    c, nat, ref = surface_models()
    assert (nat[0] != ref[0]).nnz == 0 and (nat[1] != ref[1]).nnz == 0 and nat[0].shape == ref[0].shape
    assert np.array_equal(nat[2], ref[2]) and np.array_equal(nat[3], ref[3])
    assert np.array_equal(nat[4][0], ref[4][0]) and np.array_equal(nat[4][1], ref[4][1])
    assert np.diff(nat[0].tocsc().indptr).max() > 2  # circuit noise: columns heavier than the phenomenological two
    check_annotations(c, engine="native")


def test_the_derived_model_runs_in_the_dem_engine_on_both_engines(gpu_ready):
    from bp_osd_amd import dem_decode_sim

    _, (H, L, priors, _, _), _ = surface_models()
    runs = [dem_decode_sim(H, L, priors, batch_size=4096, engine=e, seed=dc.RUN_SEED, target_runs=4096, **dc.DECODER) for e in ("native", "numpy")]
    for name in dem_decode_sim._COUNTS:
        assert getattr(runs[0], name) == getattr(runs[1], name), name
    assert runs[0].run_count == runs[1].run_count == 4096


def test_the_derived_model_runs_in_the_window_engine(gpu_ready):
    """Window (2, 1) on the basis-z model of hgp(rep_code(3)): its Z checks are independent, so every window has full row rank
    (``window_plan`` checks that when the engine is made) and the residual is zero."""
    from bp_osd_amd import windowed_dem_decode_sim

    _, (H, L, priors, detector_time, _), _ = surface_models()
    sim = windowed_dem_decode_sim(H, L, priors, detector_time, (2, 1), batch_size=4096, engine="native", seed=dc.RUN_SEED, target_runs=4096,
                                  **dc.DECODER)
    assert sim.run_count == 4096 and sim.residual_count == 0 and len(sim.plan.windows) > 1


# -------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("what,edit,match", [
    ("pos_behind_T", lambda f, T: f.pos.__setitem__(-1, T + 1), "outside 0 .. T"),
    ("pauli_0_on_qa", lambda f, T: f.pa.__setitem__(3, 0), "Pauli code 0 on qa"),
    ("unsorted", lambda f, T: f.pos.__setitem__(5, f.pos[4] - 1), "not sorted"),
    ("qubit", lambda f, T: f.qa.__setitem__(2, 5), "qa = 5"),
    ("qubit_b", lambda f, T: (f.qb.__setitem__(2, 7), f.pb.__setitem__(2, 1)), "qb = 7"),
    ("same_qubit", lambda f, T: (f.qb.__setitem__(2, f.qa[2]), f.pb.__setitem__(2, 1)), "qa == qb"),
])
def test_fault_refusals_name_the_fault_and_launch_nothing(gpu_ready, what, edit, match):
    from bp_osd_amd.circuit import Faults, FramePropagator

    c, fa, want = opcode_case(65)
    bad = Faults(*[a.copy() for a in fa])
    bad.pos[:] = np.arange(65) // 2 + 1  # (ascending, below T, with room for the edits)
    assert bad.pos[-1] < c.T
    edit(bad, c.T)
    prop = FramePropagator(c)
    try:
        assert_same(prop.columns(fa, prefill=SENTINEL), want)
        before = prop.launches()
        assert before == 3
        with pytest.raises(ValueError, match=match):
            prop.columns(bad)
        assert prop.launches() == before
        with pytest.raises(ValueError, match="no bposd_frame_columns call has succeeded"):  # the refused call left nothing to fetch
            out = [np.zeros(66, np.int64), np.zeros(1 << 12, np.int32), np.zeros(66, np.int64), np.zeros(1 << 12, np.int32)]
            prop._libmod.check_frame(prop.lib, prop._h, prop.lib.bposd_frame_fetch(prop._h, *[a.ctypes.data for a in out]))
        assert_same(prop.columns(fa, prefill=SENTINEL), want)
    finally:
        prop.close()


def test_create_refusals_give_no_handle(gpu_ready):
    from bp_osd_amd.circuit import Circuit, FramePropagator

    c = Circuit(2)
    c.cx(0, 1)
    c.detector([c.m(0)])
    for edit, match in ((lambda ops: ops.__setitem__(0, (8, 0, 0)), "a == b == 0"), (lambda ops: ops.__setitem__(1, (2, 2, 0)), "qubit a = 2"),
                        (lambda ops: ops.pop(), "measurement index is out of range")):
        bad = Circuit(2)
        bad._ops, bad._n_meas, bad._detectors, bad._detector_time = list(c._ops), c._n_meas, c._detectors, c._detector_time
        edit(bad._ops)
        with pytest.raises(ValueError, match=match):
            FramePropagator(bad)
