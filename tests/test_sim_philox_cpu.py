"""The harness's own random stream (rng="philox": Philox4x32-10 indexed by shot and qubit) on the host: known answers,
batch-size independence of a whole simulation through the CPU oracle, and the argument checks of engine="native"."""
import numpy as np
import pytest

from bp_osd_amd.sim import css_decode_sim, philox4x32_10, philox_uniforms
from tests.sim_util import OracleAdapter

COUNTS = ("bp_converge_count_x", "bp_converge_count_z", "bp_success_count", "osd0_success_count", "osdw_success_count")


@pytest.mark.parametrize("counter,key,expect", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox4x32_10_known_answers(counter, key, expect):
    """Random123's known-answer vectors for ten rounds."""
    assert tuple(int(w) for w in philox4x32_10(counter, key)) == expect


def test_uniforms_known_values_and_indexing():
    u = philox_uniforms(5, 0, 1, 3)
    assert [float(x).hex() for x in u[0]] == ["0x1.882ed00476146p-1", "0x1.f7ac587dce789p-1", "0x1.8cc668a9efe82p-2"]
    # u(s, i) depends on (seed, s, i) alone: any window of shots and any N give the same numbers
    full = philox_uniforms(5, 0, 40, 13)
    assert (philox_uniforms(5, 17, 9, 13) == full[17:26]).all()
    assert (philox_uniforms(5, 0, 40, 8) == full[:, :8]).all()
    assert ((full >= 0) & (full < 1)).all() and len(np.unique(full)) == full.size
    assert not (philox_uniforms(6, 0, 4, 13) == full[:4]).any()
    # the high word of the shot index and of the seed reach the counter / key
    hi = philox_uniforms(5, 2 ** 32, 2, 13)
    assert not (hi == full[:2]).any()
    o = philox4x32_10((0, 1, 0, 0), (5, 0))
    assert hi[0, 0] == ((int(o[0]) >> 5) * 2 ** 26 + (int(o[1]) >> 6)) * 2.0 ** -53
    assert not (philox_uniforms(5 + 2 ** 32, 0, 2, 13) == full[:2]).any()


def test_philox_harness_is_independent_of_batch_size(surface13):
    """engine="numpy", rng="philox" through the CPU oracle: the shots are those of the stream whatever the batches are."""
    opts = dict(hx=surface13.hx, hz=surface13.hz, error_rate=0.12, xyz_error_bias=[1, 1, 1], target_runs=512, seed=7,
                channel_update="x->z", bp_method="ms", ms_scaling_factor=0.625, osd_method="osd_cs", osd_order=2,
                decoder_factory=OracleAdapter, engine="numpy", rng="philox", tqdm_disable=1)
    a = css_decode_sim(batch_size=64, **opts)
    b = css_decode_sim(batch_size=256, **opts)
    for k in COUNTS + ("min_logical_weight", "run_count", "osdw_logical_error_rate", "osdw_word_error_rate"):
        assert getattr(a, k) == getattr(b, k), (k, getattr(a, k), getattr(b, k))
    assert a.run_count == 512
    # the figures the stream's specification gives with the CPU oracle (converge x / z, bp / osd0 / osdw success, weight)
    assert [getattr(a, k) for k in COUNTS] + [a.min_logical_weight] == [469, 415, 360, 420, 426, 3]
    assert 0 < a.bp_success_count < a.osd0_success_count <= a.osdw_success_count < 512, [getattr(a, k) for k in COUNTS]
    # a different stream than numpy's legacy one, and a different one per seed
    opts["seed"] = 8
    c = css_decode_sim(batch_size=256, **opts)
    assert [getattr(c, k) for k in COUNTS] != [getattr(a, k) for k in COUNTS]


def test_philox_errors_follow_the_channel(surface13):
    """The classification of _generate_errors on the Philox numbers: Z below pz, X in [pz, pz + px), Y in [pz + px, px + py + pz)."""
    sim = css_decode_sim(hx=surface13.hx, hz=surface13.hz, error_rate=0.3, xyz_error_bias=[1, 2, 3], seed=11, run_sim=0,
                         decoder_factory=OracleAdapter, rng="philox", tqdm_disable=1)
    sim.run_count = 100  # the draw starts at the shot the run has reached
    ex, ez = sim._generate_errors(2000)
    u = philox_uniforms(11, 100, 2000, 13)
    px, py, pz = 0.3 * np.array([1, 2, 3.0]) / 6
    z, x, y = u < pz, (pz <= u) & (u < pz + px), (pz + px <= u) & (u < px + py + pz)
    assert (ez == (z | y)).all() and (ex == (x | y)).all()
    assert abs(ez.mean() - (pz + py)) < 0.01 and abs(ex.mean() - (px + py)) < 0.01


def test_native_engine_arguments_are_validated(surface13):
    base = dict(hx=surface13.hx, hz=surface13.hz, error_rate=0.05, target_runs=4, seed=3, run_sim=0, tqdm_disable=1)
    with pytest.raises(ValueError, match="decoder_factory must be None"):
        css_decode_sim(engine="native", decoder_factory=OracleAdapter, **base)
    with pytest.raises(ValueError, match="rng must be 'philox'"):
        css_decode_sim(engine="native", rng="numpy", **base)
    with pytest.raises(ValueError, match="rng must be 'philox'"):
        css_decode_sim(engine="native", rng="torch", **base)
    with pytest.raises(ValueError):
        css_decode_sim(engine="torch", rng="philox", **base)
    with pytest.raises(ValueError):
        css_decode_sim(engine="numpy", rng="mt19937", decoder_factory=OracleAdapter, **base)
    sim = css_decode_sim(engine="numpy", rng="philox", decoder_factory=OracleAdapter, **base)
    assert "_rng" not in sim.output_dict() and "_mc" not in sim.output_dict()
    with pytest.raises(RuntimeError):
        sim.last_batch("flags")
