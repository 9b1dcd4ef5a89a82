"""The Monte-Carlo engine of the library (bposd_mc_*, css_decode_sim(engine="native")) on the MI355X: the sampler against the
host restatement of the Philox stream bit for bit, the scorer against sim._logical_fail, whole simulations against the CPU
oracle driven by the same stream, the HBM-resident decoders underneath it, and the absence of torch."""
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ("bp_converge_count_x", "bp_converge_count_z", "bp_success_count", "osd0_success_count", "osdw_success_count")
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


def _native(code, batch_size, run_sim=0, **opts):
    from bp_osd_amd.sim import css_decode_sim

    kw = dict(error_rate=0.05, xyz_error_bias=[1, 1, 1], seed=5, bp_method="ms", ms_scaling_factor=0.625, max_iter=4,
              osd_method="osd_cs", osd_order=2, channel_update=None, tqdm_disable=1, target_runs=batch_size)
    kw.update(opts)
    return css_decode_sim(hx=code.hx, hz=code.hz, batch_size=batch_size, engine="native", run_sim=run_sim, **kw)


def _unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")[:, :n]


def _host_errors(sim, first_shot, B):
    """The host draw of the same shots: _generate_errors on the Philox numbers (it starts at sim.run_count)."""
    keep, sim.run_count = sim.run_count, first_shot
    try:
        return sim._generate_errors(B)
    finally:
        sim.run_count = keep


def _packed(rows):
    by = np.packbits(rows, axis=1, bitorder="little")
    out = np.zeros((rows.shape[0], 8 * ((rows.shape[1] + 63) // 64)), np.uint8)
    out[:, :by.shape[1]] = by
    return out.view("<u8")


SAMPLER_CASES = [
    dict(id="hgp400-depolarising", code="hgp400", B=200, opts=dict(error_rate=0.09)),
    dict(id="hgp400-z-only", code="hgp400", B=131, opts=dict(error_rate=0.06, xyz_error_bias=[0, 0, 1])),
    dict(id="hgp400-hadamard", code="hgp400", B=77, opts=dict(error_rate=0.08, xyz_error_bias=[1, 2, 5], hadamard_rotate=1,
                                                              hadamard_rotate_sector1_length=137)),
    dict(id="h1922-depolarising", code="h1922", B=193, opts=dict(error_rate=0.05)),
    dict(id="h1922-z-only-high-shot", code="h1922", B=70, first_shot=2 ** 32 + 12345, opts=dict(error_rate=0.04, xyz_error_bias=[0, 0, 1])),
    dict(id="h1922-hadamard", code="h1922", B=129, opts=dict(error_rate=0.06, xyz_error_bias=[3, 1, 2], hadamard_rotate=1,
                                                            hadamard_rotate_sector1_length=961)),
]


@pytest.mark.parametrize("case", SAMPLER_CASES, ids=[c["id"] for c in SAMPLER_CASES])
def test_sampler_equals_host_stream(gpu_ready, request, case):
    """mc_sample_kernel: packed error rows = np.packbits of the host draw, syndromes = the sparse products of them."""
    from bp_osd_amd.sim import _mod2_mul

    code = request.getfixturevalue(case["code"])
    B, first = case["B"], case.get("first_shot", 0)
    sim = _native(code, 256, **case["opts"])
    sim.run_count = first
    sim._run_batch(B)
    assert sim.run_count == first + B
    ex, ez = _host_errors(sim, first, B)
    assert ex.any() or case["opts"].get("xyz_error_bias") == [0, 0, 1]
    assert ez.any()
    got_x, got_z = sim.last_batch("error_x"), sim.last_batch("error_z")
    assert got_x.shape == (B, (code.N + 63) // 64) and got_x.dtype == np.dtype("<u8")
    assert (got_x == _packed(ex)).all(), "error_x differs from the host stream"
    assert (got_z == _packed(ez)).all(), "error_z differs from the host stream"
    sx, sz = _mod2_mul(sim.hz, ex), _mod2_mul(sim.hx, ez)
    assert (sim.last_batch("syndrome_x") == sx).all() and (sim.last_batch("syndrome_z") == sz).all()
    assert (sim.last_batch("syndrome_x_packed") == _packed(sx)).all() and (sim.last_batch("syndrome_z_packed") == _packed(sz)).all()
    if first:  # the high counter word matters: the same rows of shot 12345 .. differ
        assert not (_packed(_host_errors(sim, first - 2 ** 32, B)[1]) == got_z).all()


def _numpy_score(sim, ex, ez, rx, rz):
    """Flag bytes and the seven counters of a batch from sim._logical_fail (css_decode_sim.py:250-365 restated)."""
    B = len(ex)
    flags = np.zeros(B, np.uint8)
    counters = [int(rx["conv"].sum()), int(rz["conv"].sum())]
    success, wmin = {}, {}
    for o, key in enumerate(("bp", "osd0", "osdw")):
        fx, fz, weight = sim._logical_fail(ex, ez, rx[key], rz[key]) if sim.K else (np.zeros(B, bool), np.zeros(B, bool), np.zeros(B, int))
        flags |= (fx.astype(np.uint8) << (2 * o)) | (fz.astype(np.uint8) << (2 * o + 1))
        failed = fx | fz
        success[key] = int((~failed).sum()) if key != "bp" else int((rx["conv"] & rz["conv"] & ~failed).sum())
        wmin[key] = int(weight[failed].min()) if failed.any() else INT_MAX
    return flags, counters + [success["bp"], success["osd0"], success["osdw"], wmin["osd0"], wmin["osdw"]]


def _decode_like_the_engine(sim, synd_x, synd_z):
    """The two decodes of a batch through the host-pointer API of the same decoder objects (channel already set up by the engine)."""
    if sim.channel_update is None:
        rz, rx = sim._decode(sim.bpd_z, synd_z), sim._decode(sim.bpd_x, synd_x)
    elif sim.channel_update == "x->z":
        rx = sim._decode(sim.bpd_x, synd_x)
        p1, _ = sim._updated_channel(sim.channel_probs_x, sim.channel_probs_z)
        rz = sim._decode(sim.bpd_z, synd_z, select=rx["osdw"], alt=p1)
    else:
        rz = sim._decode(sim.bpd_z, synd_z)
        p1, _ = sim._updated_channel(sim.channel_probs_z, sim.channel_probs_x)
        rx = sim._decode(sim.bpd_x, synd_x, select=rz["osdw"], alt=p1)
    return {k: np.array(v) for k, v in rx.items()}, {k: np.array(v) for k, v in rz.items()}


def _check_batch_against_numpy(sim, B, first=0):
    """Run one native batch; flags and counters must be the numpy checks of the fetched errors and of decode_batch's outputs."""
    before = {k: getattr(sim, k) for k in COUNTS}
    sim.run_count = first
    sim._run_batch(B)
    N = sim.N
    ex, ez = _unpack(sim.last_batch("error_x"), N), _unpack(sim.last_batch("error_z"), N)
    hx_, hz_ = _host_errors(sim, first, B)
    assert (ex == hx_).all() and (ez == hz_).all()
    flags = sim.last_batch("flags")
    rx, rz = _decode_like_the_engine(sim, sim.last_batch("syndrome_x"), sim.last_batch("syndrome_z"))
    want_flags, want = _numpy_score(sim, ex, ez, rx, rz)
    assert (flags == want_flags).all(), np.flatnonzero(flags != want_flags)[:10]
    got = [getattr(sim, k) - before[k] for k in COUNTS]
    assert got == want[:5], (got, want)
    return want, flags, rx, rz


@pytest.mark.parametrize("channel_update", [None, "x->z", "z->x"])
@pytest.mark.parametrize("name,B,rate", [("hgp400", 333, 0.09), ("h1922", 200, 0.08)])
def test_scorer_equals_numpy_logical_checks(gpu_ready, request, name, B, rate, channel_update):
    """mc_score_kernel against sim._logical_fail, shot by shot (flag bytes) and in the seven counters."""
    code = request.getfixturevalue(name)
    sim = _native(code, 512, error_rate=rate, channel_update=channel_update, max_iter=6, osd_order=4)
    sim.min_logical_weight = 10 ** 9
    want, flags, rx, rz = _check_batch_against_numpy(sim, B)
    # the batch is not a trivial one: BP fails to converge somewhere, some output fails a logical check, some succeeds
    assert 0 < want[0] < B and 0 < want[1] < B, want
    assert flags.any() and not flags.all(), "no logical failure (or nothing but failures) in the batch"
    assert min(want[5], want[6]) < INT_MAX, "no osd0 / osdw failure in the batch: the smallest weight is not exercised"
    assert sim.min_logical_weight == min(want[5], want[6]) > 0
    # a second batch accumulates, and continues the stream at the next shot
    sim.min_logical_weight = 10 ** 9
    _check_batch_against_numpy(sim, 100, first=B)


@pytest.mark.parametrize("channel_update", [None, "x->z", "z->x"])
def test_native_engine_equals_oracle_harness(gpu_ready, hgp400, channel_update):
    """The whole engine against engine="numpy", rng="philox" on the CPU oracle, with different batch sizes on the two sides."""
    from bp_osd_amd.sim import css_decode_sim
    from tests.sim_util import OracleAdapter

    opts = dict(hx=hgp400.hx, hz=hgp400.hz, error_rate=0.09, xyz_error_bias=[1, 1, 1], target_runs=768, seed=5, bp_method="ms",
                ms_scaling_factor=0, max_iter=0, osd_method="osd_cs", osd_order=6, channel_update=channel_update, tqdm_disable=1)
    ref = css_decode_sim(batch_size=96, engine="numpy", rng="philox", decoder_factory=OracleAdapter, **opts)
    got = css_decode_sim(batch_size=256, engine="native", **opts)
    print("oracle side:", [getattr(ref, k) for k in COUNTS], ref.min_logical_weight, "native:", [getattr(got, k) for k in COUNTS],
          got.min_logical_weight)
    assert ref.run_count == 768
    for k in COUNTS:  # so that equality is not trivial
        assert 0.1 * ref.run_count < getattr(ref, k) < 0.9 * ref.run_count, (k, getattr(ref, k))
    for k in ("run_count",) + COUNTS + ("min_logical_weight", "osdw_logical_error_rate", "osdw_word_error_rate"):
        assert getattr(got, k) == getattr(ref, k), (k, getattr(got, k), getattr(ref, k))
    assert sorted(json.loads(got.output_dict())) == sorted(json.loads(ref.output_dict()))


@pytest.mark.parametrize("size,shifts,K,bp_kernel,rate,max_iter", [(45, (0, 2, 5), 0, "bp_local_kernel", 0.06, 8),
                                                                  (48, (0, 1, 2), 8, "bp_large_kernel", 0.03, 16)],
                         ids=["circulant45-0-2-5", "circulant48-0-1-2"])
def test_native_engine_on_the_hbm_resident_kernels(gpu_ready, size, shifts, K, bp_kernel, rate, max_iter):
    """Products beyond the LDS / register-resident kernels under the engine, against its own fetched arrays pushed through
    decode_batch and the numpy checks.  hgp(circulant(45, (0, 2, 5))), 2025 x 4050, is the parity suite's large code: OSD
    runs in osd_large_kernel (m > 1024), BP still in LDS (m <= 2048).  Its seed has full rank, so K = 0: the engine runs
    with no logical to fail, below css_decode_sim's rate formulas (they divide by K).  hgp(circulant(48, (0, 1, 2))),
    2304 x 4608, has the same degrees, K = 8, runs bp_large_kernel too and goes through the whole harness (its seed's short
    cycles want a lower error rate for BP to converge anywhere; at distance 32 only BP's own output fails a logical check)."""
    from bp_osd_amd.codes import circulant, hgp

    code = hgp(circulant(size, shifts), compute_logicals=False)
    B = 160
    sim = _native(code, 256, error_rate=rate, channel_update="x->z", max_iter=max_iter, osd_method="osd_e", osd_order=5, check_code=0)
    assert sim.N == 2 * size * size and sim.K == K
    if sim.K == 0:
        sim._update_rates = lambda: None  # 1 / K
    want, flags, rx, rz = _check_batch_against_numpy(sim, B)
    print("large path:", size, shifts, want)
    assert sim.bpd_x.bp_kernel_info()["kernel"] == bp_kernel and sim.bpd_x.last_osd_kernel() == "osd_large_kernel"
    assert 0 < want[0] < B and 0 < want[1] < B, want
    if sim.K == 0:
        assert not flags.any() and want[3] == want[4] == B and want[5] == want[6] == INT_MAX
    else:
        assert flags.any() and not flags.all()


def test_native_engine_imports_no_torch(gpu_ready):
    """A device-resident simulation in a fresh process (this session's conftest imports torch) never loads torch."""
    child = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from bp_osd_amd.codes import surface13\n"
        "from bp_osd_amd.sim import css_decode_sim\n"
        "c = surface13()\n"
        "sim = css_decode_sim(hx=c.hx, hz=c.hz, error_rate=0.1, target_runs=300, batch_size=128, seed=3, engine='native', tqdm_disable=1,\n"
        "                     bp_method='ms', osd_method='osd_cs', osd_order=2)\n"
        "assert sim.run_count == 300 and 0 < sim.osdw_success_count < 300, sim.output_dict()\n"
        "assert sim.last_batch('flags').shape == (300 - 256,)\n"
        "assert 'torch' not in sys.modules, 'torch was imported'\n"
        "print('native ok', sim.osdw_success_count)\n")
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "native ok" in r.stdout, r.stdout + r.stderr


def test_engine_arguments_are_checked_by_the_library(gpu_ready, surface13, hgp400):
    """B beyond the capacity, a fetch of the wrong size, decoders that do not fit the matrices: BPOSD_ERR_INVALID with a message."""
    import ctypes as C

    from bp_osd_amd import BpOsdDecoder, _lib

    sim = _native(surface13, 64, error_rate=0.1)
    with pytest.raises(RuntimeError):
        sim.last_batch("flags")
    with pytest.raises(ValueError, match="capacity"):
        sim._run_batch(65)
    assert sim.run_count == 0
    sim._run_batch(64)
    out = np.empty(63, np.uint8)
    rc = gpu_ready.bposd_mc_fetch(sim._mc, _lib.MC_ITEMS["flags"], out.ctypes.data, out.nbytes)
    assert rc == _lib.BPOSD_ERR_INVALID and b"bytes" in gpu_ready.bposd_mc_last_error(sim._mc)
    assert gpu_ready.bposd_mc_fetch(sim._mc, 99, out.ctypes.data, out.nbytes) == _lib.BPOSD_ERR_INVALID
    with pytest.raises(ValueError):
        sim.last_batch("nothing")
    assert sim.mc_device_bytes() > 6 * 64 * 13
    # a decoder of another code: shapes do not match
    other = BpOsdDecoder(hgp400.hz, error_rate=0.1)
    sim2 = _native(surface13, 64, error_rate=0.1)
    sim2.bpd_x = other
    with pytest.raises(ValueError, match="do not match"):
        sim2._run_batch(8)
    mc = C.c_void_p()
    assert gpu_ready.bposd_mc_create(None, None, None, None, None, 0, None, None, 0, 0, None, None, 0, None, None, None, None, C.byref(mc)) \
        == _lib.BPOSD_ERR_INVALID
    assert not mc.value and gpu_ready.bposd_mc_last_error(None)
    # the rows of hx need not be sorted (css_decode_sim sorts them, so bposd_mc_create is called directly): an engine whose hx
    # has the column indices of one row reversed is accepted and gives the batch of the sorted one
    import scipy.sparse as sp

    def one_batch(reversed_row):
        s = _native(surface13, 64, error_rate=0.1)
        hx, hz = sp.csr_matrix(s.hx), sp.csr_matrix(s.hz)
        hx.sort_indices()
        hz.sort_indices()
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        hx_indices = i32(hx.indices).copy()
        if reversed_row is not None:
            lo, hi = hx.indptr[reversed_row], hx.indptr[reversed_row + 1]
            assert hi - lo >= 2
            hx_indices[lo:hi] = hx_indices[lo:hi][::-1].copy()
            assert (np.diff(hx_indices[lo:hi]) < 0).all()
        keep = [i32(hx.indptr), hx_indices, i32(hz.indptr), i32(hz.indices), BpOsdDecoder.pack_rows(np.asarray(s.lx, dtype=np.uint8) & 1),
                BpOsdDecoder.pack_rows(np.asarray(s.lz, dtype=np.uint8) & 1), f64(s.channel_probs_x), f64(s.channel_probs_y), f64(s.channel_probs_z)]
        ptr = [a.ctypes.data for a in keep]
        cfg = _lib.BposdMcConfig(device=int(s.bpd_x.device), channel_update=_lib.MC_UPDATE[None], seed=5, capacity=64)
        eng = C.c_void_p()
        rc = gpu_ready.bposd_mc_create(C.byref(cfg), s.bpd_x._h, s.bpd_z._h, ptr[0], ptr[1], hx.shape[0], ptr[2], ptr[3], hz.shape[0], s.N, ptr[4],
                                       ptr[5], int(np.asarray(s.lx).shape[0]), ptr[6], ptr[7], ptr[8], None, C.byref(eng))
        assert rc == 0 and eng.value, gpu_ready.bposd_mc_last_error(None)
        try:
            c = (C.c_int64 * 7)()
            assert gpu_ready.bposd_mc_run(eng, 0, 64, c) == 0, gpu_ready.bposd_mc_last_error(eng)
            flags = np.empty(64, np.uint8)
            assert gpu_ready.bposd_mc_fetch(eng, _lib.MC_ITEMS["flags"], flags.ctypes.data, flags.nbytes) == 0
        finally:
            gpu_ready.bposd_mc_destroy(eng)
        return [int(v) for v in c], flags

    (want_counters, want_flags), (got_counters, got_flags) = one_batch(None), one_batch(0)
    assert got_counters == want_counters and (got_flags == want_flags).all()
    assert (want_flags == sim.last_batch("flags")).all()  # (and the sorted one is css_decode_sim's own engine: seed 5, shots 0 .. 63)
    assert want_counters[:5] == [getattr(sim, k) for k in COUNTS]


def test_engine_create_destroy_cycles_release_device_memory(gpu_ready, hgp400):
    """Twelve create -> run -> destroy cycles of the engine (and its decoders) leave the device's free memory where it was."""
    import torch

    def cycle():
        sim = _native(hgp400, 4096, run_sim=1, error_rate=0.08, channel_update="x->z", target_runs=4096)
        out = [getattr(sim, k) for k in COUNTS]
        del sim
        gc.collect()
        return out

    first = cycle()
    cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(12):
        assert cycle() == first
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 64 * 2 ** 20, f"device memory not returned: {(free0 - free1) / 2 ** 20:.0f} MB after 12 cycles"
