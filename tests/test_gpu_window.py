"""The sliding-window engine of the library (bposd_window_*, windowed_dem_decode_sim(engine="native"), WindowedDemDecoder) on
the MI355X: window_step_kernel alone against a numpy restatement, whole runs against the per-shot definition on the CPU
oracle bit for bit, a single window against the unwindowed engine, the decode-only interface and the engine's lifecycle.
Tables and references: tests/window_cases.py."""
import ctypes as C

import numpy as np
import pytest

from tests import dem_cases as dc
from tests import window_cases as wc

pytestmark = pytest.mark.gpu

STEP_B = 4101  # above 8 workgroups per CU (2048 on an MI355X) and no multiple of it: a workgroup meets a second and a third shot


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


# (model, window, step, decoded rows packed, syndrome rows packed)
STEP_CASES = [
    ("random-520-129-65", (2, 1), 0, False, False),   # gather only, byte syndrome
    ("random-520-129-65", (2, 1), 0, False, True),    # gather only, packed syndrome
    ("random-520-129-65", (2, 1), 2, False, False),   # commit and gather, bytes both ways; two observable words
    ("random-520-129-65", (2, 1), 2, True, True),     # ... packed both ways
    ("random-520-129-65", (2, 1), 4, True, False),    # commit only (the last step)
    ("random-1031-130-3", (3, 2), 1, False, True),    # bytes in, packed out
    ("random-1031-130-3", (3, 2), 1, True, False),    # packed in, bytes out
    ("random-1031-130-3", (3, 2), 2, False, False),   # commit only, byte rows
    ("hgp400-R3", (2, 1), 2, True, True),             # a staged range that does not start at word 0
]


@pytest.mark.parametrize("name,window,s,dec_packed,syn_packed", STEP_CASES,
                         ids=[f"{c[0]}-w{c[1][0]}{c[1][1]}-s{c[2]}-{'p' if c[3] else 'b'}{'p' if c[4] else 'b'}" for c in STEP_CASES])
def test_step_kernel_equals_numpy(gpu_ready, name, window, s, dec_packed, syn_packed):
    """window_step_kernel alone on rows no decoder wrote: running row, observable row, correction row, next syndrome with its
    padding bits, conv_all and iters are the numpy restatement's."""
    from bp_osd_amd import _lib, window_plan

    H, L, priors, times = wc.model(name)
    plan = window_plan(H, times, window, priors=priors)
    M, N = H.shape
    k = L.shape[0]
    B = STEP_B
    rng = np.random.default_rng(1000 * s + M)
    running = (rng.random((B, M)) < 0.3).astype(np.uint8)
    obs = (rng.random((B, k)) < 0.5).astype(np.uint8)
    corr = (rng.random((B, N)) < 0.05).astype(np.uint8)
    conv_all = (rng.random(B) < 0.7).astype(np.uint8)
    iters = rng.integers(0, 50, B).astype(np.int32)
    prev_conv = (rng.random(B) < 0.5).astype(np.uint8)
    prev_iters = rng.integers(0, 9, B).astype(np.int32)
    prev = plan.windows[s - 1] if s > 0 else None
    nxt = plan.windows[s] if s < len(plan.windows) else None
    decoded = (rng.random((B, prev.fault.size)) < 0.1).astype(np.uint8) if prev is not None else None
    want = wc.numpy_step(plan, H, L, s, running, obs, corr, decoded, prev_conv, prev_iters, conv_all, iters)

    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    keep = [i32(H.indptr), i32(H.indices), i32(L.indptr), i32(L.indices)]
    a = _lib.BposdWindowStep(device=0, M=M, N=N, k=k, B=B)
    a.h_indptr, a.h_indices, a.l_indptr, a.l_indices = (v.ctypes.data for v in keep)
    g_running, g_obs, g_corr = dc.pack(running).copy(), dc.pack(obs).copy(), dc.pack(corr).copy()
    g_conv, g_iters = conv_all.copy(), iters.copy()
    a.running, a.observables, a.correction = g_running.ctypes.data, g_obs.ctypes.data, g_corr.ctypes.data
    a.conv_all, a.iters = g_conv.ctypes.data, g_iters.ctypes.data
    if prev is not None:
        sel = np.flatnonzero(prev.commit)
        pos, fault = i32(sel), i32(prev.fault[sel])
        rows = dc.pack(decoded).copy() if dec_packed else np.ascontiguousarray(decoded)
        a.n_commit, a.commit_pos, a.commit_fault = sel.size, pos.ctypes.data, fault.ctypes.data
        a.decoded_cols, a.decoded_packed, a.decoded = prev.fault.size, int(dec_packed), rows.ctypes.data
        a.prev_converged, a.prev_iters = prev_conv.ctypes.data, prev_iters.ctypes.data
    if nxt is not None:
        det = i32(nxt.det)
        synd = np.full((B, (det.size + 63) // 64), 0xA5A5A5A5A5A5A5A5, "<u8") if syn_packed else np.full((B, det.size), 0xA5, np.uint8)
        a.n_gather, a.gather_det, a.syndrome_packed, a.syndrome = det.size, det.ctypes.data, int(syn_packed), synd.ctypes.data
    rc = gpu_ready.bposd_debug_window_step(C.byref(a))
    assert rc == 0, gpu_ready.bposd_window_last_error(None)
    assert tuple(a.word_range) == plan.step_words[s]
    if name == "hgp400-R3":
        assert a.word_range[0] > 0

    w_running, w_obs, w_corr, w_synd, w_conv, w_iters = want
    for label, got, ref in (("running", g_running, dc.pack(w_running)), ("observables", g_obs, dc.pack(w_obs)), ("correction", g_corr, dc.pack(w_corr))):
        bad = np.flatnonzero((got != ref).any(axis=1))
        assert bad.size == 0, f"{label} rows differ in {bad.size} shots, first {bad[:5]}"
    assert (g_conv == w_conv).all() and (g_iters == w_iters).all()
    if prev is None:  # a gather-only step folds nothing and changes no row
        assert (g_conv == conv_all).all() and (g_iters == iters).all() and (g_running == dc.pack(running)).all()
    else:
        assert (g_running != dc.pack(running)).any() and (g_corr != dc.pack(corr)).any()  # the commit did something
    if nxt is not None:
        ref = dc.pack(w_synd) if syn_packed else w_synd
        bad = np.flatnonzero((synd != ref).any(axis=1))
        assert bad.size == 0, f"syndrome rows differ in {bad.size} shots, first {bad[:5]}"


def _native(name, window, B, batch_size=None, **kw):
    from bp_osd_amd import windowed_dem_decode_sim

    H, L, priors, times = wc.model(name)
    return windowed_dem_decode_sim(H, L, priors, times, window, batch_size=batch_size or B, engine="native", seed=wc.RUN_SEED, target_runs=B,
                                   **dict(wc.DECODER, **kw))


@pytest.mark.parametrize("case", wc.RUN_CASES, ids=[c["id"] for c in wc.RUN_CASES])
def test_whole_runs_equal_the_oracle(gpu_ready, case):
    """Sample, windows and scoring on the device against the host loop around the CPU oracle: every item of the batch bit
    for bit, the four counters, and a residual of zero."""
    ref = wc.run_reference(case["id"])
    sim = _native(case["model"], case["window"], case["B"])
    for key in wc.COUNTS:
        assert getattr(sim, key) == ref[key], key
    assert sim.bp_converge_count == case["oracle"]["converged"]
    assert case["B"] - sim.osdw_success_count == case["oracle"]["wrong"]
    assert sim.trivial_count == case["oracle"]["quiet"]
    for item in wc.ITEMS:
        got = sim.last_batch(item)
        assert got.shape == ref[item].shape and got.dtype == ref[item].dtype, item
        assert (got == ref[item]).all(), f"{item} differs in shots {np.flatnonzero((got != ref[item]).reshape(len(got), -1).any(axis=1))[:5]}"
    assert sim.residual_count == 0 and not sim.last_batch("residual").any()
    assert (sim.osdw_observable_error_rates == ref["osdw_observable_error_rates"]).all()
    step_ms, score_ms = sim.kernel_ms()
    assert step_ms > 0 and score_ms > 0


@pytest.mark.parametrize("name", sorted(wc.SINGLE_WINDOW))
def test_a_single_window_is_the_unwindowed_engine(gpu_ready, name):
    from bp_osd_amd import dem_decode_sim

    H, L, priors, times = wc.model(name)
    T = int(times.max()) + 1
    B = dc.RUN_BY_ID[wc.SINGLE_WINDOW[name]]["B"]
    sim = _native(name, (T, T), B)
    whole = dem_decode_sim(H, L, priors, batch_size=B, engine="native", seed=wc.RUN_SEED, target_runs=B, **wc.DECODER)
    assert len(sim.plan.windows) == 1
    assert (sim.last_batch("obs_osdw") == whole.last_batch("obs_osdw")).all()
    assert (sim.last_batch("detectors") == whole.last_batch("detectors")).all()
    assert sim.osdw_success_count == whole.osdw_success_count == B - dc.RUN_BY_ID[wc.SINGLE_WINDOW[name]]["oracle"]["wrong"][2]
    assert sim.trivial_count == whole.trivial_count
    assert sim.bp_converge_count == whole.bp_converge_count


@pytest.mark.parametrize("case_id", ["surface13-R5-w21", "random-520-w21"])
def test_decode_only_returns_the_runs_rows(gpu_ready, case_id):
    """WindowedDemDecoder on the detectors fetched from a run: host form (bytes and packed words, in chunks) and device-pointer
    form give that run's rows.  The decoder shares the run's BpOsdDecoder objects: two engines over the same handles."""
    import torch
    from bp_osd_amd import WindowedDemDecoder

    case = wc.RUN_BY_ID[case_id]
    H, L, priors, times = wc.model(case["model"])
    B = case["B"]
    sim = _native(case["model"], case["window"], B)
    det = sim.last_batch("detectors")
    want = {item: sim.last_batch(item) for item in ("obs_osdw", "correction", "residual", "converged", "iters")}
    dec = WindowedDemDecoder(H, L, priors, times, case["window"], batch_size=96, decoders=sim.decoders)  # 96 < B: three chunks
    got = dec.decode_batch(det)
    assert got.dtype == np.dtype("<u8") and (got == want["obs_osdw"]).all()
    assert (dec.batch_correction == want["correction"]).all() and (dec.batch_residual == want["residual"]).all()
    assert (dec.batch_converge == want["converged"].astype(bool)).all() and (dec.batch_iter == want["iters"]).all()
    got = dec.decode_batch(dc.unpack(det, H.shape[0]))
    assert got.dtype == np.uint8 and (dc.pack(got) == want["obs_osdw"]).all()
    assert (dc.pack(dec.batch_correction) == want["correction"]).all() and not dec.batch_residual.any()

    n = 90  # device-pointer form: one call of at most batch_size rows
    words = lambda c: (c + 63) // 64
    d_det = torch.from_numpy(det[:n].view(np.int64).copy()).cuda()
    outs = {key: torch.full((n, words(c)), -1, dtype=torch.int64, device="cuda") for key, c in (("obs", L.shape[0]), ("corr", H.shape[1]), ("res", H.shape[0]))}
    d_conv = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    d_iters = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.decode_batch_device(d_det.data_ptr(), n, outs["obs"].data_ptr(), outs["corr"].data_ptr(), outs["res"].data_ptr(), d_conv.data_ptr(),
                            d_iters.data_ptr(), wait=True)
    assert (outs["obs"].cpu().numpy().view(np.uint64) == want["obs_osdw"][:n]).all()
    assert (outs["corr"].cpu().numpy().view(np.uint64) == want["correction"][:n]).all()
    assert not outs["res"].cpu().numpy().any()
    assert (d_conv.cpu().numpy() == want["converged"][:n]).all() and (d_iters.cpu().numpy() == want["iters"][:n]).all()
    assert (d_det.cpu().numpy().view(np.uint64) == det[:n]).all()  # the input rows are not written
    obs_only = torch.full((n, words(L.shape[0])), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    dec.decode_batch_device(d_det.data_ptr(), n, obs_only.data_ptr())  # every optional output left out
    dec.synchronize()
    assert (obs_only.cpu().numpy().view(np.uint64) == want["obs_osdw"][:n]).all()
    with pytest.raises(ValueError, match="outside"):
        dec.decode_batch_device(d_det.data_ptr(), 97, obs_only.data_ptr())
    # the run's own engine still works after the other engine used its decoders, and the engines go before the decoders
    keep = sim.decoders
    dec.close()
    again = _native(case["model"], case["window"], B)
    assert (again.last_batch("obs_osdw") == want["obs_osdw"]).all()
    del sim, again
    assert keep[0].decode_batch(np.zeros((1, keep[0].m), np.uint8)).shape == (1, keep[0].n)


def test_batches_of_100_and_device_bytes(gpu_ready):
    case = wc.RUN_BY_ID["surface13-R3-w21"]
    ref = wc.run_reference(case["id"])
    sim = _native(case["model"], case["window"], case["B"], batch_size=100)
    for key in wc.COUNTS:
        assert getattr(sim, key) == ref[key], key
    assert (sim.last_batch("obs_osdw") == ref["obs_osdw"][200:]).all() and sim.last_batch("flags").shape == (56,)
    assert (sim.osdw_observable_error_rates == ref["osdw_observable_error_rates"]).all()
    # device memory: the rows include/bposd_mi355x.h documents at bposd_window_create
    H, L, priors, times = wc.model(case["model"])
    plan, cap = sim.plan, 100
    M, N = H.shape
    k = L.shape[0]
    dw, ow, fw = (M + 63) // 64, (k + 63) // 64, (N + 63) // 64
    packed = [d.bp_kernel_info()["kernel"] not in ("bp_anydeg_kernel", "bp_serial_kernel") for d in sim.decoders]
    row = lambda cols, p: 8 * ((cols + 63) // 64) if p else cols
    nc = sum(int(w.commit.sum()) for w in plan.windows)
    ncw = sum(len(set((w.fault[w.commit != 0] >> 6).tolist())) for w in plan.windows)
    synd = max(row(w.det.size, packed[w.handle]) for w in plan.windows)
    decd = max(row(w.fault.size, packed[w.handle]) for w in plan.windows)
    blocks = [4 * (N + 1), 4 * (H.nnz + L.nnz), 4 * nc, 4 * nc, 4 * nc, 4 * ncw, 4 * sum(w.det.size for w in plan.windows),
              8 * cap * dw, 8 * cap * ow, 8 * cap * ow, 8 * cap * fw, cap * synd, cap * decd, cap, 4 * cap, cap, 4 * cap, cap, 32, 4 * k]
    assert sim.device_bytes() == sum(max(b, 256) for b in blocks)


def test_create_refuses_what_the_header_says(gpu_ready):
    """A decoder of another window's shape is refused with the window named; so is a decoder list of the wrong length."""
    from bp_osd_amd import WindowedDemDecoder

    H, L, priors, times = wc.model("surface13-R3")
    dec = WindowedDemDecoder(H, L, priors, times, (2, 1), batch_size=8, **wc.DECODER)
    assert len(dec.decoders) == 2
    with pytest.raises(ValueError, match=r"window 2: decoder shape"):
        WindowedDemDecoder(H, L, priors, times, (2, 1), batch_size=8, decoders=[dec.decoders[0], dec.decoders[0]])
    with pytest.raises(ValueError, match="distinct windows"):
        WindowedDemDecoder(H, L, priors, times, (2, 1), batch_size=8, decoders=dec.decoders[:1])
