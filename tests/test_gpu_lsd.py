"""The LSD mode on the device (``BpOsdDecoder(..., lsd=cfg)``, ``lsd_kernel``) bit for bit against ``LsdReferenceDecoder``
(bp_osd_amd/lsd.py: the CPU oracle's BP and OSD around the numpy definition): every case of tests/lsd_cases.py under every
run (generous and small caps, OSD off and osd_cs 7, both tie policies), caps on and next to cluster sizes that occur at
the kernel's ceilings, the packed and device-pointer forms, a per-shot channel, observables, a host call of two chunks, the
DEM engine, the mode switched off again, and the handle's refusals.  tests/test_lsd_cpu.py checks the reference itself and
that the cases are not trivial."""
import numpy as np
import pytest

from tests import lsd_cases as lc

pytestmark = pytest.mark.gpu

ROWS = ("osdw", "osd0", "bp")
STATS = ("status", "rounds", "clusters", "max_bits")
ALL = ROWS + ("converged", "iters") + STATS


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


def _decode(dec, S, **kw):
    osdw = dec.decode_batch(S, want_osd0=True, want_bp=True, want_llr=True, **kw)
    out = dict(osdw=osdw, osd0=dec.batch_osd0, bp=dec.batch_bp, converged=dec.batch_converge, iters=dec.batch_iter, llr=dec.batch_llr)
    if dec.lsd is not None:
        out.update(dec.lsd_stats())
    return out


def _decode_packed(dec, S):
    n = dec.n
    osdw = dec.decode_batch(dec.pack_rows(S), want_osd0=True, want_bp=True, packed=True)
    out = dict(osdw=dec.unpack_rows(osdw, n), osd0=dec.unpack_rows(dec.batch_osd0, n), bp=dec.unpack_rows(dec.batch_bp, n),
               converged=dec.batch_converge, iters=dec.batch_iter)
    out.update(dec.lsd_stats())
    return out


def _decode_device(dec, S):
    """One ``decode_batch_device`` call: the whole batch runs as one launch on one lane."""
    import torch

    B, n = len(S), dec.n
    d_syn = torch.from_numpy(np.array(S)).cuda()
    d = [torch.zeros((B, n), dtype=torch.uint8, device="cuda") for _ in range(3)]
    d_conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
    d_it = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.decode_batch_device(d_syn.data_ptr(), B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_conv.data_ptr(), d_it.data_ptr())
    lane = dec.last_lane
    dec.synchronize()
    out = dict(osdw=d[0].cpu().numpy(), osd0=d[1].cpu().numpy(), bp=d[2].cpu().numpy(), converged=d_conv.cpu().numpy().astype(bool),
               iters=d_it.cpu().numpy(), lane=lane)
    out.update(dec.lsd_stats(lane))
    return out


def _same(got, want, keys=ALL):
    for key in keys:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape, (key, a.shape, b.shape)
        bad = np.flatnonzero((a.astype(np.int64) != b.astype(np.int64)).reshape(len(a), -1).any(axis=1))
        assert bad.size == 0, (key, "shots", bad[:10], "status of the reference there", np.asarray(want["status"])[bad[:10]])


def _decoder(case, run, lsd=True):
    from bp_osd_amd import BpOsdDecoder

    return BpOsdDecoder(lc.matrix(case["code"]), lsd=lc.config_of(run) if lsd else None, **lc.settings(case, run))


@pytest.mark.parametrize("run", lc.RUNS, ids=[lc.run_id(r) for r in lc.RUNS])
@pytest.mark.parametrize("case", lc.CASES, ids=[c["id"] for c in lc.CASES])
def test_table_against_reference(gpu_ready, case, run):
    """Host bytes (the small path or a chunk, by the size of the case) and host packed words."""
    S, ref = lc.syndromes(case["id"]), lc.reference(case["id"], run)
    g = _decoder(case, run)
    got = _decode(g, S)
    if case["id"] in lc.BP_KERNEL:
        assert g.bp_kernel_info()["kernel"] == lc.BP_KERNEL[case["id"]]
    if case["id"] in lc.OSD_KERNEL and run[2] != "osd_off":
        assert g.last_osd_kernel() == lc.OSD_KERNEL[case["id"]]
    _same(got, ref)
    assert (np.ascontiguousarray(got["llr"]).view(np.uint64) == np.ascontiguousarray(ref["llr"]).view(np.uint64)).all(), "LLR bits differ"
    _same(_decode_packed(g, S), ref)


@pytest.mark.parametrize("edge", lc.EDGE_RUNS, ids=[f"{e[0]}_b{e[1]}_c{e[2]}" for e in lc.EDGE_RUNS])
def test_caps_at_the_ceilings(gpu_ready, edge):
    """A cap that some cluster meets exactly and another exceeds by one, at 64 (a second row per lane, a second word per
    row), 129 and the ceilings of 256 (tests/test_lsd_cpu.py asserts that the shots are there)."""
    case, run = lc.CASE_BY_ID[edge[0]], lc.edge_run(edge)
    S, ref = lc.syndromes(case["id"]), lc.reference(case["id"], run)
    assert (ref["status"] == 0).any() and (ref["status"] == 1).any()
    g = _decoder(case, run)
    _same(_decode(g, S), ref)
    _same(_decode_device(g, S), ref)


def test_device_pointer_call_and_lanes(gpu_ready):
    """``decode_batch_device``: consecutive calls land on different lanes, each lane keeps the words of its own call; more
    listed shots than the grid has workgroups."""
    case, run = lc.CASE_BY_ID["hgp_rep5"], lc.RUNS[0]
    S, ref = lc.syndromes(case["id"]), lc.reference(case["id"], run)
    g = _decoder(case, run)
    first = _decode_device(g, S)
    second = _decode_device(g, S[5:25])
    assert first["lane"] != second["lane"]
    _same(first, ref)
    _same(second, {k: v[5:25] for k, v in ref.items()})
    _same(g.lsd_stats(first["lane"]), ref, STATS)  # the earlier call's words are still on its lane
    reps = -(-(8 * 256 + 1) // int((ref["status"] >= 0).sum()))
    _same(_decode_device(g, np.ascontiguousarray(np.tile(S, (reps, 1)))), {k: np.tile(v, (reps,) + (1,) * (v.ndim - 1)) for k, v in ref.items()})


def test_per_shot_channel_rows(gpu_ready):
    """``channel_probs_rows=``: the LLRs the clusters grow by are the shot's own."""
    case, run = lc.CASE_BY_ID["hgp_rep5"], lc.RUNS[0]
    H, S = lc.matrix(case["code"]), lc.syndromes(case["id"])
    B, n = len(S), H.shape[1]
    P = np.clip(case["p"] * np.exp(np.random.default_rng(6).uniform(-1, 1, (B, n)) * np.log(3)), 1e-3, 0.4)
    kw = {k: v for k, v in lc.settings(case, run).items() if k != "error_rate"}
    want = {k: [] for k in ALL}
    for b in range(B):  # a decoder per shot: the oracle has one channel per handle
        r = lc.reference_decoder(H, lsd=lc.config_of(run), channel_probs=P[b], **kw).decode_batch(S[b:b + 1])
        for k in ALL:
            want[k].append(r[k])
    want = {k: np.concatenate(v) for k, v in want.items()}
    uniform = lc.reference(case["id"], run)
    assert (want["status"] == 0).sum() > 20 and (want["osdw"] != uniform["osdw"]).any()
    g = _decoder(case, run)
    _same(_decode(g, S, channel_probs_rows=P), want)
    _same(_decode(g, S), uniform)  # the handle's own channel is untouched


def test_observables(gpu_ready):
    """``decode_batch_observables``: obs_kernel reads the rows lsd_kernel wrote."""
    case, run = lc.CASE_BY_ID["hgp_rep5"], lc.RUNS[0]
    from bp_osd_amd import codes

    L = np.asarray(codes.hgp(codes.rep_code(5)).lz, dtype=np.uint8)
    S, ref = lc.syndromes(case["id"]), lc.reference(case["id"], run)
    g = _decoder(case, run)
    g.set_observables(L)
    obs = g.decode_batch_observables(S, want_osd0=True, want_bp=True)
    for key, got in (("osdw", obs), ("osd0", g.batch_obs_osd0), ("bp", g.batch_obs_bp)):
        want = (ref[key].astype(np.int64) @ L.T.astype(np.int64)) & 1
        assert (np.asarray(got) == want).all(), key
    _same(g.lsd_stats(), ref, STATS)


def test_host_call_of_two_chunks(gpu_ready, monkeypatch):
    """A packed host call cut into two chunks on two lanes: the rows of both chunks come from the compact copies."""
    case, run = lc.CASE_BY_ID["hgp_rep5"], lc.RUNS[0]
    S, ref = lc.syndromes(case["id"]), lc.reference(case["id"], run)
    half = (len(S) + 1) // 2
    monkeypatch.setenv("BPOSD_HOST_CHUNK", str(half))
    for r in (run, lc.RUNS[3]):  # (all shots solved by LSD; the OSD kernel behind a small cap)
        ref = lc.reference(case["id"], r)
        g = _decoder(case, r)
        n = g.n
        osdw = g.decode_batch(g.pack_rows(S), want_osd0=True, want_bp=True, packed=True)
        got = dict(osdw=g.unpack_rows(osdw, n), osd0=g.unpack_rows(g.batch_osd0, n), bp=g.unpack_rows(g.batch_bp, n),
                   converged=g.batch_converge, iters=g.batch_iter)
        _same(got, ref, ROWS + ("converged", "iters"))
        _same(g.lsd_stats(1), {k: ref[k][half:] for k in STATS}, STATS)  # the second chunk ran on lane 1
        _same(g.lsd_stats(0), {k: ref[k][:half] for k in STATS}, STATS)


def test_through_the_dem_engine(gpu_ready):
    """``dem_decode_sim(engine="native", lsd=cfg)`` against engine="numpy" around the reference, counter for counter."""
    from bp_osd_amd import LsdConfig, dem_decode_sim
    from bp_osd_amd.codes import surface13
    from bp_osd_amd.dem import phenomenological_dem
    from tests.dem_cases import COUNTS, ITEMS

    cd = surface13()
    H, L, priors = phenomenological_dem(cd.hz, cd.lz, 3, 0.04, 0.04)
    B = 384
    kw = dict(batch_size=B, seed=5, target_runs=B, bp_method="ms", ms_scaling_factor=0.625, max_iter=4, osd_method="osd_cs", osd_order=7,
              lsd=LsdConfig(6, 256))
    ref = dem_decode_sim(H, L, priors, engine="numpy", decoder_factory=lc.reference_decoder, **kw)
    sim = dem_decode_sim(H, L, priors, engine="native", **kw)
    st = ref.decoder.last["status"]
    assert (st == 0).sum() > 10 and (st == 1).any() and 0 < ref.bp_converge_count < B
    for c in COUNTS:
        assert getattr(sim, c) == getattr(ref, c), (c, getattr(sim, c), getattr(ref, c))
    for item in ITEMS:
        got, want = sim.last_batch(item), ref.last_batch(item)
        assert got.shape == want.shape and (got == want).all(), item
    _same(sim.decoder.lsd_stats(), ref.decoder.last, STATS)


def test_switching_off_and_refusals(gpu_ready):
    """``set_lsd(None)`` returns the handle's plain outputs and kernels; every refusal names the culprit and leaves the
    handle as it was."""
    from bp_osd_amd import LsdConfig, RelayConfig, _lib, windowed_dem_decode_sim

    case, run = lc.CASE_BY_ID["hgp_rep5"], lc.RUNS[0]
    S, ref = lc.syndromes(case["id"]), lc.reference(case["id"], run)
    g = _decoder(case, run, lsd=False)
    assert g.lsd is None
    plain = _decode(g, S)
    inst, osd = g.last_instance(), g.last_osd_kernel()
    with pytest.raises(ValueError, match="LSD mode"):
        g.lsd_stats()
    g.set_lsd(lc.config_of(run))
    _same(_decode(g, S), ref)
    assert (ref["osdw"] != plain["osdw"]).any()  # LSD-0 and osd_cs 7 differ on some shot
    g.set_lsd(None)
    assert g.lsd is None
    again = _decode(g, S)
    assert g.last_instance() == inst and g.last_osd_kernel() == osd
    for k in ROWS + ("converged", "iters"):
        assert (np.asarray(again[k]) == np.asarray(plain[k])).all(), k
    with pytest.raises(ValueError, match="LSD mode"):
        g.lsd_stats()
    # refusals
    lib = gpu_ready
    for args, word in (((1, 0, 4), "max_cluster_bits"), ((1, 257, 4), "max_cluster_bits"), ((1, 4, 0), "max_cluster_checks"),
                       ((1, 4, 257), "max_cluster_checks")):
        assert lib.bposd_set_lsd(g._h, *args) == _lib.BPOSD_ERR_INVALID, word
        assert word in lib.bposd_last_error(g._h).decode()
    assert g.lsd is None and g.bp_kernel_info()["kernel"] == lc.BP_KERNEL[case["id"]]
    with pytest.raises(TypeError):
        g.set_lsd((4, 4))
    with pytest.raises(ValueError, match="lane"):
        g.set_lsd(LsdConfig()) or g.lsd_stats(lane=99)
    relay = RelayConfig(np.zeros((1, g.n)), [3])
    with pytest.raises(ValueError, match="relay mode cannot be combined with LSD mode"):
        g.set_relay(relay)
    g.set_lsd(None)
    g.set_relay(relay)
    with pytest.raises(ValueError, match="LSD mode cannot be combined with relay mode"):
        g.set_lsd(LsdConfig())
    assert g.lsd is None
    from bp_osd_amd.codes import surface13
    from bp_osd_amd.dem import phenomenological_dem, phenomenological_detector_times

    cd = surface13()
    H, L, priors = phenomenological_dem(cd.hz, cd.lz, 4, 0.02, 0.02)
    with pytest.raises(ValueError, match="no lsd= argument"):
        windowed_dem_decode_sim(H, L, priors, phenomenological_detector_times(cd.hz.shape[0], 4), (2, 1), lsd=LsdConfig(), run_sim=False)
