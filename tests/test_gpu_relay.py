"""The relay mode on the device (``BpOsdDecoder(..., relay=cfg)``, ``bp_relay_kernel``) bit for bit against the numpy
reference of bp_osd_amd/relay.py: every case of tests/relay_cases.py with byte and packed rows, OSD off and on, the
degenerate setting against the same handle with the mode off, per-shot channels, both kernel instances at the LDS threshold,
degrees beyond the tuned kernels, one shot and more shots than workgroups, the DEM engine, and the handle's refusals.
tests/test_relay_cpu.py checks the reference itself and that the cases are not trivial."""
import numpy as np
import pytest

from tests import relay_cases as rc

pytestmark = pytest.mark.gpu

ROWS = ("osdw", "osd0", "bp")
STATS = ("solutions", "best_leg", "weight")


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _decode(dec, S, **kw):
    osdw = dec.decode_batch(S, want_osd0=True, want_bp=True, want_llr=True, **kw)
    out = dict(osdw=osdw, osd0=dec.batch_osd0, bp=dec.batch_bp, converged=dec.batch_converge, iters=dec.batch_iter, llr=dec.batch_llr)
    if dec.relay is not None:
        out.update(dec.relay_stats())
    return out


def _decode_packed(dec, S):
    n = dec.n
    osdw = dec.decode_batch(dec.pack_rows(S), want_osd0=True, want_bp=True, packed=True)
    out = dict(osdw=dec.unpack_rows(osdw, n), osd0=dec.unpack_rows(dec.batch_osd0, n), bp=dec.unpack_rows(dec.batch_bp, n),
               converged=dec.batch_converge, iters=dec.batch_iter)
    out.update(dec.relay_stats())
    return out


def _decode_device(dec, S):
    """One ``decode_batch_device`` call: the whole batch runs as one launch on one lane."""
    import torch

    B, n = len(S), dec.n
    d_syn = torch.from_numpy(np.array(S)).cuda()
    d = [torch.zeros((B, n), dtype=torch.uint8, device="cuda") for _ in range(3)]
    d_conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
    d_it = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_llr = torch.zeros((B, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dec.decode_batch_device(d_syn.data_ptr(), B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_conv.data_ptr(), d_it.data_ptr(),
                            d_llr.data_ptr())
    lane = dec.last_lane
    dec.synchronize()
    out = dict(osdw=d[0].cpu().numpy(), osd0=d[1].cpu().numpy(), bp=d[2].cpu().numpy(), converged=d_conv.cpu().numpy().astype(bool),
               iters=d_it.cpu().numpy(), llr=d_llr.cpu().numpy(), lane=lane)
    out.update(dec.relay_stats(lane))
    return out


def _same(got, want, keys=None):
    for key in keys or [k for k in want if k in got]:
        if key == "llr":
            assert (_bits(got[key]) == _bits(want[key])).all(), "LLR bits differ"
        else:
            a, b = np.asarray(got[key]), np.asarray(want[key])
            assert a.shape == b.shape and (a.astype(np.int64) == b.astype(np.int64)).all(), (key, np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))[:10])


def _decoder(H, priors, ms, cfg, osd=("osd_off", 0), **kw):
    from bp_osd_amd import BpOsdDecoder

    return BpOsdDecoder(H, channel_probs=priors, max_iter=12, bp_method="ms", ms_scaling_factor=ms, osd_method=osd[0], osd_order=osd[1],
                        relay=cfg, **kw)


def _with_osd(H, priors, S, ref, osd):
    """The reference with the oracle's OSD on M for the shots without a solution."""
    from oracle import OracleDecoder

    o = OracleDecoder(H, channel_probs=priors, osd_method=osd[0], osd_order=osd[1])
    want = {k: np.array(v) for k, v in ref.items()}
    for b in np.flatnonzero(~ref["converged"]):
        r = o.osd(S[b], ref["llr"][b])
        want["osdw"][b], want["osd0"][b] = r["osdw"], r["osd0"]
    return want


@pytest.mark.parametrize("osd", [("osd_off", 0), ("osd_cs", 7)], ids=["osd_off", "osd_cs7"])
@pytest.mark.parametrize("case", rc.CASES, ids=[c["id"] for c in rc.CASES])
def test_table_against_reference(gpu_ready, case, osd):
    H, S, p, ref = rc.matrix(case["code"]), rc.syndromes(case["id"]), rc.priors_of(case), rc.reference(case["id"])
    want = ref if osd[0] == "osd_off" else _with_osd(H, p, S, ref, osd)
    if osd[0] != "osd_off" and not ref["converged"].all():
        assert (want["osdw"] != ref["bp"]).any(), "OSD changed no row"
    g = _decoder(H, p, case["ms"], rc.config_of(case), osd)
    got = _decode(g, S)
    assert g.last_instance()["bp"] == ("bp_relay_kernel", (1, 256), False), g.last_instance()
    assert g.bp_kernel_info()["kernel"] == "bp_relay_kernel"
    _same(got, want, ROWS + ("converged", "iters", "llr") + STATS)
    packed = _decode_packed(g, S)
    assert g.last_instance()["bp"] == ("bp_relay_kernel", (1, 256), True), g.last_instance()
    _same(packed, want, ROWS + ("converged", "iters") + STATS)


def test_degenerate_relay_and_switching_off(gpu_ready):
    """legs = 1, gammas = 0, leg_iters = [max_iter], stop_after = 1 is the handle's plain min-sum, OSD stage included; with
    the mode switched off again the handle launches what it launched before."""
    from bp_osd_amd import RelayConfig

    case = rc.CASE_BY_ID["hgp_nonuniform_negative"]
    H, S, p = rc.matrix(case["code"]), rc.syndromes("hgp_p10_r4_s2"), rc.priors_of(case)
    for ms in (0.0, 0.625):
        g = _decoder(H, p, ms, None, ("osd_cs", 7))
        assert g.relay is None
        plain = _decode(g, S)
        inst = g.last_instance()
        assert inst["bp"][0] != "bp_relay_kernel" and 0 < plain["converged"].sum() < len(S)
        with pytest.raises(ValueError, match="relay mode"):
            g.relay_stats()
        g.set_relay(RelayConfig(np.zeros((1, H.shape[1])), [12]))
        relay = _decode(g, S)
        assert g.last_instance()["bp"][0] == "bp_relay_kernel" and g.last_instance()["osd"] == inst["osd"]
        _same(relay, plain, ROWS + ("converged", "iters", "llr"))
        assert (relay["solutions"] == (plain["converged"] & S.any(axis=1))).all()
        assert (relay["best_leg"] == np.where(relay["solutions"] > 0, 0, -1)).all()
        # a real setting in between, then off
        g.set_relay(rc.config_of(case))
        assert (_decode(g, S)["iters"] != plain["iters"]).any()
        g.set_relay(None)
        assert g.relay is None
        again = _decode(g, S)
        assert g.last_instance() == inst
        _same(again, plain, ROWS + ("converged", "iters", "llr"))
        with pytest.raises(ValueError, match="relay mode"):
            g.relay_stats()


def test_per_shot_channels(gpu_ready):
    """``channel_probs_rows=`` and ``prior_select=``: priors and weights are the shot's own."""
    from bp_osd_amd import relay_decode_reference

    case = rc.CASE_BY_ID["hgp_p10_r4_s2_keep"]
    H, S, cfg = rc.matrix(case["code"]), rc.syndromes(case["id"]), rc.config_of(case)
    B, n = len(S), H.shape[1]
    rng = np.random.default_rng(6)
    P = np.clip(0.10 * np.exp(rng.uniform(-1, 1, (B, n)) * np.log(3)), 1e-3, 0.4)
    g = _decoder(H, np.full(n, 0.10), 0.625, cfg)
    want = relay_decode_reference(H, S, P, cfg, 0.625)
    uniform = rc.reference(case["id"])
    assert (want["weight"] != uniform["weight"]).any() and (want["solutions"] > 0).sum() > 5
    _same(_decode(g, S, channel_probs_rows=P), want)
    sel = (rng.random((B, n)) < 0.3).astype(np.uint8)
    alt = rng.uniform(0.02, 0.3, n)
    want = relay_decode_reference(H, S, np.full(n, 0.10), cfg, 0.625, prior_select=sel, alt_priors=alt)
    assert (want["weight"] != uniform["weight"]).any()
    _same(_decode(g, S, prior_select=sel, alt_channel_probs=alt), want)
    _same(_decode(g, S), uniform)  # the handle's own channel is untouched


@pytest.mark.parametrize("case", rc.SHAPE_CASES, ids=[c["id"] for c in rc.SHAPE_CASES])
def test_instances_and_shapes(gpu_ready, case):
    """Both instances at the LDS threshold and check degree 20 / bit degree 9; m and n are no multiples of 64.  One shot,
    the case's few shots, and more shots than the grid has workgroups (8 per CU at the most)."""
    H, S, ref = rc.matrix(case["code"]), rc.shape_syndromes(case["id"]), rc.shape_reference(case["id"])
    assert rc.expected_instance(H) == case["instance"]
    g = _decoder(H, np.full(H.shape[1], case["p"]), 0.625, rc.shape_config(case))
    keys = ROWS + ("converged", "iters", "llr") + STATS
    got = _decode(g, S)
    bp = g.last_instance()["bp"]
    assert bp[0] == "bp_relay_kernel" and bp[1][0] == case["instance"] and bp[2] is False, bp
    _same(got, ref, keys)
    _same(_decode(g, S[:1]), {k: v[:1] for k, v in ref.items()}, keys)
    _same(_decode_packed(g, S), ref, ROWS + ("converged", "iters") + STATS)
    # more shots than workgroups (256 CUs; 8 per CU at the most, 1 at the threshold, 4 on the workspace), one device-pointer call
    per_cu = 8 if case["id"] == "degrees_20_9" else (1 if case["instance"] == 1 else 4)
    reps = -(-(per_cu * 256 + 1) // len(S))
    many = np.ascontiguousarray(np.tile(S, (reps, 1)))
    _same(_decode_device(g, many), {k: np.tile(v, (reps,) + (1,) * (v.ndim - 1)) for k, v in ref.items()}, keys)


def test_device_pointer_call_and_lanes(gpu_ready):
    """``decode_batch_device``: consecutive calls land on different lanes, each lane keeps the words of its own call."""
    case = rc.CASE_BY_ID["hgp_p06_r6_s3"]
    H, S, ref = rc.matrix(case["code"]), rc.syndromes(case["id"]), rc.reference(case["id"])
    g = _decoder(H, rc.priors_of(case), case["ms"], rc.config_of(case))
    first = _decode_device(g, S)
    second = _decode_device(g, S[5:25])
    assert first["lane"] != second["lane"]
    _same(first, ref)
    _same(second, {k: v[5:25] for k, v in ref.items()})
    _same(g.relay_stats(first["lane"]), {k: ref[k] for k in STATS})  # the earlier call's words are still on its lane
    _same(g.relay_stats(), {k: ref[k][5:25] for k in STATS})


def test_through_the_dem_engine(gpu_ready):
    """``dem_decode_sim(engine="native", relay=cfg)`` against engine="numpy" around the reference: the counters and every
    ``last_batch`` item of one batch (observables of the three rows, flags, converged, iterations)."""
    from bp_osd_amd import RelayConfig, RelayReferenceDecoder, dem_decode_sim, relay_gammas
    from bp_osd_amd.codes import surface13
    from bp_osd_amd.dem import phenomenological_dem
    from tests.dem_cases import COUNTS, ITEMS

    cd = surface13()
    H, L, priors = phenomenological_dem(cd.hz, cd.lz, 3, 0.04, 0.04)
    B = 384
    cfg = RelayConfig(relay_gammas(H.shape[1], 4, seed=8), [8, 6, 6, 6], stop_after=2)
    kw = dict(batch_size=B, seed=5, target_runs=B, bp_method="ms", ms_scaling_factor=0.625, max_iter=26, osd_method="osd_off", relay=cfg)
    ref = dem_decode_sim(H, L, priors, engine="numpy", decoder_factory=RelayReferenceDecoder, **kw)
    sim = dem_decode_sim(H, L, priors, engine="native", **kw)
    assert sim.decoder.bp_kernel_info()["kernel"] == "bp_relay_kernel"
    assert 0 < ref.bp_converge_count < B and 0 < ref.bp_success_count < ref.bp_converge_count
    later = ref.decoder.last
    assert (later["best_leg"] >= 1).any() and (later["solutions"] == 0).any()
    for c in COUNTS:
        assert getattr(sim, c) == getattr(ref, c), (c, getattr(sim, c), getattr(ref, c))
    for item in ITEMS:
        got, want = sim.last_batch(item), ref.last_batch(item)
        assert got.shape == want.shape and (got == want).all(), item


def test_handle_refusals(gpu_ready):
    """``bposd_set_relay``: every refusal names the culprit and leaves the handle as it was."""
    from bp_osd_amd import BpOsdDecoder, RelayConfig, _lib

    case = rc.CASE_BY_ID["hgp_p06_r6_s3"]
    H, S, ref, cfg = rc.matrix(case["code"]), rc.syndromes(case["id"]), rc.reference(case["id"]), rc.config_of(case)
    n = H.shape[1]
    g = _decoder(H, rc.priors_of(case), case["ms"], cfg)
    lib = gpu_ready
    gam = np.ascontiguousarray(cfg.gammas)
    its = np.ascontiguousarray(cfg.leg_iters)
    bad_g = np.array(gam)
    bad_g[2, 7] = np.inf
    bad_i = np.array(its)
    bad_i[3] = 0
    for args, word in (((6, bad_g.ctypes.data, its.ctypes.data, 3, 0), "gammas[2][7]"),
                       ((6, gam.ctypes.data, bad_i.ctypes.data, 3, 0), "leg_iters[3]"),
                       ((6, gam.ctypes.data, its.ctypes.data, 0, 0), "stop_after"),
                       ((6, gam.ctypes.data, its.ctypes.data, 3, 2), "leg_init"),
                       ((6, None, its.ctypes.data, 3, 0), "gammas"),
                       ((6, gam.ctypes.data, None, 3, 0), "leg_iters"),
                       ((-1, gam.ctypes.data, its.ctypes.data, 3, 0), "legs")):
        assert lib.bposd_set_relay(g._h, *args) == _lib.BPOSD_ERR_INVALID, word
        assert word in lib.bposd_last_error(g._h).decode(), (word, lib.bposd_last_error(g._h))
        _same(_decode(g, S), ref)  # the mode and its tables are what they were
    with pytest.raises(ValueError, match="bits"):
        g.set_relay(RelayConfig(np.zeros((1, n + 1)), [3]))
    with pytest.raises(ValueError):
        g.relay_stats(lane=99)
    sol = np.zeros(len(S) + 1, np.int32)
    assert lib.bposd_relay_stats(g._h, -1, sol.ctypes.data, None, None, len(S) + 1) == _lib.BPOSD_ERR_INVALID
    for kw, word in ((dict(bp_method="ps"), "min-sum"), (dict(schedule="serial"), "flooding")):
        h = BpOsdDecoder(H, error_rate=0.06, max_iter=12, **{**dict(bp_method="ms"), **kw})
        with pytest.raises(Exception, match=word):
            h.set_relay(cfg)
        assert h.relay is None
        h.decode_batch(S)
        assert h.bp_kernel_info()["kernel"] != "bp_relay_kernel"


@pytest.mark.parametrize("window", [(3, 1), (4, 2)], ids=["w3c1", "w4c2"])
def test_through_the_window_engine(gpu_ready, window):
    """``windowed_dem_decode_sim(engine="native", relay=cfg)`` with cfg over all faults of the model against engine="numpy"
    around the reference: the windows have different widths, every one runs with its own columns of the strengths."""
    from bp_osd_amd import RelayConfig, RelayReferenceDecoder, relay_gammas, windowed_dem_decode_sim
    from tests import window_cases as wc

    H, L, priors, times = wc.model("surface13-R5")
    B = 256
    cfg = RelayConfig(relay_gammas(H.shape[1], 3, seed=12), [6, 5, 5], stop_after=2)
    kw = dict(batch_size=B, seed=5, target_runs=B, bp_method="ms", ms_scaling_factor=0.625, osd_method="osd_off", relay=cfg)
    ref = windowed_dem_decode_sim(H, L, priors, times, window, engine="numpy", decoder_factory=RelayReferenceDecoder, **kw)
    sim = windowed_dem_decode_sim(H, L, priors, times, window, engine="native", **kw)
    assert len({w.fault.size for w in sim.plan.windows}) > 1
    assert all(d.bp_kernel_info()["kernel"] == "bp_relay_kernel" and d.relay.n == d.n for d in sim.decoders)
    assert 0 < ref.bp_converge_count < B and 0 < ref.osdw_success_count < B
    for c in wc.COUNTS:
        assert getattr(sim, c) == getattr(ref, c), (c, getattr(sim, c), getattr(ref, c))
    for item in wc.ITEMS:
        got, want = sim.last_batch(item), ref.last_batch(item)
        assert got.shape == want.shape and (got == want).all(), item
