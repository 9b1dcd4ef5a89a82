"""The higher LSD orders on the device (``lsd_kernel<true>``: a candidate sweep inside every final cluster, growth for free
bits) bit for bit against ``LsdReferenceDecoder`` around the CPU oracle: every row of tests/lsd_order_cases.py as host
bytes and packed words under four runs (osd_cs 7 behind and OSD off, each under both tie policies), the device-pointer form with more
listed shots than workgroups, the two fp64 cases, observables, a host call of two chunks, the DEM engine on both engines,
switching back to LSD-0 and its kernel instance, and the refusals.  tests/test_lsd_order_cpu.py checks the reference itself
and that the rows are not trivial."""
import numpy as np
import pytest

from tests import lsd_cases as lc
from tests import lsd_order_cases as oc

pytestmark = pytest.mark.gpu

ROWS = ("osdw", "osd0", "bp")
STATS = ("status", "rounds", "clusters", "max_bits", "max_free", "improved")
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


def _decoder(case_id, order, run, **more):
    from bp_osd_amd import BpOsdDecoder

    kw = dict(oc.settings(case_id, run), **more)
    return BpOsdDecoder(oc.matrix(case_id), lsd=oc.config_of(order) if order is not None else None, **kw)


@pytest.mark.parametrize("run", oc.RUNS, ids=[oc.run_id(r) for r in oc.RUNS])
@pytest.mark.parametrize("row", oc.TABLE, ids=[oc.row_id(r) for r in oc.TABLE])
def test_table_against_reference(gpu_ready, row, run):
    """Host bytes and host packed words; every launch is of the second instance."""
    case_id, order = row
    S, ref = oc.syndromes(case_id), oc.reference(case_id, order, run)
    g = _decoder(case_id, order, run)
    _same(_decode(g, S), ref)
    _same(_decode_packed(g, S), ref)
    launches = g.lsd_launches()
    assert launches[0] == 0 and launches[1] >= 2


def test_device_pointer_call_and_lanes(gpu_ready):
    """``decode_batch_device``: each lane keeps the six words of its own call; more listed shots than the grid has
    workgroups (every workgroup decodes several shots from one set of LDS arrays)."""
    case_id, order = oc.TABLE[0]
    run = oc.RUNS[0]
    S, ref = oc.syndromes(case_id), oc.reference(case_id, order, run)
    g = _decoder(case_id, order, run)
    first = _decode_device(g, S)
    second = _decode_device(g, S[5:25])
    assert first["lane"] != second["lane"]
    _same(first, ref)
    _same(second, {k: v[5:25] for k, v in ref.items()})
    _same(g.lsd_stats(first["lane"]), ref, STATS)  # the earlier call's words are still on its lane
    reps = -(-(8 * 256 + 1) // int((ref["status"] >= 0).sum()))
    _same(_decode_device(g, np.ascontiguousarray(np.tile(S, (reps, 1)))), {k: np.tile(v, (reps,) + (1,) * (v.ndim - 1)) for k, v in ref.items()})


def test_two_valued_channel(gpu_ready):
    """``prior_select=`` / ``alt_channel_probs=``: the sweep weighs with the shot's choice between the two channels (fp64)."""
    c = oc.TWO_VALUED
    want, _ = oc.per_shot_reference("two_valued")
    sel, alt = oc.two_valued_channel()
    assert want["improved"].sum() >= 3
    g = _decoder(c["case"], c["order"], oc.RUNS[0])
    _same(_decode(g, oc.syndromes(c["case"]), prior_select=sel, alt_channel_probs=alt), want)


def test_per_shot_channel_rows(gpu_ready):
    """``channel_probs_rows=``: the sweep weighs with the shot's own row (fp64), behind osd_cs 7 and with OSD off."""
    c = oc.ROWS
    S = oc.syndromes(c["case"])
    for run in oc.RUNS[:2]:
        want, P = oc.per_shot_reference("rows", run)
        assert want["improved"].sum() >= 3
        g = _decoder(c["case"], c["order"], run)
        _same(_decode(g, S, channel_probs_rows=P), want)
    _same(_decode(g, S), oc.reference(c["case"], c["order"], run))  # the handle's own channel is untouched


def test_per_shot_channel_rows_on_the_device(gpu_ready):
    """``decode_batch_device(d_prior_llr_rows=, d_cost_rows=)`` with a sweep on: the shot's own weights reach the sweep with
    OSD off too, and there the weight rows are required (the refusal names the sweep and launches nothing)."""
    import torch

    from bp_osd_amd import BpOsdDecoder

    c = oc.ROWS
    S = oc.syndromes(c["case"])
    B = len(S)
    run = oc.RUNS[1]  # OSD off: only the sweep weighs
    want, P = oc.per_shot_reference("rows", run)
    g = _decoder(c["case"], c["order"], run)
    llr0, cost = BpOsdDecoder.channel_tables(P)
    d_l0, d_cost = torch.from_numpy(llr0).cuda(), torch.from_numpy(cost).cuda()
    d_syn = torch.from_numpy(np.array(S)).cuda()
    d = [torch.zeros((B, g.n), dtype=torch.uint8, device="cuda") for _ in range(3)]
    d_conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
    d_it = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    before = g.lsd_launches()
    with pytest.raises(ValueError, match="LSD sweep"):
        g.decode_batch_device(d_syn.data_ptr(), B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_conv.data_ptr(), d_it.data_ptr(),
                              d_prior_llr_rows=d_l0.data_ptr())
    assert g.lsd_launches() == before
    g.decode_batch_device(d_syn.data_ptr(), B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_conv.data_ptr(), d_it.data_ptr(),
                          d_prior_llr_rows=d_l0.data_ptr(), d_cost_rows=d_cost.data_ptr())
    lane = g.last_lane
    g.synchronize()
    got = dict(osdw=d[0].cpu().numpy(), osd0=d[1].cpu().numpy(), bp=d[2].cpu().numpy(), converged=d_conv.cpu().numpy().astype(bool),
               iters=d_it.cpu().numpy())
    got.update(g.lsd_stats(lane))
    _same(got, want)
    g.set_lsd(oc.config_of(oc.order_kw("lsd_0", 0, 8)))  # growth alone weighs nothing: the weight rows may be missing again
    g.decode_batch_device(d_syn.data_ptr(), B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_conv.data_ptr(), d_it.data_ptr(),
                          d_prior_llr_rows=d_l0.data_ptr())
    g.synchronize()


def test_bit_order_of_lsd_e_and_weight_fn(gpu_ready):
    """``osd_e_bit_order=1`` reverses the patterns of lsd_e; ``weight_fn=1`` counts bits on a non-uniform channel."""
    for case_id, w, more in (("hgp_rep5", 5, dict(osd_e_bit_order=1)), ("chain_248", 8, dict(weight_fn=1)), ("chain_248", 8, dict(osd_e_bit_order=1))):
        order = oc.order_kw("lsd_e", w, 8)
        run = ("osd_e", 5, 0)
        S = oc.syndromes(case_id)
        kw = dict(oc.settings(case_id, run), **more)
        ref = lc.reference_decoder(oc.matrix(case_id), lsd=oc.config_of(order), **kw).decode_batch(S)
        assert ref["improved"].any()
        _same(_decode(_decoder(case_id, order, run, **more), S), ref)


def test_observables(gpu_ready):
    """``decode_batch_observables``: obs_kernel reads the rows lsd_kernel wrote."""
    from bp_osd_amd import codes

    case_id, order = oc.TABLE[1]
    run = oc.RUNS[0]
    L = np.asarray(codes.hgp(codes.rep_code(5)).lz, dtype=np.uint8)
    S, ref = oc.syndromes(case_id), oc.reference(case_id, order, run)
    g = _decoder(case_id, order, run)
    g.set_observables(L)
    obs = g.decode_batch_observables(S, want_osd0=True, want_bp=True)
    for key, got in (("osdw", obs), ("osd0", g.batch_obs_osd0), ("bp", g.batch_obs_bp)):
        want = (ref[key].astype(np.int64) @ L.T.astype(np.int64)) & 1
        assert (np.asarray(got) == want).all(), key
    _same(g.lsd_stats(), ref, STATS)


def test_host_call_of_two_chunks(gpu_ready, monkeypatch):
    """A packed host call cut into two chunks on two lanes: both rows of both chunks come from the compact copies."""
    case_id, order = oc.TABLE[1]
    S = oc.syndromes(case_id)
    half = (len(S) + 1) // 2
    monkeypatch.setenv("BPOSD_HOST_CHUNK", str(half))
    for run, bits in ((oc.RUNS[0], lc.LSD_MAX), (("osd_cs", 7, 1), 24)):  # (all shots solved by LSD; the OSD kernel behind a small cap)
        cfg = oc.config_of(order, bits=bits)
        ref = lc.reference_decoder(oc.matrix(case_id), lsd=cfg, **oc.settings(case_id, run)).decode_batch(S)
        assert (ref["status"] == 0).any() and (bits == lc.LSD_MAX or (ref["status"] == 1).any())
        from bp_osd_amd import BpOsdDecoder

        g = BpOsdDecoder(oc.matrix(case_id), lsd=cfg, **oc.settings(case_id, run))
        n = g.n
        osdw = g.decode_batch(g.pack_rows(S), want_osd0=True, want_bp=True, packed=True)
        got = dict(osdw=g.unpack_rows(osdw, n), osd0=g.unpack_rows(g.batch_osd0, n), bp=g.unpack_rows(g.batch_bp, n),
                   converged=g.batch_converge, iters=g.batch_iter)
        _same(got, ref, ROWS + ("converged", "iters"))
        _same(g.lsd_stats(1), {k: ref[k][half:] for k in STATS}, STATS)  # the second chunk ran on lane 1
        _same(g.lsd_stats(0), {k: ref[k][:half] for k in STATS}, STATS)


def test_through_the_dem_engine(gpu_ready):
    """``dem_decode_sim(engine="native", lsd=cfg)`` with growth and a sweep against engine="numpy" around the reference,
    counter for counter."""
    from bp_osd_amd import LsdConfig, dem_decode_sim
    from bp_osd_amd.codes import surface13
    from bp_osd_amd.dem import phenomenological_dem
    from tests.dem_cases import COUNTS, ITEMS

    cd = surface13()
    H, L, priors = phenomenological_dem(cd.hz, cd.lz, 3, 0.04, 0.04)
    B = 384
    kw = dict(batch_size=B, seed=5, target_runs=B, bp_method="ms", ms_scaling_factor=0.625, max_iter=4, osd_method="osd_cs", osd_order=7,
              lsd=LsdConfig(24, 256, method="lsd_cs", order=7, min_free_bits=4))
    ref = dem_decode_sim(H, L, priors, engine="numpy", decoder_factory=lc.reference_decoder, **kw)
    sim = dem_decode_sim(H, L, priors, engine="native", **kw)
    last = ref.decoder.last
    assert (last["status"] == 0).sum() > 10 and (last["status"] == 1).any() and last["improved"].any() and last["max_free"].max() >= 4
    for c in COUNTS:
        assert getattr(sim, c) == getattr(ref, c), (c, getattr(sim, c), getattr(ref, c))
    for item in ITEMS:
        got, want = sim.last_batch(item), ref.last_batch(item)
        assert got.shape == want.shape and (got == want).all(), item
    _same(sim.decoder.lsd_stats(), last, STATS)


def test_switching_back_and_refusals(gpu_ready):
    """``set_lsd(LsdConfig())`` after a higher order gives LSD-0's reference from the LSD-0 instance; every refusal names the
    culprit, leaves the handle as it was and launches nothing."""
    from bp_osd_amd import LsdConfig, RelayConfig, _lib, windowed_dem_decode_sim

    case_id, order = oc.TABLE[1]
    run = oc.RUNS[0]
    S, ref = oc.syndromes(case_id), oc.reference(case_id, order, run)
    ref0 = lc.reference(case_id, lc.RUNS[0])
    assert (ref["osdw"] != ref0["osdw"]).any()
    g = _decoder(case_id, order, run)
    _same(_decode(g, S), ref)
    assert g.lsd_launches() == (0, 1)
    g.set_lsd(LsdConfig())
    got = _decode(g, S)
    _same(got, ref0, ROWS + ("converged", "iters", "status", "rounds", "clusters", "max_bits"))
    assert not got["max_free"].any() and not got["improved"].any()
    assert g.lsd_launches() == (1, 1)
    g.set_lsd(LsdConfig(min_free_bits=8))  # growth alone: the second instance, no sweep
    grown = lc.reference_decoder(oc.matrix(case_id), lsd=LsdConfig(min_free_bits=8), **oc.settings(case_id, run)).decode_batch(S)
    _same(_decode(g, S), grown)
    assert (grown["osd0"] == grown["osdw"]).all() and grown["max_free"].max() >= 8 and g.lsd_launches() == (1, 2)
    g.set_lsd(None)  # the order settings stay on the handle; a plain switch-on in C keeps them
    assert gpu_ready.bposd_set_lsd(g._h, 1, 256, 256) == 0
    _same(_decode_no_cfg(g, S), grown, ROWS + ("converged", "iters"))
    assert g.lsd_launches() == (1, 3)
    g.set_lsd(oc.config_of(order))
    # refusals
    lib = gpu_ready
    before = g.lsd_launches()
    for args, word in (((3, 1, 0, 256), "method"), ((-1, 0, 0, 256), "method"), ((0, 1, 0, 256), "order"), ((1, 0, 0, 256), "order"),
                       ((1, 65, 0, 256), "order"), ((2, 11, 0, 256), "order"), ((1, 7, -1, 256), "min_free_bits"), ((1, 7, 65, 256), "min_free_bits"),
                       ((1, 7, 8, 0), "grow_bits_limit"), ((1, 7, 8, 257), "grow_bits_limit")):
        assert lib.bposd_set_lsd_order(g._h, *args) == _lib.BPOSD_ERR_INVALID, (args, word)
        assert word in lib.bposd_last_error(g._h).decode(), (args, word)
    with pytest.raises(TypeError):
        g.set_lsd(("lsd_cs", 7))
    with pytest.raises(ValueError, match="syndromes, not"):
        _lib.check(lib, g._h, lib.bposd_lsd_order_stats(g._h, -1, np.zeros(3, np.int32).ctypes.data, None, 3))
    _same(_decode(g, S), ref)  # the handle as it was
    assert g.lsd_launches() == (before[0], before[1] + 1)
    relay = RelayConfig(np.zeros((1, g.n)), [3])
    with pytest.raises(ValueError, match="relay mode cannot be combined with LSD mode"):
        g.set_relay(relay)
    g.set_lsd(None)
    g.set_relay(relay)
    with pytest.raises(ValueError, match="LSD mode cannot be combined with relay mode"):
        g.set_lsd(oc.config_of(order))
    assert g.lsd is None and g.lsd_launches() == (before[0], before[1] + 1)
    from bp_osd_amd.codes import surface13
    from bp_osd_amd.dem import phenomenological_dem, phenomenological_detector_times

    cd = surface13()
    H, L, priors = phenomenological_dem(cd.hz, cd.lz, 4, 0.02, 0.02)
    with pytest.raises(ValueError, match="no lsd= argument"):
        windowed_dem_decode_sim(H, L, priors, phenomenological_detector_times(cd.hz.shape[0], 4), (2, 1), lsd=oc.config_of(order), run_sim=False)


def _decode_no_cfg(dec, S):
    osdw = dec.decode_batch(S, want_osd0=True, want_bp=True)
    return dict(osdw=osdw, osd0=dec.batch_osd0, bp=dec.batch_bp, converged=dec.batch_converge, iters=dec.batch_iter)
