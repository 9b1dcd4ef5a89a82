"""bp_local_kernel's park at drain under every channel form and in front of every stage (run with -m gpu on an MI355X).

tests/test_gpu_local_park.py pins save and restore of a shot under one kind of call (uniform channel, constant scaling
factor, OSD-0).  The continuation also reads what the record does not hold: the shot's priors, from ``llr0[bit]``, from row
``s`` of the caller's rows or through ``sel[s]`` with ``s`` the shot index of the record; the scaling factor, from the
restored iteration; and the stage behind BP reads the list, the LLR rows and the output rows both launches wrote.  This
file parks shots (force mode: every shot that reaches its first chunk boundary parks there, nothing depends on timing)
under each of these, with the method of that file: one handle, mode never then mode force, the same device-pointer call
on outputs pre-filled with sentinels, and osdw, osd0, bp, converged and iters compared bit for bit three ways (force ==
never, never == reference, force == reference).  The reference is the CPU oracle, ``update_channel_probs`` of the shot's
row then decode (``LsdReferenceDecoder`` around it in LSD mode); it is never the device.

The plan is tests/park_forms_cases.py (asserted without a GPU by tests/test_park_forms_cpu.py).  ``last_parked`` equals
the planned count at B_EXACT shots and lies between the floor and the planned count at the batch size that selects the
kernel shape, as tests/test_gpu_local_park.py states it; ``last_instance()["bp"]`` is asserted for every call.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import park_forms_cases as pf
from tests.local_park_cases import CH, batch_index, crosses

pytestmark = pytest.mark.gpu
OUTPUTS = ("osdw", "osd0", "bp", "converged", "iters")
LSD_STATS = ("status", "rounds", "clusters", "max_bits", "max_free", "improved")
B_EXACT = pf.B_EXACT


@pytest.fixture(scope="module")
def gpu_ready():
    import torch

    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0 and torch.cuda.is_available(), "no MI355X visible"
    return torch


def _decoders(row_id, setting, max_iters, osd=("osd0", 0), tie=0, lsd=None):
    from bp_osd_amd import BpOsdDecoder

    H = pf.plan(row_id, setting)["H"]
    make = lambda mi: BpOsdDecoder(H, lsd=pf.lsd_config(lsd), **pf.settings(row_id, setting, mi, osd, tie))
    with ThreadPoolExecutor(max_workers=len(max_iters)) as ex:  # (every constructor runs the layout search)
        return dict(zip(max_iters, ex.map(make, max_iters)))


class _Batch:
    """The device inputs of one (matrix, setting, batch size): syndromes in both forms and the channel arrays, every batch
    row b holding pool row b mod N_POOL."""

    def __init__(self, torch, dec, row_id, setting, B):
        from bp_osd_amd import BpOsdDecoder

        p, ch = pf.plan(row_id, setting), pf.channel(row_id, setting)
        self.torch, self.setting, self.B, self.n = torch, setting, B, dec.n
        self.idx = batch_index(B)
        dev = torch.device("cuda", 0)
        self.at = torch.from_numpy(self.idx).to(dev)
        self.syn = torch.from_numpy(np.array(p["pool"])).to(dev)[self.at].contiguous()
        self.words = torch.from_numpy(dec.pack_rows(np.array(p["pool"])).view(np.int64)).to(dev)[self.at].contiguous()
        self.kw = {}
        if setting == "rows":
            llr, cost = BpOsdDecoder.channel_tables(ch["R"][p["rows"]])  # the pool's 32 rows, then the batch by index
            self.l0 = torch.from_numpy(llr).to(dev)[self.at].contiguous()
            self.cost = torch.from_numpy(cost).to(dev)[self.at].contiguous()
            self.kw = dict(d_prior_llr_rows=self.l0.data_ptr(), d_cost_rows=self.cost.data_ptr())
        elif setting == "sel":
            self.sel = torch.from_numpy(ch["sel"][p["rows"]]).to(dev)[self.at].contiguous()
            self.kw = dict(d_prior_select=self.sel.data_ptr(), alt_channel_probs=np.array(ch["alt"]))

    def decode(self, dec, packed=False, llr=False):
        """One device-pointer call on sentinel-filled outputs of its own: ({name: device tensor}, lane)."""
        torch, B, n = self.torch, self.B, self.n
        dev = self.syn.device
        out = dict(converged=torch.full((B,), 7, dtype=torch.uint8, device=dev), iters=torch.full((B,), -7, dtype=torch.int32, device=dev))
        if packed:
            out.update({k: torch.full((B, (n + 63) // 64), -1, dtype=torch.int64, device=dev) for k in ("osdw", "osd0", "bp")})
            assert not self.kw and not llr
            dec.decode_batch_device_packed(self.words.data_ptr(), B, out["osdw"].data_ptr(), out["osd0"].data_ptr(), out["bp"].data_ptr(),
                                           out["converged"].data_ptr(), out["iters"].data_ptr())
        else:
            out.update({k: torch.full((B, n), 9, dtype=torch.uint8, device=dev) for k in ("osdw", "osd0", "bp")})
            if llr:
                out["llr"] = torch.full((B, n), -3.0, dtype=torch.float64, device=dev)
            dec.decode_batch_device(self.syn.data_ptr(), B, out["osdw"].data_ptr(), out["osd0"].data_ptr(), out["bp"].data_ptr(),
                                    out["converged"].data_ptr(), out["iters"].data_ptr(), out["llr"].data_ptr() if llr else None, **self.kw)
        lane = dec.last_lane
        dec.synchronize()
        return out, lane

    def expected(self, dec, ref, packed):
        """The reference's pool rows as the device tensors a call must produce."""
        torch, dev = self.torch, self.syn.device
        want = {}
        for key in OUTPUTS:
            a = np.asarray(ref[key])
            if key == "iters":
                a = a.astype(np.int32)
            elif key == "converged" or not packed:
                a = a.astype(np.uint8)
            else:
                a = dec.pack_rows(a.astype(np.uint8)).view(np.int64)
            want[key] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)[self.at]
        return want


def _assert_equal(got, want, what, keys=OUTPUTS):
    for key in keys:
        g, w = got[key], want[key]
        assert g.shape == w.shape and g.dtype == w.dtype, what + (key, g.shape, w.shape, g.dtype, w.dtype)
        bad = (g != w).reshape(len(g), -1).any(dim=1)
        if bool(bad.any()):
            raise AssertionError(what + (key, "first at batch row", int(bad.nonzero()[0][0])))


def _assert_parked(parked, ref_iters, idx, nb, max_iter, n_cu, what):
    want = int(crosses(ref_iters[idx], max_iter).sum())
    print(*what, "planned", want, "parked", parked)
    if nb == B_EXACT or want == 0:
        assert parked == want, what + ("parked", parked, "planned", want)
    else:
        floor = int(crosses(ref_iters[idx[:min(nb, n_cu)]], max_iter).sum())
        assert 1 <= floor <= parked <= want, what + ("parked", parked, "planned", want, "among the first grid rows", floor)
    return want


def _never_and_force(dec, batch, ref, max_iter, n_cu, what, packed=False, instance=None):
    """The method of this file on one handle and one batch; returns (never's outputs, force's outputs, lane of force)."""
    want = batch.expected(dec, ref, packed)
    dec.set_park("never")
    never, lane = batch.decode(dec, packed)
    if instance is not None:
        assert dec.last_instance()["bp"] == instance, what + (dec.last_instance(),)
    assert dec.last_instance()["bp"][0] == "bp_local_kernel", what + (dec.last_instance(),)
    assert dec.last_parked(lane) == 0, what
    _assert_equal(never, want, what + ("never != reference",))
    dec.set_park("force")
    forced, lane = batch.decode(dec, packed)
    if instance is not None:
        assert dec.last_instance()["bp"] == instance, what + (dec.last_instance(),)
    parked = dec.last_parked(lane)
    _assert_equal(forced, want, what + ("force != reference",))
    _assert_equal(forced, never, what + ("force != never",))
    _assert_parked(parked, np.asarray(ref["iters"]), batch.idx, batch.B, max_iter, n_cu, what)
    return never, forced, lane


@pytest.mark.parametrize("case", pf.CASES, ids=[c["id"] for c in pf.CASES])
def test_forced_park_under_a_channel_form(gpu_ready, case):
    """Every setting at the batch size that selects its kernel shape and at B_EXACT, max_iter CH (the control: nothing
    parks), CH + 1, 2 CH and 2 CH + 8."""
    torch = gpu_ready
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    row_id, setting = case["row"], case["setting"]
    decs = _decoders(row_id, setting, pf.MAX_ITERS)
    for nb in (case["B"], B_EXACT):
        batch = _Batch(torch, decs[pf.MAX_ITERS[0]], row_id, setting, nb)
        for max_iter in pf.MAX_ITERS:
            dec, ref = decs[max_iter], pf.reference(row_id, setting, max_iter)
            for packed in case["forms"]:
                instance, pair, _ = pf.expected_instance(row_id, setting, nb, packed)
                what = (case["id"], "max_iter", max_iter, "B", nb, "packed" if packed else "bytes")
                _never_and_force(dec, batch, ref, max_iter, n_cu, what, packed, instance)
                assert (dec.last_pair_key() >= 0) == pair, what + ("PAIRKEY", dec.last_pair_key())
        assert all(pf.planned_parks(row_id, setting, nb, mi) > 0 for mi in pf.MAX_ITERS if mi > CH)


@pytest.mark.parametrize("stage", pf.STAGES, ids=[s["id"] for s in pf.STAGES])
def test_stage_behind_a_parked_bp(gpu_ready, stage):
    """osd_cs with the fp64 weights (the handle's ``cost`` and the caller's ``cost_rows``, both tie policies) and lsd_kernel
    (in front of osd_cs 7, alone with osd_off, with one lsd_cs sweep) read the list and the LLR rows of both launches."""
    torch = gpu_ready
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    row_id, setting = stage["row"], stage["setting"]
    decs = _decoders(row_id, setting, pf.STAGE_ITERS, stage["osd"], stage["tie"], stage["lsd"])
    for nb in (pf.STAGE_B, B_EXACT):
        batch = _Batch(torch, decs[pf.STAGE_ITERS[0]], row_id, setting, nb)
        instance = pf.expected_instance(row_id, setting, nb, False)[0]
        for max_iter in pf.STAGE_ITERS:
            dec, ref = decs[max_iter], pf.stage_reference(stage, max_iter)
            what = (stage["id"], "max_iter", max_iter, "B", nb)
            want = batch.expected(dec, ref, False)
            for mode in ("never", "force"):
                dec.set_park(mode)
                got, lane = batch.decode(dec)
                assert dec.last_instance()["bp"] == instance, what + (mode, dec.last_instance())
                _assert_equal(got, want, what + (mode + " != reference",))
                parked = dec.last_parked(lane)
                if mode == "never":
                    assert parked == 0, what
                    never = got
                else:
                    _assert_equal(got, never, what + ("force != never",))
                    assert _assert_parked(parked, np.asarray(ref["iters"]), batch.idx, nb, max_iter, n_cu, what) > 0
                if stage["lsd"] is not None:  # (the words of the lane's last call: read before the next one)
                    stats = dec.lsd_stats(lane)
                    # (the device keeps max_free and improved for the instance with a sweep only: zeros for LSD-0)
                    for k in LSD_STATS if pf.lsd_config(stage["lsd"]).higher_order else LSD_STATS[:4]:
                        assert (stats[k] == np.asarray(ref[k])[batch.idx]).all(), what + (mode, "lsd_stats", k)
            if stage["lsd"] is not None:
                assert (np.asarray(ref["status"])[batch.idx] == 0).any(), what


def test_observables_behind_a_parked_bp(gpu_ready):
    """``decode_observables_device``: obs_kernel multiplies rows both launches and the OSD kernel wrote."""
    torch = gpu_ready
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    row_id, setting = pf.OBS_ROW, "bit"
    decs = _decoders(row_id, setting, pf.STAGE_ITERS, ("osd_cs", 6))
    dev = torch.device("cuda", 0)
    for max_iter, dec in decs.items():
        L = pf.observable_matrix(dec.n)
        dec.set_observables(L)
        ref = pf.reference(row_id, setting, max_iter, ("osd_cs", 6))
        kw = (pf.OBS_K + 63) // 64
        assert kw == 2
        for nb in (pf.STAGE_B, B_EXACT):
            batch = _Batch(torch, dec, row_id, setting, nb)
            what = ("observables", "max_iter", max_iter, "B", nb)
            want = {k: torch.from_numpy(pf.observables_packed(ref[k], L).view(np.int64)).to(dev)[batch.at] for k in ("osdw", "osd0", "bp")}
            want["converged"] = torch.from_numpy(np.asarray(ref["converged"]).astype(np.uint8)).to(dev)[batch.at]
            want["iters"] = torch.from_numpy(np.asarray(ref["iters"]).astype(np.int32)).to(dev)[batch.at]
            got = {}
            for mode in ("never", "force"):
                dec.set_park(mode)
                out = {k: torch.full((nb, kw), -1, dtype=torch.int64, device=dev) for k in ("osdw", "osd0", "bp")}
                out.update(converged=torch.full((nb,), 7, dtype=torch.uint8, device=dev), iters=torch.full((nb,), -7, dtype=torch.int32, device=dev))
                dec.decode_observables_device(batch.syn.data_ptr(), nb, out["osdw"].data_ptr(), out["osd0"].data_ptr(), out["bp"].data_ptr(),
                                              out["converged"].data_ptr(), out["iters"].data_ptr())
                lane = dec.last_lane
                dec.synchronize()
                # (an observables call runs its kernels in the packed form whatever the form of the syndromes)
                assert dec.last_instance()["bp"] == pf.expected_instance(row_id, setting, nb, True)[0], what + (dec.last_instance(),)
                _assert_equal(out, want, what + (mode + " != L reference",))
                parked = dec.last_parked(lane)
                if mode == "never":
                    assert parked == 0, what
                else:
                    assert _assert_parked(parked, np.asarray(ref["iters"]), batch.idx, nb, max_iter, n_cu, what) > 0
                got[mode] = out
            _assert_equal(got["force"], got["never"], what + ("force != never",))


def test_dem_engine_behind_a_parked_bp(gpu_ready):
    """``dem_decode_sim(engine="native")`` on a local-kernel H with non-uniform priors: the decode inside the engine parks
    in force mode, and every counter and ``last_batch`` item equals engine="numpy" around the oracle and the run in mode
    never."""
    from bp_osd_amd import dem_decode_sim
    from tests.dem_cases import COUNTS, ITEMS

    H, L, priors = pf.dem_model()
    ref = pf.dem_reference()
    assert int(crosses(ref.last_batch("iters"), pf.DEM_KW["max_iter"]).sum()) > 0
    sims = {}
    for mode in ("never", "force"):
        sim = dem_decode_sim(H, L, priors, engine="native", run_sim=False, **pf.DEM_KW)
        sim.decoder.set_park(mode)
        sim.run_decode_sim()
        assert sim.decoder.last_instance()["bp"][:2] == ("bp_local_kernel", (1, 1024, 8, 0)), sim.decoder.last_instance()
        parked = max(sim.decoder.last_parked(lane) for lane in range(sim.decoder.num_lanes))
        print("dem", mode, "parked", parked)
        assert (parked > 0) == (mode == "force"), (mode, parked)
        for c in COUNTS:
            assert getattr(sim, c) == getattr(ref, c), (mode, c, getattr(sim, c), getattr(ref, c))
        for item in ITEMS:
            got, want = sim.last_batch(item), ref.last_batch(item)
            assert got.shape == want.shape and (got == want).all(), (mode, item)
        sims[mode] = sim
    for item in ITEMS:
        assert (sims["force"].last_batch(item) == sims["never"].last_batch(item)).all(), item


def test_refusals_on_the_device(gpu_ready):
    """What park_rule refuses whatever the mode, asserted on the device in force mode: a call with an LLR output, a handle
    with no stage behind BP (osd_off, no LSD) and max_iter = CH (the chunk ends at max_iter) write no record, and their
    outputs are those of mode never and of the reference."""
    torch = gpu_ready
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    row_id, setting, top = pf.REFUSAL_ROW, "bit", pf.MAX_ITERS[-1]
    assert pf.planned_parks(row_id, setting, B_EXACT, top) > 0  # (each of the first two would park without the refusal)
    for name, max_iter, osd, llr in (("llr output", top, ("osd0", 0), True), ("osd_off", top, ("osd_off", 0), False), ("max_iter CH", CH, ("osd0", 0), False)):
        dec = _decoders(row_id, setting, (max_iter,), osd)[max_iter]
        ref = pf.reference(row_id, setting, max_iter, osd)
        for nb in (pf.STAGE_B, B_EXACT):
            batch = _Batch(torch, dec, row_id, setting, nb)
            want = batch.expected(dec, ref, False)
            got = {}
            for mode in ("never", "force"):
                dec.set_park(mode)
                got[mode], lane = batch.decode(dec, llr=llr)
                assert dec.last_instance()["bp"] == pf.expected_instance(row_id, setting, nb, False)[0]
                assert dec.last_parked(lane) == 0, (name, mode, nb)
                _assert_equal(got[mode], want, (name, nb, mode + " != reference"))
            _assert_equal(got["force"], got["never"], (name, nb, "force != never"))
            if llr:  # compared as bits
                assert bool((got["force"]["llr"].view(torch.int64) == got["never"]["llr"].view(torch.int64)).all())
    # the same settings park once the LLR output is gone
    dec = _decoders(row_id, setting, (top,))[top]
    batch = _Batch(torch, dec, row_id, setting, B_EXACT)
    lane = _never_and_force(dec, batch, pf.reference(row_id, setting, top), top, n_cu, ("no llr output", B_EXACT))[2]
    assert dec.last_parked(lane) > 0
    # ... and a lane no call has run on reports 0, whatever its counter block's allocation held before (the handle above
    # has just freed blocks with a count in them)
    del dec
    fresh = _decoders(row_id, setting, (top,))[top]
    assert [fresh.last_parked(lane) for lane in range(fresh.num_lanes)] == [0] * fresh.num_lanes
