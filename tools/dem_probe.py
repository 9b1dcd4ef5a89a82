"""Rates of the detector-error-model Monte-Carlo engine (``dem_decode_sim(engine="native")``, bposd_dem_*) on one MI355X.

``--model h1922``: ``phenomenological_dem(h1922.hz, lz, R=0, 0.05, -)`` -- the headline matrix under the headline decoder
(min-sum, osd_cs 7), so the decode underneath is the known observables call.  ``--model hgp400r3``: the R = 3 model of
hgp(mkmn_16_4_6) (768 x 2176, k = 16, p = q = 0.02), which runs on the HBM-resident kernels.

Per model, ``--rounds`` rounds, alternating, of ``--steps`` calls each:
  (a) ``bposd_dem_run`` (the C call alone) at ``--batch`` shots: runs/s, the two kernels' times from the HIP events the library records around
      them, ``bposd_dem_device_bytes``;
  (b) the bare ``decode_observables_device`` call on one of those batches' detector rows (device-resident, one call at a
      time, as the engine issues it): the engine's overhead over it is (a) - (b), with its spread over the rounds;
  (c) once, the loop the engine replaces on ``--host-shots`` of the same shots: host Philox draw, ``_mod2_mul``,
      ``decode_batch_observables``, numpy compare -- and its counters against the engine's on those shots.
Prints one line per figure; ``--out FILE`` appends them there (profiles/dem_rates.txt).

``--sample-scale BETA`` measures importance sampling instead (profiles/dem_weight_rates.txt): three engines on the model --
plain, weighted with q = p (the same faults: what the weighted instance of the sampler costs by itself) and weighted with
``sample_scale=BETA`` (more faults fire, and the decoder gets harder shots) -- alternating over the rounds, whole batches:
the sampler's HIP-event time, the ``bposd_dem_run`` call, and the batch as ``dem_decode_sim`` runs it with its fetches.

``--harvest K`` measures the harvest of failing shots instead (profiles/dem_harvest_rates.txt): two engines on the model, one
with ``harvest=K``, alternating over the rounds -- the three harvest kernels' time by HIP events, the ``bposd_dem_run`` call and
the batch as ``dem_decode_sim`` runs it, off and on -- and the kernels' time on one failure-rich batch (every shot of the
last batch selected through ``bposd_debug_dem_harvest``, against a correction of zeros).

``--fault-weight W --subset MODE`` measures the fixed-weight sampler instead (profiles/dem_subset_rates.txt): two sample-only
calls on the model, ``bposd_dem_sample`` with Bernoulli rows and with sets of weight W (``enumerate`` or ``random``),
alternating over the rounds -- each sampler's HIP-event time -- and one whole ``bposd_dem_run`` batch of the stratum.

``--fault-sums`` measures the per-fault sums over selected shots instead (profiles/dem_fault_sums_rates.txt): one engine with
the harvest on, over the rounds in turn fault_sums_kernel by HIP events on the failing shots of a batch ("failing", weighted),
on every shot ("all", weighted and counts only) and on a failure-rich batch (every shot listed through
``bposd_debug_dem_fault_sums``), the whole ``bposd_dem_fault_sums`` call, and the path it replaces: ``bposd_dem_fetch`` of the
fault rows plus ``np.unpackbits(...).sum(0)`` on the host.  Then a batch as a level of ``fit_sample_priors`` runs it next to a
plain batch."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def model(name):
    from bp_osd_amd import phenomenological_dem
    from bp_osd_amd.codes import h1922, hgp

    if name == "h1922":
        code = h1922(compute_logicals=True)
        kw = dict(max_iter=0, bp_method="ms", ms_scaling_factor=0, osd_method="osd_cs", osd_order=7)
        return phenomenological_dem(code.hz, code.lz, 0, 0.05, 0.0), kw, "[[1922,50]] hz, R = 0, p = 0.05; min-sum, osd_cs 7"
    seed = np.loadtxt(os.path.join(ROOT, "tests", "golden", "mkmn_16_4_6.txt")).astype(np.uint8)
    code = hgp(seed)
    kw = dict(max_iter=0, bp_method="ms", ms_scaling_factor=0, osd_method="osd_cs", osd_order=7)
    return phenomenological_dem(code.hz, code.lz, 3, 0.02, 0.02), kw, "hgp(mkmn_16_4_6) hz, R = 3, p = q = 0.02; min-sum, osd_cs 7"


def weighted_probe(a, say):
    """--sample-scale: the weighted sampler against the plain one."""
    import ctypes as C

    from bp_osd_amd import dem_decode_sim

    (H, L, priors), kw, what = model(a.model)
    B, seed = a.batch, 5
    say(f"# tools/dem_probe.py --sample-scale {a.sample_scale:g} on one MI355X: {what}; H {H.shape[0]} x {H.shape[1]}, k = {L.shape[0]}, B = {B}; "
        f"{a.rounds} rounds of {a.steps} batches per engine, alternating")
    make = lambda **tilt: dem_decode_sim(H, L, priors, batch_size=B, engine="native", seed=seed, target_runs=0, run_sim=False, **tilt, **kw)
    sims = {"plain": make(), "weighted, q = p": make(sample_priors=priors.copy()), f"weighted, scale {a.sample_scale:g}": make(sample_scale=a.sample_scale)}
    for sim in sims.values():
        for _ in range(2):  # warm-up: workspaces, the kernels' first launch
            sim._run_batch_native(B)
    t = {name: dict(sample=[], call=[], batch=[]) for name in sims}
    c5 = (C.c_int64 * 5)()
    for _ in range(a.rounds):
        for name, sim in sims.items():
            call = batch = 0.0
            for _ in range(a.steps):
                t0 = time.perf_counter()
                rc = sim._lib.bposd_dem_run(sim._dem, sim.run_count, B, c5)
                t1 = time.perf_counter()
                assert rc == 0, sim._lib.bposd_dem_last_error(sim._dem)
                sim._last_B = B
                sim._accumulate(B, [int(v) for v in c5], sim.last_batch("obs_fail"))
                if sim._tilted:
                    sim._accumulate_weighted(sim.last_batch("flags"), sim.last_batch("converged"), sim.last_batch("logw"))
                t2 = time.perf_counter()
                call += t1 - t0
                batch += t2 - t0
                t[name]["sample"].append(sim.kernel_ms()[0])
            t[name]["call"].append(call / a.steps * 1e3)
            t[name]["batch"].append(batch / a.steps * 1e3)
    fmt = lambda v: " / ".join(f"{x:.2f}" for x in v)
    base = np.mean(t["plain"]["sample"])
    for name, sim in sims.items():
        r = t[name]
        say(f"{name}: dem_sample_kernel, HIP events: mean {np.mean(r['sample']):.3f} ms (min {min(r['sample']):.3f}, max {max(r['sample']):.3f}, "
            f"{len(r['sample'])} batches) = {np.mean(r['sample']) / base:.2f} x plain; bposd_dem_run, ms per batch and round: {fmt(r['call'])}; "
            f"whole batch with its fetches: {fmt(r['batch'])} ({B / np.mean(r['batch']) * 1e3:,.0f} runs/s); device {sim.device_bytes() / B:.1f} B per shot")
        extra = f", weight_mean {sim.weight_mean:.4f}, effective sample fraction {sim.effective_sample_fraction:.3f}" if sim._tilted else ""
        say(f"    after {sim.run_count} shots: osdw logical error rate {sim.osdw_logical_error_rate:.3e} +- {sim.osdw_logical_error_rate_eb:.1e}, "
            f"osdw failures among the shots as sampled {1 - sim.osdw_success_count / sim.run_count:.5f}{extra}")


def subset_probe(a, say):
    """--fault-weight / --subset: dem_subset_kernel against dem_sample_kernel, the samplers alone."""
    import ctypes as C

    from bp_osd_amd import _lib, dem_decode_sim

    (H, L, priors), kw, what = model(a.model)
    B, seed = a.batch, 5
    say(f"# tools/dem_probe.py --fault-weight {a.fault_weight} --subset {a.subset} on one MI355X: {what}; H {H.shape[0]} x {H.shape[1]}, k = {L.shape[0]}, "
        f"B = {B}; {a.rounds} rounds of {a.steps} bposd_dem_sample calls per engine, alternating")
    make = lambda **more: dem_decode_sim(H, L, priors, batch_size=B, engine="native", seed=seed, target_runs=B, run_sim=False, **more, **kw)
    sims = {"Bernoulli rows": make(), f"sets of weight {a.fault_weight}, {a.subset}": make(fault_weight=a.fault_weight, subset=a.subset)}
    lib = sims["Bernoulli rows"]._lib
    t = {name: [] for name in sims}
    for name, sim in sims.items():  # warm-up: the kernels' first launch
        _lib.check_dem(lib, sim._dem, lib.bposd_dem_sample(sim._dem, 0, B))
    for r in range(a.rounds):
        for name, sim in sims.items():
            for i in range(a.steps):
                first = (r * a.steps + i) * B
                if sim._subset == "enumerate":  # stay inside the stratum
                    first %= sim.stratum_size - B + 1
                _lib.check_dem(lib, sim._dem, lib.bposd_dem_sample(sim._dem, first, B))
                sim._last_B = B
                t[name].append(sim.kernel_ms()[0])
    base = np.mean(t["Bernoulli rows"])
    for name, sim in sims.items():
        v = t[name]
        kernel = "dem_subset_kernel" if sim._subset else "dem_sample_kernel"
        say(f"{name}: {kernel}, HIP events: mean {np.mean(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f}, {len(v)} batches) = {np.mean(v) / base:.2f} x Bernoulli; "
            f"device {sim.device_bytes() / B:.1f} B per shot")
    sub = sims[f"sets of weight {a.fault_weight}, {a.subset}"]
    c5 = (C.c_int64 * 5)()
    t0 = time.perf_counter()
    _lib.check_dem(lib, sub._dem, lib.bposd_dem_run(sub._dem, 0, B, c5))
    dt = time.perf_counter() - t0
    say(f"one bposd_dem_run of {B} such sets (stratum of {sub.stratum_size:.4g}, mass {sub.stratum_mass:.3e}): {dt * 1e3:.1f} ms, "
        f"osdw failures {B - int(c5[3])}, bp converged {int(c5[0])}")


def harvest_probe(a, say):
    """--harvest: a batch with the harvest on against the same batch with it off."""
    import ctypes as C

    from bp_osd_amd import _lib, dem_decode_sim

    (H, L, priors), kw, what = model(a.model)
    B, seed, K = a.batch, 5, a.harvest
    N = H.shape[1]
    fw = (N + 63) // 64
    say(f"# tools/dem_probe.py --harvest {K} on one MI355X: {what}; H {H.shape[0]} x {N}, k = {L.shape[0]}, B = {B}; "
        f"{a.rounds} rounds of {a.steps} batches per engine, alternating")
    make = lambda **more: dem_decode_sim(H, L, priors, batch_size=B, engine="native", seed=seed, target_runs=0, run_sim=False, **more, **kw)
    sims = {"off": make(), "on": make(harvest=K)}
    for sim in sims.values():
        for _ in range(2):  # warm-up: workspaces, the kernels' first launch
            sim._run_batch_native(B)
    on = sims["on"]
    lib = on._lib
    t = {name: dict(call=[], batch=[]) for name in sims}
    k_ms, fails = [], []
    c5, ms = (C.c_int64 * 5)(), C.c_double()
    for _ in range(a.rounds):
        for name, sim in sims.items():
            call = 0.0
            if name == "on":
                _lib.check_dem(lib, sim._dem, lib.bposd_dem_set_harvest(sim._dem, K))
            for _ in range(a.steps):  # the C call alone
                t0 = time.perf_counter()
                rc = lib.bposd_dem_run(sim._dem, sim.run_count, B, c5)
                call += time.perf_counter() - t0
                assert rc == 0, lib.bposd_dem_last_error(sim._dem)
                sim._last_B = B
                sim._accumulate(B, [int(v) for v in c5], sim.last_batch("obs_fail"))
                if name == "on":
                    _lib.check_dem(lib, sim._dem, lib.bposd_debug_dem_harvest_timing(sim._dem, C.byref(ms)))
                    k_ms.append(ms.value)
                    fails.append(B - int(c5[3]))
            t0 = time.perf_counter()
            for _ in range(a.steps):  # the batch as dem_decode_sim runs it: with the fetches of a harvest
                sim._run_batch_native(B)
            t[name]["call"].append(call / a.steps * 1e3)
            t[name]["batch"].append((time.perf_counter() - t0) / a.steps * 1e3)
    fmt = lambda v: " / ".join(f"{x:.2f}" for x in v)
    say(f"harvest kernels (list + rows + min), HIP events: mean {np.mean(k_ms):.4f} ms (min {min(k_ms):.4f}, max {max(k_ms):.4f}, {len(k_ms)} batches); "
        f"failing shots per batch: mean {np.mean(fails):.1f} (min {min(fails)}, max {max(fails)}); bytes moved per batch: {B} flag bytes + "
        f"{2 * 8 * fw} B read per failing shot = {B + 2 * 8 * fw * np.mean(fails):,.0f} B, up to {2 * 8 * fw} B written per kept row")
    for name in sims:
        say(f"harvest {name}: bposd_dem_run, ms per batch and round: {fmt(t[name]['call'])}; whole batch as dem_decode_sim runs it: {fmt(t[name]['batch'])}; "
            f"device {sims[name].device_bytes() / B:.1f} B per shot")
    say(f"harvest kernels / bposd_dem_run with the harvest on: {100 * np.mean(k_ms) / np.mean(t['on']['call']):.3f} %; "
        f"on minus off, mean of the rounds: call {np.mean(t['on']['call']) - np.mean(t['off']['call']):+.3f} ms, whole batch "
        f"{np.mean(t['on']['batch']) - np.mean(t['off']['batch']):+.3f} ms")
    say(f"after {on.run_count} shots: min_logical_weight {on.min_logical_weight} at shot {on.min_logical_shot}, {int(on.failure_weight_counts.sum())} failing shots "
        f"weighed ({int(on.failure_weight_counts[on.min_logical_weight])} of that weight), {on.failures['shot'].size} kept")
    # ---- one failure-rich batch: every shot of the last batch selected, against a correction of zeros
    faults = np.ascontiguousarray(on.last_batch("faults"))
    zeros, ones = np.zeros_like(faults), np.ones(B, np.uint8)
    _lib.check_dem(lib, on._dem, lib.bposd_dem_set_harvest(on._dem, K))
    rich = []
    for _ in range(a.rounds):
        _lib.check_dem(lib, on._dem, lib.bposd_debug_dem_harvest(on._dem, faults.ctypes.data, zeros.ctypes.data, 1, ones.ctypes.data, B))
        _lib.check_dem(lib, on._dem, lib.bposd_debug_dem_harvest_timing(on._dem, C.byref(ms)))
        rich.append(ms.value)
    info = (C.c_int64 * 3)()
    _lib.check_dem(lib, on._dem, lib.bposd_dem_harvest_info(on._dem, info))
    say(f"failure-rich batch (all {int(info[0])} shots selected, K = {K}): harvest kernels, HIP events, ms: {' / '.join(f'{x:.4f}' for x in rich)}; "
        f"{B + 2 * 8 * fw * B:,} B read; batch time with such a batch: not measured (the decode of a batch that fails everywhere is another workload)")


def fault_sums_probe(a, say):
    """--fault-sums: fault_sums_kernel on the selections a batch offers, against fetching the rows."""
    import ctypes as C

    from bp_osd_amd import _lib, dem_decode_sim
    from bp_osd_amd.dem import weight_multipliers

    (H, L, priors), kw, what = model(a.model)
    B, seed = a.batch, 5
    N = H.shape[1]
    fw = (N + 63) // 64
    say(f"# tools/dem_probe.py --fault-sums on one MI355X: {what}; H {H.shape[0]} x {N}, k = {L.shape[0]}, B = {B}; {a.rounds} rounds, the forms in turn")
    sim = dem_decode_sim(H, L, priors, batch_size=B, engine="native", seed=seed, target_runs=0, run_sim=False, harvest=1, sample_priors=priors.copy(), **kw)
    lib = sim._lib
    for _ in range(2):  # warm-up: workspaces, the kernels' first launch
        sim._run_batch_native(B)
    ones32, every = np.ones(B, np.uint32), np.ones(B, np.uint8)
    forms = ("failing, weighted", "all, weighted", "all, counts", "rich, weighted", "fetch + unpackbits")
    t = {f: dict(kernel=[], call=[]) for f in forms}
    fails, bits_fail, bits_all = [], [], []
    ms = C.c_double()
    for _ in range(a.rounds):
        sim._run_batch_native(B)
        rows = sim.last_batch("fail_rows")
        v = weight_multipliers(sim.last_batch("logw")[rows])
        for form in forms[:3]:
            sel, mult = ("failing", v) if form.startswith("failing") else ("all", ones32 if form.endswith("weighted") else None)
            t0 = time.perf_counter()
            counts, _ = sim.fault_sums(sel, mult)
            t[form]["call"].append((time.perf_counter() - t0) * 1e3)
            t[form]["kernel"].append(sim.fault_sums_ms())
            (bits_fail if sel == "failing" else bits_all).append(int(counts.sum()))
        fails.append(rows.size)
        t0 = time.perf_counter()
        words = sim.last_batch("faults")
        t1 = time.perf_counter()
        host = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little").sum(0)[:N]
        t2 = time.perf_counter()
        assert (host == counts.astype(np.int64)).all()
        t["fetch + unpackbits"]["call"].append((t2 - t0) * 1e3)
        t["fetch + unpackbits"]["kernel"].append((t1 - t0) * 1e3)  # (the fetch alone)
        # a failure-rich batch: every shot of this one listed
        c, s_ = np.zeros(N, np.uint64), np.zeros(N, np.uint64)
        t0 = time.perf_counter()
        _lib.check_dem(lib, sim._dem, lib.bposd_debug_dem_fault_sums(sim._dem, words.ctypes.data, every.ctypes.data, ones32.ctypes.data, B,
                                                                      c.ctypes.data, s_.ctypes.data))
        t["rich, weighted"]["call"].append((time.perf_counter() - t0) * 1e3)
        _lib.check_dem(lib, sim._dem, lib.bposd_debug_dem_fault_sums_timing(sim._dem, C.byref(ms)))
        t["rich, weighted"]["kernel"].append(ms.value)
        assert (c == counts).all() and (s_ == counts).all()
    fmt = lambda v: " / ".join(f"{x:.4f}" for x in v)
    say(f"failing shots per batch: mean {np.mean(fails):.1f} (min {min(fails)}, max {max(fails)}); set bits walked: {np.mean(bits_fail):,.0f} in the failing rows, "
        f"{np.mean(bits_all):,.0f} in all rows; bytes read: {8 * fw} B per selected row = {8 * fw * np.mean(fails):,.0f} B (failing), {8 * fw * B:,} B (all)")
    for form in forms[:4]:
        note = " (the call uploads the rows first: the kernel's time is the figure)" if form.startswith("rich") else ""
        say(f"{form}: fault_sums_kernel, HIP events, ms per round: {fmt(t[form]['kernel'])}; the whole call, ms: {fmt(t[form]['call'])}{note}")
    r = t["fetch + unpackbits"]
    say(f"the path it replaces: bposd_dem_fetch(BPOSD_DEM_FAULTS) of {8 * fw * B:,} B, ms per round: {fmt(r['kernel'])}; with np.unpackbits(...).sum(0): {fmt(r['call'])}")
    say(f"device {sim.device_bytes() / B:.1f} B per shot ({16 * N + 4 * B:,} B of it for the sums and the multipliers)")
    # ---- a batch of a fit_sample_priors level next to a plain batch: what a level adds per batch is the fetch of the failing
    # rows' numbers and of the log-weights, the multipliers and the sums
    plain = dem_decode_sim(H, L, priors, batch_size=B, engine="native", seed=seed, target_runs=0, run_sim=False, **kw)
    for _ in range(2):
        plain._run_batch_native(B)
    t_plain, t_level, t_extra = [], [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            plain._run_batch_native(B)
        t1 = time.perf_counter()
        extra = 0.0
        for _ in range(a.steps):
            sim._run_batch_native(B)
            t2 = time.perf_counter()
            rows = sim.last_batch("fail_rows")
            v = weight_multipliers(sim.last_batch("logw")[rows])
            sim.fault_sums("failing", v)
            extra += time.perf_counter() - t2
        t3 = time.perf_counter()
        t_plain.append((t1 - t0) / a.steps * 1e3)
        t_level.append((t3 - t1) / a.steps * 1e3)
        t_extra.append(extra / a.steps * 1e3)
    fmt2 = lambda v: " / ".join(f"{x:.2f}" for x in v)
    say(f"a plain batch as dem_decode_sim runs it, ms per batch and round: {fmt2(t_plain)}; a batch of a fit_sample_priors level (weighted sampling, harvest of 1 "
        f"row, then fail_rows, logw, multipliers and the sums): {fmt2(t_level)}, of which the steps behind the batch: {fmt2(t_extra)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("h1922", "hgp400r3"), default="h1922")
    ap.add_argument("--batch", type=int, default=131072)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-shots", type=int, default=16384)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sample-scale", type=float, default=None, help="measure the weighted sampler against the plain one at this sample_scale")
    ap.add_argument("--harvest", type=int, default=None, help="measure the harvest of failing shots (this many rows kept) against a plain engine")
    ap.add_argument("--fault-weight", type=int, default=None, help="measure the fixed-weight sampler (sets of this weight) against the Bernoulli one")
    ap.add_argument("--fault-sums", action="store_true", help="measure the per-fault sums over selected shots against fetching the rows")
    ap.add_argument("--subset", choices=("enumerate", "random"), default="random", help="with --fault-weight: every set in turn, or drawn uniformly")
    a = ap.parse_args()
    if a.sample_scale is not None or a.harvest is not None or a.fault_weight is not None or a.fault_sums:
        lines = []

        def say(s):
            print(s, flush=True)
            lines.append(s)

        (fault_sums_probe if a.fault_sums else weighted_probe if a.sample_scale is not None else harvest_probe if a.harvest is not None
         else subset_probe)(a, say)
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n\n")
        return

    import torch  # (plumbing of (b) only: a device buffer for the bare decode call)
    torch.cuda.init()  # torch's HIP runtime before libbposd_mi355x.so pulls in the system one
    from bp_osd_amd import BpOsdDecoder, dem_decode_sim
    from bp_osd_amd.sim import _mod2_mul, philox_uniforms

    (H, L, priors), kw, what = model(a.model)
    M, N = H.shape
    k = L.shape[0]
    B, seed = a.batch, 5
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/dem_probe.py on one MI355X: {what}; H {M} x {N}, k = {k}, B = {B}; {a.rounds} rounds of {a.steps} calls, alternating")
    sim = dem_decode_sim(H, L, priors, batch_size=B, engine="native", seed=seed, target_runs=0, run_sim=False, **kw)
    dec = sim.decoder
    for _ in range(2):  # warm-up: workspaces, the kernels' first launch
        sim._run_batch_native(B)
    say(f"bposd_dem_device_bytes: {sim.device_bytes():,} B for capacity {B} = {sim.device_bytes() / B:.1f} B per shot "
        f"(faults {8 * ((N + 63) // 64)}, detectors {8 * ((M + 63) // 64)}, observables 4 x {8 * ((k + 63) // 64)}, flags + converged + iters 6)")
    det = sim.last_batch("detectors")
    kw_ = (k + 63) // 64
    d_det = torch.from_numpy(det.view(np.int64)).cuda()
    d_obs = [torch.empty((B, kw_), dtype=torch.int64, device="cuda") for _ in range(3)]
    d_conv = torch.empty(B, dtype=torch.uint8, device="cuda")
    d_it = torch.empty(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def bare():
        dec.decode_observables_device(d_det.data_ptr(), B, d_obs[0].data_ptr(), d_obs[1].data_ptr(), d_obs[2].data_ptr(), d_conv.data_ptr(),
                                      d_it.data_ptr(), packed=True)
        dec.synchronize()

    bare()
    same = (d_obs[0].cpu().numpy().view(np.uint64) == sim.last_batch("obs_osdw")).all()
    say(f"the bare call on the last batch's detector rows returns the engine's osdw observables: {same}")

    import ctypes as C

    t_run, t_bare, k_sample, k_score = [], [], [], []
    c5, shot = (C.c_int64 * 5)(), sim.run_count
    for _ in range(a.rounds):
        dt = 0.0
        for _ in range(a.steps):  # the C call alone is timed: the event reads below are the probe's, not the engine's
            t0 = time.perf_counter()
            rc = sim._lib.bposd_dem_run(sim._dem, shot, B, c5)
            dt += time.perf_counter() - t0
            assert rc == 0, sim._lib.bposd_dem_last_error(sim._dem)
            sim._last_B = B
            sim._accumulate(B, [int(v) for v in c5], sim.last_batch("obs_fail"))
            shot += B
            ms = sim.kernel_ms()
            k_sample.append(ms[0])
            k_score.append(ms[1])
        t_run.append(dt / a.steps * 1e3)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            bare()
        t_bare.append((time.perf_counter() - t0) / a.steps * 1e3)
    fmt = lambda v: " / ".join(f"{x:.2f}" for x in v)
    over = [r - b for r, b in zip(t_run, t_bare)]
    say(f"bposd_dem_run, ms per batch: {fmt(t_run)} ({B / np.mean(t_run) * 1e3:,.0f} runs/s)")
    say(f"bare decode_observables_device on device-resident detectors, ms per call: {fmt(t_bare)} ({B / np.mean(t_bare) * 1e3:,.0f} syndromes/s)")
    say(f"engine minus bare call, per round: {fmt(over)} ms; mean {np.mean(over):+.3f} ms, spread {max(over) - min(over):.3f} ms "
        f"({100 * np.mean(over) / np.mean(t_bare):+.1f} % of the bare call)")
    say(f"dem_sample_kernel, HIP events: mean {np.mean(k_sample):.3f} ms (min {min(k_sample):.3f}, max {max(k_sample):.3f}, {len(k_sample)} batches); "
        f"dem_score_kernel: mean {np.mean(k_score):.3f} ms (min {min(k_score):.3f}, max {max(k_score):.3f})")
    say(f"after {sim.run_count} shots: osdw logical error rate {sim.osdw_logical_error_rate:.5f} +- {sim.osdw_logical_error_rate_eb:.5f}, "
        f"bp converged {sim.bp_converge_count / sim.run_count:.4f}, no detector fired {sim.trivial_count / sim.run_count:.5f}")

    # ---- (c) the loop the engine replaces, on shots [0, host_shots) of the same stream
    Bh = min(a.host_shots, B)
    ref = dem_decode_sim(H, L, priors, batch_size=B, engine="native", seed=seed, target_runs=Bh, decoder_factory=None, **kw)
    want = [ref.bp_converge_count, ref.bp_success_count, ref.osd0_success_count, ref.osdw_success_count, ref.trivial_count]
    host = BpOsdDecoder(H, channel_probs=priors, **kw)
    host.set_observables(L)
    host.decode_batch_observables(np.zeros((64, M), np.uint8), want_osd0=True, want_bp=True)  # warm-up
    t0 = time.perf_counter()
    faults = (philox_uniforms(seed, 0, Bh, N) < priors).astype(np.uint8)
    t1 = time.perf_counter()
    detectors, truth = _mod2_mul(H, faults), _mod2_mul(L, faults)
    t2 = time.perf_counter()
    ow = host.decode_batch_observables(detectors, want_osd0=True, want_bp=True)
    t3 = time.perf_counter()
    wrong = [(o != truth).any(axis=1) for o in (host.batch_obs_bp, host.batch_obs_osd0, ow)]
    conv = host.batch_converge
    got = [int(conv.sum()), int((conv & ~wrong[0]).sum()), int((~wrong[1]).sum()), int((~wrong[2]).sum()), int((~detectors.any(axis=1)).sum())]
    t4 = time.perf_counter()
    say(f"host loop on {Bh} of the same shots: {Bh / (t4 - t0):,.0f} runs/s (Philox draw {1e3 * (t1 - t0):.0f} ms, _mod2_mul {1e3 * (t2 - t1):.0f} ms, "
        f"decode_batch_observables {1e3 * (t3 - t2):.0f} ms, numpy compare {1e3 * (t4 - t3):.0f} ms); its five counters equal the engine's: {got == want} {got}")
    say(f"engine / host loop: {B / np.mean(t_run) * 1e3 / (Bh / (t4 - t0)):.0f} x")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
