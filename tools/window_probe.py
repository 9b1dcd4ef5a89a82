"""Rates of the sliding-window engine (``windowed_dem_decode_sim(engine="native")``, bposd_window_*) on one MI355X, against
the unwindowed engine on the same shots.

Model: the phenomenological model of hgp(mkmn_16_4_6) ([[400,16,6]], hz 192 x 400), p = q = ``--p``; decoder min-sum 0.625,
``--max-iter`` iterations, osd_cs 7 for every leg.

1. ``--rounds`` noisy rounds (default 11): legs ``dem_decode_sim`` (one matrix) and one windowed run per ``--windows`` entry.
   After a warm-up batch per leg, ``--repeats`` rounds alternate the legs, one batch of ``--batch`` shots each.  Per leg: ms
   per batch, runs/s, device bytes of the engine, the logical error rate with its error bar over every shot the leg saw (all
   legs see the same shots), and for a windowed leg the summed window_step_kernel time and the window_score_kernel time from
   the HIP events the library records around them.
2. ``--long-rounds`` noisy rounds (default 63; N = 37696): the unwindowed constructor's refusal, verbatim, and the windowed
   runs/s at the first ``--windows`` entry.
Prints one line per figure; ``--out FILE`` appends them there (profiles/window_rates.txt)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def model(rounds, p):
    from bp_osd_amd import phenomenological_dem, phenomenological_detector_times
    from bp_osd_amd.codes import hgp

    seed = np.loadtxt(os.path.join(ROOT, "tests", "golden", "mkmn_16_4_6.txt")).astype(np.uint8)
    code = hgp(seed)
    H, L, priors = phenomenological_dem(code.hz, code.lz, rounds, p, p)
    return H, L, priors, phenomenological_detector_times(code.hz.shape[0], rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--long-rounds", type=int, default=63)
    ap.add_argument("--p", type=float, default=0.01)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=32)
    ap.add_argument("--windows", default="3,1 4,2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from bp_osd_amd import dem_decode_sim, windowed_dem_decode_sim

    kw = dict(max_iter=a.max_iter, bp_method="ms", ms_scaling_factor=0.625, osd_method="osd_cs", osd_order=7)
    windows = [tuple(int(v) for v in w.split(",")) for w in a.windows.split()]
    B, seed = a.batch, 5
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- 1. windowed against unwindowed
    H, L, priors, times = model(a.rounds, a.p)
    M, N = H.shape
    say(f"# tools/window_probe.py on one MI355X: hgp(mkmn_16_4_6) hz, R = {a.rounds}, p = q = {a.p}; H {M} x {N}, k = {L.shape[0]}, B = {B}; "
        f"min-sum 0.625, max_iter {a.max_iter}, osd_cs 7; warm-up, then {a.repeats} rounds alternating the legs, one batch each")
    legs = [("unwindowed", dem_decode_sim(H, L, priors, batch_size=B, engine="native", seed=seed, target_runs=0, run_sim=False, **kw))]
    for w in windows:
        sim = windowed_dem_decode_sim(H, L, priors, times, w, batch_size=B, engine="native", seed=seed, target_runs=0, run_sim=False, **kw)
        shapes = sorted({sim.plan.windows[u].H.shape for u in sim.plan.unique})
        say(f"window {w}: {len(sim.plan.windows)} windows on {len(sim.plan.unique)} decoders, shapes {shapes}")
        legs.append((f"window {w}", sim))
    ms = {name: [] for name, _ in legs}
    kernel = {name: [] for name, _ in legs}
    for name, sim in legs:  # warm-up: workspaces, the kernels' first launch
        sim._run_batch_native(B)
    for _ in range(a.repeats):
        for name, sim in legs:
            t0 = time.perf_counter()
            sim._run_batch_native(B)
            ms[name].append((time.perf_counter() - t0) * 1e3)
            if name != "unwindowed":
                kernel[name].append(sim.kernel_ms())
    fmt = lambda v: " / ".join(f"{x:.2f}" for x in v)
    for name, sim in legs:
        say(f"{name}: ms per batch {fmt(ms[name])} ({B / np.mean(ms[name]) * 1e3:,.0f} runs/s); engine device bytes {sim.device_bytes():,}; "
            f"after {sim.run_count} shots osdw logical error rate {sim.osdw_logical_error_rate:.5f} +- {sim.osdw_logical_error_rate_eb:.5f}, "
            f"bp converged {sim.bp_converge_count / sim.run_count:.4f}")
        if kernel[name]:
            st, sc = [k[0] for k in kernel[name]], [k[1] for k in kernel[name]]
            say(f"{name}: window_step_kernel, summed over the batch's {len(sim.plan.windows) + 1} launches, HIP events: mean {np.mean(st):.3f} ms "
                f"(min {min(st):.3f}, max {max(st):.3f}); window_score_kernel: mean {np.mean(sc):.3f} ms; residual not zero in {sim.residual_count} shots")
    del legs

    # ---- 2. beyond the unwindowed decoder's limits
    H, L, priors, times = model(a.long_rounds, a.p)
    M, N = H.shape
    say(f"# R = {a.long_rounds}: H {M} x {N}")
    try:
        dem_decode_sim(H, L, priors, batch_size=B, engine="native", seed=seed, target_runs=0, run_sim=False, **kw)
        say("unwindowed: the constructor accepted the model")
    except ValueError as e:
        say(f"unwindowed: refused -- {e}")
    w = windows[0]
    t0 = time.perf_counter()
    sim = windowed_dem_decode_sim(H, L, priors, times, w, batch_size=B, engine="native", seed=seed, target_runs=0, run_sim=False, **kw)
    say(f"window {w}: {len(sim.plan.windows)} windows on {len(sim.plan.unique)} decoders; plan, decoders and engine made in {time.perf_counter() - t0:.1f} s; "
        f"engine device bytes {sim.device_bytes():,}")
    sim._run_batch_native(B)
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        sim._run_batch_native(B)
        t.append((time.perf_counter() - t0) * 1e3)
    st = sim.kernel_ms()
    say(f"window {w}: ms per batch {fmt(t)} ({B / np.mean(t) * 1e3:,.0f} runs/s, {B * a.long_rounds / np.mean(t) * 1e3:,.0f} shot-rounds/s); window_step_kernel summed "
        f"{st[0]:.3f} ms, window_score_kernel {st[1]:.3f} ms; after {sim.run_count} shots osdw logical error rate {sim.osdw_logical_error_rate:.5f} +- "
        f"{sim.osdw_logical_error_rate_eb:.5f}, residual not zero in {sim.residual_count} shots")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
