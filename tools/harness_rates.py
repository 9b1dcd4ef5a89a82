"""Rates of the batched Monte-Carlo harness (bp_osd_amd.sim.css_decode_sim) on the [[1922,50]] code, p = 0.05 depolarising:
default numpy engine, torch engine fed numpy's random stream (identical counters), torch engine with the device RNG, and the
library's own engine (engine="native": sampling, syndromes, decodes and logical checks in HIP, the Philox stream).

    python tools/harness_rates.py                      # every row once
    python tools/harness_rates.py --rows torch/torch,native/philox --repeats 3 --memory

--rows picks engine/rng pairs, --repeats runs each timed window that many times (the spread is the margin rows are compared by),
--memory adds the device memory of a batch: the native engine's own allocations, torch's max_memory_allocated."""
import argparse, os, sys, time
import numpy as np
import torch  # noqa: F401  (before the decoder: INTEGRATION.md)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bp_osd_amd.codes import h1922
from bp_osd_amd.sim import css_decode_sim

c = h1922()
base = dict(hx=c.hx, hz=c.hz, error_rate=0.05, xyz_error_bias=[1, 1, 1], seed=1, bp_method="ms", ms_scaling_factor=0, max_iter=0,
            osd_method="osd_cs", osd_order=7, tqdm_disable=1)
ROWS = (("numpy", "numpy", 65536, 2), ("torch", "numpy", 65536, 3), ("torch", "torch", 131072, 8), ("native", "philox", 131072, 8))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", default=",".join(f"{e}/{r}" for e, r, _, _ in ROWS))
ap.add_argument("--repeats", type=int, default=1)
ap.add_argument("--memory", action="store_true")
args = ap.parse_args()
for cu in (None, "x->z"):
    for engine, rng, B, nb in ROWS:
        if f"{engine}/{rng}" not in args.rows.split(","):
            continue
        if args.memory and engine == "torch":
            torch.cuda.reset_peak_memory_stats()
        sim = css_decode_sim(target_runs=B, batch_size=B, channel_update=cu, engine=engine, rng=rng, **base)  # warm-up batch
        for rep in range(args.repeats):
            t0 = time.time()
            sim.target_runs = sim.run_count + B * nb
            sim.run_decode_sim()
            dt = time.time() - t0
            print(f"channel_update={cu!s:5} engine={engine:6} rng={rng:6}: {nb * B / dt:10.0f} runs/s   "
                  f"LER {sim.osdw_logical_error_rate:.2e} +- {sim.osdw_logical_error_rate_eb:.1e} after {sim.run_count} runs", flush=True)
        if args.memory and engine == "native":
            print(f"    device memory of a batch of {B}: {sim.mc_device_bytes() / 2**20:.0f} MiB held by the engine", flush=True)
        if args.memory and engine == "torch":
            print(f"    device memory of a batch of {B}: {torch.cuda.max_memory_allocated() / 2**20:.0f} MiB torch max_memory_allocated", flush=True)
        del sim
