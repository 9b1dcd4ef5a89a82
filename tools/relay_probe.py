"""Relay mode on [[1922,50]] (hz, 961 x 1922, 5766 edges): kernel times against the any-degree kernel and the tuned default,
and what a real relay setting buys.  Writes profiles/relay_rates.txt.

    python tools/relay_probe.py [--batch 131072] [--rounds 5] [--p 0.05] [--max-iter 32] [--out profiles/relay_rates.txt]

Part 1 (the kernel against its yardstick, same syndromes, OSD off, `--rounds` timed device-pointer calls each after one
warm-up; kernel time from the call's HIP events):
  relay at legs = 1, gammas = 0, leg_iters = [max_iter]   -- plain min-sum through bp_relay_kernel
  bposd_set_bp_variant(64)                                 -- bp_anydeg_kernel: the same indexing and work, messages in HBM
  the tuned default kernel
Part 2 (a real setting: relay_gammas defaults, 5 legs of 60 / 30 / 30 / 30 / 30 iterations, stop_after = 1): the share of
shots without a solution against plain min-sum's non-converged share at the same 180 iterations, and the logical error rate
of relay alone against min-sum + osd_cs 7 through dem_decode_sim on the code-capacity model.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_calls(dec, d_syn, B, bufs, rounds):
    """Kernel ms of `rounds` device-pointer calls after one warm-up, and the outputs of the last one."""
    ms = []
    for k in range(rounds + 1):
        dec.decode_batch_device(d_syn.data_ptr(), B, bufs["osdw"].data_ptr(), None, bufs["bp"].data_ptr(), bufs["conv"].data_ptr(),
                                bufs["iters"].data_ptr(), None)
        dec.synchronize()
        if k:
            ms.append(dec.last_timing()["bp_ms"])
    return ms


def line(name, ms, B):
    lo, hi, med = min(ms), max(ms), float(np.median(ms))
    return f"{name:<44} kernel ms median {med:9.3f}  range {lo:9.3f} .. {hi:9.3f}   {B / med * 1e3:14.0f} shots/s"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=131072)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--p", type=float, default=0.05)
    ap.add_argument("--max-iter", type=int, default=32)
    ap.add_argument("--ler-shots", type=int, default=32768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relay_rates.txt"))
    a = ap.parse_args()

    import torch

    from bp_osd_amd import BpOsdDecoder, RelayConfig, dem_decode_sim, relay_gammas
    from bp_osd_amd.codes import h1922
    from bp_osd_amd.dem import phenomenological_dem

    code = h1922()
    H = code.hz
    m, n = H.shape
    B = a.batch
    rng = np.random.default_rng(0)
    err = (rng.random((B, n)) < a.p).astype(np.uint8)
    S = np.ascontiguousarray((np.asarray(H.astype(np.int32) @ err.T.astype(np.int32)) & 1).T.astype(np.uint8))
    d_syn = torch.from_numpy(S).cuda()
    bufs = dict(osdw=torch.zeros((B, n), dtype=torch.uint8, device="cuda"), bp=torch.zeros((B, n), dtype=torch.uint8, device="cuda"),
                conv=torch.zeros(B, dtype=torch.uint8, device="cuda"), iters=torch.zeros(B, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    out = [f"relay_probe: [[1922,50]] hz {m} x {n}, {H.nnz} edges, p = {a.p}, B = {B}, min-sum 0.625, measured {time.strftime('%Y-%m-%d')}", ""]

    def decoder(max_iter, **kw):
        return BpOsdDecoder(H, error_rate=a.p, max_iter=max_iter, bp_method="ms", ms_scaling_factor=0.625, osd_method="osd_off", **kw)

    # ---- part 1
    out.append(f"Part 1: one BP launch of {B} shots, max_iter {a.max_iter}, OSD off, {a.rounds} rounds after one warm-up")
    results = {}
    for name, make in (("relay, legs 1, gammas 0 (bp_relay_kernel)", lambda: decoder(a.max_iter, relay=RelayConfig(np.zeros((1, n)), [a.max_iter]))),
                       ("set_bp_variant(64) (bp_anydeg_kernel)", lambda: decoder(a.max_iter)),
                       ("tuned default", lambda: decoder(a.max_iter))):
        dec = make()
        if "variant" in name:
            dec.set_bp_variant(64)
        ms = timed_calls(dec, d_syn, B, bufs, a.rounds)
        inst = dec.last_instance()["bp"]
        results[name] = (ms, bufs["bp"].cpu().numpy().copy(), bufs["iters"].cpu().numpy().copy())
        out.append(line(name, ms, B) + f"   {inst[0]} {inst[1]}")
    names = list(results)
    same = all((results[names[0]][1] == results[k][1]).all() and (results[names[0]][2] == results[k][2]).all() for k in names[1:])
    med = {k: float(np.median(v[0])) for k, v in results.items()}
    out.append(f"identical decisions and iteration counts across the three: {same}")
    out.append(f"relay / any-degree = {med[names[0]] / med[names[1]]:.3f}   relay / tuned default = {med[names[0]] / med[names[2]]:.3f}")
    out.append("")

    # ---- part 2
    legs = [60, 30, 30, 30, 30]
    cfg = RelayConfig(relay_gammas(n, len(legs)), legs, stop_after=1)
    out.append(f"Part 2: relay_gammas defaults (not tuned), legs {legs}, stop_after 1, against plain min-sum at max_iter {sum(legs)}")
    dec = decoder(sum(legs), relay=cfg)
    ms = timed_calls(dec, d_syn, B, bufs, a.rounds)
    st = dec.relay_stats(dec.last_lane)
    open_relay = float((st["solutions"] == 0).mean()) - float((~S.any(axis=1)).mean())
    out.append(line("relay", ms, B))
    out.append("first solution by leg: " + ", ".join(f"{r}: {int((st['best_leg'] == r).sum())}" for r in range(len(legs))))
    dec = decoder(sum(legs))
    ms = timed_calls(dec, d_syn, B, bufs, a.rounds)
    open_plain = 1.0 - float(bufs["conv"].cpu().numpy().mean())
    out.append(line("plain min-sum, tuned default", ms, B))
    out.append(f"shots without a solution: relay {open_relay:.5f}   plain min-sum not converged {open_plain:.5f}")
    Hm, L, priors = phenomenological_dem(code.hz, code.lz, 0, a.p, 0.0)
    common = dict(batch_size=min(a.ler_shots, 16384), engine="native", seed=1, target_runs=a.ler_shots, bp_method="ms", ms_scaling_factor=0.625,
                  max_iter=sum(legs))
    for name, kw in (("relay alone (osd_off)", dict(osd_method="osd_off", relay=cfg)), ("min-sum + osd_cs 7", dict(osd_method="osd_cs", osd_order=7))):
        sim = dem_decode_sim(Hm, L, priors, **common, **kw)
        out.append(f"{name:<24} logical error rate {sim.osdw_logical_error_rate:.5f} +- {sim.osdw_logical_error_rate_eb:.5f}  ({a.ler_shots} shots, "
                   f"bp converged {sim.bp_converge_count})")
    out.append("")
    out.append("Not measured here: circuit-level models, tuned memory strengths, stop_after > 1.")
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
