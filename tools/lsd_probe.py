"""LSD mode next to the OSD stage it stands in front of, on the same shots.  Writes profiles/lsd_rates.txt.

    python tools/lsd_probe.py [--batch 131072] [--rounds 3] [--only headline,mi32,circuit] [--out profiles/lsd_rates.txt]
    python tools/lsd_probe.py --method lsd_cs --order 7 --growth 4:256,4:32 --out profiles/lsd_order_rates.txt

Per workload (the [[1922,50]] code's hz at the headline settings and at max_iter 32, p = 0.05; the circuit-level model of the
[[400,16,6]] code's memory experiment), one batch of shots through four handles of the same BP settings:
  osd_0 and osd_cs 7 without the mode   -- the OSD stage over BP's whole list
  LSD with osd_off                      -- lsd_kernel alone over the same list
  LSD with osd_cs 7 behind it           -- what a user would run
Stage times are the second interval of the call's HIP events (``last_timing()["osd_ms"]``: everything on the OSD stream
between BP's end and the call's end), `--rounds` device-pointer calls after one warm-up.  Then the share of listed shots
per LSD status at the default caps, and the logical error rate of each handle's osdw rows with binomial error bars.

With ``--method`` other than lsd_0 (or a growth setting) the handles are those of the higher orders instead: LSD-0; the
method at ``--order`` without growth; for every ``min_free_bits:grow_bits_limit`` pair of ``--growth`` the method grown for
that many free bits below that many bits, once alone and once in front of osd_cs 7; and osd_cs 7 alone.  The LSD lines then
also carry the most free columns in a cluster and the share of listed shots whose osdw row the sweep changed.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stage_ms(dec, S, rounds):
    """(median BP ms, median OSD-stream ms, osdw rows, converged) of `rounds` device-pointer calls after one warm-up."""
    import torch

    B, n = len(S), dec.n
    d_syn = torch.from_numpy(S).cuda()
    d_osdw = torch.zeros((B, n), dtype=torch.uint8, device="cuda")
    d_conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
    bp, osd = [], []
    for k in range(rounds + 1):
        dec.decode_batch_device(d_syn.data_ptr(), B, d_osdw.data_ptr(), None, None, d_conv.data_ptr(), None, None)
        dec.synchronize()
        if k:
            t = dec.last_timing()
            bp.append(t["bp_ms"])
            osd.append(t["osd_ms"])
    return float(np.median(bp)), float(np.median(osd)), d_osdw.cpu().numpy(), d_conv.cpu().numpy().astype(bool)


def rate(fail):
    p = float(fail.mean())
    return f"{p:.5f} +- {np.sqrt(p * (1 - p) / len(fail)):.5f}"


def growth_pairs(a):
    """[(min_free_bits, grow_bits_limit)] of ``--growth``."""
    return [tuple(int(x) for x in pair.split(":")) for pair in a.growth.split(",") if pair]


def order_legs(a):
    """The handles of the higher orders: (label, OSD settings, LsdConfig or None)."""
    from bp_osd_amd import LsdConfig

    off, cs7 = dict(osd_method="osd_off"), dict(osd_method="osd_cs", osd_order=7)
    name = f"{a.method} {a.order}"
    legs = [("BP + LSD-0 (osd_off)", off, LsdConfig())]
    if a.method != "lsd_0":
        legs.append((f"BP + {name} (osd_off)", off, LsdConfig(method=a.method, order=a.order)))
    for mf, limit in growth_pairs(a):
        cfg = LsdConfig(method=a.method, order=a.order, min_free_bits=mf, grow_bits_limit=limit)
        legs.append((f"BP + {name} free {mf} limit {limit} (osd_off)", off, cfg))
        legs.append((f"BP + {name} free {mf} limit {limit} + osd_cs 7", cs7, cfg))
    legs.append(("BP + osd_cs 7", cs7, None))
    return legs


def workload(say, name, H, L, priors, B, rounds, seed, legs=None, **bp_kw):
    from bp_osd_amd import BpOsdDecoder, LsdConfig
    from bp_osd_amd.sim import _mod2_mul

    import scipy.sparse as sp

    L = sp.csr_matrix(L)  # (a dense product with L takes minutes per handle at this batch size)
    rng = np.random.default_rng(seed)
    e = (rng.random((B, H.shape[1])) < priors).astype(np.uint8)
    S = _mod2_mul(H, e)
    truth = _mod2_mul(L, e)
    say(f"## {name}: {H.shape[0]} x {H.shape[1]}, {B} shots, {bp_kw}")
    legs = legs or (("BP + osd_0", dict(osd_method="osd_0"), None), ("BP + osd_cs 7", dict(osd_method="osd_cs", osd_order=7), None),
            ("BP + LSD-0 (osd_off)", dict(osd_method="osd_off"), LsdConfig()),
            ("BP + LSD-0 + osd_cs 7", dict(osd_method="osd_cs", osd_order=7), LsdConfig()))
    for label, osd_kw, cfg in legs:
        dec = BpOsdDecoder(H, channel_probs=priors, lsd=cfg, **bp_kw, **osd_kw)
        bp_ms, osd_ms, rows, conv = stage_ms(dec, S, rounds)
        fail = (_mod2_mul(L, rows) != truth).any(axis=1)
        line = f"{label:<44} BP {bp_ms:9.3f} ms   OSD-stream stage {osd_ms:9.3f} ms   listed {int((~conv).sum()):7d}   logical error rate {rate(fail)}"
        if cfg is not None:
            st = dec.lsd_stats()
            listed = st["status"] >= 0
            shares = [float((st["status"][listed] == k).mean()) if listed.any() else 0.0 for k in (0, 1, 2)]
            line += (f"   status 0 / 1 / 2 of the listed: {shares[0]:.4f} / {shares[1]:.4f} / {shares[2]:.4f}; rounds <= {int(st['rounds'].max())}, "
                     f"clusters <= {int(st['clusters'].max())}, bits per cluster <= {int(st['max_bits'].max())}")
            if cfg.higher_order:
                line += f", free columns <= {int(st['max_free'].max())}, improved {float(st['improved'][listed].mean()) if listed.any() else 0.0:.4f} of the listed"
        say(line)
        del dec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=131072)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--circuit-rounds", type=int, default=3)
    ap.add_argument("--circuit-p", type=float, default=2e-3)
    ap.add_argument("--only", default="headline,mi32,circuit", help="the workloads to run")
    ap.add_argument("--method", default="lsd_0", choices=("lsd_0", "lsd_cs", "lsd_e"))
    ap.add_argument("--order", type=int, default=0)
    ap.add_argument("--growth", default="", help="growth settings min_free_bits:grow_bits_limit, comma separated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lsd_rates.txt"))
    a = ap.parse_args()

    import torch

    from bp_osd_amd import codes
    from bp_osd_amd.circuit import circuit_dem, css_memory_circuit

    assert torch.cuda.is_available(), "no MI355X visible"
    only = set(a.only.split(","))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()  # a run replaces the file; lines are then appended as they come, so a run that is cut short leaves what it had

    def say(s):
        print(s, flush=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")

    legs = order_legs(a) if a.method != "lsd_0" or growth_pairs(a) else None
    say(f"# tools/lsd_probe.py on one MI355X: stage times are medians of {a.rounds} device-pointer calls after one warm-up")
    code = codes.h1922()
    n = code.hz.shape[1]
    for mi in [v for v, key in ((0, "headline"), (32, "mi32")) if key in only]:
        workload(say, f"[[1922,50]] hz, p = 0.05, min-sum (variable scaling factor), max_iter {mi or n}", code.hz, code.lz, np.full(n, 0.05),
                 a.batch, a.rounds, 11, legs=legs, bp_method="ms", ms_scaling_factor=0.0, max_iter=mi)
    if "circuit" not in only:
        return
    seed = np.loadtxt(os.path.join(ROOT, "tests", "golden", "mkmn_16_4_6.txt")).astype(np.uint8)
    cd = codes.hgp(seed)
    noise = {key: a.circuit_p for key in ("cx", "h", "reset", "meas", "idle", "data")}
    H, L, priors, _, _ = circuit_dem(css_memory_circuit(cd.hx, cd.hz, cd.lx, cd.lz, a.circuit_rounds, "z", noise))
    workload(say, f"circuit_dem(css_memory_circuit([[400,16,6]], rounds {a.circuit_rounds}, basis z, every noise term {a.circuit_p}))", H, L, priors,
             min(a.batch, 32768), a.rounds, 12, legs=legs, bp_method="ms", ms_scaling_factor=0.625, max_iter=32)


if __name__ == "__main__":
    main()
