"""Rates of the per-shot channel on [[1922,50]] (hz, min-sum, osd_cs 7, the headline configuration) at B = 131072.

Device-resident: the plain call, the two-valued ``prior_select`` call and the rows call (``d_prior_llr_rows`` /
``d_cost_rows``), the last two on the SAME channel (rows = where(select, alt, q)) so that they decode the same work; the
errors are drawn from that channel, so the plain call decodes them with a mismatched (uniform) channel.  Next
to them the only way to give every shot its own channel without the rows call -- ``update_channel_probs`` + ``decode`` per
shot, over 2000 shots -- and the host-pointer rows call (validation, conversion and upload of 16 B per bit and shot
included).  Prints one line per rate; ``--out FILE`` also writes them there (profiles/channel_rows_rates.txt)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=131072)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--loop-shots", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from bp_osd_amd import BpOsdDecoder
    from bp_osd_amd.codes import h1922

    H = h1922(compute_logicals=False).hz
    m, n = H.shape
    B, q = a.batch, 0.05
    rng = np.random.default_rng(0)
    sel = rng.random((B, n)) < 0.2
    alt = rng.uniform(0.02, 0.2, n)
    P = np.where(sel, alt, q)  # the channel of the select call, row by row
    err = (rng.random((B, n)) < P).astype(np.uint8)
    S = np.empty((B, m), np.uint8)
    for lo in range(0, B, 8192):
        S[lo:lo + 8192] = (np.asarray(H @ err[lo:lo + 8192].T.astype(np.int32)) & 1).T
    del err
    kw = dict(error_rate=q, max_iter=0, bp_method="ms", ms_scaling_factor=0, osd_method="osd_cs", osd_order=7)
    dec = BpOsdDecoder(H, **kw)

    d_syn = torch.from_numpy(S).cuda()
    d_sel = torch.from_numpy(sel.astype(np.uint8)).cuda()
    # the rows as channel_tables() makes them, assembled on the device from the tables of the two channels they mix
    (l0_q, cost_q), (l0_alt, cost_alt) = BpOsdDecoder.channel_tables([q]), BpOsdDecoder.channel_tables(alt)
    d_l0 = torch.where(d_sel != 0, torch.from_numpy(l0_alt).cuda(), torch.from_numpy(l0_q).cuda())
    d_cost = torch.where(d_sel != 0, torch.from_numpy(cost_alt).cuda(), torch.from_numpy(cost_q).cuda())
    assert d_l0.shape == (B, n) and d_l0.dtype == torch.float64 and d_l0.is_contiguous()
    d_out = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    d_conv = torch.empty(B, dtype=torch.uint8, device="cuda")
    d_it = torch.empty(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    common = (d_syn.data_ptr(), B, d_out.data_ptr(), None, None, d_conv.data_ptr(), d_it.data_ptr(), None)
    calls = (("plain", {}),
             ("prior_select", dict(d_prior_select=d_sel.data_ptr(), alt_channel_probs=alt)),
             ("rows", dict(d_prior_llr_rows=d_l0.data_ptr(), d_cost_rows=d_cost.data_ptr())))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ref = None
    for name, extra in calls:
        dec.decode_batch_device(*common, **extra)  # warm-up: workspaces, the kernels' first launch
        dec.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            dec.decode_batch_device(*common, **extra)
        dec.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        out = d_out.cpu().numpy()
        if name == "prior_select":
            ref = out
        elif name == "rows":
            agree = float((out == ref).all(axis=1).mean())
            name = f"rows (agrees with prior_select on {agree:.4f} of the shots)"
        inst = dec.last_instance()
        say(f"device-resident {name}: {B / dt:,.0f} syndromes/s ({dt * 1e3:.2f} ms per call of {B}; {inst['bp'][0]}{inst['bp'][1]}, {inst['osd'][0]}; "
            f"{int((d_conv == 0).sum())} shots through OSD)")

    k = a.loop_shots
    one = BpOsdDecoder(H, **kw)
    one.update_channel_probs(P[0])
    one.decode(S[0])
    t0 = time.perf_counter()
    for b in range(k):
        one.update_channel_probs(P[b])
        one.decode(S[b])
    dt = time.perf_counter() - t0
    say(f"update_channel_probs + decode, shot by shot: {k / dt:,.0f} syndromes/s ({dt / k * 1e6:.0f} us per shot, {k} shots)")

    host = BpOsdDecoder(H, **kw)
    host.decode_batch(S, want_osd0=False, want_bp=False, channel_probs_rows=P)  # warm-up: staging and output buffers
    t0 = time.perf_counter()
    got = host.decode_batch(S, want_osd0=False, want_bp=False, channel_probs_rows=P)
    dt = time.perf_counter() - t0
    say(f"host-pointer rows call: {B / dt:,.0f} syndromes/s ({dt * 1e3:.0f} ms per call of {B}; agrees with prior_select on "
        f"{float((got == ref).all(axis=1).mean()):.4f} of the shots)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
