"""Rates of the decode to logical observables on [[1922,50]] (hz, min-sum, osd_cs 7, the headline configuration) at
B = 131072 with the code's own k = 50 logical operators (``bp_osd_amd.codes.h1922().lz``).

(a) Device-resident: ``decode_batch_device_packed`` (three packed row sets out) against ``decode_observables_device`` (three
    observable row sets out), alternating, three rounds of ``--steps`` pipelined calls each, in ms per call; obs_kernel's own
    time -- the one launch over three row sets that the call makes -- from the HIP events the library records around it
    (``obs_kernel_ms``), inside those rounds and for a lone call on an idle device; and the same with the kernel's grid held at
    two workgroups per CU (``BPOSD_OBS_WG_PER_CU=2``) instead of as many as are resident.
(b) Host to host: the ``decode_batch_packed_into(wait=False)`` stream against the ``decode_batch_observables_into(wait=False)``
    stream, page-locked buffers, three calls in flight, the same rounds.
Every observables result is checked against ``(rows @ L.T) & 1`` of the packed call's rows.  Prints one line per figure;
``--out FILE`` also writes them there (profiles/observables_rates.txt)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=131072)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from bp_osd_amd import BpOsdDecoder
    from bp_osd_amd.codes import h1922

    code = h1922(compute_logicals=True)
    H, L = code.hz, np.ascontiguousarray(code.lz, dtype=np.uint8)
    m, n = H.shape
    k = L.shape[0]
    B, q = a.batch, 0.05
    wm, wn, kw = (m + 63) // 64, (n + 63) // 64, (k + 63) // 64
    rng = np.random.default_rng(0)
    S = np.empty((B, m), np.uint8)
    for lo in range(0, B, 8192):
        e = rng.random((min(8192, B - lo), n)) < q
        S[lo:lo + 8192] = (np.asarray(H @ e.T.astype(np.int32)) & 1).T
    SW = np.concatenate([BpOsdDecoder.pack_rows(S[lo:lo + 16384]) for lo in range(0, B, 16384)])
    dec = BpOsdDecoder(H, error_rate=q, max_iter=0, bp_method="ms", ms_scaling_factor=0, osd_method="osd_cs", osd_order=7)
    dec.set_observables(L)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/observables_probe.py on one MI355X: [[{n},{k}]] hz, min-sum, osd_cs 7, B = {B}, k = {k} logicals; {a.rounds} rounds of {a.steps} calls, alternating")

    # ---- (a) device-resident
    i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device="cuda")
    d_synw = torch.from_numpy(SW.view(np.int64)).cuda()
    nsl = 2  # calls in flight, as bench.py pipelines its steps
    rows = [dict(osdw=i64(B, wn), osd0=i64(B, wn), bp=i64(B, wn)) for _ in range(nsl)]
    obs = [dict(osdw=i64(B, kw), osd0=i64(B, kw), bp=i64(B, kw)) for _ in range(nsl)]
    d_conv = [torch.empty(B, dtype=torch.uint8, device="cuda") for _ in range(nsl)]
    d_it = [torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(nsl)]
    torch.cuda.synchronize()

    def call_packed(s):
        dec.decode_batch_device_packed(d_synw.data_ptr(), B, rows[s]["osdw"].data_ptr(), rows[s]["osd0"].data_ptr(), rows[s]["bp"].data_ptr(),
                                       d_conv[s].data_ptr(), d_it[s].data_ptr())

    def call_obs(s):
        dec.decode_observables_device(d_synw.data_ptr(), B, obs[s]["osdw"].data_ptr(), obs[s]["osd0"].data_ptr(), obs[s]["bp"].data_ptr(),
                                      d_conv[s].data_ptr(), d_it[s].data_ptr(), packed=True)

    def pipelined(call, kernel_ms=None):
        """ms per call of a.steps calls, nsl in flight; kernel_ms (a list) collects obs_kernel's event time of every call"""
        lanes = [None] * nsl
        t0 = time.perf_counter()
        for i in range(a.steps):
            s = i % nsl
            if lanes[s] is not None:
                dec.synchronize(lanes[s])
                if kernel_ms is not None:
                    kernel_ms.append(dec.obs_kernel_ms(lanes[s]))
            call(s)
            lanes[s] = dec.last_lane
        dec.synchronize()
        dt = (time.perf_counter() - t0) / a.steps * 1e3
        if kernel_ms is not None:
            kernel_ms.extend(dec.obs_kernel_ms(l) for l in lanes if l is not None)
        return dt

    for call in (call_packed, call_obs):  # warm-up: workspaces, the kernels' first launch
        call(0)
        call(1)
        dec.synchronize()
    Lt = torch.from_numpy(L.astype(np.float32)).cuda()

    def device_reference(words):
        w = words.cpu().numpy().view(np.uint64)
        out = np.empty((B, k), np.uint8)
        for lo in range(0, B, 16384):
            r = torch.from_numpy(BpOsdDecoder.unpack_rows(w[lo:lo + 16384], n)).cuda().to(torch.float32)
            out[lo:lo + 16384] = ((r @ Lt.T) % 2).to(torch.uint8).cpu().numpy()
        return out

    want = {key: device_reference(rows[0][key]) for key in ("osdw", "osd0", "bp")}
    same = all((BpOsdDecoder.unpack_rows(obs[0][key].cpu().numpy().view(np.uint64), k) == want[key]).all() for key in want)
    say(f"device-resident observables equal (rows @ L.T) & 1 of the packed call's rows, all three outputs, {B} shots: {same}")
    def lone_kernel_ms():
        call_obs(0)
        dec.synchronize()
        return dec.obs_kernel_ms(dec.last_lane)

    def with_env(name, value, f, *args):
        os.environ[name] = value
        try:
            return f(*args)
        finally:
            del os.environ[name]

    t_rows, t_obs, t_obs2, k_obs, k_obs2 = [], [], [], [], []
    for _ in range(a.rounds):
        t_rows.append(pipelined(call_packed))
        t_obs.append(pipelined(call_obs, k_obs))
        t_obs2.append(with_env("BPOSD_OBS_WG_PER_CU", "2", pipelined, call_obs, k_obs2))
    lone = [lone_kernel_ms() for _ in range(3)]
    lone2 = [with_env("BPOSD_OBS_WG_PER_CU", "2", lone_kernel_ms) for _ in range(3)]
    fmt = lambda v: " / ".join(f"{x:.2f}" for x in v)
    say(f"device-resident decode_batch_device_packed, ms per call: {fmt(t_rows)} ({B / np.mean(t_rows) * 1e3:,.0f} syndromes/s)")
    say(f"device-resident decode_observables_device, ms per call: {fmt(t_obs)} ({B / np.mean(t_obs) * 1e3:,.0f} syndromes/s)")
    say(f"obs_kernel, one launch over three row sets, HIP events: inside those calls mean {np.mean(k_obs):.3f} ms (min {min(k_obs):.3f}, max {max(k_obs):.3f}, "
        f"{len(k_obs)} calls); a lone call on an idle device {fmt(lone)} ms")
    # (inside the calls the event pair also spans the kernel's wait for workgroup slots next to the other call's persistent BP
    # grid; the bar takes the smaller figure, the kernel alone)
    spread = max(max(t_rows) - min(t_rows), max(t_obs) - min(t_obs))
    diff, bar = np.mean(t_obs) - np.mean(t_rows), min(np.mean(k_obs), np.mean(lone)) + spread
    say(f"observables call minus packed call: {diff:+.3f} ms; bar = the kernel's own time ({min(np.mean(k_obs), np.mean(lone)):.3f} ms) + the run-to-run "
        f"spread of the rounds ({spread:.3f} ms) = {bar:.3f} ms: {'inside' if diff <= bar else 'OUTSIDE'} the bar")
    say(f"the same with the kernel's grid at 2 workgroups per CU: decode_observables_device {fmt(t_obs2)} ms per call; obs_kernel inside those calls "
        f"mean {np.mean(k_obs2):.3f} ms (min {min(k_obs2):.3f}, max {max(k_obs2):.3f}); a lone call {fmt(lone2)} ms")

    # ---- (b) host to host, streams of asynchronous calls on page-locked buffers
    nsl = 3
    h_synw = dec.pinned_empty((B, wm), np.uint64)
    h_synw[...] = SW
    pk = [dict(osdw=dec.pinned_empty((B, wn), np.uint64), osd0=dec.pinned_empty((B, wn), np.uint64), bp=dec.pinned_empty((B, wn), np.uint64),
               conv=dec.pinned_empty((B,)), iters=dec.pinned_empty((B,), np.int32)) for _ in range(nsl)]
    ob = [dict(osdw=dec.pinned_empty((B, kw), np.uint64), osd0=dec.pinned_empty((B, kw), np.uint64), bp=dec.pinned_empty((B, kw), np.uint64),
               conv=dec.pinned_empty((B,)), iters=dec.pinned_empty((B,), np.int32)) for _ in range(nsl)]
    issue_rows = lambda b: dec.decode_batch_packed_into(h_synw, b["osdw"], b["osd0"], b["bp"], b["conv"], b["iters"], wait=False)
    issue_obs = lambda b: dec.decode_batch_observables_into(h_synw, b["osdw"], b["osd0"], b["bp"], b["conv"], b["iters"], wait=False)

    def stream(issue, bufs):
        ncalls = max(2 * nsl, a.steps)
        lanes = [None] * nsl
        t0 = time.perf_counter()
        for i in range(ncalls):
            s = i % nsl
            if lanes[s] is not None:
                dec.synchronize(lanes[s])
            lanes[s] = issue(bufs[s])
        dec.synchronize()
        return (time.perf_counter() - t0) / ncalls * 1e3

    for issue, bufs in ((issue_rows, pk), (issue_obs, ob)):  # warm-up: the buffers of every lane grow here
        for s in range(nsl):
            issue(bufs[s])
        dec.synchronize()
    same = all((BpOsdDecoder.unpack_rows(ob[0][key], k) == want[key]).all() for key in want) and (ob[0]["iters"] == pk[0]["iters"]).all()
    say(f"host-to-host observables equal the same reference, all three outputs, and the packed stream's iteration counts: {same}")
    s_rows, s_obs = [], []
    for _ in range(a.rounds):
        s_rows.append(stream(issue_rows, pk))
        s_obs.append(stream(issue_obs, ob))
    say(f"host-to-host stream decode_batch_packed_into(wait=False), ms per call: {fmt(s_rows)} ({B / np.mean(s_rows) * 1e3:,.0f} syndromes/s; "
        f"{3 * wn * 8} B per shot down)")
    say(f"host-to-host stream decode_batch_observables_into(wait=False), ms per call: {fmt(s_obs)} ({B / np.mean(s_obs) * 1e3:,.0f} syndromes/s; "
        f"{3 * kw * 8} B per shot down)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
