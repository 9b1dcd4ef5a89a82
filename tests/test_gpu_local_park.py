"""bp_local_kernel's park at drain on the GPU (run with -m gpu on an MI355X): save and restore of a shot, bit for bit.

A device-pointer call whose BP kernel parks runs two launches: the first writes the state of every unfinished shot it
parks into a record (the whole message region of LDS, the mismatch bitmap, per thread the local messages and the decision
mask, the shot and the iteration to go on from) and the continuation restores it.  Whatever a record drops or misplaces
shows as a different iteration count, hard decision or -- for a shot BP gives up on -- a different OSD result, because OSD-0
orders its columns by the restored LLRs.  So this file decodes, in force mode (every shot that reaches its first chunk
boundary parks there: nothing depends on timing), batches whose shots the oracle has decoded beforehand, and compares osdw,
osd0, bp, converged and iters with the oracle's rows and with the same handle in mode never.

The plan is tests/local_park_cases.py (asserted without a GPU by tests/test_local_park_cpu.py): per matrix a pool with a
shot of exactly CH - 1, CH and CH + 1 iterations and one BP gives up on, decoded at max_iter CH - 1, CH (nothing may park),
CH + 1, 2 CH and 2 CH + 8.  Matrices: m = 64 and 65 (one check per thread), m = 128 and 1024 (two checks per thread; no
padding position at 1024), a 2048-position row, the smallest row with a pair loop and a generic wave, H1922 at B = 2048;
each in byte and in packed form.

The record count.  A workgroup that parks leaves the kernel, so a launch writes at most one record per workgroup, and the
continuation decodes whatever the first launch left in the queue.  With more shots than workgroups, how many of the planned
shots meet a workgroup that has not parked yet depends on the order of the tickets: there the count has an upper bound,
planned, and a lower one: every workgroup of the grid draws a ticket, tickets are consecutive and a ticket is always drawn
by a workgroup that has not parked, so every planned shot among the first G batch rows parks, G = the smallest grid a
launch can have (one workgroup per CU, or the batch).  With at most as many shots as the smallest grid (one workgroup per CU) every
ticket is drawn by a workgroup that has not parked, so ``last_parked`` equals the planned count: that is the small batch.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests.local_codes import decoder_settings, row_by_id
from tests.local_park_cases import CH, MAX_ITERS, N_POOL, PARK_ROWS, batch_index, crosses, plan, planned_parks

pytestmark = pytest.mark.gpu
OUTPUTS = ("osdw", "osd0", "bp", "converged", "iters")
B_EXACT = 128  # at most one shot per workgroup of any grid


@pytest.fixture(scope="module")
def gpu_ready():
    import torch

    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0 and torch.cuda.is_available(), "no MI355X visible"
    return torch


def _decode_device(torch, dec, syn, packed):
    """One device-pointer call on buffers of its own; returns (host copies of the five outputs as 0/1 bytes, lane)."""
    B, n = len(syn), dec.n
    dev = torch.device("cuda", 0)
    conv = torch.full((B,), 7, dtype=torch.uint8, device=dev)
    iters = torch.full((B,), -7, dtype=torch.int32, device=dev)
    if packed:
        wpr = (n + 63) // 64
        d_syn = torch.from_numpy(dec.pack_rows(syn).view(np.int64)).to(dev)
        rows = {k: torch.full((B, wpr), -1, dtype=torch.int64, device=dev) for k in ("osdw", "osd0", "bp")}
        dec.decode_batch_device_packed(d_syn.data_ptr(), B, rows["osdw"].data_ptr(), rows["osd0"].data_ptr(), rows["bp"].data_ptr(),
                                       conv.data_ptr(), iters.data_ptr())
    else:
        d_syn = torch.from_numpy(syn).to(dev)
        rows = {k: torch.full((B, n), 9, dtype=torch.uint8, device=dev) for k in ("osdw", "osd0", "bp")}
        dec.decode_batch_device(d_syn.data_ptr(), B, rows["osdw"].data_ptr(), rows["osd0"].data_ptr(), rows["bp"].data_ptr(),
                                conv.data_ptr(), iters.data_ptr(), None)
    lane = dec.last_lane
    dec.synchronize()
    out = {k: v.cpu().numpy() for k, v in rows.items()}
    if packed:
        out = {k: dec.unpack_rows(v.view(np.uint64), n) for k, v in out.items()}
    out["converged"], out["iters"] = conv.cpu().numpy(), iters.cpu().numpy()
    return out, lane


def _assert_equal(got, want, idx, what):
    for key in OUTPUTS:
        w = np.asarray(want[key])
        w = (w[idx] if idx is not None else w).astype(got[key].dtype)
        bad = np.asarray(got[key]) != w
        assert not bad.any(), what + (key, "first at batch row", int(np.argwhere(bad)[0][0]))


@pytest.mark.parametrize("row_id,B", PARK_ROWS, ids=[r for r, _ in PARK_ROWS])
def test_forced_park_against_oracle_and_never(gpu_ready, row_id, B):
    from bp_osd_amd import BpOsdDecoder

    torch = gpu_ready
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    p = plan(row_id)
    with ThreadPoolExecutor(max_workers=len(MAX_ITERS)) as ex:  # (every constructor runs the layout search)
        decs = dict(zip(MAX_ITERS, ex.map(lambda mi: BpOsdDecoder(p["H"], **decoder_settings(p["q"], mi)), MAX_ITERS)))
    for max_iter in MAX_ITERS:
        dec, ref = decs[max_iter], p["refs"][max_iter]
        for nb in (B, B_EXACT):
            idx = batch_index(nb)
            syn = np.ascontiguousarray(p["pool"][idx])
            want = planned_parks(p, nb, max_iter)
            for packed in (False, True):
                what = (row_id, "max_iter", max_iter, "B", nb, "packed" if packed else "bytes")
                dec.set_park("never")
                never, lane = _decode_device(torch, dec, syn, packed)
                assert dec.last_instance()["bp"][0] == "bp_local_kernel", what + (dec.last_instance(),)
                assert dec.last_parked(lane) == 0, what
                _assert_equal(never, ref, idx, what + ("never != oracle",))
                dec.set_park("force")
                forced, lane = _decode_device(torch, dec, syn, packed)
                parked = dec.last_parked(lane)
                print(*what, "planned", want, "parked", parked)
                _assert_equal(forced, ref, idx, what + ("force != oracle",))
                _assert_equal(forced, never, None, what + ("force != never",))
                if nb == B_EXACT or want == 0:
                    assert parked == want, what + ("parked", parked, "planned", want)
                else:
                    floor = int(crosses(ref["iters"][idx[:min(nb, n_cu)]], max_iter).sum())
                    assert 1 <= floor <= parked <= want, what + ("parked", parked, "planned", want, "among the first grid rows", floor)
    assert all(planned_parks(p, B_EXACT, mi) > 0 for mi in MAX_ITERS if mi > CH)


@pytest.mark.parametrize("B", [8192, 40960])
def test_auto_mode_four_calls_on_the_lanes(gpu_ready, B):
    """Four consecutive device calls, no wait in between: from the second on another lane has work in flight and the rule
    lets a call that is not small (40960 shots: two checks per thread; 8192 is a small call and never parks by the rule)
    park when its queue runs dry.  How many shots park is a matter of timing (printed, not asserted: on a given run the
    40960 case may park nothing, and the 8192 case, the size first planned for this test, compares two runs that cannot
    park); the outputs are those of mode never.  What pins the continuation of the two-checks-per-thread PAIRKEY instance
    whatever the timing is the forced test above, on the row with a pair loop."""
    from bp_osd_amd import BpOsdDecoder

    torch = gpu_ready
    p = plan("h1922_hx")
    dec = BpOsdDecoder(p["H"], **decoder_settings(p["q"], MAX_ITERS[-1]))
    assert dec.num_lanes >= 2
    dev = torch.device("cuda", 0)
    n = dec.n
    syn = [torch.from_numpy(np.ascontiguousarray(p["pool"][(batch_index(B) + k) % N_POOL])).to(dev) for k in range(4)]
    results = {}
    for mode in ("never", "auto"):
        dec.set_park(mode)
        outs = [dict(osdw=torch.full((B, n), 9, dtype=torch.uint8, device=dev), osd0=torch.full((B, n), 9, dtype=torch.uint8, device=dev),
                     bp=torch.full((B, n), 9, dtype=torch.uint8, device=dev), converged=torch.full((B,), 7, dtype=torch.uint8, device=dev),
                     iters=torch.full((B,), -7, dtype=torch.int32, device=dev)) for _ in range(4)]
        lanes = []
        for k in range(4):
            o = outs[k]
            dec.decode_batch_device(syn[k].data_ptr(), B, o["osdw"].data_ptr(), o["osd0"].data_ptr(), o["bp"].data_ptr(),
                                    o["converged"].data_ptr(), o["iters"].data_ptr(), None)
            lanes.append(dec.last_lane)
        dec.synchronize()
        print("mode", mode, "lanes", lanes, "parked on each lane's last call", {l: dec.last_parked(l) for l in sorted(set(lanes))})
        results[mode] = [{k: v.cpu().numpy() for k, v in o.items()} for o in outs]
    ref = p["refs"][MAX_ITERS[-1]]
    for k in range(4):
        _assert_equal(results["auto"][k], results["never"][k], None, ("call", k, "auto != never"))
        _assert_equal(results["never"][k], ref, (batch_index(B) + k) % N_POOL, ("call", k, "never != oracle"))
