"""Lifetime of what a handle holds (csrc/owned.h): a create that fails at any depth gives everything back and leaves the
library usable, and one handle's buffers grow, are used below their size and grow again -- every output against the oracle."""
import ctypes as C
import gc

import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_gpu_parity import _compare_exact, _syndromes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


def _outputs(dec, osdw):
    return dict(osdw=osdw, osd0=dec.batch_osd0, bp=dec.batch_bp, converged=dec.batch_converge, iters=dec.batch_iter, llr=dec.batch_llr)


def _head(ref, B):
    return {k: v[:B] for k, v in ref.items() if v is not None}


def _create_raw(lib, H, schedule=0, **kw):
    """bposd_create called directly: (return code, handle, bposd_last_error(NULL))."""
    from bp_osd_amd import _lib

    h = sp.csr_matrix(H)
    h.sort_indices()
    indptr, indices = np.ascontiguousarray(h.indptr, np.int32), np.ascontiguousarray(h.indices, np.int32)
    probs = np.full(h.shape[1], kw["error_rate"])
    cfg = _lib.BposdConfig(device=0, bp_method=1, ms_scaling_factor=0.0, max_iter=kw["max_iter"], osd_method=kw["osd_method"],
                           osd_order=kw["osd_order"], schedule=schedule)
    out = C.c_void_p()
    rc = lib.bposd_create(C.byref(cfg), indptr.ctypes.data, indices.ctypes.data, h.shape[0], h.shape[1], probs.ctypes.data, C.byref(out))
    return rc, out, lib.bposd_last_error(None)


def _column9():
    """9 x 12, three ones per row, the first column in every row (bit degree 9: beyond the serial-schedule kernel)."""
    H = np.zeros((9, 12), np.uint8)
    for r in range(9):
        H[r, [0, 1 + r, 1 + (r + 2) % 11]] = 1
    return H


OSD_E, OSD_CS = 2, 3
# (name, matrix, create arguments that fail, environment, return code, creation error, settings of the good decoder)
FAILURES = [
    ("early", "surface", dict(osd_method=OSD_E, osd_order=8), {}, "INVALID",
     b"osd_order 8 exceeds the number of non-pivot columns n - rank = 7", dict(osd_method="osd_e", osd_order=7)),
    ("after_tables", "column9", dict(osd_method=OSD_CS, osd_order=2, schedule=1), {}, "UNSUPPORTED",
     b"serial schedule: bit degree 9 exceeds 8", dict(osd_method="osd_cs", osd_order=2)),
    ("after_rank_probe", "surface", dict(osd_method=OSD_E, osd_order=8), {"BPOSD_FORCE_LARGE_OSD": "1"}, "INVALID",
     b"osd_order 8 exceeds the number of non-pivot columns n - rank = 7", dict(osd_method="osd_e", osd_order=7)),
]


@pytest.mark.parametrize("case", FAILURES, ids=[f[0] for f in FAILURES])
def test_failed_create_gives_everything_back(gpu_ready, surface13, monkeypatch, case):
    """32 creates that fail -- before any table exists, after the tables, after the device rank probe -- return the code and
    the text they always did, a decoder made afterwards on the same code decodes like the oracle, and the device's free
    memory is where it was (the 64 MB margin of test_create_destroy_cycles_release_device_memory)."""
    import torch

    from bp_osd_amd import BpOsdDecoder, _lib
    from oracle import OracleDecoder

    _, which, bad, env, code, text, good = case
    H = sp.csr_matrix(surface13.hz if which == "surface" else _column9())
    q = 0.08 if which == "surface" else 0.2  # (the oracle sends 12 resp. 11 of the 64 shots to OSD)
    base = dict(error_rate=q, max_iter=13)
    kw = dict(base, bp_method="ms", ms_scaling_factor=0, **good)
    _, syn = _syndromes(H, q, 64, 11)

    def good_decode():
        g = BpOsdDecoder(H, **kw)
        out = _outputs(g, g.decode_batch(syn, want_osd0=True, want_bp=True, want_llr=True))
        del g
        gc.collect()
        return out

    good_decode()  # warm: code objects loaded, allocator pools settled
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (read by bposd_create)
    for _ in range(32):
        rc, handle, err = _create_raw(gpu_ready, H, **dict(base, **bad))
        assert rc == getattr(_lib, "BPOSD_ERR_" + code) and not handle.value
        assert err == text
    for k in env:
        monkeypatch.delenv(k)
    got = good_decode()
    ref = OracleDecoder(H, **kw).decode_batch(syn)
    assert not ref["converged"].all(), "no shot reached OSD"
    _compare_exact(got, ref)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 64 * 2**20, f"device memory not returned: {(free0 - free1) / 2**20:.0f} MB after 32 failed creates"


def test_buffers_grow_idle_and_regrow_on_one_handle(gpu_ready, hgp400, monkeypatch):
    """One [[400,16,6]] decoder, chunks of 256: the zero-copy stage (B = 1), twelve chunks in three rounds of the lanes
    (B = 3000: past the stage's 1 MiB, the page-locked OSD lists appear), the stage again, a channel row per shot through the
    stage (B = 2), one chunk (B = 200) and twelve larger ones (B = 3000: the page-locked row block appears, then regrows), the
    asynchronous packed call (B = 512, then 3000), more select calls than lanes (every lane's alternative-channel block is
    made, the first lane's reused), and B = 6000, which regrows every lane buffer after use.  Then chunks of 1024: four
    tapered chunks, one per lane (B = 4096), four equal ones (B = 4095) and the synchronous packed call (B = 4096), each with
    the call's OSD count summed over its chunk records.  Every output of every call, LLR bits included where the entry point
    returns them, equals the oracle's on the same syndromes."""
    import torch

    from bp_osd_amd import BpOsdDecoder
    from oracle import OracleDecoder
    from tests import channel_rows_cases as cr

    monkeypatch.setenv("BPOSD_HOST_CHUNK", "256")  # (read by every host-pointer call)
    H = hgp400.hz
    m, n = H.shape
    q = 0.05
    kw = dict(max_iter=20, bp_method="ms", ms_scaling_factor=0, osd_method="osd_cs", osd_order=10)
    _, S = _syndromes(H, q, 6000, 71)
    ref = OracleDecoder(H, error_rate=q, **kw).decode_batch(S)
    assert (~ref["converged"]).mean() >= 0.1 and not ref["converged"][0]
    # a channel row per shot, eight distinct channels in turn: the reference is update_channel_probs(P[b]), decode S[b]
    rng = np.random.default_rng(4)
    chans = rng.uniform(0.02, 0.12, (8, n))
    P = chans[np.arange(3000) % 8]
    o = OracleDecoder(H, error_rate=q, **kw)
    ref_rows = {k: np.empty_like(v[:3000]) for k, v in ref.items() if v is not None}
    for c in range(8):
        o.update_channel_probs(chans[c])
        r = o.decode_batch(S[c:3000:8])
        for k in ref_rows:
            ref_rows[k][c::8] = r[k]
    assert (~ref_rows["converged"]).mean() >= 0.1 and not ref_rows["converged"][0] and any((ref_rows[k] != ref[k][:3000]).any() for k in ("osdw", "bp", "iters"))

    g = BpOsdDecoder(H, error_rate=q, **kw)

    def plain(B):
        _compare_exact(_outputs(g, g.decode_batch(S[:B], want_osd0=True, want_bp=True, want_llr=True)), _head(ref, B))

    def rows(B):
        got = _outputs(g, g.decode_batch(S[:B], want_osd0=True, want_bp=True, want_llr=True, channel_probs_rows=P[:B]))
        _compare_exact(got, _head(ref_rows, B))

    def packed_async(B):
        wn = (n + 63) // 64
        out = dict(osdw=np.zeros((B, wn), np.uint64), osd0=np.zeros((B, wn), np.uint64), bp=np.zeros((B, wn), np.uint64),
                   conv=np.zeros(B, np.uint8), iters=np.zeros(B, np.int32))
        g.decode_batch_packed_into(g.pack_rows(S[:B]), out["osdw"], out["osd0"], out["bp"], out["conv"], out["iters"], wait=False)
        g.synchronize()
        got = dict(osdw=g.unpack_rows(out["osdw"], n), osd0=g.unpack_rows(out["osd0"], n), bp=g.unpack_rows(out["bp"], n),
                   converged=out["conv"].astype(bool), iters=out["iters"])
        _compare_exact(got, _head(ref, B))

    plain(1)
    plain(3000)
    plain(1)
    rows(2)
    rows(200)
    rows(3000)
    packed_async(512)
    packed_async(3000)

    # the per-shot two-valued channel with everything on the device, two alternative channels in turn
    Bs = 256
    sel = (rng.random((Bs, n)) < 0.2).astype(np.uint8)
    alts = [rng.uniform(0.02, 0.3, n) for _ in range(2)]
    ref_sel = [cr.oracle_rows(H, dict(kw, error_rate=q), np.where(sel != 0, alt, q), S[:Bs]) for alt in alts]
    assert (ref_sel[0]["osdw"] != ref_sel[1]["osdw"]).any()
    d_syn, d_sel = torch.from_numpy(S[:Bs].copy()).cuda(), torch.from_numpy(sel).cuda()
    calls = []
    for _ in range(g.num_lanes + 1):
        d = dict(osdw=torch.zeros((Bs, n), dtype=torch.uint8, device="cuda"), osd0=torch.zeros((Bs, n), dtype=torch.uint8, device="cuda"),
                 bp=torch.zeros((Bs, n), dtype=torch.uint8, device="cuda"), converged=torch.zeros(Bs, dtype=torch.uint8, device="cuda"),
                 iters=torch.zeros(Bs, dtype=torch.int32, device="cuda"), llr=torch.zeros((Bs, n), dtype=torch.float64, device="cuda"))
        calls.append(d)
    torch.cuda.synchronize()
    for k, d in enumerate(calls):
        g.decode_batch_device(d_syn.data_ptr(), Bs, d["osdw"].data_ptr(), d["osd0"].data_ptr(), d["bp"].data_ptr(), d["converged"].data_ptr(),
                              d["iters"].data_ptr(), d["llr"].data_ptr(), d_prior_select=d_sel.data_ptr(), alt_channel_probs=alts[k % 2])
    g.synchronize()
    for k, d in enumerate(calls):
        got = {key: t.cpu().numpy() for key, t in d.items()}
        got["converged"] = got["converged"].astype(bool)
        _compare_exact(got, ref_sel[k % 2])

    plain(6000)

    # chunks of 1024 on the same handle: 4096 shots are one tapered chunk per lane (bounds 0, 1216, 2432, 3456, 4096), 4095
    # four equal ones, one shot short of the taper; a synchronous packed call patches its OSD rows from packed compact copies
    # in every chunk.  The OSD count of the call sums the four chunk records.
    monkeypatch.setenv("BPOSD_HOST_CHUNK", "1024")
    failed = ref["converged"] == 0  # (the oracle's flags are uint8: ~ is no mask)
    taper = [0, 1216, 2432, 3456, 4096]
    assert all(failed[lo:hi].any() for lo, hi in zip(taper, taper[1:])), "a chunk without a shot for OSD"

    def packed_sync(B):
        wn = (n + 63) // 64
        out = dict(osdw=np.zeros((B, wn), np.uint64), osd0=np.zeros((B, wn), np.uint64), bp=np.zeros((B, wn), np.uint64),
                   conv=np.zeros(B, np.uint8), iters=np.zeros(B, np.int32))
        g.decode_batch_packed_into(g.pack_rows(S[:B]), out["osdw"], out["osd0"], out["bp"], out["conv"], out["iters"], wait=True)
        got = dict(osdw=g.unpack_rows(out["osdw"], n), osd0=g.unpack_rows(out["osd0"], n), bp=g.unpack_rows(out["bp"], n),
                   converged=out["conv"].astype(bool), iters=out["iters"])
        _compare_exact(got, _head(ref, B))

    for call, B in ((plain, 4096), (plain, 4095), (packed_sync, 4096)):
        call(B)
        assert g.last_timing()["osd_invocations"] == int(failed[:B].sum())
