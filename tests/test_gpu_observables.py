"""Decode straight to logical observables (``decode_batch_observables`` and the entry points behind it) against the oracle.

The cases are those of tests/channel_rows_cases.py -- every producer of rows: bp_kernel pairs, any-degree and serial (byte
rows), class, both HBM-resident BP forms, osd_kernel, osd_large_kernel, bp_local_kernel at both strides; n % 64 in
{0, 2, 16, 44, 58} and n % 8 != 0 -- decoded on the constructor channel.  The reference is ``(oracle_rows @ L.T) & 1`` in numpy
(tests/observables_cases.py); tests/test_observables_cpu.py asserts on the oracle that the three row sets differ in their
observables, so a kernel that mixes them up cannot pass.  Every output is compared exactly and no shot is left out."""
import numpy as np
import pytest

from tests import channel_rows_cases as cr
from tests import observables_cases as oc

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


def _decoder(case, **over):
    from bp_osd_amd import BpOsdDecoder

    g = BpOsdDecoder(cr.matrix(case["code"]), **cr.settings(case, **over))
    g.set_osd_variant(cr.osd_variant(case))
    return g


def _n(case):
    return cr.matrix(case["code"]).shape[1]


def _got(g, obs):
    return dict(osdw=obs, osd0=g.batch_obs_osd0, bp=g.batch_obs_bp, converged=g.batch_converge, iters=g.batch_iter)


def _same(got, ref, keys=("osdw", "osd0", "bp", "converged", "iters")):
    for key in keys:
        a, b = np.asarray(got[key]), np.asarray(ref[key])
        assert a.shape == b.shape, (key, a.shape, b.shape)
        bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
        assert bad.size == 0, f"{key}: {bad.size} of {len(a)} shots differ, first {bad[:8]}"


def _packed_ref(ref):
    return dict(ref, osdw=oc.pack(ref["osdw"]), osd0=oc.pack(ref["osd0"]), bp=oc.pack(ref["bp"]))


TABLE_CASES = [cr.CASE_BY_ID[i] for i in cr.TABLE_IDS]


@pytest.mark.parametrize("case", TABLE_CASES, ids=list(cr.TABLE_IDS))
def test_observables_vs_oracle(gpu_ready, case):
    _, S = cr.case_inputs(case)
    L = oc.edge_matrix(_n(case), 65)
    ref = oc.reference(case["id"], L)
    g = _decoder(case)
    g.set_observables(L)
    g.decode_batch(S)
    plain_kernel = g.bp_kernel_info()["kernel"]
    got = _got(g, g.decode_batch_observables(S, want_osd0=True, want_bp=True))
    assert g.bp_kernel_info()["kernel"] == plain_kernel != "none"
    assert got["osdw"].dtype == np.uint8 and got["osdw"].shape == (len(S), 65)
    _same(got, ref)
    assert len(got["osdw"]) == len(S) == len(ref["osdw"])
    # osdw alone: the nullable outputs left out
    only = g.decode_batch_observables(S)
    assert g.batch_obs_osd0 is None and g.batch_obs_bp is None
    _same(dict(osdw=only), ref, keys=("osdw",))


@pytest.mark.parametrize("code,ks", [("bp_pair_8_4", (1, 63, 64, 128, 257, 819, 820)), ("reg1025_s1", (1024,)), ("large_n2048_m1000", (4096,))])
def test_observable_counts(gpu_ready, code, ks):
    """k at the word and workgroup edges on n = 620 (10 words), and at the edge of the kernel's 64 KB table budget there: k = 819
    is the largest table kept in LDS (65520 B, with the staged rows more than the 64 KB a kernel gets without asking), k = 820
    the smallest read from global memory; k = 1024 on 33 words (270 KB) and the cap k = 4096 (1 MB) are far beyond it."""
    case = cr.CASE_BY_ID[code]
    _, S = cr.case_inputs(case)
    g = _decoder(case)
    for k in ks:
        L = oc.edge_matrix(_n(case), k)
        ref = oc.reference(code, L)
        g.set_observables(L)
        assert g.num_observables == k
        got = _got(g, g.decode_batch_observables(S, want_osd0=True, want_bp=True))
        _same(got, ref)
        words = g.decode_batch_observables(S, want_osd0=True, want_bp=True, packed=True)
        assert words.dtype == np.uint64 and words.shape == (len(S), (k + 63) // 64)
        _same(_got(g, words), _packed_ref(ref))  # (padding bits zero)


@pytest.mark.parametrize("n", [64, 620, 2050])
def test_rows_entry_both_forms(gpu_ready, n):
    """obs_kernel alone on random rows that no decoder wrote: the byte form and the packed form equal numpy and each other."""
    import torch
    from bp_osd_amd import BpOsdDecoder
    from tests.edge_codes import EDGE_BY_ID, pcm_for

    if n == 64:
        g = BpOsdDecoder(pcm_for(EDGE_BY_ID["osd_kernel_W2_n64"]), error_rate=0.05, bp_method="ms", max_iter=4)
    else:
        g = _decoder(cr.CASE_BY_ID[{620: "bp_pair_8_4", 2050: "reg1025_s1"}[n]])
    assert g.n == n
    k = 65
    L = oc.edge_matrix(n, k)
    g.set_observables(L)
    rng = np.random.default_rng(5)
    for B in (1, 7, 1000):
        rows = (rng.random((B, n)) < 0.5).astype(np.uint8)
        want = oc.pack(oc.observables(rows, L))
        d_bytes = torch.from_numpy(rows).cuda()
        d_words = torch.from_numpy(BpOsdDecoder.pack_rows(rows).view(np.int64)).cuda()
        outs = [torch.full((B, 2), -1, dtype=torch.int64, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        g.observables_device(d_bytes.data_ptr(), B, outs[0].data_ptr(), packed=False, lane=0)
        g.observables_device(d_words.data_ptr(), B, outs[1].data_ptr(), packed=True, lane=g.num_lanes - 1)
        g.synchronize()
        from_bytes, from_words = (o.cpu().numpy().view(np.uint64) for o in outs)
        assert (from_bytes == want).all(), (B, np.nonzero((from_bytes != want).any(axis=1))[0][:8])
        assert (from_words == want).all(), (B, np.nonzero((from_words != want).any(axis=1))[0][:8])
    with pytest.raises(ValueError, match="lane"):
        g.observables_device(d_bytes.data_ptr(), 1, outs[0].data_ptr(), packed=False, lane=g.num_lanes)


@pytest.mark.parametrize("code", ["bp_pair_8_4", "bp_serial_dv8"])
def test_device_entry_over_lanes(gpu_ready, code):
    """Six device-pointer calls -- more than the lanes -- on disjoint slices with buffers of their own, plain device decodes
    in between, one synchronize() at the end.  The syndromes alternate between bytes and packed words: on either code one
    of the two forms is converted on the lane first."""
    import torch
    from bp_osd_amd import BpOsdDecoder

    case = cr.CASE_BY_ID[code]
    _, S = cr.case_inputs(case)
    n, k, per = _n(case), 65, 8
    L = oc.edge_matrix(n, k)
    ref, rows_ref = oc.reference(code, L), cr.uniform_reference(code)
    g = _decoder(case)
    g.set_observables(L)
    assert 6 > g.num_lanes and 6 * per == len(S)
    d_syn = torch.from_numpy(np.array(S)).cuda()
    d_synw = torch.from_numpy(BpOsdDecoder.pack_rows(S).view(np.int64)).cuda()
    obs = {key: torch.full((len(S), 2), -1, dtype=torch.int64, device="cuda") for key in ("osdw", "osd0", "bp")}
    d_conv = torch.full((len(S),), 9, dtype=torch.uint8, device="cuda")
    d_it = torch.full((len(S),), -1, dtype=torch.int32, device="cuda")
    d_rows = torch.full((len(S), n), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for c in range(6):
        lo = c * per
        syn = d_synw[lo:lo + per] if c % 2 else d_syn[lo:lo + per]
        g.decode_observables_device(syn.data_ptr(), per, obs["osdw"][lo:].data_ptr(), obs["osd0"][lo:].data_ptr(), obs["bp"][lo:].data_ptr(),
                                    d_conv[lo:].data_ptr(), d_it[lo:].data_ptr(), packed=bool(c % 2))
        g.decode_batch_device(d_syn[lo:lo + per].data_ptr(), per, d_rows[lo:].data_ptr())
    g.synchronize()
    got = {key: v.cpu().numpy().view(np.uint64) for key, v in obs.items()}
    got.update(converged=d_conv.cpu().numpy().astype(bool), iters=d_it.cpu().numpy())
    _same(got, _packed_ref(ref))
    assert (d_rows.cpu().numpy() == rows_ref["osdw"]).all()
    # osdw alone, and an empty batch
    only = torch.full((len(S), 2), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    g.decode_observables_device(d_syn.data_ptr(), 0, only.data_ptr())
    g.decode_observables_device(d_syn.data_ptr(), len(S), only.data_ptr())
    g.synchronize()
    assert (only.cpu().numpy().view(np.uint64) == oc.pack(ref["osdw"])).all()
    # obs_kernel's own events: there for the lane of an observables call, gone once a plain decode has taken the lane
    lane = g.last_lane
    assert g.obs_kernel_ms(lane) > 0
    g.decode_batch_device(d_syn.data_ptr(), per, d_rows.data_ptr())
    for _ in range(g.num_lanes - 1):
        g.decode_batch_device(d_syn.data_ptr(), per, d_rows.data_ptr())
    with pytest.raises(ValueError, match="no observables call"):
        g.obs_kernel_ms(lane)


@pytest.mark.parametrize("code", ["bp_pair_8_4", "bp_serial_dv8"])
def test_host_stream(gpu_ready, code):
    """Five asynchronous host-pointer calls on page-locked buffers, byte and packed syndromes alternating, then one
    synchronize(); the synchronous call with packed=True and with packed syndromes gives the same words."""
    from bp_osd_amd import BpOsdDecoder

    case = cr.CASE_BY_ID[code]
    _, S = cr.case_inputs(case)
    k = 65
    L = oc.edge_matrix(_n(case), k)
    want = _packed_ref(oc.reference(code, L))
    g = _decoder(case)
    g.set_observables(L)
    B, kw = len(S), (k + 63) // 64
    calls = []
    for c in range(5):
        s = g.pinned_empty(BpOsdDecoder.pack_rows(S).shape, np.uint64) if c % 2 else g.pinned_empty(S.shape, np.uint8)
        s[...] = BpOsdDecoder.pack_rows(S) if c % 2 else S
        out = dict(osdw=g.pinned_empty((B, kw), np.uint64), osd0=g.pinned_empty((B, kw), np.uint64) if c != 3 else None,
                   bp=g.pinned_empty((B, kw), np.uint64) if c != 4 else None, converged=g.pinned_empty((B,), np.uint8),
                   iters=g.pinned_empty((B,), np.int32))
        for a in out.values():
            if a is not None:
                a[...] = 0x5A
        lane = g.decode_batch_observables_into(s, out["osdw"], out["osd0"], out["bp"], out["converged"], out["iters"], wait=False)
        assert lane == c % g.num_lanes
        calls.append(out)
    g.synchronize()
    for out in calls:
        keys = [key for key, a in out.items() if a is not None]
        _same(dict(out, converged=out["converged"].astype(bool)), want, keys=keys)
    assert g.decode_batch_observables_into(np.zeros((0, g.m), np.uint8), np.zeros((0, kw), np.uint64), wait=False) is None
    for syndromes in (S, BpOsdDecoder.pack_rows(S)):
        words = g.decode_batch_observables(syndromes, want_osd0=True, want_bp=True, packed=True)
        _same(_got(g, words), want)


def test_host_chunks_over_lanes(gpu_ready, monkeypatch):
    """The synchronous host-pointer call in ten chunks of five shots (the last one of three): every lane is reused."""
    case = cr.CASE_BY_ID["bp_pair_8_4"]
    _, S = cr.case_inputs(case)
    L = oc.edge_matrix(_n(case), 65)
    g = _decoder(case)
    g.set_observables(L)
    monkeypatch.setenv("BPOSD_HOST_CHUNK", "5")
    got = _got(g, g.decode_batch_observables(S, want_osd0=True, want_bp=True))
    _same(got, oc.reference(case["id"], L))
    assert g.last_timing()["osd_invocations"] == int((~oc.reference(case["id"], L)["converged"]).sum())
    assert g.obs_kernel_ms() > 0  # (summed over the chunks; last_timing ends in front of that kernel)


def test_table_lifecycle_and_errors(gpu_ready):
    import torch
    from bp_osd_amd import _lib

    case = cr.CASE_BY_ID["bp_pair_8_4"]
    _, S = cr.case_inputs(case)
    S8 = np.array(S)
    n, B = _n(case), len(S)
    g = _decoder(case)

    def refused():
        """every decode entry refuses and enqueues nothing: the outputs keep their fill pattern"""
        with pytest.raises(ValueError, match="observables"):
            g.decode_batch_observables(S)
        out = np.full((B, 2), FILL, np.uint64)
        conv = np.full(B, 9, np.uint8)
        for name in ("bposd_decode_batch_observables", "bposd_decode_batch_observables_async"):
            rc = getattr(gpu_ready, name)(g._h, S8.ctypes.data, B, out.ctypes.data, None, None, conv.ctypes.data, None)
            assert rc == _lib.BPOSD_ERR_INVALID and b"observables" in gpu_ready.bposd_last_error(g._h)
        d_syn = torch.from_numpy(S8).cuda()
        d_out = torch.full((B, 2), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(ValueError, match="observables"):
            g.decode_observables_device(d_syn.data_ptr(), B, d_out.data_ptr())
        with pytest.raises(ValueError, match="observables"):
            g.observables_device(d_syn.data_ptr(), 1, d_out.data_ptr(), packed=False, lane=0)
        g.synchronize()
        assert (out == FILL).all() and (conv == 9).all() and (d_out.cpu().numpy() == 7).all()

    refused()  # before set_observables
    L1, L2 = oc.edge_matrix(n, 65), oc.plain_matrix(n, 7)
    g.set_observables(L1)
    _same(_got(g, g.decode_batch_observables(S, want_osd0=True, want_bp=True)), oc.reference(case["id"], L1))
    g.set_observables(L2)  # replaces the table: other k, other rows
    got = _got(g, g.decode_batch_observables(S, want_osd0=True, want_bp=True))
    assert got["osdw"].shape == (B, 7)
    _same(got, oc.reference(case["id"], L2))
    # a required output missing, and a table that does not fit the decoder
    out = np.full((B, 1), FILL, np.uint64)
    assert gpu_ready.bposd_decode_batch_observables(g._h, S8.ctypes.data, B, None, out.ctypes.data, None, None, None) == _lib.BPOSD_ERR_INVALID
    assert (out == FILL).all()
    with pytest.raises(ValueError, match="shape"):
        g.set_observables(oc.plain_matrix(n + 1, 7))
    assert gpu_ready.bposd_set_observables(g._h, None, 4097) == _lib.BPOSD_ERR_INVALID
    _same(_got(g, g.decode_batch_observables(S, want_osd0=True, want_bp=True)), oc.reference(case["id"], L2))  # (still L2)
    g.set_observables(None)  # k = 0 removes it
    assert g.num_observables == 0
    refused()
    # and a plain decode afterwards is the oracle's
    ref = cr.uniform_reference(case["id"])
    osdw = g.decode_batch(S)
    assert (osdw == ref["osdw"]).all() and (g.batch_osd0 == ref["osd0"]).all() and (g.batch_bp == ref["bp"]).all()
    assert (g.batch_converge == np.asarray(ref["converged"]).astype(bool)).all() and (g.batch_iter == ref["iters"]).all()
