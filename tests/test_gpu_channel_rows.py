"""A channel of its own for every shot (``decode_batch(S, channel_probs_rows=P)``) against the oracle used the documented
way: ``update_channel_probs(P[b])``, then decode ``S[b]``, shot by shot.

The cases (tests/channel_rows_cases.py) reach every BP family, osd_kernel, osd_large_kernel, and the LDS-resident and the
HBM-resident BP; tests/test_channel_rows_cpu.py asserts on the oracle that their shots differ from the uniform-channel
decode and mix converged with non-converged shots.  Every output and every LLR bit must equal the oracle's, no shot is
left out, and ``last_instance()`` must name the instance the case was chosen for."""
import numpy as np
import pytest

from tests import channel_rows_cases as cr
from tests.test_gpu_parity import _compare_exact

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


def _outputs(dec, osdw):
    return dict(osdw=osdw, osd0=dec.batch_osd0, bp=dec.batch_bp, converged=dec.batch_converge, iters=dec.batch_iter, llr=dec.batch_llr)


def _decode(dec, S, **kw):
    return _outputs(dec, dec.decode_batch(S, want_osd0=True, want_bp=True, want_llr=True, **kw))


def _same(a, b):
    _compare_exact(a, b)
    assert b.get("llr") is not None and a.get("llr") is not None


def _decoder(case, **over):
    from bp_osd_amd import BpOsdDecoder

    g = BpOsdDecoder(cr.matrix(case["code"]), **cr.settings(case, **over))
    g.set_osd_variant(cr.osd_variant(case))
    return g


@pytest.mark.parametrize("case", cr.CASES, ids=[c["id"] for c in cr.CASES])
def test_rows_vs_oracle_shot_by_shot(gpu_ready, case):
    P, S = cr.case_inputs(case)
    g = _decoder(case)
    got = _decode(g, S, channel_probs_rows=P)
    inst = g.last_instance()
    bp, osd = cr.expected_instances(case)
    ref = cr.reference(case["id"])
    assert inst["bp"] == bp, inst
    if not ref["converged"].all():  # (the OSD kernel is launched for non-converged shots only)
        assert inst["osd"] == osd, inst
    if cr.is_local(case):
        assert g.last_pair_key() == -1
    _same(got, ref)
    assert len(got["osdw"]) == len(S) == len(ref["osdw"])


@pytest.mark.parametrize("code", ["bp_pair_8_4", "bp_class_mp256_m170"])
@pytest.mark.parametrize("form", [0, 1])
def test_rows_product_sum_vs_oracle(gpu_ready, code, form):
    """Product-sum in both evaluation orders, clipped at 20: every prior is finite and every message clipped, so all shots
    compare exactly (the oracle's matching ps_math is 2 - form, as in tests/test_gpu_ps_edges.py)."""
    case = cr.CASE_BY_ID[code]
    P, S = cr.case_inputs(case)
    over = dict(bp_method="ps", ps_clip=20.0)
    g = _decoder(case, ps_math_form=form, **over)
    got = _decode(g, S, channel_probs_rows=P)
    assert g.last_instance()["bp"] == cr.expected_instances(case)[0], g.last_instance()
    ref = cr.oracle_rows(cr.matrix(code), cr.settings(case, ps_math=2 - form, **over), P, S)
    assert np.isfinite(ref["llr"]).all()
    _same(got, ref)


def test_rows_equivalences(gpu_ready):
    from oracle import OracleDecoder

    case = cr.CASE_BY_ID["bp_pair_8_4"]
    P, S = cr.case_inputs(case)
    B, n = P.shape
    q = cr.case_q(case)
    g = _decoder(case)
    plain = _decode(g, S)
    # rows all equal to the ctor channel
    _same(_decode(g, S, channel_probs_rows=np.full((B, n), q)), plain)
    # rows = where(sel, alt, base)
    rng = np.random.default_rng(8)
    sel = (rng.random((B, n)) < 0.25).astype(np.uint8)
    alt = rng.uniform(0.02, 0.3, n)
    want = _decode(g, S, prior_select=sel, alt_channel_probs=alt)
    _same(_decode(g, S, channel_probs_rows=np.where(sel != 0, alt, q)), want)
    assert any((want[k] != plain[k]).any() for k in ("osdw", "bp", "iters")), "the select call changed nothing"
    # a rows call in between leaves the handle's own channel and its alternative channel alone
    _decode(g, S, channel_probs_rows=P)
    _same(_decode(g, S), OracleDecoder(cr.matrix(case["code"]), **cr.settings(case)).decode_batch(S))
    _same(_decode(g, S), plain)


@pytest.mark.parametrize("osd", [("osd_cs", 6), ("osd0", 0)])
def test_rows_device_pointer_entry(gpu_ready, osd):
    import torch
    from bp_osd_amd import BpOsdDecoder

    case = cr.CASE_BY_ID["bp_pair_8_4"]
    P, S = cr.case_inputs(case)
    B, n = P.shape
    over = dict(osd_method=osd[0], osd_order=osd[1])
    host = _decode(_decoder(case, **over), S, channel_probs_rows=P)
    g = _decoder(case, **over)
    llr_rows, cost_rows = BpOsdDecoder.channel_tables(P)
    assert llr_rows.shape == cost_rows.shape == (B, n)
    d_syn = torch.from_numpy(np.array(S)).cuda()
    d_l0, d_cost = torch.from_numpy(llr_rows).cuda(), torch.from_numpy(cost_rows).cuda()
    runs = [d_cost.data_ptr()] if osd[0] != "osd0" else [d_cost.data_ptr(), None]  # (without weights only where OSD does not weigh)
    for cost_ptr in runs:
        d_w, d_0, d_bp = (torch.zeros((B, n), dtype=torch.uint8, device="cuda") for _ in range(3))
        d_conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
        d_it = torch.zeros(B, dtype=torch.int32, device="cuda")
        d_llr = torch.zeros((B, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        g.decode_batch_device(d_syn.data_ptr(), B, d_w.data_ptr(), d_0.data_ptr(), d_bp.data_ptr(), d_conv.data_ptr(), d_it.data_ptr(),
                              d_llr.data_ptr(), d_prior_llr_rows=d_l0.data_ptr(), d_cost_rows=cost_ptr)
        g.synchronize()
        dev = dict(osdw=d_w.cpu().numpy(), osd0=d_0.cpu().numpy(), bp=d_bp.cpu().numpy(), converged=d_conv.cpu().numpy().astype(bool),
                   iters=d_it.cpu().numpy(), llr=d_llr.cpu().numpy())
        _same(dev, host)
    if osd[0] != "osd0":  # the weights are required where OSD ranks its candidates with them
        with pytest.raises(ValueError, match="cost_rows"):
            g.decode_batch_device(d_syn.data_ptr(), B, d_w.data_ptr(), d_prior_llr_rows=d_l0.data_ptr())
    with pytest.raises(ValueError):
        g.decode_batch_device(d_syn.data_ptr(), B, d_w.data_ptr(), d_prior_llr_rows=d_l0.data_ptr(), d_cost_rows=d_cost.data_ptr(),
                              d_prior_select=d_syn.data_ptr(), alt_channel_probs=np.full(n, 0.1))
    with pytest.raises(ValueError):
        g.decode_batch_device(d_syn.data_ptr(), B, d_w.data_ptr(), d_cost_rows=d_cost.data_ptr())


def test_rows_argument_errors(gpu_ready):
    from bp_osd_amd import _lib

    case = cr.CASE_BY_ID["bp_pair_8_4"]
    P, S = cr.case_inputs(case)
    B, n = P.shape
    g = _decoder(case)
    for bad_shape in (P[:-1], P[:, :-1], P[0]):
        with pytest.raises(ValueError, match="shape"):
            g.decode_batch(S, channel_probs_rows=bad_shape)
    for bad in (-0.1, 1.5, np.nan):
        Q = np.array(P)
        Q[5, 17] = bad
        Q[9, 3] = bad  # (the first offending entry is the one named)
        with pytest.raises(ValueError, match=r"channel_probs_rows\[5\]\[17\]"):
            g.decode_batch(S, channel_probs_rows=Q)
    with pytest.raises(ValueError):
        g.decode_batch(S, channel_probs_rows=P, prior_select=np.zeros((B, n), np.uint8), alt_channel_probs=np.full(n, 0.1))
    with pytest.raises(ValueError):
        g.decode_batch(S, channel_probs_rows=P, packed=True)
    # the C entry called directly with a NaN: refused before anything is enqueued, the outputs stay as they were
    Q = np.array(P)
    Q[2, 1] = np.nan
    S8 = np.array(S)
    out = np.full((B, n), 9, np.uint8)
    rc = gpu_ready.bposd_decode_batch_rows(g._h, S8.ctypes.data, B, Q.ctypes.data, out.ctypes.data, None, None, None, None, None)
    assert rc == _lib.BPOSD_ERR_INVALID and (out == 9).all()
    assert b"channel_probs_rows[2][1]" in gpu_ready.bposd_last_error(g._h)
    rc = gpu_ready.bposd_decode_batch_rows(g._h, S8.ctypes.data, B, None, out.ctypes.data, None, None, None, None, None)
    assert rc == _lib.BPOSD_ERR_INVALID
    # and the decoder still works
    _same(_decode(g, S, channel_probs_rows=P), cr.reference(case["id"]))
