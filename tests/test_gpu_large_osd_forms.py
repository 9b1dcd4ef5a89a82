"""osd_large_kernel<RPT> on every panel form and at the limits of its shape window, against the CPU oracle (run with -m gpu
on an MI355X).

The panel phase of the HBM-resident OSD kernel picks one of six forms from the length of the panel's list of non-zero rows
-- a property of the data, which ``last_instance()`` cannot name.  The matrices of tests/large_osd_cases.py PANEL_CASES fix
OSD's column order through the channel (one min-sum iteration scaled by 2**-20 leaves the prior order standing) and are
built so that every panel's list has a designed length: 128 / 129, 256 / 257, 512 / 513, 1024 / 1025 and 2048 / 2049 rows,
in Gaussian (osd_0, osd_e) and in Gauss-Jordan mode (osd_cs), for every RPT, at m = 8192 / 8193 and m = 16384.
Panels of every form find fewer than 64 pivots (columns that are sums of two others), so that a pivot's ordinal is not its
column, and four matrices complete their rank in the middle of a panel.  tests/test_large_osd_cpu.py proves the lengths, the
pivots per panel and the order without a GPU.  Every output and every LLR bit equals the
oracle's; uniformly random syndromes, outside the column space of these tall matrices, are held to the contract of
tests/gpu_contract.py.  Two matrices are also decoded with a channel per shot that reorders whole panels, so that a form
is met with any number of groups open.

LIMIT_CASES: n = 8192 / 8193 and 16384 / 16385 (the sort sizes 8192 -> 16384 -> 32768 and the cross-block passes of
osdl_sort), n = 32767, RPT 16 on a square-ish matrix, and the refusals one past m = 16384 and n = 32767."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import large_osd_cases as lc
from tests.gpu_contract import check_outside_column_space
from tests.test_gpu_parity import _compare_exact, _gpu_decode

pytestmark = pytest.mark.gpu

PANEL_RUNS = [(c["id"], method, order) for c in lc.PANEL_CASES for method, order in c["runs"]]
LIMIT_RUNS = [(c["id"], method, order) for c in lc.LIMIT_CASES for method, order in c["runs"]]
ANYDEG = ("bp_anydeg_kernel", (), False)


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


def _rows(r, sl):
    return {k: (v[sl] if v is not None else None) for k, v in r.items() if k != "rank"}


def _same_again(g, syn, got, **kw):
    osdw = g.decode_batch(syn, want_osd0=True, want_bp=True, want_llr=True, **kw)
    again = dict(osdw=osdw, osd0=g.batch_osd0, bp=g.batch_bp, converged=g.batch_converge, iters=g.batch_iter, llr=g.batch_llr)
    for k in ("osdw", "osd0", "bp", "converged", "iters"):
        assert (again[k] == got[k]).all(), f"{k} differs between two decodes of the same batch"
    assert (again["llr"].view(np.uint64) == got["llr"].view(np.uint64)).all(), "LLR bits differ between two decodes"


def _packed_equals(g, syn, got, osd):
    B, n = len(syn), g.n
    wn = (n + 63) // 64
    osdw, osd0, bp = (np.empty((B, wn), np.uint64) for _ in range(3))
    conv, iters = np.empty(B, np.uint8), np.empty(B, np.int32)
    g.decode_batch_packed_into(g.pack_rows(syn), osdw, osd0, bp, conv, iters)
    # (bp_anydeg_kernel takes byte rows, so the host API packs and unpacks around the PACKED = false instances; the
    # PACKED = true instance of osd_large_kernel is met in tests/test_gpu_edges.py)
    assert g.last_instance()["osd"] == osd + (False,) and g.last_instance()["bp"] == ANYDEG, g.last_instance()
    for words, rows in ((osdw, got["osdw"]), (osd0, got["osd0"]), (bp, got["bp"])):
        assert (g.unpack_rows(words, n) == rows).all()
    assert (conv.astype(bool) == got["converged"]).all() and (iters == got["iters"]).all()


@pytest.mark.parametrize("run", PANEL_RUNS, ids=[f"{i}-{m}{o}" for i, m, o in PANEL_RUNS])
def test_panel_forms_vs_oracle(gpu_ready, run):
    from bp_osd_amd import BpOsdDecoder
    from oracle import OracleDecoder

    case_id, method, order = run
    case = lc.PANEL_BY_ID[case_id]
    H, _ = lc.panel_pcm(case_id)
    syn, c = lc.run_syndromes(case_id, method, order)
    kw = lc.settings(case, method, order)
    ref = lc.reference(case_id, method, order)
    g = BpOsdDecoder(H, **kw)
    assert g.rank == int(ref["rank"])  # (the kernel's own probe run at creation)
    got = _gpu_decode(g, np.array(syn))
    inst = g.last_instance()
    osd = ("osd_large_kernel", (lc.rpt_of(H.shape[0]),))
    assert inst["bp"] == ANYDEG and inst["osd"] == osd + (False,), inst
    assert (~got["converged"]).sum() == len(syn) - 1, "every shot but the zero one goes to OSD"
    _compare_exact(_rows(got, slice(0, c)), _rows(ref, slice(0, c)))
    if len(syn) > c:  # outside the column space: BP exact, OSD by the contract
        bad = check_outside_column_space(H, OracleDecoder(H, **kw), syn, got, ref, c)
        assert bad.all(), "a random syndrome of a tall rank-deficient matrix inside the column space"
    _same_again(g, np.array(syn), got)
    if case.get("packed"):
        _packed_equals(g, np.array(syn), got, osd)


@pytest.mark.parametrize("case_id", [c["id"] for c in lc.PANEL_CASES if c["rows"]])
def test_panel_order_per_shot_vs_oracle(gpu_ready, case_id):
    """Every shot's channel sorts the panels into an order of its own (tests/large_osd_cases.py shot_orders): the oracle,
    shot by shot with update_channel_probs, is the reference."""
    from bp_osd_amd import BpOsdDecoder

    case = lc.PANEL_BY_ID[case_id]
    H, _ = lc.panel_pcm(case_id)
    P, S = lc.rows_inputs(case_id)
    ref = lc.rows_reference(case_id)
    g = BpOsdDecoder(H, **lc.settings(case, *case["rows"]))
    kw = dict(channel_probs_rows=np.array(P))
    osdw = g.decode_batch(np.array(S), want_osd0=True, want_bp=True, want_llr=True, **kw)
    got = dict(osdw=osdw, osd0=g.batch_osd0, bp=g.batch_bp, converged=g.batch_converge, iters=g.batch_iter, llr=g.batch_llr)
    inst = g.last_instance()
    assert inst["bp"] == ANYDEG and inst["osd"] == ("osd_large_kernel", (lc.rpt_of(H.shape[0]),), False), inst
    assert not got["converged"].any()
    _compare_exact(got, ref)
    assert got["llr"] is not None and len(got["osdw"]) == len(S) == lc.ROWS_SHOTS
    _same_again(g, np.array(S), got, **kw)


@pytest.mark.parametrize("run", LIMIT_RUNS, ids=[f"{i}-{m}{o}" for i, m, o in LIMIT_RUNS])
def test_shape_limits_vs_oracle(gpu_ready, run):
    from bp_osd_amd import BpOsdDecoder

    case_id, method, order = run
    case = lc.LIMIT_BY_ID[case_id]
    H = lc.limit_pcm(case_id)
    syn = np.array(lc.limit_run_syndromes(case_id, method))
    ref = lc.limit_reference(case_id, method, order)
    g = BpOsdDecoder(H, osd_method=method, osd_order=order, **lc.LIMIT_SETTINGS)
    assert g.rank == int(ref["rank"])
    got = _gpu_decode(g, syn)
    inst = g.last_instance()
    osd = ("osd_large_kernel", (lc.rpt_of(case["m"]),))
    assert inst["bp"] == lc.limit_bp_instance(H) + (False,) and inst["osd"] == osd + (False,), inst
    assert not got["converged"].any()
    _compare_exact(got, _rows(ref, slice(None)))
    _same_again(g, syn, got)
    if case["packed"]:
        _packed_equals(g, syn, got, osd)


def test_refusals_one_past_the_last_shape(gpu_ready):
    """m = 16385 and n = 32768 are refused with the limits named; 16384 x 744 (rpt16_m16384) and 1100 x 32767 (wide_n32767)
    are taken: the tests above decode them."""
    from bp_osd_amd import BpOsdDecoder

    def thin(m, n):  # row i holds columns i mod n and (i + 1) mod n
        r = np.repeat(np.arange(m), 2)
        cidx = (r + np.tile([0, 1], m)) % n
        return sp.csr_matrix((np.ones(2 * m, np.uint8), (r, cidx)), shape=(m, n))

    kw = dict(error_rate=0.05, max_iter=2, bp_method="ms", osd_method="osd_0", osd_order=0)
    for m, n in ((16385, 616), (1100, 32768), (16385, 32768)):
        with pytest.raises(ValueError, match=r"limits 16384 / 32767"):
            BpOsdDecoder(thin(m, n), **kw)
