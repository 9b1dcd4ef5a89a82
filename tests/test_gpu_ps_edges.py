"""Product-sum on every BP kernel instance against the CPU oracle (run with -m gpu on an MI355X).

Every BP kernel is compiled three times per instance -- min-sum, product-sum in the reference's operation order
(ps_math_form = 0) and product-sum with two divisions per edge (ps_math_form = 1) -- or switches on ps_form at run time;
tests/test_gpu_edges.py pins every instance at the edges of its window with min-sum only.  One parametrized case here per
row of tests/edge_codes.py PS_EDGES: the same matrices (and (3,6)-regular / degree-class codes for the REG and class
instances), both forms against ``OracleDecoder(ps_math = 2 - form)``, without a clip and with one, cut after one to three
iterations (most shots reach OSD) and after twelve (unclipped messages saturate: a check of degree 1 sends log(2 / 0), and
the kernels reach degrees below the template maximum through per-lane predicates and padded slots, which must stay exactly
neutral with +-inf around), and on some rows a per-bit channel, the per-shot two-valued channel and the packed host API.

Per run: ``last_instance()`` names the row's instance; on ALL shots the NaN masks of the LLRs, converged, iters, the BP
decision and every LLR bit that is no NaN -- infinities included -- equal the oracle's; shots in the column space of H whose
LLRs hold no NaN (or nothing else) equal the oracle's on every output; shots outside it keep the OSD contract of
tests/test_gpu_edges.py wherever OSD ran (the oracle's OSD from the GPU's LLRs on the syndrome H x0 returns x0 and the same
osdw); a second decode returns the same.  A shot whose LLRs MIX numbers and NaN has no defined OSD order
(tests/test_gpu_parity.py::test_product_sum_clip_vs_oracle_live): it is left out of the OSD comparison only, must still
reproduce its syndrome where that is possible, and no run may leave out more than 1/8 of its shots, a clipped run none.
What the oracle's own output must show for a run to test anything is edge_codes.ps_oracle_conditions, asserted here and,
without a GPU, in tests/test_ps_edges_cpu.py.  tests/test_gpu_portable_math.py tells a failure of the arithmetic from one
of the message schedule.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.edge_codes import (PS_EDGES, ps_case_id, ps_cases, ps_oracle_conditions, ps_oracle_select, ps_pcm, ps_select,
                              ps_settings)
from tests.test_gpu_edges import _rows, _syndromes
from tests.test_gpu_parity import _compare_exact, _gpu_decode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


def _decode(g, syn, sel=None, alt=None):
    if sel is None:
        return _gpu_decode(g, syn)
    osdw = g.decode_batch(syn, want_osd0=True, want_bp=True, want_llr=True, prior_select=sel, alt_channel_probs=alt)
    return dict(osdw=osdw, osd0=g.batch_osd0, bp=g.batch_bp, converged=g.batch_converge, iters=g.batch_iter, llr=g.batch_llr)


def _bits(llr):
    """LLR doubles as integers, NaN (whose sign and payload are the platform's) as 0."""
    a = np.ascontiguousarray(llr)
    return np.where(np.isnan(a), np.uint64(0), a.view(np.uint64))


def _run(row, case, H, syn, c):
    from bp_osd_amd import BpOsdDecoder
    from oracle import OracleDecoder

    m, n = H.shape
    Hi = sp.csr_matrix(H, dtype=np.int32)
    synd_of = lambda X: (np.asarray(Hi @ X.T.astype(np.int32)) % 2).T
    kw = ps_settings(row, case, n)
    g = BpOsdDecoder(H, ps_math_form=case["form"], **kw)
    if row.get("bp_variant"):
        g.set_bp_variant(row["bp_variant"])
    o = OracleDecoder(H, ps_math=2 - case["form"], **kw)
    sel = alt = None
    if case["kind"] == "select":
        sel, alt = ps_select(row, len(syn), n)
        ref = ps_oracle_select(o, syn, sel, alt)
    else:
        ref = o.decode_batch(syn)
    got = _decode(g, syn, sel, alt)
    inst = g.last_instance()
    assert inst["bp"] == row["bp"] + (False,), inst
    mixed = ps_oracle_conditions(row, case, ref, syn)  # the exclusion cap and the non-triviality of the run
    # all shots: BP itself
    nan = np.isnan(ref["llr"])
    assert (np.isnan(got["llr"]) == nan).all(), "NaN masks of the LLRs differ"
    for k in ("converged", "iters", "bp"):
        assert (np.asarray(got[k]) == np.asarray(ref[k]).astype(got[k].dtype)).all(), k
    assert (_bits(got["llr"]) == _bits(ref["llr"])).all(), "LLR bits differ"
    if case["clip"] > 0:
        assert np.isfinite(got["llr"]).all()
    # in the column space of H (the first c by construction; later ones where the oracle's OSD-0 reproduces the syndrome):
    # every output, unless the LLRs mix numbers and NaN
    in_space = (synd_of(ref["osd0"]) == syn).all(axis=1)
    assert in_space[:c].all()
    full = in_space & ~mixed
    _compare_exact(_rows(dict(got, llr=None), full), _rows(dict(ref, llr=None), full))  # (the LLR bits: above, on all shots)
    excl = in_space & mixed
    assert (synd_of(got["osdw"][excl]) == syn[excl]).all() and (synd_of(got["osd0"][excl]) == syn[excl]).all()
    # beyond the first c: the OSD contract, from the GPU's own LLRs, for every shot that went through OSD (a shot BP converged
    # on returns the BP decision as osd0 and osdw: it is in the column space and was compared in full above; shots with a NaN
    # LLR have no order to check)
    bad = ~(synd_of(got["osd0"]) == syn).all(axis=1)
    assert not bad[:c][~mixed[:c]].any() and not got["converged"][bad].any()
    assert in_space[got["converged"]].all()
    for b in range(c, len(syn)):
        if nan[b].any() or got["converged"][b]:
            continue
        if sel is not None:
            o.update_channel_probs(np.where(sel[b] != 0, alt, np.full(n, kw["error_rate"])))
        x0 = got["osd0"][b]
        r = o.osd((np.asarray(H @ x0.astype(np.int64)) % 2).astype(np.uint8), got["llr"][b])
        assert (r["osd0"] == x0).all(), ("osd0 is no OSD-0 solution of the checks it satisfies", b)
        assert (r["osdw"] == got["osdw"][b]).all(), ("osdw is not the oracle's search from osd0", b)
    again = _decode(g, syn, sel, alt)
    for k in ("osdw", "osd0", "bp", "converged", "iters"):
        assert (again[k] == got[k]).all(), f"{k} differs between two decodes of the same batch"
    assert (_bits(again["llr"]) == _bits(got["llr"])).all(), "LLRs differ between two decodes of the same batch"
    if case["kind"] == "packed":
        B, wn = len(syn), (n + 63) // 64
        osdw, osd0, bp = (np.empty((B, wn), np.uint64) for _ in range(3))
        conv, iters = np.empty(B, np.uint8), np.empty(B, np.int32)
        g.decode_batch_packed_into(g.pack_rows(syn), osdw, osd0, bp, conv, iters)
        assert g.last_instance()["bp"] == row["bp"] + (True,), g.last_instance()
        for words, rows in ((osdw, got["osdw"]), (osd0, got["osd0"]), (bp, got["bp"])):
            assert (g.unpack_rows(words, n) == rows).all(), "the packed host API returns other rows"
        assert (conv.astype(bool) == got["converged"]).all() and (iters == got["iters"]).all()
    inf = np.isinf(ref["llr"]).any(axis=1)
    return dict(excluded=int(mixed.sum()), shots=len(syn), unconverged=int((~got["converged"]).sum()), inf=int(inf.sum()),
                nan=int(nan.any(axis=1).sum()), outside=int((~in_space).sum()))


@pytest.mark.parametrize("row", PS_EDGES, ids=[r["id"] for r in PS_EDGES])
def test_ps_instance_vs_oracle(gpu_ready, row):
    """Every run of the row (edge_codes.ps_cases); a failing run does not hide the ones after it."""
    H = ps_pcm(row)
    syn, c = _syndromes(H, row)
    failures = []
    for case in ps_cases(row):
        try:
            f = _run(row, case, H, syn, c)
            print(f"PS_EDGES {row['id']} {ps_case_id(case)}: {row['bp'][0]}{row['bp'][1]} excluded {f['excluded']}/{f['shots']} "
                  f"unconverged {f['unconverged']} with_inf {f['inf']} with_nan {f['nan']} outside_column_space {f['outside']}")
        except AssertionError as e:
            failures.append(f"{ps_case_id(case)}: {e}")
            print(f"PS_EDGES {row['id']} {ps_case_id(case)}: FAILED {e}")
    assert not failures, "\n".join(failures)

