"""Every kernel instance at the edges of its size window against the CPU oracle (run with -m gpu on an MI355X).

One parametrized case per (instance, edge) of tests/edge_codes.py EDGES: a rank-deficient matrix of the exact shape and
degrees that puts the dispatch on that instance, BP cut after one to three iterations so that most shots reach OSD, and a
batch of syndromes H e, the all-zero syndrome, uniformly random syndromes and the all-ones syndrome.  ``last_instance()``
names the instance the case was written for -- a change of the dispatch rules fails here instead of moving the edge.

Syndromes in the column space of H: every output and every LLR bit equals the oracle's.  Syndromes outside it (most
random ones, the all-ones one always): BP's outputs and LLR bits equal the oracle's, and OSD keeps the contract of
include/bposd_mi355x.h -- an OSD-0 solution x0 that satisfies the checks of the kernel's own pivot rows (which rows those
are is the kernel's choice; the oracle takes the reference's partial pivoting), and the same candidate search as the
oracle's from there: the oracle's OSD on the syndrome H x0, with the GPU's LLRs, returns the same osd0 and osdw.  That
catches a reduced syndrome that counts the unsatisfied checks of the non-pivot rows into the candidate weights.  Every
output is the same on a second decode of the batch, and at the largest n of an instance the packed host API (the
PACKED = true instance) gives the same rows.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.edge_codes import EDGES, edge_pcm, kprime, order_of, pcm_for
from tests.gpu_contract import check_outside_column_space
from tests.test_gpu_parity import _compare_exact, _gpu_decode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


def _syndromes(H, case):
    """(syndromes, c): H e for random e and the all-zero syndrome -- the first c rows, in the column space of H -- then
    uniformly random syndromes and the all-ones one (outside the column space wherever they break one of the sums the
    appended rows are; the all-ones one always does: three rows that sum to zero).  129 rows by default, 2049 with a large
    batch: an odd number, no multiple of the waves of a workgroup."""
    rng = np.random.default_rng(1000 + case["seed"])
    m, n = H.shape
    n_he, n_rand = case.get("shots") or (95, 32)
    if case.get("batch"):
        n_he = case["batch"] + 1 - n_rand - 2
    q = 0.1 if n < 400 else 0.07
    e = (rng.random((n_he, n)) < q).astype(np.uint8)
    he = (np.asarray(sp.csr_matrix(H, dtype=np.int32) @ e.T.astype(np.int32)) % 2).T
    rand = rng.integers(0, 2, size=(n_rand, m))
    rows = [he, np.zeros((1, m), np.int64), rand, np.ones((1, m), np.int64)]
    return np.ascontiguousarray(np.concatenate(rows).astype(np.uint8)), n_he + 1


def _settings(case, n):
    kw = dict(max_iter=1 + case["seed"] % 3, bp_method="ms", ms_scaling_factor=(0.625, 0.0)[case["seed"] % 2],
              osd_method=case["method"], osd_order=order_of(case))
    if case.get("probs") == "channel":
        kw["channel_probs"] = np.random.default_rng(case["seed"]).uniform(0.03, 0.15, size=n)
    else:
        kw["error_rate"] = 0.08
    if "bit_order" in case:
        kw["osd_e_bit_order"] = case["bit_order"]
    if case.get("schedule"):
        kw["schedule"] = case["schedule"]
    return kw


def _rows(r, sl):
    return {k: (v[sl] if v is not None else None) for k, v in r.items()}


@pytest.mark.parametrize("case", EDGES, ids=[c["id"] for c in EDGES])
def test_instance_edge_vs_oracle(gpu_ready, case):
    from bp_osd_amd import BpOsdDecoder
    from oracle import OracleDecoder

    H = pcm_for(case)
    m, n = H.shape
    syn, c = _syndromes(H, case)
    kw = _settings(case, n)
    g = BpOsdDecoder(H, **kw)
    g.set_osd_variant(case["osd_variant"])
    if case.get("bp_variant"):
        g.set_bp_variant(case["bp_variant"])
    o = OracleDecoder(H, **kw)
    assert g.rank == o.rank == n - kprime(case)
    got = _gpu_decode(g, syn)
    inst = g.last_instance()
    assert inst["bp"] == case["bp"] + (False,) and inst["osd"] == case["osd"] + (False,), inst
    assert (~got["converged"]).mean() > 0.5, "the elimination hardly ran"
    ref = o.decode_batch(syn)
    _compare_exact(_rows(got, slice(0, c)), _rows(ref, slice(0, c)))
    # outside the column space: BP exact, OSD by the contract (module docstring; tests/gpu_contract.py)
    bad = check_outside_column_space(H, o, syn, got, ref, c)
    assert bad.sum() >= len(syn) - c - (len(syn) - c) // 2, "too few syndromes outside the column space"
    again = _gpu_decode(g, syn)
    for k in ("osdw", "osd0", "bp", "converged", "iters"):
        assert (again[k] == got[k]).all(), f"{k} differs between two decodes of the same batch"
    if case.get("packed"):
        B, wn = len(syn), (n + 63) // 64
        osdw, osd0, bp = (np.empty((B, wn), np.uint64) for _ in range(3))
        conv, iters = np.empty(B, np.uint8), np.empty(B, np.int32)
        g.decode_batch_packed_into(g.pack_rows(syn), osdw, osd0, bp, conv, iters)
        assert g.last_instance()["osd"] == case["osd"] + (True,), g.last_instance()
        for words, rows in ((osdw, got["osdw"]), (osd0, got["osd0"]), (bp, got["bp"])):
            assert (g.unpack_rows(words, n) == rows).all()
        assert (conv.astype(bool) == got["converged"]).all() and (iters == got["iters"]).all()


def test_order_caps_on_the_small_path(gpu_ready):
    """osd_e 20 and osd_cs 64 are the highest orders the small path takes; 21 and 65 are refused (with n - rank above both,
    so that the cap and not the number of non-pivot columns refuses them)."""
    from bp_osd_amd import BpOsdDecoder

    H = edge_pcm(120, 250, 8, 4, rank_deficit=3, seed=7)
    for method, top in (("osd_e", 20), ("osd_cs", 64)):
        BpOsdDecoder(H, error_rate=0.05, max_iter=2, bp_method="ms", osd_method=method, osd_order=top)
        with pytest.raises(ValueError, match=f"> {top} not supported"):
            BpOsdDecoder(H, error_rate=0.05, max_iter=2, bp_method="ms", osd_method=method, osd_order=top + 1)
