"""What a decode must keep for syndromes outside the column space of H, where OSD has no solution to return.

BP's outputs and LLR bits equal the oracle's, and OSD keeps the contract of include/bposd_mi355x.h: an OSD-0 solution x0
that satisfies the checks of the kernel's own pivot rows (which rows those are is the kernel's choice; the oracle takes the
reference's partial pivoting), and the same candidate search as the oracle's from there -- the oracle's OSD on the syndrome
H x0, with the GPU's LLRs, returns the same osd0 and osdw.  That catches a reduced syndrome that counts the unsatisfied
checks of the non-pivot rows into the candidate weights.  Shared by tests/test_gpu_edges.py and
tests/test_gpu_large_osd_forms.py."""
import numpy as np
import scipy.sparse as sp


def check_outside_column_space(H, o, syn, got, ref, c):
    """Rows c.. of a decode (``got``: the GPU's outputs, ``ref``: the oracle's, ``o``: the oracle decoder with the same
    settings) by the contract above.  Returns the mask, over those rows, of the syndromes that osd0 does not reproduce."""
    bad = ((np.asarray(sp.csr_matrix(H, dtype=np.int32) @ got["osd0"][c:].T.astype(np.int32)) % 2).T != syn[c:]).any(axis=1)
    for k in ("converged", "iters", "bp"):
        assert (np.asarray(got[k][c:]) == np.asarray(ref[k][c:]).astype(got[k].dtype)).all(), k
    assert (got["llr"][c:].view(np.uint64) == ref["llr"][c:].view(np.uint64)).all(), "LLR bits differ"
    assert not got["converged"][c:][bad].any()
    for b in range(c, len(syn)):
        x0 = got["osd0"][b]
        r = o.osd((np.asarray(H @ x0.astype(np.int64)) % 2).astype(np.uint8), got["llr"][b])
        assert (r["osd0"] == x0).all(), ("osd0 is no OSD-0 solution of the checks it satisfies", b)
        assert (r["osdw"] == got["osdw"][b]).all(), ("osdw is not the oracle's search from osd0", b)
    return bad
