"""The plan of tests/test_gpu_local_park.py, shared with tests/test_local_park_cpu.py (which asserts it without a GPU).

bp_local_kernel runs its loops without LLR stores in chunks of CH iterations (csrc/local_park.h).  A shot that starts at
iteration 1 meets its first chunk boundary behind iteration CH, and it meets it only if the chunk was full and the shot is
not finished: max_iter >= CH + 1 (the last iteration is the LLR body's and belongs to no chunk) and no convergence seen
at the top of an iteration <= CH.  The test at the top of iteration it sees the decisions of iteration it - 1, so a shot
the oracle converges in CH - 1 iterations leaves inside the chunk, one it converges in CH iterations reaches the boundary
(and would converge at the first test behind it), and every shot with more iterations reaches it too:

    a shot crosses its first boundary  <=>  max_iter >= CH + 1  and  the oracle's iters >= CH

(a shot BP gives up on has iters = max_iter).  In force mode every such shot that a workgroup of the first launch holds
parks there; the continuation restores it and must end where the oracle ends.

The pool of a matrix (``plan``; CPU only): from seeded ``H e`` candidates at the row's rate q, scanned by the oracle at
max_iter 2 CH + 8 -- the zero syndrome, the first candidates the oracle converges in exactly CH - 1, CH and CH + 1
iterations, the first one it does not converge, and the first ordinary candidates up to N_POOL rows.  The pool is then
decoded by the oracle at max_iter CH - 1 and CH (nothing crosses: the chunk ends at max_iter), CH + 1 (the continuation
enters at max_iter: the LLR body alone), 2 CH (the LLR body's iteration closes the second chunk) and 2 CH + 8 (the three
edge shots converge).  The batch repeats the pool in order.
"""
import functools
import os
import re

import numpy as np

from tests.local_codes import LOCAL_CODES, decoder_settings, matrix_of, row_by_id, syndrome_seed, syndromes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POOL = 32


def chunk():
    """CH, read from the header the kernel and the host share."""
    src = open(os.path.join(ROOT, "bp_osd_amd", "csrc", "local_park.h")).read()
    return int(re.search(r"#define BPOSD_BPL_CH (\d+)", src).group(1))


CH = chunk()
MAX_ITERS = (CH - 1, CH, CH + 1, 2 * CH, 2 * CH + 8)
SCAN = 2 * CH + 8


def _row_pair_and_generic():
    rows = [r for r in LOCAL_CODES if r["MP"] == 1024 and r["pairkey"] >= 0 and r["generic"] >= 1]
    return min(rows, key=lambda r: r["m"])["id"]  # (the first of equal m)


# (row of tests/local_codes.py, batch size).  At most 40000 shots a 1024-position call runs one check per thread
# (<1, 1024, 8>), above it two (<2, 1024, 8>, the PAIRKEY instance where the wave table has a pair loop); the 2048-position
# kernel has one shape.  Two checks per thread therefore need the large batch; the oracle decodes the pool only.
B_ONE, B_TWO, B_2048 = 2048 + 3, 40000 + 3, 1024 + 7
PARK_ROWS = (("reg64_s1", B_ONE), ("reg65_s1", B_ONE), ("reg128_s1", B_TWO), ("reg1024_s7", B_TWO), ("reg1900_s3", B_2048),
             (_row_pair_and_generic(), B_TWO), ("h1922_hx", 2048))


def crosses(iters, max_iter):
    """bool per shot: does it cross its first chunk boundary (module docstring)?"""
    return (np.asarray(iters) >= CH) & (max_iter >= CH + 1)


@functools.lru_cache(maxsize=None)
def plan(row_id):
    """dict(H, q, pool, edge {CH - 1, CH, CH + 1: pool row}, stuck (pool row), refs {max_iter: the oracle's result})."""
    from oracle import OracleDecoder

    row = row_by_id(row_id)
    H, q = matrix_of(row), row["q"]
    # (shots of exactly CH - 1, CH and CH + 1 iterations are a few per thousand: the small matrices and the q = 0.04 ones need more candidates)
    cand = syndromes(H, q, 4096 if (row["m"] <= 128 or q < 0.05) else 1024, syndrome_seed(row))
    kw = decoder_settings(q, SCAN)
    scan = OracleDecoder(H, **kw).decode_batch(cand)
    conv, it = scan["converged"] != 0, scan["iters"]
    he = np.arange(len(cand)) >= 34  # (the candidates in front are the all-ones and uniformly random syndromes)
    picks = [0]
    edge = {}
    for k in (CH - 1, CH, CH + 1):
        hit = np.flatnonzero(he & conv & (it == k))
        assert hit.size, (row_id, "no candidate converges in exactly", k, "iterations")
        edge[k] = len(picks)
        picks.append(int(hit[0]))
    hit = np.flatnonzero(he & ~conv)
    assert hit.size, (row_id, "every candidate converges")
    stuck = len(picks)
    picks.append(int(hit[0]))
    picks += [i for i in np.flatnonzero(he) if i not in picks][:N_POOL - len(picks)]
    pool = np.ascontiguousarray(cand[picks])
    refs = {mi: OracleDecoder(H, **decoder_settings(q, mi)).decode_batch(pool) for mi in MAX_ITERS}
    return dict(H=H, q=q, pool=pool, edge=edge, stuck=stuck, refs=refs)


def batch_index(B):
    return np.arange(B) % N_POOL


def planned_parks(p, B, max_iter):
    """Shots of the batch that cross a boundary, by the oracle alone."""
    return int(crosses(p["refs"][max_iter]["iters"][batch_index(B)], max_iter).sum())
