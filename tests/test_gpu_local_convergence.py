"""The exits of bp_local_kernel's iteration loops, pinned against the oracle (the GPU tests run with -m gpu on an MI355X).

Every wave of bp_local_kernel reads the whole mismatch bitmap (MP / 64 b64 words, one per lane) at the top of an iteration
and leaves on its own when it is zero; the same test runs once more after the last bit pass.  What can go wrong is an exit:
one iteration early or late, a wave that disagrees with the others, a bitmap that carries a bit over from the syndrome the
workgroup decoded before.  So this file decodes syndromes whose iteration counts the oracle has fixed beforehand.

The plan of a matrix (``plan``: tests/bp_exit_cases.py ``plan_for``, shared with the other BP families' test
tests/test_gpu_bp_exits.py; CPU only, asserted by ``test_oracle_alone_produces_every_case`` without a GPU):
- a pool of syndromes: the all-zero one (iters = 0), H e for one error of weight 1 (min-sum flips that bit in the first
  iteration: iters = 1), and H e for 30 random errors of the row's rate q;
- the *target*: the pool row the oracle converges in the fewest iterations k >= 3 at max_iter 30;
- the pool decoded by the oracle with max_iter k + 1 (the target converges inside the loop), k (it converges in the last
  iteration: the test after the last bit pass), k - 1 (it misses by one: iters = max_iter, OSD takes it) and 1.
``CASES`` names what must occur; the plan asserts each on the oracle's results, the GPU test on the kernel's.

The batch repeats the pool in order, with the target, the zero syndrome and the one-iteration syndrome at its first and last
three indices.  It is larger than the grid (at most 1024 workgroups), so a workgroup takes converged, missed and ordinary
syndromes one after the other from the queue and reuses its bitmap.  The whole batch is compared bit for bit with the
oracle's rows: converged, iters, bp, osd0, osdw, and the LLR bit patterns where LLRs are asked for.

Matrices, from tests/local_codes.py (tests/test_local_codes_cpu.py pins their wave tables):
- 1024 positions: the smallest row with a pair loop and a generic wave (16 bitmap words);
- 2048 positions: ``reg1900_s3`` (32 bitmap words; pair loop, two generic waves, a padding-only group);
- the window edges m = 64 and m = 65: one and two bitmap words with a set bit at all, padding-only groups.
Batches: 2051 syndromes (at most 40000: one check per thread, ``<1, 1024, 8>``) and 40003 (two checks per thread).  The
2048-position kernel has the one shape ``<2, 2048, 4>`` at every batch size and runs the small batch (1031) only.  Forms:
LLRs asked for (the LLR loop runs every iteration), not asked for (keyed, pair and generic loops, the LLR loop in the last
iteration) and packed I/O.
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests.bp_exit_cases import CASES, N_POOL, _occurred, batch_index, plan_for
from tests.local_codes import LOCAL_CODES, decoder_settings, matrix_of, row_by_id, syndrome_seed
from tests.test_gpu_local_bodies import FORMS, OUTPUTS, _decode, _expected_local


def _row_1024():
    rows = [r for r in LOCAL_CODES if r["MP"] == 1024 and r["pairkey"] >= 0 and r["generic"] >= 1]
    return min(rows, key=lambda r: r["m"])["id"]  # (the first of equal m)


ROW_IDS = (_row_1024(), "reg1900_s3", "reg64_s1", "reg65_s1")
B_ONE_CHECK = {1024: 2048 + 3, 2048: 1024 + 7}  # a few syndromes per workgroup (grids of 512 and 256); odd
B_TWO_CHECKS = 40000 + 3  # just above the small-call threshold (launch_bp_local.hip)
GPU_CASES = [(rid, "small") for rid in ROW_IDS] + [(rid, "large") for rid in ROW_IDS if row_by_id(rid)["MP"] == 1024]


@functools.lru_cache(maxsize=None)
def plan(row_id):
    """The plan of a LOCAL_CODES row (tests/bp_exit_cases.py plan_for): dict(H, q, pool, target, k, max_iters, refs
    {max_iter: the oracle's result for the pool}); see the module docstring."""
    row = row_by_id(row_id)
    kw = decoder_settings(row["q"], 0)
    del kw["max_iter"]
    return plan_for(matrix_of(row), kw, row["q"], syndrome_seed(row), what=(row_id,))


@pytest.mark.parametrize("row_id", ROW_IDS)
def test_oracle_alone_produces_every_case(row_id):
    """No GPU: the plan of every matrix holds all CASES (``plan`` asserts it), with a target of 3 <= k < 30 iterations."""
    p = plan(row_id)
    assert 3 <= p["k"] < 30 and p["max_iters"] == (p["k"] + 1, p["k"], p["k"] - 1, 1)
    idx = batch_index(B_ONE_CHECK[1024], p["target"])
    assert idx[0] == idx[-1] == p["target"] and set(idx) == set(range(N_POOL))


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


def _assert_rows(dec, r, ref, idx, want_llr, packed, what):
    """Batch row i of the kernel's result is the oracle's pool row idx[i], bit for bit."""
    for lo in range(0, len(idx), 8192):
        want = idx[lo:lo + 8192]
        for key in OUTPUTS:
            g = r[key][lo:lo + 8192]
            if packed and key in ("osdw", "osd0", "bp"):
                g = dec.unpack_rows(g, dec.n)
            bad = np.asarray(g) != ref[key][want].astype(np.asarray(g).dtype)
            assert not bad.any(), what + (key, "GPU != oracle, first at batch row", lo + int(np.argwhere(bad)[0][0]))
        if want_llr:
            bad = r["llr"][lo:lo + 8192].view(np.uint64) != ref["llr"][want].view(np.uint64)
            assert not bad.any(), what + ("LLR bits", "GPU != oracle, first at batch row", lo + int(np.argwhere(bad)[0][0]))


@pytest.mark.gpu
@pytest.mark.parametrize("row_id,size", GPU_CASES, ids=[f"{r}-{s}" for r, s in GPU_CASES])
def test_exits_against_oracle(gpu_ready, row_id, size):
    """One matrix at one batch size: max_iter k + 1, k, k - 1 and 1, each with LLRs, without and packed."""
    from bp_osd_amd import BpOsdDecoder

    row, p = row_by_id(row_id), plan(row_id)
    B = B_ONE_CHECK[row["MP"]] if size == "small" else B_TWO_CHECKS
    idx = batch_index(B, p["target"])
    syn = np.ascontiguousarray(p["pool"][idx])
    with ThreadPoolExecutor(max_workers=4) as ex:  # (every constructor runs the layout search)
        decs = dict(zip(p["max_iters"], ex.map(lambda mi: BpOsdDecoder(p["H"], **decoder_settings(p["q"], mi)), p["max_iters"])))
    seen = set()
    for max_iter in p["max_iters"]:
        dec, ref = decs[max_iter], p["refs"][max_iter]
        for form, want_llr, packed in FORMS:
            what = (row_id, size, max_iter, form)
            r = _decode(dec, syn, want_llr, packed)
            inst, pk = _expected_local(row, B, True, packed)
            assert dec.last_instance()["bp"] == inst and dec.last_pair_key() == pk, what + (dec.last_instance(), dec.last_pair_key())
            _assert_rows(dec, r, ref, idx, want_llr, packed, what)
            # the cases, read from the kernel's own result at one place of each pool row (the last repetition of the pool)
            at = np.array([np.flatnonzero(idx == i)[-1] for i in range(N_POOL)])
            got = _occurred(dict(converged=r["converged"][at], iters=r["iters"][at]), p["target"], p["k"], max_iter)
            assert got == _occurred(ref, p["target"], p["k"], max_iter), what
            seen |= got
    assert seen == set(CASES), (row_id, size, "not exercised", sorted(set(CASES) - seen))
