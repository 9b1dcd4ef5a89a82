"""The loop exits and the workgroup reuse of every BP kernel family but bp_local_kernel, pinned against the oracle (run with
-m gpu on an MI355X).  tests/test_gpu_local_convergence.py does the same for bp_local_kernel.

Every launcher sizes its grid as min(B, CUs x workgroups per CU), and tests/test_gpu_edges.py decodes 129 syndromes at most: there
each workgroup decodes one syndrome and leaves, after 1 to 3 iterations.  Here every row of tests/bp_exit_cases.py EXIT_ROWS --
one per instance of bp_kernel (the five predicated degree pairs, REG at shapes 1, 2 and 4, shape 2 on request, shape 8 at two
pairs), bp_class_kernel (three strides, five degree classes), bp_large_kernel (<12, 6> and <16, 8>, both min-sum forms),
bp_anydeg_kernel and bp_serial_kernel -- decodes a pool of syndromes whose iteration counts the oracle has fixed beforehand
(``plan_for``), repeated to a batch above twice the largest possible grid, so that some workgroup decodes at least three shots:
4101 (a kernel of at least 256 threads: at most 8 workgroups on each of 256 CUs), 8197 for bp_class_kernel (at most 16), and for
the class row with m <= 160 also 65539, where a workgroup takes 8 .. 1 shots per queue atomic.

Per row, all bit for bit against the oracle's pool rows (converged, iters, bp, osd0, osdw, LLR bit patterns), with
``last_instance()`` pinned on every decode:
- max_iter k + 1, k, k - 1 and 1 (k: the iterations of the target) x LLRs / no LLRs / packed; the CASES read from the kernel's
  own result equal the oracle's and are complete.  Catches an exit one iteration early or late at either loop exit, a flag or
  bitmap word carried over from a shot that left at max_iter, hard decisions or message slices carried into the next shot.
  bp_large_kernel rows run it twice: check data in LDS, and whole check records in the workspace (set_bp_variant(63)).
- the adaptive factor past iteration 53: factor 0, max_iter 56, LLRs; some pool row is still unconverged at 56, so its LLRs
  carry the factors of iterations 53 (1 - 2^-53), 54 and later (1.0).
- product-sum (the row's form, a finite clip) with a plan of its own: max_iter k + 1, k, k - 1, LLRs.
- per-shot priors: pool row i always travels with select row i, so a thread that keeps the prior of the shot before fails;
  max_iter k, no LLRs.

OSD.  Rows on osd_kernel decode everything with osd0.  Rows that land on osd_large_kernel (EXIT_ROWS ``large_osd``: m > 1024 or
n > 2047 -- bp_shape1_m1024_n2048_dc16, bp_shape2_m1024_n2048_variant2, bp_shape8_8_4, bp_shape8_6_3 and the three bp_large
rows) decode the big batches with osd_off and add one osd0 decode of the bare pool per max_iter.  No further row was moved to
that scheme.

Wall time per case, measured on an MI355X inside the test (plans on the oracle, constructors, every decode and comparison;
one process per case): 0.3 .. 0.6 s the bp_kernel pair rows, 1.1 s bp_shape1_m1024_n2048_dc16, 1.4 s each REG row, 0.9 s
bp_shape2_m1024_n2048_variant2, 2.8 s bp_shape8_8_4 (2.3 s of it constructors), 1.9 s bp_shape8_6_3, 1.0 s bp_class_mp256_m150
(both batches), 0.7 .. 1.4 s the other surface-class rows, 1.1 / 2.0 / 0.7 / 1.2 s the classes 7 / 6 / 4 / 8, 1.2 / 1.2 / 1.6 s the
three bp_large rows (both forms), 0.4 s each bp_anydeg row, 0.9 / 1.0 s the bp_serial rows.  No case comes near 10 s.
"""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests.bp_exit_cases import EXIT_ROWS, N_POOL, _occurred, batch_index, exit_plan, has_ps, select_reference
from tests.test_gpu_local_bodies import FORMS, _decode
from tests.test_gpu_local_convergence import _assert_rows


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


def _instance(row, kind, packed, variant63=False):
    """What last_instance()["bp"] must report: the row's instance; bp_large_kernel's third integer is its form (2 min-sum with
    the check data in LDS, 1 with whole records in the workspace, 0 product-sum); the serial and the any-degree kernel have
    no packed instance (unpack / pack kernels surround them)."""
    name, t = row["bp"]
    if name == "bp_large_kernel":
        t = t[:2] + ((0,) if kind == "ps" else ((1,) if variant63 else (2,)))
    return (name, t, packed and name not in ("bp_serial_kernel", "bp_anydeg_kernel"))


def _decoders(row, H, jobs):
    """{key: decoder} for jobs {key: keywords}; constructors side by side (the class layout search is host time)."""
    from bp_osd_amd import BpOsdDecoder

    keys = list(jobs)
    with ThreadPoolExecutor(max_workers=4) as ex:
        decs = dict(zip(keys, ex.map(lambda k: BpOsdDecoder(H, **jobs[k]), keys)))
    for d in decs.values():
        if row.get("bp_variant"):
            d.set_bp_variant(row["bp_variant"])
    return decs


def _cases_of(r, idx, p, max_iter):
    """The CASES of the kernel's own result, read at one place of each pool row (the last repetition of the pool)."""
    at = np.array([np.flatnonzero(idx == i)[-1] for i in range(N_POOL)])
    return _occurred(dict(converged=r["converged"][at], iters=r["iters"][at]), p["target"], p["k"], max_iter)


def _plan_runs(row, p, decs, kind, forms, batches, variant63=False):
    """Every max_iter of a plan in the given forms and batches; the CASES the kernel shows equal the oracle's and are complete."""
    for B in batches:
        idx = batch_index(B, p["target"])
        syn = np.ascontiguousarray(p["pool"][idx])
        seen = set()
        for max_iter in p["max_iters"]:
            dec, ref = decs[(kind, max_iter)], p["refs"][max_iter]
            for form, want_llr, packed in forms:
                what = (row["id"], kind, "variant 63" if variant63 else "", B, max_iter, form)
                r = _decode(dec, syn, want_llr, packed)
                assert dec.last_instance()["bp"] == _instance(row, kind, packed, variant63), what + (dec.last_instance(),)
                _assert_rows(dec, r, ref, idx, want_llr, packed, what)
                got = _cases_of(r, idx, p, max_iter)
                assert got == _occurred(ref, p["target"], p["k"], max_iter), what
                seen |= got
        assert seen == set(p["cases"]), (row["id"], kind, B, "not exercised", sorted(set(p["cases"]) - seen))


@pytest.mark.gpu
@pytest.mark.parametrize("row", EXIT_ROWS, ids=[r["id"] for r in EXIT_ROWS])
def test_exits_against_oracle(gpu_ready, monkeypatch, row):
    """One row: the four runs of the module docstring."""
    for name, value in row.get("env", {}).items():  # (read by bposd_create)
        monkeypatch.setenv(name, value)
    t0 = time.perf_counter()
    p, f56 = exit_plan(row["id"], "ms"), exit_plan(row["id"], "f56")
    ps = exit_plan(row["id"], "ps") if has_ps(row) else None
    H = p["H"]
    jobs = {("ms", mi): dict(p["kw"], max_iter=mi) for mi in p["max_iters"]}
    jobs[("f56", 56)] = dict(f56["kw"], max_iter=56)
    if ps:
        jobs.update({("ps", mi): dict(ps["kw"], max_iter=mi) for mi in ps["max_iters"]})
    if row["large_osd"]:
        jobs.update({("osd0", mi): dict(p["kw"], max_iter=mi, osd_method="osd0") for mi in p["max_iters"]})
    decs = _decoders(row, H, jobs)
    B = row["batches"][0]
    t1 = time.perf_counter()

    # min-sum: the exits, in every form and batch
    _plan_runs(row, p, decs, "ms", FORMS, row["batches"])
    if row["family"] == "bp_large_kernel":
        for mi in p["max_iters"]:
            decs[("ms", mi)].set_bp_variant(63)
        _plan_runs(row, p, decs, "ms", FORMS, row["batches"], variant63=True)
        for mi in p["max_iters"]:
            decs[("ms", mi)].set_bp_variant(0)
    if row["large_osd"]:  # the big batches ran with osd_off: the bare pool through osd_large_kernel, once per max_iter
        every = np.arange(N_POOL)
        for mi in p["max_iters"]:
            dec = decs[("osd0", mi)]
            r = _decode(dec, p["pool"], True, False)
            inst = dec.last_instance()
            assert inst["bp"] == _instance(row, "ms", False) and inst["osd"][0] == "osd_large_kernel", (row["id"], mi, inst)
            assert not r["converged"].all(), (row["id"], mi, "no shot reached OSD")
            _assert_rows(dec, r, p["refs_osd0"][mi], every, True, False, (row["id"], "osd0 on the pool", mi))
    else:  # the small path (osd_kernel, or the wave kernels auto-selection takes for a large batch)
        assert decs[("ms", 1)].last_instance()["osd"][0] in ("osd_kernel", "osd_wave_kernel", "osd_mw_kernel"), row["id"]
    t2 = time.perf_counter()

    # the adaptive factor past iteration 53
    idx = batch_index(B, f56["target"])
    dec = decs[("f56", 56)]
    r = _decode(dec, np.ascontiguousarray(f56["pool"][idx]), True, False)
    assert dec.last_instance()["bp"] == _instance(row, "ms", False), (row["id"], "f56", dec.last_instance())
    _assert_rows(dec, r, f56["ref"], idx, True, False, (row["id"], "factor 0, max_iter 56"))
    assert not r["converged"][0] and r["iters"][0] == 56
    t3 = time.perf_counter()

    # product-sum, with its own plan
    if ps:
        _plan_runs(row, ps, decs, "ps", FORMS[:1], (B,))
    t4 = time.perf_counter()

    # per-shot priors: pool row i with select row i, wherever it stands in the batch
    k = p["k"]
    sel, alt, ref = select_reference(row, p)
    idx = batch_index(B, p["target"])
    dec = decs[("ms", k)]
    osdw = dec.decode_batch(np.ascontiguousarray(p["pool"][idx]), want_osd0=True, want_bp=True,
                            prior_select=np.ascontiguousarray(sel[idx]), alt_channel_probs=alt)
    r = dict(osdw=osdw, osd0=dec.batch_osd0, bp=dec.batch_bp, converged=dec.batch_converge, iters=dec.batch_iter, llr=None)
    assert dec.last_instance()["bp"] == _instance(row, "ms", False), (row["id"], "select", dec.last_instance())
    _assert_rows(dec, r, ref, idx, False, False, (row["id"], "per-shot priors", k))
    t5 = time.perf_counter()
    print(f"BP_EXITS {row['id']}: k {p['k']} ps k {ps['k'] if ps else '-'}  constructors {t1 - t0:.1f} s, min-sum {t2 - t1:.1f} s, "
          f"56 iterations {t3 - t2:.1f} s, product-sum {t4 - t3:.1f} s, per-shot priors {t5 - t4:.1f} s, total {t5 - t0:.1f} s")
