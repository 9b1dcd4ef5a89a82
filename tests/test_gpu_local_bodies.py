"""Every loop body of bp_local_kernel and every edge of its size window, on the GPU (run with -m gpu on an MI355X).

One bp_local_kernel instance holds seven keyed iteration loops, a generic loop, a generic loop with LLR stores and -- in a
PAIRKEY instance -- a pair loop; which of them a wave runs is decided by the host's layout search for the matrix.
tests/local_codes.py LOCAL_CODES pins, per matrix, the wave table that search gives, and tests/test_local_codes_cpu.py
proves without a GPU that the rows together reach every body with checks in both groups.  This file decodes every row.

What is compared with what
- The instance auto-selection picks (``last_instance()`` and ``last_pair_key()`` are asserted, and so is the wave table,
  read live: a layout search that drops a body fails here as it does on the CPU) against a second implementation that
  shares none of the loop bodies: the LDS kernel bp_kernel, through ``set_bp_variant(1)`` -- ``<6, 3, 1, 1024>`` up to 1024
  checks, the two-checks-per-thread shape ``<6, 3, 2, 1024>`` above.  osdw, osd0, bp, converged and iters are equal on the
  whole batch, and so is every LLR bit where LLRs are asked for.
- Both against the CPU oracle on the first rows of the batch (``_compare_exact``: the five outputs and the LLR bits).  For
  a syndrome outside the column space of a rank-deficient matrix OSD's pivot rows are the kernel's choice
  (tests/test_gpu_edges.py), so there the oracle is the reference for bp, converged, iters and the LLR bits only.
- max_iter 1 (the last-iteration LLR body alone), 2 (one iteration of a keyed / pair / generic body before it) and 30 at
  a physical error rate for which the oracle alone leaves between 0.1 % and 60 % of the ``H e`` syndromes unconverged
  (the row's ``q``); a uniform ``error_rate`` (the scalar-prior instances ``<., 1024, 8, ., uprior>``) and per-bit
  ``channel_probs`` (``<2, 1024, 6>``); LLRs asked for (every iteration runs the LLR body), not asked for (the keyed, pair
  and generic bodies run) and the packed form.  The batch holds the all-zero syndrome, the all-ones syndrome and 32
  uniformly random ones next to the ``H e`` rows.
- Above 40000 syndromes a 1024-position call runs the two-checks-per-thread instance (a wave of two groups exists only
  there: pair and generic bodies); a call of at most 40000 runs ``<1, 1024, 8>`` (one group per wave: every key through the
  one-check-per-thread loops).  Every row does both.  The 2048-position kernel has one shape at every batch size.
- The numbered variants 17 .. 22, 24 and 26 without LLRs (the plain instance: the generic body on the (k, mixed) wave).

A limit that cannot be tested away.  Posterior LLRs are written by the LLR body only, so the fp64 sums of a keyed, pair or
generic loop never appear as LLR bits of their own: they show through the integer outputs (the hard decisions, the
iteration at which BP converged), through the input they leave for the last iteration's LLR body, and through osd0, whose
column order is the order of those LLRs.  Hence the large batches, the 30 iterations near the convergence threshold and
OSD-0 on every unconverged row.  (When written, a wrong dl in one slot of one keyed loop, in group 0 of a pair loop or in
one select of bit_update_mixed each failed the rows that run that body.)
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests.local_codes import (ALL_KEYS_ROWS, LOCAL_CODES, N_SPECIAL, PAST_WINDOW, assert_row_tables, decoder_settings,
                               matrix_of, per_bit_probs, row_by_id, syndrome_seed, syndromes, wave_tables)
from tests.test_gpu_parity import _compare_exact

pytestmark = pytest.mark.gpu

B_TWO_GROUPS = 40960 + 512  # above the small-call threshold (launch_bp_local.hip: 40000): two checks per thread
B_2048 = 8192 + 34  # the 2048-position kernel has one shape whatever the batch
B_SMALL = 2048 + 34
N_ORACLE = N_SPECIAL + 256  # rows the oracle decodes: the all-zero, the all-ones and 32 random syndromes, 256 H e rows
FORMS = (("llr", True, False), ("no_llr", False, False), ("packed", False, True))
OUTPUTS = ("osdw", "osd0", "bp", "converged", "iters")


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


def _decode(dec, syn, want_llr, packed):
    """The arrays are the decoder's own buffers: they hold until its next decode."""
    if packed:
        osdw = dec.decode_batch(syn, want_osd0=True, want_bp=True, packed=True)
    else:
        osdw = dec.decode_batch(syn, want_osd0=True, want_bp=True, want_llr=want_llr)
    return dict(osdw=osdw, osd0=dec.batch_osd0, bp=dec.batch_bp, converged=dec.batch_converge, iters=dec.batch_iter,
                llr=dec.batch_llr if want_llr else None)


def _build(H, q, max_iters):
    """{(max_iter, 'local' / 'lds'): decoder}.  Every constructor runs the layout search (seconds of host time on three
    threads); up to four constructors of one row run side by side."""
    from bp_osd_amd import BpOsdDecoder

    keys = [(mi, which) for mi in max_iters for which in ("local", "lds")]
    with ThreadPoolExecutor(max_workers=min(4, len(keys))) as ex:
        decs = list(ex.map(lambda k: BpOsdDecoder(H, **decoder_settings(q, k[0])), keys))
    out = dict(zip(keys, decs))
    for (mi, which), d in out.items():
        if which == "lds":
            d.set_bp_variant(1)
    return out


def _lds_instance(MP, packed):
    return ("bp_kernel", (6, 3, 1, 1024) if MP == 1024 else (6, 3, 2, 1024), packed)


def _same(ra, rb, want_llr, what):
    for k in OUTPUTS:
        assert (ra[k] == rb[k]).all(), what + (k, "local kernel != LDS kernel")
    if want_llr:
        assert (ra["llr"].view(np.uint64) == rb["llr"].view(np.uint64)).all(), what + ("LLR bits", "local kernel != LDS kernel")


def _against_oracle(dec, r, ref, packed, in_space, what):
    """The first rows of a GPU result against the oracle's: everything (LLR bits included where the GPU has them) on the rows
    in the column space of H, BP's outputs and the LLR bits on the others."""
    k = len(ref["iters"])
    g = {key: (r[key][:k] if r[key] is not None else None) for key in r}
    if packed:
        for key in ("osdw", "osd0", "bp"):
            g[key] = dec.unpack_rows(g[key], dec.n)
    try:
        _compare_exact({key: (v[in_space] if v is not None else None) for key, v in g.items()},
                       {key: (v[in_space] if v is not None else None) for key, v in ref.items()})
        out = ~in_space
        if out.any():
            for key in ("converged", "iters", "bp"):
                assert (np.asarray(g[key][out]) == np.asarray(ref[key][out]).astype(g[key].dtype)).all(), key
            if g["llr"] is not None:
                assert (g["llr"][out].view(np.uint64) == ref["llr"][out].view(np.uint64)).all(), "LLR bits differ"
    except AssertionError as e:
        raise AssertionError(f"{what}: GPU != oracle: {e}") from e


def _expected_local(row, B, uniform, packed):
    """(instance, PAIRKEY) auto-selection takes (launch_bp_local.hip)"""
    if row["MP"] == 2048:
        return ("bp_local_kernel", (2, 2048, 4, 0), packed), row["pairkey"]
    if B <= 40000:
        return ("bp_local_kernel", (1, 1024, 8, 0), packed), -1
    return ("bp_local_kernel", (2, 1024, 8 if uniform else 6, 0), packed), row["pairkey"]


@pytest.mark.parametrize("row", LOCAL_CODES, ids=[r["id"] for r in LOCAL_CODES])
def test_row_auto_instance_vs_lds_kernel_and_oracle(gpu_ready, row):
    """One LOCAL_CODES row through the decode matrix of the module docstring."""
    from oracle import OracleDecoder

    H = matrix_of(row)
    m, n = H.shape
    assert_row_tables(row, wave_tables(gpu_ready, H))  # the guard against a silent loss of coverage
    MP, q = row["MP"], row["q"]
    B = B_TWO_GROUPS if MP == 1024 else B_2048
    syn = syndromes(H, q, B, syndrome_seed(row))
    in_space = np.ones(N_ORACLE, bool)
    if not row["full_rank"]:
        in_space[1:N_SPECIAL] = False  # (a random syndrome of a rank-deficient matrix may be in the column space: then
        # the comparison of OSD's outputs with the oracle is merely left out for it)
    probs = per_bit_probs(row)
    decs = _build(H, q, (1, 2, 30))
    for max_iter in (1, 2, 30):
        a, b = decs[(max_iter, "local")], decs[(max_iter, "lds")]
        o = OracleDecoder(H, **decoder_settings(q, max_iter))
        for channel in ("uniform", "per_bit"):
            if channel == "per_bit":
                for d in (a, b, o):
                    d.update_channel_probs(probs)
            ref = o.decode_batch(syn[:N_ORACLE])
            if max_iter == 30:
                unconverged = float((ref["converged"][N_SPECIAL:] == 0).mean())
                print(row["id"], channel, "oracle: unconverged H e rows", unconverged)
                assert 0.001 <= unconverged <= 0.6, (row["id"], channel, unconverged)
            calls = [(B, f) for f in FORMS]
            if max_iter == 30 and channel == "uniform":  # the small call: one check per thread, one group per wave
                calls += [(B_SMALL, f) for f in FORMS]
            for nb, (form, want_llr, packed) in calls:
                what = (row["id"], channel, max_iter, form, nb)
                ra = _decode(a, syn[:nb], want_llr, packed)
                inst, pk = _expected_local(row, nb, channel == "uniform", packed)
                assert a.last_instance()["bp"] == inst, what + (a.last_instance(),)
                assert a.last_pair_key() == pk, what + (a.last_pair_key(),)
                rb = _decode(b, syn[:nb], want_llr, packed)
                assert b.last_instance()["bp"] == _lds_instance(MP, packed), what + (b.last_instance(),)
                assert b.bp_kernel_info()["kernel"] == "bp_kernel" and b.last_pair_key() == -1
                _same(ra, rb, want_llr, what)
                _against_oracle(a, ra, ref, packed, in_space, what)


VARIANTS_1024 = {17: (2, 1024, 8, 0), 18: (1, 1024, 8, 0), 19: (4, 1024, 4, 1), 20: (2, 1024, 6, 1), 21: (4, 1024, 3, 1),
                 22: (2, 1024, 8, 0), 24: (2, 1024, 6, 0), 26: (1, 1024, 8, 0)}


@pytest.mark.parametrize("row_id", ALL_KEYS_ROWS)
def test_numbered_variants_without_llr(gpu_ready, row_id):
    """Variants 17 .. 22, 24 and 26 with want_llr=False (the variant sweep of tests/test_gpu_parity.py asks for LLRs, so every
    iteration of it runs the LLR body) on one row per MP that holds all seven keys: the plain instance of every shape -- its
    keyed loops where the shape has them, the generic loop on the (k, mixed) wave and in the A/B shapes -- against the LDS
    kernel on the whole batch and the oracle on the first rows.  max_iter 2 and 30, uniform channel (22, 24 and 26 are the
    scalar-prior shapes).  At 2048 positions every number is the one shape ``<2, 2048, 4>``, plain: 17 and 22 only."""
    from oracle import OracleDecoder

    row = row_by_id(row_id)
    H = matrix_of(row)
    t = wave_tables(gpu_ready, H)
    assert_row_tables(row, t)
    assert set(t["group_key"]) == {0, 1, 2, 5, 6, 10, 15}
    MP, q = row["MP"], row["q"]
    syn = syndromes(H, q, 4096 + N_SPECIAL, syndrome_seed(row))
    in_space = np.ones(N_ORACLE, bool)
    assert row["full_rank"]
    decs = _build(H, q, (2, 30))
    for max_iter in (2, 30):
        a, b = decs[(max_iter, "local")], decs[(max_iter, "lds")]
        ref = OracleDecoder(H, **decoder_settings(q, max_iter)).decode_batch(syn[:N_ORACLE])
        rb = _decode(b, syn, False, False)
        assert b.last_instance()["bp"] == _lds_instance(MP, False)
        _against_oracle(b, rb, ref, False, in_space, (row_id, "lds", max_iter))
        # (at 2048 positions every number is the same plain instance: two of them are enough)
        for variant, shape in VARIANTS_1024.items() if MP == 1024 else [(17, None), (22, None)]:
            a.set_bp_variant(variant)
            ra = _decode(a, syn, False, False)
            what = (row_id, "variant", variant, max_iter)
            assert a.last_instance()["bp"] == ("bp_local_kernel", shape if MP == 1024 else (2, 2048, 4, 0), False), what
            assert a.last_pair_key() == -1, what
            _same(ra, rb, False, what)
            _against_oracle(a, ra, ref, False, in_space, what)


def test_one_past_the_window_takes_another_kernel(gpu_ready):
    """A (3,6)-regular matrix with m one step past 2048: no layout (the host-only export refuses it), the local-edge kernel on
    request is refused, and auto-selection takes what bposd_capi.hip's rules give for it -- no LDS shape holds 2050 checks
    (shape 8 ends at 2048), so BP is HBM-resident: bp_large_kernel ``<12, 6, 2>`` -- which agrees with the oracle."""
    from bp_osd_amd import BpOsdDecoder
    from oracle import OracleDecoder

    row = PAST_WINDOW
    H = matrix_of(row)
    with pytest.raises(ValueError, match="status -2"):
        wave_tables(gpu_ready, H)
    syn = syndromes(H, row["q"], N_ORACLE, syndrome_seed(row))
    kw = decoder_settings(row["q"], 30)
    g = BpOsdDecoder(H, **kw)
    with pytest.raises(ValueError, match="local-edge BP kernel needs"):
        g.set_bp_variant(16)
    got = _decode(g, syn, True, False)
    assert g.last_instance()["bp"] == ("bp_large_kernel", (12, 6, 2), False), g.last_instance()
    assert g.last_pair_key() == -1
    ref = OracleDecoder(H, **kw).decode_batch(syn)
    _against_oracle(g, got, ref, False, np.ones(len(syn), bool), (row["id"],))
