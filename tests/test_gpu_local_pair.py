"""bp_local_kernel instances with a pair body (a loop of its own for the wave of a uniform group and the mixed one) against
the generic LDS kernel (set_bp_variant(1)) as a second implementation: five outputs and LLR bits, byte and packed forms."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 40960 + 512  # above the small-call threshold: auto-selection takes the two-checks-per-thread kernel
MIXED = 15


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


def _code(name):
    from bp_osd_amd.codes import h1922, hgp, regular_ldpc_seed

    if name.startswith("h1922"):
        return getattr(h1922(compute_logicals=False), name[-2:])
    return hgp(regular_ldpc_seed(31, 31, 3, 3, seed=3), compute_logicals=False).hz  # a wave of two different uniform keys: not covered


def _wave_table(lib, H):
    from tests.local_codes import wave_tables

    t = wave_tables(lib, H)
    return t["body"], t["pairkey"], t["generic"]


def _syndromes(H, q, nb, seed):
    rng = np.random.default_rng(seed)
    err = (rng.random((nb, H.shape[1])) < q).astype(np.uint8)
    return np.ascontiguousarray(np.asarray((H @ err.T) % 2).T.astype(np.uint8))


def _decode(dec, syn, want_llr, packed):
    if packed:
        osdw = dec.decode_batch(syn, want_osd0=True, want_bp=True, packed=True)
        out = dict(osdw=osdw.copy(), osd0=dec.batch_osd0.copy(), bp=dec.batch_bp.copy())
    else:
        osdw = dec.decode_batch(syn, want_osd0=True, want_bp=True, want_llr=want_llr)
        out = dict(osdw=osdw.copy(), osd0=dec.batch_osd0.copy(), bp=dec.batch_bp.copy())
        if want_llr:
            out["llr"] = dec.batch_llr.copy()
    out["converged"] = dec.batch_converge.copy()
    out["iters"] = dec.batch_iter.copy()
    return out


@pytest.mark.parametrize("channel", ["uniform", "per_bit"])
@pytest.mark.parametrize("name", ["h1922_hz", "h1922_hx", "random31_hz"])
def test_pair_instance_against_the_lds_kernel(gpu_ready, name, channel):
    """H1922 hz / hx (their one wave of unequal groups is covered: no generic wave) and a code with a wave the instance does
    not cover (generic body inside a PAIRKEY instance), decoded by the instance auto-selection picks and by the generic LDS
    kernel: osdw, osd0, bp, converged, iters and the LLR bits identical -- with out_llr (every iteration runs the LLR body) and
    without (the pair body runs, the LLRs reach OSD-0 through the workspace), byte and packed rows, max_iter 1 and 2 (the
    last-iteration LLR body alone / one iteration of the pair body before it) and 30 (a batch with non-converging syndromes).
    uniform: the scalar-prior instance <2,1024,8,false,true>; per_bit: <2,1024,6,false,false>."""
    from bp_osd_amd import BpOsdDecoder

    H = _code(name)
    body, pairkey, generic = _wave_table(gpu_ready, H)
    assert pairkey >= 0 and (32 + pairkey) in body
    assert (generic == 0) == name.startswith("h1922")
    q = 0.06
    syn = _syndromes(H, q, B, 77)
    probs = None
    if channel == "per_bit":
        probs = q * (0.75 + 0.5 * np.random.default_rng(5).random(H.shape[1]))
    for max_iter in (1, 2, 30):
        kw = dict(max_iter=max_iter, bp_method="ms", ms_scaling_factor=0.0, osd_method="osd0")
        kw.update(dict(error_rate=q) if probs is None else dict(channel_probs=probs))
        for want_llr, packed in ((True, False), (False, False), (False, True)):
            a = BpOsdDecoder(H, **kw)
            ra = _decode(a, syn, want_llr, packed)
            inst = a.last_instance()["bp"]
            assert inst[0] == "bp_local_kernel" and inst[1][:2] == (2, 1024) and inst[2] == packed, inst
            assert inst[1][2] == (8 if channel == "uniform" else 6), inst
            assert a.last_pair_key() == pairkey
            b = BpOsdDecoder(H, **kw)
            b.set_bp_variant(1)
            rb = _decode(b, syn, want_llr, packed)
            assert b.bp_kernel_info()["kernel"] == "bp_kernel" and b.last_pair_key() == -1
            if max_iter == 30:
                assert 0.001 < (~ra["converged"]).mean() < 0.999
            for k in ("osdw", "osd0", "bp", "converged", "iters"):
                assert (ra[k] == rb[k]).all(), (name, channel, max_iter, want_llr, packed, k)
            if want_llr:
                assert (ra["llr"].view(np.uint64) == rb["llr"].view(np.uint64)).all(), (name, channel, max_iter)


def test_variant_by_number_is_the_plain_instance(gpu_ready):
    """A variant asked for by number (22: the headline shape) launches the plain instance -- the generic body for the wave
    of unequal groups -- and agrees with the pair instance."""
    from bp_osd_amd import BpOsdDecoder

    H = _code("h1922_hz")
    syn = _syndromes(H, 0.06, B, 78)
    kw = dict(error_rate=0.06, max_iter=20, bp_method="ms", ms_scaling_factor=0.0, osd_method="osd0")
    a, b = BpOsdDecoder(H, **kw), BpOsdDecoder(H, **kw)
    b.set_bp_variant(22)
    ra, rb = _decode(a, syn, False, False), _decode(b, syn, False, False)
    assert a.last_pair_key() >= 0 and b.last_pair_key() == -1
    assert a.last_instance()["bp"] == b.last_instance()["bp"]
    for k in ("osdw", "osd0", "bp", "converged", "iters"):
        assert (ra[k] == rb[k]).all(), k
