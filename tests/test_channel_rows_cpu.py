"""Per-shot channel rows without a GPU: ``bposd_channel_tables`` is the host's libm bit for bit and refuses what the
constructor refuses, and the inputs of tests/test_gpu_channel_rows.py (tests/channel_rows_cases.py), decoded on the
oracle, exercise what that test is about -- so that it cannot go vacuous."""
import math

import numpy as np
import pytest

from bp_osd_amd import _lib, BpOsdDecoder
from bp_osd_amd.build import build_library
from tests import channel_rows_cases as cr


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _lib.load()


def test_library_exports_the_rows_calls(lib):
    for name in ("bposd_channel_tables", "bposd_decode_batch_rows", "bposd_decode_batch_rows_device"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_channel_tables_are_libm_bit_for_bit(lib):
    rng = np.random.default_rng(11)
    # 0.5 (prior LLR exactly 0), the clip values of the GPU test, the ends of the range, and a spread over normal numbers
    # only: log-uniform over 1e-300 .. 1 and uniform over (0, 1)
    p = np.concatenate([[0.5, 1e-3, 0.4, 0.0, 1.0, 2.0 ** -1022], 10.0 ** rng.uniform(-300, 0, 4997), rng.uniform(0, 1, 4997)])
    assert p.size == 10 ** 4 and (p[5:] >= 2.0 ** -1022).all()
    llr, cost = BpOsdDecoder.channel_tables(p)
    with np.errstate(divide="ignore"):
        # (math.log raises at 0 where the C library returns -inf: log(0 / 1) = -inf, log(1 / 0) = +inf)
        want_llr = np.array([math.log((1 - x) / x) if 0 < x < 1 else (math.inf if x == 0 else -math.inf) for x in p])
        want_cost = np.array([math.log(1 / x) if x > 0 else math.inf for x in p])
    assert (llr.view(np.uint64) == want_llr.view(np.uint64)).all()
    assert (cost.view(np.uint64) == want_cost.view(np.uint64)).all()
    assert llr[0] == 0.0 and not np.signbit(llr[0])
    # any shape, and either output alone through the C entry
    l2, c2 = BpOsdDecoder.channel_tables(p.reshape(100, 100))
    assert l2.shape == (100, 100) and (l2.ravel().view(np.uint64) == llr.view(np.uint64)).all() and (c2.ravel() == cost).all()
    only = np.empty_like(p)
    assert lib.bposd_channel_tables(p.ctypes.data, p.size, None, only.ctypes.data) == 0 and (only == cost).all()
    assert lib.bposd_channel_tables(p.ctypes.data, p.size, only.ctypes.data, None) == 0 and (only.view(np.uint64) == llr.view(np.uint64)).all()
    assert lib.bposd_channel_tables(None, 0, None, None) == 0


@pytest.mark.parametrize("bad", [-0.1, 1.5, math.nan])
def test_channel_tables_reject_what_the_ctor_rejects(lib, bad):
    p = np.array([0.1, 0.2, bad, 0.3])
    with pytest.raises(ValueError, match=r"probs\[2\]"):
        BpOsdDecoder.channel_tables(p)
    out = np.full(4, 7.0)
    assert lib.bposd_channel_tables(p.ctypes.data, 4, out.ctypes.data, out.ctypes.data) == _lib.BPOSD_ERR_INVALID
    assert (out == 7.0).all(), "written in spite of the error"


def _counts(case_id):
    ref, uni = cr.reference(case_id), cr.uniform_reference(case_id)
    differ = (ref["osdw"] != uni["osdw"]).any(axis=1) | (ref["bp"] != uni["bp"]).any(axis=1) | (ref["iters"] != uni["iters"])
    return int((ref["converged"] == 0).sum()), int(differ.sum()), len(differ)


# non-converged shots / shots whose osdw, bp or iteration count differ from the uniform-channel decode / B
TABLE = {"bp_pair_4_2": (48, 48, 48), "bp_pair_8_4": (48, 48, 48), "bp_pair_16_8": (21, 41, 48), "bp_anydeg_dc17": (28, 38, 48),
         "bp_serial_dv8": (22, 35, 48), "bp_class_mp256_m170": (48, 48, 48), "bp_hbm_m1025_dc9": (11, 11, 11),
         "bp_shape8_m1025_dc8": (11, 11, 11), "large_n2048_m1000": (11, 11, 11), "reg64_s1": (29, 45, 48),
         "reg128_s1": (33, 47, 48), "random31_s3_hz": (26, 48, 48), "reg1025_s1": (11, 11, 11)}


def test_oracle_table_keeps_the_gpu_test_honest():
    assert set(TABLE) == set(cr.TABLE_IDS)
    got = {i: _counts(i) for i in cr.TABLE_IDS}
    print(got)
    for i, (nonconv, differ, B) in got.items():
        assert differ * 4 >= B, f"{i}: only {differ} of {B} shots differ from the uniform-channel decode"
    both = [i for i, (nonconv, _, B) in got.items() if nonconv >= 10 and B - nonconv >= 10]
    assert len(both) >= 4, both
    nonconv, _, B = _counts("reg1025_s1_q0.03")
    assert B - nonconv >= 8, "reg1025_s1 at q = 0.03 has too few converged shots"
    assert got == TABLE, "the inputs have drifted from the measured table"
    # the 0.5 entries are there: prior LLR exactly 0 in every case
    for c in cr.CASES:
        P, S = cr.case_inputs(c)
        assert (P == 0.5).any() and P.min() >= 1e-3 and P[P != 0.5].max() <= 0.4 and S.shape == (len(P), cr.matrix(c["code"]).shape[0])


def test_expected_instances_cover_every_family():
    bps = {cr.expected_instances(c)[0][0] for c in cr.CASES}
    osds = {cr.expected_instances(c)[1][:2] for c in cr.CASES}
    assert bps == {"bp_kernel", "bp_anydeg_kernel", "bp_serial_kernel", "bp_class_kernel", "bp_large_kernel", "bp_local_kernel"}
    assert ("osd_large_kernel", (2,)) in osds and any(o[0] == "osd_kernel" for o in osds)
    strides = {cr.expected_instances(c)[0][1][1] for c in cr.CASES if cr.is_local(c)}
    assert strides == {1024, 2048}
