"""bp_osd_amd/csrc/portable_math.h evaluated ON THE DEVICE against the host compile of the same header (run with -m gpu on
an MI355X).

The product-sum parity tests compare kernels with an oracle that compiles one header with them.  One header compiled by gcc
for x86 and by hipcc for gfx950 is not thereby one function: division, subnormals and contraction can differ.  Here
``bposd_debug_portable_math`` runs every routine of the header one thread per element on the GPU, and the result must equal
the oracle library's (gcc, -ffp-contract=off) BIT FOR BIT -- there is no tolerance, the project's contract is equality; where
the host returns NaN the device must return a NaN (sign and payload of a generated NaN are the platform's).  Inputs: the
random sets of tests/test_portable_math.py (same generators and seeds), its special values, +-64 ulps around every branch
point of the header, subnormals down to the smallest one, and the arguments where the log ratio is +-inf.  When a product-sum
parity case fails, this module says whether the arithmetic or the message schedule is at fault.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# which: bposd_debug_portable_math's selector (include/bposd_mi355x_debug.h)
TANH, LOG, EXPM1, TANH_HALF, LOG_QUOT, PS_TANH_HALF_0, PS_TANH_HALF_1, PS_LOG_RATIO_0, PS_LOG_RATIO_1 = range(9)
NAMES = ("pm_tanh", "pm_log", "pm_expm1", "pm_tanh_half", "pm_log_quot", "pm_ps_tanh_half(., 0)", "pm_ps_tanh_half(., 1)",
         "pm_ps_log_ratio(., 0)", "pm_ps_log_ratio(., 1)")


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


def _device(lib, which, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    y = np.full(a.shape, -7.0)
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float64)
        assert b.shape == a.shape
    rc = lib.bposd_debug_portable_math(which, a.ctypes.data, b.ctypes.data if b is not None else None, y.ctypes.data, a.size)
    assert rc == 0, rc
    return y


def _host(which, a, b=None):
    import oracle

    if which <= EXPM1:
        return oracle.portable_math(("tanh", "log", "expm1")[which], a)
    if which == TANH_HALF:
        return oracle.portable_tanh_half(a)
    if which == LOG_QUOT:
        return oracle.portable_log_quot(a, b)
    if which in (PS_TANH_HALF_0, PS_TANH_HALF_1):
        return oracle.portable_ps_tanh_half(a, which - PS_TANH_HALF_0)
    return oracle.portable_ps_log_ratio(a, which - PS_LOG_RATIO_0)


def _assert_same(lib, which, a, b=None, what=""):
    with np.errstate(all="ignore"):
        ref = _host(which, a, b)
    got = _device(lib, which, a, b)
    nan = np.isnan(ref)
    assert (np.isnan(got) == nan).all(), f"{NAMES[which]} {what}: NaN masks differ"
    diff = (got.view(np.uint64) != ref.view(np.uint64)) & ~nan
    if diff.any():
        i = int(np.flatnonzero(diff)[0])
        arg = (float(a[i]).hex(),) + ((float(b[i]).hex(),) if b is not None else ())
        raise AssertionError(f"{NAMES[which]} {what}: {int(diff.sum())} of {diff.size} results differ from the host's; first at "
                             f"{arg}: device {float(got[i]).hex()}, host {float(ref[i]).hex()}")
    return ref


def _around(x, ulps=64):
    """x and the `ulps` doubles on either side of it (x > 0), both signs."""
    u = np.array([x], dtype=np.float64).view(np.int64)[0]
    w = (u + np.arange(-ulps, ulps + 1, dtype=np.int64))
    w = w[w >= 0].view(np.float64)
    return np.concatenate([w, -w])


# the branch points of portable_math.h (and of tests/test_portable_math.py): where tanh rounds to 1 (|x| = 19.06..) and the
# test's 19.07 / 19.1, pm_tanh's 22 and 1 and 2^-55; pm_tanh_half's saturation 38.2 (twice 19.06..), its 40, 2 and 2^-54;
# pm_expm1's ln2 / 2, 3 ln2 / 2, 56 ln2, the overflow threshold, 2^-54, its k = 20 and k = 56 steps; pm_log's sqrt(2) fold, 1,
# the smallest normal (the subnormal rescaling), 0.5 and 2
_BRANCH = (19.061547465398498, 19.07, 19.1, 22.0, 1.0, 2.0 ** -55, 38.123094930796995, 38.2, 38.3, 40.0, 2.0, 2.0 ** -54, 4.0,
           3.46573590279972654709e-01, 1.03972077083991796413e+00, 3.88162421113569373274e+01, 7.09782712893383973096e+02,
           0.5 * 3.46573590279972654709e-01, 0.5 * 1.03972077083991796413e+00, 0.5 * 3.88162421113569373274e+01,
           20 * 0.6931471805599453, 56 * 0.6931471805599453, 10 * 0.6931471805599453, 28 * 0.6931471805599453,
           1.4142135623730951, 0.7071067811865476, 0.5, 0.25, 2.2250738585072014e-308, 2 * 2.2250738585072014e-308,
           18014398509481984.0, 0.1716, 44.0, 11.0)


def _specials():
    with np.errstate(all="ignore"):
        sp1 = np.array([0.0, -0.0, 1e-320, 4.9e-324, 1.0, -1.0, 0.5, 2.0, 21.999, 22.0, 1e300, np.inf, -np.inf, np.nan,
                        1 - 1e-16, 2.2250738585072014e-308])              # test_special_values
        sp2 = np.array([19.1, -30.0, 400.0, 18.0])
        sp3 = np.array([0.0, -0.0, 1e-300, -1e-20, 38.3, -50.0, np.inf, -np.inf, 36.0, np.nan])  # the two-division test
        sub = np.concatenate([np.arange(0, 129, dtype=np.int64).view(np.float64),                 # 0 .. 128 ulps: 4.9e-324 up
                              2.0 ** np.arange(-1074.0, -1021.0), 3.0 * 2.0 ** np.arange(-1074.0, -1023.0),
                              np.float64(2.2250738585072014e-308) - 2.0 ** np.arange(-1074.0, -1023.0)])
        one = np.array([1.0, -1.0, 1 - 2.0 ** -53, -(1 - 2.0 ** -53), 1 - 2.0 ** -52, 1 + 2.0 ** -52, -(1 + 2.0 ** -52)])
    sweep = np.concatenate([_around(b) for b in _BRANCH])
    return np.concatenate([sp1, -sp1, sp2, sp3, sub, -sub, one, sweep])


def test_special_values_branch_points_and_subnormals(gpu_ready):
    s = _specials()
    assert np.isin([4.9e-324, 2.2250738585072014e-308, 1.0, -1.0, 1 - 2.0 ** -53, -(1 - 2.0 ** -53)], s).all()
    for which in (TANH, LOG, EXPM1, TANH_HALF, PS_TANH_HALF_0, PS_TANH_HALF_1, PS_LOG_RATIO_0, PS_LOG_RATIO_1):
        ref = _assert_same(gpu_ready, which, s, what="specials")
        if which in (PS_LOG_RATIO_0, PS_LOG_RATIO_1):  # x = +-1 and 1 -+ 2^-53: log(2 / 0) and log(0 / 2)
            x = np.array([1.0, -1.0])
            assert (_device(gpu_ready, which, x) == np.array([np.inf, -np.inf])).all()
            assert (ref[np.isin(s, x)] != 0).all() and np.isinf(ref[np.isin(s, x)]).all()
            near = _device(gpu_ready, which, np.array([1 - 2.0 ** -53, -(1 - 2.0 ** -53)]))
            assert np.isfinite(near).all() and near[0] == -near[1] and 36.0 < near[0] < 38.2
        if which in (TANH, PS_TANH_HALF_0, PS_TANH_HALF_1, TANH_HALF):
            assert np.abs(ref[~np.isnan(ref)]).max() == 1.0
    # pm_log_quot: the arguments the check update forms, (1 + x, 1 - x), and every pair of the list with its reverse
    with np.errstate(all="ignore"):
        _assert_same(gpu_ready, LOG_QUOT, 1 + s, 1 - s, what="(1 + x, 1 - x)")
    _assert_same(gpu_ready, LOG_QUOT, s, s[::-1].copy(), what="pairs")
    _assert_same(gpu_ready, LOG_QUOT, np.array([2.0, 0.0, 1.0, 1.5, np.nan, 0.0]), np.array([0.0, 2.0, 1.0, 0.5, 1.0, 0.0]))
    # saturation on the device itself, as tests/test_portable_math.py states it for the host
    assert _device(gpu_ready, TANH, np.array([19.1, -30.0, 400.0])).tolist() == [1.0, -1.0, 1.0]
    assert _device(gpu_ready, TANH, np.array([18.0]))[0] < 1.0
    t = _device(gpu_ready, TANH_HALF, np.array([0.0, -0.0, 1e-300, -1e-20, 38.3, -50.0, np.inf, -np.inf, 36.0]))
    assert t[:8].tolist() == [0.0, -0.0, 5e-301, -5e-21, 1.0, -1.0, 1.0, -1.0] and np.signbit(t[:2]).tolist() == [False, True] and t[8] < 1.0


def test_random_sets_of_the_host_accuracy_test(gpu_ready):
    """The generators and seeds of tests/test_portable_math.py::test_accuracy_against_libm (2 M points each)."""
    rng = np.random.default_rng(0)
    n = 2_000_000
    x = (rng.random(n) * 2 - 1) * 10.0 ** (rng.random(n) * 6 - 4)
    _assert_same(gpu_ready, TANH, x, what="x")
    y = 10.0 ** (rng.random(n) * 40 - 20)
    _assert_same(gpu_ready, LOG, y, what="y")
    z = (rng.random(n) * 2 - 1) * 50
    _assert_same(gpu_ready, EXPM1, z, what="z")
    ha, hb = (rng.random(n) * 60 - 30) / 2, (rng.random(n) * 60 - 30) / 2
    a, b = _assert_same(gpu_ready, TANH, ha, what="a"), _assert_same(gpu_ready, TANH, hb, what="b")
    with np.errstate(all="ignore"):
        r = (1 + a * b) / (1 - a * b)
    ref = _assert_same(gpu_ready, LOG, r, what="(1 + ab) / (1 - ab)")
    assert np.isfinite(ref).all() and (ref != 0).any()
    # the same arguments through the check update's own entry points, both evaluation orders
    for form in (0, 1):
        _assert_same(gpu_ready, PS_TANH_HALF_0 + form, 2 * ha, what="2 ha")
        _assert_same(gpu_ready, PS_TANH_HALF_0 + form, x, what="x")
        _assert_same(gpu_ready, PS_LOG_RATIO_0 + form, a * b, what="ab")
    _assert_same(gpu_ready, EXPM1, x, what="x")


def test_random_sets_of_the_two_division_test(gpu_ready):
    """The generators and seeds of tests/test_portable_math.py::test_two_division_form_of_the_check_update (1 M points)."""
    rng = np.random.default_rng(1)
    n = 1_000_000
    x = (rng.random(n) * 2 - 1) * 10.0 ** (rng.random(n) * 7 - 5)
    _assert_same(gpu_ready, TANH_HALF, x, what="x")
    X = np.tanh((rng.random(n) * 60 - 30) / 2) * np.tanh((rng.random(n) * 60 - 30) / 2)
    ref = _assert_same(gpu_ready, LOG_QUOT, 1 + X, 1 - X, what="(1 + X, 1 - X)")
    assert np.isfinite(ref).all() and (ref != 0).any()
    for form in (0, 1):
        _assert_same(gpu_ready, PS_TANH_HALF_0 + form, x, what="x")
        _assert_same(gpu_ready, PS_LOG_RATIO_0 + form, X, what="X")
    _assert_same(gpu_ready, TANH, x / 2, what="x / 2")


def test_arguments_are_checked(gpu_ready):
    x = np.ones(4)
    y = np.zeros(4)
    f = gpu_ready.bposd_debug_portable_math
    assert f(9, x.ctypes.data, None, y.ctypes.data, 4) == -1 and f(-1, x.ctypes.data, None, y.ctypes.data, 4) == -1
    assert f(LOG_QUOT, x.ctypes.data, None, y.ctypes.data, 4) == -1 and f(0, None, None, y.ctypes.data, 4) == -1
    assert f(0, x.ctypes.data, None, y.ctypes.data, C.c_int64(-1)) == -1
    assert f(0, x.ctypes.data, None, y.ctypes.data, 0) == 0 and not y.any()
