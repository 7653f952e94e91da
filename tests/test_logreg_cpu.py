"""Logistic regression in one launch, the part that needs no GPU: the C ABI's three entries and their argument
checks, and the float64 restatement of the device algorithm (tests/logreg_ref.py) against the reference's recorded
fits (tests/golden/g15_logreg.npz, tools/make_golden_logreg.py).

The yardstick is the strong-convexity bound.  liblinear, the restatement and the kernel minimise the same
    f(v) = 1/2 v.v + C sum_i (w_i / max w) log(1 + exp(-s_i z_i)),
whose Hessian is >= I, so for ANY two points ||v_a - v_b|| <= ||grad f(v_a)|| + ||grad f(v_b)||: a bound from the
two answers' own gradients (evaluated in extended precision, logreg_ref.gradient), not a guessed tolerance."""
import ctypes
import os

import numpy as np
import pytest

import logreg_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    from rlvi_amd import _build, _lib
    _build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def g15():
    return np.load(os.path.join(GOLDEN, "g15_logreg.npz"))


@pytest.fixture(scope="module")
def ref_runs(g15):
    """The restatement's estimator on every case, once: {case: (theta, weights, outer, trace)}."""
    return {k: logreg_ref.logistic_regression(g15[k + "/X"].astype(np.float64), g15[k + "/y"])
            for k in g15["cases"]}


def fits_of(g, key):
    """(X, y, w, liblinear's v) of every recorded fit of a case."""
    X, y = g[key + "/X"].astype(np.float64), g[key + "/y"]
    for w, theta in zip(g[key + "/fit_w"], g[key + "/fit_theta"]):
        yield X, y, w, logreg_ref.to_v(theta)


def test_exports_and_ctypes_table(lib):
    from rlvi_amd import _lib
    for name in ("rlvi_logistic_regression_f64", "rlvi_logistic_fit_f64", "rlvi_logistic_regression_check"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.rlvi_abi_version() == 3


def test_check_says_which_shapes_the_launch_takes(lib):
    for (n, d) in ((1, 1), (4096, 30), (200, 2)):
        assert lib.rlvi_logistic_regression_check(n, d) == 0, (n, d)
    assert lib.rlvi_logistic_regression_check(4097, 2) == -5
    assert lib.rlvi_logistic_regression_check(200, 31) == -5
    for (n, d) in ((0, 2), (-1, 2), (200, 0), (200, -3)):
        assert lib.rlvi_logistic_regression_check(n, d) == -2, (n, d)
    from rlvi_amd import ops
    assert ops.logistic_regression_check(200, 2) and not ops.logistic_regression_check(4097, 2)


def test_argument_errors_without_a_gpu(lib):
    """Validated on the host before any launch: null (-1), shape (-2), alignment (-3), limit (-5)."""
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255
    est, fit = lib.rlvi_logistic_regression_f64, lib.rlvi_logistic_fit_f64
    assert est(None, p, 8, 2, 5, 1e-2, 1e-3, 100, 100.0, p, p, None, p, p, None) == -1
    assert est(p, p, 8, 2, 5, 1e-2, 1e-3, 100, 100.0, p, p, None, None, p, None) == -1
    assert est(p, p, 8, 2, 5, 1e-2, 1e-3, 100, 100.0, p, p, None, p, None, None) == -1
    assert est(p, p, 0, 2, 5, 1e-2, 1e-3, 100, 100.0, p, p, None, p, p, None) == -2
    assert est(p, p, 8, 2, -1, 1e-2, 1e-3, 100, 100.0, p, p, None, p, p, None) == -2
    assert est(p, p, 8, 2, 5, 1e-2, 1e-3, 100, 0.0, p, p, None, p, p, None) == -2           # C must be positive
    assert est(p, p, 4097, 2, 5, 1e-2, 1e-3, 100, 100.0, p, p, None, p, p, None) == -5
    assert est(p, p, 8, 31, 5, 1e-2, 1e-3, 100, 100.0, p, p, None, p, p, None) == -5
    assert est(p + 4, p, 8, 2, 5, 1e-2, 1e-3, 100, 100.0, p, p, None, p, p, None) == -3
    assert est(p, p, 8, 2, 5, 1e-2, 1e-3, 100, 100.0, p, p, None, p + 2, p, None) == -3     # info: 4-byte aligned
    assert est(p, p, 8, 2, 5, 1e-2, 1e-3, 100, 100.0, p, p, None, p, p + 8, None) == -3     # workspace: 256
    assert fit(p, p, None, 8, 2, 100.0, p, p, p, p, None) == -1
    assert fit(p, p, p, 8, 2, 100.0, p, None, p, p, None) == -1
    assert fit(p, p, p, 8, 0, 100.0, p, p, p, p, None) == -2
    assert fit(p, p, p, 4097, 2, 100.0, p, p, p, p, None) == -5
    assert fit(p, p, p + 4, 8, 2, 100.0, p, p, p, p, None) == -3


def test_restatement_and_liblinear_within_the_strong_convexity_bound(g15):
    """Every recorded fit: ||v_ref.py - v_liblinear|| <= ||grad f(v_ref.py)|| + ||grad f(v_liblinear)||, and the
    restatement meets liblinear's stop criterion (a small gradient) at least as well as liblinear's own answer."""
    nfits = 0
    for key in g15["cases"]:
        for (X, y, w, v_lib) in fits_of(g15, key):
            theta, losses, steps = logreg_ref.fit(X, y, w)
            v = logreg_ref.to_v(theta)
            ga = np.linalg.norm(logreg_ref.gradient(X, y, w, v))
            gb = np.linalg.norm(logreg_ref.gradient(X, y, w, v_lib))
            dist = np.linalg.norm(v - v_lib)
            assert dist <= ga + gb, (key, dist, ga, gb)
            assert ga <= gb, (key, ga, gb)
            assert 1 <= steps <= logreg_ref.NEWTON_CAP
            np.testing.assert_allclose(losses, np.logaddexp(0.0, logreg_ref.design(X) @ v), rtol=1e-15)
            nfits += 1
    assert nfits >= 40


def test_restatement_takes_the_reference_outer_count(g15, ref_runs):
    tried, kept = g15["seeds_tried_kept"]
    assert kept == len(g15["cases"]) and tried - kept <= 0.1 * tried
    for key in g15["cases"]:
        theta, w, outer, trace = ref_runs[key]
        assert outer == int(g15[key + "/outer"]), key
        assert len(trace) == outer and len(g15[key + "/trace"]) == outer


def test_restatement_on_g5_within_the_existing_bar():
    """tests/test_gpu_parity.py holds the liblinear path to rtol=1e-3, atol=1e-4 on G5 logreg/*: so is this."""
    g = np.load(os.path.join(GOLDEN, "g5_standard.npz"))
    theta, _, _, _ = logreg_ref.logistic_regression(g["logreg/X"], g["logreg/y"])
    np.testing.assert_allclose(theta, g["logreg/theta"], rtol=1e-3, atol=1e-4)
