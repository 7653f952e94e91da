"""The batch forms of the one-launch estimators without a device: the five C entries are exported and validate their
arguments on the host, the fixture tests/golden/g17_sweep.npz is what tools/make_golden_batch.py says it is, and the
numpy-facing standard.*_batch raise on bad arguments before anything reaches a device."""
import ctypes
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENTRIES = ("rlvi_linear_regression_batch_f64", "rlvi_logistic_regression_batch_f64", "rlvi_robust_mean_batch_f64",
           "rlvi_robust_pca_batch_f64", "rlvi_robust_covariance_batch_f64")
MAXBATCH = 1 << 20


@pytest.fixture(scope="module")
def lib():
    from rlvi_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_the_five_entries_are_exported_and_bound(lib):
    from rlvi_amd import _lib, ops, standard
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        single = _lib.SIGNATURES[name.replace("_batch", "")][1]
        # the single entry's argument list with `int64_t batch` in front of n
        k = 2 if "regression" in name else 1
        assert _lib.SIGNATURES[name][1] == single[:k] + [ctypes.c_int64] + single[k:]
    for fn in ("linear_regression_batch", "logistic_regression_batch", "robust_mean_batch", "robust_pca_batch",
               "robust_covariance_batch"):
        assert callable(getattr(ops, fn))
    for fn in ("linear_regression_batch", "logistic_regression_batch", "mean_batch", "pca_batch", "covariance_batch"):
        assert callable(getattr(standard, fn))
    assert lib.rlvi_abi_version() == 3


def calls(lib, p):
    """name -> call(X, batch, n, out): each entry with the host pointer p everywhere else"""
    return {
        "linreg": lambda X, B, n, out=p, d=2: lib.rlvi_linear_regression_batch_f64(
            X, p, B, n, d, 100, 1e-3, 1e-3, 100, out, p, p, p, None),
        "logreg": lambda X, B, n, out=p, d=2: lib.rlvi_logistic_regression_batch_f64(
            X, p, B, n, d, 100, 1e-2, 1e-3, 100, 100.0, out, p, None, p, p, None),
        "mean": lambda X, B, n, out=p, d=2: lib.rlvi_robust_mean_batch_f64(
            X, B, n, d, 100, 1e-3, 1e-3, 100, out, p, p, p, None),
        "pca": lambda X, B, n, out=p, d=2: lib.rlvi_robust_pca_batch_f64(
            X, B, n, d, 100, 1e-2, None, 1e-3, 100, out, p, p, p, None),
        "cov": lambda X, B, n, out=p, d=2: lib.rlvi_robust_covariance_batch_f64(
            X, B, n, d, 0.6 * n, 100, 1e-2, 1e-3, 100, out, p, p, p, None),
    }


@pytest.mark.parametrize("name", ["linreg", "logreg", "mean", "pca", "cov"])
def test_argument_errors_without_a_gpu(name, lib):
    """Validation happens on the host before any launch: NULL -> -1, batch <= 0 -> -2, a batch or a shape beyond the
    limits -> -5, a misaligned pointer -> -3."""
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255
    call = calls(lib, p)[name]
    assert call(None, 4, 40) == -1
    assert call(p, 4, 40, out=None) == -1
    assert call(p, 0, 40) == -2 and call(p, -3, 40) == -2
    assert call(p, 4, 0) == -2
    assert call(p, MAXBATCH + 1, 40) == -5
    assert call(p, 4, 4097) == -5
    assert call(p, 4, 40, d=40) == -5
    assert call(p + 4, 4, 40) == -3
    assert call(p, 4, 40, out=p + 4) == -3


def test_g17_fixture_is_what_the_tool_says():
    g = np.load(os.path.join(GOLDEN, "g17_sweep.npz"))
    assert g["linreg/X"].shape == (32, 40, 10) and g["linreg/y"].shape == (32, 40)
    assert g["linreg/theta"].shape == (32, 10)
    assert g["mean/sample"].shape == (32, 100, 2) and g["mean/theta"].shape == (32, 2)
    assert g["logreg/X"].shape == (16, 200, 2) and g["logreg/y"].shape == (16, 200)
    assert g["logreg/theta"].shape == (16, 3)
    assert g["pca/sample"].shape == (16, 40, 2) and g["pca/theta"].shape == (16, 2)
    assert g["pca/theta_init"].shape == (2,)
    assert g["cov/sample"].shape == (16, 50, 2) and g["cov/theta"].shape == (16, 2, 2)
    assert float(g["cov_eps"]) == 0.4
    for kind in ("linreg", "mean"):
        assert np.array_equal(g[kind + "/eps"], np.repeat([0.0, 0.13, 0.27, 0.4], 8))
    for kind in ("linreg", "mean", "logreg", "pca", "cov"):
        B = len(g[kind + "/theta"])
        assert g[kind + "/outer"].shape == (B,) and (g[kind + "/outer"] >= 1).all()
        assert g[kind + "/seed"].shape == (B,) and len(set(g[kind + "/seed"].tolist())) == B
    assert set(np.unique(g["logreg/y"])) == {0.0, 1.0}
    assert all(np.isfinite(g[k]).all() for k in g.files if g[k].dtype == np.float64)
    tried, kept = (int(v) for v in g["seeds_tried_kept"])
    assert kept == 32 + 32 + 16 + 16 + 16 and tried - kept <= 0.1 * tried


def sweep(B=5, n=40, d=2, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((B, n, d))
    y = (rng.random((B, n)) < 0.5).astype(np.float64)
    y[:, 0], y[:, 1] = 0.0, 1.0
    return X, y


def test_standard_batch_checks_raise_before_touching_a_device(lib, monkeypatch):
    """NaN in problem 3, a one-class y in problem 1, eps = 1, shapes beyond the one launch: raised with the problem's
    index, and no device is asked for (standard._dev is made to fail the test if it is)."""
    from rlvi_amd import _lib, standard

    def no_device():
        raise AssertionError("a device was asked for before the arguments were checked")
    monkeypatch.setattr(standard, "_dev", no_device)
    X, y = sweep()
    Xn = X.copy()
    Xn[3, 7, 1] = np.nan
    with pytest.raises(ValueError, match=r"infs or NaNs \(problem 3\)"):
        standard.linear_regression_batch(Xn, y)
    with pytest.raises(ValueError, match=r"NaN or infinity. \(problem 3\)"):
        standard.logistic_regression_batch(Xn, y)
    for fn in (standard.mean_batch, standard.pca_batch):
        with pytest.raises(ValueError, match=r"NaN or infinity. \(problem 3\)"):
            fn(Xn)
    with pytest.raises(ValueError, match=r"NaN or infinity. \(problem 3\)"):
        standard.covariance_batch(Xn, 0.4)
    yn = y.copy()
    yn[3, 5] = np.inf
    with pytest.raises(ValueError, match=r"\(problem 3\)"):
        standard.linear_regression_batch(X, yn)
    y1 = y.copy()
    y1[1] = 1.0
    with pytest.raises(ValueError, match=r"at least 2 classes in the data \(problem 1\)"):
        standard.logistic_regression_batch(X, y1)
    y2 = y.copy()
    y2[2, 4] = 0.5
    with pytest.raises(ValueError, match=r"class labels 0 and 1 \(problem 2\)"):
        standard.logistic_regression_batch(X, y2)
    for eps in (1.0, 0.0, 1.5):
        with pytest.raises(ValueError, match="0 < eps < 1"):
            standard.covariance_batch(X, eps)
    with pytest.raises(ValueError, match="theta_init"):
        standard.pca_batch(X, theta_init=np.ones(3))
    with pytest.raises(ValueError, match="theta_init|NaN"):
        standard.pca_batch(X, theta_init=np.array([np.nan, 1.0]))
    # a shape beyond the one-launch limits is an error, never a loop of single calls
    big = np.zeros((2, 4097, 2))
    bigy = np.tile([0.0, 1.0], (2, 2049))[:, :4097]
    with pytest.raises(_lib.RlviError, match="one launch"):
        standard.linear_regression_batch(big, bigy)
    with pytest.raises(_lib.RlviError, match="one launch"):
        standard.logistic_regression_batch(big, bigy)
    with pytest.raises(_lib.RlviError, match="one launch"):
        standard.mean_batch(big)
    with pytest.raises(_lib.RlviError, match="one launch"):
        standard.covariance_batch(np.zeros((2, 40, 9)), 0.4)
    with pytest.raises(ValueError):
        standard.mean_batch(X[0])                         # [n, d]: not a batch
    with pytest.raises(ValueError):
        standard.linear_regression_batch(X, y[:, :-1])
