"""RRM's logistic regression in one launch (rlvi_amd/csrc/robust_logreg.hip, rlvi_amd/rrm.py), the part that needs no
GPU: the numpy restatement tests/robust_logreg_ref.py against every run the reference left in
tests/golden/g20_rrm_logreg.npz, the signatures, the host-side errors and the return codes of the argument checks.

The bars: the restatement takes every stored outer count with every stop decision clear of the edge (margin >= 1e-4,
the fixture's rule); its theta is within theta_bar of the reference's, theta_bar the largest relative distance
||theta_restatement - theta_reference|| / ||theta_reference|| that tools/make_golden_rrm_logreg.py measured (liblinear's
tolerance) -- times 1 + 1e-3 for another numpy's order of sums, which moves the restatement by 1e-12 and the bar by
nothing; the weights of a stored rule call within w_bar, measured and stored the same way, atol 1e-300.  Each test
prints its distances before it asserts (pytest -s shows them)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import robust_logreg_ref as R
import rrm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G20 = np.load(os.path.join(ROOT, "tests", "golden", "g20_rrm_logreg.npz"))
CASES = [str(k) for k in G20["cases"]]
RUNS = [str(k) for k in G20["runs"]]
THETA_BAR, W_BAR = float(G20["theta_bar"]), float(G20["w_bar"])
ENTRIES = ("rlvi_rrm_logistic_regression_f64", "rlvi_rrm_logistic_regression_batch_f64")

_runs = {}


def run_eps(run):
    return float(run.rsplit("/eps", 1)[1])


def run_data(run):
    key = run.rsplit("/", 1)[0]
    return G20[key + "/X"].astype(np.float64), G20[key + "/y"].astype(np.float64)


def ref_run(run):
    """The restatement on a G20 run, computed once: (theta, weights, count, trace)."""
    if run not in _runs:
        _runs[run] = R.rrm_logistic_regression(*run_data(run), run_eps(run))
    return _runs[run]


@pytest.fixture(scope="module")
def lib():
    from rlvi_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_the_fixture_holds_the_runs_of_the_issue():
    want = [f"gen_{n}x2_c{c}" for n in (17, 64, 100, 200) for c in (0.05, 0.3)]
    want += ["gauss_1000x20_c0.0", "gauss_1025x23_c0.0", "gauss_4096x30_c0.0"]
    assert CASES == want
    want_runs = [f"{k}/eps{e}" for k in want[:-1] for e in (0.3, 0.4)] + [want[-1] + "/eps0.4"]
    assert RUNS == want_runs
    examined, passed = (int(v) for v in G20["runs_examined_passed"])
    assert passed >= len(RUNS) and examined - passed <= 0.1 * examined
    for key in CASES:
        n, d = (int(v) for v in key.split("_")[1].split("x"))
        assert G20[key + "/X"].shape == (n, d) and G20[key + "/y"].shape == (n,)
    for run in RUNS:
        n = run_data(run)[0].shape[0]
        count = int(G20[run + "/count"])
        assert G20[run + "/trace"].shape == (count,)
        assert (run + "/estep_losses" in G20) == (n <= 200)
        if n <= 200:
            assert G20[run + "/estep_losses"].shape == (count, n) and G20[run + "/estep_w"].shape == (count, n)
    assert int(G20["gen_17x2_c0.3/eps0.3/count"]) == 100             # the reference's limit cycle: all 100 iterations
    assert 0.0 < THETA_BAR < 1e-2 and 0.0 < W_BAR < 1e-4             # liblinear's and Brent's tolerances, not a bug's
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g20_rrm_logreg.npz")) < 1 << 20


@pytest.mark.parametrize("run", RUNS)
def test_restatement_against_every_g20_run(run):
    theta, w, count, trace = ref_run(run)
    ref = G20[run + "/theta"]
    dist = np.linalg.norm(theta - ref) / np.linalg.norm(ref)
    print(f"{run}: count {count} (fixture {int(G20[run + '/count'])}), |theta - reference's| / |.| = {dist:.3e} "
          f"(theta_bar {THETA_BAR:.3e}), least stop margin {R.margin(trace):.1e}")
    assert count == int(G20[run + "/count"])
    assert R.margin(trace) >= 1e-4
    assert dist <= THETA_BAR * (1 + 1e-3)
    assert abs(w.sum() - 1.0) <= 1e-12


@pytest.mark.parametrize("run", [r for r in RUNS if r + "/estep_losses" in G20])
def test_restatement_weights_on_every_stored_rule_call(run):
    eps, worst = run_eps(run), 0.0
    for l_in, w_ref in zip(G20[run + "/estep_losses"], G20[run + "/estep_w"]):
        assert abs(w_ref.sum() - 1.0) <= 1e-9                        # (the reference's floor moved no sum: G18's rule)
        w = rrm_ref.update_weights(l_in, eps)[0]
        big = w_ref > 1e-300
        worst = max(worst, float(np.max(np.abs(w[big] - w_ref[big]) / w_ref[big])))
        np.testing.assert_allclose(w, w_ref, rtol=W_BAR * (1 + 1e-3), atol=1e-300)
    print(f"{run}: {len(G20[run + '/estep_w'])} rule calls, largest relative weight distance {worst:.3e} "
          f"(w_bar {W_BAR:.3e})")


def test_signatures_are_the_references(lib):
    import rlvi_amd
    from rlvi_amd import _lib, ops, rrm
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rlvi_hip.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in include/rlvi_hip.h"
    for fn in (rrm.logistic_regression, rrm.logistic_regression_batch):
        sig = inspect.signature(fn).parameters
        assert list(sig) == ["X", "y", "eps", "maxiter", "tol", "return_info"]           # rrm.py:76
        assert sig["eps"].default is inspect.Parameter.empty
        assert sig["maxiter"].default == 100 and sig["tol"].default == 1e-2
        assert sig["return_info"].kind is inspect.Parameter.KEYWORD_ONLY and sig["return_info"].default is False
    for fn in (ops.rrm_logistic_regression, ops.rrm_logistic_regression_batch):
        assert {"out", "info", "ws"} <= set(inspect.signature(fn).parameters)
        assert list(inspect.signature(fn).parameters)[:5] == ["X", "y", "eps", "maxiter", "tol"]
    assert rlvi_amd.rrm_logistic_regression is rrm.logistic_regression
    assert rlvi_amd.rrm_logistic_regression_batch is rrm.logistic_regression_batch
    assert "logistic_regression(X, y, eps, maxiter=100, tol=1e-2)" in rrm.__doc__
    assert "logistic_regression_batch" in rrm.__doc__


def test_host_side_errors_need_no_device(lib, monkeypatch):
    """eps, values that are not finite, labels of one class, shapes beyond the launch: raised before anything reaches
    the device -- the device is made unreachable, so a call that got that far would fail otherwise."""
    from rlvi_amd import _lib, rrm
    from rlvi_amd import standard as _std

    def no_device():
        raise AssertionError("the call reached the device")
    monkeypatch.setattr(_std, "_dev", no_device)
    rng = np.random.default_rng(0)
    X = rng.standard_normal((40, 2))
    y = (np.arange(40) % 2).astype(np.float64)
    XB, yB = np.stack([X, X, X]), np.stack([y, y, y])
    for eps in (0.0, 1.0, -0.5, 1.5, 0.98):                          # 0.98: (1 - eps) n = 0.8 <= 1
        with pytest.raises(ValueError, match="eps"):
            rrm.logistic_regression(X, y, eps)
        with pytest.raises(ValueError, match="eps"):
            rrm.logistic_regression_batch(XB, yB, eps)
    for bad in (np.nan, np.inf):
        Xb = X.copy()
        Xb[7, 1] = bad
        with pytest.raises(ValueError, match="Input contains NaN or infinity"):
            rrm.logistic_regression(Xb, y, 0.4)
        yb = y.copy()
        yb[3] = bad
        with pytest.raises(ValueError, match="Input contains NaN or infinity"):
            rrm.logistic_regression(X, yb, 0.4)
        with pytest.raises(ValueError, match=r"Input contains NaN or infinity.*problem 1"):
            rrm.logistic_regression_batch(np.stack([X, Xb, X]), yB, 0.4)
    for label in (0.0, 1.0):
        with pytest.raises(ValueError, match="This solver needs samples of at least 2 classes in the data"):
            rrm.logistic_regression(X, np.full(40, label), 0.4)
        with pytest.raises(ValueError, match=r"at least 2 classes in the data \(problem 2\)"):
            rrm.logistic_regression_batch(XB, np.stack([y, y, np.full(40, label)]), 0.4)
    for shape in ((4097, 2), (50, 31)):
        Z = np.zeros(shape)
        t = (np.arange(shape[0]) % 2).astype(np.float64)
        with pytest.raises(_lib.RlviError, match="4096.*30"):
            rrm.logistic_regression(Z, t, 0.4)
        with pytest.raises(_lib.RlviError, match="4096.*30"):
            rrm.logistic_regression_batch(Z[None], t[None], 0.4)
    with pytest.raises(ValueError):
        rrm.logistic_regression(X, y[:-1], 0.4)
    with pytest.raises(ValueError):
        rrm.logistic_regression_batch(X, y, 0.4)
    with pytest.raises(AssertionError, match="reached the device"):  # (and a clean call does get that far)
        rrm.logistic_regression(X, y, 0.4)


def test_argument_checks_return_their_codes_without_a_gpu(lib):
    """NULL, SHAPE, LIMIT, ALIGN in this order, all before any launch: the checks of rlvi_logistic_regression_f64 and
    the eps rule of the RRM regressions."""
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255
    one = lambda X=p, y=p, n=100, d=2, eps=0.4, it=100, C=100.0, th=p, w=p, info=p, ws=p: \
        lib.rlvi_rrm_logistic_regression_f64(X, y, n, d, eps, it, 1e-2, C, th, w, info, ws, None)       # noqa: E731
    bat = lambda X=p, B=3, n=100, d=2, eps=0.4, it=100, C=100.0, ws=p: \
        lib.rlvi_rrm_logistic_regression_batch_f64(X, p, B, n, d, eps, it, 1e-2, C, p, p, p, ws, None)  # noqa: E731
    for kw in (dict(X=None), dict(y=None), dict(th=None), dict(w=None), dict(info=None), dict(ws=None)):
        assert one(**kw) == -1, kw
    assert one(n=0) == -2 and one(d=0) == -2 and one(n=-4) == -2 and one(it=-1) == -2
    assert one(C=0.0) == -2 and one(C=-1.0) == -2 and one(C=float("nan")) == -2
    assert one(n=4097) == -5 and one(d=31) == -5 and one(n=4096, d=30, X=p + 4) == -3
    assert one(X=p + 4) == -3 and one(th=p + 4) == -3 and one(info=p + 2) == -3 and one(ws=p + 8) == -3
    assert one(X=None, n=0) == -1 and one(n=0, d=31) == -2 and one(n=4097, X=p + 4) == -5       # the order
    for eps in (0.0, 1.0, -0.5, 1.5, float("nan"), 0.995):                # 0.995: (1 - eps) n = 0.5 <= 1
        assert one(eps=eps) == -2 and bat(eps=eps) == -2, eps
    assert bat(X=None) == -1 and bat(B=0) == -2 and bat(B=-1) == -2 and bat(B=(1 << 20) + 1) == -5
    assert bat(n=4097) == -5 and bat(d=31) == -5 and bat(X=p + 4) == -3 and bat(ws=p + 8) == -3
    assert bat(C=0.0) == -2 and bat(it=-1) == -2
