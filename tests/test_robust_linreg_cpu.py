"""RRM and Huber linear regression in one launch (rlvi_amd/csrc/robust_linreg.hip, rlvi_amd/rrm.py, rlvi_amd/huber.py),
the part that needs no GPU: the numpy restatement tests/robust_linreg_ref.py against every case the reference left in
tests/golden/g19_robust_linreg.npz, Huber's alpha by erf against scipy's chi-square distribution, the new symbols and
the return codes of their argument checks.

The bars: theta against the reference's at rtol 1e-8 + 10 x theta_bar, theta_bar the largest relative distance
tools/make_golden_robust_linreg.py measured between the restatement's theta and the reference's (RRM: what Brent's
tolerance on xi leaves; Huber: rounding); iteration counts equal; the weights of a stored E-step at rtol 10 x w_bar /
atol 1e-300, as tests/test_rrm_cpu.py.  Each test prints its distances before it asserts (pytest -s shows them)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import robust_linreg_ref as R
import rrm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G19 = np.load(os.path.join(ROOT, "tests", "golden", "g19_robust_linreg.npz"))
CASES = [str(k) for k in G19["cases"]]
RUNS = [str(k) for k in G19["runs"]]
BAR = {"rrm": float(G19["theta_bar_rrm"]), "huber": float(G19["theta_bar_huber"])}
W_BAR = float(G19["w_bar"])
ENTRIES = ("rlvi_rrm_linear_regression_f64", "rlvi_rrm_linear_regression_batch_f64",
           "rlvi_huber_linear_regression_f64", "rlvi_huber_linear_regression_batch_f64", "rlvi_huber_alpha")

_runs = {}


def run_param(run):
    return float(run[len("rrm_eps"):]) if run.startswith("rrm") else float(run[len("huber_sigma"):])


def ref_run(key, run):
    """The restatement on a G19 case, computed once: (theta, weights | sigma, count, trace, E-steps)."""
    if (key, run) not in _runs:
        X, y = G19[key + "/X"].astype(np.float64), G19[key + "/y"].astype(np.float64)
        steps = []
        if run.startswith("rrm"):
            r = R.rrm_linear_regression(X, y, run_param(run), steps=steps)
        else:
            r = R.huber_linear_regression(X, y, sigma0=run_param(run))
        _runs[(key, run)] = r + (steps,)
    return _runs[(key, run)]


@pytest.fixture(scope="module")
def lib():
    from rlvi_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_the_fixture_holds_the_cases_of_the_issue():
    assert CASES == ["gen_17x3", "gen_40x10", "gen_257x20", "gauss_1000x20", "gauss_1025x31"]
    assert RUNS == ["rrm_eps0.2", "rrm_eps0.4", "huber_sigma1.0", "huber_sigma0.1"]
    examined, passed = (int(v) for v in G19["runs_examined_passed"])        # (runs, not seeds: the tool says why)
    assert passed >= len(CASES) * len(RUNS) and examined - passed <= 0.1 * examined
    for key in CASES:
        n, d = (int(v) for v in key.split("_")[1].split("x"))
        assert G19[key + "/X"].shape == (n, d) and G19[key + "/y"].shape == (n,)
        for run in RUNS[:2]:
            assert (f"{key}/{run}/estep_losses" in G19) == (n * d <= 257 * 20)
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", "g19_robust_linreg.npz"))
    assert size <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "g18_rrm.npz"))


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("key", CASES)
def test_restatement_against_every_g19_case(key, run):
    est = run.split("_")[0]
    theta, second, count, trace, steps = ref_run(key, run)
    ref = G19[f"{key}/{run}/theta"]
    margin = R.rrm_margin(trace) if est == "rrm" else R.huber_margin(trace)
    print(f"{key} {run}: count {count} (fixture {int(G19[f'{key}/{run}/count'])}), |theta - reference's| / |.| = "
          f"{np.linalg.norm(theta - ref) / np.linalg.norm(ref):.3e} (bar {BAR[est]:.3e}), least stop margin {margin:.1e}")
    assert count == int(G19[f"{key}/{run}/count"])
    assert margin >= (1e-6 if est == "rrm" else 1e-3)
    np.testing.assert_allclose(theta, ref, rtol=1e-8 + 10 * BAR[est])
    if est == "rrm":
        assert len(steps) == count and abs(second.sum() - 1.0) <= 1e-12
    else:
        assert second > 0.0


@pytest.mark.parametrize("run", RUNS[:2])
@pytest.mark.parametrize("key", [k for k in CASES if f"{k}/rrm_eps0.2/estep_losses" in G19])
def test_restatement_weights_on_every_stored_estep(key, run):
    eps = run_param(run)
    for k, (l_in, w_ref) in enumerate(zip(G19[f"{key}/{run}/estep_losses"], G19[f"{key}/{run}/estep_w"])):
        w = rrm_ref.update_weights(l_in, eps)[0]
        big = w_ref > 1e-300
        print(f"{key} {run} E-step {k}: relative weight distance "
              f"{np.max(np.abs(w[big] - w_ref[big]) / w_ref[big]):.3e} (w_bar {W_BAR:.3e})")
        np.testing.assert_allclose(w, w_ref, rtol=10 * W_BAR, atol=1e-300)


def test_alpha_by_erf_is_scipys_chi_square(lib):
    from scipy.stats import chi2
    for c in (0.05, 0.3, 0.7317, 1.0, 1.345, 2.0, 3.5, 6.0):
        want = c ** 2 * (1 - chi2.cdf(c ** 2, df=1)) + chi2.cdf(c ** 2, df=3)
        got, ref = lib.rlvi_huber_alpha(c), R.huber_alpha(c)
        print(f"c = {c}: alpha {got!r}, scipy's {want!r}, relative distance {abs(got - want) / want:.2e}")
        # F3 = F1 - sqrt(2 / pi) c exp(-c^2 / 2) cancels for small c: alpha ~ c^2 there and the absolute error stays eps
        assert abs(got - want) <= 4e-16 + 1e-14 * want
        assert abs(got - ref) <= 4e-16


def test_new_symbols_are_built_declared_and_exported(lib):
    from rlvi_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rlvi_hip.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in include/rlvi_hip.h"
    import rlvi_amd
    from rlvi_amd import huber, ops, rrm
    assert list(inspect.signature(rrm.linear_regression).parameters) == ["X", "y", "eps", "maxiter", "tol",
                                                                         "return_info"]
    assert list(inspect.signature(huber.linear_regression).parameters) == ["X", "y", "c", "sigma0", "maxiter",
                                                                           "return_info"]
    sig = inspect.signature(huber.linear_regression).parameters
    assert sig["c"].default == 0.7317 and sig["sigma0"].default == 1 and sig["maxiter"].default == 1000
    assert sig["maxiter"].kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (ops.rrm_linear_regression, ops.rrm_linear_regression_batch, ops.huber_linear_regression,
               ops.huber_linear_regression_batch):
        assert {"out", "info", "ws"} <= set(inspect.signature(fn).parameters)
    assert rlvi_amd.rrm_linear_regression is rrm.linear_regression
    assert rlvi_amd.rrm_linear_regression_batch is rrm.linear_regression_batch
    assert rlvi_amd.huber_linear_regression is huber.linear_regression
    assert rlvi_amd.huber_linear_regression_batch is huber.linear_regression_batch
    assert np.array_equal(huber.psi_huber(np.array([-3.0, -0.5, 0.0, 0.7, 2.0]), 0.7), [-0.7, -0.5, 0.0, 0.7, 0.7])


def test_argument_checks_return_their_codes_without_a_gpu(lib):
    """NULL, SHAPE, LIMIT, ALIGN in this order, all before any launch."""
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255
    rrm1 = lambda X=p, y=p, n=40, d=10, eps=0.2, it=100, th=p, w=p, info=p, ws=p: \
        lib.rlvi_rrm_linear_regression_f64(X, y, n, d, eps, it, 1e-3, th, w, info, ws, None)          # noqa: E731
    rrmb = lambda X=p, B=3, n=40, d=10, eps=0.2, it=100, ws=p: \
        lib.rlvi_rrm_linear_regression_batch_f64(X, p, B, n, d, eps, it, 1e-3, p, p, p, ws, None)      # noqa: E731
    hub1 = lambda X=p, y=p, n=40, d=10, c=0.7317, s0=1.0, it=1000, th=p, sc=p, info=p, ws=p: \
        lib.rlvi_huber_linear_regression_f64(X, y, n, d, c, s0, it, th, sc, info, ws, None)            # noqa: E731
    hubb = lambda X=p, B=3, n=40, d=10, c=0.7317, s0=1.0, it=1000, ws=p: \
        lib.rlvi_huber_linear_regression_batch_f64(X, p, B, n, d, c, s0, it, p, p, p, ws, None)        # noqa: E731
    for fn in (rrm1, hub1):
        for kw in (dict(X=None), dict(y=None), dict(th=None), dict(info=None), dict(ws=None)):
            assert fn(**kw) == -1, kw
        assert fn(n=0) == -2 and fn(d=0) == -2 and fn(n=-4) == -2 and fn(it=-1) == -2
        assert fn(n=4097) == -5 and fn(d=32) == -5
        assert fn(X=p + 4) == -3 and fn(th=p + 4) == -3 and fn(info=p + 2) == -3 and fn(ws=p + 8) == -3
        assert fn(X=None, n=0) == -1 and fn(n=0, d=32) == -2 and fn(n=4097, X=p + 4) == -5       # the order
    assert rrm1(w=None) == -1 and hub1(sc=None) == -1
    for eps in (0.0, 1.0, -0.5, 1.5, float("nan"), 0.98):                   # 0.98: (1 - eps) n = 0.8 <= 1
        assert rrm1(eps=eps) == -2 and rrmb(eps=eps) == -2, eps
    for c, s0 in ((0.0, 1.0), (-1.0, 1.0), (0.7, 0.0), (0.7, -2.0), (float("nan"), 1.0), (0.7, float("nan"))):
        assert hub1(c=c, s0=s0) == -2 and hubb(c=c, s0=s0) == -2, (c, s0)
    for fn in (rrmb, hubb):
        assert fn(X=None) == -1 and fn(B=0) == -2 and fn(B=-1) == -2 and fn(B=(1 << 20) + 1) == -5
        assert fn(n=4097) == -5 and fn(d=32) == -5 and fn(X=p + 4) == -3 and fn(ws=p + 8) == -3
