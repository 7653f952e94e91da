"""Robust Risk Minimization's mean, PCA and covariance in one launch (rlvi_amd/csrc/moments.hip, rlvi_amd/rrm.py), the
part that needs no GPU: the numpy restatement tests/rrm_ref.py against every case the reference left in
tests/golden/g18_rrm.npz, the entropy identity, the no-root limit, the new exports and the argument errors.

The bars on theta are those the project holds against G7 (tests/test_gpu_parity.py): mean rtol 1e-9 / atol 1e-12, pca
1e-7 / 1e-10, covariance 1e-6 / 1e-9.  The weights of a stored E-step are held at rtol 10 x w_bar / atol 1e-300, w_bar
the largest relative distance tools/make_golden_rrm.py measured over the fixture: what Brent's tolerance on xi, times
l / alpha, leaves between the reference's weights and the exact root's.  Each test prints its distances before it
asserts (pytest -s shows them)."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import rrm_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G18 = np.load(os.path.join(GOLDEN, "g18_rrm.npz"))
CASES = [str(k) for k in G18["cases"]]
ONLY = dict(zip(CASES, (bool(v) for v in G18["restatement_only"])))
STEP_CASES = [k for k in CASES if k + "/estep_losses" in G18]
W_BAR = float(G18["w_bar"])
BARS = {"mean": (1e-9, 1e-12), "pca": (1e-7, 1e-10), "cov": (1e-6, 1e-9)}

_ref_runs = {}


def ref_run(key):
    """The restatement's estimator on a G18 case, computed once: (theta, weights, outer, trace, E-steps)."""
    if key not in _ref_runs:
        x = G18[key + "/sample"].astype(np.float64)
        eps = float(G18[key + "/eps"])
        kind = key.split("_")[0]
        steps = []
        if kind == "mean":
            r = R.mean(x, eps, steps=steps)
        elif kind == "pca":
            r = R.pca(x, eps, theta_init=G18[key + "/theta_init"] if key + "/theta_init" in G18 else None, steps=steps)
        else:
            r = R.covariance(x, eps, steps=steps)
        _ref_runs[key] = r + (steps,)
    return _ref_runs[key]


@pytest.fixture(scope="module")
def lib():
    from rlvi_amd import _build, _lib
    _build.build()
    return _lib.load()


@pytest.mark.parametrize("key", CASES)
def test_restatement_against_every_g18_case(key):
    kind = key.split("_")[0]
    theta, w, outer, trace, steps = ref_run(key)
    ref = G18[key + "/theta"]
    rtol, atol = BARS[kind]
    print(f"{key}: outer {outer} (fixture {int(G18[key + '/outer'])}), max |theta - reference's| = "
          f"{np.max(np.abs(theta - ref)):.3e}, relative {np.linalg.norm(theta - ref) / np.linalg.norm(ref):.3e}, "
          f"least stop margin {np.min(np.abs(trace - (1e-3 if kind == 'mean' else 1e-2))):.1e}")
    assert outer == int(G18[key + "/outer"]) == len(steps)
    assert theta.shape == ref.shape
    assert abs(w.sum() - 1.0) <= 1e-12
    if not ONLY[key]:                                            # (a restatement-only case carries no reference bar)
        np.testing.assert_allclose(theta, ref, rtol=rtol, atol=atol)


@pytest.mark.parametrize("key", STEP_CASES)
def test_restatement_weights_and_entropy_on_every_stored_estep(key):
    """The restatement's rule on the losses the reference's update_weights was handed: its weights at 10 x w_bar, and
    the entropy of the restatement's weights = log((1 - eps) n) to 1e-12 wherever there was a root."""
    eps = float(G18[key + "/eps"])
    for k, (l_in, w_ref) in enumerate(zip(G18[key + "/estep_losses"], G18[key + "/estep_w"])):
        w, alpha, had_root = R.update_weights(l_in, eps)
        n = l_in.shape[0]
        big = w_ref > 1e-300
        print(f"{key} E-step {k}: alpha {alpha:.6g}, had_root {had_root}, largest l / alpha "
              f"{(l_in.max() - l_in.min()) / alpha if had_root else np.inf:.1f}, relative weight distance "
              f"{np.max(np.abs(w[big] - w_ref[big]) / w_ref[big]):.3e} (w_bar {W_BAR:.3e}), entropy - target "
              f"{R.entropy(w) - np.log((1 - eps) * n):.3e}")
        np.testing.assert_allclose(w, w_ref, rtol=10 * W_BAR, atol=1e-300)
        assert abs(w.sum() - 1.0) <= 1e-12
        if had_root:
            assert abs(R.entropy(w) - np.log((1 - eps) * n)) <= 1e-12


def test_fixture_records_its_bookkeeping():
    tried, kept = (int(v) for v in G18["seeds_tried_kept"])
    assert kept == len(CASES) and tried >= kept and tried - kept <= 0.1 * tried
    kinds = [k.split("_")[0] for k in CASES]
    assert kinds.count("mean") == kinds.count("pca") == kinds.count("cov") == 10
    assert {float(G18[k + "/eps"]) for k in CASES} == {0.2, 0.4}
    assert 0.0 < W_BAR < 1e-3
    for kind in ("mean", "pca", "cov"):                          # at most the two largest shapes, restatement only
        assert sum(ONLY[k] for k in CASES if k.startswith(kind)) <= 2
    assert os.path.getsize(os.path.join(GOLDEN, "g18_rrm.npz")) <= os.path.getsize(
        os.path.join(GOLDEN, "g16_moments.npz"))
    for key in CASES:
        assert G18[key + "/sample"].ndim == 2 and int(G18[key + "/outer"]) >= 1


def test_no_root_limit():
    """5 minima tied among 8 at eps 0.5 ((1 - eps) n = 4 <= 5), and all-equal losses: 1 / m on the minima."""
    l = np.array([3.0, 1.5, 1.5, 7.0, 1.5, 1.5, 2.0, 1.5])
    w, alpha, had_root = R.update_weights(l, 0.5)
    assert not had_root and alpha == 0.0
    assert np.array_equal(w, np.where(l == 1.5, 0.2, 0.0))
    w, alpha, had_root = R.update_weights(np.full(9, -4.25), 0.3)
    assert not had_root and np.array_equal(w, np.full(9, 1.0 / 9))
    # one fewer tie than (1 - eps) n: a root, and it is sharp
    w, alpha, had_root = R.update_weights(np.array([1.0, 1.0, 1.0, 2.0, 5.0, 9.0, 9.0, 9.0]), 0.5)
    assert had_root and abs(R.entropy(w) - np.log(4.0)) <= 1e-12 and abs(w.sum() - 1.0) <= 1e-12
    for bad in (0.0, 1.0, -0.1, 0.9):                            # 0.9: (1 - eps) n = 0.8 <= 1
        with pytest.raises(ValueError):
            R.update_weights(l, bad)


def test_restatement_is_invariant_to_a_shift_of_the_losses():
    """What the shift by min l is for: negative losses (a covariance whose log det is) and losses at 1e6 give the
    weights of the same losses at 0."""
    rng = np.random.default_rng(18)
    l = rng.chisquare(2, 100)
    w0 = R.update_weights(l, 0.2)[0]
    for shift in (-50.0, 1e6):
        np.testing.assert_allclose(R.update_weights(l + shift, 0.2)[0], w0, rtol=1e-7, atol=1e-300)


NEW = ("rlvi_rrm_mean_f64", "rlvi_rrm_pca_f64", "rlvi_rrm_covariance_f64", "rlvi_rrm_mean_batch_f64",
       "rlvi_rrm_pca_batch_f64", "rlvi_rrm_covariance_batch_f64", "rlvi_rrm_update_weights_f64")


def test_new_symbols_are_in_the_header_and_in_the_library(lib):
    from rlvi_amd import _lib, ops, rrm
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "rlvi_hip.h")).read()
    for name in NEW:
        assert f"int {name}(" in header
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for name in ("rrm_mean", "rrm_pca", "rrm_covariance", "rrm_mean_batch", "rrm_pca_batch", "rrm_covariance_batch",
                 "rrm_update_weights"):
        assert callable(getattr(ops, name))
    for name in ("update_weights", "mean", "pca", "covariance", "mean_batch", "pca_batch", "covariance_batch"):
        assert callable(getattr(rrm, name))
        p = inspect.signature(getattr(rrm, name)).parameters["return_info"]
        assert p.default is False and p.kind == inspect.Parameter.KEYWORD_ONLY
    E = inspect.Parameter.empty
    assert [(p.name, p.default) for p in inspect.signature(rrm.pca).parameters.values()][:5] == [
        ("sample", E), ("eps", E), ("maxiter", 100), ("tol", 1e-2), ("theta_init", None)]
    assert [(p.name, p.default) for p in inspect.signature(rrm.mean).parameters.values()][:4] == [
        ("sample", E), ("eps", E), ("maxiter", 100), ("tol", 1e-3)]
    assert [(p.name, p.default) for p in inspect.signature(rrm.covariance).parameters.values()][:4] == [
        ("sample", E), ("eps", E), ("maxiter", 100), ("tol", 1e-2)]


def test_c_entries_answer_argument_errors_without_a_device(lib):
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255
    mean, pca, cov, uw = (lib.rlvi_rrm_mean_f64, lib.rlvi_rrm_pca_f64, lib.rlvi_rrm_covariance_f64,
                          lib.rlvi_rrm_update_weights_f64)
    mean_b, pca_b, cov_b = lib.rlvi_rrm_mean_batch_f64, lib.rlvi_rrm_pca_batch_f64, lib.rlvi_rrm_covariance_batch_f64
    # NULL
    assert mean(None, 10, 2, 0.2, 5, 1e-3, p, p, p, p, None) == -1
    assert pca(p, 10, 2, 0.2, 5, 1e-2, None, p, None, p, p, None) == -1
    assert cov(p, 10, 2, 0.2, 5, 1e-2, p, p, p, None, None) == -1
    assert uw(None, 10, 0.2, p, p, p, None) == -1 and uw(p, 10, 0.2, p, None, p, None) == -1
    assert mean_b(p, 3, 10, 2, 0.2, 5, 1e-3, p, p, None, p, None) == -1
    # sizes
    assert mean(p, -10, 2, 0.2, 5, 1e-3, p, p, p, p, None) == -2
    assert pca(p, 10, 2, 0.2, -1, 1e-2, None, p, p, p, p, None) == -2
    assert cov(p, 10, 0, 0.2, 5, 1e-2, p, p, p, p, None) == -2
    assert uw(p, 0, 0.2, p, p, p, None) == -2
    assert cov_b(p, 0, 10, 2, 0.2, 5, 1e-2, p, p, p, p, None) == -2
    # limits
    assert mean(p, 4097, 2, 0.2, 5, 1e-3, p, p, p, p, None) == -5
    assert pca(p, 100, 9, 0.2, 5, 1e-2, None, p, p, p, p, None) == -5
    assert cov(p, 4096, 5, 0.2, 5, 1e-2, p, p, p, p, None) == -5
    assert uw(p, 4097, 0.2, p, p, p, None) == -5
    assert pca_b(p, (1 << 20) + 1, 10, 2, 0.2, 5, 1e-2, None, p, p, p, p, None) == -5
    # alignment
    assert mean(p + 4, 10, 2, 0.2, 5, 1e-3, p, p, p, p, None) == -3
    assert pca(p, 10, 2, 0.2, 5, 1e-2, p + 4, p, p, p, p, None) == -3
    assert uw(p, 10, 0.2, p, p + 2, p, None) == -3


def test_rrm_argument_errors_need_no_device(lib):
    from rlvi_amd import _lib, rrm
    x = np.random.default_rng(1).standard_normal((50, 2))
    for fn in (rrm.mean, rrm.pca, rrm.covariance):
        for eps in (0.0, 1.0, -0.2, 0.99):                       # 0.99: (1 - eps) n = 0.5 <= 1
            with pytest.raises(ValueError, match="eps"):
                fn(x, eps)
        xb = x.copy()
        xb[3, 1] = np.nan
        with pytest.raises(ValueError, match="NaN or infinity"):
            fn(xb, 0.2)
        with pytest.raises(ValueError, match=r"\[n, d\]"):
            fn(x[:, 0], 0.2)
        for shape in ((4097, 2), (100, 9), (4096, 5), (1, 2)):
            with pytest.raises((_lib.RlviError, ValueError), match="4096.*8.*16384|eps"):
                fn(np.zeros(shape), 0.2)
    with pytest.raises(ValueError, match="theta_init"):
        rrm.pca(x, 0.2, theta_init=np.ones(3))
    for fn in (rrm.mean_batch, rrm.pca_batch, rrm.covariance_batch):
        with pytest.raises(ValueError, match=r"\[B, n, d\]"):
            fn(x, 0.2)
        with pytest.raises(ValueError, match="eps"):
            fn(x[None], 1.0)
        xb = np.stack([x, x, x])
        xb[1, 0, 0] = np.inf
        with pytest.raises(ValueError, match="problem 1"):
            fn(xb, 0.2)
        with pytest.raises(_lib.RlviError, match="4096.*8.*16384"):
            fn(np.zeros((2, 100, 9)), 0.2)
    for eps in (0.0, 1.0):
        with pytest.raises(ValueError, match="eps"):
            rrm.update_weights(np.arange(8.0), eps)
    with pytest.raises(ValueError, match="NaN or infinity"):
        rrm.update_weights(np.array([1.0, np.nan, 2.0]), 0.2)
    with pytest.raises(ValueError):
        rrm.update_weights(np.zeros((3, 3)), 0.2)
    with pytest.raises(_lib.RlviError, match="4096"):
        rrm.update_weights(np.zeros(4097), 0.2)
