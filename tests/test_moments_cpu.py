"""Mean, PCA and covariance in one launch (rlvi_amd/csrc/moments.hip), the part that needs no GPU: the numpy
restatement tests/moments_ref.py against every case the reference left in tests/golden/g16_moments.npz, the fixture's
own bookkeeping, the new exports, the limits and the argument errors of the C entries, and the Python signatures.

The bars are those the project already holds against G7 (tests/test_gpu_parity.py,
test_estimators_mean_pca_covariance_golden): mean rtol 1e-9 / atol 1e-12, pca rtol 1e-7 / atol 1e-10, covariance
rtol 1e-6 / atol 1e-9 -- the covariance bar covers what the exact KKT root leaves against scipy's Brent search on
its square (at most 6.7e-9 relative on 120 rehearsed cases).  Each test prints its distances before it
asserts (pytest -s shows them)."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import moments_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G16 = np.load(os.path.join(GOLDEN, "g16_moments.npz"))
CASES = [str(k) for k in G16["cases"]]
BARS = {"mean": (1e-9, 1e-12), "pca": (1e-7, 1e-10), "cov": (1e-6, 1e-9)}

_ref_runs = {}


def ref_run(key):
    """The restatement's estimator on a G16 case, computed once: (theta, weights, outer, trace, E-steps)."""
    if key not in _ref_runs:
        x = G16[key + "/sample"].astype(np.float64)
        kind = key.split("_")[0]
        steps = []
        if kind == "mean":
            r = R.mean(x)
        elif kind == "pca":
            r = R.pca(x, theta_init=G16[key + "/theta_init"] if key + "/theta_init" in G16 else None)
        else:
            r = R.covariance(x, float(G16["cov_eps"]), steps=steps)
        _ref_runs[key] = r + (steps,)
    return _ref_runs[key]


@pytest.fixture(scope="module")
def lib():
    from rlvi_amd import _build, _lib
    _build.build()
    return _lib.load()


@pytest.mark.parametrize("key", CASES)
def test_restatement_against_every_g16_case(key):
    kind = key.split("_")[0]
    theta, w, outer, trace, steps = ref_run(key)
    ref = G16[key + "/theta"]
    rtol, atol = BARS[kind]
    print(f"{key}: outer {outer} (fixture {int(G16[key + '/outer'])}), max |theta - reference's| = "
          f"{np.max(np.abs(theta - ref)):.3e}, relative {np.linalg.norm(theta - ref) / np.linalg.norm(ref):.3e}")
    assert outer == int(G16[key + "/outer"])
    assert theta.shape == ref.shape
    np.testing.assert_allclose(theta, ref, rtol=rtol, atol=atol)
    np.testing.assert_allclose(trace, G16[key + "/trace"], rtol=1e-4, atol=1e-9)
    if kind == "cov":
        active = G16[key + "/estep_active"]
        assert len(active) == outer == len(G16[key + "/estep_losses"])
        for k, (l_in, w_ref) in enumerate(zip(G16[key + "/estep_losses"], G16[key + "/estep_w"])):
            w_k, act = R.update_weights_constrained(l_in, l_in.shape[0] * (1 - float(G16["cov_eps"])))
            print(f"    E-step {k}: active {act}, max relative weight distance "
                  f"{np.max(np.abs(w_k - w_ref) / np.maximum(w_ref, 1e-300)):.3e}")
            assert act == bool(active[k])
            np.testing.assert_allclose(w_k, w_ref, rtol=1e-6, atol=1e-300)
            if act:
                assert abs(w_k.sum() - 0.6 * l_in.shape[0]) <= 1e-9 * l_in.shape[0]


def test_fixture_records_its_seed_bookkeeping():
    tried, kept = (int(v) for v in G16["seeds_tried_kept"])
    assert kept == len(CASES) and tried >= kept and tried - kept <= 0.1 * tried
    kinds = [k.split("_")[0] for k in CASES]
    assert kinds.count("mean") == 9 and kinds.count("pca") == 9 and kinds.count("cov") == 6
    for key in CASES:
        assert G16[key + "/sample"].ndim == 2 and int(G16[key + "/outer"]) >= 1


def test_new_exports_exist(lib):
    from rlvi_amd import _lib, ops
    for name in ("rlvi_moments_check", "rlvi_robust_mean_f64", "rlvi_robust_pca_f64", "rlvi_robust_covariance_f64",
                 "rlvi_update_weights_constrained_f64"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for name in ("robust_mean", "robust_pca", "robust_covariance", "update_weights_constrained", "moments_check"):
        assert callable(getattr(ops, name))
    assert lib.rlvi_abi_version() == 3


def test_limits_are_answered_without_a_device(lib):
    assert lib.rlvi_moments_check(4096, 4) == 0
    assert lib.rlvi_moments_check(4096, 5) == -5          # n d > 16384
    assert lib.rlvi_moments_check(2048, 8) == 0
    assert lib.rlvi_moments_check(2049, 8) == -5
    assert lib.rlvi_moments_check(1, 2) == -5             # n < 2
    assert lib.rlvi_moments_check(100, 9) == -5           # d > 8
    assert lib.rlvi_moments_check(2, 1) == 0 and lib.rlvi_moments_check(4097, 1) == -5
    assert lib.rlvi_moments_check(0, 2) == -2 and lib.rlvi_moments_check(10, 0) == -2
    assert lib.rlvi_moments_check(-3, 2) == -2


def test_argument_errors_are_answered_without_a_device(lib):
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255
    mean, pca, cov, uwc = (lib.rlvi_robust_mean_f64, lib.rlvi_robust_pca_f64, lib.rlvi_robust_covariance_f64,
                           lib.rlvi_update_weights_constrained_f64)
    # NULL
    assert mean(None, 10, 2, 5, 1e-3, 1e-3, 100, p, p, p, p, None) == -1
    assert mean(p, 10, 2, 5, 1e-3, 1e-3, 100, None, p, p, p, None) == -1
    assert pca(p, 10, 2, 5, 1e-2, None, 1e-3, 100, p, None, p, p, None) == -1
    assert cov(p, 10, 2, 6.0, 5, 1e-2, 1e-3, 100, p, p, None, p, None) == -1
    assert cov(p, 10, 2, 6.0, 5, 1e-2, 1e-3, 100, p, p, p, None, None) == -1
    assert uwc(None, 10, 6.0, 1e-3, 100, p, p, p, None) == -1 and uwc(p, 10, 6.0, 1e-3, 100, None, p, p, None) == -1
    # sizes
    assert mean(p, -10, 2, 5, 1e-3, 1e-3, 100, p, p, p, p, None) == -2
    assert mean(p, 10, 0, 5, 1e-3, 1e-3, 100, p, p, p, p, None) == -2
    assert pca(p, 10, 2, -1, 1e-2, None, 1e-3, 100, p, p, p, p, None) == -2
    assert cov(p, 10, 2, 6.0, 5, 1e-2, 1e-3, -1, p, p, p, p, None) == -2
    assert uwc(p, 0, 6.0, 1e-3, 100, p, p, p, None) == -2 and uwc(p, 10, 6.0, 1e-3, -1, p, p, p, None) == -2
    # limits
    assert mean(p, 4097, 2, 5, 1e-3, 1e-3, 100, p, p, p, p, None) == -5
    assert pca(p, 100, 9, 5, 1e-2, None, 1e-3, 100, p, p, p, p, None) == -5
    assert cov(p, 4096, 5, 6.0, 5, 1e-2, 1e-3, 100, p, p, p, p, None) == -5
    assert uwc(p, 4097, 6.0, 1e-3, 100, p, p, p, None) == -5
    # alignment
    assert mean(p + 4, 10, 2, 5, 1e-3, 1e-3, 100, p, p, p, p, None) == -3
    assert pca(p, 10, 2, 5, 1e-2, p + 4, 1e-3, 100, p, p, p, p, None) == -3
    assert uwc(p, 10, 6.0, 1e-3, 100, p, p + 2, p, None) == -3


def test_signatures_keep_the_reference_positions_and_the_defaults():
    from rlvi_amd import standard
    E = inspect.Parameter.empty
    sig = inspect.signature(standard.pca)
    assert [(p.name, p.default) for p in sig.parameters.values()][:4] == [
        ("sample", E), ("maxiter", 100), ("tol", 1e-2), ("theta_init", None)]
    assert sig.parameters["theta_init"].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD
    sig_m, sig_c = inspect.signature(standard.mean), inspect.signature(standard.covariance)
    assert [(p.name, p.default) for p in sig_m.parameters.values()][:3] == [("sample", E), ("maxiter", 100), ("tol", 1e-3)]
    assert [(p.name, p.default) for p in sig_c.parameters.values()][:4] == [
        ("sample", E), ("eps", E), ("maxiter", 100), ("tol", 1e-2)]
    for s in (sig, sig_m, sig_c):
        for name in ("one_launch", "return_info"):
            assert s.parameters[name].default is False and s.parameters[name].kind == inspect.Parameter.KEYWORD_ONLY


def test_restatement_two_pass_moments_hold_at_an_offset_of_1e6():
    """What the two passes are for: a cloud at 1e6 (1, 1) with unit covariance keeps its covariance to 1e-9, where
    S2 - m m^T keeps four digits."""
    rng = np.random.default_rng(3)
    dev = rng.standard_normal((200, 2))
    w = 0.5 + 0.5 * rng.random(200)
    _, _, s2_far = R.moments(1e6 + dev, w)
    _, _, s2_near = R.moments(dev, w)
    print(f"two-pass at 1e6: relative distance {np.linalg.norm(s2_far - s2_near) / np.linalg.norm(s2_near):.3e}")
    np.testing.assert_allclose(s2_far, s2_near, rtol=1e-9)
