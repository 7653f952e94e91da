"""Mean, PCA and covariance in one launch (rlvi_amd/csrc/moments.hip) on the GPU: every case of the reference in
tests/golden/g16_moments.npz, the constrained E-step on its own, the unchanged defaults, the shapes at which the
kernel takes another path, a cloud far from the origin, outliers at 1e6 sigma, maxiter=0, errors, determinism and
graph capture.

The bars: against the numpy restatement tests/moments_ref.py (the same algorithm, only the order of the sums
differs) theta at rtol 1e-8 and the weights at rtol 1e-6 / atol 1e-300 -- what linear_regression and
logistic_regression hold against theirs; against the reference's own theta the bars of G7 (tests/test_gpu_parity.py:
mean 1e-9 / 1e-12, pca 1e-7 / 1e-10, covariance 1e-6 / 1e-9).  Each test prints its figures before it asserts."""
import os

import numpy as np
import pytest

import moments_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G16 = np.load(os.path.join(GOLDEN, "g16_moments.npz"))
G7 = np.load(os.path.join(GOLDEN, "g7_estimators.npz"))
CASES = [str(k) for k in G16["cases"]]
COV_CASES = [k for k in CASES if k.startswith("cov_")]
COV_EPS = float(G16["cov_eps"])
BARS = {"mean": (1e-9, 1e-12), "pca": (1e-7, 1e-10), "cov": (1e-6, 1e-9)}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rlvi_amd import _lib, ops
    _lib.load()
    return torch, ops, torch.device("cuda:0")


@pytest.fixture(autouse=True)
def no_sticky_status_left_behind():
    yield
    import torch
    if torch.cuda.is_available():
        from rlvi_amd import ops
        assert ops.workspace(torch.device("cuda:0")).status() == 0


def ref_estimator(kind, x, theta_init=None, eps=COV_EPS, **kw):
    if kind == "mean":
        return R.mean(x, **kw)
    if kind == "pca":
        return R.pca(x, theta_init=theta_init, **kw)
    return R.covariance(x, eps, **kw)


def one_launch(kind, x, theta_init=None, eps=COV_EPS, **kw):
    from rlvi_amd import standard
    if kind == "mean":
        return standard.mean(x, one_launch=True, return_info=True, **kw)
    if kind == "pca":
        return standard.pca(x, theta_init=theta_init, one_launch=True, return_info=True, **kw)
    return standard.covariance(x, eps, one_launch=True, return_info=True, **kw)


_ref_runs = {}


def ref_run(key):
    """The restatement's estimator on a G16 case, computed once: (theta, weights, outer, trace)."""
    if key not in _ref_runs:
        init = G16[key + "/theta_init"] if key + "/theta_init" in G16 else None
        _ref_runs[key] = ref_estimator(key.split("_")[0], G16[key + "/sample"].astype(np.float64), theta_init=init)
    return _ref_runs[key]


def against_restatement(what, theta, w, th_ref, w_ref):
    print(f"    {what}: |theta - moments_ref's| / |.| = {np.linalg.norm(theta - th_ref) / np.linalg.norm(th_ref):.3e}, "
          f"max |w - moments_ref's| = {np.max(np.abs(w - w_ref)):.3e}")
    np.testing.assert_allclose(theta, th_ref, rtol=1e-8)
    np.testing.assert_allclose(w, w_ref, rtol=1e-6, atol=1e-300)


@pytest.mark.parametrize("key", CASES)
def test_every_g16_case_in_one_launch(key, gpu):
    kind = key.split("_")[0]
    x = G16[key + "/sample"].astype(np.float64)
    init = G16[key + "/theta_init"] if key + "/theta_init" in G16 else None
    theta, w, info = one_launch(kind, x, theta_init=init)
    th_ref, w_ref, outer_ref, _ = ref_run(key)
    ref = G16[key + "/theta"]
    print(f"{key}: info {info.tolist()} (fixture outer {int(G16[key + '/outer'])}), |theta - reference's| / |.| = "
          f"{np.linalg.norm(theta - ref) / np.linalg.norm(ref):.3e}")
    assert info[0] == int(G16[key + "/outer"]) == outer_ref and info[3] == 0
    against_restatement(key, theta, w, th_ref, w_ref)
    np.testing.assert_allclose(theta, ref, rtol=BARS[kind][0], atol=BARS[kind][1])
    if kind == "cov":
        assert info[2] == int(G16[key + "/estep_active"].sum())
    theta2, w2, info2 = one_launch(kind, x, theta_init=init)
    assert np.array_equal(theta, theta2) and np.array_equal(w, w2) and np.array_equal(info, info2)


def dev_uwc(gpu, losses, n_eff):
    torch, ops, dev = gpu
    w, info = ops.update_weights_constrained(torch.from_numpy(np.ascontiguousarray(losses, np.float64)).to(dev), n_eff)
    return w.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("key", COV_CASES + ["g7_uwc"])
def test_constrained_estep_on_its_own(key, gpu):
    """ops.update_weights_constrained on every E-step the reference's covariance made, and on G7's uwc/*: the
    reference's weights at rtol 1e-6; where the constraint was active the weights sum to n_eff."""
    if key == "g7_uwc":
        steps = [(G7["uwc/losses"], G7["uwc/w"], None)]
        n_eff = float(G7["uwc/n_eff"])
    else:
        steps = list(zip(G16[key + "/estep_losses"], G16[key + "/estep_w"], G16[key + "/estep_active"]))
        n_eff = steps[0][0].shape[0] * (1 - COV_EPS)
    for k, (l_in, w_ref, active) in enumerate(steps):
        w, info = dev_uwc(gpu, l_in, n_eff)
        n = l_in.shape[0]
        print(f"{key} E-step {k}: info {info.tolist()}, max relative distance to the reference's weights "
              f"{np.max(np.abs(w - w_ref) / np.maximum(w_ref, 1e-300)):.3e}, sum w - n_eff = {w.sum() - n_eff:.3e}")
        assert info[3] == 0
        if active is not None:
            assert info[2] == int(active)
        np.testing.assert_allclose(w, w_ref, rtol=1e-6, atol=1e-300)
        if info[2] == 1:
            assert abs(w.sum() - n_eff) <= 1e-9 * n
            assert 1 <= info[0] <= 200
        w_r, act_r = R.update_weights_constrained(l_in, n_eff)
        assert act_r == bool(info[2])
        np.testing.assert_allclose(w, w_r, rtol=1e-9, atol=1e-300)


def parent_mean(sample, maxiter=100, tol=1e-3):
    """The body standard.mean had before it got `one_launch`, statement for statement, on the pieces it is made of:
    what the default must still return, bit for bit.  (parent_pca, parent_covariance: the same.)"""
    from rlvi_amd import standard
    sample = np.asarray(sample, np.float64)
    w = np.ones(sample.shape[0])
    theta = w @ sample / np.sum(w)
    losses = standard._gauss_losses(sample, theta, w)
    for _ in range(maxiter):
        w = standard.update_weights(losses)
        prev = theta.copy()
        theta = w @ sample / np.sum(w)
        losses = standard._gauss_losses(sample, theta, w)
        if np.linalg.norm(theta - prev) / np.linalg.norm(prev) <= tol:
            break
    return theta


def parent_pca(sample, maxiter=100, tol=1e-2):
    from rlvi_amd import standard
    sample = np.asarray(sample, np.float64)
    w = np.ones(sample.shape[0])
    theta, losses = standard._pca_step(sample, w)
    for _ in range(maxiter):
        w = standard.update_weights(losses)
        prev = theta.copy()
        theta, losses = standard._pca_step(sample, w)
        if np.linalg.norm(theta - prev) / np.linalg.norm(prev) <= tol:
            break
    return theta


def parent_covariance(sample, eps, maxiter=100, tol=1e-2):
    from rlvi_amd import standard
    sample = np.asarray(sample, np.float64)
    n = sample.shape[0]
    n_eff = n * (1 - eps)
    w = np.ones(n)
    theta, losses = standard._cov_step(sample, w)
    for _ in range(maxiter):
        w = standard.update_weights_constrained(losses, n_eff)
        prev = theta.copy()
        theta, losses = standard._cov_step(sample, w)
        if np.linalg.norm(theta - prev, ord='fro') / np.linalg.norm(prev, ord='fro') <= tol:
            break
    return theta


@pytest.mark.parametrize("size", [60, 200])
def test_defaults_are_unchanged_and_theta_init_on_the_default_path(size, gpu):
    from rlvi_amd import standard, synth
    x = synth.heavy_tail_cloud(size=size, eps=0.2, seed=int(G7[f"seed_{size}"]))
    assert np.array_equal(standard.mean(x), parent_mean(x))
    assert np.array_equal(standard.pca(x), parent_pca(x))
    assert np.array_equal(standard.covariance(x, eps=0.4), parent_covariance(x, 0.4))
    assert np.array_equal(standard.pca(x, 100, 1e-2, None), parent_pca(x))
    with pytest.raises(ValueError):
        standard.mean(x, return_info=True)                  # (the host loop keeps no info)
    # theta_init on the default path: the restatement's outer count (seen through update_weights), its theta
    t = np.array([0.1, 1.0])
    t /= np.linalg.norm(t)
    calls = []
    orig = standard.update_weights
    standard.update_weights = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        theta = standard.pca(x, theta_init=t)
    finally:
        standard.update_weights = orig
    th_ref, _, outer_ref, _ = R.pca(x, theta_init=t)
    print(f"pca({size} x 2, theta_init) on the default path: outer {len(calls)} (restatement {outer_ref}), "
          f"max |theta - restatement's| = {np.max(np.abs(theta - th_ref)):.3e}")
    assert len(calls) == outer_ref
    np.testing.assert_allclose(theta, th_ref, rtol=1e-7, atol=1e-10)
    # and the one launch takes the same count
    th1, _, info = standard.pca(x, theta_init=t, one_launch=True, return_info=True)
    assert info[0] == outer_ref
    np.testing.assert_allclose(th1, th_ref, rtol=1e-8)


def shape_cloud(n, d):
    """A contaminated cloud: column c of standard deviation 2^(-c/2) about c / 2, a fifth of the rows' deviations
    divided by sqrt(chi2_1.5 / 1.5).  (2, 1): the rows 2 and 0 -- with two samples every estimator's second fit equals
    its first whatever they are, and on these two every sum is exact, so that the device and the restatement see the
    same zero discrepancy.)"""
    if n == 2:
        return np.array([[2.0], [0.0]])[:, :d]
    rng = np.random.default_rng(1000 * n + d)
    dev = rng.standard_normal((n, d)) * 2.0 ** (-0.5 * np.arange(d))
    k = max(1, n // 5)
    dev[:k] /= np.sqrt(rng.chisquare(1.5, k) / 1.5)[:, None]
    return dev + 0.5 * np.arange(d)


# two samples; one past a 16-row block; around a wave's 64; 256 | 257: one and two samples per thread; d = 2 | 3, 4 | 5:
# the padded sizes 2 / 4 / 8 of the d x d algebra; 1024 | 1025: four and sixteen samples per thread; the limits
# n d = 16 384 at d = 8 and d = 4, and n = 4096 at d = 1
SHAPES = [(2, 1), (17, 2), (63, 2), (64, 3), (65, 2), (256, 2), (257, 4), (1024, 8), (1025, 5), (2048, 8), (4096, 4),
          (4096, 1)]


@pytest.mark.parametrize("n,d", SHAPES)
def test_shapes_that_take_another_path(n, d, gpu):
    x = shape_cloud(n, d)
    for kind in ("mean", "pca", "cov"):
        theta, w, info = one_launch(kind, x, maxiter=2, tol=0.0)
        th_ref, w_ref, outer_ref, trace = ref_estimator(kind, x, maxiter=2, tol=0.0)
        print(f"{n} x {d} {kind}: info {info.tolist()}, restatement's outer {outer_ref}, trace {trace}")
        assert info[0] == outer_ref and info[3] == 0 and 1 <= info[1] <= 100
        against_restatement(f"{n} x {d} {kind}", theta, w, th_ref, w_ref)


def test_a_cloud_far_from_the_origin(gpu):
    """1e6 (1, 1) + N(0, I), n = 200: mean and covariance within 1e-8 of the restatement -- and of the same cloud at
    the origin, which one-pass moments (S2 - m m^T keeps four digits here) would miss."""
    rng = np.random.default_rng(5)
    dev = rng.standard_normal((200, 2))
    x = 1e6 + dev
    th, w, info = one_launch("mean", x)
    th_ref, w_ref, outer_ref, _ = R.mean(x)
    assert info[0] == outer_ref and info[3] == 0
    against_restatement("mean at 1e6", th, w, th_ref, w_ref)
    cov, wc, info = one_launch("cov", x)
    cov_ref, wc_ref, outer_ref, _ = R.covariance(x, COV_EPS)
    assert info[0] == outer_ref and info[3] == 0
    against_restatement("covariance at 1e6", cov, wc, cov_ref, wc_ref)
    cov0 = one_launch("cov", x - 1e6)[0]
    print(f"covariance at 1e6 vs at the origin: {np.linalg.norm(cov - cov0) / np.linalg.norm(cov0):.3e}")
    np.testing.assert_allclose(cov, cov0, rtol=1e-8)


def outlier_cloud(kind):
    """190 samples about (5, 10) along (1, 2) / sqrt 5 and ten outliers 1e6 sigma away.  pca: across that axis (an
    outlier ON the axis has the loss 0 and is no outlier to this estimator).  mean, covariance: in ten directions
    around the circle -- outliers on ONE line make the first, unit-weight covariance a matrix of condition 1e12, whose
    Mahalanobis distances no two summation orders compute alike to eight digits; spread out, every covariance of the
    run is well conditioned and the comparison with the restatement means something."""
    rng = np.random.default_rng(9)
    z = rng.standard_normal(200)
    x = np.column_stack([z, 2 * z + 0.25 * rng.standard_normal(200)]) + np.array([5.0, 10.0])
    far = 1e6 * (1 + 0.1 * rng.random(10))[:, None]
    if kind == "pca":
        dirs = np.where(np.arange(10) % 2 == 0, 1.0, -1.0)[:, None] * np.array([2.0, -1.0]) / np.sqrt(5.0)
    else:
        ang = 2 * np.pi * (np.arange(10) + 0.3) / 10
        dirs = np.column_stack([np.cos(ang), np.sin(ang)])
    x[:10] = np.array([5.0, 10.0]) + far * dirs
    return x


def test_outliers_at_1e6_sigma_get_the_weight_zero(gpu):
    """Losses of about 1e12: exp underflows, every form has to be the overflow-safe one.  All outputs finite, the
    outliers' weights exactly 0, flag 0, and the restatement's results."""
    t = np.array([0.1, 1.0])
    t /= np.linalg.norm(t)
    for kind in ("mean", "pca", "cov"):
        x = outlier_cloud(kind)
        theta, w, info = one_launch(kind, x, theta_init=t if kind == "pca" else None)
        th_ref, w_ref, outer_ref, _ = ref_estimator(kind, x, theta_init=t if kind == "pca" else None)
        print(f"outliers, {kind}: info {info.tolist()}, theta {theta.ravel()}, outliers' weights {w[:10]}")
        assert info[3] == 0 and info[0] == outer_ref
        assert np.isfinite(theta).all() and np.isfinite(w).all()
        assert np.array_equal(w[:10], np.zeros(10)) and np.array_equal(w_ref[:10], np.zeros(10))
        against_restatement(f"outliers {kind}", theta, w, th_ref, w_ref)
    # the E-step on its own at losses of 1e12
    losses = np.concatenate([np.full(10, 1e12), np.linspace(0.5, 3.0, 90)])
    w, info = dev_uwc(gpu, losses, 60.0)
    assert info[3] == 0 and info[2] == 1 and np.isfinite(w).all() and np.array_equal(w[:10], np.zeros(10))
    assert abs(w.sum() - 60.0) <= 1e-9 * 100
    np.testing.assert_allclose(w, R.update_weights_constrained(losses, 60.0)[0], rtol=1e-9, atol=1e-300)


def test_maxiter_zero_is_the_unit_weight_fit(gpu):
    x = shape_cloud(200, 3)
    n = x.shape[0]
    theta, w, info = one_launch("mean", x, maxiter=0)
    assert info[0] == 0 and info[3] == 0 and np.array_equal(w, np.ones(n))
    np.testing.assert_allclose(theta, x.mean(0), rtol=1e-13)
    theta, w, info = one_launch("pca", x, maxiter=0)
    assert info[0] == 0 and info[3] == 0 and np.array_equal(w, np.ones(n))
    np.testing.assert_allclose(theta, R._pca_fit(x, np.ones(n)), rtol=1e-8)
    theta, w, info = one_launch("cov", x, maxiter=0)
    assert info[0] == 0 and info[3] == 0 and np.array_equal(w, np.ones(n))
    np.testing.assert_allclose(theta, np.cov(x.T, bias=True), rtol=1e-12)


def test_errors(gpu):
    torch, ops, dev = gpu
    from rlvi_amd import _lib, standard
    x = shape_cloud(200, 2)
    ws = ops.workspace(dev)
    for bad in (np.nan, np.inf):
        xb = x.copy()
        xb[3, 1] = bad
        for kind in ("mean", "pca", "cov"):
            with pytest.raises(ValueError):
                one_launch(kind, xb)
        assert ws.status() == 0
    for shape in ((4097, 2), (100, 9), (4096, 5)):
        for kind in ("mean", "pca", "cov"):
            with pytest.raises(_lib.RlviError, match="4096.*8.*16384"):
                one_launch(kind, np.zeros(shape))
    with pytest.raises(ValueError, match="Singular covariance matrix"):
        standard.covariance(np.column_stack([x[:, 0], x[:, 0]]), 0.4, one_launch=True)
    for eps in (0.0, 1.0):
        with pytest.raises(ValueError):
            standard.covariance(x, eps, one_launch=True)
    assert ws.status() == 0
    # the C entries themselves, handed what the Python layer refuses: flag 1, nothing written
    xb = x.copy()
    xb[3, 1] = np.nan
    xd = torch.from_numpy(xb).to(dev)
    for fn, numel, args in ((ops.robust_mean, 2, ()), (ops.robust_pca, 2, ()), (ops.robust_covariance, 4, (120.0,))):
        theta = torch.full((numel,), 7.0, dtype=torch.float64, device=dev)
        w = torch.full((200,), 7.0, dtype=torch.float64, device=dev)
        _, _, info = fn(xd, *args, theta=theta, weights=w)
        assert info.cpu().numpy()[3] == 1 and bool((theta == 7.0).all()) and bool((w == 7.0).all())
    for n_eff in (0.0, 200.0, 250.0):
        theta = torch.full((4,), 7.0, dtype=torch.float64, device=dev)
        _, _, info = ops.robust_covariance(torch.from_numpy(x).to(dev), n_eff, theta=theta)
        assert info.cpu().numpy()[3] == 1 and bool((theta == 7.0).all())
    out = torch.full((100,), 7.0, dtype=torch.float64, device=dev)
    _, info = ops.update_weights_constrained(torch.full((100,), float("nan"), dtype=torch.float64, device=dev), 60.0,
                                             out=out)
    assert info.cpu().numpy()[3] == 1 and bool((out == 7.0).all())
    assert ws.status() == 0


def test_same_bits_twice_and_under_graph_capture(gpu):
    torch, ops, dev = gpu
    x = G16["cov_cloud_1024x4/sample"].astype(np.float64)
    n, d = x.shape
    n_eff = n * (1 - COV_EPS)
    xd = torch.from_numpy(x).to(dev)
    a = [t.cpu().numpy() for t in ops.robust_covariance(xd, n_eff)]
    b = [t.cpu().numpy() for t in ops.robust_covariance(xd, n_eff)]
    assert all(np.array_equal(p, q) for p, q in zip(a, b)) and a[2][3] == 0 and a[2][0] >= 1
    theta = torch.zeros(d, d, dtype=torch.float64, device=dev)
    w = torch.zeros(n, dtype=torch.float64, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ws = ops.Workspace(dev, n, 0)
        ops.robust_covariance(xd, n_eff, theta=theta, weights=w, info=info, ws=ws)      # (warm-up outside the capture)
        torch.cuda.synchronize()
        theta.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ops.robust_covariance(xd, n_eff, theta=theta, weights=w, info=info, ws=ws)
        g.replay()
        torch.cuda.synchronize()
    assert np.array_equal(theta.cpu().numpy(), a[0]) and np.array_equal(w.cpu().numpy(), a[1])
    assert np.array_equal(info.cpu().numpy(), a[2]) and ws.status() == 0
