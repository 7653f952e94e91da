"""Robust Risk Minimization's mean, PCA and covariance in one launch (rlvi_amd/csrc/moments.hip, MODE 3 .. 5) on the
GPU: every case of the reference in tests/golden/g18_rrm.npz, the weight rule on its own, the shapes at which the kernel
takes another path, a cloud far from the origin, outliers at 1e6 sigma, negative losses, the no-root limit, maxiter=0,
errors, the batch forms, determinism and graph capture.

The bars: against the numpy restatement tests/rrm_ref.py (the same algorithm, only the order of the sums differs)
theta at rtol 1e-8 and the weights at rtol 1e-6 / atol 1e-300 -- what the other one-workgroup estimators hold against
theirs; the weight rule on its own at rtol 1e-9 / atol 1e-300, as update_weights_constrained; against the reference's
own theta the bars of G7 (mean 1e-9 / 1e-12, pca 1e-7 / 1e-10, covariance 1e-6 / 1e-9); against the reference's
weights rtol 10 x w_bar, w_bar the largest relative distance the fixture's generator measured between the exact root's
weights and the reference's (Brent's tolerance times l / alpha), as in tests/test_rrm_cpu.py.  Each test prints its
figures before it asserts."""
import os

import numpy as np
import pytest

import rrm_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G18 = np.load(os.path.join(GOLDEN, "g18_rrm.npz"))
CASES = [str(k) for k in G18["cases"]]
ONLY = dict(zip(CASES, (bool(v) for v in G18["restatement_only"])))
STEP_CASES = [k for k in CASES if k + "/estep_losses" in G18]
W_BAR = float(G18["w_bar"])
BARS = {"mean": (1e-9, 1e-12), "pca": (1e-7, 1e-10), "cov": (1e-6, 1e-9)}
ROOT_CAP = 200                                                       # MO_ROOT_CAP
KINDS = ("mean", "pca", "cov")


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


def ref_estimator(kind, x, eps, theta_init=None, **kw):
    if kind == "mean":
        return R.mean(x, eps, **kw)
    if kind == "pca":
        return R.pca(x, eps, theta_init=theta_init, **kw)
    return R.covariance(x, eps, **kw)


def one_launch(kind, x, eps, theta_init=None, **kw):
    from rlvi_amd import rrm
    if kind == "mean":
        return rrm.mean(x, eps, return_info=True, **kw)
    if kind == "pca":
        return rrm.pca(x, eps, theta_init=theta_init, return_info=True, **kw)
    return rrm.covariance(x, eps, return_info=True, **kw)


_ref_runs = {}


def ref_run(key):
    """The restatement's estimator on a G18 case, computed once: (theta, weights, outer, trace)."""
    if key not in _ref_runs:
        init = G18[key + "/theta_init"] if key + "/theta_init" in G18 else None
        _ref_runs[key] = ref_estimator(key.split("_")[0], G18[key + "/sample"].astype(np.float64),
                                       float(G18[key + "/eps"]), theta_init=init)
    return _ref_runs[key]


def against_restatement(what, theta, w, th_ref, w_ref):
    print(f"    {what}: |theta - rrm_ref's| / |.| = {np.linalg.norm(theta - th_ref) / np.linalg.norm(th_ref):.3e}, "
          f"max |w - rrm_ref's| = {np.max(np.abs(w - w_ref)):.3e}")
    np.testing.assert_allclose(theta, th_ref, rtol=1e-8)
    np.testing.assert_allclose(w, w_ref, rtol=1e-6, atol=1e-300)


@pytest.mark.parametrize("key", CASES)
def test_every_g18_case_in_one_launch(key, gpu):
    kind = key.split("_")[0]
    x = G18[key + "/sample"].astype(np.float64)
    eps = float(G18[key + "/eps"])
    init = G18[key + "/theta_init"] if key + "/theta_init" in G18 else None
    theta, w, info = one_launch(kind, x, eps, theta_init=init)
    th_ref, w_ref, outer_ref, _ = ref_run(key)
    ref = G18[key + "/theta"]
    print(f"{key}: info {info.tolist()} (fixture outer {int(G18[key + '/outer'])}), |theta - reference's| / |.| = "
          f"{np.linalg.norm(theta - ref) / np.linalg.norm(ref):.3e}")
    assert info[0] == int(G18[key + "/outer"]) == outer_ref and info[3] == 0
    assert 1 <= info[1] <= ROOT_CAP
    against_restatement(key, theta, w, th_ref, w_ref)
    if not ONLY[key]:
        np.testing.assert_allclose(theta, ref, rtol=BARS[kind][0], atol=BARS[kind][1])
    theta2, w2, info2 = one_launch(kind, x, eps, theta_init=init)
    assert np.array_equal(theta, theta2) and np.array_equal(w, w2) and np.array_equal(info, info2)


def dev_rule(gpu, losses, eps, **kw):
    torch, ops, dev = gpu
    w, info = ops.rrm_update_weights(torch.from_numpy(np.ascontiguousarray(losses, np.float64)).to(dev), eps, **kw)
    return w.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("key", STEP_CASES)
def test_weight_rule_on_every_stored_estep(key, gpu):
    """ops.rrm_update_weights on the losses the reference's update_weights was handed in every outer iteration."""
    eps = float(G18[key + "/eps"])
    for k, (l_in, w_ref) in enumerate(zip(G18[key + "/estep_losses"], G18[key + "/estep_w"])):
        w, info = dev_rule(gpu, l_in, eps)
        w_r, _, had_root = R.update_weights(l_in, eps)
        big = w_ref > 1e-300
        print(f"{key} E-step {k}: info {info.tolist()}, relative distance to the restatement's weights "
              f"{np.max(np.abs(w - w_r) / np.maximum(w_r, 1e-300)):.3e}, to the reference's "
              f"{np.max(np.abs(w[big] - w_ref[big]) / w_ref[big]):.3e} (w_bar {W_BAR:.3e}), "
              f"sum w - 1 = {w.sum() - 1:.3e}")
        assert info[3] == 0 and info[2] == int(had_root)
        np.testing.assert_allclose(w, w_r, rtol=1e-9, atol=1e-300)
        np.testing.assert_allclose(w, w_ref, rtol=10 * W_BAR, atol=1e-300)
        assert abs(w.sum() - 1.0) <= 1e-12
        assert 1 <= info[0] <= ROOT_CAP


def shape_cloud(n, d, seed=0):
    """A contaminated cloud: column c of standard deviation 2^(-c/2) about c / 2, a fifth of the rows' deviations
    divided by sqrt(chi2_1.5 / 1.5).  (2, 1): the rows 2 and 0 -- with two samples every estimator's second fit equals
    its first whatever they are, and on these two every sum is exact, so that the device and the restatement see the
    same zero discrepancy.  (The recipe of tests/test_moments_gpu.py; seed: further clouds of a shape, for a batch.)"""
    if n == 2:
        return np.array([[2.0], [0.0]])[:, :d]
    rng = np.random.default_rng(1000 * n + d + 7919 * seed)
    dev = rng.standard_normal((n, d)) * 2.0 ** (-0.5 * np.arange(d))
    k = max(1, n // 5)
    dev[:k] /= np.sqrt(rng.chisquare(1.5, k) / 1.5)[:, None]
    return dev + 0.5 * np.arange(d)


# test_moments_gpu.SHAPES: two samples; one past a 16-row block; around a wave's 64; 256 | 257: one and two samples per
# thread; d = 2 | 3, 4 | 5: the padded sizes 2 / 4 / 8 of the d x d algebra; 1024 | 1025: four and sixteen samples per
# thread; the limits n d = 16 384 at d = 8 and d = 4, and n = 4096 at d = 1
SHAPES = [(2, 1), (17, 2), (63, 2), (64, 3), (65, 2), (256, 2), (257, 4), (1024, 8), (1025, 5), (2048, 8), (4096, 4),
          (4096, 1)]


@pytest.mark.parametrize("n,d", SHAPES)
def test_shapes_that_take_another_path(n, d, gpu):
    x = shape_cloud(n, d)
    eps = 0.25 if n == 2 else 0.2                                   # (2, 1): (1 - eps) n = 1.5 > 1
    for kind in KINDS:
        theta, w, info = one_launch(kind, x, eps, maxiter=2, tol=0.0)
        th_ref, w_ref, outer_ref, trace = ref_estimator(kind, x, eps, maxiter=2, tol=0.0)
        print(f"{n} x {d} {kind}: info {info.tolist()}, restatement's outer {outer_ref}, trace {trace}")
        assert info[0] == outer_ref and info[3] == 0 and 0 <= info[1] <= ROOT_CAP
        against_restatement(f"{n} x {d} {kind}", theta, w, th_ref, w_ref)
        assert abs(w.sum() - 1.0) <= 1e-12


def test_a_cloud_far_from_the_origin(gpu):
    """1e6 (1, 1) + N(0, I), n = 200: mean and covariance within 1e-8 of the restatement -- and the covariance of the
    same cloud at the origin."""
    rng = np.random.default_rng(5)
    x = 1e6 + rng.standard_normal((200, 2))
    th, w, info = one_launch("mean", x, 0.2)
    th_ref, w_ref, outer_ref, _ = R.mean(x, 0.2)
    assert info[0] == outer_ref and info[3] == 0
    against_restatement("mean at 1e6", th, w, th_ref, w_ref)
    cov, wc, info = one_launch("cov", x, 0.2)
    cov_ref, wc_ref, outer_ref, _ = R.covariance(x, 0.2)
    assert info[0] == outer_ref and info[3] == 0
    against_restatement("covariance at 1e6", cov, wc, cov_ref, wc_ref)
    cov0 = one_launch("cov", x - 1e6, 0.2)[0]
    print(f"covariance at 1e6 vs at the origin: {np.linalg.norm(cov - cov0) / np.linalg.norm(cov0):.3e}")
    np.testing.assert_allclose(cov, cov0, rtol=1e-8)


def outlier_cloud(kind):
    """190 samples about (5, 10) along (1, 2) / sqrt 5 and ten outliers 1e6 sigma away.  pca: across that axis (an
    outlier ON the axis has the loss 0); mean, covariance: in ten directions around the circle, so that every
    covariance of the run is well conditioned.  (The recipe of tests/test_moments_gpu.py.)"""
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
    """Losses of about 1e12 beside losses of about 1: exp underflows, l / alpha passes the cut at 800.  All outputs
    finite, the outliers' weights exactly 0, flag 0, and the restatement's results."""
    t = np.array([0.1, 1.0])
    t /= np.linalg.norm(t)
    for kind in KINDS:
        x = outlier_cloud(kind)
        theta, w, info = one_launch(kind, x, 0.2, theta_init=t if kind == "pca" else None)
        th_ref, w_ref, outer_ref, _ = ref_estimator(kind, x, 0.2, theta_init=t if kind == "pca" else None)
        print(f"outliers, {kind}: info {info.tolist()}, theta {theta.ravel()}, outliers' weights {w[:10]}")
        assert info[3] == 0 and info[0] == outer_ref
        assert np.isfinite(theta).all() and np.isfinite(w).all()
        assert np.array_equal(w[:10], np.zeros(10)) and np.array_equal(w_ref[:10], np.zeros(10))
        against_restatement(f"outliers {kind}", theta, w, th_ref, w_ref)
    # the rule on its own at losses of 1e12
    losses = np.concatenate([np.full(10, 1e12), np.linspace(0.5, 3.0, 90)])
    w, info = dev_rule(gpu, losses, 0.4)
    assert info[3] == 0 and info[2] == 1 and np.isfinite(w).all() and np.array_equal(w[:10], np.zeros(10))
    assert abs(w.sum() - 1.0) <= 1e-12
    np.testing.assert_allclose(w, R.update_weights(losses, 0.4)[0], rtol=1e-9, atol=1e-300)


def test_covariance_with_every_loss_negative(gpu):
    """A Gaussian cloud scaled by 1e-4: log det C is about -37 and every loss of every E-step negative (the
    restatement's steps say so) -- the form without the shift by min l would sum exp(+17 / alpha)."""
    rng = np.random.default_rng(11)
    x = 1e-4 * (rng.standard_normal((100, 2)) @ np.array([[1.0, 0.3], [0.0, 0.7]]) + np.array([1.0, -2.0]))
    steps = []
    cov_ref, w_ref, outer_ref, _ = R.covariance(x, 0.2, steps=steps)
    assert steps and all((l < 0.0).all() for l, _, _, _ in steps)
    cov, w, info = one_launch("cov", x, 0.2)
    print(f"negative losses: info {info.tolist()}, largest loss {max(l.max() for l, _, _, _ in steps):.3f}")
    assert info[0] == outer_ref and info[3] == 0 and np.isfinite(cov).all() and np.isfinite(w).all()
    against_restatement("negative losses", cov, w, cov_ref, w_ref)
    # and the rule on its own on the first of them
    w1, info1 = dev_rule(gpu, steps[0][0], 0.2)
    assert info1[3] == 0
    np.testing.assert_allclose(w1, steps[0][1], rtol=1e-9, atol=1e-300)


def test_no_root_limit(gpu):
    """5 minima tied among 8 at eps 0.5 ((1 - eps) n = 4 <= 5), and all-equal losses: 1 / m on the minima, no flag, no
    evaluation."""
    l = np.array([3.0, 1.5, 1.5, 7.0, 1.5, 1.5, 2.0, 1.5])
    w, info = dev_rule(gpu, l, 0.5)
    assert info.tolist() == [0, 0, 0, 0]
    assert np.array_equal(w, np.where(l == 1.5, 0.2, 0.0)) and np.array_equal(w, R.update_weights(l, 0.5)[0])
    for n in (9, 300, 4096):
        w, info = dev_rule(gpu, np.full(n, -4.25), 0.3)
        assert info.tolist() == [0, 0, 0, 0] and np.array_equal(w, np.full(n, 1.0 / n))
    # an estimator on coincident samples but one: every loss of the first fit but one is tied
    x = np.ones((8, 2))
    x[0] = (3.0, 5.0)
    theta, w, info = one_launch("mean", x, 0.5, maxiter=1, tol=0.0)
    th_ref, w_ref, _, _ = R.mean(x, 0.5, maxiter=1, tol=0.0)
    assert info[3] == 0 and info[1] == 0 and np.array_equal(w, w_ref) and w[0] == 0.0
    np.testing.assert_allclose(theta, th_ref, rtol=1e-13)


def test_maxiter_zero_is_the_uniform_weight_fit(gpu):
    x = shape_cloud(200, 3)
    n = x.shape[0]
    theta, w, info = one_launch("mean", x, 0.2, maxiter=0)
    assert info[0] == 0 and info[3] == 0 and np.array_equal(w, np.ones(n) / n)
    np.testing.assert_allclose(theta, x.mean(0), rtol=1e-13)
    theta, w, info = one_launch("pca", x, 0.2, maxiter=0)
    assert info[0] == 0 and info[3] == 0 and np.array_equal(w, np.ones(n) / n)
    np.testing.assert_allclose(theta, R._pca_fit(x, np.ones(n) / n), rtol=1e-8)
    theta, w, info = one_launch("cov", x, 0.2, maxiter=0)
    assert info[0] == 0 and info[3] == 0 and np.array_equal(w, np.ones(n) / n)
    np.testing.assert_allclose(theta, np.cov(x.T, bias=True), rtol=1e-12)


def test_errors(gpu):
    torch, ops, dev = gpu
    from rlvi_amd import _lib, rrm
    x = shape_cloud(200, 2)
    ws = ops.workspace(dev)
    for bad in (np.nan, np.inf):
        xb = x.copy()
        xb[3, 1] = bad
        for kind in KINDS:
            with pytest.raises(ValueError):
                one_launch(kind, xb, 0.2)
        with pytest.raises(ValueError):
            rrm.update_weights(xb[:, 1], 0.2)
    for shape in ((4097, 2), (100, 9), (4096, 5)):
        for kind in KINDS:
            with pytest.raises(_lib.RlviError, match="4096.*8.*16384"):
                one_launch(kind, np.zeros(shape), 0.2)
    with pytest.raises(ValueError, match="Singular covariance matrix"):
        rrm.covariance(np.column_stack([x[:, 0], x[:, 0]]), 0.4)
    for kind in KINDS:
        for eps in (0.0, 1.0, 0.996):                               # 0.996: (1 - eps) n = 0.8 <= 1
            with pytest.raises(ValueError):
                one_launch(kind, x, eps)
    assert ws.status() == 0
    # the C entries themselves, handed what the Python layer refuses: flag 1, nothing written
    xb = x.copy()
    xb[3, 1] = np.nan
    entries = ((ops.rrm_mean, 2), (ops.rrm_pca, 2), (ops.rrm_covariance, 4))
    for xd, epss in ((torch.from_numpy(xb).to(dev), (0.2,)), (torch.from_numpy(x).to(dev), (0.0, 1.0, -0.5, 0.996))):
        for eps in epss:
            for fn, numel in entries:
                theta = torch.full((numel,), 7.0, dtype=torch.float64, device=dev)
                w = torch.full((200,), 7.0, dtype=torch.float64, device=dev)
                _, _, info = fn(xd, eps, theta=theta, weights=w)
                assert info.cpu().numpy()[3] == 1 and bool((theta == 7.0).all()) and bool((w == 7.0).all())
    for losses, eps in ((torch.full((100,), float("nan"), dtype=torch.float64, device=dev), 0.4),
                        (torch.full((100,), float("inf"), dtype=torch.float64, device=dev), 0.4),
                        (torch.arange(100, dtype=torch.float64, device=dev), 0.0),
                        (torch.arange(100, dtype=torch.float64, device=dev), 1.0),
                        (torch.arange(100, dtype=torch.float64, device=dev), 0.995)):
        out = torch.full((100,), 7.0, dtype=torch.float64, device=dev)
        _, info = ops.rrm_update_weights(losses, eps, out=out)
        assert info.cpu().numpy()[3] == 1 and bool((out == 7.0).all())
    assert ws.status() == 0


def batch_of(n, d, B):
    return np.stack([shape_cloud(n, d, seed=b) for b in range(B)])


@pytest.mark.parametrize("B", [3, 70])
@pytest.mark.parametrize("n,d", [(65, 2), (257, 4)])
def test_batch_has_the_bits_of_single_calls(n, d, B, gpu):
    torch, ops, dev = gpu
    X = torch.from_numpy(batch_of(n, d, B)).to(dev)
    t = torch.from_numpy(np.arange(1.0, d + 1.0) / np.linalg.norm(np.arange(1.0, d + 1.0))).to(dev)
    forms = (("mean", ops.rrm_mean_batch, ops.rrm_mean, {}), ("pca", ops.rrm_pca_batch, ops.rrm_pca, {}),
             ("pca, theta_init", ops.rrm_pca_batch, ops.rrm_pca, dict(theta_init=t)),
             ("cov", ops.rrm_covariance_batch, ops.rrm_covariance, {}))
    for what, batch_fn, single_fn, kw in forms:
        th, w, info = (v.cpu().numpy() for v in batch_fn(X, 0.2, **kw))
        assert info.shape == (B, 4) and (info[:, 3] == 0).all() and (info[:, 0] >= 1).all()
        print(f"{what} {B} x {n} x {d}: outer {info[:, 0].min()} .. {info[:, 0].max()}, evaluations of the last "
              f"root-find {info[:, 1].min()} .. {info[:, 1].max()}")
        for b in range(B):
            th1, w1, info1 = (v.cpu().numpy() for v in single_fn(X[b], 0.2, **kw))
            assert np.array_equal(th[b], th1) and np.array_equal(w[b], w1) and np.array_equal(info[b], info1), (what, b)
    # numpy in, numpy out: the same bits again, theta alone by default
    from rlvi_amd import rrm
    th, w, info = rrm.mean_batch(X.cpu().numpy(), 0.2, return_info=True)
    th1, w1, info1 = rrm.mean(X[B - 1].cpu().numpy(), 0.2, return_info=True)
    assert np.array_equal(th[B - 1], th1) and np.array_equal(w[B - 1], w1) and np.array_equal(info[B - 1], info1)
    assert np.array_equal(rrm.mean_batch(X.cpu().numpy(), 0.2), th)


def test_one_problem_with_a_nan_flags_only_itself(gpu):
    torch, ops, dev = gpu
    Xh = batch_of(65, 2, 5)
    clean = torch.from_numpy(Xh).to(dev)
    Xh[3, 10, 1] = np.nan
    dirty = torch.from_numpy(Xh).to(dev)
    for batch_fn, nt in ((ops.rrm_mean_batch, 2), (ops.rrm_pca_batch, 2), (ops.rrm_covariance_batch, 4)):
        th0, w0, info0 = (v.cpu().numpy() for v in batch_fn(clean, 0.2))
        theta = torch.full((5, nt), 7.0, dtype=torch.float64, device=dev)
        w = torch.full((5, 65), 7.0, dtype=torch.float64, device=dev)
        th, w, info = (v.cpu().numpy().reshape(v.shape[0], -1) for v in batch_fn(dirty, 0.2, theta=theta, weights=w))
        assert info[:, 3].tolist() == [0, 0, 0, 1, 0]
        assert (th[3] == 7.0).all() and (w[3] == 7.0).all()
        keep = [0, 1, 2, 4]
        assert np.array_equal(th[keep], th0.reshape(5, -1)[keep]) and np.array_equal(w[keep], w0[keep])
        assert np.array_equal(info[keep], info0[keep])
    from rlvi_amd import rrm
    with pytest.raises(ValueError, match="problem 3"):
        rrm.covariance_batch(Xh, 0.2)
    assert ops.workspace(dev).status() == 0


def test_same_bits_twice_and_under_graph_capture(gpu):
    torch, ops, dev = gpu
    x = G18["cov_cloud_512x4_eps0.2/sample"].astype(np.float64)
    n, d = x.shape
    xd = torch.from_numpy(x).to(dev)
    a = [t.cpu().numpy() for t in ops.rrm_covariance(xd, 0.2)]
    b = [t.cpu().numpy() for t in ops.rrm_covariance(xd, 0.2)]
    assert all(np.array_equal(p, q) for p, q in zip(a, b)) and a[2][3] == 0 and a[2][0] >= 1
    theta = torch.zeros(d, d, dtype=torch.float64, device=dev)
    w = torch.zeros(n, dtype=torch.float64, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ws = ops.Workspace(dev, n, 0)
        ops.rrm_covariance(xd, 0.2, theta=theta, weights=w, info=info, ws=ws)           # (warm-up outside the capture)
        torch.cuda.synchronize()
        theta.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ops.rrm_covariance(xd, 0.2, theta=theta, weights=w, info=info, ws=ws)
        g.replay()
        torch.cuda.synchronize()
    assert np.array_equal(theta.cpu().numpy(), a[0]) and np.array_equal(w.cpu().numpy(), a[1])
    assert np.array_equal(info.cpu().numpy(), a[2]) and ws.status() == 0
