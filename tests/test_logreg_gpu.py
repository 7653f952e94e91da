"""Logistic regression in one launch (rlvi_amd/csrc/logreg.hip) on the GPU: every recorded fit of the reference
(tests/golden/g15_logreg.npz), the whole estimator, the shapes at which the kernel takes another path, extremes,
errors, determinism and graph capture.

The yardstick (tests/test_logreg_cpu.py has the argument): liblinear, the numpy restatement tests/logreg_ref.py and
the kernel minimise the same f, whose Hessian is >= I, so any two answers satisfy
    ||v_a - v_b|| <= ||grad f(v_a)|| + ||grad f(v_b)||
with the gradients evaluated in extended precision by logreg_ref.gradient.  Each test prints its figures before it
asserts (pytest -s shows them)."""
import os

import numpy as np
import pytest

import logreg_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G15 = np.load(os.path.join(GOLDEN, "g15_logreg.npz"))
CASES = [str(k) for k in G15["cases"]]


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


_ref_runs = {}


def ref_run(key):
    """The restatement's estimator on a G15 case, computed once: (theta, weights, outer, trace)."""
    if key not in _ref_runs:
        _ref_runs[key] = R.logistic_regression(G15[key + "/X"].astype(np.float64), G15[key + "/y"])
    return _ref_runs[key]


def gnorm(X, y, w, v):
    return float(np.linalg.norm(R.gradient(X, y, w, v)))


def dev_fit(gpu, X, y, w):
    torch, ops, dev = gpu
    theta, losses, info = ops.logistic_fit(*(torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
                                             for a in (X, y, w)))
    return theta.cpu().numpy(), losses.cpu().numpy(), info.cpu().numpy()


def within_bound(X, y, w, va, vb, what):
    dist, ga, gb = float(np.linalg.norm(va - vb)), gnorm(X, y, w, va), gnorm(X, y, w, vb)
    print(f"    {what}: dist {dist:.3e}  grads {ga:.3e} + {gb:.3e}")
    assert dist <= ga + gb, (what, dist, ga, gb)


@pytest.mark.parametrize("key", CASES)
def test_every_recorded_fit(key, gpu):
    """ops.logistic_fit on the (X, y, w) of every liblinear fit the reference made: the device answer meets
    liblinear's stop criterion (a small gradient) at least as well as liblinear's own, lies within the
    strong-convexity bound of liblinear's and of the restatement's, and its losses are log(1 + exp(Z v_dev))."""
    X, y = G15[key + "/X"].astype(np.float64), G15[key + "/y"]
    Z = R.design(X)
    for k, (w, th_lib) in enumerate(zip(G15[key + "/fit_w"], G15[key + "/fit_theta"])):
        theta, losses, info = dev_fit(gpu, X, y, w)
        assert info[3] == 0 and 1 <= info[2] <= 50, info
        v, v_lib, v_ref = R.to_v(theta), R.to_v(th_lib), R.to_v(R.fit(X, y, w)[0])
        g_dev, g_lib = gnorm(X, y, w, v), gnorm(X, y, w, v_lib)
        print(f"{key} fit {k}: Newton steps {info[2]}, |grad| device {g_dev:.3e}  liblinear {g_lib:.3e}")
        assert g_dev <= g_lib
        within_bound(X, y, w, v, v_lib, "device vs liblinear")
        within_bound(X, y, w, v, v_ref, "device vs logreg_ref")
        np.testing.assert_allclose(losses, np.logaddexp(0, Z @ v), rtol=1e-12)


@pytest.mark.parametrize("key", CASES)
def test_whole_estimator_on_g15(key, gpu):
    """standard.logistic_regression(solver="newton"): the reference's outer count, theta and the final weights at
    the bars linear_regression holds against its oracle (1e-8, 1e-6), and a numpy refit with the returned weights
    within the strong-convexity bound of the returned theta.  The distance to the reference's (liblinear's) theta is
    printed, not asserted: profiles/r15_logreg.md has the figures."""
    from rlvi_amd import standard
    X, y = G15[key + "/X"].astype(np.float64), G15[key + "/y"]
    theta, w, outer = standard.logistic_regression(X, y, solver="newton", return_info=True)
    th_ref, w_ref, outer_ref, _ = ref_run(key)
    th_lib = G15[key + "/theta"]
    print(f"{key}: outer {outer} (fixture {int(G15[key + '/outer'])}), |theta - liblinear's| / |.| = "
          f"{np.linalg.norm(theta - th_lib) / np.linalg.norm(th_lib):.3e}, |theta - logreg_ref's| / |.| = "
          f"{np.linalg.norm(theta - th_ref) / np.linalg.norm(th_ref):.3e}")
    assert outer == int(G15[key + "/outer"]) == outer_ref
    np.testing.assert_allclose(theta, th_ref, rtol=1e-8)
    np.testing.assert_allclose(w, w_ref, rtol=1e-6, atol=1e-300)
    within_bound(X, y, w, R.to_v(theta), R.to_v(R.fit(X, y, w)[0]), "returned theta vs numpy refit")
    assert np.array_equal(standard.logistic_regression(X, y, solver="newton"), theta)


def parent_logistic_regression(gpu, X, y, maxiter=100, tol=1e-2):
    """The body standard.logistic_regression had before it got a `solver`, statement for statement, on the pieces it
    is made of (a liblinear fit on the host, the losses and the E-step on the device): what the default must still
    return, bit for bit."""
    torch, ops, dev = gpu
    from rlvi_amd import standard
    Xh = np.ascontiguousarray(X, dtype=np.float64)
    yh = np.asarray(y)
    Xd = torch.from_numpy(Xh).to(dev)
    w = torch.ones(Xh.shape[0], dtype=torch.float64, device=dev)
    theta, losses = standard._sklearn_log_reg(Xh, yh, Xd, w)
    for _ in range(maxiter):
        w, _ = ops.update_weights_f64(losses)
        prev = theta.copy()
        theta, losses = standard._sklearn_log_reg(Xh, yh, Xd, w)
        if np.linalg.norm(theta - prev) / np.linalg.norm(prev) <= tol:
            break
    return theta


def test_g5_newton_within_the_liblinear_bar_and_default_unchanged(gpu):
    """G5 logreg/*: solver="newton" lies within the bar the liblinear path is held to (tests/test_gpu_parity.py:
    rtol=1e-3, atol=1e-4), takes the restatement's outer count; the default is still liblinear: the same bits as
    solver="liblinear" and as the loop the function was before it had a solver (parent_logistic_regression), within
    the same bar, and the signature's defaults are what they were."""
    import inspect
    from rlvi_amd import standard
    g = np.load(os.path.join(GOLDEN, "g5_standard.npz"))
    X, y = g["logreg/X"], g["logreg/y"]
    theta, w, outer = standard.logistic_regression(X.copy(), y.copy(), solver="newton", return_info=True)
    th_ref, w_ref, outer_ref, _ = R.logistic_regression(X, y)
    print(f"G5: outer {outer}, |theta - liblinear's| / |.| = "
          f"{np.linalg.norm(theta - g['logreg/theta']) / np.linalg.norm(g['logreg/theta']):.3e}")
    np.testing.assert_allclose(theta, g["logreg/theta"], rtol=1e-3, atol=1e-4)
    assert outer == outer_ref
    np.testing.assert_allclose(theta, th_ref, rtol=1e-8)
    default = standard.logistic_regression(X.copy(), y.copy())
    np.testing.assert_allclose(default, g["logreg/theta"], rtol=1e-3, atol=1e-4)
    assert np.array_equal(default, standard.logistic_regression(X.copy(), y.copy(), solver="liblinear"))
    assert np.array_equal(default, parent_logistic_regression(gpu, X.copy(), y.copy()))
    sig = inspect.signature(standard.logistic_regression)
    assert [(p.name, p.default) for p in sig.parameters.values()][:4] == [
        ("X", inspect.Parameter.empty), ("y", inspect.Parameter.empty), ("maxiter", 100), ("tol", 1e-2)]
    assert sig.parameters["solver"].default == "liblinear" and sig.parameters["solver"].kind == sig.parameters[
        "solver"].KEYWORD_ONLY


def shape_data(n, d):
    rng = np.random.default_rng(100 * n + d)
    X = rng.standard_normal((n, d))
    beta = rng.standard_normal(d) / np.sqrt(d)
    y = (rng.random(n) < 1 / (1 + np.exp(-(0.2 + 2 * X @ beta)))).astype(np.float64)
    if n > 1:
        y[0], y[1] = 0.0, 1.0
    return X, y, 0.05 + 0.95 * rng.random(n)


# one sample; one past a 16-row block; around a wave's 64; 257: two samples per thread; d = 3 | 4, 14 | 15 | 16 and
# 23 | 24: the padded system's sizes and the column-block edge of [X | 1] and the gradient's column; 1024 | 1025: four
# and sixteen samples per thread; the limits
SHAPES = [(1, 1), (17, 2), (63, 3), (64, 4), (65, 5), (257, 14), (200, 15), (200, 16), (300, 24), (1024, 23),
          (1025, 23), (4096, 30)]


@pytest.mark.parametrize("n,d", SHAPES)
def test_shapes_that_take_another_path(n, d, gpu):
    """One weighted fit and a two-iteration estimator against the restatement at every shape at which the launcher
    picks another kernel or a loop gets a tail."""
    torch, ops, dev = gpu
    X, y, w = shape_data(n, d)
    Z = R.design(X)
    theta, losses, info = dev_fit(gpu, X, y, w)
    assert info[3] == 0, info
    th_ref, _, steps_ref = R.fit(X, y, w)
    v = R.to_v(theta)
    g0 = gnorm(X, y, w, np.zeros(d + 1))
    print(f"{n} x {d}: Newton steps {info[2]} (restatement {steps_ref}), |grad| / |grad(0)| = {gnorm(X, y, w, v) / g0:.3e}")
    within_bound(X, y, w, v, R.to_v(th_ref), "device vs logreg_ref")
    np.testing.assert_allclose(losses, np.logaddexp(0, Z @ v), rtol=1e-12)
    if n == 1:
        return                                            # (one class: the estimator's weights are all that differ)
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    th, wts, inf = ops.logistic_regression(Xd, yd, maxiter=2, tol=0.0)
    th_r, w_r, outer_r, _ = R.logistic_regression(X, y, maxiter=2, tol=0.0)
    inf = inf.cpu().numpy()
    assert inf[0] == outer_r == 2 and inf[3] == 0 and 1 <= inf[1] <= 100, inf
    np.testing.assert_allclose(th.cpu().numpy(), th_r, rtol=1e-8)
    np.testing.assert_allclose(wts.cpu().numpy(), w_r, rtol=1e-6, atol=1e-300)


def test_logits_of_700_stay_finite(gpu):
    """A scaled design: a noisy bulk fixes the slope, eight far samples at +-2000 on it reach logits beyond +-700 --
    exp overflows there unless every form is the overflow-safe one.  theta finite, the restatement's, the losses
    z itself where z is large."""
    rng = np.random.default_rng(7)
    n = 128
    X = rng.standard_normal((n, 2))
    y = (rng.random(n) < 1 / (1 + np.exp(-2 * X[:, 0]))).astype(np.float64)
    X[:8, 0] = np.array([2000.0, -2000.0] * 4)
    X[:8, 1] = 0.0
    y[:8] = np.array([1.0, 0.0] * 4)
    w = np.ones(n)
    theta, losses, info = dev_fit(gpu, X, y, w)
    z = R.design(X) @ R.to_v(theta)
    print(f"logits in [{z.min():.1f}, {z.max():.1f}], Newton steps {info[2]}, theta {theta}")
    assert info[3] == 0 and np.isfinite(theta).all() and np.isfinite(losses).all()
    assert z.max() >= 700 and z.min() <= -700
    within_bound(X, y, w, R.to_v(theta), R.to_v(R.fit(X, y, w)[0]), "device vs logreg_ref")
    np.testing.assert_allclose(losses, np.logaddexp(0, z), rtol=1e-12)
    from rlvi_amd import standard
    th = standard.logistic_regression(X, y, solver="newton")
    assert np.isfinite(th).all()
    np.testing.assert_allclose(th, R.logistic_regression(X, y)[0], rtol=1e-8)


def test_separable_data_converges(gpu):
    """Perfectly separable data: the regulariser keeps the minimiser finite and Newton reaches it well inside its
    50 steps -- no RLVI_ST_NOCONV, flag 0."""
    torch, ops, dev = gpu
    rng = np.random.default_rng(11)
    X = rng.standard_normal((96, 3))
    X[:, 0] += np.where(X[:, 0] > 0, 0.5, -0.5)
    y = (X[:, 0] > 0).astype(np.float64)
    w = np.ones(96)
    theta, losses, info = dev_fit(gpu, X, y, w)
    print(f"separable: Newton steps {info[2]}, theta {theta}")
    assert info[3] == 0 and info[2] < 50
    assert ops.workspace(dev).status() == 0
    within_bound(X, y, w, R.to_v(theta), R.to_v(R.fit(X, y, w)[0]), "device vs logreg_ref")
    from rlvi_amd import standard
    th, wts, outer = standard.logistic_regression(X, y, solver="newton", return_info=True)
    th_r, w_r, outer_r, _ = R.logistic_regression(X, y)
    assert outer == outer_r
    np.testing.assert_allclose(th, th_r, rtol=1e-8)


def test_maxiter_zero_is_the_unit_weight_fit(gpu):
    torch, ops, dev = gpu
    from rlvi_amd import standard
    X, y, _ = shape_data(200, 2)
    theta, w, outer = standard.logistic_regression(X, y, maxiter=0, solver="newton", return_info=True)
    fit_theta, _, _ = dev_fit(gpu, X, y, np.ones(200))
    assert outer == 0 and np.array_equal(w, np.ones(200))
    assert np.array_equal(theta, fit_theta)               # the same device code from the same start: the same bits


def test_errors_are_raised_before_anything_runs(gpu):
    torch, ops, dev = gpu
    from rlvi_amd import _lib, standard
    X, y, _ = shape_data(200, 2)
    ws = ops.workspace(dev)
    for bad in (np.nan, np.inf):
        Xb = X.copy()
        Xb[3, 1] = bad
        with pytest.raises(ValueError):
            standard.logistic_regression(Xb, y, solver="newton")
        assert ws.status() == 0
    with pytest.raises(ValueError):
        standard.logistic_regression(X, np.ones(200), solver="newton")            # a single class
    with pytest.raises(ValueError):
        standard.logistic_regression(X, np.where(y > 0, 2.0, 0.0), solver="newton")   # labels outside {0, 1}
    with pytest.raises(ValueError):
        standard.logistic_regression(X, y, solver="lbfgs")
    X2, y2, _ = shape_data(4097, 2)
    with pytest.raises(_lib.RlviError, match="4096"):
        standard.logistic_regression(X2, y2, solver="newton")
    with pytest.raises(_lib.RlviError, match="30"):
        standard.logistic_regression(np.zeros((200, 31)), y, solver="newton")
    assert ws.status() == 0
    # the C entry itself, handed what the Python layer refuses: flag 1, nothing written
    Xb = X.copy()
    Xb[3, 1] = np.nan
    theta = torch.full((3,), 7.0, dtype=torch.float64, device=dev)
    _, _, info = ops.logistic_regression(torch.from_numpy(Xb).to(dev), torch.from_numpy(y).to(dev), theta=theta)
    assert info.cpu().numpy()[3] == 1 and bool((theta == 7.0).all())
    assert ws.status() == 0


def test_same_bits_twice_and_under_graph_capture(gpu):
    torch, ops, dev = gpu
    X, y, _ = shape_data(1000, 20)
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    a = [t.cpu().numpy() for t in ops.logistic_regression(Xd, yd)]
    b = [t.cpu().numpy() for t in ops.logistic_regression(Xd, yd)]
    assert all(np.array_equal(p, q) for p, q in zip(a, b)) and a[2][3] == 0 and a[2][0] >= 1
    theta = torch.zeros(21, dtype=torch.float64, device=dev)
    w = torch.zeros(1000, dtype=torch.float64, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ws = ops.Workspace(dev, 1000, 0)
        ops.logistic_regression(Xd, yd, theta=theta, weights=w, info=info, ws=ws)      # (warm-up outside the capture)
        torch.cuda.synchronize()
        theta.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ops.logistic_regression(Xd, yd, theta=theta, weights=w, info=info, ws=ws)
        g.replay()
        torch.cuda.synchronize()
    assert np.array_equal(theta.cpu().numpy(), a[0]) and np.array_equal(w.cpu().numpy(), a[1])
    assert np.array_equal(info.cpu().numpy(), a[2]) and ws.status() == 0
