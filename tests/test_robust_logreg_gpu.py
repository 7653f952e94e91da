"""RRM's logistic regression in one launch (rlvi_amd/csrc/robust_logreg.hip) on the GPU: every run of the reference in
tests/golden/g20_rrm_logreg.npz through numpy and through ops, one shape per dispatch arm, maxiter = 0, the no-root
limit, a weight that underflows to exactly 0, logits beyond +-700, the batch forms, a bad label inside a batch,
determinism and graph capture.

The bars: against the numpy restatement tests/robust_logreg_ref.py (logreg_ref.fit and rrm_ref.update_weights composed
as the kernel composes them; only the order of the sums and the solve differ) the outer count equal, theta at rtol 1e-8
and the weights at rtol 1e-6 / atol 1e-300 -- what tests/test_logreg_gpu.py and tests/test_rrm_gpu.py hold for this fit
and this rule; against the reference's own theta the relative distance theta_bar (1 + 1e-3), theta_bar what the
fixture's tool measured between the restatement and the reference (liblinear's tolerance): the device may add at most
its 1e-8 to it.  Designs beyond the fixture are seeded gauss_case designs at the first seed on which every stop decision
of the restatement is clear of the edge (margin >= 1e-4, the fixture's rule).  Each test prints its figures before it
asserts."""
import os

import numpy as np
import pytest

import logreg_ref
import robust_logreg_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G20 = np.load(os.path.join(ROOT, "tests", "golden", "g20_rrm_logreg.npz"))
RUNS = [str(k) for k in G20["runs"]]
THETA_BAR = float(G20["theta_bar"])
ROOT_CAP = 200                                                       # MO_ROOT_CAP
EPS = 0.4                                                            # main.py:382


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


def run_eps(run):
    return float(run.rsplit("/eps", 1)[1])


def run_data(run):
    key = run.rsplit("/", 1)[0]
    # (the generator's X is a column stack: row-major here, as the device tensors must be)
    return np.ascontiguousarray(G20[key + "/X"], dtype=np.float64), G20[key + "/y"].astype(np.float64)


_ref_runs = {}


def ref_run(run):
    """The restatement on a G20 run, computed once."""
    if run not in _ref_runs:
        _ref_runs[run] = R.rrm_logistic_regression(*run_data(run), run_eps(run))
    return _ref_runs[run]


def through_ops(gpu, X, y, eps, **kw):
    torch, ops, dev = gpu
    return tuple(t.cpu().numpy() for t in ops.rrm_logistic_regression(torch.from_numpy(X).to(dev),
                                                                      torch.from_numpy(y).to(dev), eps, **kw))


def against_restatement(what, got, ref):
    theta, w, info = got
    th_ref, w_ref, count_ref, trace = ref
    print(f"    {what}: info {info.tolist()} (restatement's count {count_ref}, least stop margin {R.margin(trace):.1e}), "
          f"|theta - restatement's| / |.| = {np.linalg.norm(theta - th_ref) / np.linalg.norm(th_ref):.3e}, "
          f"max |w - its| = {np.max(np.abs(w - w_ref)):.3e}, |sum w - 1| = {abs(w.sum() - 1.0):.1e}")
    assert info[0] == count_ref and info[3] == 0
    assert 0 <= info[1] <= ROOT_CAP and info[2] >= count_ref + 1     # (every fit takes a Newton step at least)
    np.testing.assert_allclose(theta, th_ref, rtol=1e-8)
    np.testing.assert_allclose(w, w_ref, rtol=1e-6, atol=1e-300)
    assert abs(w.sum() - 1.0) <= 1e-12


@pytest.mark.parametrize("run", RUNS)
def test_every_g20_run_in_one_launch(run, gpu):
    from rlvi_amd import rrm
    X, y = run_data(run)
    eps, ref = run_eps(run), G20[run + "/theta"]
    got = rrm.logistic_regression(X, y, eps, return_info=True)
    dist = np.linalg.norm(got[0] - ref) / np.linalg.norm(ref)
    print(f"{run}: fixture count {int(G20[run + '/count'])}, |theta - reference's| / |.| = {dist:.3e} "
          f"(theta_bar {THETA_BAR:.3e})")
    assert got[2][0] == int(G20[run + "/count"])
    against_restatement("numpy", got, ref_run(run))
    assert dist <= THETA_BAR * (1 + 1e-3)
    assert np.array_equal(rrm.logistic_regression(X, y, eps), got[0])
    dev_got = through_ops(gpu, X, y, eps)
    against_restatement("ops", dev_got, ref_run(run))
    assert all(np.array_equal(a, b) for a, b in zip(got, dev_got))   # the same launch: the same bits


# One shape per (samples per thread, padded system): n <= 256 | <= 1024 | <= 4096 by d <= 3 | 14 | 23 | 30, each arm at its
# edges -- 17: one past a 16-row block; 256 | 257 and 1024 | 1025: the thresholds of E; d = 3 | 4, 14 | 15, 23 | 24: the
# thresholds of the system's size and of the second column block; 4096 x 30: the limits
SHAPES = [(17, 1), (256, 3), (256, 4), (17, 14), (256, 15), (17, 23), (256, 24), (17, 30),
          (257, 3), (1024, 4), (257, 14), (1024, 15), (257, 23), (1024, 24), (257, 30),
          (1025, 1), (1025, 3), (1025, 4), (1025, 14), (1025, 15), (1025, 23), (1025, 24), (1025, 30), (4096, 30)]
MAX_SEEDS = 5


@pytest.fixture(scope="module")
def shape_cases():
    """{(n, d): (X, y, the restatement's result)}, each at the first seed with both classes whose stop decisions are
    clear of the edge, and how many seeds that took: computed once, on the host."""
    cases, seeds = {}, {"tried": 0, "skipped": 0}
    for n, d in SHAPES:
        for t in range(MAX_SEEDS):
            X, y = R.gauss_case(1000 * n + d + 7919 * t, n, d)
            seeds["tried"] += 1
            if y.min() != y.max():
                ref = R.rrm_logistic_regression(X, y, EPS)
                if R.margin(ref[3]) >= 1e-4:
                    cases[(n, d)] = (X, y, ref)
                    break
            seeds["skipped"] += 1
        else:
            raise AssertionError(f"no seed of {n} x {d} is clear of the edge")
    return cases, seeds


@pytest.mark.parametrize("n,d", SHAPES)
def test_every_dispatch_arm(n, d, shape_cases, gpu):
    X, y, ref = shape_cases[0][(n, d)]
    against_restatement(f"{n} x {d}", through_ops(gpu, X, y, EPS), ref)


def test_no_more_than_one_seed_in_ten_was_skipped(shape_cases):
    seeds = shape_cases[1]
    print(f"seeds tried {seeds['tried']}, skipped {seeds['skipped']}")
    assert seeds["tried"] >= len(SHAPES) and seeds["skipped"] <= 0.1 * seeds["tried"]


@pytest.mark.parametrize("n,d", [(200, 2), (1025, 23)])
def test_maxiter_zero_is_the_unit_weight_fit(n, d, gpu):
    torch, ops, dev = gpu
    from rlvi_amd import rrm
    X, y = R.gauss_case(3, n, d)
    theta, w, info = rrm.logistic_regression(X, y, EPS, maxiter=0, return_info=True)
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    fit_theta, _, fit_info = (t.cpu().numpy() for t in ops.logistic_fit(Xd, yd, torch.ones(n, dtype=torch.float64,
                                                                                          device=dev)))
    print(f"{n} x {d}: info {info.tolist()}, the fit's {fit_info.tolist()}")
    assert info.tolist() == [0, 0, int(fit_info[2]), 0] and fit_info[3] == 0
    assert np.array_equal(theta, fit_theta)               # the same device code from the same start: the same bits
    assert np.array_equal(w, np.ones(n) / n)


def test_all_zero_design_hits_the_no_root_limit(gpu):
    """X = 0: every z is the bias, every loss the same.  The rule has no root (all n tied at the minimum): weights
    1 / n and no evaluation; the refit returns the same theta, the discrepancy is 0 and the loop stops after one
    iteration."""
    n = 64
    X = np.zeros((n, 2))
    y = (np.arange(n) < 40).astype(np.float64)
    theta, w, info = through_ops(gpu, X, y, EPS)
    th_ref, w_ref, outer_ref, trace = R.rrm_logistic_regression(X, y, EPS)
    print(f"all-zero design: info {info.tolist()}, theta {theta}, restatement's {th_ref}, trace {trace}")
    assert info[:2].tolist() == [1, 0] and info[3] == 0 and outer_ref == 1
    assert np.array_equal(w, np.ones(n) / n) and np.array_equal(w_ref, w)
    assert theta[0] > 0.0 and np.array_equal(theta[1:], [0.0, 0.0])
    np.testing.assert_allclose(theta, th_ref, rtol=1e-8)


def test_a_weight_that_underflows_to_exactly_zero(gpu):
    """One sample 300 lengths out along the fitted direction, on its own side: its logit is 800, its loss 800 and its
    weight exp(-800 / alpha) = 0 exactly.  The objective's 1/2 v.v keeps the Hessian >= I: the fit goes on without it."""
    X, y = R.gauss_case(5, 100, 2)
    v = logreg_ref.to_v(R.rrm_logistic_regression(X, y, EPS)[0])
    X[0] = 300.0 * v[:2] / np.linalg.norm(v[:2])
    y[0] = 1.0
    ref = R.rrm_logistic_regression(X, y, EPS)
    assert R.margin(ref[3]) >= 1e-4 and ref[1][0] == 0.0 and np.count_nonzero(ref[1] == 0.0) == 1
    got = through_ops(gpu, X, y, EPS)
    against_restatement("far-out sample", got, ref)
    assert got[1][0] == 0.0 and np.count_nonzero(got[1] == 0.0) == 1 and np.isfinite(got[0]).all()


def test_logits_beyond_700_stay_finite(gpu):
    """The scaled design of tests/test_logreg_gpu.py: a noisy bulk fixes the slope, eight far samples at +-2000 on it
    reach logits beyond +-700 -- exp overflows there unless every form is the overflow-safe one -- and losses of
    thousands go into the rule, whose t = l / alpha is cut at 800."""
    rng = np.random.default_rng(7)
    n = 128
    X = rng.standard_normal((n, 2))
    y = (rng.random(n) < 1 / (1 + np.exp(-2 * X[:, 0]))).astype(np.float64)
    X[:8, 0] = np.array([2000.0, -2000.0] * 4)
    X[:8, 1] = 0.0
    y[:8] = np.array([1.0, 0.0] * 4)
    ref = R.rrm_logistic_regression(X, y, EPS)
    assert R.margin(ref[3]) >= 1e-4
    got = through_ops(gpu, X, y, EPS)
    z = logreg_ref.design(X) @ logreg_ref.to_v(got[0])
    print(f"logits in [{z.min():.1f}, {z.max():.1f}], theta {got[0]}, weights in [{got[1].min():.3e}, {got[1].max():.3e}]")
    assert z.max() >= 700 and z.min() <= -700
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    against_restatement("logits of 700", got, ref)


def batch_of(n, d, B):
    data = [R.gauss_case(100 * n + d + 31 * b, n, d) for b in range(B)]
    assert all(y.min() != y.max() for _, y in data)
    return np.stack([x for x, _ in data]), np.stack([v for _, v in data])


@pytest.mark.parametrize("B", [1, 3, 300])
@pytest.mark.parametrize("n,d", [(100, 2), (257, 15)])
def test_batch_has_the_bits_of_single_calls(n, d, B, gpu):
    torch, ops, dev = gpu
    from rlvi_amd import rrm
    Xh, yh = batch_of(n, d, B)
    X, y = torch.from_numpy(Xh).to(dev), torch.from_numpy(yh).to(dev)
    th, w, info = (v.cpu().numpy() for v in ops.rrm_logistic_regression_batch(X, y, EPS))
    assert th.shape == (B, d + 1) and w.shape == (B, n) and info.shape == (B, 4)
    assert (info[:, 3] == 0).all() and (info[:, 0] >= 1).all()
    print(f"{B} x {n} x {d}: outer iterations {info[:, 0].min()} .. {info[:, 0].max()}")
    for b in range(B):
        th1, w1, info1 = (v.cpu().numpy() for v in ops.rrm_logistic_regression(X[b], y[b], EPS))
        assert np.array_equal(th[b], th1) and np.array_equal(w[b], w1) and np.array_equal(info[b], info1), b
    # numpy in, numpy out: the same bits again, theta alone by default
    b = B - 1
    thn, wn, infon = rrm.logistic_regression_batch(Xh, yh, EPS, return_info=True)
    assert np.array_equal(thn, th) and np.array_equal(wn, w) and np.array_equal(infon, info)
    th1, w1, info1 = rrm.logistic_regression(Xh[b], yh[b], EPS, return_info=True)
    assert np.array_equal(thn[b], th1) and np.array_equal(wn[b], w1) and np.array_equal(infon[b], info1)
    assert np.array_equal(rrm.logistic_regression_batch(Xh, yh, EPS), th)


def test_a_bad_label_in_the_middle_is_flagged_alone(gpu):
    torch, ops, dev = gpu
    from rlvi_amd import rrm
    Xh, yh = batch_of(100, 2, 5)
    th0, w0, info0 = rrm.logistic_regression_batch(Xh, yh, EPS, return_info=True)
    assert (info0[:, 3] == 0).all()
    bad = yh.copy()
    bad[2, 7] = 2.0
    keep = [0, 1, 3, 4]
    th, w, info = rrm.logistic_regression_batch(Xh, bad, EPS, return_info=True)
    assert info[:, 3].tolist() == [0, 0, 1, 0, 0] and np.isnan(th[2]).all() and np.isnan(w[2]).all()
    assert np.array_equal(th[keep], th0[keep]) and np.array_equal(w[keep], w0[keep])
    assert np.array_equal(info[keep], info0[keep])
    with pytest.raises(ValueError, match=r"labels 0 and 1.*problem 2"):
        rrm.logistic_regression_batch(Xh, bad, EPS)
    with pytest.raises(ValueError, match="labels 0 and 1"):
        rrm.logistic_regression(Xh[2], bad[2], EPS)
    # the C entry: flag 1, nothing written
    theta = torch.full((5, 3), 7.0, dtype=torch.float64, device=dev)
    weights = torch.full((5, 100), 7.0, dtype=torch.float64, device=dev)
    _, _, inf = ops.rrm_logistic_regression_batch(torch.from_numpy(Xh).to(dev), torch.from_numpy(bad).to(dev), EPS,
                                                  out=(theta, weights))
    assert inf.cpu().numpy()[:, 3].tolist() == [0, 0, 1, 0, 0]
    assert bool((theta[2] == 7.0).all()) and bool((weights[2] == 7.0).all())
    assert np.array_equal(theta.cpu().numpy()[keep], th0[keep])


def test_same_bits_twice_and_under_graph_capture(gpu):
    """Two eager runs and a captured, replayed one (a single branch): the same bits."""
    torch, ops, dev = gpu
    X, y = (torch.from_numpy(a).to(dev) for a in run_data("gauss_1000x20_c0.0/eps0.4"))
    n, d = X.shape
    a = [t.cpu().numpy() for t in ops.rrm_logistic_regression(X, y, EPS)]
    b = [t.cpu().numpy() for t in ops.rrm_logistic_regression(X, y, EPS)]
    assert all(np.array_equal(p, q) for p, q in zip(a, b)) and a[2][3] == 0 and a[2][0] >= 1
    theta = torch.zeros(d + 1, dtype=torch.float64, device=dev)
    w = torch.zeros(n, dtype=torch.float64, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ws = ops.Workspace(dev, n, 0)
        ops.rrm_logistic_regression(X, y, EPS, out=(theta, w), info=info, ws=ws)          # (warm-up outside the capture)
        torch.cuda.synchronize()
        theta.zero_()
        w.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ops.rrm_logistic_regression(X, y, EPS, out=(theta, w), info=info, ws=ws)
        g.replay()
        torch.cuda.synchronize()
    assert np.array_equal(theta.cpu().numpy(), a[0]) and np.array_equal(w.cpu().numpy(), a[1])
    assert np.array_equal(info.cpu().numpy(), a[2]) and ws.status() == 0
