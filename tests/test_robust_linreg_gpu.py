"""RRM and Huber linear regression in one launch (rlvi_amd/csrc/robust_linreg.hip) on the GPU: every case of the reference
in tests/golden/g19_robust_linreg.npz, the smallest shapes that reach every dispatch path, maxiter = 0, columns scaled
by 2^+-200, a duplicated column, an exactly interpolating y, the no-root limit, Huber's cap, the size limit, the batch
forms, determinism and graph capture.

The bars: against the numpy restatement tests/robust_linreg_ref.py (the same algorithms; only the order of the sums and
the factorisation differ) theta and sigma at rtol 1e-8 and RRM's weights at rtol 1e-6 / atol 1e-300 -- what the other
one-workgroup estimators hold against theirs -- and the iteration counts equal; against the reference's own theta rtol
1e-8 + 10 x theta_bar, theta_bar the largest relative distance the fixture's generator measured between the restatement
and the reference (RRM: Brent's tolerance; Huber: rounding).  Shapes beyond the fixture take the first seed on which the
restatement's stop decisions are clear of the edge (RRM |discrepancy - tol| >= 1e-6, Huber |discrepancy / 1e-6 - 1| >=
1e-3: the fixture's rules); no more than one seed in ten may be skipped.  Each test prints its figures before it
asserts."""
import os

import numpy as np
import pytest

import linreg_designs as L
import robust_linreg_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G19 = np.load(os.path.join(ROOT, "tests", "golden", "g19_robust_linreg.npz"))
CASES = [str(k) for k in G19["cases"]]
RUNS = [str(k) for k in G19["runs"]]
BAR = {"rrm": float(G19["theta_bar_rrm"]), "huber": float(G19["theta_bar_huber"])}
ROOT_CAP = 200                                                       # MO_ROOT_CAP


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


def run_param(run):
    return float(run[len("rrm_eps"):]) if run.startswith("rrm") else float(run[len("huber_sigma"):])


def device_run(run, X, y, **kw):
    """(theta, weights | sigma, info) of the numpy-in / numpy-out call"""
    from rlvi_amd import huber, rrm
    if run.startswith("rrm"):
        return rrm.linear_regression(X, y, run_param(run), return_info=True, **kw)
    return huber.linear_regression(X, y, sigma0=run_param(run), return_info=True, **kw)


def restatement(run, X, y):
    if run.startswith("rrm"):
        return R.rrm_linear_regression(X, y, run_param(run))
    return R.huber_linear_regression(X, y, sigma0=run_param(run))


def margin_ok(run, trace):
    return R.rrm_margin(trace) >= 1e-6 if run.startswith("rrm") else R.huber_margin(trace) >= 1e-3


def against_restatement(what, run, got, ref):
    theta, second, info = got
    th_ref, second_ref, count_ref, _ = ref
    print(f"    {what} {run}: info {info.tolist()} (restatement's count {count_ref}), |theta - restatement's| / |.| = "
          f"{np.linalg.norm(theta - th_ref) / np.linalg.norm(th_ref):.3e}, "
          f"{'max |w - its|' if run.startswith('rrm') else '|sigma / its - 1|'} = "
          f"{np.max(np.abs(second - second_ref)) if run.startswith('rrm') else abs(second / second_ref - 1):.3e}")
    assert info[0] == count_ref and info[3] == 0
    np.testing.assert_allclose(theta, th_ref, rtol=1e-8)
    if run.startswith("rrm"):
        assert 0 <= info[1] <= ROOT_CAP and info[2] >= info[1]
        np.testing.assert_allclose(second, second_ref, rtol=1e-6, atol=1e-300)
        assert abs(second.sum() - 1.0) <= 1e-12
    else:
        np.testing.assert_allclose(second, second_ref, rtol=1e-8)


_ref_runs = {}


def ref_run(key, run):
    """The restatement on a G19 case, computed once."""
    if (key, run) not in _ref_runs:
        _ref_runs[(key, run)] = restatement(run, G19[key + "/X"].astype(np.float64), G19[key + "/y"].astype(np.float64))
    return _ref_runs[(key, run)]


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("key", CASES)
def test_every_g19_case_in_one_launch(key, run, gpu):
    X, y = G19[key + "/X"].astype(np.float64), G19[key + "/y"].astype(np.float64)
    est = run.split("_")[0]
    got = device_run(run, X, y)
    ref = G19[f"{key}/{run}/theta"]
    print(f"{key} {run}: fixture count {int(G19[f'{key}/{run}/count'])}, |theta - reference's| / |.| = "
          f"{np.linalg.norm(got[0] - ref) / np.linalg.norm(ref):.3e} (theta_bar {BAR[est]:.3e})")
    assert got[2][0] == int(G19[f"{key}/{run}/count"])
    against_restatement(key, run, got, ref_run(key, run))
    np.testing.assert_allclose(got[0], ref, rtol=1e-8 + 10 * BAR[est])
    again = device_run(run, X, y)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]) and np.array_equal(got[2], again[2])


# The dispatch table of the launcher, each entry at the smallest shapes that reach it: 2 x 1, 3 x 2 the smallest systems;
# 17 x 3 one past a 16-row block; 40 x 12 | 65 x 13 the 12- and the 16-row system; 100 x 15 | 100 x 16: y the last column
# of block 0 | the first of block 1 (20-row system, x1s in LDS); 1023 x 20, 1024 x 23: the resident design's last shapes
# (24-row system); 1024 x 24, 64 x 31: streamed with four samples per thread (32-row system); 1025 x 12, 1027 x 15,
# 1025 x 20, 1025 x 24, 4096 x 31: sixteen samples per thread at every padded system size, and the limits
SHAPES = [(2, 1), (3, 2), (17, 3), (40, 12), (65, 13), (100, 15), (100, 16), (1023, 20), (1024, 23), (1024, 24), (64, 31),
          (1025, 12), (1027, 15), (1025, 20), (1025, 24), (4096, 31)]
SHAPE_RUNS = ("rrm_eps0.2", "huber_sigma1.0")
MAX_SEEDS = 5


@pytest.fixture(scope="module")
def shape_cases():
    """{(n, d, run): (X, y, the restatement's result)} on the generator's recipe, each at the first seed whose stop
    decisions are clear of the edge, and the seeds' statistics {"tried", "skipped"}: computed once, on the host."""
    from rlvi_amd import synth
    cases, seeds = {}, {"tried": 0, "skipped": 0}
    for n, d in SHAPES:
        for run in SHAPE_RUNS:
            for t in range(MAX_SEEDS):
                X, y = synth.linreg_data(n, d, eps=0.2, nu=2.5, seed=1000 * n + d + 7919 * t)
                ref = restatement(run, X, y)
                seeds["tried"] += 1
                if margin_ok(run, ref[3]):
                    cases[(n, d, run)] = (X, y, ref)
                    break
                seeds["skipped"] += 1
            else:
                raise AssertionError(f"no seed of {n} x {d} {run} is clear of the edge")
    return cases, seeds


@pytest.mark.parametrize("n,d", SHAPES)
def test_shapes_that_take_another_path(n, d, shape_cases, gpu):
    for run in SHAPE_RUNS:
        X, y, ref = shape_cases[0][(n, d, run)]
        against_restatement(f"{n} x {d}", run, device_run(run, X, y), ref)


def test_no_more_than_one_seed_in_ten_was_skipped(shape_cases):
    seeds = shape_cases[1]
    print(f"seeds tried {seeds['tried']}, skipped {seeds['skipped']}")
    assert seeds["tried"] >= len(SHAPES) * len(SHAPE_RUNS) and seeds["skipped"] <= 0.1 * seeds["tried"]


def test_maxiter_zero_is_the_first_fit(gpu):
    from rlvi_amd import synth
    X, y = synth.linreg_data(200, 7, eps=0.2, nu=2.5, seed=3)
    ols = np.linalg.lstsq(X, y, rcond=None)[0]
    theta, w, info = device_run("rrm_eps0.2", X, y, maxiter=0)
    assert info.tolist() == [0, 0, 0, 0] and np.array_equal(w, np.ones(200) / 200)
    np.testing.assert_allclose(theta, ols, rtol=1e-11)
    theta, sigma, info = device_run("huber_sigma0.1", X, y, maxiter=0)
    assert info.tolist() == [0, 0, 0, 0] and sigma == 0.1
    np.testing.assert_allclose(theta, ols, rtol=1e-11)


@pytest.mark.parametrize("n,d", [(40, 10), (100, 20), (1025, 12)])
def test_columns_scaled_by_powers_of_two(n, d, gpu):
    """Column j times 2^k_j, |k| up to 200 (linreg_designs.patterns).  Neither estimator reads it as rank deficiency: that
    is checked on the full, converged runs of both.  Huber's theta 2^k keeps every bit -- THIS DEVIATES from the issue's
    wording, which asks for it of the run as a whole: the bits are compared after five iterations through ops (which
    reports the cap as flag 3), not after convergence.  The stop test ||theta - theta0|| / ||theta0|| is not invariant
    under a scaling of single columns, in the reference either, so a scaled design may stop at another iteration and
    the converged thetas then differ by a step of 1e-6; bit-equality can be asked only where no stop decision is taken,
    as tests/test_linreg_designs_gpu.py does for the RLVI estimator."""
    torch, ops, dev = gpu
    from rlvi_amd import huber, rrm
    X, y = L.base(n, d)
    yd = torch.from_numpy(y).to(dev)
    ws = ops.workspace(dev)

    def five(Xh):
        th, s, info = (t.cpu().numpy() for t in ops.huber_linear_regression(torch.from_numpy(Xh).to(dev), yd, maxiter=5))
        ws.clear_status()
        return th, s, info
    th0, s0, info0 = five(X)
    assert info0.tolist() == [5, 0, 0, 3]
    flagged, moved = [], []
    for name, kv in L.patterns(d, ks=(-200, 200)):
        Xs = L.scaled(X, kv)
        th, s, info = five(Xs)
        if not (np.array_equal(L.unscale(th, kv), th0) and np.array_equal(s, s0) and np.array_equal(info, info0)):
            moved.append((name, info.tolist(), float(np.max(np.abs(L.unscale(th, kv) / th0 - 1)))))
        th_h, sig, info_h = huber.linear_regression(Xs, y, return_info=True)
        th_r, w_r, info_r = rrm.linear_regression(Xs, y, 0.2, return_info=True)
        if info_h[3] != 0 or info_r[3] != 0 or not (np.isfinite(th_h).all() and np.isfinite(th_r).all()):
            flagged.append((name, info_h.tolist(), info_r.tolist()))
    print(f"{n} x {d}: flagged {flagged}; Huber bits moved {moved}")
    assert not flagged and not moved


def test_a_duplicated_column(gpu):
    """X^T X is singular: Huber raises what numpy.linalg.solve raises at huber.py:17; RRM takes the general path -- the
    minimum-norm solution, as the reference's lstsq -- and returns a finite theta that fits as the full-rank design does."""
    from rlvi_amd import huber, rrm
    X, y = L.base(40, 10)
    Z = L.rank_deficient(X)["duplicate"]
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):
        huber.linear_regression(Z, y)
    theta, w, info = rrm.linear_regression(Z, y, 0.2, return_info=True)
    print(f"duplicate column: info {info.tolist()}, theta {theta}")
    assert info[3] == 1 and info[0] >= 1 and np.isfinite(theta).all() and np.isfinite(w).all()
    assert abs(theta[0] - theta[-1]) <= 1e-8 * abs(theta[0])         # minimum norm: the twin columns share their weight
    th_ref = R.rrm_linear_regression(np.column_stack([Z[:, 0] * 2, Z[:, 1:-1]]), y, 0.2)[0]
    np.testing.assert_allclose(np.concatenate([[theta[0]], theta[1:-1]]), th_ref, rtol=1e-6)


def test_an_exactly_interpolating_y(gpu):
    """Residuals that are exactly 0 (orthogonal columns of power-of-two length, integer theta): sigma = 0, the
    reference's lstsq meets a NaN and raises; flag 2 and the same ValueError here."""
    torch, ops, dev = gpu
    from rlvi_amd import huber
    X = np.tile(np.eye(2), (4, 1))
    y = X @ np.array([3.0, -5.0])
    with pytest.raises(ValueError, match="array must not contain infs or NaNs"):
        huber.linear_regression(X, y)
    th = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    _, _, info = ops.huber_linear_regression(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev), out=(th, None))
    assert info.cpu().numpy().tolist() == [1, 0, 0, 2] and bool((th == 7.0).all())
    with pytest.raises(FloatingPointError):
        R.huber_linear_regression(X, y)


def test_all_equal_losses_hit_the_no_root_limit(gpu):
    """x = 1 and y = +-1 in equal numbers: theta = 0 exactly and every loss is 1.  The rule has no root (all n tied at the
    minimum): weights 1 / n, no evaluation, and the refit returns the same theta -- the discrepancy 0 / 0 is a NaN and
    the loop runs to maxiter, as the reference's does."""
    n = 64
    X = np.ones((n, 1))
    y = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    theta, w, info = device_run("rrm_eps0.2", X, y, maxiter=3)
    th_ref, w_ref, outer_ref, trace = R.rrm_linear_regression(X, y, 0.2, maxiter=3)
    print(f"all-equal losses: info {info.tolist()}, theta {theta}, restatement's outer {outer_ref}, trace {trace}")
    assert info.tolist() == [outer_ref, 0, 0, 0] and outer_ref == 3
    assert np.array_equal(theta, [0.0]) and np.array_equal(th_ref, [0.0])
    assert np.array_equal(w, np.ones(n) / n) and np.array_equal(w_ref, w)


def test_hubers_cap_and_the_size_limit(gpu):
    torch, ops, dev = gpu
    from rlvi_amd import _lib, huber, rrm, synth
    X, y = synth.linreg_data(40, 10, eps=0.2, nu=2.5, seed=1)
    with pytest.raises(_lib.RlviError, match="maxiter = 3"):
        huber.linear_regression(X, y, maxiter=3)
    assert ops.workspace(dev).status() == 0
    theta, sigma, info = (t.cpu().numpy() for t in ops.huber_linear_regression(
        torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev), maxiter=3))
    assert info.tolist() == [3, 0, 0, 3] and ops.workspace(dev).status() == _lib.ST_NOCONV
    ops.workspace(dev).clear_status()
    ref = R.huber_linear_regression(X, y, maxiter=3)
    np.testing.assert_allclose(theta, ref[0], rtol=1e-8)
    np.testing.assert_allclose(sigma[0], ref[1], rtol=1e-8)
    for shape in ((4097, 3), (50, 32)):
        with pytest.raises(_lib.RlviError, match="4096.*31"):
            rrm.linear_regression(np.zeros(shape), np.zeros(shape[0]), 0.2)
        with pytest.raises(_lib.RlviError, match="4096.*31"):
            huber.linear_regression(np.zeros(shape), np.zeros(shape[0]))
    bad = y.copy()
    bad[5] = np.nan
    for call in (lambda: rrm.linear_regression(X, bad, 0.2), lambda: huber.linear_regression(X, bad)):
        with pytest.raises(ValueError, match="array must not contain infs or NaNs"):
            call()
    for eps in (0.0, 1.0, 0.98):
        with pytest.raises(ValueError):
            rrm.linear_regression(X, y, eps)
    for c, s0 in ((0.0, 1.0), (0.7, 0.0), (0.7, -1.0)):
        with pytest.raises(ValueError):
            huber.linear_regression(X, y, c, s0)


def batch_of(n, d, B):
    from rlvi_amd import synth
    data = [synth.linreg_data(n, d, eps=0.2, nu=2.5, seed=100 * n + d + b) for b in range(B)]
    return np.stack([x for x, _ in data]), np.stack([v for _, v in data])


@pytest.mark.parametrize("B", [1, 3, 300])
@pytest.mark.parametrize("n,d", [(40, 10), (1025, 12)])
def test_batch_has_the_bits_of_single_calls(n, d, B, gpu):
    torch, ops, dev = gpu
    Xh, yh = batch_of(n, d, B)
    X, y = torch.from_numpy(Xh).to(dev), torch.from_numpy(yh).to(dev)
    forms = (("rrm", ops.rrm_linear_regression_batch, ops.rrm_linear_regression, (0.2,)),
             ("huber", ops.huber_linear_regression_batch, ops.huber_linear_regression, ()))
    for what, batch_fn, single_fn, args in forms:
        th, second, info = (v.cpu().numpy() for v in batch_fn(X, y, *args))
        assert info.shape == (B, 4) and (info[:, 3] == 0).all() and (info[:, 0] >= 1).all()
        print(f"{what} {B} x {n} x {d}: iterations {info[:, 0].min()} .. {info[:, 0].max()}")
        for b in range(B):
            th1, s1, info1 = (v.cpu().numpy() for v in single_fn(X[b], y[b], *args))
            assert np.array_equal(th[b], th1) and np.array_equal(second[b].ravel(), s1.ravel()), (what, b)
            assert np.array_equal(info[b], info1), (what, b)
    # numpy in, numpy out: the same bits again, theta alone by default
    from rlvi_amd import huber, rrm
    b = B - 1
    th, w, info = rrm.linear_regression_batch(Xh, yh, 0.2, return_info=True)
    th1, w1, info1 = rrm.linear_regression(Xh[b], yh[b], 0.2, return_info=True)
    assert np.array_equal(th[b], th1) and np.array_equal(w[b], w1) and np.array_equal(info[b], info1)
    assert np.array_equal(rrm.linear_regression_batch(Xh, yh, 0.2), th)
    th, sig, info = huber.linear_regression_batch(Xh, yh, return_info=True)
    th1, sig1, info1 = huber.linear_regression(Xh[b], yh[b], return_info=True)
    assert np.array_equal(th[b], th1) and sig[b] == sig1 and np.array_equal(info[b], info1)
    assert np.array_equal(huber.linear_regression_batch(Xh, yh), th)


def test_a_singular_problem_in_the_middle_is_flagged_alone(gpu):
    torch, ops, dev = gpu
    from rlvi_amd import huber, rrm
    Xh, yh = batch_of(40, 10, 5)
    clean = torch.from_numpy(Xh).to(dev)
    Xh[2, :, -1] = Xh[2, :, 0]
    dirty, y = torch.from_numpy(Xh).to(dev), torch.from_numpy(yh).to(dev)
    keep = [0, 1, 3, 4]
    for batch_fn, args, k in ((ops.rrm_linear_regression_batch, (0.2,), 40), (ops.huber_linear_regression_batch, (), 1)):
        th0, s0, info0 = (v.cpu().numpy() for v in batch_fn(clean, y, *args))
        theta = torch.full((5, 10), 7.0, dtype=torch.float64, device=dev)
        second = torch.full((5, k), 7.0, dtype=torch.float64, device=dev)
        th, s, info = (v.cpu().numpy() for v in batch_fn(dirty, y, *args, out=(theta, second)))
        s, s0 = s.reshape(5, -1), s0.reshape(5, -1)
        assert info[:, 3].tolist() == [0, 0, 1, 0, 0]
        assert (th[2] == 7.0).all() and (s[2] == 7.0).all()
        assert np.array_equal(th[keep], th0[keep]) and np.array_equal(s[keep], s0[keep])
        assert np.array_equal(info[keep], info0[keep])
    th, w, info = rrm.linear_regression_batch(Xh, yh, 0.2, return_info=True)
    assert info[:, 3].tolist() == [0, 0, 1, 0, 0] and np.isnan(th[2]).all() and np.isnan(w[2]).all()
    assert np.isfinite(th[keep]).all()
    th, sig, info = huber.linear_regression_batch(Xh, yh, return_info=True)
    assert info[:, 3].tolist() == [0, 0, 1, 0, 0] and np.isnan(th[2]).all() and np.isnan(sig[2])
    with pytest.raises(np.linalg.LinAlgError, match="problem 2"):
        huber.linear_regression_batch(Xh, yh)
    with pytest.raises(ValueError, match="problem 2"):
        rrm.linear_regression_batch(Xh, yh, 0.2)


def test_same_bits_under_graph_capture(gpu):
    """One ops call of each estimator captured and replayed (a single branch): the bits of the eager call."""
    torch, ops, dev = gpu
    key = "gen_257x20"
    X = torch.from_numpy(G19[key + "/X"].astype(np.float64)).to(dev)
    y = torch.from_numpy(G19[key + "/y"].astype(np.float64)).to(dev)
    n, d = X.shape
    for fn, args, k in ((ops.rrm_linear_regression, (0.2,), n), (ops.huber_linear_regression, (), 1)):
        eager = [t.cpu().numpy() for t in fn(X, y, *args)]
        assert eager[2][3] == 0 and eager[2][0] >= 1
        theta = torch.zeros(d, dtype=torch.float64, device=dev)
        second = torch.zeros(k, dtype=torch.float64, device=dev)
        info = torch.zeros(4, dtype=torch.int32, device=dev)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ws = ops.Workspace(dev, n, 0)
            fn(X, y, *args, out=(theta, second), info=info, ws=ws)                      # (warm-up outside the capture)
            torch.cuda.synchronize()
            theta.zero_()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                fn(X, y, *args, out=(theta, second), info=info, ws=ws)
            g.replay()
            torch.cuda.synchronize()
        assert np.array_equal(theta.cpu().numpy(), eager[0]) and np.array_equal(second.cpu().numpy(), eager[1])
        assert np.array_equal(info.cpu().numpy(), eager[2]) and ws.status() == 0
