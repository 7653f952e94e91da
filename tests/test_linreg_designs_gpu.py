"""Linear regression on designs beyond synth.linreg_data's range (columns uniform in [-5, 5], condition number 1.4),
on the GPU: the weighted solve of the general path (wls.hip) and the one-launch estimator (standard.hip), single and
batched.  The pieces and their CPU premises are tests/linreg_designs.py and tests/test_linreg_designs_cpu.py.

  a  a column scaled by a power of two -- down to 2^-200, up to 2^200, at the first, the last and the 17th position, or
     all columns graded over 2^40 -- changes NO BIT of the solution (times 2^k) and is not read as rank deficiency: the
     pivot test is on 1 - R^2, pivot against the column's own diagonal entry;
  b  the same for the whole estimator: bit for bit where no stop decision is taken (the stop test ||theta - prev|| /
     ||prev|| is not scale-invariant, in the reference either), and count for count against the oracle on the scaled
     design where one is;
  c  conditioning that no scaling removes costs kappa_eq^2 eps, against the exact rational solution;
  d  rank deficiency is still named, scaled or not;
  e  a scaled problem in the middle of a batch stays in the one launch;
  f  a NaN or inf in y alone raises the reference's error at maxiter = 0 too.
Each test goes through all of its patterns, prints what it found and asserts at the end, so that a failing build shows
WHICH patterns it fails (pytest -s)."""
import numpy as np
import pytest

import linreg_designs as L
from test_gpu_parity import dev_status
from test_gpu_parity import gpu, no_process_state_left_behind  # noqa: F401  (fixtures: the device, the hygiene check)

pytestmark = pytest.mark.gpu

ALL_SHAPES = L.SHAPES + [s for s in L.EXACT_SHAPES if s not in L.SHAPES]
ST_SINGULAR = 8


def bar(kq):
    """C kappa_eq^2 eps: C = 8 R_MEASURED rounded up to a power of two (tests/linreg_designs.py)"""
    return L.C_BAR * kq * kq * L.EPS


@pytest.mark.parametrize("n,d", ALL_SHAPES)
def test_wls_solve_is_invariant_under_column_scaling(n, d, gpu):
    """ops.wls_solve (Gram matrix on the matrix cores, Cholesky in one workgroup) on every scaling pattern: theta 2^k
    has the bits of the unscaled call's theta -- every product, sum and division of the path commutes with a power of
    two, and so does the square root of a pivot scaled by 2^2k -- and RLVI_ST_SINGULAR is not raised.  At the shapes
    where the exact rational solve is affordable theta is within C kappa_eq^2 eps of it."""
    torch, ops, dev = gpu
    X, y = L.base(n, d)
    w = L.weights(n)
    yd, wd = torch.from_numpy(y).to(dev), torch.from_numpy(w).to(dev)
    th0 = ops.wls_solve(torch.from_numpy(X).to(dev), yd, wd).cpu().numpy()
    assert dev_status(ops, dev) == 0 and np.isfinite(th0).all()
    ws = ops.workspace(dev)
    flagged, moved = [], []
    for name, kv in L.patterns(d):
        th = ops.wls_solve(torch.from_numpy(L.scaled(X, kv)).to(dev), yd, wd).cpu().numpy()
        if ws.status() & ST_SINGULAR:
            flagged.append(name)
        elif not np.array_equal(L.unscale(th, kv), th0):
            moved.append((name, float(np.max(np.abs(L.unscale(th, kv) / th0 - 1)))))
        ws.clear_status()
    print(f"{n} x {d}: read as rank-deficient {flagged}; bits moved {moved}")
    assert not flagged and not moved
    if (n, d) in L.EXACT_SHAPES:
        _, _, _, exact, kq = L.exact_case(n, d, "base", True)
        err = L.rel_err(th0, exact)
        print(f"{n} x {d}: error against the exact solution {err:.3g} = {err / (kq * kq * L.EPS):.3f} kappa_eq^2 eps "
              f"(kappa_eq {kq:.3g}, bar {bar(kq):.3g})")
        assert err <= bar(kq)


@pytest.mark.parametrize("n,d", L.SHAPES)
def test_one_launch_without_a_stop_decision_is_invariant_under_column_scaling(n, d, gpu):
    """ops.linear_regression with tol = 0, maxiter = 3 -- three outer iterations whatever theta does -- on every
    scaling pattern: info[3] = 0, theta 2^k AND the weights have the bits of the unscaled launch, the outer and inner
    counts are the same (the residuals x_ij theta_j are the same products, so the E-step sees the same losses)."""
    torch, ops, dev = gpu
    X, y = L.base(n, d)
    yd = torch.from_numpy(y).to(dev)

    def run(Xs):
        th, w, info = ops.linear_regression(torch.from_numpy(Xs).to(dev), yd, maxiter=3, tol=0.0)
        return th.cpu().numpy(), w.cpu().numpy(), info.cpu().numpy()
    th0, w0, info0 = run(X)
    assert info0[3] == 0 and info0[0] == 3, info0
    flagged, moved = [], []
    for name, kv in L.patterns(d):
        th, w, info = run(L.scaled(X, kv))
        if info[3] != 0:
            flagged.append(name)
        elif not (np.array_equal(L.unscale(th, kv), th0) and np.array_equal(w, w0) and np.array_equal(info, info0)):
            moved.append((name, info.tolist(), float(np.max(np.abs(L.unscale(th, kv) / th0 - 1))),
                          float(np.max(np.abs(w - w0)))))
    print(f"{n} x {d}: info {info0.tolist()}; read as rank-deficient {flagged}; bits moved {moved}")
    assert not flagged and not moved
    assert dev_status(ops, dev) == 0


@pytest.mark.parametrize("n,d", L.SHAPES)
def test_one_launch_on_scaled_designs_vs_oracle(n, d, gpu, oracle):
    """ops.linear_regression with the default tol and maxiter on every pattern the oracle is a reference for
    (linreg_designs.ORACLE_K: one column scaled by 2^-12, 2^-21, 2^-30 or 2^27, at every position): info[3] = 0, the
    outer count is the oracle's on the SCALED design (test_outer_counts_are_clear_of_the_edge keeps these cases away
    from tol), theta 2^k agrees with the oracle's to 1e-6 -- the precision of the oracle's lstsq on such a design --
    and the numpy mirror returns the bits of the device call and leaves the workspace status 0."""
    torch, ops, dev = gpu
    from rlvi_amd import standard
    X, y = L.base(n, d)
    yd = torch.from_numpy(y).to(dev)
    bad = []
    for name, kv in L.oracle_patterns(d):
        Xs = L.scaled(X, kv)
        th_o, w_o, outer_o = oracle.linear_regression(Xs, y, trace=True)
        th, w, info = ops.linear_regression(torch.from_numpy(Xs).to(dev), yd)
        th, w, info = th.cpu().numpy(), w.cpu().numpy(), info.cpu().numpy()
        if info[3] != 0:
            bad.append((name, "read as rank-deficient"))
            continue
        dth = float(np.max(np.abs(L.unscale(th, kv) / L.unscale(th_o, kv) - 1)))
        print(f"{n} x {d} {name}: outer {info[0]} (oracle {outer_o}), theta against the oracle {dth:.3g}")
        if info[0] != outer_o:
            bad.append((name, f"outer {info[0]}, oracle {outer_o}"))
            continue
        if not np.allclose(L.unscale(th, kv), L.unscale(th_o, kv), rtol=1e-6, atol=0.0):
            bad.append((name, f"theta {dth}"))
        th_m, w_m, outer_m = standard.linear_regression(Xs, y, return_info=True)
        if not (outer_m == info[0] and np.array_equal(th_m, th) and np.array_equal(w_m, w)):
            bad.append((name, "the mirror left the one launch"))
        if dev_status(ops, dev) != 0:
            bad.append((name, f"status {dev_status(ops, dev)}"))
            ops.workspace(dev).clear_status()
    print(f"{n} x {d}: {bad}")
    assert not bad


@pytest.mark.parametrize("n,d", L.EXACT_SHAPES)
def test_conditioning_ladder_vs_the_exact_solution(n, d, gpu):
    """Columns 1e2 ... 1e4 from the origin and a last column within 1e-3 / 1e-5 of the first (kappa_eq up to 4e5)
    through ops.wls_solve with weights(n) and through ops.linear_regression(maxiter=0): accepted as full rank, and
    max_j |theta_j - exact_j| / max_j |exact_j| <= C kappa_eq^2 eps against the exact rational solution -- at the
    ladder's worst below 1e-3, where a wrong or dropped coefficient is an error of order one."""
    torch, ops, dev = gpu
    bad = []
    for case in L.LADDER_CASES:
        for weighted in (True, False):
            X, y, w, exact, kq = L.exact_case(n, d, case, weighted)
            Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
            if weighted:
                th = ops.wls_solve(Xd, yd, torch.from_numpy(w).to(dev)).cpu().numpy()
                ok = dev_status(ops, dev) == 0
                ops.workspace(dev).clear_status()
            else:
                th, wo, info = ops.linear_regression(Xd, yd, maxiter=0)
                th, info = th.cpu().numpy(), info.cpu().numpy()
                ok = info[3] == 0 and info[0] == 0 and bool((wo == 1.0).all())
            err = L.rel_err(th, exact) if ok else float("nan")
            print(f"{n} x {d} {case:14s} {'wls_solve' if weighted else 'one launch'}: kappa_eq {kq:9.3g} error "
                  f"{err:9.3g} = {err / (kq * kq * L.EPS):6.3f} kappa_eq^2 eps (bar {bar(kq):.3g})")
            if not ok or not err <= bar(kq):
                bad.append((case, weighted, ok, err))
    assert not bad, bad


@pytest.mark.parametrize("n,d", L.SHAPES)
def test_rank_deficiency_is_still_named(n, d, gpu):
    """A duplicated column, a duplicate times 2^-23, an all-zero column: the one launch ends with info[3] = 1 and
    leaves theta alone, the general path raises RLVI_ST_SINGULAR and returns the minimum-norm solution -- numpy's
    lstsq for the two well-scaled designs.  For the scaled duplicate only the flag and a finite theta are asserted: the
    minimum-norm solution is not scale-invariant, and the general path's cutoff on the eigenvalues of the Gram matrix
    (lambda_max d 64 eps) cannot follow gelsd's on the singular values of X there -- a remaining limit."""
    torch, ops, dev = gpu
    X, y = L.base(n, d)
    yd = torch.from_numpy(y).to(dev)
    ones = torch.ones(n, dtype=torch.float64, device=dev)
    ws = ops.workspace(dev)
    for case, Z in L.rank_deficient(X).items():
        Zd = torch.from_numpy(Z).to(dev)
        theta = torch.full((d,), 7.0, dtype=torch.float64, device=dev)
        _, _, info = ops.linear_regression(Zd, yd, theta=theta)
        assert int(info.cpu()[3]) == 1 and bool((theta == 7.0).all()), case
        assert ws.status() == 0
        th = ops.wls_solve(Zd, yd, ones).cpu().numpy()
        st = ws.status()
        ws.clear_status()
        print(f"{n} x {d} {case}: info[3] 1, status {st}")
        assert st == ST_SINGULAR and np.isfinite(th).all(), case
        if case != "duplicate*2^-23":
            np.testing.assert_allclose(th, np.linalg.lstsq(Z, y, rcond=None)[0], rtol=1e-8, atol=1e-10, err_msg=case)


@pytest.mark.parametrize("n,d", L.SHAPES)
def test_batch_with_a_scaled_problem_stays_in_the_one_launch(n, d, gpu):
    """standard.linear_regression_batch on five problems, problem 2 with its last column scaled by 2^-30: no problem
    leaves the launch (info[:, 3] = 0) and every problem has the bits of its single call."""
    torch, ops, dev = gpu
    from rlvi_amd import standard, synth
    B = 5
    Xs, ys = zip(*(synth.linreg_data(n, d, eps=0.3, nu=2.5, seed=9000 + n + d + b) for b in range(B)))
    X, y = np.stack(Xs), np.stack(ys)
    kv = np.zeros(d, dtype=np.int64)
    kv[d - 1] = -30
    X[2] = L.scaled(X[2], kv)
    theta, w, info = standard.linear_regression_batch(X, y, return_info=True)
    print(f"{n} x {d}: info {info.tolist()}")
    assert (info[:, 3] == 0).all(), info
    for b in range(B):
        th1, w1, outer1 = standard.linear_regression(X[b], y[b], return_info=True)
        assert outer1 == info[b, 0] and np.array_equal(th1, theta[b]) and np.array_equal(w1, w[b]), b
    assert dev_status(ops, dev) == 0


@pytest.mark.parametrize("maxiter", [0, 100])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_y_raises_the_references_error(value, maxiter, gpu):
    """A NaN or inf in y with a finite X: the Gram matrix X^T W X is finite and the pivot test passes, so with
    maxiter = 0 the one launch returns a non-finite theta with info[3] = 0 -- the mirror raises what the reference's
    lstsq raises (check_finite), as its general path does, and leaves no status behind."""
    torch, ops, dev = gpu
    from rlvi_amd import standard
    X, y = L.base(40, 10)
    y = y.copy()
    y[3] = value
    with pytest.raises(ValueError, match="array must not contain infs or NaNs"):
        standard.linear_regression(X, y, maxiter=maxiter)
    assert dev_status(ops, dev) == 0
