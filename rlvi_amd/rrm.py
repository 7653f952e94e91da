"""MI355X mirror of standard-learning/rrm.py (Robust Risk Minimization, Osama et al. 2020): numpy in, numpy out, fp64,
the reference's names and argument order.

    update_weights(losses, eps)                                       reference rrm.py:12-33
    mean(sample, eps, maxiter=100, tol=1e-3)                          reference rrm.py:36-52
    pca(sample, eps, maxiter=100, tol=1e-2, theta_init=None)          reference rrm.py:94-107
    covariance(sample, eps, maxiter=100, tol=1e-2)                    reference rrm.py:110-124
    linear_regression(X, y, eps, maxiter=100, tol=1e-3)               reference rrm.py:55-73
    mean_batch / pca_batch / covariance_batch                         the loops of reference main.py:180-188, :489-494,
                                                                      :539-544: B problems of one shape in ONE launch
    linear_regression_batch                                           the sweep of reference main.py:261-273
    logistic_regression(X, y, eps, maxiter=100, tol=1e-2)             reference rrm.py:76-91
    logistic_regression_batch                                         the sweep of reference main.py:372-401

Every estimator is ONE launch of moments.hip (rlvi_rrm_*_f64) between one pinned copy in and one out, through the
staging helpers of rlvi_amd.standard; there is no host loop.  The weight rule returns the exact minimiser of the
reference's objective (the root of "entropy of w = log((1 - eps) n)") where the reference stops at Brent's tolerance:
the two agree to about 1e-8 in theta, not to the bit.  linear_regression (below) is ONE launch of
robust_linreg.hip, logistic_regression ONE launch of robust_logreg.hip (its fit is the minimiser liblinear approximates:
theta agrees to liblinear's tolerance).  return_info: (theta, weights, info int32[4] = {outer iterations,
evaluations of the last root-find, evaluations in all -- pca: Jacobi sweeps, logistic_regression: Newton steps in all --,
flag}).
"""
import numpy as np

from . import _lib, ops
from . import standard as _std


_NONFINITE = "array must not contain infs or NaNs"
_LOGREG_FLAG1 = ("y must hold the class labels 0 and 1, and the fit must not meet numbers that are not finite (a design "
                 "scaled beyond what fp64 resolves)")
# what the kernels' flags raise (standard._raise_flags); flag 1 of the single linear_regression is its general path
_UPDATE_FLAGS = {1: (ValueError, "{name}: a loss is not finite", False), 2: _std._CAP}
_LINREG_FLAGS = {2: (ValueError, _NONFINITE, False), 3: _std._CAP}
_LINREG_BATCH_FLAGS = {1: (ValueError, "{name}: a rank-deficient design (rrm.linear_regression takes its general path "
                                       "there)", False),
                       2: (ValueError, "{name}: " + _NONFINITE, False), 3: _std._CAP}
_LOGREG_FLAGS = {1: (ValueError, "{name}: " + _LOGREG_FLAG1, False), 2: _std._CAP, 3: _std._CAP}


def update_weights(losses, eps, *, return_info=False):
    '''Optimize sample weights for Robust Risk Minimization (reference rrm.py:12-33); n <= 4096.'''
    l = np.ascontiguousarray(losses, dtype=np.float64)
    if l.ndim != 1 or l.size == 0:
        raise ValueError("losses must be a vector of n >= 2 elements")
    if not np.isfinite(l).all():
        raise ValueError("Input contains NaN or infinity.")
    _std._rrm_eps("rrm.update_weights", eps, l.size)
    if l.size > 4096:
        raise _lib.RlviError(f"rrm.update_weights takes n <= 4096 losses in its one launch: got n = {l.size}")
    _, w, inf, _, ws = _std._one_launch_call("rrm.update_weights", ops.rrm_update_weights, [(l, None)], (eps,),
                                             l.size, (0,), (l.size,), pair=True)
    _std._raise_flags(ws, inf, return_info, "rrm.update_weights", _UPDATE_FLAGS)
    return (w, inf) if return_info else w


def mean(sample, eps, maxiter=100, tol=1e-3, *, return_info=False):
    """rrm.py:36-52 in ONE launch (2 <= n <= 4096, d <= 8, n d <= 16384: RlviError beyond)."""
    return _std._moments("mean", sample, maxiter, tol, return_info, eps=eps, rrm=True)


def pca(sample, eps, maxiter=100, tol=1e-2, theta_init=None, *, return_info=False):
    """rrm.py:94-107 in ONE launch; theta_init replaces the first fit and is used as is (utils.py:81-88)."""
    return _std._moments("pca", sample, maxiter, tol, return_info, theta_init=theta_init, eps=eps, rrm=True)


def covariance(sample, eps, maxiter=100, tol=1e-2, *, return_info=False):
    """rrm.py:110-124 in ONE launch; ValueError("Singular covariance matrix") as utils.py:99-100."""
    return _std._moments("covariance", sample, maxiter, tol, return_info, eps=eps, rrm=True)


def mean_batch(sample, eps, maxiter=100, tol=1e-3, *, return_info=False):
    """B calls of mean as ONE launch: sample [B, n, d] -> theta [B, d]; with return_info (theta, weights [B, n], info
    int32[B, 4]), a flagged problem's rows NaN and nothing raised."""
    return _std._moments("mean", sample, maxiter, tol, return_info, eps=eps, rrm=True, batch=True)


def pca_batch(sample, eps, maxiter=100, tol=1e-2, theta_init=None, *, return_info=False):
    """B calls of pca as ONE launch: sample [B, n, d], ONE theta_init [d] for all problems -> theta [B, d]."""
    return _std._moments("pca", sample, maxiter, tol, return_info, theta_init=theta_init, eps=eps, rrm=True,
                        batch=True)


def covariance_batch(sample, eps, maxiter=100, tol=1e-2, *, return_info=False):
    """B calls of covariance as ONE launch: sample [B, n, d], ONE eps for all problems -> theta [B, d, d]."""
    return _std._moments("covariance", sample, maxiter, tol, return_info, eps=eps, rrm=True, batch=True)


def _linreg_limits(what, n, d):
    if n == 0 or d == 0 or not ops.linear_regression_check(n, d):
        raise _lib.RlviError(f"{what} takes n <= 4096 samples and 1 <= d <= 31 features in its one launch: got "
                             f"n = {n}, d = {d}")


def _linreg_inputs(what, X, y):
    # (not finite: what scipy's lstsq (check_finite) raises at rrm.py:58)
    Xh, yh, n, d = _std._design_inputs(X, y, nonfinite=_NONFINITE)
    _linreg_limits(what, n, d)
    return Xh, yh, n, d


def _linear_regression_host_loop(X, y, eps, maxiter, tol, ws):
    """The general path of linear_regression (a design the one launch reports as rank-deficient: the reference's lstsq
    returns the minimum-norm solution there): one launch per statement of rrm.py:56-71 and the stop test on the host.
    X, y: device tensors.  Returns (theta, weights, outer) as numpy arrays."""
    import torch
    n = X.shape[0]
    w = torch.full((n,), 1.0 / n, dtype=torch.float64, device=X.device)
    theta = _std._wls(X, y, w)                                       # rrm.py:57-58
    losses = (y - X @ theta) ** 2                                    # rrm.py:59
    outer = 0
    for _ in range(maxiter):
        outer += 1
        w, inf = ops.rrm_update_weights(losses, eps, ws=ws)          # rrm.py:62
        flag = int(inf[3])
        if flag == 1:
            ws.clear_status()
            raise ValueError("array must not contain infs or NaNs")
        if flag == 2:
            ws.raise_on_status("rrm.linear_regression", mask=_lib.ST_NOCONV)
        prev = theta
        theta = _std._wls(X, y, w)                                   # rrm.py:65-66
        losses = (y - X @ theta) ** 2                                # rrm.py:67
        if bool(torch.linalg.norm(theta - prev) / torch.linalg.norm(prev) <= tol):     # rrm.py:69-71
            break
    th = theta.cpu().numpy()
    ws.raise_on_status("rrm.linear_regression", mask=_lib.ST_TIMEOUT | _lib.ST_NOCONV)
    ws.clear_status()                                                # (RLVI_ST_SINGULAR is information here)
    if not np.isfinite(th).all():
        raise ValueError("array must not contain infs or NaNs")
    return th, w.cpu().numpy(), outer


def linear_regression(X, y, eps, maxiter=100, tol=1e-3, *, return_info=False):
    """rrm.py:55-73 in ONE launch (n <= 4096, d <= 31: RlviError beyond).  A design the launch reports as
    rank-deficient -- or one that weights of exactly 0 make so -- is recomputed by the general path (ops.rrm_update_weights
    + the minimum-norm least-squares solve, one launch per statement), as the reference's lstsq handles it; info is
    then {its outer iterations, 0, 0, 1}."""
    Xh, yh, n, d = _linreg_inputs("rrm.linear_regression", X, y)
    _std._rrm_eps("rrm.linear_regression", eps, n)
    theta, w, inf, (Xd, yd), ws = _std._one_launch_call("rrm.linear_regression", ops.rrm_linear_regression,
                                                        [(Xh, (n, d)), (yh, None)], (eps, maxiter, tol), n, (d,), (n,),
                                                        pair=True)
    if inf[3] == 1:
        th, wh, outer = _linear_regression_host_loop(Xd.view(n, d), yd, eps, maxiter, tol, ws)
        return (th, wh, np.array([outer, 0, 0, 1], np.int32)) if return_info else th
    bad = _std._raise_flags(ws, inf, return_info, "rrm.linear_regression", _LINREG_FLAGS)
    return _std._results(theta, w, inf, bad, return_info)


def linear_regression_batch(X, y, eps, maxiter=100, tol=1e-3, *, return_info=False):
    """B calls of linear_regression (the sweep of main.py:261-273) as ONE launch: X [B, n, d], y [B, n], one eps for
    all -> theta [B, d]; every problem has the bits of its single one-launch call.  A flagged problem raises what the
    single call's launch reports for it (flag 1: a rank-deficient design -- the batch form has no general path), naming
    the problem; with return_info (theta, weights [B, n], info int32[B, 4]) nothing is raised and its rows are NaN."""
    Xh, yh, B, n, d = _std._batch_inputs("X", X, y, nonfinite=_NONFINITE)
    _linreg_limits("rrm.linear_regression_batch", n, d)
    _std._rrm_eps("rrm.linear_regression_batch", eps, n)
    theta, w, inf, _, ws = _std._one_launch_call("rrm.linear_regression_batch", ops.rrm_linear_regression_batch,
                                                 [(Xh, (B, n, d)), (yh, (B, n))], (eps, maxiter, tol), n, (d,), (n,),
                                                 batch=B, pair=True)
    bad = _std._raise_flags(ws, inf, return_info, "rrm.linear_regression_batch", _LINREG_BATCH_FLAGS, batch=True)
    return _std._results(theta, w, inf, bad, return_info)


def _logreg_checks(what, yh, n, d, eps, problems=False):
    """What is raised before anything reaches the device: labels of a single class (sklearn's message, as
    standard.logistic_regression(solver="newton")), shapes beyond the one launch, eps out of range."""
    y2 = yh.reshape(-1, n) if n else yh.reshape(1, 0)
    one = np.ones(len(y2), bool) if n == 0 else y2.min(axis=1) == y2.max(axis=1)
    if one.any():
        where = f" (problem {int(np.argmax(one))})" if problems else ""
        raise ValueError(f"This solver needs samples of at least 2 classes in the data{where}")
    if d == 0 or not ops.logistic_regression_check(n, d):
        raise _lib.RlviError(f"{what} takes n <= 4096 samples and 1 <= d <= 30 features in its one launch: got "
                             f"n = {n}, d = {d}")
    _std._rrm_eps(what, eps, n)


def logistic_regression(X, y, eps, maxiter=100, tol=1e-2, *, return_info=False):
    """rrm.py:76-91 in ONE launch (n <= 4096, 1 <= d <= 30: RlviError beyond) -> theta [d + 1] = (intercept, coef).
    Each fit is the minimiser liblinear approximates to its tol = 1e-4 and each weight update the exact root of the
    rule, so theta agrees with the reference's to liblinear's tolerance, not to the bit.  Reaching maxiter is silent,
    as in the reference.  return_info: (theta, weights [n], info int32[4] = {outer iterations, evaluations of the last
    root-find, Newton steps in all, flag})."""
    # (not finite: what sklearn's fit raises a ValueError for, utils.py:68)
    Xh, yh, n, d = _std._design_inputs(X, y)
    _logreg_checks("rrm.logistic_regression", yh, n, d, eps)
    theta, w, inf, _, ws = _std._one_launch_call("rrm.logistic_regression", ops.rrm_logistic_regression,
                                                 [(Xh, (n, d)), (yh, None)], (eps, maxiter, tol), n, (d + 1,), (n,),
                                                 pair=True)
    bad = _std._raise_flags(ws, inf, return_info, "rrm.logistic_regression", _LOGREG_FLAGS)
    return _std._results(theta, w, inf, bad, return_info)


def logistic_regression_batch(X, y, eps, maxiter=100, tol=1e-2, *, return_info=False):
    """B calls of logistic_regression (the sweep of main.py:372-401) as ONE launch: X [B, n, d], y [B, n] of 0 / 1 with
    both classes in every problem, one eps for all -> theta [B, d + 1]; every problem has the bits of its single call.
    A flagged problem raises what its single call raises, naming the problem; with return_info (theta, weights [B, n],
    info int32[B, 4]) nothing is raised and its rows are NaN."""
    Xh, yh, B, n, d = _std._batch_inputs("X", X, y)
    _logreg_checks("rrm.logistic_regression_batch", yh, n, d, eps, problems=True)
    theta, w, inf, _, ws = _std._one_launch_call("rrm.logistic_regression_batch", ops.rrm_logistic_regression_batch,
                                                 [(Xh, (B, n, d)), (yh, (B, n))], (eps, maxiter, tol), n, (d + 1,),
                                                 (n,), batch=B, pair=True)
    bad = _std._raise_flags(ws, inf, return_info, "rrm.logistic_regression_batch", _LOGREG_FLAGS, batch=True)
    return _std._results(theta, w, inf, bad, return_info)
