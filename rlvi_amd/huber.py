"""MI355X mirror of standard-learning/huber.py (Huber's M-estimator of regression with a concomitant scale): numpy in,
numpy out, fp64, the reference's names and argument order.

    psi_huber(vec, c)                                         reference huber.py:5-10
    linear_regression(X, y, c=0.7317, sigma0=1)               reference huber.py:13-40
    linear_regression_batch                                   the sweep of reference main.py:261-273 around it

linear_regression is ONE launch of robust_linreg.hip (rlvi_huber_linear_regression_f64) between one pinned copy in and
one out, through the staging helpers of rlvi_amd.standard: X^T X is formed and factored once, every iteration is the
residuals, two clips, one sum for the scale, X^T r_psi and one substitution; there is no host loop.  The reference's
`while True` is capped: maxiter (1000; it takes 38 .. 63 iterations on the reference's designs) -- a run that still
moves at the cap raises RlviError, it is never returned silently.  alpha (huber.py:15) is computed with erf where the
reference calls scipy.stats.chi2.cdf: the two agree to 1e-15.  return_info: (theta, sigma, info int32[4] = {iterations,
0, 0, flag}).
"""
import numpy as np

from . import _lib, ops
from . import rrm as _rrm
from . import standard as _std

_NONFINITE = "array must not contain infs or NaNs"
_FLAGS = {1: "Singular matrix", 2: _NONFINITE}


def psi_huber(vec, c):
    """huber.py:5-10 (host; the kernel applies it as a clip of the residuals at c sigma)."""
    vec = np.asarray(vec, np.float64)
    return np.where(np.abs(vec) <= c, vec, c * np.sign(vec))


def _params(what, c, sigma0, maxiter):
    if not (c > 0.0 and sigma0 > 0.0 and np.isfinite(c) and np.isfinite(sigma0)):
        raise ValueError(f"{what} needs c > 0 and sigma0 > 0: got c = {c}, sigma0 = {sigma0}")
    if maxiter < 0:
        raise ValueError(f"{what} needs maxiter >= 0: got {maxiter}")


def _capped(what, ws, maxiter, where=""):
    ws.clear_status()
    raise _lib.RlviError(f"{what}: the iteration still moved by more than 1e-6 after maxiter = {maxiter} "
                         f"iterations{where}")


def linear_regression(X, y, c=0.7317, sigma0=1, *, maxiter=1000, return_info=False):
    """huber.py:13-40 in ONE launch (n <= 4096, d <= 31: RlviError beyond).  numpy.linalg.LinAlgError("Singular
    matrix") where numpy.linalg.solve raises it at huber.py:17; ValueError for input that is not finite and for an
    exactly interpolating fit (sigma = 0: the reference's lstsq meets a NaN); RlviError when the cap is reached."""
    Xh, yh, n, d = _rrm._linreg_inputs("huber.linear_regression", X, y)
    _params("huber.linear_regression", c, sigma0, maxiter)
    dev = _std._dev()
    ws = ops.workspace(dev, n, 0)
    theta, scale, inf, _ = _std._one_launch_roundtrip(
        dev, "huber_linreg", [(Xh, n * d), (yh, n)], d, 1,
        lambda v, out: ops.huber_linear_regression(v[0].view(n, d), v[1], c, sigma0, maxiter=maxiter,
                                                   out=(out["theta"], out["weights"]), info=out["info"], ws=ws))
    inf = inf.copy()
    if inf[3] == 1:
        raise np.linalg.LinAlgError(_FLAGS[1])
    if inf[3] == 2:
        raise ValueError(_NONFINITE)
    if inf[3] == 3:
        _capped("huber.linear_regression", ws, maxiter)
    return (theta.copy(), float(scale[0]), inf) if return_info else theta.copy()


def linear_regression_batch(X, y, c=0.7317, sigma0=1, *, maxiter=1000, return_info=False):
    """B calls of linear_regression (the sweep of main.py:261-273) as ONE launch: X [B, n, d], y [B, n], one c and one
    sigma0 for all -> theta [B, d]; every problem has the bits of its single call.  A flagged problem raises what the
    single call raises for it, naming the problem; with return_info (theta, sigma [B], info int32[B, 4]) nothing is
    raised and its rows are NaN."""
    Xh, yh, B, n, d = _std._batch_inputs("X", X, y, nonfinite=_NONFINITE)
    if n == 0 or d == 0 or not ops.linear_regression_check(n, d):
        raise _lib.RlviError(f"huber.linear_regression_batch takes n <= 4096 samples and 1 <= d <= 31 features in its "
                             f"one launch: got n = {n}, d = {d}")
    _params("huber.linear_regression_batch", c, sigma0, maxiter)
    dev = _std._dev()
    ws = ops.workspace(dev, n, 0)
    theta, scale, inf, _ = _std._one_launch_roundtrip(
        dev, "huber_linreg_batch", [(Xh, B * n * d), (yh, B * n)], d, 1,
        lambda v, out: ops.huber_linear_regression_batch(v[0].view(B, n, d), v[1].view(B, n), c, sigma0,
                                                         maxiter=maxiter, out=(out["theta"], out["weights"]),
                                                         info=out["info"], ws=ws), batch=B)
    inf = inf.copy().reshape(B, 4)
    flagged = np.flatnonzero(inf[:, 3] != 0)
    if flagged.size and (inf[:, 3] == 3).any():
        ws.clear_status()
    if flagged.size and not return_info:
        b = int(flagged[0])
        if inf[b, 3] == 1:
            raise np.linalg.LinAlgError(f"{_FLAGS[1]} (problem {b})")
        if inf[b, 3] == 2:
            raise ValueError(f"{_NONFINITE} (problem {b})")
        _capped("huber.linear_regression_batch", ws, maxiter, f" (problem {b})")
    if not return_info:
        return theta.copy().reshape(B, d)
    theta, scale, inf = _std._batch_results(theta, scale, inf, B, (d,), 1, True)
    return theta, scale.reshape(B), inf
