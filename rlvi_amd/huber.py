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
# what the kernel's flags raise (standard._raise_flags): the cap has a message of its own, not the status word's
_FLAGS = {1: (np.linalg.LinAlgError, "Singular matrix", False), 2: (ValueError, _NONFINITE, False),
          3: (_lib.RlviError, "{name}: the iteration still moved by more than 1e-6 after maxiter = {maxiter} "
                              "iterations", True)}


def psi_huber(vec, c):
    """huber.py:5-10 (host; the kernel applies it as a clip of the residuals at c sigma)."""
    vec = np.asarray(vec, np.float64)
    return np.where(np.abs(vec) <= c, vec, c * np.sign(vec))


def _params(what, c, sigma0, maxiter):
    if not (c > 0.0 and sigma0 > 0.0 and np.isfinite(c) and np.isfinite(sigma0)):
        raise ValueError(f"{what} needs c > 0 and sigma0 > 0: got c = {c}, sigma0 = {sigma0}")
    if maxiter < 0:
        raise ValueError(f"{what} needs maxiter >= 0: got {maxiter}")


def linear_regression(X, y, c=0.7317, sigma0=1, *, maxiter=1000, return_info=False):
    """huber.py:13-40 in ONE launch (n <= 4096, d <= 31: RlviError beyond).  numpy.linalg.LinAlgError("Singular
    matrix") where numpy.linalg.solve raises it at huber.py:17; ValueError for input that is not finite and for an
    exactly interpolating fit (sigma = 0: the reference's lstsq meets a NaN); RlviError when the cap is reached."""
    Xh, yh, n, d = _rrm._linreg_inputs("huber.linear_regression", X, y)
    _params("huber.linear_regression", c, sigma0, maxiter)
    theta, scale, inf, _, ws = _std._one_launch_call("huber.linear_regression", ops.huber_linear_regression,
                                                     [(Xh, (n, d)), (yh, None)], (c, sigma0, maxiter), n, (d,), (),
                                                     pair=True)
    _std._raise_flags(ws, inf, return_info, "huber.linear_regression", _FLAGS, maxiter=maxiter)
    return (theta, float(scale), inf) if return_info else theta


def linear_regression_batch(X, y, c=0.7317, sigma0=1, *, maxiter=1000, return_info=False):
    """B calls of linear_regression (the sweep of main.py:261-273) as ONE launch: X [B, n, d], y [B, n], one c and one
    sigma0 for all -> theta [B, d]; every problem has the bits of its single call.  A flagged problem raises what the
    single call raises for it, naming the problem; with return_info (theta, sigma [B], info int32[B, 4]) nothing is
    raised and its rows are NaN."""
    Xh, yh, B, n, d = _std._batch_inputs("X", X, y, nonfinite=_NONFINITE)
    _rrm._linreg_limits("huber.linear_regression_batch", n, d)
    _params("huber.linear_regression_batch", c, sigma0, maxiter)
    theta, scale, inf, _, ws = _std._one_launch_call("huber.linear_regression_batch", ops.huber_linear_regression_batch,
                                                     [(Xh, (B, n, d)), (yh, (B, n))], (c, sigma0, maxiter), n, (d,), (),
                                                     batch=B, pair=True)
    bad = _std._raise_flags(ws, inf, return_info, "huber.linear_regression_batch", _FLAGS, batch=True, maxiter=maxiter)
    return _std._results(theta, scale, inf, bad, return_info)
