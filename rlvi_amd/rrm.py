"""MI355X mirror of standard-learning/rrm.py (Robust Risk Minimization, Osama et al. 2020): numpy in, numpy out, fp64,
the reference's names and argument order.

    update_weights(losses, eps)                                       reference rrm.py:12-33
    mean(sample, eps, maxiter=100, tol=1e-3)                          reference rrm.py:36-52
    pca(sample, eps, maxiter=100, tol=1e-2, theta_init=None)          reference rrm.py:94-107
    covariance(sample, eps, maxiter=100, tol=1e-2)                    reference rrm.py:110-124
    mean_batch / pca_batch / covariance_batch                         the loops of reference main.py:180-188, :489-494,
                                                                      :539-544: B problems of one shape in ONE launch

Every estimator is ONE launch of moments.hip (rlvi_rrm_*_f64) between one pinned copy in and one out, through the
staging helpers of rlvi_amd.standard; there is no host loop.  The weight rule returns the exact minimiser of the
reference's objective (the root of "entropy of w = log((1 - eps) n)") where the reference stops at Brent's tolerance:
the two agree to about 1e-8 in theta, not to the bit.  linear_regression and logistic_regression under RRM
are not mirrored.  return_info: (theta, weights, info int32[4] = {outer iterations, evaluations of the last root-find,
evaluations in all -- pca: Jacobi sweeps in all --, flag}).
"""
import numpy as np

from . import _lib, ops
from . import standard as _std


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
    dev = _std._dev()
    ws = ops.workspace(dev, l.size, 0)
    _, w, inf, _ = _std._one_launch_roundtrip(
        dev, "rrm_update_weights", [(l, l.size)], 0, l.size,
        lambda v, out: ops.rrm_update_weights(v[0], eps, out=out["weights"], info=out["info"], ws=ws))
    inf = inf.copy()
    if inf[3] == 1:
        raise ValueError("rrm.update_weights: a loss is not finite")
    if inf[3] == 2:
        ws.raise_on_status("rrm.update_weights", mask=_lib.ST_NOCONV)
    return (w.copy(), inf) if return_info else w.copy()


def mean(sample, eps, maxiter=100, tol=1e-3, *, return_info=False):
    """rrm.py:36-52 in ONE launch (2 <= n <= 4096, d <= 8, n d <= 16384: RlviError beyond)."""
    return _std._moments_one_launch("mean", sample, maxiter, tol, return_info, eps=eps, rrm=True)


def pca(sample, eps, maxiter=100, tol=1e-2, theta_init=None, *, return_info=False):
    """rrm.py:94-107 in ONE launch; theta_init replaces the first fit and is used as is (utils.py:81-88)."""
    return _std._moments_one_launch("pca", sample, maxiter, tol, return_info, theta_init=theta_init, eps=eps, rrm=True)


def covariance(sample, eps, maxiter=100, tol=1e-2, *, return_info=False):
    """rrm.py:110-124 in ONE launch; ValueError("Singular covariance matrix") as utils.py:99-100."""
    return _std._moments_one_launch("covariance", sample, maxiter, tol, return_info, eps=eps, rrm=True)


def mean_batch(sample, eps, maxiter=100, tol=1e-3, *, return_info=False):
    """B calls of mean as ONE launch: sample [B, n, d] -> theta [B, d]; with return_info (theta, weights [B, n], info
    int32[B, 4]), a flagged problem's rows NaN and nothing raised."""
    return _std._moments_batch("mean", sample, maxiter, tol, return_info, eps=eps, rrm=True)


def pca_batch(sample, eps, maxiter=100, tol=1e-2, theta_init=None, *, return_info=False):
    """B calls of pca as ONE launch: sample [B, n, d], ONE theta_init [d] for all problems -> theta [B, d]."""
    return _std._moments_batch("pca", sample, maxiter, tol, return_info, theta_init=theta_init, eps=eps, rrm=True)


def covariance_batch(sample, eps, maxiter=100, tol=1e-2, *, return_info=False):
    """B calls of covariance as ONE launch: sample [B, n, d], ONE eps for all problems -> theta [B, d, d]."""
    return _std._moments_batch("covariance", sample, maxiter, tol, return_info, eps=eps, rrm=True)
