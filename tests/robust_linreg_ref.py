"""Float64 numpy restatement of rlvi_amd/csrc/robust_linreg.hip (test infrastructure; imports nothing of the product).

    rrm_linear_regression(X, y, eps, maxiter, tol)          -> (theta, weights, outer, trace)     rrm.py:55-73
    huber_alpha(c)                                          -> alpha                              huber.py:15
    huber_linear_regression(X, y, c, sigma0, maxiter)       -> (theta, sigma, iterations, trace)  huber.py:13-40

The same algorithms as the kernels; only the order of the sums and the factorisation of the normal equations differ
(numpy.linalg.solve / scipy's Cholesky here, a straight-line L D L^T there).
  * RRM: weights 1 / n, theta = the weighted least-squares fit from the normal equations, losses = (y - X theta)^2; then
    `maxiter` times { rrm_ref.update_weights (the exact entropy root), theta and losses again, stop when
    ||theta - prev|| / ||prev|| <= tol } -- the test comes after each refit, maxiter = 0 returns the first fit.  `steps`,
    if a list, receives (losses in, weights out) of every E-step.
  * Huber: X^T X factored once; theta0 = its solve with X^T y; an iteration is r = y - X theta0, the clip of r at
    c sigma0, sigma = sqrt(sum of its squares / (2 n alpha)), the clip of r at c sigma, delta = the solve with X^T of it,
    theta = theta0 + delta; it goes on while ||theta - theta0|| / ||theta0|| > 1e-6 (sigma0 <- sigma, theta0 <- theta), at
    most maxiter times.  sigma psi(r / sigma, c) of the reference is that clip up to one rounding.  A scale that is not
    positive and finite raises FloatingPointError (the kernel's flag 2).
`trace` holds the discrepancy of every stop decision.
"""
import math

import numpy as np

import rrm_ref


def wls(X, y, w):
    """argmin sum w_i (y_i - x_i.theta)^2 from the normal equations"""
    Xw = X * w[:, None]
    return np.linalg.solve(X.T @ Xw, Xw.T @ y)


def _disc(theta, prev):
    with np.errstate(invalid="ignore", divide="ignore"):             # (0 / 0 is a NaN, as in the reference: no stop)
        return float(np.linalg.norm(theta - prev) / np.linalg.norm(prev))


def rrm_linear_regression(X, y, eps, maxiter=100, tol=1e-3, steps=None):
    X = np.asarray(X, np.float64)
    y = np.asarray(y, np.float64)
    n = X.shape[0]
    w = np.ones(n) / n                                               # rrm.py:56
    theta = wls(X, y, w)
    losses = (y - X @ theta) ** 2
    outer, trace = 0, []
    for _ in range(maxiter):
        outer += 1
        w = rrm_ref.update_weights(losses, eps)[0]
        if steps is not None:
            steps.append((losses.copy(), w.copy()))
        prev = theta
        theta = wls(X, y, w)
        losses = (y - X @ theta) ** 2
        trace.append(_disc(theta, prev))
        if trace[-1] <= tol:
            break
    return theta, w, outer, np.array(trace)


def huber_alpha(c):
    """c^2 (1 - F1(c^2)) + F3(c^2): F1(c^2) = erf(c / sqrt 2), F3(c^2) = F1(c^2) - sqrt(2 / pi) c exp(-c^2 / 2)"""
    f1 = math.erf(c / math.sqrt(2.0))
    f3 = f1 - math.sqrt(2.0 / math.pi) * c * math.exp(-0.5 * c * c)
    return c * c * (1.0 - f1) + f3


def clip(r, cs):
    return np.where(np.abs(r) <= cs, r, np.copysign(cs, r))


def huber_linear_regression(X, y, c=0.7317, sigma0=1.0, maxiter=1000):
    from scipy.linalg import cho_factor, cho_solve
    X = np.asarray(X, np.float64)
    y = np.asarray(y, np.float64)
    n = X.shape[0]
    tna = 2.0 * n * huber_alpha(c)
    fac = cho_factor(X.T @ X)                                        # once: X never changes
    theta0 = cho_solve(fac, X.T @ y)
    sigma, it, trace = float(sigma0), 0, []
    theta = theta0
    while it < maxiter:
        it += 1
        r = y - X @ theta0
        p = clip(r, c * sigma0)
        sigma = math.sqrt(float(np.sum(p * p)) / tna)
        if not (sigma > 0.0 and math.isfinite(sigma)):
            raise FloatingPointError("huber: the scale is not positive and finite")
        theta = theta0 + cho_solve(fac, X.T @ clip(r, c * sigma))
        trace.append(_disc(theta, theta0))
        if not trace[-1] > 1e-6:
            break
        sigma0, theta0 = sigma, theta
    return theta, sigma, it, np.array(trace)


def rrm_margin(trace, tol=1e-3):
    """the smallest |discrepancy - tol| over the stop decisions"""
    return float(np.min(np.abs(trace - tol))) if len(trace) else math.inf


def huber_margin(trace):
    """the smallest |discrepancy / 1e-6 - 1| over the stop decisions"""
    return float(np.min(np.abs(trace / 1e-6 - 1.0))) if len(trace) else math.inf
