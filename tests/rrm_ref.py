"""Float64 numpy restatement of the RRM side of rlvi_amd/csrc/moments.hip (test infrastructure; imports nothing of the
product).

    update_weights(losses, eps)                          -> (weights, alpha, had_root)        rrm.py:12-33
    mean(sample, eps, maxiter, tol)                      -> (theta, weights, outer, trace)    rrm.py:36-52
    pca(sample, eps, maxiter, tol, theta_init=None)      -> (theta, weights, outer, trace)    rrm.py:94-107, utils.py:76-89
    covariance(sample, eps, maxiter, tol)                -> (theta, weights, outer, trace)    rrm.py:110-124, utils.py:92-108

The same algorithm as the kernel.  The fits are those of tests/moments_ref.py (two-pass weighted moments, the first
principal component by numpy.linalg.eigh with sklearn's sign rule, a Cholesky factorisation for the Mahalanobis
distances and log det); the mean's losses are ||theta - x||^2 with no variance (rrm.py:39, :46); the first weights are
1 / n.  The weight rule minimises g(alpha) = alpha (log sum_i exp(-l_i / alpha) - log((1 - eps) n)) over alpha =
exp(xi): g is convex and stationary where the entropy of w_i = phi_i / S equals log((1 - eps) n),

    H(xi) = log S + (sum phi_i t_i) / S = log((1 - eps) n),   t_i = (l_i - min l) / alpha,  phi_i = exp(-t_i),  S = sum phi_i

(the shift by min l moves g by a constant and leaves w as it is; S >= 1, so the reference's floor of 1e-16 under every
phi is not needed and is dropped: it moves S by at most n 1e-16 relative).  H increases in xi from log m, m the number
of samples tied at the minimum, to log n: the root is found by bisection on xi in [XI_MIN, XI_MAX] down to one ulp
(the kernel: a bracket grown geometrically, then safeguarded Newton to the same root).  With m >= (1 - eps) n -- or
no sign change down to XI_MIN -- there is no root, the minimiser runs off to alpha -> 0 and the rule returns that
limit: 1 / m on the minima, 0 elsewhere (had_root False, alpha 0).  `trace` holds the discrepancies
||theta - prev|| / ||prev|| of the outer iterations; `steps`, if a list, receives (losses in, weights out, alpha,
had_root) of every E-step.  Only the order of the sums differs from the kernel.
"""
import numpy as np

from moments_ref import _cov_step, _pca_fit, _pca_losses, moments

XI_MIN, XI_MAX = -700.0, 700.0      # alpha = exp(xi) stays a normal number
T_MAX = 800.0                       # exp(-800) is 0: a larger t is cut here, so that phi t is 0 and never 0 inf


def _phi(l0, xi):
    with np.errstate(over="ignore", under="ignore"):
        t = np.minimum(l0 * np.exp(-xi), T_MAX)
        return np.exp(-t), t


def entropy_gap(l0, xi, target):
    """H(xi) - target on the shifted losses l0 = l - min l"""
    phi, t = _phi(l0, xi)
    s = np.sum(phi)
    return np.log(s) + np.sum(phi * t) / s - target


def update_weights(losses, eps):
    """rrm.py:12-33 with the exact entropy root in place of Brent's search on g -> (weights, alpha, had_root)."""
    l = np.asarray(losses, np.float64)
    n = l.shape[0]
    if not (0.0 < eps < 1.0 and (1.0 - eps) * n > 1.0):
        raise ValueError("update_weights needs 0 < eps < 1 and (1 - eps) n > 1")
    l0 = l - np.min(l)
    if not np.isfinite(l0).all():
        raise ValueError("update_weights: a loss is not finite")
    keep = (1.0 - eps) * n
    target = np.log(keep)
    m = int(np.sum(l0 == 0.0))
    lo, hi = XI_MIN, XI_MAX
    if m >= keep or entropy_gap(l0, lo, target) >= 0.0:
        return np.where(l0 == 0.0, 1.0 / m, 0.0), 0.0, False
    while True:
        mid = lo + 0.5 * (hi - lo)
        if mid == lo or mid == hi:
            break
        if entropy_gap(l0, mid, target) < 0.0:
            lo = mid
        else:
            hi = mid
    # of the two ends, the one whose entropy is nearer
    xi = lo if abs(entropy_gap(l0, lo, target)) <= abs(entropy_gap(l0, hi, target)) else hi
    phi, _ = _phi(l0, xi)
    return phi / np.sum(phi), float(np.exp(xi)), True


def entropy(w):
    """-sum w log w over the positive weights"""
    p = w[w > 0.0]
    return float(-np.sum(p * np.log(p)))


def _mean_step(x, w):
    _, theta, _ = moments(x, w)
    return theta, np.sum((theta - x) ** 2, axis=1)


def _disc(theta, prev):
    return np.linalg.norm(theta - prev) / np.linalg.norm(prev)      # (Frobenius for a matrix: numpy's default)


def _loop(x, eps, maxiter, tol, step, first, steps):
    n = x.shape[0]
    w = np.ones(n) / n                                              # rrm.py:37 / :95 / :111
    theta, losses = first(w)
    outer, trace = 0, []
    for _ in range(maxiter):
        outer += 1
        w, alpha, had_root = update_weights(losses, eps)
        if steps is not None:
            steps.append((losses.copy(), w.copy(), alpha, had_root))
        prev = theta.copy()
        theta, losses = step(w)
        trace.append(_disc(theta, prev))
        if trace[-1] <= tol:
            break
    return theta, w, outer, np.array(trace)


def mean(sample, eps, maxiter=100, tol=1e-3, steps=None):
    x = np.asarray(sample, np.float64)
    return _loop(x, eps, maxiter, tol, lambda w: _mean_step(x, w), lambda w: _mean_step(x, w), steps)


def pca(sample, eps, maxiter=100, tol=1e-2, theta_init=None, steps=None):
    x = np.asarray(sample, np.float64)

    def step(w):
        theta = _pca_fit(x, w)
        return theta, _pca_losses(x, theta)

    def first(w):
        if theta_init is None:
            return step(w)
        theta = np.array(theta_init, np.float64)
        return theta, _pca_losses(x, theta)
    return _loop(x, eps, maxiter, tol, step, first, steps)


def covariance(sample, eps, maxiter=100, tol=1e-2, steps=None):
    x = np.asarray(sample, np.float64)
    return _loop(x, eps, maxiter, tol, lambda w: _cov_step(x, w), lambda w: _cov_step(x, w), steps)
