"""Float64 numpy restatement of rlvi_amd/csrc/moments.hip (test infrastructure; imports nothing of the product).

    mean(sample, maxiter, tol)                      -> (theta, weights, outer, trace)     rlvi.py:46-65
    pca(sample, maxiter, tol, theta_init=None)      -> (theta, weights, outer, trace)     rlvi.py:111-125, utils.py:76-89
    covariance(sample, eps, maxiter, tol)           -> (theta, weights, outer, trace)     rlvi.py:128-144, utils.py:92-108
    update_weights_constrained(losses, n_eff, ...)  -> (weights, active)                  rlvi.py:23-43

The same algorithm as the kernel: weighted moments in two passes (the sums, then the second moment about the mean just
found), the first principal component as the eigenvector of the largest eigenvalue of the d x d scatter matrix of the
centred rows w x (numpy.linalg.eigh here, Jacobi sweeps there) with sklearn's sign rule, a Cholesky factorisation
for the Mahalanobis distances and log det, and the constrained E-step's shift as the EXACT root of
    sum_i 1 / (1 + c exp(l_i - s)) = n_eff,   c = (n - n_eff) / n_eff,
found by bisection down to one ulp (the kernel: safeguarded Newton to the same root).  `trace` holds the
discrepancies ||theta - prev|| / ||prev|| of the outer iterations.  Only the order of the sums differs.
"""
import numpy as np


def update_weights(losses, tol=1e-3, maxiter=100):
    """rlvi.py:8-20, statement for statement."""
    with np.errstate(under="ignore"):
        e = np.exp(-losses)
    weights = 0.95 * np.ones_like(losses)
    new_weights = np.copy(weights)
    for _ in range(maxiter):
        eps = 1 - np.mean(weights)
        ratio = eps / (1 - eps)
        new_weights = e / (ratio + e)
        error = np.linalg.norm(new_weights - weights)
        weights = np.copy(new_weights)
        if error < tol:
            break
    return new_weights


def _constrained(losses, c, s):
    with np.errstate(over="ignore", under="ignore"):
        return 1.0 / (1.0 + c * np.exp(losses - s))


def kkt_root(losses, n_eff):
    """The shift s at which the constrained weights sum to n_eff: bisection on [min l, max l] to one ulp."""
    n = len(losses)
    c = (n - n_eff) / n_eff
    lo, hi = float(np.min(losses)), float(np.max(losses))
    while True:
        mid = lo + 0.5 * (hi - lo)
        if mid == lo or mid == hi:
            break
        if np.sum(_constrained(losses, c, mid)) < n_eff:
            lo = mid
        else:
            hi = mid
    # of the two ends, the one whose sum is nearer
    glo, ghi = np.sum(_constrained(losses, c, lo)), np.sum(_constrained(losses, c, hi))
    return lo if abs(glo - n_eff) <= abs(ghi - n_eff) else hi


def update_weights_constrained(losses, n_eff, tol=1e-3, maxiter=100):
    """rlvi.py:23-43 with the exact KKT root in place of Brent's search on the square -> (weights, active)."""
    losses = np.asarray(losses, np.float64)
    n = len(losses)
    w = update_weights(losses, tol=tol, maxiter=maxiter)
    if np.sum(w) < n_eff:
        return _constrained(losses, (n - n_eff) / n_eff, kkt_root(losses, n_eff)), True
    return w, False


def moments(x, a):
    """sum a, the mean sum a x / sum a and the second moment sum a (x - m)(x - m)^T about it: two passes."""
    s0 = np.sum(a)
    m = a @ x / s0
    c = x - m
    return s0, m, c.T @ (a[:, None] * c)


def _mean_step(x, w):
    s0, theta, _ = moments(x, w)
    r = np.sum((theta - x) ** 2, axis=1)
    sigma2 = w @ r / s0
    if not (sigma2 > 0 and np.isfinite(sigma2)):
        raise ValueError("mean: the weighted variance is not positive")
    return theta, 0.5 * r / sigma2


def _pca_fit(x, w):
    n, d = x.shape
    if d == 1:
        return np.ones(1)
    z = w[:, None] * x
    zc = z - z.sum(0) / n
    _, vecs = np.linalg.eigh(zc.T @ zc)
    theta = vecs[:, -1] / np.linalg.norm(vecs[:, -1])
    if theta[np.argmax(np.abs(theta))] < 0:          # sklearn's svd_flip(u_based_decision=False)
        theta = -theta
    return theta


def _pca_losses(x, theta):
    return np.sum(x ** 2, axis=1) - (x @ theta) ** 2


def _cov_step(x, w):
    s0, mu, s2 = moments(x, w)
    cov = s2 / s0
    try:
        chol = np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        raise ValueError("Singular covariance matrix")
    z = np.linalg.solve(chol, (x - mu).T)
    r = np.sum(z * z, axis=0)
    logdet = 2.0 * np.sum(np.log(np.diag(chol)))
    return cov, 0.5 * (r + logdet + x.shape[1] * np.log(2 * np.pi))


def _disc(theta, prev):
    return np.linalg.norm(theta - prev) / np.linalg.norm(prev)      # (Frobenius for a matrix: numpy's default)


def mean(sample, maxiter=100, tol=1e-3):
    x = np.asarray(sample, np.float64)
    w = np.ones(x.shape[0])
    theta, losses = _mean_step(x, w)
    outer, trace = 0, []
    for _ in range(maxiter):
        outer += 1
        w = update_weights(losses)
        prev = theta.copy()
        theta, losses = _mean_step(x, w)
        trace.append(_disc(theta, prev))
        if trace[-1] <= tol:
            break
    return theta, w, outer, np.array(trace)


def pca(sample, maxiter=100, tol=1e-2, theta_init=None):
    x = np.asarray(sample, np.float64)
    w = np.ones(x.shape[0])
    theta = _pca_fit(x, w) if theta_init is None else np.array(theta_init, np.float64)
    losses = _pca_losses(x, theta)
    outer, trace = 0, []
    for _ in range(maxiter):
        outer += 1
        w = update_weights(losses)
        prev = theta.copy()
        theta = _pca_fit(x, w)
        losses = _pca_losses(x, theta)
        trace.append(_disc(theta, prev))
        if trace[-1] <= tol:
            break
    return theta, w, outer, np.array(trace)


def covariance(sample, eps, maxiter=100, tol=1e-2, steps=None):
    """steps, if a list: receives (losses in, weights out, active) of every E-step."""
    x = np.asarray(sample, np.float64)
    n = x.shape[0]
    n_eff = n * (1 - eps)
    w = np.ones(n)
    theta, losses = _cov_step(x, w)
    outer, trace = 0, []
    for _ in range(maxiter):
        outer += 1
        w, active = update_weights_constrained(losses, n_eff)
        if steps is not None:
            steps.append((losses.copy(), w.copy(), active))
        prev = theta.copy()
        theta, losses = _cov_step(x, w)
        trace.append(_disc(theta, prev))
        if trace[-1] <= tol:
            break
    return theta, w, outer, np.array(trace)
