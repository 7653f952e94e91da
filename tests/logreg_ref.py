"""Float64 numpy restatement of rlvi_amd/csrc/logreg.hip (test infrastructure; imports nothing of the product).

    fit(X, y, w, C=100.0)                       -> (theta, losses, newton_steps)     one M-step, utils.py:61-73
    logistic_regression(X, y, maxiter, tol)     -> (theta, weights, outer, trace)    rlvi.py:92-108

The same algorithm, statement for statement, as the kernel: damped Newton from v = 0 on
    f(v) = 1/2 v.v + C sum_i (w_i / max w) log(1 + exp(-s_i z_i)),   v = (coef, bias), z = X coef + bias, s = 2y - 1,
with Armijo halving, the stop test ||g|| <= 1e-12 ||g(0)||, the rounding floor (where f can no longer tell -- the
model's decrease g.delta is below 1e-10 |f| and the full step changes f by rounding only -- the full step is taken on
the gradient's word, and the fit ends once the gradient stops shrinking by half per step), z carried along the steps
and computed afresh at the end; the E-step is rlvi.py:8-20.  Only the order of the sums differs.

objective / gradient evaluate f and its gradient for ANY v in extended precision (np.longdouble): the yardstick of
the strong-convexity bound ||v_a - v_b|| <= ||grad f(v_a)|| + ||grad f(v_b)||, which holds for every pair of points
because the Hessian of f is >= I.
"""
import numpy as np

NEWTON_CAP = 50
HALVINGS = 40
GTOL2 = 1e-24
ARMIJO = 1e-4
FLOOR = 1e-10
NOISE = 1e-12


def _softplus_neg(m):
    """log(1 + exp(-m)), overflow-safe."""
    return np.log1p(np.exp(-np.abs(m))) + np.maximum(-m, 0.0)


def design(X):
    """Z = [X | 1]: v = (coef, bias)."""
    X = np.asarray(X, np.float64)
    return np.hstack([X, np.ones((X.shape[0], 1))])


def to_v(theta):
    """theta = (intercept, coef ...) (utils.py:69) -> v = (coef ..., bias)."""
    theta = np.asarray(theta)
    return np.concatenate([theta[1:], theta[:1]])


def to_theta(v):
    return np.concatenate([v[-1:], v[:-1]])


def gradient(X, y, w, v, C=100.0):
    """grad f(v) in extended precision, returned as float64."""
    L = np.longdouble
    Z = design(X).astype(L)
    s = 2 * np.asarray(y, L) - 1
    w = np.asarray(w, L)
    cw = L(C) * (w / w.max())
    v = np.asarray(v, L)
    m = s * (Z @ v)
    em = np.exp(-np.abs(m))
    p = np.where(m >= 0, em / (1 + em), 1 / (1 + em))            # sigma(-m)
    return np.asarray(v - Z.T @ (cw * s * p), np.float64)


def objective(X, y, w, v, C=100.0):
    L = np.longdouble
    Z = design(X).astype(L)
    s = 2 * np.asarray(y, L) - 1
    w = np.asarray(w, L)
    v = np.asarray(v, L)
    return float(0.5 * v @ v + np.sum(L(C) * (w / w.max()) * _softplus_neg(s * (Z @ v))))


def fit(X, y, w, C=100.0):
    """One weighted fit from v = 0.  Returns (theta = (intercept, coef), losses = log(1 + exp(z)), Newton steps)."""
    Z = design(X)
    n, D = Z.shape
    s = 2.0 * np.asarray(y, np.float64) - 1.0
    w = np.asarray(w, np.float64)
    cw = C * (w / np.max(w))
    v = np.zeros(D)
    z = np.zeros(n)
    g0 = 0.0
    gg_noise = -1.0
    steps = 0
    for step in range(NEWTON_CAP + 1):
        m = s * z
        em = np.exp(-np.abs(m))
        r = 1.0 / (1.0 + em)
        p = np.where(m >= 0, em * r, r)
        q1 = np.where(m >= 0, r, em * r)
        f = 0.5 * (v @ v) + np.sum(cw * _softplus_neg(m))
        if not np.isfinite(f):
            raise FloatingPointError("logreg_ref.fit: objective not finite")
        h = cw * p * q1
        g = v - Z.T @ (cw * s * p)
        gg = g @ g
        if step == 0:
            g0 = gg
        if gg <= GTOL2 * g0:
            break
        if gg_noise >= 0.0 and not gg <= 0.25 * gg_noise:
            break
        gg_noise = -1.0
        if step >= NEWTON_CAP:
            raise FloatingPointError("logreg_ref.fit: Newton cap")
        H = np.eye(D) + Z.T @ (h[:, None] * Z)
        delta = np.linalg.solve(H, g)
        steps += 1
        gd = g @ delta
        zd = Z @ delta
        t, accepted, at_floor = 1.0, False, False
        for k in range(HALVINGS):
            vt = v - t * delta
            ft = 0.5 * (vt @ vt) + np.sum(cw * _softplus_neg(s * (z - t * zd)))
            if ft <= f - ARMIJO * t * gd:
                accepted = True
                break
            if k == 0 and gd <= FLOOR * abs(f):
                at_floor = True
                if ft <= f + NOISE * abs(f):
                    accepted, gg_noise = True, gg
                break
            t *= 0.5
        if not accepted:
            if not at_floor:
                raise FloatingPointError("logreg_ref.fit: no acceptable step")
            break
        v = v - t * delta
        z = z - t * zd
    z = Z @ v
    return to_theta(v), np.logaddexp(0.0, z), steps


def update_weights(losses, tol=1e-3, maxiter=100):
    """rlvi.py:8-20."""
    weights = 0.95 * np.ones_like(losses)
    new = np.copy(weights)
    for _ in range(maxiter):
        eps = 1 - np.mean(weights)
        ratio = eps / (1 - eps)
        new = np.exp(-losses) / (ratio + np.exp(-losses))
        error = np.linalg.norm(new - weights)
        weights = np.copy(new)
        if error < tol:
            break
    return new


def logistic_regression(X, y, maxiter=100, tol=1e-2, C=100.0):
    """rlvi.py:92-108 on fit() above.  Returns (theta, final weights, outer iterations, discrepancy trace)."""
    X = np.asarray(X, np.float64)
    w = np.ones(X.shape[0])
    theta, losses, _ = fit(X, y, w, C)
    outer, trace = 0, []
    for _ in range(maxiter):
        outer += 1
        w = update_weights(losses)
        prev = theta.copy()
        theta, losses, _ = fit(X, y, w, C)
        disc = np.linalg.norm(theta - prev) / np.linalg.norm(prev)
        trace.append(disc)
        if disc <= tol:
            break
    return theta, w, outer, np.array(trace)
