"""Float64 numpy restatement of rlvi_amd/csrc/robust_logreg.hip (test infrastructure; imports nothing of the product).

    rrm_logistic_regression(X, y, eps, maxiter, tol, C)     -> (theta, weights, outer, trace)     rrm.py:76-91
    margin(trace, tol)                                      -> the smallest |disc / tol - 1| over the stop decisions

logreg_ref.fit (the damped Newton fit, to the minimiser liblinear approximates) and rrm_ref.update_weights (the exact
entropy root of the RRM rule) composed as the kernel composes them: weights 1 / n -- so C w / max w = C --, the first
fit; then `maxiter` times { losses log(1 + exp(z)) of EVERY sample (utils.py:62-64), the rule, the fit with
C w / max w, stop when ||theta - prev|| / ||prev|| <= tol }.  The test comes after each refit; maxiter = 0 returns the
first fit and weights 1 / n; reaching maxiter is silent.  `steps`, if a list, receives (losses in, weights out) of every
rule call.  Only the order of the sums and the solve of the Newton system differ from the kernel.
"""
import math

import numpy as np

import logreg_ref
import rrm_ref


def _disc(theta, prev):
    with np.errstate(invalid="ignore", divide="ignore"):             # (0 / 0 is a NaN, as in the reference: no stop)
        return float(np.linalg.norm(theta - prev) / np.linalg.norm(prev))


def rrm_logistic_regression(X, y, eps, maxiter=100, tol=1e-2, C=100.0, steps=None):
    X = np.asarray(X, np.float64)
    y = np.asarray(y, np.float64)
    n = X.shape[0]
    w = np.ones(n) / n                                               # rrm.py:77
    theta, losses, _ = logreg_ref.fit(X, y, w, C)                    # rrm.py:78
    outer, trace = 0, []
    for _ in range(maxiter):
        outer += 1
        w = rrm_ref.update_weights(losses, eps)[0]                   # rrm.py:81
        if steps is not None:
            steps.append((losses.copy(), w.copy()))
        prev = theta
        theta, losses, _ = logreg_ref.fit(X, y, w, C)                # rrm.py:84
        trace.append(_disc(theta, prev))
        if trace[-1] <= tol:                                         # rrm.py:87-89
            break
    return theta, w, outer, np.array(trace)


def gauss_case(seed, n, d):
    """The Gaussian design of G15's and G20's tools (tools/make_golden_logreg.py: gauss_case) at any shape: entries
    exactly representable in fp16, labels from a logistic model with a tenth flipped.  Returns fp64 arrays."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float16).astype(np.float64)
    beta = rng.standard_normal(d) / np.sqrt(d)
    p = 1 / (1 + np.exp(-(0.3 + 2 * X @ beta)))
    y = (rng.random(n) < p).astype(np.float64)
    flip = rng.choice(n, n // 10, replace=False)
    y[flip] = 1 - y[flip]
    return X, y


def margin(trace, tol=1e-2):
    """the smallest |discrepancy / tol - 1| over the stop decisions"""
    trace = np.asarray(trace, np.float64)
    return float(np.min(np.abs(trace / tol - 1.0))) if len(trace) else math.inf
