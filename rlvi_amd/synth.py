"""Seeded synthetic inputs for the RLVI hot path (numpy only).

Shared by bench.py, the parity tests and oracle/make_golden.py so that a
fixture can carry a recipe name + seed instead of a large array.  Recipes follow
SURVEY.md section 8(d).
"""
import numpy as np

BENCH_SEED = 20240131


def mstep_inputs(B, C, N=None, seed=BENCH_SEED, clean_frac=0.55, shift=12.0,
                 zero_frac=0.0):
    """logits ~ 3*N(0,1); `clean_frac` of the rows get +shift on the label logit
    (bimodal NLL); idx = first B of a permutation of N; lagged pi ~ U(0,1)."""
    rng = np.random.default_rng(seed)
    N = B if N is None else N
    logits = (3.0 * rng.standard_normal((B, C))).astype(np.float32)
    labels = rng.integers(0, C, B).astype(np.int64)
    clean = rng.random(B) < clean_frac
    logits[np.nonzero(clean)[0], labels[clean]] += np.float32(shift)
    idx = rng.permutation(N)[:B].astype(np.int64)
    weights = rng.random(N).astype(np.float32)
    if zero_frac > 0:
        weights[rng.random(N) < zero_frac] = 0.0
    return dict(logits=logits, labels=labels, idx=idx, weights=weights,
                residuals=np.zeros(N, np.float32))


def residual_vector(kind, N, seed=0):
    """Per-sample NLL vectors that exercise the E-step (golden set G1)."""
    rng = np.random.default_rng(seed)
    if kind == "equal":
        r = np.full(N, 0.7, np.float32)
    elif kind == "exp":
        r = rng.exponential(1.0, N).astype(np.float32)
    elif kind == "bimodal":
        r = rng.exponential(0.05, N).astype(np.float32)
        bad = rng.random(N) >= 0.55
        r[bad] += (12.0 + rng.standard_normal(int(bad.sum()))).astype(np.float32)
    elif kind == "heavy":
        r = rng.exponential(1.0, N).astype(np.float32)
        r[::7] += np.float32(95.0)              # exp(-l) underflows to 0 in fp32
    elif kind == "zeros10":
        r = (0.3 + rng.exponential(1.0, N)).astype(np.float32)
        r[rng.random(N) < 0.10] = 0.0           # Food-101 unvisited-slot quirk
    elif kind == "narrow":
        # every loss within 0.01 of the others (a converged or near-clean epoch): the trajectory crawls,
        # the stop tests are long sums of nearly equal steps
        r = (2.0 + 0.01 * rng.random(N)).astype(np.float32)
    elif kind == "ce":
        d = mstep_inputs(N, 10, seed=seed)
        z = d["logits"].astype(np.float64)
        m = z.max(1, keepdims=True)
        lse = m[:, 0] + np.log(np.exp(z - m).sum(1))
        r = (lse - z[np.arange(N), d["labels"]]).astype(np.float32)
    else:
        raise ValueError(kind)
    return r


def estep_trace64(residuals, weights, tol=1e-3, maxiter=40, stop=True):
    """update_sample_weights (train_rlvi.py:26-38) restated in float64 on the given inputs.

    Returns (count, err[count], pi): pi is divided by its maximum as :38 does.  stop=False runs all
    `maxiter` iterations and returns every error (the bisection of near_tie needs the tests past the stop)."""
    r = np.asarray(residuals).astype(np.float64)          # (fp32 inputs, or an fp64 NLL of fp32 logits)
    w = np.asarray(weights).astype(np.float64)
    e = np.exp(-(r - r.min()))
    avg = 0.95
    errs = []
    for _ in range(maxiter):
        ratio = avg / (1.0 - avg)
        nw = ratio * e / (1.0 + ratio * e)
        errs.append(float(np.sqrt(np.sum((nw - w) ** 2))))
        w = nw
        avg = float(w.mean())
        if stop and errs[-1] < tol:
            break
    return len(errs), np.array(errs), w / w.max()


NEAR_TIE_KINDS = ("bimodal", "exp", "zeros10", "ce", "heavy", "narrow")


def _first_pi(r):
    """pi after the first iteration (avg_weight = 0.95), in fp64."""
    e = np.exp(-(r.astype(np.float64) - float(r.min())))
    return 19.0 * e / (1.0 + 19.0 * e)


def _tie_direction(N, seed):
    """Unit vector of +-1/sqrt(N) along which the caller's pi is moved for a tie at test 0."""
    rng = np.random.default_rng(seed + 7919)
    return np.where(rng.random(N) < 0.5, -1.0, 1.0) / np.sqrt(N)


def near_tie_vectors(kind, N, seed, k, knob):
    """(residuals fp32, caller weights fp32) of a near-tie recipe.  k >= 1: residuals = fp32(base * knob) and
    the caller's pi all ones; k = 0: the base residuals and the caller's pi = fp32(pi_1 + knob * v), pi_1 the
    first iteration's pi and v a fixed +-1/sqrt(N) direction, so that test 0 measures |knob|."""
    base = residual_vector(kind, N, seed)
    if k >= 1:
        return (base.astype(np.float64) * knob).astype(np.float32), np.ones(N, np.float32)
    w = _first_pi(base) + knob * _tie_direction(N, seed)
    return base, np.clip(w, 0.0, 1.0).astype(np.float32)


def _bisect(f, lo, hi, target, steps=60):
    """x in [lo, hi] with f(x) ~ target, f monotone between the ends (either direction)."""
    flo = f(lo) - target
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        fm = f(mid) - target
        if fm == 0.0:
            return mid
        if (fm < 0) == (flo < 0):
            lo, flo = mid, fm
        else:
            hi = mid
    return lo if abs(flo) <= abs(f(hi) - target) else hi


def near_tie(kind, N, seed, tol, maxiter, k, margin, side, bracket=None):
    """Inputs whose stop test k (0-based: the error of iteration k+1) sits at tol * (1 + side * margin) in
    float64, every earlier test above tol: the decisions of the E-step placed at a chosen distance from tol.

    The knob is bisected on the final fp32 vectors (near_tie_vectors).  k = 0: the caller's pi (test 0 is
    taken against it); k >= 1: a scale on the base residuals (it sets the spread, and with it how fast the
    trajectory moves).  Returns dict(residuals, weights, knob, margins, count, bracket): `margins` are the
    reached (err64_j - tol) / tol of every test up to the fp64 stop.  `bracket` (returned, and accepted back
    for the other margins of the same k) is the knob interval in which test k crosses tol."""
    target = tol * (1.0 + side * margin)
    if k == 0:
        def f(a):
            r, w = near_tie_vectors(kind, N, seed, 0, a)
            return estep_trace64(r, w, tol, 1, stop=False)[1][0]
        bracket = bracket or (0.0, 4.0 * tol)
        knob = _bisect(f, bracket[0], bracket[1], target)
    else:
        def trace(s):
            r, w = near_tie_vectors(kind, N, seed, k, s)
            return estep_trace64(r, w, tol, k + 1, stop=False)[1]
        if bracket is None:
            # a log grid of scales: the first pair of neighbours between which test k crosses tol while
            # every earlier test stays above it at both ends
            grid = np.exp(np.linspace(np.log(1e-4), np.log(1e3), 281))
            prev = None
            for s in grid:
                t = trace(s)
                ok = len(t) == k + 1 and np.all(t[:k] > tol)
                cur = (s, t[k] - tol) if ok else None
                if prev is not None and cur is not None and (prev[1] < 0) != (cur[1] < 0):
                    bracket = (prev[0], cur[0])
                    break
                prev = cur
            if bracket is None:
                raise ValueError(f"no scale puts stop test {k} at tol for {kind} N={N} tol={tol}")
        # the bracket holds tol; widen it (geometrically, about its middle) until it holds the target too
        f = lambda s: trace(s)[k] - target   # noqa: E731
        lo, hi = bracket
        for _ in range(40):
            if (f(lo) < 0) != (f(hi) < 0):
                break
            c = np.sqrt(lo * hi)
            lo, hi = c * (lo / c) ** 1.5, c * (hi / c) ** 1.5
        knob = _bisect(lambda s: trace(s)[k], lo, hi, target)
    r, w = near_tie_vectors(kind, N, seed, k, knob)
    cnt, errs, _ = estep_trace64(r, w, tol, maxiter)
    return dict(residuals=r, weights=w, knob=float(knob), margins=(errs - tol) / tol, count=cnt,
                bracket=bracket)


def linreg_data(size=1000, d=20, eps=0.3, nu=2.5, seed=0):
    """cfg1 inputs: the recipe of standard-learning/main.py:69-85 at size x d."""
    rng = np.random.default_rng(seed)
    X = -5 + 10 * rng.random(size=(size, d))
    n2 = rng.binomial(n=size, p=eps)
    n1 = size - n2
    theta = np.ones(d)
    y1 = X[:n1] @ theta + 0.25 * rng.normal(size=n1)
    u = rng.chisquare(df=nu, size=n2) / nu
    v = rng.normal(size=n2)
    y2 = X[n1:] @ theta + v / np.sqrt(u)
    return X, np.concatenate([y1, y2])


def logistic_data(B=256, d=60, seed=0):
    """cfg2 stand-in (the HAR .mat is not shipped): X ~ N(0,1), w ~ N(0,1)/sqrt(d)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((B, d))
    w = rng.standard_normal(d) / np.sqrt(d)
    b = 0.1
    return X, w, b


def heavy_tail_cloud(size=200, eps=0.2, nu=1.5, seed=0, corr=0.8):
    """2-D sample for the mean / pca / covariance estimators: a correlated Gaussian cloud with an
    eps-fraction of multivariate-t outliers (the recipe of standard-learning/main.py:44-67,
    :124-167 with a fixed seed)."""
    rng = np.random.default_rng(seed)
    n2 = rng.binomial(n=size, p=eps)
    n1 = size - n2
    root = np.linalg.cholesky(np.array([[1.0, corr], [corr, 1.0]]))
    s1 = root @ rng.normal(size=(2, n1))
    u = rng.chisquare(df=nu, size=n2) / nu
    s2 = (root @ rng.normal(size=(2, n2))) / np.sqrt(u[None, :])
    return np.hstack([s1, s2]).T


def jocor_loop_inputs(seed=1212, N=256, D=16, C=10, noise=0.3):
    """Inputs of the three-epoch JoCoR run of golden set G12: features X [N, D] fp32, labels [N] int64 of a
    linear teacher with `noise` of them replaced at random."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)).astype(np.float32)
    W = rng.standard_normal((D, C))
    labels = np.argmax(X.astype(np.float64) @ W, axis=1).astype(np.int64)
    flip = rng.random(N) < noise
    labels[flip] = rng.integers(0, C, int(flip.sum()))
    return X, labels


def jocor_rate_schedule(forget_rate, n_epoch, num_gradual, exponent=1.0):
    """rate_schedule of deep-learning/main.py:172-180."""
    rs = np.ones(n_epoch) * forget_rate
    rs[:num_gradual] = np.linspace(0, forget_rate ** exponent, num_gradual)
    return rs


def bare_dense_inputs(B, C, scale, seed):
    """Inputs of golden set G14's dense cases: logits scale * N(0, 1) [B, C] fp32 and uniform labels [B] int64 --
    softmax columns of one narrow mode each, so that many rows sit near BARE's mean + k * std boundary."""
    rng = np.random.default_rng(seed)
    logits = (scale * rng.standard_normal((B, C))).astype(np.float32)
    labels = rng.integers(0, C, B).astype(np.int64)
    return logits, labels
