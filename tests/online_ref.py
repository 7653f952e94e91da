"""Float64 numpy restatement of rlvi_amd/csrc/online_sgd.hip (test infrastructure; imports nothing of the product).

    sgd_order(n, seed=SEED)                                   scikit-learn's shuffle of one partial_fit call
    update_weights_rlvi(losses, tol, maxiter)  -> (w, iters)  online-learning/main.py:45-58
    update_weights_rrm(losses, eps)            -> (w, had_root)   main.py:61-81 as the exact root (rrm_ref.py: bisection)
    sgd_pass(X, y, sw, order, state, alpha, tree, counters)   one pass of _plain_sgd with the reference's settings
    step(...)                                                 one mini-batch: residuals -> weights -> pass -> counts
    stream(...)                                               T consecutive mini-batches for S methods

The pass is scikit-learn's `_plain_sgd` for SGDClassifier(loss='log_loss', random_state=1): L2 penalty, learning rate
'optimal', an intercept, one epoch, shuffled, no averaging, class weights 1.  State = (coef [d], intercept, t), t a double
that starts at 1.0 and grows by one per sample.  `tree`: the dot product of a row summed as the kernel's wave sums it
(lane l holds columns l and l + 64, then a butterfly over 64 lanes) instead of left to right; the distance between the
two is the `noise` the GPU tests scale their coefficient bar by.  With d <= 3 the tree is the sequential sum and that
distance is 0 whatever the recurrence does to a rounding; tree="ulp" (every dot product one unit in the last place up)
is the second run there.  `counters` (a dict, optional) counts how often each
branch of the pass is taken: tail (p <= -37), zero_update, reset (the wscale fold) and clip.

The gradient of the log loss is scikit-learn 1.7.2's (CyHalfBinomialLoss.cy_gradient, labels 0 / 1): with e = exp(-p),
((1 - y) - y e) / (1 + e) for p > -37 and exp(p) - y below.  (Up to scikit-learn 1.5 the SGD module had a loss class of
its own, with labels -1 / 1 and two tails at |p y| > 18; the two differ by exp(-18) there, and by a rounding elsewhere.)
"""
import numpy as np

import rrm_ref

SEED = 2135392491            # the second draw of RandomState(1): randint(1, 2^31 - 1), then randint(2^31 - 1)
METHODS = {"SGD": 0, "RLVI": 1, "RRM": 2, "GIVEN": 3}
COUNTERS = ("tail", "zero_update", "reset", "clip")
LOG2 = 0.6931471805599453
MAX_DLOSS = 1e12


def sgd_order(n, seed=SEED):
    """Fisher-Yates on the identity, j = i + r() % (n - i), r a 32-bit xorshift (13, 17, 5) taken modulo 2^31."""
    idx = np.arange(n, dtype=np.int32)
    s = seed & 0xFFFFFFFF
    if s == 0:
        s = 1
    for i in range(n - 1):
        s ^= (s << 13) & 0xFFFFFFFF
        s ^= s >> 17
        s ^= (s << 5) & 0xFFFFFFFF
        j = i + (s % 2147483648) % (n - i)
        idx[i], idx[j] = idx[j], idx[i]
    return idx


def update_weights_rlvi(losses, tol=1e-3, maxiter=100):
    e = np.exp(-np.asarray(losses, np.float64))
    w = 0.5 * np.ones_like(e)
    new, it = w, 0
    for _ in range(maxiter):
        avg = np.mean(w)
        ratio = avg / (1 - avg)
        t = ratio * e
        new = t / (1 + t)
        it += 1
        if np.linalg.norm(new - w) < tol:
            break
        w = new
    return new / (np.max(new) * len(new)), it


def update_weights_rrm(losses, eps):
    w, _, had_root = rrm_ref.update_weights(losses, eps)
    return w, had_root


def tree_dot(a, b):
    """sum a b as a wave of 64 lanes sums it: lane l takes columns l and l + 64 (a product, then a fused multiply-add
    is restated as two roundings), then the xor butterfly 1, 2, 4, 8, 16, 32"""
    d = a.shape[0]
    v = np.zeros(64)
    lo = min(d, 64)
    v[:lo] = a[:lo] * b[:lo]
    if d > 64:
        v[:d - 64] += a[64:] * b[64:]
    for s in (1, 2, 4, 8, 16, 32):
        v = v + v[np.arange(64) ^ s]
    return float(v[0])


def seq_dot(a, b):
    acc = 0.0
    for u, v in zip(a.tolist(), b.tolist()):
        acc += u * v
    return acc


def ulp_dot(a, b):
    """the sequential sum moved up by one unit in the last place: what stands in for another order of summation where
    there is none (up to three columns the wave's tree IS the sequential sum)"""
    return float(np.nextafter(seq_dot(a, b), np.inf))


def _dot_of(tree):
    return ulp_dot if tree == "ulp" else (tree_dot if tree else seq_dot)


def constants(alpha):
    typw = np.sqrt(1.0 / np.sqrt(alpha))
    e = np.exp(typw)
    dl = -e / (1.0 + e)                             # the gradient at y = 1, p = -typw
    eta0 = typw / max(1.0, dl)                      # (dl < 0: eta0 = typw)
    return 1.0 / (eta0 * alpha)


def sgd_pass(X, y, sw, order, state, alpha=1e-4, tree=False, counters=None):
    """One pass over the rows of X in `order`; returns the new state (coef, intercept, t)."""
    coef, intercept, t = state
    d = X.shape[1]
    w = np.array(coef, np.float64).reshape(d).copy()
    intercept, t = float(intercept), float(t)
    dot = _dot_of(tree)
    c = counters if counters is not None else {}
    optimal_init = constants(alpha)
    wscale = 1.0
    y01 = np.where(np.asarray(y) == 1, 1.0, 0.0)
    for i in order:
        x = X[i]
        p = wscale * dot(w, x) + intercept
        eta = 1.0 / (alpha * (optimal_init + t - 1.0))
        yi = y01[i]
        with np.errstate(over="ignore"):
            if p > -37.0:
                e = np.exp(-p)
                g = ((1.0 - yi) - yi * e) / (1.0 + e)
            else:
                g = np.exp(p) - yi
                c["tail"] = c.get("tail", 0) + 1
        if g < -MAX_DLOSS or g > MAX_DLOSS:
            g = -MAX_DLOSS if g < 0 else MAX_DLOSS
            c["clip"] = c.get("clip", 0) + 1
        update = -eta * g
        update *= 1.0 * sw[i]
        wscale *= max(0.0, 1.0 - eta * alpha)
        if wscale < 1e-9:
            w *= wscale
            wscale = 1.0
            c["reset"] = c.get("reset", 0) + 1
        if update != 0.0:
            w += x * (update / wscale)
            intercept += update
        else:
            c["zero_update"] = c.get("zero_update", 0) + 1
        t += 1.0
    return w * wscale, intercept, t


def residuals(X, coef, intercept, tree=False):
    dot = _dot_of(tree)
    p = np.array([dot(coef, x) for x in X]) + intercept
    with np.errstate(over="ignore"):
        return np.where(p >= 0.0, np.log1p(np.exp(-p)), -p + np.log1p(np.exp(p)))


def counts(Xt, yt, coef, intercept, tree=False):
    """(tp, tn, fp, fn) of main.py:320-331 with the prediction z > 0, and the decision values"""
    dot = _dot_of(tree)
    z = np.array([dot(coef, x) for x in Xt]) + intercept if len(Xt) else np.zeros(0)
    pred = z > 0.0
    yt = np.asarray(yt)
    c = np.array([np.count_nonzero(pred & (yt == 1)), np.count_nonzero(~pred & (yt == 0)),
                  np.count_nonzero(pred & (yt == 0)), np.count_nonzero(~pred & (yt == 1))], np.int32)
    return c, z


def step(X, y, method, state, first, eps=0.3, sample_weight=None, Xt=None, yt=None, order=None, alpha=1e-4,
         tol=1e-3, maxiter=100, tree=False, counters=None):
    """One mini-batch -> dict(state, sample_weight, counts, decision, iters, flag).  method: 0 unit weights, 1 RLVI,
    2 RRM with eps, 3 the weights given.  flag 1: a coefficient or the intercept is not finite."""
    X = np.asarray(X, np.float64)
    n, d = X.shape
    coef, intercept, t = state
    iters = 0
    if method in (1, 2):
        res = np.full(n, LOG2) if first else residuals(X, np.asarray(coef, np.float64), intercept, tree)
        if method == 1:
            sw, iters = update_weights_rlvi(res, tol, maxiter)
        else:
            sw, _ = update_weights_rrm(res, eps)
    elif method == 0:
        sw = np.ones(n)
    else:
        sw = np.asarray(sample_weight, np.float64)
    if order is None:
        order = np.arange(n)
    new = sgd_pass(X, y, sw, order, state, alpha, tree, counters)
    flag = 0 if np.isfinite(new[0]).all() and np.isfinite(new[1]) else 1
    if Xt is None:
        Xt, yt = np.zeros((0, d)), np.zeros(0)
    cnt, z = counts(np.asarray(Xt, np.float64), yt, new[0], new[1], tree)
    return dict(state=new, sample_weight=sw, counts=cnt, decision=z, iters=iters, flag=flag)


def pack_state(state):
    coef, intercept, t = state
    return np.concatenate([np.asarray(coef, np.float64).ravel(), [intercept, t]])


def stream(X, y, Xt, yt, rows, methods, eps=0.3, given=None, alpha=1e-4, tol=1e-3, maxiter=100, tree=False,
           counters=None, shuffle=True):
    """T mini-batches (X [T, n, d] padded, rows [T, 2] = (n_t, m_t)) for each of `methods` -> dict of state_hist
    [S, T, d + 2], counts [S, T, 4], weights [S, T, n] (0 beyond n_t), iters [S, T], flags [S, T]."""
    T, n, d = X.shape
    S = len(methods)
    out = dict(state_hist=np.zeros((S, T, d + 2)), counts=np.zeros((S, T, 4), np.int32), weights=np.zeros((S, T, n)),
               iters=np.zeros((S, T), np.int32), flags=np.zeros((S, T), np.int32))
    for s, m in enumerate(methods):
        state = (np.zeros(d), 0.0, 1.0)
        for k in range(T):
            nt, mt = int(rows[k, 0]), int(rows[k, 1])
            r = step(X[k, :nt], y[k, :nt], m, state, k == 0, eps,
                     None if given is None else given[s, k, :nt], Xt[k, :mt], yt[k, :mt],
                     sgd_order(nt) if shuffle else None, alpha, tol, maxiter, tree, counters)
            state = r["state"]
            out["state_hist"][s, k] = pack_state(state)
            out["counts"][s, k] = r["counts"]
            out["weights"][s, k, :nt] = r["sample_weight"]
            out["iters"][s, k] = r["iters"]
            out["flags"][s, k] = r["flag"]
    return out
