"""MI355X mirror of online-learning/main.py (numpy in, numpy out, fp64).

    update_weights_rlvi(losses, tol=1e-3, maxiter=100)    reference main.py:45-58
    update_weights_rrm(residuals, eps)                    reference main.py:61-81
    cross_entropy(log_proba, targets)                     reference main.py:84-85
    residuals(X, coef, intercept)                         reference main.py:295-296 (log-sigmoid)
    rlvi_sample_weight(X, coef, intercept)                the E-step inputs of main.py:291-299
    sgd_order(n, random_state=1)                          the order of one partial_fit pass
    SGDClassifier(loss='log_loss', random_state=1)        the classifier of main.py:16-20
    run_stream(X_train, y_train, X_test, y_test, ...)     the loop of main.py:288-339 in ONE launch

The M-step of the reference is sklearn's SGDClassifier.partial_fit(sample_weight=...): one pass of sequential per-sample
SGD (log loss, L2 penalty, learning rate 'optimal', an intercept, the rows in the order of a seeded shuffle).  That pass
is a deterministic recurrence and is pinned against scikit-learn 1.7.2 (tests/golden/g21_online_sgd.npz):
SGDClassifier below runs it on the device, `partial_fit_weighted` together with the residuals, the sample weights and
the test counts of its mini-batch in ONE launch (rlvi_online_step_f64), and with this class in place of sklearn's the
loop of main.py:288-339 runs as it is written.  run_stream is that whole loop -- every mini-batch, every classifier --
as one launch (rlvi_online_stream_f64).  Dataset I/O, the scaler, the label corruption and the plots are not here.
"""
import numpy as np
import torch

from . import _lib, ops
from .standard import _dev

SGD_SEED_1 = 2135392491       # random_state=1: the second draw of RandomState(1) (randint(1, 2^31 - 1), randint(2^31 - 1))
_ORDERS = {}                  # (device index, n) -> the device copy of sgd_order(n)


def update_weights_rlvi(losses, tol=1e-3, maxiter=100):
    '''Optimize Bernoulli probabilities (reference main.py:45-58).'''
    from .standard import _roundtrip_f64
    return _roundtrip_f64(losses, lambda l: ops.update_weights_f64(l, tol=tol, maxiter=maxiter, online=True)[0])


def update_weights_rrm(residuals, eps):
    '''Optimize sample weights for Robust Risk Minimization (reference main.py:61-81): the rule of rrm.update_weights
    (standard-learning/rrm.py:12-33), normalised to sum 1 as main.py:79-80 does.'''
    from . import rrm
    return rrm.update_weights(residuals, eps)


def cross_entropy(log_proba, targets):
    """reference main.py:84-85: -t*lp - (1-t)*lp, i.e. -log_proba whatever the target."""
    return -targets * log_proba - (1 - targets) * log_proba


def residuals(X, coef, intercept):
    """-log sigmoid(X @ coef + intercept): main.py:295-296 with cross_entropy folded in."""
    dev = _dev()
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(dev)
    wd = torch.from_numpy(np.ascontiguousarray(coef, dtype=np.float64).ravel()).to(dev)
    return ops.logistic_nll(Xd, wd, float(intercept)).cpu().numpy()


def rlvi_sample_weight(X, coef=None, intercept=0.0, tol=1e-3, maxiter=100):
    """sample_weight for clf.partial_fit (main.py:291-299).  coef None = classifier not fitted
    yet: log_proba = log(0.5) for every row (main.py:293).
    One launch (rlvi_sample_weight_online_f64: X.coef on the fp64 matrix cores -> -log sigmoid -> the online
    E-step) between one pinned H2D copy of [X | coef] and one pinned D2H copy; the host waits once.  Batches of
    more than 4096 rows take the two-launch composition."""
    from .standard import _STAGE
    dev = _dev()
    n = len(X)
    first = coef is None
    if n > 4096:
        if first:
            l = torch.full((n,), float(-np.log(0.5)), dtype=torch.float64, device=dev)
        else:
            Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(dev)
            wd = torch.from_numpy(np.ascontiguousarray(coef, dtype=np.float64).ravel()).to(dev)
            l = ops.logistic_nll(Xd, wd, float(intercept))
        w, _ = ops.update_weights_f64(l, tol=tol, maxiter=maxiter, online=True)
        return w.cpu().numpy()
    Xh = np.ascontiguousarray(X, dtype=np.float64)
    d = Xh.shape[1] if Xh.ndim == 2 else 1
    h_in, h_out, d_in, d_out = _STAGE.get(dev, "online", (n * d + d, n), device_side=True)
    if not first:
        h_in.numpy()[:n * d] = Xh.reshape(-1)
        h_in.numpy()[n * d:] = np.ascontiguousarray(coef, dtype=np.float64).ravel()
        d_in.copy_(h_in, non_blocking=True)
    ops.sample_weight_online(d_in[:n * d].view(n, d), d_in[n * d:], float(intercept), first=first,
                             tol=tol, maxiter=maxiter, out=d_out)
    h_out.copy_(d_out, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    return h_out.numpy()[:n].copy()


def sgd_order(n, random_state=1):
    """The order in which one partial_fit call of scikit-learn's SGDClassifier(random_state=1) visits its n rows (int32
    [n]): a Fisher-Yates shuffle of the identity, j = i + r() % (n - i), r a 32-bit xorshift (13, 17, 5) taken modulo
    2^31.  Its seed is the same in every call, so the order depends on n alone."""
    if random_state != 1:
        raise ValueError("sgd_order knows the seed of random_state=1 only (the reference's, main.py:17-19)")
    idx = np.arange(n, dtype=np.int32)
    s = SGD_SEED_1
    for i in range(n - 1):
        s ^= (s << 13) & 0xFFFFFFFF
        s ^= s >> 17
        s ^= (s << 5) & 0xFFFFFFFF
        j = i + (s % 2147483648) % (n - i)
        idx[i], idx[j] = idx[j], idx[i]
    return idx


def _order_on(dev, n):
    key = (dev.index, n)
    if key not in _ORDERS:
        _ORDERS[key] = torch.from_numpy(sgd_order(n)).to(dev)
    return _ORDERS[key]


def _raise_flags(info, name):
    """The one reading of info[..., 3] (ops.ONLINE_FLAGS): the first flagged (classifier, batch) raises."""
    flags = np.asarray(info).reshape(-1, 4)[:, 3]
    bad = np.flatnonzero(flags)
    if bad.size:
        cls, text = ops.ONLINE_FLAGS.get(int(flags[bad[0]]), (None, "{name}: flag " + str(int(flags[bad[0]]))))
        where = f" (classifier, batch {divmod(int(bad[0]), np.asarray(info).shape[-2])})" if np.ndim(info) == 3 else ""
        raise (cls or _lib.RlviError)(text.format(name=name) + where)


def _labels(y, n):
    yh = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    if yh.size != n or not np.isin(yh, (0.0, 1.0)).all():
        raise ValueError("y must hold one class label 0 or 1 per row")
    return yh


class SGDClassifier:
    """scikit-learn's SGDClassifier as the reference uses it (main.py:16-20): loss='log_loss', random_state=1, every
    other setting at its default (L2 penalty alpha, learning rate 'optimal', an intercept, shuffle, no averaging), two
    classes [0, 1], at most 128 features and 4096 rows per call.  coef_ (1, d), intercept_ (1,), t_ and classes_ exist
    once partial_fit has run (main.py:269-270 asks for classes_)."""

    def __init__(self, loss='log_loss', random_state=1, alpha=1e-4):
        if loss != 'log_loss' or random_state != 1:
            raise ValueError("this mirror runs loss='log_loss' with random_state=1 (main.py:17-19)")
        if not alpha > 0:
            raise ValueError("alpha must be positive")
        self.loss, self.random_state, self.alpha = loss, random_state, float(alpha)
        self.last_info_ = None

    # ---- the fused step
    def _step(self, X, y, method, eps, sample_weight, X_test, y_test):
        from .standard import _STAGE
        dev = _dev()
        Xh = np.ascontiguousarray(X, dtype=np.float64)
        if Xh.ndim != 2 or Xh.shape[0] == 0:
            raise ValueError("X must be [n, d] with n >= 1")
        n, d = Xh.shape
        yh = _labels(y, n)
        first = not hasattr(self, "classes_")
        if not first and d != self.coef_.shape[1]:
            raise ValueError(f"X has {d} features, the classifier {self.coef_.shape[1]}")
        if n > 4096 or d > 128:
            raise _lib.RlviError(f"the online step takes n <= 4096 rows and d <= 128 features: got n = {n}, d = {d}")
        m = 0
        if X_test is not None:
            Xt = np.ascontiguousarray(X_test, dtype=np.float64)
            m = Xt.shape[0]
            if Xt.ndim != 2 or Xt.shape[1] != d or m > 4096:
                raise ValueError("X_test must be [m <= 4096, d]")
            yt = np.ascontiguousarray(y_test, dtype=np.float64).reshape(-1)
            if yt.size != m:
                raise ValueError("y_test must hold one label per test row")
        if method == "GIVEN":
            sw = np.ascontiguousarray(sample_weight, dtype=np.float64).reshape(-1)
            if sw.size != n:
                raise ValueError("sample_weight must hold one weight per row")
            if not np.isfinite(sw).all():
                raise ValueError("Input sample_weight contains NaN or infinity.")
        # one pinned buffer in -- [X | y | state | weights | X_test | y_test] -- and one out -- [state | weights |
        # counts, info]; the host waits once
        sizes = (n * d, n, d + 2, n, m * d, m)
        off = np.concatenate([[0], np.cumsum(sizes)])
        h_in, h_out, d_in, d_out = _STAGE.get(dev, "online_step", (int(off[-1]), d + 2 + n + 4), device_side=True)
        hv = h_in.numpy()
        hv[off[0]:off[1]] = Xh.reshape(-1)
        hv[off[1]:off[2]] = yh
        if first:
            hv[off[2]:off[3]] = 0.0
        else:
            hv[off[2]:off[2] + d] = self.coef_.reshape(-1)
            hv[off[2] + d] = self.intercept_[0]
            hv[off[2] + d + 1] = self.t_
        if method == "GIVEN":
            hv[off[3]:off[4]] = sw
        if m:
            hv[off[4]:off[5]] = Xt.reshape(-1)
            hv[off[5]:off[6]] = yt
        d_in.copy_(h_in, non_blocking=True)
        part = [d_in[off[k]:off[k + 1]] for k in range(6)]
        ints = d_out[d + 2 + n:].view(torch.int32)
        ops.online_step(part[0].view(n, d), part[1], part[2], method=method, eps=0.3 if eps is None else eps,
                        first=first, order=_order_on(dev, n), X_test=part[4].view(m, d) if m else None,
                        y_test=part[5] if m else None, alpha=self.alpha, sample_weight=part[3], counts=ints[:4],
                        info=ints[4:])
        d_out[:d + 2].copy_(part[2], non_blocking=True)
        d_out[d + 2:d + 2 + n].copy_(part[3], non_blocking=True)
        h_out.copy_(d_out, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        res = h_out.numpy()
        tail = res[d + 2 + n:].view(np.int32)
        counts, info = tail[:4].copy(), tail[4:8].copy()
        self.last_info_ = info
        _raise_flags(info, "SGDClassifier.partial_fit")
        self.coef_ = res[:d].copy().reshape(1, d)
        self.intercept_ = res[d:d + 1].copy()
        self.t_ = float(res[d + 1])
        self.classes_ = np.array([0, 1])
        return res[d + 2:d + 2 + n].copy(), (counts if m else None)

    @staticmethod
    def _classes(classes, first):
        if classes is None:
            if first:
                raise ValueError("classes must be passed on the first call to partial_fit.")
        elif list(np.asarray(classes).reshape(-1)) != [0, 1]:
            raise ValueError("this mirror takes classes=[0, 1] (main.py:299)")

    def partial_fit(self, X, y, classes=None, sample_weight=None):
        """One pass over (X, y) with the weights given (None: ones), as clf.partial_fit of main.py:299, :309, :313."""
        self._classes(classes, not hasattr(self, "classes_"))
        self._step(X, y, "SGD" if sample_weight is None else "GIVEN", None, sample_weight, None, None)
        return self

    def partial_fit_weighted(self, X, y, method, eps=None, X_test=None, y_test=None):
        """The mini-batch of main.py:291-313 and :318-331 in ONE launch: the residuals of (X, y) under the current
        state, the sample weights of `method` ('SGD', 'RLVI', 'RRM' with eps), the pass, and the counts of the test
        rows.  Returns (sample_weight [n], counts int32[4] = (tp, tn, fp, fn), or None without test rows)."""
        if method not in ("SGD", "RLVI", "RRM"):
            raise ValueError("method must be 'SGD', 'RLVI' or 'RRM'")
        if method == "RRM":
            from .standard import _rrm_eps
            _rrm_eps("SGDClassifier.partial_fit_weighted", eps, len(X))
        return self._step(X, y, method, eps, None, X_test, y_test)

    # ---- what the reference's loop asks of a fitted classifier (existing ops: rlvi_logistic_nll_f64)
    def predict_log_proba(self, X):
        if not hasattr(self, "classes_"):
            raise AttributeError("this SGDClassifier is not fitted yet")
        dev = _dev()
        Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(dev)
        wd = torch.from_numpy(self.coef_.reshape(-1).copy()).to(dev)
        b = float(self.intercept_[0])
        out = torch.stack([-ops.logistic_nll(Xd, -wd, -b), -ops.logistic_nll(Xd, wd, b)], dim=1)
        return out.cpu().numpy()

    def decision_function(self, X):
        """X coef + intercept as the logit of predict_log_proba: log sigmoid(z) - log sigmoid(-z) = z"""
        lp = self.predict_log_proba(X)
        return lp[:, 1] - lp[:, 0]

    def predict(self, X):
        return self.classes_[(self.decision_function(X) > 0).astype(np.int64)]

    def score(self, X, y):
        return float(np.mean(self.predict(X) == np.asarray(y).reshape(-1)))


def run_stream(X_train, y_train, X_test, y_test, methods=('SGD', 'RRM', 'RLVI'), eps=0.3, alpha=1e-4):
    """The loop of main.py:288-339 as ONE launch: X_train, y_train, X_test, y_test are sequences of T mini-batches
    (their row counts may differ: the reference's last batch is short), one classifier per entry of `methods`, each
    unfitted at the start.  Returns {method: dict(coef_history [T, d], intercept_history [T], t_history [T], counts
    int32[T, 4] = (tp, tn, fp, fn), tp, tn, f1, acc [T] as main.py:320-339 defines them, sample_weight: list of T
    vectors)}."""
    dev = _dev()
    T = len(X_train)
    if T == 0 or not (len(y_train) == len(X_test) == len(y_test) == T):
        raise ValueError("run_stream takes T >= 1 mini-batches of each of its four inputs")
    if len(set(methods)) != len(methods) or not set(methods) <= {"SGD", "RRM", "RLVI"} or not methods:
        raise ValueError("methods: distinct names among 'SGD', 'RRM', 'RLVI'")
    Xs = [np.ascontiguousarray(x, dtype=np.float64) for x in X_train]
    Ts = [np.ascontiguousarray(x, dtype=np.float64) for x in X_test]
    d = Xs[0].shape[1]
    rows = np.array([[x.shape[0], t.shape[0]] for x, t in zip(Xs, Ts)], np.int32)
    n, m = int(rows[:, 0].max()), int(rows[:, 1].max())
    if rows[:, 0].min() < 1 or n > 4096 or m > 4096 or d > 128:
        raise _lib.RlviError("run_stream takes 1 <= n <= 4096 rows, m <= 4096 test rows and d <= 128 features per batch")
    if "RRM" in methods:
        from .standard import _rrm_eps
        _rrm_eps("run_stream", eps, int(rows[:, 0].min()))
    X = np.zeros((T, n, d))
    y = np.zeros((T, n))
    Xt = np.zeros((T, max(m, 1), d))
    yt = np.zeros((T, max(m, 1)))
    orders = np.zeros((T, n), np.int32)
    for k in range(T):
        nk, mk = rows[k]
        if Xs[k].shape != (nk, d) or Ts[k].shape != (mk, d):
            raise ValueError("every mini-batch must have the same number of features")
        X[k, :nk] = Xs[k]
        y[k, :nk] = _labels(y_train[k], nk)
        Xt[k, :mk] = Ts[k]
        yt[k, :mk] = np.asarray(y_test[k], np.float64).reshape(-1)
        orders[k, :nk] = sgd_order(int(nk))
    to = lambda a: torch.from_numpy(a).to(dev)          # noqa: E731
    hist, counts, weights, info = ops.online_stream(to(X), to(y), to(Xt), to(yt), methods=methods, eps=eps,
                                                    rows=to(rows), orders=to(orders), alpha=alpha)
    hist, counts, weights, info = hist.cpu().numpy(), counts.cpu().numpy(), weights.cpu().numpy(), info.cpu().numpy()
    _raise_flags(info, "run_stream")
    out = {}
    for s, name in enumerate(methods):
        c = counts[s].astype(np.float64)
        tp, tn, fp, fn = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
        pos = np.array([np.count_nonzero(np.asarray(v) == 1) for v in y_test], np.float64)
        neg = np.array([np.count_nonzero(np.asarray(v) == 0) for v in y_test], np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[name] = dict(coef_history=hist[s, :, :d].copy(), intercept_history=hist[s, :, d].copy(),
                             t_history=hist[s, :, d + 1].copy(), counts=counts[s].copy(), tp=tp / pos, tn=tn / neg,
                             f1=tp / (tp + (fp + fn) / 2.0), acc=(tp + tn) / rows[:, 1],
                             sample_weight=[weights[s, k, :rows[k, 0]].copy() for k in range(T)], info=info[s].copy())
    return out
