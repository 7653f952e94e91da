"""MI355X mirror of standard-learning/rlvi.py (numpy in, numpy out, fp64).

    update_weights(losses, tol=1e-3, maxiter=100)             reference rlvi.py:8-20
    update_weights_constrained(losses, n_eff, ...)            reference rlvi.py:23-43
    mean / pca / covariance                                    reference rlvi.py:46-65, :111-144
                                                               (one_launch=True: one launch each, moments.hip)
    linear_regression(X, y, maxiter=100, tol=1e-3) -> theta    reference rlvi.py:68-89
    logistic_regression(X, y, maxiter=100, tol=1e-2) -> theta  reference rlvi.py:92-108
    linear_regression_batch / logistic_regression_batch /      the Monte-Carlo loops of reference main.py:170-572:
    mean_batch / pca_batch / covariance_batch                  B problems of one shape in ONE launch

The E-step fixed point and the per-sample NLL (the X.theta contraction) run in
librlvi_gfx950.so, and so does the weighted least-squares solve of linear_regression (normal
equations on the fp64 MFMA units + Cholesky); logistic regression keeps sklearn's liblinear on
the host by default, as the reference has it, and runs as one launch of its own Newton solver
with solver="newton" (logreg.hip).
Host arrays cross PCIe once per call; use rlvi_amd.ops directly to keep data resident.
"""
import collections
import math
import threading

import numpy as np
import torch

from . import _lib, ops


def _dev():
    if not torch.cuda.is_available():
        from ._lib import RlviError
        raise RlviError("rlvi_amd.standard needs an MI355X HIP device (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


# The staging set of a one-launch call: the pinned input buffer and its numpy view, the device input buffer and the
# device views of its parts, the pinned and the device output buffer, the device views {theta, weights, info} of the
# latter and the numpy views (theta, weights, info) of the former.
_OneLaunchSet = collections.namedtuple("_OneLaunchSet", "h_in host d_in views h_out d_out outs res")


class _Staging:
    """Pinned host buffers for the numpy-in / numpy-out calls: one set per (thread, device, tag, sizes), least
    recently used evicted beyond 32 sets.  Keyed by the thread as well: the buffers are written, copied
    asynchronously and read back around ONE host wait, so two threads must never share a set.  A one-launch call's
    set (one_launch) is keyed by how its two buffers are split and keeps the views of the parts with them: a call
    slices nothing."""

    def __init__(self, cap=32):
        self._lock = threading.Lock()
        self._sets = collections.OrderedDict()
        self._cap = cap

    def get(self, dev, tag, sizes, dtype=torch.float64, device_side=False):
        """(h_0, h_1, ...) pinned host buffers of the given lengths; device_side: followed by device buffers of the
        same lengths (kept with the set: a call then allocates nothing)."""
        key = (threading.get_ident(), dev.index, tag, tuple(map(int, sizes)), dtype, device_side)
        with self._lock:
            st = self._sets.get(key)
            if st is not None:
                self._sets.move_to_end(key)
                return st
        st = tuple(torch.empty(max(int(x), 1), dtype=dtype).pin_memory() for x in sizes)
        if device_side:
            st = st + tuple(torch.empty(max(int(x), 1), dtype=dtype, device=dev) for x in sizes)
        return self._keep(key, st)

    def one_launch(self, dev, tag, lengths, nt, n, batch):
        """The set of a one-launch call (_OneLaunchSet) -- inputs of the given lengths in one buffer, {theta [nt],
        weights [n], info int32[4 batch]} in another -- with its views, made once."""
        key = (threading.get_ident(), dev.index, tag, lengths, nt, n, batch)
        with self._lock:
            st = self._sets.get(key)
            if st is not None:
                self._sets.move_to_end(key)
                return st
        sizes = (max(sum(lengths), 1), nt + n + 2 * batch)
        h_in, h_out = (torch.empty(k, dtype=torch.float64).pin_memory() for k in sizes)
        d_in, d_out = (torch.empty(k, dtype=torch.float64, device=dev) for k in sizes)
        offs = [sum(lengths[:i]) for i in range(len(lengths))]
        res = h_out.numpy()
        # info: 4 x int32 per problem behind theta and the weights
        return self._keep(key, _OneLaunchSet(
            h_in, h_in.numpy(), d_in, tuple(d_in[o:o + k] for o, k in zip(offs, lengths)), h_out, d_out,
            dict(theta=d_out[:nt], weights=d_out[nt:nt + n], info=d_out[nt + n:].view(torch.int32)),
            (res[:nt], res[nt:nt + n], res[nt + n:].view(np.int32))))

    def _keep(self, key, st):
        with self._lock:
            self._sets[key] = st
            while len(self._sets) > self._cap:
                self._sets.popitem(last=False)
        return st


_STAGE = _Staging()


def _roundtrip_f64(host_in, fn):
    """numpy in, numpy out through pinned staging buffers: both copies are queued on the stream around the
    launch and the host waits ONCE -- a pageable `.to(device)` and a `.cpu()` are two synchronising copies of
    their own (update_weights at n = 40 ... 1000: 60-66 -> 51-54 us per call; the fp64 iterative kernel and four
    torch calls are the rest).  The result has the input's shape."""
    dev = _dev()
    a = np.ascontiguousarray(host_in, dtype=np.float64)
    shape = a.shape
    a = a.reshape(-1)
    if a.size == 0:
        return np.empty(shape, np.float64)
    h_in, h_out = _STAGE.get(dev, "roundtrip", (a.size, a.size))
    h_in.numpy()[:] = a
    d_out = fn(h_in.to(dev, non_blocking=True))
    h_out.copy_(d_out, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    return h_out.numpy().copy().reshape(shape)


def _one_launch_roundtrip(dev, tag, parts, nt, n, launch, batch=1):
    """The numpy-in / numpy-out call of a one-launch estimator: the host arrays `parts` = [(array or None, length)]
    packed into ONE pinned buffer and copied to the device, launch(device views of the parts, dict(theta [nt],
    weights [n], info int32[4])), ONE pinned copy of {theta, weights, info} back and the one host wait of the call.
    Returns (theta, weights, info) as views of the pinned result -- copy what is handed out -- and the device views.
    batch = B: the batch forms, whose theta, weights and info are B rows of nt, n and 4 (returned flat)."""
    st = _STAGE.one_launch(dev, tag, tuple([int(length) for _, length in parts]), batch * nt, batch * n, batch)
    off = 0
    for a, length in parts:
        if a is not None:
            st.host[off:off + length] = a.reshape(-1)
        off += length
    st.d_in.copy_(st.h_in, non_blocking=True)
    launch(st.views, dict(st.outs))                     # (a copy: launch may add to it)
    st.h_out.copy_(st.d_out, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    return (*st.res, st.views)


def _one_launch_call(name, fn, inputs, args, n, theta_row, second_row, batch=None, pair=False, theta_init=None):
    """What every numpy-level one-launch estimator does around its launch.  fn: the rlvi_amd.ops callee (the batch
    form's with batch = B); inputs: [(host array, shape of its device view -- None: flat)], its leading arguments;
    args: the scalars after them; theta_init: a host vector staged behind the inputs and passed by that keyword; n: the
    samples of a problem; theta_row, second_row: the shape of one problem's theta and of its weights (or scale).  The
    staged output views go to fn as theta=, weights=, info= -- pair: as out=(theta, weights), info= (a theta_row of no
    elements: out=weights) -- with the workspace.  One staging set per `name`, which is the estimator and its form.
    Returns owned copies of theta, the second output and info, [B, ...] with batch = B and unbatched without, then the
    flat device views of the staged arrays and the workspace."""
    dev = _dev()
    ws = ops.workspace(dev, n, 0)
    nt, ns = math.prod(theta_row), math.prod(second_row)
    parts = [(a, a.size) for a, _ in inputs]
    if theta_init is not None:
        parts.append((theta_init, theta_init.size))

    def launch(views, out):
        kw = out
        if pair:
            kw = dict(out=(out["theta"], out["weights"]) if nt else out["weights"], info=out["info"])
        if theta_init is not None:
            kw["theta_init"] = views[-1]
        fn(*[t if shape is None else t.view(shape) for t, (_, shape) in zip(views, inputs)], *args, ws=ws, **kw)
    theta, second, info, views = _one_launch_roundtrip(dev, name, parts, nt, ns, launch, batch=batch or 1)
    theta, second, info = theta.copy(), second.copy(), info.copy()
    if batch is not None:
        lead = (batch,)
        theta, second, info = theta.reshape(lead + theta_row), second.reshape(lead + second_row), info.reshape(batch, 4)
    elif len(theta_row) != 1 or len(second_row) != 1:                # (a covariance matrix, Huber's scalar scale)
        theta, second = theta.reshape(theta_row), second.reshape(second_row)
    return theta, second, info, views, ws


# What a kernel's flag (info[..., 3]) means to the caller, per estimator: {flag: (exception class, message, cap)}.  The
# message is formatted with the estimator's name (and what else _raise_flags is given); cap: the kernel also raised
# RLVI_ST_NOCONV in the workspace's sticky status word.  _CAP: a cap reported through that word.
_CAP = (None, None, True)


def _raise_flags(ws, info, return_info, name, table, batch=False, **fmt):
    """The one reading of info[..., 3].  The lowest flagged problem raises what `table` has for its flag -- a batch
    naming the problem; a single form is a batch of one that does not, and raises with return_info as well.  With
    return_info a batch raises nothing: the caller blanks the flagged rows, info says which.  A _CAP flag raises
    through ws.raise_on_status, which clears the sticky status word; on every other way out the word is cleared here
    if any problem holds a cap flag.  Returns the mask of the flagged problems."""
    flags = info.reshape(-1, 4)[:, 3]
    bad = flags != 0
    if not bad.any():
        return bad
    b = int(np.argmax(bad))
    where = f" (problem {b})" if batch else ""
    # (a flag the table does not know, which no kernel writes today, is taken for a cap: never silent)
    cls, text, _ = table.get(int(flags[b]), _CAP)
    quiet = batch and return_info
    if quiet or cls is not None:
        if any(table.get(int(f), _CAP)[2] for f in flags[bad]):
            ws.clear_status()
        if quiet:
            return bad
        raise cls(text.format(name=name, **fmt) + where)
    try:
        ws.raise_on_status(name, mask=_lib.ST_NOCONV)
    except _lib.RlviError as e:
        raise _lib.RlviError(f"{e}{where}") from None
    return bad


def update_weights(losses, tol=1e-3, maxiter=100):
    '''Optimize Bernoulli probabilities (reference rlvi.py:8-20).'''
    return _roundtrip_f64(losses, lambda l: ops.update_weights_f64(l, tol=tol, maxiter=maxiter)[0])


def _wls(X, y, w):
    """theta = argmin sum_i w_i (y_i - x_i.theta)^2 (rlvi.py:70-71,79-80; the reference materialises
    the n x n diag(sqrt(w)) and calls scipy lstsq).  Here: the weighted Gram matrix on the fp64
    matrix cores + a Cholesky solve, all on the device (rlvi_wls_solve_f64); d > 63 falls back to
    torch.linalg.lstsq on the sqrt(w)-scaled rows."""
    if X.shape[1] <= 63:
        return ops.wls_solve(X, y, w)
    sw = torch.sqrt(w)
    sol = torch.linalg.lstsq(sw[:, None] * X, (sw * y)[:, None])
    return sol.solution[:, 0]


def _linear_regression_host_loop(X, y, maxiter, tol):
    """The general path (any n, d <= 63 on the device solver, rank-deficient designs through the minimum-norm
    kernel): one launch per statement of rlvi.py:76-87 and the stop test on the host, one sync per outer
    iteration.  X, y: device tensors."""
    dev = X.device
    w = torch.ones(X.shape[0], dtype=torch.float64, device=dev)
    theta = _wls(X, y, w)
    losses, _ = ops.linreg_losses(X, y, theta, w)          # rlvi.py:72-74
    outer = 0
    for _ in range(maxiter):
        outer += 1
        w, _ = ops.update_weights_f64(losses)               # rlvi.py:77
        prev = theta
        theta = _wls(X, y, w)                               # rlvi.py:79-80
        losses, _ = ops.linreg_losses(X, y, theta, w)       # rlvi.py:81-83
        disc = torch.linalg.norm(theta - prev) / torch.linalg.norm(prev)
        if bool(disc <= tol):                               # rlvi.py:85-87 (one host sync)
            break
    return theta, w, outer


def linear_regression(X, y, maxiter=100, tol=1e-3, return_info=False):
    """rlvi.py:68-89.  n <= 4096, d <= 31 (the reference's 40 x 10, BASELINE's 1000 x 20): the whole estimator is
    ONE launch (rlvi_linear_regression_f64: E-step, weighted least squares on the fp64 matrix cores, NLL and
    the stop test ||theta - prev|| / ||prev|| <= tol all on the device) between one pinned H2D copy of [X | y]
    and one pinned D2H copy of {theta, weights, info}; the host waits once.  Beyond that, or when the launch
    reports a rank-deficient design: the general path."""
    Xh = np.ascontiguousarray(X, dtype=np.float64)
    yh = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    n, d = Xh.shape
    if n > 0 and d > 0 and ops.linear_regression_check(n, d):
        theta, w, inf, (Xd, yd), ws = _one_launch_call("linear_regression", ops.linear_regression,
                                                       [(Xh, (n, d)), (yh, None)], (maxiter, tol), n, (d,), (n,))
        if inf[3] == 0:
            if not np.isfinite(theta).all():
                # a NaN or inf in y alone passes the pivot test (which looks at X^T W X) and, with maxiter = 0, no
                # second solve meets the NaN weights it makes: the reference's error, as the general path below
                ws.clear_status()
                raise ValueError("array must not contain infs or NaNs")
            if return_info:
                return theta, w, int(inf[0])
            return theta
        Xd = Xd.view(n, d)
    else:
        dev = _dev()
        ws = ops.workspace(dev, n, 0)
        Xd, yd = torch.from_numpy(Xh).to(dev), torch.from_numpy(yh).to(dev)
    theta, w, outer = _linear_regression_host_loop(Xd, yd, maxiter, tol)
    th = theta.cpu().numpy()
    if not np.isfinite(th).all():
        # the reference's error behaviour: scipy's lstsq (rlvi.py:71,80; check_finite) raises this ValueError as
        # soon as a non-finite number reaches it -- in X or y, or in the weights of an exactly interpolating fit
        # (variance 0 -> 0/0 losses); here the NaN has run through to theta instead, which happens in no other case
        ws.clear_status()
        raise ValueError("array must not contain infs or NaNs")
    # a cooperating launch that could not run, a fixed point that did not converge: never silent
    # (RLVI_ST_SINGULAR is information: the minimum-norm solution was returned, as lstsq does)
    ws.raise_on_status("linear_regression", mask=_lib.ST_TIMEOUT | _lib.ST_NOCONV)
    if return_info:
        return th, w.cpu().numpy(), outer
    return th


def _sklearn_log_reg(X_host, y_host, X_dev, w_dev, reg_coeff=1e2):
    """utils.sklearn_log_reg (standard-learning/utils.py:61-73): liblinear fit on the host (third
    party), per-sample loss -log p(class 0 | x) on the device (it does not depend on y)."""
    from sklearn.linear_model import LogisticRegression
    w = (w_dev / w_dev.max()).cpu().numpy()                 # utils.py:66
    clf = LogisticRegression(solver="liblinear", C=reg_coeff)
    clf.fit(X_host, y_host, sample_weight=w)
    theta = np.hstack([clf.intercept_.flatten(), clf.coef_.flatten()])
    coef = torch.from_numpy(clf.coef_.flatten().copy()).to(X_dev.device)
    # -log p(class 0) = -log sigmoid(-(x.w + b)) = logistic_nll(X, -w, -b)
    losses = ops.logistic_nll(X_dev, -coef, -float(clf.intercept_[0]))
    return theta, losses


def _design_inputs(X, y, nonfinite="Input contains NaN or infinity."):
    """X [n, d] and y [n] as contiguous fp64 host arrays, all finite (what is not raises `nonfinite`), before anything
    reaches the device: the single forms' _batch_inputs.  Returns (X, y, n, d)."""
    Xh = np.ascontiguousarray(X, dtype=np.float64)
    yh = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    if Xh.ndim != 2 or yh.shape[0] != Xh.shape[0]:
        raise ValueError("X must be [n, d] and y [n]")
    if not (np.isfinite(Xh).all() and np.isfinite(yh).all()):
        raise ValueError(nonfinite)
    return Xh, yh, *Xh.shape


_LOGREG_FLAGS = {1: (ValueError, "logistic_regression: the fit met numbers that are not finite, or a pivot of its "
                                 "Newton system that is not safely positive (a design scaled beyond what fp64 "
                                 "resolves)", False),
                 2: _CAP}


def _logistic_regression_newton(X, y, maxiter, tol, return_info):
    """solver="newton": one pinned H2D copy of [X | y], ONE launch (rlvi_logistic_regression_f64), one pinned D2H
    copy of {theta, weights, info}, one host wait."""
    # what sklearn's fit raises a ValueError for, before anything reaches the device
    Xh, yh, n, d = _design_inputs(X, y)
    if not np.isin(yh, (0.0, 1.0)).all():
        raise ValueError("y must hold the class labels 0 and 1")
    if n == 0 or yh.min() == yh.max():
        raise ValueError("This solver needs samples of at least 2 classes in the data")
    if d == 0 or not ops.logistic_regression_check(n, d):
        raise _lib.RlviError(f"logistic_regression(solver='newton') takes n <= 4096 samples and 1 <= d <= 30 features "
                             f"in its one launch: got n = {n}, d = {d} (solver='liblinear' has no such limit)")
    theta, w, inf, _, ws = _one_launch_call("logistic_regression", ops.logistic_regression,
                                            [(Xh, (n, d)), (yh, None)], (maxiter, tol), n, (d + 1,), (n,))
    _raise_flags(ws, inf, return_info, "logistic_regression", _LOGREG_FLAGS)
    if return_info:
        return theta, w, int(inf[0])
    return theta


def logistic_regression(X, y, maxiter=100, tol=1e-2, *, solver="liblinear", return_info=False):
    """rlvi.py:92-108.  solver="liblinear" (the default): sklearn's liblinear on the host once per outer iteration,
    as the reference has it.  solver="newton": the whole estimator in ONE launch (n <= 4096, d <= 30, RlviError
    beyond; never a silent change of solver) -- each fit is the minimiser liblinear approximates to its tol = 1e-4,
    so theta agrees with the default's to about 1e-5 relative, not to the bit.  return_info (solver="newton"):
    (theta, weights, outer iterations)."""
    if solver == "newton":
        return _logistic_regression_newton(X, y, maxiter, tol, return_info)
    if solver != "liblinear":
        raise ValueError(f"unknown solver {solver!r}: 'liblinear' or 'newton'")
    if return_info:
        raise ValueError("return_info needs solver='newton'")
    dev = _dev()
    Xh = np.ascontiguousarray(X, dtype=np.float64)
    yh = np.asarray(y)
    Xd = torch.from_numpy(Xh).to(dev)
    w = torch.ones(Xh.shape[0], dtype=torch.float64, device=dev)
    theta, losses = _sklearn_log_reg(Xh, yh, Xd, w)
    for _ in range(maxiter):
        w, _ = ops.update_weights_f64(losses)
        prev = theta.copy()
        theta, losses = _sklearn_log_reg(Xh, yh, Xd, w)
        if np.linalg.norm(theta - prev) / np.linalg.norm(prev) <= tol:
            break
    return theta


# ---- the remaining estimators of standard-learning/rlvi.py on the same GPU E-step.
# n is tens to hundreds here: by default the E-step runs in librlvi_gfx950.so, the small dense algebra around
# it (weighted means, a 2x2 SVD / solve, scipy's 1-D KKT solve) stays on the host as numpy, exactly
# where the reference has it; one_launch=True runs the whole estimator as ONE launch (moments.hip).
def update_weights_constrained(losses, n_eff, tol=1e-3, maxiter=100):
    """rlvi.py:23-43."""
    from scipy import optimize as opt
    losses = np.asarray(losses, np.float64)
    n = len(losses)
    w = update_weights(losses, tol=tol, maxiter=maxiter)

    def shift_obj(s):
        return np.square(np.sum(np.exp(-losses + s) / ((n - n_eff) / n_eff + np.exp(-losses + s))) - n_eff)
    if np.sum(w) < n_eff:
        shift = opt.minimize_scalar(shift_obj)['x']
        w = np.exp(-losses + shift) / ((n - n_eff) / n_eff + np.exp(-losses + shift))
    return w


def _gauss_losses(sample, theta, w):
    r = np.linalg.norm(theta - sample, axis=1) ** 2
    return 0.5 * r / (w @ r / np.sum(w))


def _rrm_eps(what, eps, n):
    if not (0.0 < eps < 1.0 and (1.0 - eps) * n > 1.0):
        raise ValueError(f"{what} needs 0 < eps < 1 and (1 - eps) n > 1: got eps = {eps}, n = {n}")


_VARIANCE_FLAGS = {1: (ValueError, "{kind}: the estimator met numbers that are not finite, or a variance that is not "
                                   "safely positive", False),
                   2: _CAP}
_SINGULAR_FLAGS = {1: (ValueError, "Singular covariance matrix", False), 2: _CAP}          # utils.py:99-100


def _rlvi_args(n, eps, maxiter, tol):
    return maxiter, tol


def _rrm_args(n, eps, maxiter, tol):
    return eps, maxiter, tol


# (kind, rrm) -> the rlvi_amd.ops callee, its scalars of (n, eps, maxiter, tol), theta's shape of d, its flags
_MOMENTS = {
    ("mean", False): ("robust_mean", _rlvi_args, lambda d: (d,), _VARIANCE_FLAGS),
    ("pca", False): ("robust_pca", _rlvi_args, lambda d: (d,), _VARIANCE_FLAGS),
    ("covariance", False): ("robust_covariance", lambda n, eps, maxiter, tol: (n * (1 - eps), maxiter, tol),
                            lambda d: (d, d), _SINGULAR_FLAGS),
    ("mean", True): ("rrm_mean", _rrm_args, lambda d: (d,), _VARIANCE_FLAGS),
    ("pca", True): ("rrm_pca", _rrm_args, lambda d: (d,), _VARIANCE_FLAGS),
    ("covariance", True): ("rrm_covariance", _rrm_args, lambda d: (d, d), _SINGULAR_FLAGS),
}


def _moments(kind, sample, maxiter, tol, return_info, theta_init=None, eps=None, rrm=False, batch=False):
    """one_launch=True of mean / pca / covariance (rlvi_robust_mean_f64 / _pca_f64 / _covariance_f64), rrm: the
    estimators of rlvi_amd/rrm.py on the same path (rlvi_rrm_*_f64), batch: their batch forms on [B, n, d]: one pinned
    H2D copy of the sample (and theta_init), ONE launch, one pinned D2H copy of {theta, weights, info}, one host
    wait."""
    name = ("rrm." if rrm else "") + kind + ("_batch" if batch else "")
    shown = name if rrm or batch else f"{kind}(one_launch=True)"
    if batch:
        xh, _, B, n, d = _batch_inputs("sample", sample)
    else:
        xh = np.ascontiguousarray(sample, dtype=np.float64)
        if xh.ndim != 2:
            raise ValueError("sample must be [n, d]")
        B, (n, d) = None, xh.shape
    init = None if theta_init is None else np.ascontiguousarray(theta_init, dtype=np.float64).reshape(-1)
    if init is not None and init.shape[0] != d:
        raise ValueError("theta_init must have the " + ("samples'" if batch else "sample's") + " d elements")
    # before anything reaches the device (_batch_inputs has looked at the samples of a batch)
    if not ((batch or np.isfinite(xh).all()) and (init is None or np.isfinite(init).all())):
        raise ValueError("Input contains NaN or infinity.")
    if rrm:
        _rrm_eps(name, eps, n)
    elif eps is not None and not 0.0 < eps < 1.0:                    # (eps: the covariance alone)
        raise ValueError(f"{shown} needs 0 < eps < 1 (n_eff = n (1 - eps) inside (0, n)): got {eps}")
    if n == 0 or d == 0 or not ops.moments_check(n, d):
        raise _lib.RlviError(f"{shown} takes 2 <= n <= 4096 samples of 1 <= d <= 8 dimensions with n d <= 16384 in its "
                             f"one launch: got n = {n}, d = {d}"
                             + ("" if rrm or batch else " (one_launch=False has no such limit)"))
    stem, scalars, shape, flags = _MOMENTS[kind, rrm]
    theta, w, inf, _, ws = _one_launch_call(
        name, getattr(ops, stem + "_batch" if batch else stem), [(xh, (n, d) if B is None else (B, n, d))],
        scalars(n, eps, maxiter, tol), n, shape(d), (n,), batch=B, theta_init=init)
    bad = _raise_flags(ws, inf, return_info, name, flags, batch, kind=kind)
    return _results(theta, w, inf, bad, return_info)


def _host_loop_only(one_launch, return_info):
    if return_info and not one_launch:
        raise ValueError("return_info needs one_launch=True")


def mean(sample, maxiter=100, tol=1e-3, *, one_launch=False, return_info=False):
    """rlvi.py:46-65.  one_launch=True: the whole estimator in ONE launch (2 <= n <= 4096, d <= 8, n d <= 16384,
    RlviError beyond; never a silent change of path); return_info: (theta, weights, info int32[4] = {outer
    iterations, inner iterations of the last E-step, inner iterations in all, flag})."""
    _host_loop_only(one_launch, return_info)
    if one_launch:
        return _moments("mean", sample, maxiter, tol, return_info)
    sample = np.asarray(sample, np.float64)
    w = np.ones(sample.shape[0])
    theta = w @ sample / np.sum(w)
    losses = _gauss_losses(sample, theta, w)
    for _ in range(maxiter):
        w = update_weights(losses)
        prev = theta.copy()
        theta = w @ sample / np.sum(w)
        losses = _gauss_losses(sample, theta, w)
        if np.linalg.norm(theta - prev) / np.linalg.norm(prev) <= tol:
            break
    return theta


def _pca_step(sample, w):
    """utils.pca (standard-learning/utils.py:76-89) with the PCA fit as an SVD of the centred,
    weight-scaled rows and sklearn's sign convention."""
    z = w[:, None] * sample
    z = z - z.mean(0)
    _, _, vt = np.linalg.svd(z, full_matrices=False)
    theta = vt[0] / np.linalg.norm(vt[0])
    if theta[np.argmax(np.abs(theta))] < 0:      # sklearn's svd_flip(u_based_decision=False)
        theta = -theta
    return theta, np.sum(sample ** 2, axis=1) - (sample @ theta) ** 2


def pca(sample, maxiter=100, tol=1e-2, theta_init=None, *, one_launch=False, return_info=False):
    """rlvi.py:111-125.  theta_init replaces the first fit and is used as is, not normalised (utils.py:81-88).
    one_launch=True: the whole estimator in ONE launch (limits and return_info as for mean; info[2]: Jacobi sweeps in
    all)."""
    _host_loop_only(one_launch, return_info)
    if one_launch:
        return _moments("pca", sample, maxiter, tol, return_info, theta_init=theta_init)
    sample = np.asarray(sample, np.float64)
    w = np.ones(sample.shape[0])
    if theta_init is None:
        theta, losses = _pca_step(sample, w)
    else:
        theta = np.array(theta_init, np.float64)
        losses = np.sum(sample ** 2, axis=1) - (sample @ theta) ** 2
    for _ in range(maxiter):
        w = update_weights(losses)
        prev = theta.copy()
        theta, losses = _pca_step(sample, w)
        if np.linalg.norm(theta - prev) / np.linalg.norm(prev) <= tol:
            break
    return theta


def _cov_step(sample, w):
    """utils.covariance (utils.py:92-108)."""
    mu = sample.T @ w / np.sum(w)
    c = sample - mu
    cov = c.T @ (w[:, None] * c) / np.sum(w)
    r = np.sum(c * np.linalg.solve(cov, c.T).T, axis=1)
    sign, logdet = np.linalg.slogdet(cov)
    if sign <= 0:
        raise ValueError("Singular covariance matrix")
    return cov, 0.5 * (r + logdet + mu.shape[0] * np.log(2 * np.pi))


def covariance(sample, eps, maxiter=100, tol=1e-2, *, one_launch=False, return_info=False):
    """rlvi.py:128-144.  one_launch=True: the whole estimator in ONE launch (limits and return_info as for mean;
    info[2]: E-steps in which the constraint was active).  Its constrained E-step takes the exact root of the KKT
    condition where this loop hands its square to scipy's Brent search: the two agree to about 1e-8 relative, not to
    the bit."""
    _host_loop_only(one_launch, return_info)
    if one_launch:
        return _moments("covariance", sample, maxiter, tol, return_info, eps=eps)
    sample = np.asarray(sample, np.float64)
    n = sample.shape[0]
    n_eff = n * (1 - eps)
    w = np.ones(n)
    theta, losses = _cov_step(sample, w)
    for _ in range(maxiter):
        w = update_weights_constrained(losses, n_eff)
        prev = theta.copy()
        theta, losses = _cov_step(sample, w)
        if np.linalg.norm(theta - prev, ord='fro') / np.linalg.norm(prev, ord='fro') <= tol:
            break
    return theta


# ---- a Monte-Carlo sweep in ONE launch (the loops of standard-learning/main.py:170-572): B problems of one shape
# stacked on a leading dimension, one workgroup each; problem b gets the bits of the single one-launch call on it alone.
# One pinned H2D copy of the whole batch, ONE launch, one pinned D2H copy of {theta, weights, info}, one host wait --
# never a loop of single calls: a shape beyond the one-launch limits raises RlviError.
def _batch_inputs(what, X, y=None, nonfinite="Input contains NaN or infinity."):
    """[B, n, d] (and y [B, n]) as contiguous fp64 host arrays, all finite: a problem that is not raises what the
    single form raises for it, with its index, before anything reaches the device."""
    Xh = np.ascontiguousarray(X, dtype=np.float64)
    if Xh.ndim != 3:
        raise ValueError(f"{what} must be [B, n, d]")
    B, n, d = Xh.shape
    yh = None
    if y is not None:
        yh = np.ascontiguousarray(y, dtype=np.float64)
        if yh.shape != (B, n):
            raise ValueError("X must be [B, n, d] and y [B, n]")
    if B == 0:
        raise ValueError(f"{what} holds no problem (B = 0)")
    fin = np.isfinite(Xh).reshape(B, -1).all(axis=1)
    if yh is not None:
        fin &= np.isfinite(yh).all(axis=1)
    if not fin.all():
        raise ValueError(f"{nonfinite} (problem {int(np.argmin(fin))})")
    return Xh, yh, B, n, d


def _results(theta, second, info, bad, return_info):
    """What a call hands out after _raise_flags: theta -- with return_info (theta, second, info), the rows of a
    batch's flagged problems (`bad`) NaN."""
    if not return_info:
        return theta
    if info.ndim == 2:
        theta[bad] = np.nan
        second[bad] = np.nan
    return theta, second, info


def linear_regression_batch(X, y, maxiter=100, tol=1e-3, return_info=False):
    """B calls of linear_regression (the sweep of main.py:261-273) as ONE launch: X [B, n, d], y [B, n] -> theta
    [B, d].  n <= 4096, d <= 31 (RlviError beyond).  A problem the launch reports as rank-deficient (info[b, 3] == 1)
    is recomputed by the general path on its device slice, as the single call does.  return_info: (theta, weights
    [B, n], info int32[B, 4]); a recomputed problem's row of info is {its outer iterations, 0, 0, 1}."""
    # (the single call meets a NaN on the device and raises this from its general path; a batch says so up front)
    Xh, yh, B, n, d = _batch_inputs("X", X, y, nonfinite="array must not contain infs or NaNs")
    if B == 0 or n == 0 or d == 0 or not ops.linear_regression_check(n, d):
        raise _lib.RlviError(f"linear_regression_batch takes B >= 1 problems of n <= 4096 samples and 1 <= d <= 31 "
                             f"features in its one launch: got B = {B}, n = {n}, d = {d}")
    theta, w, inf, (Xd, yd), ws = _one_launch_call("linear_regression_batch", ops.linear_regression_batch,
                                                   [(Xh, (B, n, d)), (yh, (B, n))], (maxiter, tol), n, (d,), (n,),
                                                   batch=B)
    for b in np.flatnonzero(inf[:, 3] == 1):
        th_b, w_b, outer = _linear_regression_host_loop(Xd.view(B, n, d)[b], yd.view(B, n)[b], maxiter, tol)
        theta[b] = th_b.cpu().numpy()
        if not np.isfinite(theta[b]).all():
            ws.clear_status()
            raise ValueError(f"array must not contain infs or NaNs (problem {int(b)})")     # as linear_regression
        ws.raise_on_status(f"linear_regression_batch (problem {int(b)})", mask=_lib.ST_TIMEOUT | _lib.ST_NOCONV)
        w[b] = w_b.cpu().numpy()
        inf[b] = (outer, 0, 0, 1)
    if return_info:
        return theta, w, inf
    return theta


def logistic_regression_batch(X, y, maxiter=100, tol=1e-2, return_info=False):
    """B calls of logistic_regression(solver="newton") (main.py:431-437) as ONE launch: X [B, n, d], y [B, n] of 0 / 1
    with both classes in every problem -> theta [B, d + 1].  n <= 4096, d <= 30 (RlviError beyond).  return_info:
    (theta, weights [B, n], info int32[B, 4]); nothing is raised for a problem's flag then, its rows are NaN."""
    Xh, yh, B, n, d = _batch_inputs("X", X, y)
    if not np.isin(yh, (0.0, 1.0)).all():
        b = int(np.argmin(np.isin(yh, (0.0, 1.0)).all(axis=1)))
        raise ValueError(f"y must hold the class labels 0 and 1 (problem {b})")
    if n == 0 or (yh.min(axis=1) == yh.max(axis=1)).any():
        b = 0 if n == 0 else int(np.argmax(yh.min(axis=1) == yh.max(axis=1)))
        raise ValueError(f"This solver needs samples of at least 2 classes in the data (problem {b})")
    if d == 0 or not ops.logistic_regression_check(n, d):
        raise _lib.RlviError(f"logistic_regression_batch takes n <= 4096 samples and 1 <= d <= 30 features in its one "
                             f"launch: got n = {n}, d = {d}")
    theta, w, inf, _, ws = _one_launch_call("logistic_regression_batch", ops.logistic_regression_batch,
                                            [(Xh, (B, n, d)), (yh, (B, n))], (maxiter, tol), n, (d + 1,), (n,), batch=B)
    bad = _raise_flags(ws, inf, return_info, "logistic_regression_batch", _LOGREG_FLAGS, batch=True)
    return _results(theta, w, inf, bad, return_info)


def mean_batch(sample, maxiter=100, tol=1e-3, return_info=False):
    """B calls of mean(one_launch=True) (main.py:180-188) as ONE launch: sample [B, n, d] -> theta [B, d]; limits and
    return_info as for mean, info int32[B, 4]; with return_info a flagged problem's rows are NaN, nothing is raised."""
    return _moments("mean", sample, maxiter, tol, return_info, batch=True)


def pca_batch(sample, maxiter=100, tol=1e-2, theta_init=None, return_info=False):
    """B calls of pca(one_launch=True) (main.py:489-494) as ONE launch: sample [B, n, d], ONE theta_init [d] for all
    problems (as in the reference's loop) -> theta [B, d]."""
    return _moments("pca", sample, maxiter, tol, return_info, theta_init=theta_init, batch=True)


def covariance_batch(sample, eps, maxiter=100, tol=1e-2, return_info=False):
    """B calls of covariance(one_launch=True) (main.py:539-544) as ONE launch: sample [B, n, d], ONE eps for all
    problems -> theta [B, d, d]."""
    return _moments("covariance", sample, maxiter, tol, return_info, eps=eps, batch=True)
