"""What a numpy-level one-launch estimator makes of its kernel's flag (info[..., 3]), pinned without a device: the
exception class and the whole message, what comes back with return_info, what the workspace is asked (raise_on_status:
the name and the mask) and whether the sticky status word is cleared.  Every function of rlvi_amd.standard, .rrm and
.huber that goes through one launch, in its single and its batch form, with return_info false and true, at every flag
its kernel can write (the `info` comments of rlvi_amd/ops.py).

Four seams stand in for the device: standard._dev, ops.workspace (FakeWorkspace below), standard._one_launch_roundtrip
(fabricated theta, weights and info with the flags of the case) and the two general-path loops
(standard._linear_regression_host_loop, rrm._linear_regression_host_loop).  The rule the cases pin:

    single form     raises for its flag whether return_info is set or not;
    batch form      raises for the LOWEST flagged problem, the message ending in " (problem b)"; with return_info it
                    raises nothing, the flagged problems' rows of theta and of weights / scale are NaN, info comes back
                    as the kernel wrote it;
    a cap flag      goes through ws.raise_on_status(name, ST_NOCONV), which clears the word itself -- but Huber's, which
                    has a message of its own and clears first;
    clear_status    is called when nothing goes through raise_on_status and some problem holds a cap flag;
    flag 1 of standard.linear_regression(_batch) and of rrm.linear_regression is a recomputation by the general path."""
import numpy as np
import pytest
import torch

N, D, B = 12, 2, 4
NOCONV = 4                       # _lib.ST_NOCONV
TIMEOUT_NOCONV = 6               # _lib.ST_TIMEOUT | _lib.ST_NOCONV
STATUS_TEXT = "device status 4: the cap was reached"

LOGIT_FLAG1 = ("logistic_regression: the fit met numbers that are not finite, or a pivot of its Newton system that is "
               "not safely positive (a design scaled beyond what fp64 resolves)")
MEAN_FLAG1 = "mean: the estimator met numbers that are not finite, or a variance that is not safely positive"
PCA_FLAG1 = "pca: the estimator met numbers that are not finite, or a variance that is not safely positive"
COV_FLAG1 = "Singular covariance matrix"
NONFINITE = "array must not contain infs or NaNs"
RRM_LOGIT_FLAG1 = ("y must hold the class labels 0 and 1, and the fit must not meet numbers that are not finite (a "
                   "design scaled beyond what fp64 resolves)")
HUBER_CAP = "the iteration still moved by more than 1e-6 after maxiter = 1000 iterations"

_rng = np.random.default_rng(5)
X1 = _rng.standard_normal((N, D))
Y1 = _rng.standard_normal(N)
L1 = (np.arange(N) % 2).astype(np.float64)                   # labels, both classes
XB = _rng.standard_normal((B, N, D))
YB = _rng.standard_normal((B, N))
LB = np.stack([L1] * B)


@pytest.fixture(scope="module")
def lib():
    from rlvi_amd import _build, _lib
    _build.build()
    return _lib.load()


class FakeWorkspace:
    """Records what it is asked.  raise_on_status raises on a status bit of the mask, as the real one does, without
    counting as a clear_status() call of the code under test."""

    def __init__(self):
        self.status, self.clears, self.asked = 0, 0, []

    def clear_status(self):
        self.clears += 1

    def raise_on_status(self, what, mask=7):
        from rlvi_amd import _lib
        self.asked.append((what, mask))
        if self.status & mask:
            raise _lib.RlviError(f"{what}: {STATUS_TEXT}")
        return self.status


class Seams:
    def __init__(self):
        self.ws = FakeWorkspace()
        self.flags = None
        self.fab = None              # (theta [batch, nt], second [batch, n], info [batch, 4]) as fabricated
        self.loops = []              # the general-path loops' calls: (X, y) as numpy

    def roundtrip(self, dev, tag, parts, nt, n, launch, batch=1):
        """standard._one_launch_roundtrip without a device: the parts as flat CPU tensors where the device views go,
        theta, weights and info as flat views of ONE buffer (what the pinned result is)."""
        flags = np.asarray(self.flags, np.int32).reshape(-1)
        assert flags.size == batch
        for a, length in parts:
            assert a is None or a.size == length
        views = [torch.zeros(length, dtype=torch.float64) if a is None else
                 torch.from_numpy(np.array(a, np.float64).reshape(-1)) for a, length in parts]
        res = np.empty(batch * (nt + n) + 2 * batch)
        res[:batch * nt] = 1000.0 + np.arange(batch * nt)
        res[batch * nt:batch * (nt + n)] = 2000.0 + np.arange(batch * n)
        info = res[batch * (nt + n):].view(np.int32)
        info[:] = 0
        info.reshape(batch, 4)[:, :3] = 5 + np.arange(3 * batch).reshape(batch, 3)
        info.reshape(batch, 4)[:, 3] = flags
        theta, second = res[:batch * nt], res[batch * nt:batch * (nt + n)]
        self.fab = (theta.copy().reshape(batch, nt), second.copy().reshape(batch, n), info.copy().reshape(batch, 4))
        return theta, second, info, views


@pytest.fixture
def seams(lib, monkeypatch):
    from rlvi_amd import ops, standard
    s = Seams()
    monkeypatch.setattr(standard, "_dev", lambda: torch.device("cpu"))
    monkeypatch.setattr(ops, "workspace", lambda device, n=0, b=0: s.ws)
    monkeypatch.setattr(standard, "_one_launch_roundtrip", s.roundtrip)
    return s


class Spec:
    """One estimator: its two forms as callables of return_info, the lengths of a problem's theta and second output,
    value = {flag: (exception class, the single form's message, the batch form's before the problem suffix)}, caps =
    {flag: "status" or "own"}, the names given to raise_on_status (or leading Huber's own message)."""

    def __init__(self, name, single, batch, nt, second, value, caps, what, what_batch, theta_shape=None,
                 single_value=None):
        self.name, self.single, self.batch, self.nt, self.second = name, single, batch, nt, second
        self.value, self.caps, self.what, self.what_batch = value, caps, what, what_batch
        self.theta_shape = theta_shape or (nt,)
        self.single_value = value if single_value is None else single_value      # (rrm.linear_regression: flag 1)

    def __repr__(self):
        return self.name


def _specs():
    from rlvi_amd import _lib, huber, rrm, standard
    moments = dict(nt=D, second=N, caps={2: "status"})
    S = [
        Spec("standard.logistic_regression",
             lambda ri: standard.logistic_regression(X1, L1, solver="newton", return_info=ri),
             lambda ri: standard.logistic_regression_batch(XB, LB, return_info=ri),
             D + 1, N, {1: (ValueError, LOGIT_FLAG1, LOGIT_FLAG1)}, {2: "status"},
             "logistic_regression", "logistic_regression_batch"),
        Spec("standard.mean", lambda ri: standard.mean(X1, one_launch=True, return_info=ri),
             lambda ri: standard.mean_batch(XB, return_info=ri), value={1: (ValueError, MEAN_FLAG1, MEAN_FLAG1)},
             what="mean", what_batch="mean_batch", **moments),
        Spec("standard.pca", lambda ri: standard.pca(X1, one_launch=True, return_info=ri),
             lambda ri: standard.pca_batch(XB, theta_init=[0.6, 0.8], return_info=ri),
             value={1: (ValueError, PCA_FLAG1, PCA_FLAG1)}, what="pca", what_batch="pca_batch", **moments),
        Spec("standard.covariance", lambda ri: standard.covariance(X1, 0.2, one_launch=True, return_info=ri),
             lambda ri: standard.covariance_batch(XB, 0.2, return_info=ri), D * D, N,
             {1: (ValueError, COV_FLAG1, COV_FLAG1)}, {2: "status"}, "covariance", "covariance_batch",
             theta_shape=(D, D)),
        Spec("rrm.mean", lambda ri: rrm.mean(X1, 0.2, return_info=ri),
             lambda ri: rrm.mean_batch(XB, 0.2, return_info=ri),
             value={1: (ValueError, MEAN_FLAG1, MEAN_FLAG1)}, what="rrm.mean", what_batch="rrm.mean_batch", **moments),
        Spec("rrm.pca", lambda ri: rrm.pca(X1, 0.2, theta_init=[0.6, 0.8], return_info=ri),
             lambda ri: rrm.pca_batch(XB, 0.2, return_info=ri), value={1: (ValueError, PCA_FLAG1, PCA_FLAG1)},
             what="rrm.pca", what_batch="rrm.pca_batch", **moments),
        Spec("rrm.covariance", lambda ri: rrm.covariance(X1, 0.2, return_info=ri),
             lambda ri: rrm.covariance_batch(XB, 0.2, return_info=ri), D * D, N,
             {1: (ValueError, COV_FLAG1, COV_FLAG1)}, {2: "status"}, "rrm.covariance", "rrm.covariance_batch",
             theta_shape=(D, D)),
        Spec("rrm.update_weights", lambda ri: rrm.update_weights(np.abs(Y1), 0.2, return_info=ri), None, 0, N,
             {1: (ValueError, "rrm.update_weights: a loss is not finite", None)}, {2: "status"},
             "rrm.update_weights", None),
        Spec("rrm.linear_regression", lambda ri: rrm.linear_regression(X1, Y1, 0.2, return_info=ri),
             lambda ri: rrm.linear_regression_batch(XB, YB, 0.2, return_info=ri), D, N,
             {1: (ValueError, None, "rrm.linear_regression_batch: a rank-deficient design (rrm.linear_regression takes "
                                    "its general path there)"),
              2: (ValueError, None, "rrm.linear_regression_batch: array must not contain infs or NaNs")},
             {3: "status"}, "rrm.linear_regression", "rrm.linear_regression_batch",
             single_value={2: (ValueError, NONFINITE, None)}),
        Spec("huber.linear_regression", lambda ri: huber.linear_regression(X1, Y1, return_info=ri),
             lambda ri: huber.linear_regression_batch(XB, YB, return_info=ri), D, 1,
             {1: (np.linalg.LinAlgError, "Singular matrix", "Singular matrix"), 2: (ValueError, NONFINITE, NONFINITE)},
             {3: "own"}, "huber.linear_regression", "huber.linear_regression_batch"),
        Spec("rrm.logistic_regression", lambda ri: rrm.logistic_regression(X1, L1, 0.2, return_info=ri),
             lambda ri: rrm.logistic_regression_batch(XB, LB, 0.2, return_info=ri), D + 1, N,
             {1: (ValueError, "rrm.logistic_regression: " + RRM_LOGIT_FLAG1,
                  "rrm.logistic_regression_batch: " + RRM_LOGIT_FLAG1)},
             {2: "status", 3: "status"}, "rrm.logistic_regression", "rrm.logistic_regression_batch"),
    ]
    assert _lib.ST_NOCONV == NOCONV and _lib.ST_TIMEOUT | _lib.ST_NOCONV == TIMEOUT_NOCONV
    return S


SPECS = _specs()
SINGLE_CASES = [(s, f, ri) for s in SPECS for f in [0, *s.single_value, *s.caps] for ri in (False, True)]


def _batch_flag_sets(s):
    sets = [(0, 0, 0, 0)] + [(0, 0, f, 0) for f in [*s.value, *s.caps]]
    for v in s.value:
        for c in s.caps:
            sets += [(0, v, 0, c), (0, c, 0, v)]
    return sets


BATCH_CASES = [(s, fl, ri) for s in SPECS if s.batch for fl in _batch_flag_sets(s) for ri in (False, True)]


def _expect_raise(spec, flag, what, message, suffix, any_cap):
    """(exception class, whole message, raise_on_status calls, cleared) of a raising call that reports `flag`"""
    from rlvi_amd import _lib
    if flag in spec.caps and spec.caps[flag] == "status":
        return _lib.RlviError, f"{what}: {STATUS_TEXT}{suffix}", [(what, NOCONV)], False
    if flag in spec.caps:                                             # Huber's cap: its own message, cleared first
        return _lib.RlviError, f"{what}: {HUBER_CAP}{suffix}", [], True
    cls, text = message
    return cls, text + suffix, [], any_cap


def _check_raise(seams, call, want):
    cls, text, asked, cleared = want
    with pytest.raises(cls) as e:
        call()
    assert type(e.value) is cls and str(e.value) == text
    assert seams.ws.asked == asked
    assert (seams.ws.clears >= 1) == cleared


@pytest.mark.parametrize("spec,flag,return_info", SINGLE_CASES, ids=lambda v: str(v))
def test_single_form(seams, spec, flag, return_info):
    seams.flags = [flag]
    seams.ws.status = NOCONV if flag in spec.caps else 0
    if flag:
        message = spec.single_value[flag][:2] if flag in spec.single_value else None
        _check_raise(seams, lambda: spec.single(return_info),
                     _expect_raise(spec, flag, spec.what, message, "", flag in spec.caps))
        return
    res = spec.single(return_info)
    theta, second, info = (a[0] for a in seams.fab)
    assert seams.ws.asked == [] and seams.ws.clears == 0
    if not return_info:
        want = theta.reshape(spec.theta_shape) if spec.nt else second
        assert isinstance(res, np.ndarray) and res.shape == want.shape and np.array_equal(res, want)
        return
    if spec.name == "rrm.update_weights":                             # (weights, info)
        res = (None, *res)
    assert len(res) == 3
    if spec.nt:
        assert res[0].shape == spec.theta_shape and np.array_equal(res[0], theta.reshape(spec.theta_shape))
    if spec.name == "huber.linear_regression":
        assert type(res[1]) is float and res[1] == second[0]
    else:
        assert res[1].shape == (N,) and np.array_equal(res[1], second)
    if spec.name == "standard.logistic_regression":                   # (theta, weights, outer iterations)
        assert type(res[2]) is int and res[2] == int(info[0])
    else:
        assert res[2].dtype == np.int32 and res[2].shape == (4,) and np.array_equal(res[2], info)


@pytest.mark.parametrize("spec,flags,return_info", BATCH_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_batch_form(seams, spec, flags, return_info):
    seams.flags = flags
    any_cap = any(f in spec.caps for f in flags)
    seams.ws.status = NOCONV if any_cap else 0
    flagged = [b for b, f in enumerate(flags) if f]
    if flagged and not return_info:
        b = flagged[0]
        message = (spec.value[flags[b]][0], spec.value[flags[b]][2]) if flags[b] in spec.value else None
        _check_raise(seams, lambda: spec.batch(False),
                     _expect_raise(spec, flags[b], spec.what_batch, message, f" (problem {b})", any_cap))
        return
    res = spec.batch(return_info)
    theta, second, info = seams.fab
    assert seams.ws.asked == []
    assert (seams.ws.clears >= 1) == any_cap
    if not return_info:
        assert res.shape == (B,) + spec.theta_shape and np.array_equal(res.reshape(B, -1), theta)
        return
    got_theta, got_second, got_info = res
    assert got_theta.shape == (B,) + spec.theta_shape
    assert got_second.shape == ((B,) if spec.second == 1 else (B, N))
    assert got_info.dtype == np.int32 and got_info.shape == (B, 4) and np.array_equal(got_info, info)
    got_theta, got_second = got_theta.reshape(B, -1), got_second.reshape(B, -1)
    for b in range(B):
        if flags[b]:
            assert np.isnan(got_theta[b]).all() and np.isnan(got_second[b]).all()
        else:
            assert np.array_equal(got_theta[b], theta[b]) and np.array_equal(got_second[b], second[b])


# ---- flag 1 of the linear regressions that have a general path: a recomputation, nothing raised
LOOP_THETA, LOOP_W, LOOP_OUTER = np.array([-3.0, 4.5]), 0.25 + np.arange(N) / 100.0, 7


@pytest.mark.parametrize("return_info", (False, True))
def test_standard_linear_regression_takes_the_general_path(seams, monkeypatch, return_info):
    from rlvi_amd import standard

    def loop(X, y, maxiter, tol):
        seams.loops.append((X.numpy().copy(), y.numpy().copy(), maxiter, tol))
        return torch.from_numpy(LOOP_THETA.copy()), torch.from_numpy(LOOP_W.copy()), LOOP_OUTER
    monkeypatch.setattr(standard, "_linear_regression_host_loop", loop)
    seams.flags = [1]
    res = standard.linear_regression(X1, Y1, maxiter=50, tol=1e-4, return_info=return_info)
    (Xl, yl, maxiter, tol), = seams.loops
    assert np.array_equal(Xl, X1) and np.array_equal(yl, Y1) and (maxiter, tol) == (50, 1e-4)
    assert seams.ws.asked == [("linear_regression", TIMEOUT_NOCONV)] and seams.ws.clears == 0
    if not return_info:
        assert np.array_equal(res, LOOP_THETA)
        return
    assert np.array_equal(res[0], LOOP_THETA) and np.array_equal(res[1], LOOP_W) and res[2] == LOOP_OUTER
    # and a clean launch: (theta, weights, outer iterations) as the kernel left them
    seams.flags, seams.ws.asked = [0], []
    theta, w, outer = standard.linear_regression(X1, Y1, return_info=True)
    assert np.array_equal(theta, seams.fab[0][0]) and np.array_equal(w, seams.fab[1][0])
    assert outer == int(seams.fab[2][0, 0]) and seams.ws.asked == [] and seams.ws.clears == 0
    assert np.array_equal(standard.linear_regression(X1, Y1), seams.fab[0][0])


@pytest.mark.parametrize("flags", [(0, 0, 0, 0), (0, 0, 1, 0), (0, 1, 0, 1)], ids=str)
@pytest.mark.parametrize("return_info", (False, True))
def test_standard_linear_regression_batch_takes_the_general_path(seams, monkeypatch, flags, return_info):
    from rlvi_amd import standard

    def loop(X, y, maxiter, tol):
        seams.loops.append((X.numpy().copy(), y.numpy().copy()))
        k = len(seams.loops)
        return torch.from_numpy(LOOP_THETA * k), torch.from_numpy(LOOP_W * k), LOOP_OUTER + k
    monkeypatch.setattr(standard, "_linear_regression_host_loop", loop)
    seams.flags = flags
    res = standard.linear_regression_batch(XB, YB, return_info=return_info)
    theta, w, info = seams.fab
    flagged = [b for b, f in enumerate(flags) if f]
    assert len(seams.loops) == len(flagged)
    assert seams.ws.asked == [(f"linear_regression_batch (problem {b})", TIMEOUT_NOCONV) for b in flagged]
    assert seams.ws.clears == 0
    for k, b in enumerate(flagged, 1):
        assert np.array_equal(seams.loops[k - 1][0], XB[b]) and np.array_equal(seams.loops[k - 1][1], YB[b])
        theta[b], w[b], info[b] = LOOP_THETA * k, LOOP_W * k, (LOOP_OUTER + k, 0, 0, 1)
    if not return_info:
        assert res.shape == (B, D) and np.array_equal(res, theta)
        return
    assert np.array_equal(res[0], theta) and np.array_equal(res[1], w)
    assert res[2].dtype == np.int32 and np.array_equal(res[2], info)


@pytest.mark.parametrize("return_info", (False, True))
def test_rrm_linear_regression_takes_the_general_path(seams, monkeypatch, return_info):
    from rlvi_amd import rrm

    def loop(X, y, eps, maxiter, tol, ws):
        seams.loops.append((X.numpy().copy(), y.numpy().copy(), eps, maxiter, tol, ws))
        return LOOP_THETA.copy(), LOOP_W.copy(), LOOP_OUTER
    monkeypatch.setattr(rrm, "_linear_regression_host_loop", loop)
    seams.flags = [1]
    res = rrm.linear_regression(X1, Y1, 0.2, maxiter=50, tol=1e-4, return_info=return_info)
    (Xl, yl, eps, maxiter, tol, ws), = seams.loops
    assert np.array_equal(Xl, X1) and np.array_equal(yl, Y1) and (eps, maxiter, tol) == (0.2, 50, 1e-4)
    assert ws is seams.ws and seams.ws.asked == [] and seams.ws.clears == 0
    if not return_info:
        assert np.array_equal(res, LOOP_THETA)
        return
    assert np.array_equal(res[0], LOOP_THETA) and np.array_equal(res[1], LOOP_W)
    assert res[2].dtype == np.int32 and res[2].tolist() == [LOOP_OUTER, 0, 0, 1]


def test_standard_linear_regression_refuses_a_theta_that_is_not_finite(seams, monkeypatch):
    """A clean flag over a NaN theta (a NaN in y alone), and a general path that ends in one: the reference's error,
    the status word cleared."""
    from rlvi_amd import standard
    seams.flags = [0]
    roundtrip = seams.roundtrip

    def nan_theta(*a, **kw):
        theta, w, info, views = roundtrip(*a, **kw)
        theta[1] = np.nan
        return theta, w, info, views
    monkeypatch.setattr(standard, "_one_launch_roundtrip", nan_theta)
    with pytest.raises(ValueError) as e:
        standard.linear_regression(X1, Y1)
    assert str(e.value) == NONFINITE and seams.ws.clears >= 1 and seams.ws.asked == []
    monkeypatch.setattr(standard, "_one_launch_roundtrip", roundtrip)
    monkeypatch.setattr(standard, "_linear_regression_host_loop", lambda X, y, maxiter, tol: (
        torch.tensor([np.nan, 1.0], dtype=torch.float64), torch.from_numpy(LOOP_W.copy()), 3))
    for call, text in ((lambda: standard.linear_regression(X1, Y1), NONFINITE),
                       (lambda: standard.linear_regression_batch(XB, YB), NONFINITE + " (problem 2)")):
        seams.flags, seams.ws.clears = ([1] if "problem" not in text else (0, 0, 1, 0)), 0
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text and seams.ws.clears >= 1 and seams.ws.asked == []
