"""The online path's SGD pass without a GPU: the numpy restatement tests/online_ref.py against what scikit-learn and the
reference left in tests/golden/g21_online_sgd.npz (tools/make_golden_online.py), the order of the pass, the argument
checks of the two C entries, the mirror's interface and what it raises for the kernel's flags.

Bars.  t_ and the four counts: equal.  Coefficients and intercept of a (method, batch): |delta| <=
32 x noise x max |coef|, noise the fixture's per-method distance between the restatement with sequential and with
64-leaf tree dot products; RRM, whose reference stops at Brent's tolerance: 4 x rrm_dev x max |coef|, rrm_dev measured by
the tool.  Weights: RLVI rtol 1e-9 (the online E-step's bar of tests/test_gpu_parity.py), RRM rtol 10 x w_bar of G18 (the
bar of tests/test_rrm_cpu.py), both atol 1e-300."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import online_ref as R  # noqa: E402

G21 = np.load(os.path.join(HERE, "golden", "g21_online_sgd.npz"))
W_BAR = float(np.load(os.path.join(HERE, "golden", "g18_rrm.npz"))["w_bar"])
STREAMS = [str(s) for s in G21["streams"]]
K_NOISE, K_RRM = 32.0, 4.0
_CACHE = {}


def load_stream(name):
    g = {k: G21[f"{name}/{k}"] for k in ("X", "y", "Xt", "yt", "rows", "orders", "methods", "state_hist", "weights",
                                         "counts", "noise", "rrm_dev")}
    for k in ("X", "y", "Xt", "yt"):
        g[k] = g[k].astype(np.float64)
    g["alpha"], g["eps"] = float(G21[f"{name}/alpha"]), float(G21[f"{name}/eps"])
    g["given"] = G21[f"{name}/given"] if f"{name}/given" in G21.files else None
    return g


def restated(name, tree=False):
    """the restatement's stream, computed once per (stream, summation) and shared"""
    if (name, tree) not in _CACHE:
        g = load_stream(name)
        _CACHE[name, tree] = R.stream(g["X"], g["y"], g["Xt"], g["yt"], g["rows"], list(g["methods"]), g["eps"],
                                      g["given"], g["alpha"], tree=tree)
    return _CACHE[name, tree]


def check_against_fixture(name, hist, counts, weights, what):
    """the bars of the module docstring on a [S, T, ...] result; prints every figure before it asserts"""
    g = load_stream(name)
    d = g["X"].shape[2]
    for s, m in enumerate(g["methods"]):
        ref = g["state_hist"][s]
        scale = np.abs(ref[:, :d + 1]).max(axis=1)
        dist = np.abs(hist[s][:, :d + 1] - ref[:, :d + 1]).max(axis=1)
        bar = (K_RRM * float(g["rrm_dev"]) if m == R.METHODS["RRM"] else K_NOISE * g["noise"][s]) * scale
        print(f"{what} {name} method {m}: max |coef - fixture| / max |coef| per batch "
              f"{np.array2string(dist / scale, precision=2)} (bar {np.array2string(bar / scale, precision=2)})")
        assert np.array_equal(hist[s][:, d + 1], ref[:, d + 1]), "t_"
        assert np.array_equal(counts[s], g["counts"][s]), "counts"
        assert (dist <= bar).all()
        for k in range(ref.shape[0]):
            nk = g["rows"][k, 0]
            w, w_ref = weights[s, k, :nk], g["weights"][s, k, :nk]
            if m == R.METHODS["SGD"]:
                assert np.array_equal(w, np.ones(nk))
            elif m == R.METHODS["GIVEN"]:
                assert np.array_equal(w, w_ref)
            else:
                np.testing.assert_allclose(w, w_ref, rtol=1e-9 if m == R.METHODS["RLVI"] else 10 * W_BAR, atol=1e-300)


@pytest.mark.parametrize("name", STREAMS)
def test_restatement_against_scikit_learn_and_the_reference(name):
    r = restated(name)
    check_against_fixture(name, r["state_hist"], r["counts"], r["weights"], "online_ref")
    assert not r["flags"].any()


def test_fixture_covers_the_branches_and_the_shapes():
    c = dict(zip(R.COUNTERS, G21["counters"]))
    assert c["tail"] > 0 and c["zero_update"] > 0 and c["reset"] > 0 and c["clip"] == 0
    shapes = {s: G21[f"{s}/X"].shape for s in STREAMS}
    assert shapes["har"][1:] == (100, 60) and shapes["har"][0] >= 5 and list(G21["har/rows"][-1]) == [38, 37]
    assert shapes["small"] == (6, 17, 3) and shapes["boundary"] == (4, 257, 64)
    assert shapes["two_col"][1:] == (40, 65) and shapes["widest"][2] == 128 and shapes["one_col"][2] == 1
    assert shapes["one_row"][1] == 1 and shapes["two_rows"][1] == 2
    assert (G21["given/given"] == 0.0).any() and float(G21["alpha1/alpha"]) == 1.0
    for s in STREAMS:
        assert float(G21[f"{s}/decision_min"]) >= 1e-6
        assert (G21[f"{s}/noise"] >= 2.0 ** -52).all()
    assert os.path.getsize(os.path.join(HERE, "golden", "g21_online_sgd.npz")) < 1000 * 1000
    assert str(G21["v_sklearn"]) == "1.7.2"


@pytest.mark.parametrize("n", [1, 2, 3, 17, 38, 100, 257, 4096])
def test_sgd_order_is_scikit_learns(n):
    from rlvi_amd import online
    want = G21[f"order/{n}"]
    assert sorted(want.tolist()) == list(range(n))
    assert np.array_equal(R.sgd_order(n), want)
    got = online.sgd_order(n)
    assert got.dtype == np.int32 and np.array_equal(got, want)


def test_sgd_order_knows_one_seed():
    from rlvi_amd import online
    with pytest.raises(ValueError):
        online.sgd_order(5, random_state=2)
    rs = np.random.RandomState(1)
    rs.randint(1, 2 ** 31 - 1)
    assert online.SGD_SEED_1 == R.SEED == rs.randint(2 ** 31 - 1) == 2135392491


@pytest.fixture(scope="module")
def lib():
    from rlvi_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_argument_errors_without_a_gpu(lib):
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 255) & ~255

    def step(X=p, y=p, order=None, n=8, d=3, method=0, eps=0.3, first=1, state=p, Xt=p, yt=p, m=2, alpha=1e-4,
             tol=1e-3, maxiter=100, sw=p, counts=p, info=p):
        return lib.rlvi_online_step_f64(X, y, order, n, d, method, eps, first, state, Xt, yt, m, alpha, tol, maxiter, sw,
                                        counts, info, None)
    for k in ("X", "y", "state", "counts", "info", "Xt", "yt"):
        assert step(**{k: None}) == -1, k
    assert step(sw=None, method=3) == -1
    for kw in (dict(n=0), dict(d=0), dict(m=-1), dict(maxiter=-1), dict(method=4), dict(method=-1), dict(alpha=0.0),
               dict(alpha=float("nan")), dict(method=2, eps=0.0), dict(method=2, eps=1.0)):
        assert step(**kw) == -2, kw
    for kw in (dict(n=4097), dict(m=4097), dict(d=129)):
        assert step(**kw) == -5, kw
    for k in ("X", "y", "state", "Xt", "yt", "sw"):
        assert step(**{k: p + 4}) == -3, k
    for k in ("order", "counts", "info"):
        assert step(**{k: p + 2}) == -3, k

    methods = (ctypes.c_int32 * 3)(0, 2, 1)
    eps = (ctypes.c_double * 3)(0.3, 0.3, 0.3)

    def stream(X=p, y=p, Xt=p, yt=p, rows=p, orders=p, T=2, n=8, m=2, d=3, methods=methods, eps=eps, S=3, alpha=1e-4,
               tol=1e-3, maxiter=100, hist=p, counts=p, weights=p, info=p):
        return lib.rlvi_online_stream_f64(X, y, Xt, yt, rows, orders, T, n, m, d, methods, eps, S, alpha, tol, maxiter,
                                          hist, counts, weights, info, None)
    for k in ("X", "y", "Xt", "yt", "methods", "hist", "counts", "info"):
        assert stream(**{k: None}) == -1, k
    assert stream(eps=None) == -1                                   # a method 2 without its eps
    assert stream(methods=(ctypes.c_int32 * 3)(0, 3, 1), weights=None) == -1
    for kw in (dict(T=0), dict(S=0), dict(n=0), dict(d=0), dict(m=-1), dict(alpha=-1.0),
               dict(methods=(ctypes.c_int32 * 3)(0, 5, 1)), dict(eps=(ctypes.c_double * 3)(0.3, 1.5, 0.3))):
        assert stream(**kw) == -2, kw
    for kw in (dict(S=9), dict(n=4097), dict(m=4097), dict(d=129)):
        assert stream(**kw) == -5, kw
    for k in ("X", "hist", "weights"):
        assert stream(**{k: p + 4}) == -3, k
    for k in ("rows", "orders", "counts", "info"):
        assert stream(**{k: p + 2}) == -3, k


def test_interface_matches_reference_names():
    """online-learning/main.py:45, :61, :84 and what its loop (:288-339) asks of a classifier"""
    from rlvi_amd import online
    assert list(inspect.signature(online.update_weights_rlvi).parameters) == ["losses", "tol", "maxiter"]
    assert list(inspect.signature(online.update_weights_rrm).parameters) == ["residuals", "eps"]
    assert list(inspect.signature(online.cross_entropy).parameters) == ["log_proba", "targets"]
    sig = inspect.signature(online.SGDClassifier)
    assert list(sig.parameters) == ["loss", "random_state", "alpha"]
    assert sig.parameters["alpha"].default == 1e-4
    clf = online.SGDClassifier(loss='log_loss', random_state=1)
    assert not hasattr(clf, "classes_")                             # main.py:269-270
    assert list(inspect.signature(clf.partial_fit).parameters) == ["X", "y", "classes", "sample_weight"]
    assert list(inspect.signature(clf.partial_fit_weighted).parameters) == ["X", "y", "method", "eps", "X_test", "y_test"]
    for name in ("decision_function", "predict", "predict_log_proba", "score"):
        assert callable(getattr(clf, name))
    sig = inspect.signature(online.run_stream)
    assert list(sig.parameters)[:6] == ["X_train", "y_train", "X_test", "y_test", "methods", "eps"]
    assert sig.parameters["methods"].default == ('SGD', 'RRM', 'RLVI') and sig.parameters["eps"].default == 0.3
    for bad in (dict(loss='hinge'), dict(random_state=0), dict(alpha=0.0)):
        with pytest.raises(ValueError):
            online.SGDClassifier(**bad)
    with pytest.raises(ValueError, match="classes must be passed"):
        clf.partial_fit(np.zeros((2, 2)), [0, 1])


def test_flags_raise_what_scikit_learn_raises():
    from rlvi_amd import _lib, online, ops
    online._raise_flags(np.array([3, 0, 7, 0], np.int32), "x")      # no flag: nothing
    with pytest.raises(ValueError, match="Floating-point under-/overflow occurred at epoch #1"):
        online._raise_flags(np.array([0, 0, 0, 1], np.int32), "x")
    with pytest.raises(ValueError, match="x: no sample weights"):
        online._raise_flags(np.array([0, 0, 0, 2], np.int32), "x")
    with pytest.raises(_lib.RlviError, match="200 evaluations"):
        online._raise_flags(np.array([0, 0, 0, 3], np.int32), "x")
    with pytest.raises(ValueError, match="out of range"):
        online._raise_flags(np.array([0, 0, 0, 4], np.int32), "x")
    info = np.zeros((2, 3, 4), np.int32)
    info[1, 2, 3] = 1
    with pytest.raises(ValueError, match=r"epoch #1.*\(classifier, batch \(1, 2\)\)"):
        online._raise_flags(info, "run_stream")
    assert sorted(ops.ONLINE_FLAGS) == [1, 2, 3, 4] and ops.ONLINE_METHODS == R.METHODS


def test_partial_fit_raises_for_the_non_finite_flag(monkeypatch):
    """SGDClassifier.partial_fit around a launch that reports flag 1: ValueError, and the classifier stays unfitted.
    Seams: the device, the staging buffers, the launch and the host wait."""
    import torch
    from rlvi_amd import online, ops, standard
    seen = {}

    class Stage:
        def get(self, dev, tag, sizes, dtype=torch.float64, device_side=False):
            bufs = [torch.zeros(s, dtype=dtype) for s in sizes]
            return (*bufs, *[torch.zeros(s, dtype=dtype) for s in sizes])

    class Stream:
        def synchronize(self):
            pass

    def fake_step(X, y, state, **kw):
        seen.update(kw, n=X.shape[0])
        state[:] = float("nan")
        kw["info"][:] = torch.tensor([0, 0, X.shape[0], 1], dtype=torch.int32)

    monkeypatch.setattr(online, "_dev", lambda: torch.device("cpu"))
    monkeypatch.setattr(online, "_order_on", lambda dev, n: torch.from_numpy(online.sgd_order(n)))
    monkeypatch.setattr(standard, "_STAGE", Stage())
    monkeypatch.setattr(ops, "online_step", fake_step)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: Stream())
    clf = online.SGDClassifier()
    with pytest.raises(ValueError, match="Floating-point under-/overflow"):
        clf.partial_fit(np.ones((5, 2)), [0, 1, 0, 1, 1], classes=[0, 1])
    assert seen["n"] == 5 and seen["first"] and seen["method"] == "SGD" and not hasattr(clf, "classes_")
    assert list(clf.last_info_) == [0, 0, 5, 1]
