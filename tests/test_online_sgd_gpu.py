"""The online path's mini-batch and stream on the device (online_sgd.hip): rlvi_online_step_f64 and
rlvi_online_stream_f64 against the numpy restatement tests/online_ref.py and against what scikit-learn and the
reference left in tests/golden/g21_online_sgd.npz.  Needs numpy, torch and the fixture only.

Bars (every test prints its figures before it asserts).  t_, the four counts, the iteration counts of the
RLVI rule: equal.  Coefficients and intercept: |delta| <= 32 x noise x max |coef| -- noise the distance between the
restatement with sequential and with 64-leaf tree dot products, measured per method on the CPU (the fixture's, or here
for the shapes the fixture does not hold), floored at 2^-52; 32 for the device's exp and division being a unit in the
last place or two from libm's at every step, which the summation proxy does not see.  Against the reference's RRM, which
stops at Brent's tolerance: 4 x the fixture's rrm_dev.  Weights: RLVI rtol 1e-9, RRM rtol 10 x w_bar of G18, atol 1e-300.
The batch forms are held to the bits of the single steps."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import online_ref as R  # noqa: E402
from test_online_sgd_cpu import K_NOISE, STREAMS, W_BAR, check_against_fixture, load_stream, restated  # noqa: E402

pytestmark = pytest.mark.gpu
_DEVICE = {}


@pytest.fixture(scope="module")
def dev():
    from rlvi_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def device_stream(dev, name, methods=None, nan_padding=False):
    """ops.online_stream on a fixture stream -> numpy (state_hist, counts, weights, info); the whole stream's result is
    computed once and shared"""
    from rlvi_amd import ops
    key = (name, None if methods is None else tuple(methods), nan_padding)
    if key in _DEVICE:
        return _DEVICE[key]
    g = load_stream(name)
    sel = list(range(len(g["methods"]))) if methods is None else list(methods)
    X, y, Xt, yt, orders = (g[k].copy() for k in ("X", "y", "Xt", "yt", "orders"))
    if nan_padding:
        for k, (nk, mk) in enumerate(g["rows"]):
            X[k, nk:], y[k, nk:], Xt[k, mk:], yt[k, mk:], orders[k, nk:] = np.nan, np.nan, np.nan, np.nan, 1 << 30
    T, n, _ = X.shape
    weights = None
    if g["given"] is not None:
        weights = to(dev, g["given"][sel])
    res = ops.online_stream(to(dev, X), to(dev, y), to(dev, Xt), to(dev, yt), methods=[int(g["methods"][s]) for s in sel],
                            eps=g["eps"], rows=to(dev, g["rows"]), orders=to(dev, orders), alpha=g["alpha"],
                            weights=weights)
    torch.cuda.synchronize()
    _DEVICE[key] = tuple(t.cpu().numpy() for t in res)
    return _DEVICE[key]


def check_against_restatement(name, hist, counts, weights, info, ref, noise, methods, rows):
    d = hist.shape[2] - 2
    for s, m in enumerate(methods):
        want = ref["state_hist"][s]
        scale = np.abs(want[:, :d + 1]).max(axis=1)
        dist = np.abs(hist[s][:, :d + 1] - want[:, :d + 1]).max(axis=1)
        print(f"device {name} method {m}: max |coef - online_ref| / max |coef| per batch "
              f"{np.array2string(dist / scale, precision=2)} (bar {K_NOISE * noise[s]:.2e}), info {info[s].tolist()}")
        assert not info[s][:, 3].any()
        assert np.array_equal(hist[s][:, d + 1], want[:, d + 1]) and np.array_equal(counts[s], ref["counts"][s])
        assert (dist <= K_NOISE * noise[s] * scale).all()
        if m == R.METHODS["RLVI"]:
            assert np.array_equal(info[s][:, 0], ref["iters"][s])
        for k in range(want.shape[0]):
            nk = rows[k, 0]
            rtol = {R.METHODS["RLVI"]: 1e-9, R.METHODS["RRM"]: 10 * W_BAR}.get(m, 0.0)
            np.testing.assert_allclose(weights[s, k, :nk], ref["weights"][s, k, :nk], rtol=rtol, atol=1e-300)


@pytest.mark.parametrize("name", STREAMS)
def test_stream_against_the_restatement_and_the_fixture(dev, name):
    g = load_stream(name)
    hist, counts, weights, info = device_stream(dev, name)
    check_against_restatement(name, hist, counts, weights, info, restated(name, tree=True), g["noise"], g["methods"],
                              g["rows"])
    check_against_fixture(name, hist, counts, weights, "device")


@pytest.mark.parametrize("name", ["har", "small", "boundary", "two_col", "one_row", "given", "alpha1"])
def test_stream_has_the_bits_of_the_single_steps(dev, name):
    """T x S calls of ops.online_step, the state carried from call to call, against the one launch"""
    from rlvi_amd import ops
    g = load_stream(name)
    hist, counts, weights, info = device_stream(dev, name)
    T, n, d = g["X"].shape
    for s, m in enumerate(g["methods"]):
        state = torch.full((d + 2,), float("nan"), dtype=torch.float64, device=dev)
        for k in range(T):
            nk, mk = (int(v) for v in g["rows"][k])
            sw = to(dev, g["given"][s, k, :nk]) if g["given"] is not None else None
            _, sw, c, inf = ops.online_step(to(dev, g["X"][k, :nk]), to(dev, g["y"][k, :nk]), state, method=int(m),
                                            eps=g["eps"], first=k == 0, order=to(dev, g["orders"][k, :nk]),
                                            X_test=to(dev, g["Xt"][k, :mk]), y_test=to(dev, g["yt"][k, :mk]),
                                            alpha=g["alpha"], sample_weight=sw)
            assert np.array_equal(state.cpu().numpy(), hist[s, k]), (name, m, k)
            assert np.array_equal(c.cpu().numpy(), counts[s, k]) and np.array_equal(inf.cpu().numpy(), info[s, k])
            assert np.array_equal(sw.cpu().numpy(), weights[s, k, :nk])


@pytest.mark.parametrize("name", ["har", "boundary"])
def test_three_classifiers_in_one_launch_have_the_bits_of_three_launches(dev, name):
    whole = device_stream(dev, name)
    for s in range(3):
        one = device_stream(dev, name, methods=[s])
        for a, b in zip(whole, one):
            assert np.array_equal(a[s], b[0])


def test_padded_rows_do_not_matter(dev):
    """rows beyond (n_t, m_t) filled with NaN, the orders' padding with an index far out of range: the same bits"""
    for a, b in zip(device_stream(dev, "har"), device_stream(dev, "har", nan_padding=True)):
        assert np.array_equal(a, b)
    assert np.isfinite(device_stream(dev, "har")[0]).all()


def test_first_ignores_the_state_and_is_the_unfitted_classifier(dev):
    """first: whatever the state holds (NaN here) it is the unfitted classifier, coef 0, intercept 0, t 1 -- for plain
    SGD the same bits as a step from that state spelled out; RLVI's first residuals are log 2 for every row whatever X
    holds, so its weights are those of the fixture's first batch (1 / n each)."""
    from rlvi_amd import ops
    g = load_stream("small")
    X, y, order = to(dev, g["X"][0]), to(dev, g["y"][0]), to(dev, g["orders"][0])
    n, d = g["X"].shape[1:]
    out = {}
    for tag, first, fill in (("nan", True, float("nan")), ("zero", True, 0.0), ("spelled", False, 0.0)):
        state = torch.full((d + 2,), fill, dtype=torch.float64, device=dev)
        if not first:
            state[d + 1] = 1.0
        ops.online_step(X, y, state, method="SGD", first=first, order=order)
        out[tag] = state.cpu().numpy()
    assert np.array_equal(out["nan"], out["zero"]) and np.array_equal(out["nan"], out["spelled"])
    state = torch.full((d + 2,), float("nan"), dtype=torch.float64, device=dev)
    _, w1, _, _ = ops.online_step(X, y, state, method="RLVI", first=True, order=order)
    _, w2, _, _ = ops.online_step(torch.full_like(X, float("nan")), y, state.clone(), method="RLVI", first=True,
                                  order=order)
    assert np.array_equal(w1.cpu().numpy(), w2.cpu().numpy())
    np.testing.assert_allclose(w1.cpu().numpy(), g["weights"][list(g["methods"]).index(1), 0], rtol=1e-11)


def _case(seed, n, m, d, scale=1.0):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(d) / np.sqrt(d)
    X, Xt = rng.standard_normal((n, d)), rng.standard_normal((m, d))
    y = (X @ u + 0.3 * rng.standard_normal(n) > 0).astype(np.float64)
    return scale * X, y, scale * Xt, (Xt @ u > 0).astype(np.float64), 0.5 * rng.standard_normal(d), 0.1


# (n, m, d, method, alpha, t): the widest and longest batch; the sizes at which a thread's sample count changes (256 /
# 257 is the fixture's boundary stream, 1024 / 1025 here); a fitted state at t = 1 under alpha = 2, where the first
# shrink factor is 0 and the wscale fold zeroes coefficients that are not zero
STEP_CASES = [(4096, 4096, 128, "RLVI", 1e-4, 5000.0), (1024, 3, 7, "RRM", 1e-4, 300.0), (1025, 3, 7, "RLVI", 1e-4, 300.0),
              (33, 9, 70, "SGD", 2.0, 1.0)]


@pytest.mark.parametrize("n,m,d,method,alpha,t0", STEP_CASES, ids=lambda v: str(v))
def test_step_from_a_fitted_state_against_the_restatement(dev, n, m, d, method, alpha, t0):
    from rlvi_amd import ops
    X, y, Xt, yt, coef, b = _case(n + d, n, m, d)
    if method != "SGD":
        coef = coef / np.sqrt(d)
    order = R.sgd_order(n)
    code = R.METHODS[method]
    counters = {}
    ref = {tree: R.step(X, y, code, (coef, b, t0), False, 0.3, None, Xt, yt, order, alpha, tree=tree, counters=counters)
           for tree in (False, True)}
    scale = max(np.abs(ref[True]["state"][0]).max(), abs(ref[True]["state"][1]))
    delta = np.concatenate([ref[True]["state"][0] - ref[False]["state"][0], [ref[True]["state"][1] - ref[False]["state"][1]]])
    noise = max(np.abs(delta).max() / scale, 2.0 ** -52)
    state = to(dev, R.pack_state((coef, b, t0)))
    _, sw, counts, info = ops.online_step(to(dev, X), to(dev, y), state, method=method, eps=0.3, order=to(dev, order),
                                          X_test=to(dev, Xt), y_test=to(dev, yt), alpha=alpha)
    got = state.cpu().numpy()
    want = R.pack_state(ref[True]["state"])
    dist = np.abs(got[:d + 1] - want[:d + 1]).max() / scale
    print(f"step {n} x {d} {method} alpha {alpha}: |coef - online_ref| / max |coef| = {dist:.2e} (noise {noise:.2e}, "
          f"bar {K_NOISE * noise:.2e}), info {info.tolist()}, counters {counters}")
    assert info[3] == 0 and got[d + 1] == t0 + n
    assert np.array_equal(counts.cpu().numpy(), ref[True]["counts"])
    assert dist <= K_NOISE * noise
    if alpha == 2.0:
        assert counters["reset"] == 2 and np.abs(got[:d]).max() < np.abs(coef).max()
    if method == "RLVI":
        assert int(info[0]) == ref[True]["iters"]
    rtol = {"RLVI": 1e-9, "RRM": 10 * W_BAR}.get(method, 0.0)
    np.testing.assert_allclose(sw.cpu().numpy(), ref[True]["sample_weight"], rtol=rtol, atol=1e-300)


def test_flags(dev):
    """an order index out of range and RRM on one row: nothing read, no pass, the state as it was; a NaN feature:
    flag 1 with the state written as it is"""
    from rlvi_amd import ops
    X, y, Xt, yt, coef, b = _case(3, 20, 4, 5)
    state0 = R.pack_state((coef, b, 7.0))
    order = R.sgd_order(20)
    bad = order.copy()
    bad[11] = 20
    state = to(dev, state0)
    _, _, counts, info = ops.online_step(to(dev, X), to(dev, y), state, order=to(dev, bad), X_test=to(dev, Xt),
                                         y_test=to(dev, yt))
    assert info.tolist()[3] == 4 and np.array_equal(state.cpu().numpy(), state0) and counts.tolist() == [0, 0, 0, 0]
    state = to(dev, state0)
    _, _, counts, info = ops.online_step(to(dev, X[:1]), to(dev, y[:1]), state, method="RRM", eps=0.3, X_test=to(dev, Xt),
                                         y_test=to(dev, yt))
    assert info.tolist()[3] == 2 and np.array_equal(state.cpu().numpy(), state0)
    assert np.array_equal(counts.cpu().numpy(), R.counts(Xt, yt, coef, b, tree=True)[0])
    Xn = X.copy()
    Xn[3, 2] = np.nan
    state = to(dev, state0)
    _, _, _, info = ops.online_step(to(dev, Xn), to(dev, y), state, order=to(dev, order))
    assert info.tolist()[3] == 1 and np.isnan(state.cpu().numpy()[:5]).any()


def test_mirror_runs_the_references_loop(dev):
    """rlvi_amd.online.SGDClassifier in the loop of main.py:288-339 (partial_fit with the weights of the module's own
    rules, predict, score) and run_stream, on the fixture's small stream: the fixture's states and counts"""
    from rlvi_amd import online
    g = load_stream("small")
    T = g["X"].shape[0]
    names = {0: "SGD", 1: "RLVI", 2: "RRM"}
    Xs, ys = [g["X"][k, :g["rows"][k, 0]] for k in range(T)], [g["y"][k, :g["rows"][k, 0]] for k in range(T)]
    Xts, yts = [g["Xt"][k, :g["rows"][k, 1]] for k in range(T)], [g["yt"][k, :g["rows"][k, 1]] for k in range(T)]
    res = online.run_stream(Xs, ys, Xts, yts, methods=[names[int(m)] for m in g["methods"]], eps=g["eps"])
    hist, counts, _, _ = device_stream(dev, "small")
    for s, m in enumerate(g["methods"]):
        r = res[names[int(m)]]
        assert np.array_equal(r["coef_history"], hist[s, :, :3]) and np.array_equal(r["counts"], counts[s])
        tp, tn, fp, fn = (counts[s, :, j].astype(float) for j in range(4))
        assert np.array_equal(r["f1"], tp / (tp + (fp + fn) / 2.0)) and np.array_equal(r["acc"], (tp + tn) / 5.0)
    s = list(g["methods"]).index(1)
    clf = online.SGDClassifier(loss='log_loss', random_state=1)
    for k in range(T):
        if not hasattr(clf, "classes_"):
            log_proba = np.log(0.5 * np.ones_like(ys[k]))
        else:
            log_proba = clf.predict_log_proba(Xs[k])[:, 1]
        sample_weight = online.update_weights_rlvi(online.cross_entropy(log_proba, ys[k]))
        clf.partial_fit(Xs[k], ys[k], classes=[0, 1], sample_weight=sample_weight)
        y_pred = clf.predict(Xts[k])
        tp = np.count_nonzero(np.logical_and(y_pred == 1, yts[k] == 1))
        assert tp == g["counts"][s, k, 0] and clf.t_ == g["state_hist"][s, k, 4]
        assert clf.score(Xts[k], yts[k]) == (g["counts"][s, k, 0] + g["counts"][s, k, 1]) / 5.0
        np.testing.assert_allclose(clf.coef_[0], g["state_hist"][s, k, :3], rtol=1e-8)
    fused = online.SGDClassifier()
    for k in range(T):
        _, c = fused.partial_fit_weighted(Xs[k], ys[k], "RLVI", X_test=Xts[k], y_test=yts[k])
        assert np.array_equal(np.concatenate([fused.coef_[0], fused.intercept_, [fused.t_]]), hist[s, k])
        assert np.array_equal(c, counts[s, k])
