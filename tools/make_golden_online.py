#!/usr/bin/env python3
"""Generate tests/golden/g21_online_sgd.npz by running the REFERENCE's online loop on scikit-learn (build container
only, CPU only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_online.py [--ref /root/reference] [--profile FILE]

G21 online sgd   main() of online-learning/main.py:277-339 (update_weights_rlvi :45-58, update_weights_rrm :61-81,
                 cross_entropy :84-85, sklearn's SGDClassifier.partial_fit / predict) on synthetic streams

The reference is imported read-only as oracle/make_golden.py's gen_g6 does (a synthetic humanactivity.mat
in a temporary directory, MPLBACKEND=Agg).  Its main() runs as it is written: iter_minibatches is replaced by an
iterator over a synthetic stream, the plot functions by nothing, and partial_fit_classifiers by recording subclasses of
sklearn's SGDClassifier -- every partial_fit leaves the sample weights that went in and the state that came out, every
predict the decision values.  The supplied-weights stream, which main() has no branch for, calls partial_fit directly.

Streams (T batches of n train and m test rows by d columns; inputs stored as fp16 or fp32, which they are exact in):
    har         6 x 100 / 100 x 60   SGD, RRM, RLVI   per-batch standard scaler, 30 % of the positive labels flipped,
                                                      the last batch 38 / 37 rows
    small       6 x 17 / 5 x 3       SGD, RRM, RLVI
    boundary    4 x 257 / 64 x 64    SGD, RRM, RLVI   two samples per thread begin, every lane holds one column
    two_col     3 x 40 / 8 x 65      SGD, RRM, RLVI   the first column that is a lane's second
    widest      3 x 40 / 8 x 128     SGD, RRM, RLVI
    one_col     4 x 30 / 6 x 1       SGD, RRM, RLVI
    one_row     5 x 1 / 2 x 4        SGD, RLVI        (RRM's rule needs (1 - eps) n > 1)
    two_rows    5 x 2 / 2 x 4        SGD, RRM, RLVI
    given       4 x 50 / 10 x 8      GIVEN            random weights, a third of them exact zeros
    scaled      4 x 60 / 12 x 6      SGD              features times 25: the tail of the loss (p <= -37) occurs (both
                                                      weight rules of the reference return NaN on such residuals)
    alpha1      4 x 40 / 8 x 5       SGD, RLVI        alpha = 1: the first sample's shrink factor is 0, the wscale fold
                                                      (coefficients near 0, residuals all but equal: Brent's search
                                                      and the exact root part there, RRM is left out)
Per stream: the inputs, rows = (n_t, m_t), the orders, and for every (method, batch) the sample weights, the state
(coef, intercept, t_), the counts (tp, tn, fp, fn) and the smallest |decision value| of a test row.  Measured here, never
typed in:
    noise [S]    max over the batches of |coef(online_ref, sequential dot) - coef(online_ref, 64-leaf tree dot)| /
                 max |coef|, floored at 2^-52; the GPU tests hold the device to 32 x noise x max |coef|.  With d <= 3
                 the tree IS the sequential sum and the distance is 0 however the recurrence amplifies a rounding
                 (plain SGD's early steps, eta about 10, do by orders of magnitude): there the second run moves every
                 dot product up by one unit in the last place (online_ref's tree="ulp")
    ref_dist [S] the same distance between online_ref (sequential) and scikit-learn
    rrm_dev      RRM: the distance of online_ref (exact root) from the reference (Brent's search) after T batches, over
                 max |coef|; the tests allow 4 x that
    rrm_w        RRM: the largest relative distance of the weights (above 1e-300) from the reference's
The tool asserts: every branch counter of online_ref.sgd_pass that the log loss can reach is non-zero somewhere (the
tail, a zero update, the wscale fold; the clip at 1e12 is beyond a gradient that is at most 1 and must count 0), no
test row of any batch has |decision| < 1e-6 under scikit-learn, t_ equal, counts equal.  Running it again writes the same bytes.
"""
import argparse
import os
import sys
import tempfile
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import make_golden as MG  # noqa: E402
import online_ref as R  # noqa: E402

EPS = 0.3                       # main.py:307
ALL = ("SGD", "RRM", "RLVI")
#          name       T  n    m    d    methods           kwargs
STREAMS = [("har", 6, 100, 100, 60, ALL, dict(store="f4", last=(38, 37), scaler=True)),
           ("small", 6, 17, 5, 3, ALL, {}),
           ("boundary", 4, 257, 64, 64, ALL, {}),
           ("two_col", 3, 40, 8, 65, ALL, {}),
           ("widest", 3, 40, 8, 128, ALL, {}),
           ("one_col", 4, 30, 6, 1, ALL, {}),
           ("one_row", 5, 1, 2, 4, ("SGD", "RLVI"), {}),
           ("two_rows", 5, 2, 2, 4, ALL, {}),
           ("given", 4, 50, 10, 8, ("GIVEN",), {}),
           ("scaled", 4, 60, 12, 6, ("SGD",), dict(scale=25.0)),
           ("alpha1", 4, 40, 8, 5, ("SGD", "RLVI"), dict(alpha=1.0))]


def make_stream(seed, T, n, m, d, store="f2", last=None, scaler=False, scale=1.0, **_):
    """Two Gaussian classes 3 apart along a fixed direction; 30 % of the positive train labels flipped to 0
    (main.py:258-265 at noise_rate 0.3).  Padded to [T, n, ...]; rows beyond (n_t, m_t) are zero."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(d)
    u /= np.linalg.norm(u)
    X, y, Xt, yt = np.zeros((T, n, d)), np.zeros((T, n)), np.zeros((T, m, d)), np.zeros((T, m))
    rows = np.zeros((T, 2), np.int32)
    for k in range(T):
        nk, mk = last if (last and k == T - 1) else (n, m)
        lab = (rng.random(nk + mk) < 0.5).astype(np.float64)
        lab[:2] = 1.0, 0.0                                           # (main.py:321, :326 divide by the test rows of a class)
        Z = rng.standard_normal((nk + mk, d)) + 3.0 * np.outer(lab - 0.5, u) + 0.5
        if scaler:                                                   # main.py:254-256, on the train rows
            mu, sd = Z[mk:].mean(axis=0), Z[mk:].std(axis=0)
            Z = (Z - mu) / sd
        Z = (scale * Z).astype(np.float16 if store == "f2" else np.float32).astype(np.float64)
        ytr = lab[mk:].copy()
        pos = np.flatnonzero(ytr == 1)
        ytr[rng.choice(pos, size=int(0.3 * len(pos)), replace=False)] = 0
        Xt[k, :mk], yt[k, :mk], X[k, :nk], y[k, :nk] = Z[:mk], lab[:mk], Z[mk:], ytr
        rows[k] = nk, mk
    return X, y, Xt, yt, rows


def import_reference(ref):
    import scipy.io
    tmp = tempfile.mkdtemp()
    rng = np.random.default_rng(0)
    scipy.io.savemat(os.path.join(tmp, "humanactivity.mat"),
                     {"feat": rng.standard_normal((400, 60)), "actid": rng.integers(1, 6, (400, 1))})
    cwd = os.getcwd()
    os.chdir(tmp)
    os.environ["MPLBACKEND"] = "Agg"
    sys.path.insert(0, os.path.join(ref, "online-learning"))
    try:
        import main as online
    finally:
        os.chdir(cwd)
    for name in ("plot_score_evolution", "plot_tp_evolution", "plot_tn_evolution", "plot_f1_evolution"):
        setattr(online, name, lambda *a, **k: None)
    return online


def spy_class():
    from sklearn.linear_model import SGDClassifier

    class Spy(SGDClassifier):
        """records what main()'s loop does with it (class attribute `log`: a list per instance name)"""

        def partial_fit(self, X, y, classes=None, sample_weight=None):
            out = super().partial_fit(X, y, classes=classes, sample_weight=sample_weight)
            self.log_.append(dict(sw=np.ones(len(y)) if sample_weight is None else np.array(sample_weight, np.float64),
                                  state=np.concatenate([self.coef_[0], self.intercept_, [self.t_]])))
            return out

        def predict(self, X):
            self.log_[-1]["decision"] = self.decision_function(X)
            return super().predict(X)
    return Spy


def run_reference(online, Spy, X, y, Xt, yt, rows, methods, alpha):
    """main() on the stream -> {method: list of per-batch records}"""
    T = X.shape[0]
    batches = [((X[k, :rows[k, 0]].copy(), y[k, :rows[k, 0]].astype(int)),
                (Xt[k, :rows[k, 1]].copy(), yt[k, :rows[k, 1]].astype(int))) for k in range(T)]
    clfs = {}
    for name in methods:
        clfs[name] = Spy(loss='log_loss', random_state=1, alpha=alpha)
        clfs[name].log_ = []
    online.partial_fit_classifiers = clfs
    online.iter_minibatches = lambda *a, **k: iter(batches)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        online.main()
    return {name: clf.log_ for name, clf in clfs.items()}


def run_given(Spy, X, y, Xt, yt, rows, given, alpha):
    clf = Spy(loss='log_loss', random_state=1, alpha=alpha)
    clf.log_ = []
    for k in range(X.shape[0]):
        nk, mk = rows[k]
        clf.partial_fit(X[k, :nk], y[k, :nk].astype(int), classes=[0, 1], sample_weight=given[0, k, :nk])
        clf.predict(Xt[k, :mk])
    return {"GIVEN": clf.log_}


def counts_of(decision, yt):
    pred = decision > 0
    return np.array([np.count_nonzero(pred & (yt == 1)), np.count_nonzero(~pred & (yt == 0)),
                     np.count_nonzero(pred & (yt == 0)), np.count_nonzero(~pred & (yt == 1))], np.int32)


def coef_dist(a, b, d):
    """max over the batches of |coef_a - coef_b| (the intercept with them) over max |coef_b|"""
    return float(np.max(np.abs(a[:, :d + 1] - b[:, :d + 1]).max(axis=1) / np.abs(b[:, :d + 1]).max(axis=1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--profile", help="append the measured values as a markdown table to this file")
    a = ap.parse_args()
    online = import_reference(a.ref)
    Spy = spy_class()
    out, names, lines = {}, [], []
    counters = {}
    for ci, (name, T, n, m, d, methods, kw) in enumerate(STREAMS):
        alpha = kw.get("alpha", 1e-4)
        X, y, Xt, yt, rows = make_stream(2100 + ci, T, n, m, d, **kw)
        codes = [R.METHODS[v] for v in methods]
        S = len(codes)
        given = None
        if methods == ("GIVEN",):
            rng = np.random.default_rng(77)
            given = rng.random((1, T, n)) / n
            given[rng.random((1, T, n)) < 1.0 / 3.0] = 0.0
            logs = run_given(Spy, X, y, Xt, yt, rows, given, alpha)
        else:
            logs = run_reference(online, Spy, X, y, Xt, yt, rows, methods, alpha)
        hist, weights = np.zeros((S, T, d + 2)), np.zeros((S, T, n))
        counts, dmin = np.zeros((S, T, 4), np.int32), np.inf
        for s, meth in enumerate(methods):
            for k, rec in enumerate(logs[meth]):
                hist[s, k] = rec["state"]
                weights[s, k, :rows[k, 0]] = rec["sw"]
                counts[s, k] = counts_of(rec["decision"], yt[k, :rows[k, 1]])
                dmin = min(dmin, float(np.min(np.abs(rec["decision"]))))
        assert dmin >= 1e-6, (name, dmin)
        seq = R.stream(X, y, Xt, yt, rows, codes, EPS, given, alpha, counters=counters)
        tree = R.stream(X, y, Xt, yt, rows, codes, EPS, given, alpha, tree=True)
        other = tree if d > 3 else R.stream(X, y, Xt, yt, rows, codes, EPS, given, alpha, tree="ulp")
        noise = np.array([max(coef_dist(other["state_hist"][s], seq["state_hist"][s], d), 2.0 ** -52) for s in range(S)])
        ref_dist = np.array([coef_dist(seq["state_hist"][s], hist[s], d) for s in range(S)])
        for s, meth in enumerate(methods):
            assert np.array_equal(seq["state_hist"][s, :, d + 1], hist[s, :, d + 1]), (name, meth, "t_")
            assert np.array_equal(seq["counts"][s], counts[s]) and np.array_equal(tree["counts"][s], counts[s]), \
                (name, meth, "counts")
            assert not seq["flags"][s].any()
        rrm_dev = rrm_w = 0.0
        if "RRM" in methods:
            s = methods.index("RRM")
            rrm_dev = ref_dist[s]
            big = weights[s] > 1e-300
            rrm_w = float(np.max(np.abs(seq["weights"][s][big] - weights[s][big]) / weights[s][big]))
        names.append(name)
        for key, val in dict(X=X.astype(np.float32 if kw.get("store") == "f4" else np.float16),
                             Xt=Xt.astype(np.float32 if kw.get("store") == "f4" else np.float16),
                             y=y.astype(np.int8), yt=yt.astype(np.int8), rows=rows,
                             orders=np.stack([np.pad(R.sgd_order(int(r)), (0, n - int(r))) for r in rows[:, 0]]),
                             methods=np.array(codes, np.int32), alpha=np.array(alpha), eps=np.array(EPS),
                             state_hist=hist, weights=weights, counts=counts, decision_min=np.array(dmin),
                             noise=noise, ref_dist=ref_dist, rrm_dev=np.array(rrm_dev), rrm_w=np.array(rrm_w)).items():
            out[f"{name}/{key}"] = val
        if given is not None:
            out[f"{name}/given"] = given
        line = (f"| {name} | {T} x {n} / {m} x {d} | {' '.join(methods)} | "
                f"{' '.join(f'{v:.1e}' for v in noise)} | {' '.join(f'{v:.1e}' for v in ref_dist)} | "
                f"{rrm_dev:.1e} | {rrm_w:.1e} | {dmin:.1e} |")
        lines.append(line)
        print(line, flush=True)
    print("branch counters:", counters)
    for c in ("tail", "zero_update", "reset"):
        assert counters.get(c, 0) > 0, f"the streams never take the branch {c}"
    assert counters.get("clip", 0) == 0          # |dloss| <= 1 for the log loss
    out["streams"] = np.array(names)
    out["counters"] = np.array([counters.get(c, 0) for c in R.COUNTERS], np.int64)
    out["order_sizes"] = np.array([1, 2, 3, 17, 38, 100, 257, 4096], np.int32)
    for k in out["order_sizes"]:
        out[f"order/{int(k)}"] = sklearn_order(int(k))
        assert np.array_equal(out[f"order/{int(k)}"], R.sgd_order(int(k))), k
    import scipy
    import sklearn
    out["v_sklearn"], out["v_numpy"], out["v_scipy"] = (np.array(sklearn.__version__), np.array(np.__version__),
                                                        np.array(scipy.__version__))
    MG.save_deterministic("g21_online_sgd", **out)
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", "g21_online_sgd.npz"))
    assert size < 1000 * 1000, size
    if a.profile:
        with open(a.profile, "a") as f:
            f.write("\n| stream | T x n / m x d | methods | noise | online_ref - scikit-learn | rrm_dev | rrm_w | "
                    "min abs decision |\n|---|---|---|---|---|---|---|---|\n" + "\n".join(lines) + "\n\n"
                    f"branch counters {counters}; fixture {size} bytes\n")


def sklearn_order(n):
    """the order scikit-learn itself visits n rows in: its dataset, shuffled with the seed partial_fit draws"""
    from sklearn.utils import check_random_state
    from sklearn.linear_model._base import make_dataset
    rs = check_random_state(1)
    X = np.arange(n, dtype=np.float64).reshape(n, 1)
    ds, _ = make_dataset(X, np.zeros(n), np.ones(n), random_state=rs)
    seed = rs.randint(0, np.iinfo(np.int32).max)
    ds._shuffle_py(seed)
    return np.array([int(ds._next_py()[3]) for _ in range(n)], np.int32)


if __name__ == "__main__":
    main()
