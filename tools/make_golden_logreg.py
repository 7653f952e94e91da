#!/usr/bin/env python3
"""Generate tests/golden/g15_logreg.npz by running the REFERENCE's logistic_regression (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_logreg.py [--ref /root/reference]

G15 logreg  logistic_regression, utils.sklearn_log_reg   standard-learning/rlvi.py:92-108, utils.py:61-73

The reference is imported read-only, as oracle/make_golden.py does.  rlvi.logistic_regression runs with
utils.sklearn_log_reg wrapped at run time, so that every liblinear fit leaves the weights that went in and the theta
that came out.  Cases:
  * the reference's own generator (main.py:88-123, its function compiled from the reference's file at run time and
    handed a seeded numpy Generator) at n = 17, 64, 100, 200 and eps = 0.1, 0.3;
  * Gaussian designs of this tool at 1000 x 20, 1025 x 23 and 4096 x 30 (entries exactly representable in fp16 and
    stored so: the fixture stays small; tests widen them to fp64), labels from a logistic model with a tenth flipped.
Per case: X, y, seed, theta, outer, the discrepancy trace, and per fit the weights (as update_weights returned them)
and liblinear's theta.
A seed is kept only if tests/logreg_ref.py -- the float64 restatement of the device algorithm -- takes the
reference's outer count on it (where the discrepancy hovers at tol, liblinear's slack decides, and no exact solver
can follow); tried / kept counts go into the file, and more than 10 % rejected is an error.  Running it again writes
the same bytes.
"""
import argparse
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import make_golden as MG  # noqa: E402
import logreg_ref  # noqa: E402

GEN_CASES = [(n, eps) for n in (17, 64, 100, 200) for eps in (0.1, 0.3)]
GAUSS_CASES = [(1000, 20), (1025, 23), (4096, 30)]
MAX_TRIES = 8


def reference_generator(ref):
    """generate_data_logistic_regression of the reference's main.py as a function of (random_gen, size, eps): the
    function's definition alone is compiled from the file (importing main.py draws in plotting and three other
    estimators' dependencies and creates a directory)."""
    path = os.path.join(ref, "standard-learning", "main.py")
    tree = ast.parse(open(path).read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "generate_data_logistic_regression"]
    ns = {"np": np}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)

    def gen(seed, size, eps):
        ns["random_gen"] = np.random.default_rng(seed=seed)
        return ns["generate_data_logistic_regression"](size=size, eps=eps)
    return gen


def gauss_case(seed, n, d):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float16)
    Xw = X.astype(np.float64)
    beta = rng.standard_normal(d) / np.sqrt(d)
    p = 1 / (1 + np.exp(-(0.3 + 2 * Xw @ beta)))
    y = (rng.random(n) < p).astype(np.float64)
    flip = rng.choice(n, n // 10, replace=False)
    y[flip] = 1 - y[flip]
    return X, y


def run_reference(ref_rlvi, ref_utils, X, y):
    fits = []
    orig = ref_utils.sklearn_log_reg

    def spy(Xa, ya, weights, *a, **k):
        w_in = np.array(weights, np.float64, copy=True)          # (the reference divides them in place)
        theta, losses = orig(Xa, ya, weights, *a, **k)
        fits.append((w_in, np.array(theta, np.float64, copy=True)))
        return theta, losses
    ref_utils.sklearn_log_reg = spy
    try:
        theta = ref_rlvi.logistic_regression(X.copy(), y.copy())
    finally:
        ref_utils.sklearn_log_reg = orig
    return np.asarray(theta, np.float64), fits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.ref, "standard-learning"))
    import rlvi as ref_rlvi
    import utils as ref_utils
    gen = reference_generator(a.ref)
    out, keys = {}, []
    tried = kept = 0
    todo = [("gen", n, 2, eps) for (n, eps) in GEN_CASES] + [("gauss", n, d, 0.1) for (n, d) in GAUSS_CASES]
    for ci, (kind, n, d, eps) in enumerate(todo):
        for t in range(MAX_TRIES):
            seed = 1500 + 10 * ci + t
            tried += 1
            if kind == "gen":
                X, y = gen(seed, n, eps)
                Xs = np.asarray(X, np.float64)
            else:
                Xs, y = gauss_case(seed, n, d)
            Xw = Xs.astype(np.float64)
            if y.min() == y.max():
                print(f"{kind} n={n} eps={eps} seed={seed}: one class, next seed", flush=True)
                continue
            theta, fits = run_reference(ref_rlvi, ref_utils, Xw, y)
            outer = len(fits) - 1
            th_r, w_r, outer_r, trace_r = logreg_ref.logistic_regression(Xw, y)
            if outer_r != outer:
                print(f"{kind} n={n} eps={eps} seed={seed}: outer {outer} (reference) vs {outer_r}, next seed", flush=True)
                continue
            kept += 1
            break
        else:
            raise SystemExit(f"no seed kept for {kind} n={n} eps={eps}")
        thetas = np.stack([f[1] for f in fits])
        trace = np.array([np.linalg.norm(thetas[k] - thetas[k - 1]) / np.linalg.norm(thetas[k - 1])
                          for k in range(1, len(fits))])
        key = f"{kind}_{n}x{d}_eps{eps}"
        keys.append(key)
        out[key + "/X"] = Xs
        out[key + "/y"] = y
        out[key + "/seed"] = np.array(seed, np.int64)
        out[key + "/theta"] = theta
        out[key + "/outer"] = np.array(outer, np.int64)
        out[key + "/trace"] = trace
        out[key + "/fit_w"] = np.stack([f[0] for f in fits])
        out[key + "/fit_theta"] = thetas
        rel = np.linalg.norm(th_r - theta) / np.linalg.norm(theta)
        print(f"{key}: seed {seed}, outer {outer}, {len(fits)} fits, |theta_ref.py - theta| / |theta| = {rel:.2e}",
              flush=True)
    out["cases"] = np.array(keys)
    out["seeds_tried_kept"] = np.array([tried, kept], np.int64)
    print(f"seeds tried {tried}, kept {kept}")
    if tried - kept > 0.1 * tried:
        raise SystemExit("more than 10 % of the seeds were rejected")
    import sklearn
    out["v_sklearn"] = np.array(sklearn.__version__)
    MG.save_deterministic("g15_logreg", **out)


if __name__ == "__main__":
    main()
