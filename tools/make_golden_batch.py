#!/usr/bin/env python3
"""Generate tests/golden/g17_sweep.npz by running the REFERENCE's five estimators over miniatures of its own
Monte-Carlo sweeps (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_batch.py [--ref /root/reference]

G17 sweep  the loops of standard-learning/main.py:170-572 around rlvi.py's mean, linear_regression,
           logistic_regression, pca and covariance -- what the *_batch entries run as one launch each

The reference is imported read-only, as oracle/make_golden.py does; its generators are compiled from main.py at run
time and handed a seeded numpy Generator, as tools/make_golden_moments.py does.  Only arrays are written.
  linear_regression    4 corruption levels (0, 0.13, 0.27, 0.4) x 8 runs at 40 x 10, nu = 2.5      main.py:261-273
  mean                 the same 4 x 8 at 100 x 2                                                   main.py:180-188
  logistic_regression  16 runs at 200 x 2, eps 0.05                                                main.py:431-437
  pca                  16 runs at 40 x 2, eps 0.2, the reference's theta_init (0.1, 1) / ||.||     main.py:489-494
  covariance           16 runs at 50 x 2, eps 0.2 in the data, 0.4 in the call                     main.py:539-544
Per estimator: the stacked inputs (X [B, n, d], y [B, n] / sample [B, n, d]), the reference's theta per problem, its
outer iteration counts, the seeds and (the first two) the corruption level of every problem.
A seed is kept only if the float64 restatement of the device algorithm (oracle.rlvi_oracle.linear_regression,
tests/logreg_ref.py, tests/moments_ref.py) takes the reference's outer count on it; tried / kept counts go into the
file, and more than 10 % rejected is an error.  Running it again writes the same bytes.
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
from oracle import rlvi_oracle  # noqa: E402
import logreg_ref  # noqa: E402
import moments_ref  # noqa: E402

LEVELS = (0.0, 0.13, 0.27, 0.4)
RUNS_PER_LEVEL = 8
RUNS = 16
COV_EPS = 0.4
MAX_TRIES = 8
# (kind, generator, its keywords, the problems' corruption levels)
SWEEPS = [
    ("linreg", "linear_regression", dict(size=40, nu=2.5), [e for e in LEVELS for _ in range(RUNS_PER_LEVEL)]),
    ("mean", "mean", dict(size=100), [e for e in LEVELS for _ in range(RUNS_PER_LEVEL)]),
    ("logreg", "logistic_regression", dict(size=200), [0.05] * RUNS),
    ("pca", "pca", dict(size=40), [0.2] * RUNS),
    ("cov", "cov", dict(size=50), [0.2] * RUNS),
]


def reference_generators(ref):
    """The generate_data_* functions of the reference's main.py as functions of (seed, keywords): the functions'
    definitions alone are compiled from the file (importing main.py draws in plotting and creates a directory)."""
    path = os.path.join(ref, "standard-learning", "main.py")
    tree = ast.parse(open(path).read(), path)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("generate_data_")]
    ns = {"np": np}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)

    def gen(name, seed, **kw):
        ns["random_gen"] = np.random.default_rng(seed=seed)
        return ns["generate_data_" + name](**kw)
    return gen


def theta_init():
    t = np.array([0.1, 1])                    # main.py:487-488
    t /= np.linalg.norm(t)
    return t


def run_reference(ref_rlvi, kind, data):
    """-> (theta, outer): the reference's estimator with its E-step counted (one call per outer iteration)."""
    name = "update_weights_constrained" if kind == "cov" else "update_weights"
    orig = getattr(ref_rlvi, name)
    calls = []

    def spy(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    setattr(ref_rlvi, name, spy)
    try:
        if kind == "linreg":
            theta = ref_rlvi.linear_regression(data[0].copy(), data[1].copy())
        elif kind == "logreg":
            theta = ref_rlvi.logistic_regression(data[0].copy(), data[1].copy())
        elif kind == "mean":
            theta = ref_rlvi.mean(data[0].copy())
        elif kind == "pca":
            theta = ref_rlvi.pca(data[0].copy(), theta_init=theta_init())
        else:
            theta = ref_rlvi.covariance(data[0].copy(), eps=COV_EPS)
    finally:
        setattr(ref_rlvi, name, orig)
    return np.asarray(theta, np.float64), len(calls)


def restatement_outer(kind, data):
    if kind == "linreg":
        return rlvi_oracle.linear_regression(data[0], data[1], trace=True)[2]
    if kind == "logreg":
        return logreg_ref.logistic_regression(data[0], data[1])[2]
    if kind == "mean":
        return moments_ref.mean(data[0])[2]
    if kind == "pca":
        return moments_ref.pca(data[0], theta_init=theta_init())[2]
    return moments_ref.covariance(data[0], COV_EPS)[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.ref, "standard-learning"))
    import rlvi as ref_rlvi
    gen = reference_generators(a.ref)
    out = {}
    tried = kept = 0
    for si, (kind, gname, kw, levels) in enumerate(SWEEPS):
        arrays, thetas, outers, seeds = [], [], [], []
        for pi, eps in enumerate(levels):
            for t in range(MAX_TRIES):
                seed = 17000 + 1000 * si + 10 * pi + t
                tried += 1
                data = gen(gname, seed, eps=eps, **kw)
                data = tuple(np.asarray(x, np.float64) for x in (data if isinstance(data, tuple) else (data,)))
                if kind == "logreg" and data[1].min() == data[1].max():
                    print(f"{kind} problem {pi} seed {seed}: one class, next seed", flush=True)
                    continue
                theta, outer = run_reference(ref_rlvi, kind, data)
                outer_r = restatement_outer(kind, data)
                if outer_r != outer:
                    print(f"{kind} problem {pi} seed {seed}: outer {outer} (reference) vs {outer_r}, next seed",
                          flush=True)
                    continue
                kept += 1
                break
            else:
                raise SystemExit(f"no seed kept for {kind} problem {pi}")
            arrays.append(data)
            thetas.append(theta)
            outers.append(outer)
            seeds.append(seed)
        out[kind + ("/X" if len(arrays[0]) == 2 else "/sample")] = np.stack([d[0] for d in arrays])
        if len(arrays[0]) == 2:
            out[kind + "/y"] = np.stack([d[1] for d in arrays])
        out[kind + "/theta"] = np.stack(thetas)
        out[kind + "/outer"] = np.array(outers, np.int64)
        out[kind + "/seed"] = np.array(seeds, np.int64)
        out[kind + "/eps"] = np.array(levels, np.float64)
        print(f"{kind}: {len(levels)} problems, outer counts {sorted(set(outers))}", flush=True)
    out["pca/theta_init"] = theta_init()
    out["cov_eps"] = np.array(COV_EPS)
    out["seeds_tried_kept"] = np.array([tried, kept], np.int64)
    print(f"seeds tried {tried}, kept {kept}")
    if tried - kept > 0.1 * tried:
        raise SystemExit("more than 10 % of the seeds were rejected")
    MG.save_deterministic("g17_sweep", **out)


if __name__ == "__main__":
    main()
