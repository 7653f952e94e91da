#!/usr/bin/env python3
"""Generate tests/golden/g16_moments.npz by running the REFERENCE's mean, pca and covariance (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_moments.py [--ref /root/reference]

G16 moments  mean, pca, covariance, update_weights_constrained   standard-learning/rlvi.py:23-65, :111-144,
                                                                 utils.py:76-108

The reference is imported read-only, as oracle/make_golden.py does.  Its estimators run with rlvi.update_weights,
rlvi.update_weights_constrained, utils.pca and utils.covariance wrapped at run time, so that every outer iteration
leaves its theta and every constrained E-step the losses that went in, the weights that came out and whether the
constraint was active.  Cases:
  * the reference's own generators (main.py:44-66, :126-167, their functions compiled from the reference's file at run
    time and handed a seeded numpy Generator): mean at n = 17, 100, 257 and eps = 0.2, 0.4; pca at n = 17, 40, 200, each
    with theta_init=None and with the reference's (0.1, 1) / ||.|| (main.py:487-488); covariance at n = 17, 50, 200
    with the estimator's eps = 0.4;
  * contaminated Gaussian clouds of this tool at 1024 x 4, 2048 x 8 and 4096 x 4 (column c of standard deviation
    2^(-c/2) about c / 2, a fifth of the rows' deviations divided by sqrt(chi2_1.5 / 1.5); entries exactly
    representable in fp16 and stored so: the fixture stays small, tests widen them to fp64), through all three.
Per case: sample, seed, theta, outer, the discrepancy trace; for covariance every E-step.
A seed is kept only if tests/moments_ref.py -- the float64 restatement of the device algorithm -- takes the
reference's outer count on it; tried / kept counts go into the file, and more than 10 % rejected is an error.
Running it again writes the same bytes.
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
import moments_ref  # noqa: E402

MEAN_CASES = [(n, eps) for n in (17, 100, 257) for eps in (0.2, 0.4)]
PCA_CASES = [(n, init) for n in (17, 40, 200) for init in (False, True)]
COV_CASES = [17, 50, 200]
CLOUDS = [(1024, 4), (2048, 8), (4096, 4)]
COV_EPS = 0.4
MAX_TRIES = 8


def reference_generators(ref):
    """generate_data_mean / _pca / _cov of the reference's main.py as functions of (seed, size, eps): the functions'
    definitions alone are compiled from the file (importing main.py draws in plotting and creates a directory)."""
    path = os.path.join(ref, "standard-learning", "main.py")
    tree = ast.parse(open(path).read(), path)
    names = ("generate_data_mean", "generate_data_pca", "generate_data_cov")
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    ns = {"np": np}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)

    def gen(name, seed, **kw):
        ns["random_gen"] = np.random.default_rng(seed=seed)
        return np.asarray(ns["generate_data_" + name](**kw), np.float64)
    return gen


def theta_init():
    t = np.array([0.1, 1])                    # main.py:487-488
    t /= np.linalg.norm(t)
    return t


def cloud(seed, n, d):
    rng = np.random.default_rng(seed)
    dev = rng.standard_normal((n, d)) * 2.0 ** (-0.5 * np.arange(d))
    k = n // 5
    dev[:k] /= np.sqrt(rng.chisquare(1.5, k) / 1.5)[:, None]
    return np.clip(dev + 0.5 * np.arange(d), -6e4, 6e4).astype(np.float16)


def run_reference(ref_rlvi, ref_utils, kind, x, init):
    """-> (theta, thetas of the outer iterations incl. the first fit, E-steps [(losses, weights, active)])."""
    thetas, esteps, plain = [], [], []
    o_uw, o_uwc, o_pca, o_cov = (ref_rlvi.update_weights, ref_rlvi.update_weights_constrained, ref_utils.pca,
                                 ref_utils.covariance)

    def uw(losses, *a, **k):
        w = o_uw(losses, *a, **k)
        plain.append(np.array(w, np.float64, copy=True))
        if kind == "mean":
            thetas.append(w @ x / np.sum(w))             # rlvi.py:56, the reference's own statement
        return w

    def uwc(losses, n_eff, *a, **k):
        l_in = np.array(losses, np.float64, copy=True)
        w = o_uwc(losses, n_eff, *a, **k)
        esteps.append((l_in, np.array(w, np.float64, copy=True), bool(np.sum(plain[-1]) < n_eff)))
        return w

    def spy_pca(*a, **k):
        theta, losses = o_pca(*a, **k)
        thetas.append(np.array(theta, np.float64, copy=True))
        return theta, losses

    def spy_cov(*a, **k):
        theta, losses = o_cov(*a, **k)
        thetas.append(np.array(theta, np.float64, copy=True))
        return theta, losses
    ref_rlvi.update_weights, ref_rlvi.update_weights_constrained = uw, uwc
    ref_utils.pca, ref_utils.covariance = spy_pca, spy_cov
    try:
        if kind == "mean":
            thetas.append(np.ones(len(x)) @ x / len(x))  # rlvi.py:47-48
            theta = ref_rlvi.mean(x.copy())
        elif kind == "pca":
            theta = ref_rlvi.pca(x.copy(), theta_init=None if init is None else init.copy())
        else:
            theta = ref_rlvi.covariance(x.copy(), eps=COV_EPS)
    finally:
        ref_rlvi.update_weights, ref_rlvi.update_weights_constrained = o_uw, o_uwc
        ref_utils.pca, ref_utils.covariance = o_pca, o_cov
    return np.asarray(theta, np.float64), thetas, esteps


def restatement(kind, x, init):
    if kind == "mean":
        return moments_ref.mean(x)
    if kind == "pca":
        return moments_ref.pca(x, theta_init=init)
    return moments_ref.covariance(x, COV_EPS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.ref, "standard-learning"))
    import rlvi as ref_rlvi
    import utils as ref_utils
    gen = reference_generators(a.ref)
    todo = [("mean", "gen", n, 2, eps, None) for (n, eps) in MEAN_CASES]
    todo += [("pca", "gen", n, 2, 0.2, theta_init() if init else None) for (n, init) in PCA_CASES]
    todo += [("cov", "gen", n, 2, 0.2, None) for n in COV_CASES]
    todo += [(kind, "cloud", n, d, 0.2, None) for (n, d) in CLOUDS for kind in ("mean", "pca", "cov")]
    out, keys = {}, []
    tried = kept = 0
    for ci, (kind, src, n, d, eps, init) in enumerate(todo):
        for t in range(MAX_TRIES):
            seed = 1600 + 10 * ci + t
            tried += 1
            if src == "gen":
                xs = gen(kind, seed, size=n, eps=eps)
            else:
                xs = cloud(seed, n, d)
            x = xs.astype(np.float64)
            theta, thetas, esteps = run_reference(ref_rlvi, ref_utils, kind, x, init)
            outer = len(thetas) - 1
            th_r, w_r, outer_r, trace_r = restatement(kind, x, init)
            if outer_r != outer:
                print(f"{kind} {src} n={n}: seed {seed}: outer {outer} (reference) vs {outer_r}, next seed", flush=True)
                continue
            kept += 1
            break
        else:
            raise SystemExit(f"no seed kept for {kind} {src} n={n}")
        trace = np.array([np.linalg.norm(thetas[k] - thetas[k - 1]) / np.linalg.norm(thetas[k - 1])
                          for k in range(1, len(thetas))])
        key = f"{kind}_{src}_{n}x{d}" + (f"_eps{eps}" if kind == "mean" and src == "gen" else "") + (
            "_init" if init is not None else "")
        keys.append(key)
        out[key + "/sample"] = xs
        out[key + "/seed"] = np.array(seed, np.int64)
        out[key + "/theta"] = theta
        out[key + "/outer"] = np.array(outer, np.int64)
        out[key + "/trace"] = trace
        if init is not None:
            out[key + "/theta_init"] = init
        if kind == "cov":
            out[key + "/estep_losses"] = np.stack([e[0] for e in esteps])
            out[key + "/estep_w"] = np.stack([e[1] for e in esteps])
            out[key + "/estep_active"] = np.array([e[2] for e in esteps], np.int8)
        rel = np.linalg.norm(th_r - theta) / np.linalg.norm(theta)
        print(f"{key}: seed {seed}, outer {outer}, |theta_ref.py - theta| / |theta| = {rel:.2e}"
              + (f", constraint active in {sum(e[2] for e in esteps)} of {len(esteps)}" if kind == "cov" else ""),
              flush=True)
    out["cases"] = np.array(keys)
    out["cov_eps"] = np.array(COV_EPS)
    out["seeds_tried_kept"] = np.array([tried, kept], np.int64)
    print(f"seeds tried {tried}, kept {kept}")
    if tried - kept > 0.1 * tried:
        raise SystemExit("more than 10 % of the seeds were rejected")
    MG.save_deterministic("g16_moments", **out)


if __name__ == "__main__":
    main()
