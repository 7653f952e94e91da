#!/usr/bin/env python3
"""Generate tests/golden/g18_rrm.npz by running the REFERENCE's Robust Risk Minimization estimators (build container
only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_rrm.py [--ref /root/reference]

G18 rrm  update_weights, mean, pca, covariance   standard-learning/rrm.py:12-52, :94-124, utils.py:76-108

The reference is imported read-only, as tools/make_golden_moments.py does (whose generators and theta_init are
used here).  Its estimators run with rrm.update_weights wrapped at run time, so that every call leaves the losses that
went in and the weights that came out.  Cases, each at the estimator's eps = 0.2 and 0.4:
  * the reference's own generators (main.py:44-66, :126-167) at their own sizes and one odd size each: mean at
    n = 17, 100, 257; pca at n = 17, 200 and at n = 40 with the reference's theta_init (main.py:487-488); covariance at
    n = 17, 50, 129;
  * contaminated clouds (column c of standard deviation 2^(-c/2) about 1 + c / 2, a fifth of the rows' deviations
    divided by sqrt(chi2_1.5 / 1.5); entries representable in fp16 and stored so) at 512 x 4 with every E-step, and at
    2048 x 8 and 4096 x 4 (eps = 0.2 only) WITHOUT their E-steps: one 4096-sample run's losses and weights are
    incompressible float64 and as large as the rest of the file, which is kept no larger than g16_moments.npz.  A cloud
    whose reference run takes longer than SLOW_S seconds (its np.diag(weights) is n x n) is stored with the
    restatement's theta and outer count instead and marked in `restatement_only`.
Per case: sample, seed, theta_init where used, theta, outer, eps; estep_losses / estep_w [outer, n] where stored.
A seed is kept only if tests/rrm_ref.py -- the float64 restatement of the device algorithm -- takes the reference's
outer count on it and every one of its stop decisions has a margin |discrepancy - tol| >= 1e-6 -- and if the
reference's floor of 1e-16 under every phi moved none of its sums.  The reference does NOT shift the losses by their
minimum: where min l / alpha > 36.8 (a covariance's first E-step, whose losses carry 1/2 log det of a wide first fit)
EVERY phi is under the floor, its objective is alpha (log(n 1e-16) + t) and what Brent returns minimises that, not g.
Its weights, exp(-l / alpha) over the FLOORED sum, then no longer sum to 1: a seed with |sum w - 1| > 1e-9 in any E-step
is rejected.  Tried / kept counts go into the file, and more than 10 % rejected is an error.  `w_bar`: the largest
relative distance between the restatement's and the reference's weights over all stored E-steps (weights above 1e-300)
-- what Brent's tolerance on xi, times l / alpha, leaves.  Running it again writes the same bytes.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import make_golden as MG  # noqa: E402
import make_golden_moments as MGM  # noqa: E402
import rrm_ref  # noqa: E402

EPS = (0.2, 0.4)
DATA_EPS = 0.2                               # the generators' contamination
MEAN_N = (17, 100, 257)
PCA_N = ((17, False), (200, False), (40, True))
COV_N = (17, 50, 129)
CLOUD_STEPS = (512, 4)                       # the cloud stored with its E-steps
CLOUDS_LARGE = ((2048, 8), (4096, 4))        # theta and outer only
TOLS = {"mean": 1e-3, "pca": 1e-2, "cov": 1e-2}
MARGIN = 1e-6
FLOOR_MOVED = 1e-9
MAX_TRIES = 8
SLOW_S = 120.0


def cloud(seed, n, d):
    """make_golden_moments.cloud about 1 + c / 2 instead of c / 2.  Brent's tolerance on xi leaves the reference's own
    mean some 1e-10 (absolute, on a cloud of unit spread) off the minimiser's; the mean's bar, rtol 1e-9 elementwise,
    measures that against nothing on a coordinate whose true mean is 0, as column 0 of that cloud has it."""
    rng = np.random.default_rng(seed)
    dev = rng.standard_normal((n, d)) * 2.0 ** (-0.5 * np.arange(d))
    k = n // 5
    dev[:k] /= np.sqrt(rng.chisquare(1.5, k) / 1.5)[:, None]
    return np.clip(dev + 1.0 + 0.5 * np.arange(d), -6e4, 6e4).astype(np.float16)


def run_reference(ref_rrm, kind, x, eps, init):
    """-> (theta, E-steps [(losses, weights)])"""
    esteps = []
    orig = ref_rrm.update_weights

    def spy(losses, eps_):
        l_in = np.array(losses, np.float64, copy=True)
        w = orig(losses, eps_)
        esteps.append((l_in, np.array(w, np.float64, copy=True)))
        return w
    ref_rrm.update_weights = spy
    try:
        if kind == "mean":
            theta = ref_rrm.mean(x.copy(), eps)
        elif kind == "pca":
            theta = ref_rrm.pca(x.copy(), eps, theta_init=None if init is None else init.copy())
        else:
            theta = ref_rrm.covariance(x.copy(), eps)
    finally:
        ref_rrm.update_weights = orig
    return np.asarray(theta, np.float64), esteps


def restatement(kind, x, eps, init):
    if kind == "mean":
        return rrm_ref.mean(x, eps)
    if kind == "pca":
        return rrm_ref.pca(x, eps, theta_init=init)
    return rrm_ref.covariance(x, eps)


def rel_weight_distance(w, w_ref):
    big = w_ref > 1e-300
    return float(np.max(np.abs(w[big] - w_ref[big]) / w_ref[big]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.ref, "standard-learning"))
    import rrm as ref_rrm
    gen = MGM.reference_generators(a.ref)
    todo = [("mean", "gen", n, 2, eps, None, True) for n in MEAN_N for eps in EPS]
    todo += [("pca", "gen", n, 2, eps, MGM.theta_init() if init else None, True) for (n, init) in PCA_N for eps in EPS]
    todo += [("cov", "gen", n, 2, eps, None, True) for n in COV_N for eps in EPS]
    todo += [(kind, "cloud", *CLOUD_STEPS, eps, None, True) for kind in ("mean", "pca", "cov") for eps in EPS]
    todo += [(kind, "cloud", n, d, 0.2, None, False) for (n, d) in CLOUDS_LARGE for kind in ("mean", "pca", "cov")]
    out, keys, only = {}, [], []
    tried = kept = 0
    w_bar = 0.0
    for ci, (kind, src, n, d, eps, init, with_steps) in enumerate(todo):
        for t in range(MAX_TRIES):
            seed = 1800 + 10 * ci + t
            tried += 1
            xs = gen(kind, seed, size=n, eps=DATA_EPS) if src == "gen" else cloud(seed, n, d)
            x = xs.astype(np.float64)
            th_r, w_r, outer_r, trace_r = restatement(kind, x, eps, init)
            margin = float(np.min(np.abs(trace_r - TOLS[kind]))) if len(trace_r) else np.inf
            if margin < MARGIN:
                print(f"{kind} {src} n={n} eps={eps}: seed {seed}: margin {margin:.1e}, next seed", flush=True)
                continue
            t0 = time.time()
            theta, esteps = run_reference(ref_rrm, kind, x, eps, init)
            took = time.time() - t0
            outer = len(esteps)
            slow = src == "cloud" and not with_steps and took > SLOW_S
            if outer_r != outer:
                print(f"{kind} {src} n={n} eps={eps}: seed {seed}: outer {outer} (reference) vs {outer_r}, next seed",
                      flush=True)
                continue
            floored = max(abs(float(np.sum(w)) - 1.0) for _, w in esteps)
            if floored > FLOOR_MOVED:
                print(f"{kind} {src} n={n} eps={eps}: seed {seed}: the reference's floor moved a sum (|sum w - 1| = "
                      f"{floored:.1e}), next seed", flush=True)
                continue
            kept += 1
            break
        else:
            raise SystemExit(f"no seed kept for {kind} {src} n={n} eps={eps}")
        key = f"{kind}_{src}_{n}x{d}_eps{eps}" + ("_init" if init is not None else "")
        keys.append(key)
        only.append(1 if slow else 0)
        out[key + "/sample"] = xs
        out[key + "/seed"] = np.array(seed, np.int64)
        out[key + "/eps"] = np.array(eps)
        out[key + "/theta"] = th_r if slow else theta
        out[key + "/outer"] = np.array(outer, np.int64)
        if init is not None:
            out[key + "/theta_init"] = init
        dist = 0.0
        if with_steps:
            out[key + "/estep_losses"] = np.stack([e[0] for e in esteps])
            out[key + "/estep_w"] = np.stack([e[1] for e in esteps])
            for l_in, w_ref in esteps:
                dist = max(dist, rel_weight_distance(rrm_ref.update_weights(l_in, eps)[0], w_ref))
            w_bar = max(w_bar, dist)
        rel = np.linalg.norm(th_r - theta) / np.linalg.norm(theta)
        print(f"{key}: seed {seed}, outer {outer}, margin {margin:.1e}, |theta_ref.py - theta| / |theta| = {rel:.2e}, "
              f"weights {dist:.2e}, reference {took:.1f} s" + (" (restatement only)" if slow else ""), flush=True)
    out["cases"] = np.array(keys)
    out["restatement_only"] = np.array(only, np.int8)
    out["w_bar"] = np.array(w_bar)
    out["seeds_tried_kept"] = np.array([tried, kept], np.int64)
    print(f"seeds tried {tried}, kept {kept}, rejected {tried - kept}; w_bar {w_bar:.3e}")
    if tried - kept > 0.1 * tried:
        raise SystemExit("more than 10 % of the seeds were rejected")
    MG.save_deterministic("g18_rrm", **out)


if __name__ == "__main__":
    main()
