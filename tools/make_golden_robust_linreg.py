#!/usr/bin/env python3
"""Generate tests/golden/g19_robust_linreg.npz by running the REFERENCE's RRM and Huber linear regressions (build
container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_robust_linreg.py [--ref /root/reference]

G19 robust linreg   rrm.linear_regression, huber.linear_regression   standard-learning/rrm.py:55-73, huber.py:13-40

The reference is imported read-only, as tools/make_golden_rrm.py does.  Designs, one per shape, each run through four
estimators -- RRM at eps = 0.2 and 0.4, Huber at its defaults (c = 0.7317, sigma0 = 1) and at sigma0 = 0.1:
  * the reference's generator (main.py:69-85 with nu = 2.5 as main.py:262 calls it, contamination 0.2; synth.linreg_data
    is that recipe at any size x d, the reference's own has ten columns) at 17 x 3, 40 x 10 and 257 x 20;
  * Gaussian designs (X ~ N(0, 1), the same responses) at 1000 x 20 and 1025 x 31.
X and y are rounded to float32 and stored so (half the bytes; every estimator, the reference included, sees those values).
Per design: X, y, seed.  Per run: theta (the reference's), the iteration count and, for RRM up to 257 x 20, the losses
into and the weights out of every update_weights call of the reference.
A seed is kept only if tests/robust_linreg_ref.py -- the float64 restatement of the device algorithms -- takes the
reference's iteration count in all four runs and every one of its stop decisions is clear of the edge: RRM
|discrepancy - tol| >= 1e-6, Huber |discrepancy / 1e-6 - 1| >= 1e-3; and if the reference's floor of 1e-16 under every phi
moved none of RRM's sums (|sum w - 1| <= 1e-9 in every E-step: the rule of G18).  The rules are a run's: the counts
that go into the file are runs examined / runs that passed (a design is dropped with its first failing run, the runs
before it count as passed; `runs_examined_passed`), and more than 10 % of them rejected is an error.  This is LOOSER than
a rule on seeds: five designs are six draws at the first rejection, and one draw in six is already 17 % -- a 10 % rule
on so few seeds admits no rejection at all, while a run lands inside Huber's margin about once in a hundred
(profiles/r23_robust_linreg.md).  `theta_bar_rrm`, `theta_bar_huber`: the largest relative distance ||theta_restatement - theta_reference|| / ||theta_reference|| measured; `w_bar`: the same for the weights of
the stored E-steps (weights above 1e-300), as in G18.  Running it again writes the same bytes.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import make_golden as MG  # noqa: E402
from rlvi_amd import synth  # noqa: E402
import robust_linreg_ref as R  # noqa: E402
import rrm_ref  # noqa: E402

GEN_SHAPES = ((17, 3), (40, 10), (257, 20))
GAUSS_SHAPES = ((1000, 20), (1025, 31))
RRM_EPS = (0.2, 0.4)
HUBER_SIGMA0 = (1.0, 0.1)
STEPS_UP_TO = 257 * 20
RRM_MARGIN = 1e-6
HUBER_MARGIN = 1e-3
FLOOR_MOVED = 1e-9
MAX_TRIES = 8


def design(kind, seed, n, d):
    if kind == "gen":
        X, y = synth.linreg_data(n, d, eps=0.2, nu=2.5, seed=seed)
    else:
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((n, d))
        n2 = rng.binomial(n=n, p=0.2)
        n1 = n - n2
        y1 = X[:n1] @ np.ones(d) + 0.25 * rng.normal(size=n1)
        u = rng.chisquare(df=2.5, size=n2) / 2.5
        y2 = X[n1:] @ np.ones(d) + rng.normal(size=n2) / np.sqrt(u)
        y = np.concatenate([y1, y2])
    return X.astype(np.float32), y.astype(np.float32)


def run_reference_rrm(ref_rrm, X, y, eps):
    esteps = []
    orig = ref_rrm.update_weights

    def spy(losses, eps_):
        l_in = np.array(losses, np.float64, copy=True)
        w = orig(losses, eps_)
        esteps.append((l_in, np.array(w, np.float64, copy=True)))
        return w
    ref_rrm.update_weights = spy
    try:
        theta = ref_rrm.linear_regression(X.copy(), y.copy(), eps)
    finally:
        ref_rrm.update_weights = orig
    return np.asarray(theta, np.float64), esteps


def run_reference_huber(ref_huber, X, y, sigma0):
    calls = []
    orig = ref_huber.lstsq

    def spy(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    ref_huber.lstsq = spy                        # (one call per iteration: huber.py:30)
    try:
        theta = ref_huber.linear_regression(X.copy(), y.copy(), sigma0=sigma0)
    finally:
        ref_huber.lstsq = orig
    return np.asarray(theta, np.float64), len(calls)


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.ref, "standard-learning"))
    import huber as ref_huber
    import rrm as ref_rrm
    out, keys = {}, []
    examined = passed = 0
    bar = {"rrm": 0.0, "huber": 0.0}
    w_bar = 0.0
    todo = [("gen", n, d) for n, d in GEN_SHAPES] + [("gauss", n, d) for n, d in GAUSS_SHAPES]
    for ci, (kind, n, d) in enumerate(todo):
        for t in range(MAX_TRIES):
            seed = 1900 + 10 * ci + t
            Xs, ys = design(kind, seed, n, d)
            X, y = Xs.astype(np.float64), ys.astype(np.float64)
            runs, why = {}, None
            for eps in RRM_EPS:
                examined += 1
                th_r, _, outer_r, trace = R.rrm_linear_regression(X, y, eps)
                if R.rrm_margin(trace) < RRM_MARGIN:
                    why = f"rrm eps={eps}: margin {R.rrm_margin(trace):.1e}"
                    break
                theta, esteps = run_reference_rrm(ref_rrm, X, y, eps)
                if len(esteps) != outer_r:
                    why = f"rrm eps={eps}: outer {len(esteps)} (reference) vs {outer_r}"
                    break
                floored = max(abs(float(np.sum(w)) - 1.0) for _, w in esteps)
                if floored > FLOOR_MOVED:
                    why = f"rrm eps={eps}: the reference's floor moved a sum (|sum w - 1| = {floored:.1e})"
                    break
                runs[f"rrm_eps{eps}"] = (theta, outer_r, th_r, R.rrm_margin(trace), esteps)
            for s0 in HUBER_SIGMA0 if why is None else ():
                examined += 1
                th_r, _, it_r, trace = R.huber_linear_regression(X, y, sigma0=s0)
                if R.huber_margin(trace) < HUBER_MARGIN:
                    why = f"huber sigma0={s0}: margin {R.huber_margin(trace):.1e}"
                    break
                theta, it = run_reference_huber(ref_huber, X, y, s0)
                if it != it_r:
                    why = f"huber sigma0={s0}: {it} iterations (reference) vs {it_r}"
                    break
                runs[f"huber_sigma{s0}"] = (theta, it_r, th_r, R.huber_margin(trace), None)
            if why is not None:
                print(f"{kind} {n}x{d}: seed {seed}: {why}, next seed", flush=True)
                passed += len(runs)
                continue
            passed += len(runs)
            break
        else:
            raise SystemExit(f"no seed kept for {kind} {n}x{d}")
        key = f"{kind}_{n}x{d}"
        keys.append(key)
        out[key + "/X"] = Xs
        out[key + "/y"] = ys
        out[key + "/seed"] = np.array(seed, np.int64)
        for run, (theta, count, th_r, margin, esteps) in runs.items():
            est = run.split("_")[0]
            out[f"{key}/{run}/theta"] = theta
            out[f"{key}/{run}/count"] = np.array(count, np.int64)
            dist = rel(th_r, theta)
            bar[est] = max(bar[est], dist)
            wd = 0.0
            if esteps is not None and n * d <= STEPS_UP_TO:
                out[f"{key}/{run}/estep_losses"] = np.stack([e[0] for e in esteps])
                out[f"{key}/{run}/estep_w"] = np.stack([e[1] for e in esteps])
                eps = float(run[len("rrm_eps"):])
                for l_in, w_ref in esteps:
                    big = w_ref > 1e-300
                    w = rrm_ref.update_weights(l_in, eps)[0]
                    wd = max(wd, float(np.max(np.abs(w[big] - w_ref[big]) / w_ref[big])))
                w_bar = max(w_bar, wd)
            print(f"{key} {run}: seed {seed}, count {count}, margin {margin:.1e}, |theta_ref.py - theta| / |theta| = "
                  f"{dist:.2e}, weights {wd:.2e}", flush=True)
    out["cases"] = np.array(keys)
    out["runs"] = np.array([f"rrm_eps{e}" for e in RRM_EPS] + [f"huber_sigma{s}" for s in HUBER_SIGMA0])
    out["theta_bar_rrm"] = np.array(bar["rrm"])
    out["theta_bar_huber"] = np.array(bar["huber"])
    out["w_bar"] = np.array(w_bar)
    out["runs_examined_passed"] = np.array([examined, passed], np.int64)
    print(f"runs examined {examined}, passed {passed}; theta_bar rrm {bar['rrm']:.3e}, huber {bar['huber']:.3e}, w_bar {w_bar:.3e}")
    if examined - passed > 0.1 * examined:
        raise SystemExit("more than 10 % of the runs were rejected")
    MG.save_deterministic("g19_robust_linreg", **out)


if __name__ == "__main__":
    main()
