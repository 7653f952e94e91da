#!/usr/bin/env python3
"""Generate tests/golden/g20_rrm_logreg.npz by running the REFERENCE's rrm.logistic_regression (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_rrm_logreg.py [--ref /root/reference]

G20 rrm logreg   rrm.logistic_regression   standard-learning/rrm.py:76-91 on utils.py:61-73

The reference is imported read-only, as tools/make_golden_logreg.py does, with rrm.update_weights and
utils.sklearn_log_reg wrapped at run time: every rule call leaves the losses that went in and the weights that came
out, every liblinear fit its theta.  Designs, each run at the eps values beside it:
  * the reference's own generator (main.py:88-123, compiled from the reference's file as G15's tool does) at n = 17, 64,
    100, 200 and contamination 0.05 and 0.3, eps = 0.3 and 0.4;
  * the Gaussian designs of G15's tool (gauss_case: fp16-exact entries, stored as fp16) at 1000 x 20 and 1025 x 23,
    eps = 0.3 and 0.4, and at 4096 x 30, eps = 0.4.
Per design: X, y, seed.  Per run: theta (the reference's), the outer count, the discrepancy trace of the reference and,
up to n = 200, the losses into and the weights out of every update_weights call.
A run is kept only if tests/robust_logreg_ref.py -- the float64 restatement of the device algorithm -- takes the
reference's outer count (where a discrepancy hovers at tol, liblinear's 1e-4 slack decides, and no exact solver can
follow), if every stop decision of the restatement is clear of the edge (margin = min |disc / tol - 1| >= 1e-4: the
device is held to 1e-8 of the restatement) and if the reference's floor of 1e-16 under every phi moved none of the
rule's sums (|sum w - 1| <= 1e-9 in every call: the rule of G18).  A design is dropped with its first failing run and
the next seed is drawn; the runs before it count as passed.  `runs_examined_passed` holds the counts, and more than
10 % rejected is an error.  The design at n = 17, contamination 0.3 must give a run that goes the full 100 iterations
at eps = 0.3 (the reference's limit cycle: about one seed in three): seeds that do not are passed over before anything
is examined (`seeds_passed_over`).
`theta_bar`: the largest ||theta_restatement - theta_reference|| / ||theta_reference|| over the kept runs (liblinear's
tolerance); `w_bar`: the largest relative distance of rrm_ref.update_weights from the stored weights (above 1e-300) on
the stored losses.  Both are measured here, never typed in.  Running it again writes the same bytes.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import make_golden as MG  # noqa: E402
from make_golden_logreg import gauss_case, reference_generator  # noqa: E402
import robust_logreg_ref as R  # noqa: E402
import rrm_ref  # noqa: E402

GEN_DESIGNS = [(n, c) for n in (17, 64, 100, 200) for c in (0.05, 0.3)]
GAUSS_DESIGNS = [((1000, 20), (0.3, 0.4)), ((1025, 23), (0.3, 0.4)), ((4096, 30), (0.4,))]
GEN_EPS = (0.3, 0.4)
FULL = (17, 0.3, 0.3)                 # (n, contamination, eps) of the run that must go all 100 iterations
STEPS_UP_TO = 200
TOL = 1e-2
MARGIN = 1e-4
FLOOR_MOVED = 1e-9
MAX_TRIES = 40


def run_reference(ref_rrm, ref_utils, X, y, eps):
    esteps, thetas = [], []
    orig_w, orig_fit = ref_rrm.update_weights, ref_utils.sklearn_log_reg

    def spy_w(losses, eps_):
        l_in = np.array(losses, np.float64, copy=True)
        w = orig_w(losses, eps_)
        esteps.append((l_in, np.array(w, np.float64, copy=True)))
        return w

    def spy_fit(*a, **k):
        theta, losses = orig_fit(*a, **k)
        thetas.append(np.array(theta, np.float64, copy=True))
        return theta, losses
    ref_rrm.update_weights, ref_utils.sklearn_log_reg = spy_w, spy_fit
    try:
        theta = ref_rrm.logistic_regression(X.copy(), y.copy(), eps)
    finally:
        ref_rrm.update_weights, ref_utils.sklearn_log_reg = orig_w, orig_fit
    trace = np.array([np.linalg.norm(thetas[k] - thetas[k - 1]) / np.linalg.norm(thetas[k - 1])
                      for k in range(1, len(thetas))])
    return np.asarray(theta, np.float64), esteps, trace


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.ref, "standard-learning"))
    import rrm as ref_rrm
    import utils as ref_utils
    gen = reference_generator(a.ref)
    out, keys, run_keys = {}, [], []
    examined = passed = passed_over = 0
    theta_bar = w_bar = 0.0
    todo = [("gen", n, 2, c, GEN_EPS) for n, c in GEN_DESIGNS] + [("gauss", n, d, 0.0, e) for (n, d), e in GAUSS_DESIGNS]
    for ci, (kind, n, d, contam, eps_values) in enumerate(todo):
        for t in range(MAX_TRIES):
            seed = 2000 + 100 * ci + t
            if kind == "gen":
                X, y = gen(seed, n, contam)
                Xs = np.asarray(X, np.float64)
            else:
                Xs, y = gauss_case(seed, n, d)
            y = np.asarray(y, np.float64)
            Xw = Xs.astype(np.float64)
            if y.min() == y.max():
                print(f"{kind} {n}x{d} c={contam} seed={seed}: one class, next seed", flush=True)
                continue
            if (n, contam) == FULL[:2]:
                # (a choice of design, made on the restatement before anything is examined: no rejection)
                if R.rrm_logistic_regression(Xw, y, FULL[2], tol=TOL)[2] != 100:
                    passed_over += 1
                    continue
            runs, why = {}, None
            for eps in eps_values:
                examined += 1
                steps_r = []
                th_r, _, outer_r, trace_r = R.rrm_logistic_regression(Xw, y, eps, tol=TOL, steps=steps_r)
                theta, esteps, trace = run_reference(ref_rrm, ref_utils, Xw, y, eps)
                if len(esteps) != outer_r:
                    why = f"eps={eps}: outer {len(esteps)} (reference) vs {outer_r}"
                    break
                if R.margin(trace_r, TOL) < MARGIN:
                    why = f"eps={eps}: margin {R.margin(trace_r, TOL):.1e}"
                    break
                floored = max(abs(float(np.sum(w)) - 1.0) for _, w in esteps)
                if floored > FLOOR_MOVED:
                    why = f"eps={eps}: the reference's floor moved a sum (|sum w - 1| = {floored:.1e})"
                    break
                runs[f"eps{eps}"] = (theta, outer_r, trace, th_r, R.margin(trace_r, TOL), esteps)
            passed += len(runs)
            if why is not None:
                print(f"{kind} {n}x{d} c={contam} seed={seed}: {why}, next seed", flush=True)
                continue
            break
        else:
            raise SystemExit(f"no seed kept for {kind} {n}x{d} c={contam}")
        key = f"{kind}_{n}x{d}_c{contam}"
        keys.append(key)
        out[key + "/X"] = Xs
        out[key + "/y"] = y
        out[key + "/seed"] = np.array(seed, np.int64)
        for run, (theta, count, trace, th_r, margin, esteps) in runs.items():
            run_keys.append(f"{key}/{run}")
            out[f"{key}/{run}/theta"] = theta
            out[f"{key}/{run}/count"] = np.array(count, np.int64)
            out[f"{key}/{run}/trace"] = trace
            dist = rel(th_r, theta)
            theta_bar = max(theta_bar, dist)
            wd = 0.0
            if n <= STEPS_UP_TO:
                out[f"{key}/{run}/estep_losses"] = np.stack([e[0] for e in esteps])
                out[f"{key}/{run}/estep_w"] = np.stack([e[1] for e in esteps])
                eps = float(run[len("eps"):])
                for l_in, w_ref in esteps:
                    big = w_ref > 1e-300
                    w = rrm_ref.update_weights(l_in, eps)[0]
                    wd = max(wd, float(np.max(np.abs(w[big] - w_ref[big]) / w_ref[big])))
                w_bar = max(w_bar, wd)
            print(f"{key} {run}: seed {seed}, count {count}, margin {margin:.1e}, |theta_ref.py - theta| / |theta| = "
                  f"{dist:.2e}, weights {wd:.2e}", flush=True)
    if not any(int(out[k + "/count"]) == 100 for k in run_keys):
        raise SystemExit("no kept run goes the full 100 iterations")
    out["cases"] = np.array(keys)
    out["runs"] = np.array(run_keys)
    out["theta_bar"] = np.array(theta_bar)
    out["w_bar"] = np.array(w_bar)
    out["runs_examined_passed"] = np.array([examined, passed], np.int64)
    out["seeds_passed_over"] = np.array(passed_over, np.int64)
    print(f"runs examined {examined}, passed {passed}; seeds passed over for the full-length run {passed_over}; "
          f"theta_bar {theta_bar:.3e}, w_bar {w_bar:.3e}")
    if examined - passed > 0.1 * examined:
        raise SystemExit("more than 10 % of the runs were rejected")
    import sklearn
    out["v_sklearn"] = np.array(sklearn.__version__)
    MG.save_deterministic("g20_rrm_logreg", **out)


if __name__ == "__main__":
    main()
