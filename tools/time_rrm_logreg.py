"""rrm.logistic_regression on one MI355X, numpy in and numpy out (every call ends in its one host wait): the one launch
against the same estimator as a host loop of the ops that existed before it (ops.rrm_update_weights + ops.logistic_fit,
one launch per statement of rrm.py:76-91 and one host decision per outer iteration), at 100 x 2, 200 x 2, 1000 x 20 and
4096 x 30; then a sweep of 100 problems of 200 x 2 (main.py:372-401 has 100 Monte-Carlo runs per point) as ONE batch launch
against 100 single calls.

    python tools/time_rrm_logreg.py [--reps 40] [--warm 5] [--out FILE]

The designs are those of tests/golden/g20_rrm_logreg.npz (the reference's generator at contamination 0.3, the Gaussian
designs); the sweep's problems are seeded bootstrap resamples of the fixture's two 200 x 2 designs -- the reference's
generator itself is not part of this repository.  The variants of a row are timed in turns, rep by rep, after a warm-up
of each; per row one JSON line with the median and the smallest wall-clock time per call in microseconds and the
iteration counts from `info`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EPS = 0.4                                   # main.py:382
MAXITER, TOL = 100, 1e-2
CASES = ("gen_100x2_c0.3", "gen_200x2_c0.3", "gauss_1000x20_c0.0", "gauss_4096x30_c0.0")
SWEEP = (100, ("gen_200x2_c0.05", "gen_200x2_c0.3"))


def in_turns(calls, reps, warm):
    """{name: (median us, min us)} of the calls, one of each per round"""
    for fn in calls.values():
        for _ in range(warm):
            fn()
    t = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            t[k].append(1e6 * (time.perf_counter() - t0))
    return {k: (round(float(np.median(v)), 1), round(float(np.min(v)), 1)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_rrm_logreg.py needs an MI355X: there is nothing to time without one")
    from rlvi_amd import ops, rrm
    dev = torch.device("cuda", torch.cuda.current_device())
    G20 = np.load(os.path.join(ROOT, "tests", "golden", "g20_rrm_logreg.npz"))
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def host_loop(X, y, ws):
        """rrm.py:76-91, one launch per statement; numpy in, numpy out.  Returns (theta, outer)."""
        n = X.shape[0]
        Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
        w = torch.full((n,), 1.0 / n, dtype=torch.float64, device=dev)
        theta, losses, _ = ops.logistic_fit(Xd, yd, w, ws=ws)
        outer = 0
        for _ in range(MAXITER):
            outer += 1
            w, _ = ops.rrm_update_weights(losses, EPS, ws=ws)
            prev = theta
            theta, losses, _ = ops.logistic_fit(Xd, yd, w, ws=ws)
            if bool(torch.linalg.norm(theta - prev) / torch.linalg.norm(prev) <= TOL):
                break
        return theta.cpu().numpy(), outer

    for key in CASES:
        X = np.ascontiguousarray(G20[key + "/X"], dtype=np.float64)
        y = G20[key + "/y"].astype(np.float64)
        n, d = X.shape
        ws = ops.workspace(dev, n, 0)
        theta, _, info = rrm.logistic_regression(X, y, EPS, return_info=True)
        th_loop, outer_loop = host_loop(X, y, ws)
        reps = a.reps if info[0] < 50 else max(5, a.reps // 4)
        t = in_turns({"one_launch": lambda: rrm.logistic_regression(X, y, EPS),
                      "host_loop": lambda: host_loop(X, y, ws)}, reps, a.warm)
        emit({"case": key, "n": n, "d": d, "us_median_min": t, "info": [int(v) for v in info],
              "host_loop_outer": outer_loop, "reps": reps,
              "host_loop_theta_distance": float(np.linalg.norm(th_loop - theta) / np.linalg.norm(theta))})

    B, keys = SWEEP
    rng = np.random.default_rng(24)
    Xs, ys = [], []
    while len(Xs) < B:
        key = keys[len(Xs) % len(keys)]
        X, y = np.asarray(G20[key + "/X"], np.float64), G20[key + "/y"].astype(np.float64)
        rows_ = rng.integers(0, X.shape[0], X.shape[0])
        if y[rows_].min() != y[rows_].max():
            Xs.append(X[rows_])
            ys.append(y[rows_])
    Xb, yb = np.ascontiguousarray(np.stack(Xs)), np.stack(ys)
    _, _, info = rrm.logistic_regression_batch(Xb, yb, EPS, return_info=True)

    def singles():
        for b in range(B):
            if info[b, 3] == 0:
                rrm.logistic_regression(Xb[b], yb[b], EPS)
    # (a flagged problem is reported in `flags` below, not raised in the middle of the timing)
    t = in_turns({"batch": lambda: rrm.logistic_regression_batch(Xb, yb, EPS, return_info=True), "singles": singles},
                 max(5, a.reps // 8), 1)
    emit({"sweep": "rrm_logreg", "B": B, "n": Xb.shape[1], "d": Xb.shape[2], "us_median_min": t,
          "flags": np.bincount(info[:, 3]).tolist(),
          "outer_min_mean_max": [int(info[:, 0].min()), round(float(info[:, 0].mean()), 2), int(info[:, 0].max())],
          "outer_at_maxiter": int((info[:, 0] == MAXITER).sum())})
    if a.out:
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
