"""rrm.mean / pca / covariance on one MI355X, numpy in and numpy out (every call ends in its one host wait): the RRM
one launch, the RLVI one launch of the same shape beside it, and tests/rrm_ref.py on the host; then a Monte-Carlo
sweep as ONE batch launch against as many single calls.

    python tools/time_rrm.py [--reps 40] [--warm 5] [--out FILE]

Shapes: the reference's own (mean 100 x 2, pca 200 x 2, covariance 50 x 2; synth.heavy_tail_cloud, the recipe of the
reference's generators) and a contaminated 4096 x 4 cloud through all three; eps = 0.4, the value the reference's
experiments hand to RRM (main.py:184, :222).  Sweeps: 2000 means of 100 x 2, 100 PCAs of 200 x 2, 100 covariances of
50 x 2.  The variants of a row are timed in turns, rep by rep, after a warm-up of each; per row one JSON line with the
median and the smallest wall-clock time per call in microseconds, the outer count and the evaluations of the
root-finds from `info` (last, in all, per root-find).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

EPS = 0.4
SINGLE = (("mean", 100, 2), ("pca", 200, 2), ("covariance", 50, 2), ("mean", 4096, 4), ("pca", 4096, 4),
          ("covariance", 4096, 4))
SWEEPS = (("mean", 2000, 100, 2), ("pca", 100, 200, 2), ("covariance", 100, 50, 2))


def sample(n, d, seed=0):
    from rlvi_amd import synth
    if d == 2:
        return synth.heavy_tail_cloud(size=n, eps=0.2, seed=n + seed)
    rng = np.random.default_rng(n + d + seed)
    dev = rng.standard_normal((n, d)) * 2.0 ** (-0.5 * np.arange(d))
    k = n // 5
    dev[:k] /= np.sqrt(rng.chisquare(1.5, k) / 1.5)[:, None]
    return dev + 1.0 + 0.5 * np.arange(d)


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
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_rrm.py needs an MI355X: there is nothing to time without one")
    import rrm_ref
    from rlvi_amd import rrm, standard
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
    for kind, n, d in SINGLE:
        x = sample(n, d)
        f_rrm, f_rlvi = getattr(rrm, kind), getattr(standard, kind)
        f_ref = getattr(rrm_ref, kind)
        rlvi_args = (EPS,) if kind == "covariance" else ()
        _, _, info = f_rrm(x, EPS, return_info=True)
        _, _, info_rlvi = f_rlvi(x, *rlvi_args, one_launch=True, return_info=True)
        t = in_turns({"rrm": lambda: f_rrm(x, EPS), "rlvi": lambda: f_rlvi(x, *rlvi_args, one_launch=True)},
                     a.reps, a.warm)
        t.update(in_turns({"rrm_ref_host": lambda: f_ref(x, EPS)}, max(3, a.reps // 10), 1))
        roots = int(info[0])
        emit({"estimator": kind, "n": n, "d": d, "us_median_min": t, "rrm_outer": roots,
              "rrm_evals_last": int(info[1]), "rrm_count": int(info[2]),
              "rrm_evals_per_root": round(int(info[2]) / roots, 2) if kind != "pca" and roots else None,
              "rrm_flag": int(info[3]), "rlvi_info": [int(v) for v in info_rlvi]})
    for kind, B, n, d in SWEEPS:
        X = np.stack([sample(n, d, seed=1 + b) for b in range(B)])
        f_batch, f_single = getattr(rrm, kind + "_batch"), getattr(rrm, kind)
        _, _, info = f_batch(X, EPS, return_info=True)

        def singles():
            for b in range(B):
                f_single(X[b], EPS)
        t = in_turns({"batch": lambda: f_batch(X, EPS), "singles": singles}, max(5, a.reps // 4), 2)
        emit({"sweep": kind, "B": B, "n": n, "d": d, "us_median_min": t, "flags": np.bincount(info[:, 3]).tolist(),
              "outer_min_mean_max": [int(info[:, 0].min()), round(float(info[:, 0].mean()), 2), int(info[:, 0].max())],
              "evals_last_min_mean_max": [int(info[:, 1].min()), round(float(info[:, 1].mean()), 2),
                                          int(info[:, 1].max())],
              "evals_per_root": round(float(info[:, 2].sum() / info[:, 0].sum()), 2) if kind != "pca" else None})
    if a.out:
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
