"""mean / pca / covariance on one MI355X: `one_launch=True` (rlvi_amd/csrc/moments.hip) against the default host loop
(the E-step on the GPU, numpy / scipy around it), numpy in and numpy out, in the same visit.

    python tools/time_moments.py [--reps 30] [--warm 5]

Shapes: the reference's own (mean 100 x 2, pca 40 x 2 with its theta_init (0.1, 1) / ||.||, covariance 50 x 2 with
eps = 0.4; synth.heavy_tail_cloud, the recipe of the reference's generators) and contaminated 4096 x 4 and 2048 x 8
clouds through all three.  Every (estimator, shape, path) is timed in a child process of its own under a time limit; the first one
that fails ends the run.  Per child one JSON line: the median and the smallest wall-clock time per call after the
warm-up, the outer count and -- for the one launch, from `info` -- the inner iterations of the last E-step and the
per-estimator count, so that a per-iteration figure can be read off.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("mean", 100, 2), ("pca", 40, 2), ("covariance", 50, 2), ("mean", 4096, 4), ("pca", 4096, 4),
         ("covariance", 4096, 4),
         # sixteen samples per thread with d > 4: the kernel variants that spill registers to scratch memory
         ("mean", 2048, 8), ("pca", 2048, 8), ("covariance", 2048, 8))
LIMIT_S = 240


def sample(n, d):
    from rlvi_amd import synth
    if d == 2:
        return synth.heavy_tail_cloud(size=n, eps=0.2, seed=n)
    rng = np.random.default_rng(n + d)
    dev = rng.standard_normal((n, d)) * 2.0 ** (-0.5 * np.arange(d))
    k = n // 5
    dev[:k] /= np.sqrt(rng.chisquare(1.5, k) / 1.5)[:, None]
    return dev + 0.5 * np.arange(d)


def one(kind, n, d, path, reps, warm):
    import torch
    from rlvi_amd import standard
    if not torch.cuda.is_available():
        raise SystemExit("time_moments.py needs an MI355X: there is nothing to time without one")
    x = sample(n, d)
    kw = {}
    if kind == "pca" and d == 2:
        t = np.array([0.1, 1.0])
        kw["theta_init"] = t / np.linalg.norm(t)
    args = (0.4,) if kind == "covariance" else ()
    fn = getattr(standard, kind)
    row = {"estimator": kind, "n": n, "d": d, "path": path}
    if path == "one_launch":
        theta, _, info = fn(x, *args, one_launch=True, return_info=True, **kw)
        row.update(outer=int(info[0]), inner_last=int(info[1]), count=int(info[2]), flag=int(info[3]))
        call = lambda: fn(x, *args, one_launch=True, **kw)             # noqa: E731
    else:
        calls = []
        orig = standard.update_weights
        standard.update_weights = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        try:
            theta = fn(x, *args, **kw)
        finally:
            standard.update_weights = orig
        row["outer"] = len(calls)
        call = lambda: fn(x, *args, **kw)                              # noqa: E731
    times = []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        call()
        if i >= warm:
            times.append((time.perf_counter() - t0) * 1e6)
    row.update(median_us=round(float(np.median(times)), 1), min_us=round(float(np.min(times)), 1),
               theta=[float(v) for v in np.ravel(theta)[:4]])
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--one", nargs=4, metavar=("ESTIMATOR", "N", "D", "PATH"))
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], int(a.one[1]), int(a.one[2]), a.one[3], a.reps, a.warm)
    for kind, n, d in CASES:
        for path in ("one_launch", "host_loop"):
            cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--reps",
                   str(a.reps), "--warm", str(a.warm), "--one", kind, str(n), str(d), path]
            rc = subprocess.run(cmd, cwd=ROOT).returncode
            if rc != 0:
                raise SystemExit(f"{kind} {n} x {d} {path}: exit status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
