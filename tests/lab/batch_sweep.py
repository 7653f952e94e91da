"""A Monte-Carlo sweep as ONE launch against B single calls, on one MI355X, in the same visit (profiles/r18_batch.md).

    python tests/lab/batch_sweep.py [--reps 20] [--loops 3] [--warm 3]     the table below, one JSON line per row
    python tests/lab/batch_sweep.py --single [--tree DIR]                  the single calls alone; DIR: with the
                                                                           package of another checkout (the parent's)
    python tests/lab/batch_sweep.py --kernels                              a few resident launches of each form and
                                                                           nothing else: the run to put under
                                                                           rocprofv3 --kernel-trace --stats

Per estimator at the reference's shape and sweep size (standard-learning/main.py: linear regression 40 x 10 and mean
100 x 2 with B = 2000, logistic regression 200 x 2, pca 40 x 2 and covariance 50 x 2 with B = 100), numpy in and numpy
out: the wall-clock time of one standard.*_batch call (median of --reps) and of a loop of B single one-launch calls
(median of --loops), the two alternating; then, on device tensors, device-event times of one batch launch and of one
single launch (200 queued back to back, per launch; problem 0, and the problem with the most outer iterations: a
batch cannot end before its slowest problem).  The batch results are compared with the loop's to the bit
before anything is timed.  Data: this package's contaminated generators (rlvi_amd/synth.py), the corruption level
running over the batch as in the reference's sweeps.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CASES = (("linreg", 40, 10, 2000), ("mean", 100, 2, 2000), ("logreg", 200, 2, 100), ("pca", 40, 2, 100),
         ("cov", 50, 2, 100))
COV_EPS = 0.4


def theta_init():
    t = np.array([0.1, 1.0])
    return t / np.linalg.norm(t)


def data(kind, n, d, B):
    """(X [B, n, d], y [B, n] or None)"""
    from rlvi_amd import synth
    eps = np.linspace(0.0, 0.4, B) if kind in ("linreg", "mean") else np.full(B, 0.05 if kind == "logreg" else 0.2)
    if kind == "linreg":
        pairs = [synth.linreg_data(size=n, d=d, eps=float(e), nu=2.5, seed=b) for b, e in enumerate(eps)]
        return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    if kind == "logreg":
        rng = np.random.default_rng(18)
        X = rng.standard_normal((B, n, d))
        y = (rng.random((B, n)) < 1 / (1 + np.exp(-(X[:, :, 0] + X[:, :, 1] - 0.5)))).astype(np.float64)
        flip = rng.random((B, n)) < eps[:, None]
        y = np.where(flip, 1 - y, y)
        y[:, 0], y[:, 1] = 0.0, 1.0
        return X, y
    x = np.stack([synth.heavy_tail_cloud(size=n, eps=float(e), seed=b) for b, e in enumerate(eps)])
    # (the reference's mean sweep sits at (200, 200) with a spread of 20: main.py:48-53)
    return (200.0 + 20.0 * x if kind == "mean" else x), None


def single_call(kind):
    from rlvi_amd import standard
    return {
        "linreg": lambda X, y: standard.linear_regression(X, y, return_info=True),
        "logreg": lambda X, y: standard.logistic_regression(X, y, solver="newton", return_info=True),
        "mean": lambda X, y: standard.mean(X, one_launch=True, return_info=True),
        "pca": lambda X, y: standard.pca(X, theta_init=theta_init(), one_launch=True, return_info=True),
        "cov": lambda X, y: standard.covariance(X, COV_EPS, one_launch=True, return_info=True),
    }[kind]


def batch_call(kind):
    from rlvi_amd import standard
    return {
        "linreg": lambda X, y: standard.linear_regression_batch(X, y, return_info=True),
        "logreg": lambda X, y: standard.logistic_regression_batch(X, y, return_info=True),
        "mean": lambda X, y: standard.mean_batch(X, return_info=True),
        "pca": lambda X, y: standard.pca_batch(X, theta_init=theta_init(), return_info=True),
        "cov": lambda X, y: standard.covariance_batch(X, COV_EPS, return_info=True),
    }[kind]


def resident(kind, X, y, dev, b=0):
    """(batch launch, single launch on problem b) on device tensors, outputs allocated once"""
    import torch
    from rlvi_amd import ops
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    B, n, d = X.shape
    Xd, yd = to(X), (None if y is None else to(y))
    init = to(theta_init())
    nt = {"linreg": d, "logreg": d + 1, "mean": d, "pca": d, "cov": d * d}[kind]
    ob = dict(theta=torch.zeros(B, nt, dtype=torch.float64, device=dev),
              weights=torch.zeros(B, n, dtype=torch.float64, device=dev),
              info=torch.zeros(B, 4, dtype=torch.int32, device=dev), ws=ops.workspace(dev, n, 0))
    o1 = dict(theta=torch.zeros(nt, dtype=torch.float64, device=dev),
              weights=torch.zeros(n, dtype=torch.float64, device=dev),
              info=torch.zeros(4, dtype=torch.int32, device=dev), ws=ops.workspace(dev, n, 0))
    if kind == "linreg":
        return (lambda: ops.linear_regression_batch(Xd, yd, **ob)), (lambda: ops.linear_regression(Xd[b], yd[b], **o1))
    if kind == "logreg":
        return (lambda: ops.logistic_regression_batch(Xd, yd, **ob)), (lambda: ops.logistic_regression(Xd[b], yd[b], **o1))
    if kind == "mean":
        return (lambda: ops.robust_mean_batch(Xd, **ob)), (lambda: ops.robust_mean(Xd[b], **o1))
    if kind == "pca":
        return ((lambda: ops.robust_pca_batch(Xd, theta_init=init, **ob)),
                (lambda: ops.robust_pca(Xd[b], theta_init=init, **o1)))
    n_eff = n * (1 - COV_EPS)
    return (lambda: ops.robust_covariance_batch(Xd, n_eff, **ob)), (lambda: ops.robust_covariance(Xd[b], n_eff, **o1))


def event_us(torch, fn, launches):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def wall_us(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("batch_sweep.py needs an MI355X: there is nothing to time without one")
    return torch, torch.device("cuda:0")


def run_single(reps):
    """One JSON line per estimator: the single numpy call at the reference's shape, median / min / max of `reps`
    medians-of-50 (the spread between them is the run-to-run spread of this visit)."""
    need_gpu()
    for kind, n, d, _ in CASES:
        X, y = data(kind, n, d, 4)
        one = single_call(kind)
        call = lambda: one(X[1], None if y is None else y[1])        # noqa: E731
        wall_us(call, 20)
        meds = [float(np.median(wall_us(call, 50))) for _ in range(reps)]
        print(json.dumps({"single": kind, "n": n, "d": d, "median_us": round(float(np.median(meds)), 1),
                          "min_us": round(min(meds), 1), "max_us": round(max(meds), 1)}), flush=True)


def run_kernels():
    torch, dev = need_gpu()
    for kind, n, d, B in CASES:
        X, y = data(kind, n, d, B)
        batch, single = resident(kind, X, y, dev)
        for _ in range(5):
            batch()
            single()
        torch.cuda.synchronize()
    print("launched 5 of each form", flush=True)


def run_table(reps, loops, warm):
    torch, dev = need_gpu()
    for kind, n, d, B in CASES:
        X, y = data(kind, n, d, B)
        one, many = single_call(kind), batch_call(kind)
        loop = lambda: [one(X[b], None if y is None else y[b]) for b in range(B)]      # noqa: E731
        got, want = many(X, y), loop()
        same = all(np.array_equal(got[0][b], want[b][0]) and np.array_equal(got[1][b], want[b][1]) for b in range(B))
        if not same:
            raise SystemExit(f"{kind}: the batch is not the loop's to the bit; nothing is timed")
        for _ in range(warm):
            many(X, y)
        t_batch, t_loop = [], []
        for _ in range(loops):                                     # the two alternating
            t_loop += wall_us(loop, 1)
            t_batch += wall_us(lambda: many(X, y), max(1, reps // loops))
        slow = int(np.argmax(got[2][:, 0]))                        # the problem with the most outer iterations
        batch, single = resident(kind, X, y, dev)
        _, slowest = resident(kind, X, y, dev, slow)
        row = {"estimator": kind, "n": n, "d": d, "B": B, "outer_min": int(got[2][:, 0].min()),
               "outer_max": int(got[2][:, 0].max()), "flags": int((got[2][:, 3] != 0).sum()),
               "batch_call_us": round(float(np.median(t_batch)), 1), "batch_call_min_us": round(min(t_batch), 1),
               "loop_us": round(float(np.median(t_loop)), 1), "loop_min_us": round(min(t_loop), 1),
               "batch_launch_event_us": round(event_us(torch, batch, 20), 1),
               "single_launch_event_us": round(event_us(torch, single, 200), 1),
               "slowest_single_launch_event_us": round(event_us(torch, slowest, 200), 1)}
        row["loop_over_batch"] = round(row["loop_us"] / row["batch_call_us"], 1)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--single", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--tree", help="with --single: import rlvi_amd from this checkout (built there)")
    a = ap.parse_args()
    if a.tree and not a.single:
        raise SystemExit("--tree goes with --single")
    if a.tree and os.path.abspath(a.tree) != ROOT:
        # a fresh child with the other checkout first on its path
        env = dict(os.environ, PYTHONPATH=os.path.abspath(a.tree), RLVI_BATCH_SWEEP_CHILD="1")
        cmd = [sys.executable, os.path.abspath(__file__), "--single", "--reps", str(a.reps)]
        raise SystemExit(subprocess.run(cmd, env=env, cwd=os.path.abspath(a.tree)).returncode)
    if not os.environ.get("RLVI_BATCH_SWEEP_CHILD"):
        sys.path.insert(0, ROOT)
    if a.single:
        return run_single(max(3, a.reps // 4))
    if a.kernels:
        return run_kernels()
    run_table(a.reps, a.loops, a.warm)


if __name__ == "__main__":
    main()
