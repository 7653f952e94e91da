"""rrm.linear_regression and huber.linear_regression on one MI355X, numpy in and numpy out (every call ends in its one
host wait): the one launch against (a) the host-loop composition of existing ops (RRM: ops.rrm_update_weights +
standard._wls, one launch per statement and one host decision per outer iteration) and (b) tests/robust_linreg_ref.py in
numpy on the host; standard.linear_regression (RLVI) at the same shapes beside them; then the reference's sweep of 2000
problems of 40 x 10 (main.py:261-273) as ONE batch launch against 2000 single calls.

    python tools/time_robust_linreg.py [--reps 40] [--warm 5] [--out FILE] [--rlvi-only] [--tree DIR]

--rlvi-only: standard.linear_regression alone; --tree DIR: import rlvi_amd (and its built library) from the checkout
DIR instead of this one -- together they time another build, for the line "the unchanged estimator did not move".
The variants of a row are timed in turns, rep by rep, after a warm-up of each; per row one JSON line with the median
and the smallest wall-clock time per call in microseconds and the iteration counts from `info`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EPS = 0.4                                   # what the reference's experiments hand to RRM
SHAPES = ((40, 10), (1000, 20))
SWEEP = (2000, 40, 10)


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
    ap.add_argument("--rlvi-only", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose rlvi_amd is timed (default: this one)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_robust_linreg.py needs an MI355X: there is nothing to time without one")
    import rlvi_amd
    from rlvi_amd import standard, synth
    rows = []

    def emit(row):
        row["tree"] = os.path.dirname(os.path.dirname(os.path.abspath(rlvi_amd.__file__)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    data = {(n, d): synth.linreg_data(n, d, eps=0.2, nu=2.5, seed=n + d) for n, d in SHAPES}
    B, bn, bd = SWEEP
    sweep = [synth.linreg_data(bn, bd, eps=0.2, nu=2.5, seed=1 + b) for b in range(B)]
    Xb, yb = np.stack([x for x, _ in sweep]), np.stack([v for _, v in sweep])
    for (n, d), (X, y) in data.items():
        t = in_turns({"rlvi": lambda: standard.linear_regression(X, y)}, a.reps, a.warm)
        emit({"estimator": "rlvi", "n": n, "d": d, "us_median_min": t,
              "outer": int(standard.linear_regression(X, y, return_info=True)[2])})
    t = in_turns({"batch": lambda: standard.linear_regression_batch(Xb, yb)}, max(5, a.reps // 4), 2)
    emit({"sweep": "rlvi", "B": B, "n": bn, "d": bd, "us_median_min": t})
    if not a.rlvi_only:
        import robust_linreg_ref as R
        from rlvi_amd import huber, ops, rrm
        dev = torch.device("cuda", torch.cuda.current_device())
        for (n, d), (X, y) in data.items():
            Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
            ws = ops.workspace(dev, n, 0)
            _, _, info = rrm.linear_regression(X, y, EPS, return_info=True)
            loop = rrm._linear_regression_host_loop(Xd, yd, EPS, 100, 1e-3, ws)
            t = in_turns({"one_launch": lambda: rrm.linear_regression(X, y, EPS),
                          "host_loop_resident": lambda: rrm._linear_regression_host_loop(Xd, yd, EPS, 100, 1e-3, ws)},
                         a.reps, a.warm)
            t.update(in_turns({"restatement_host": lambda: R.rrm_linear_regression(X, y, EPS)}, max(3, a.reps // 10), 1))
            emit({"estimator": "rrm", "n": n, "d": d, "us_median_min": t, "info": [int(v) for v in info],
                  "host_loop_outer": int(loop[2])})
            _, _, info = huber.linear_regression(X, y, return_info=True)
            t = in_turns({"one_launch": lambda: huber.linear_regression(X, y)}, a.reps, a.warm)
            t.update(in_turns({"restatement_host": lambda: R.huber_linear_regression(X, y)}, max(3, a.reps // 10), 1))
            emit({"estimator": "huber", "n": n, "d": d, "us_median_min": t, "info": [int(v) for v in info]})
        for name, f_batch, f_single, args in (("rrm", rrm.linear_regression_batch, rrm.linear_regression, (EPS,)),
                                              ("huber", huber.linear_regression_batch, huber.linear_regression, ())):
            _, _, info = f_batch(Xb, yb, *args, return_info=True)

            def singles():
                for b in range(B):
                    f_single(Xb[b], yb[b], *args)
            # (return_info: a flagged problem is reported in `flags` below, not raised in the middle of the timing)
            t = in_turns({"batch": lambda: f_batch(Xb, yb, *args, return_info=True), "singles": singles},
                         max(5, a.reps // 8), 1)
            emit({"sweep": name, "B": B, "n": bn, "d": bd, "us_median_min": t, "flags": np.bincount(info[:, 3]).tolist(),
                  "iterations_min_mean_max": [int(info[:, 0].min()), round(float(info[:, 0].mean()), 2),
                                              int(info[:, 0].max())]})
    if a.out:
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
