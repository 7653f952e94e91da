"""The online path on one MI355X: the device time of one mini-batch step (rlvi_online_step_f64) at 100 x 60 and at
256 x 60 for each method, and the reference's whole stream -- 54 mini-batches of 100 train and 100 test rows by 60 columns,
three classifiers (SGD, RRM, RLVI) -- as ONE launch (rlvi_online_stream_f64) against the same stream as 54 x 3 single
steps, in the same visit, the two in turns.

    python tools/time_online.py [--reps 20] [--warm 3] [--out profiles/r25_online.md]

Everything is resident on the device before the clock starts and the times are HIP events around the launches of a
rep (the single steps: 162 launches between one pair of events), so they are the device's, without copies.  The data
are synthetic (two Gaussian classes along one direction, per-batch standard scaler, 30 % of the positive labels
flipped): the reference's dataset is not part of this repository.  One condition is checked, and the exit status is 1 when it fails: the stream's
median must not be above the single steps' (it only removes launches).  No other time is a pass mark.  --out appends a
markdown section to the file.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("SGD", "RRM", "RLVI")
EPS = 0.3


def direction(rng, d):
    u = rng.standard_normal(d)
    return u / np.linalg.norm(u)


def batch(rng, n, m, d, u):
    lab = (rng.random(n + m) < 0.5).astype(np.float64)
    Z = rng.standard_normal((n + m, d)) + 3.0 * np.outer(lab - 0.5, u) + 0.5
    Z = (Z - Z[m:].mean(axis=0)) / Z[m:].std(axis=0)
    y = lab[m:].copy()
    pos = np.flatnonzero(y == 1)
    y[rng.choice(pos, size=int(0.3 * len(pos)), replace=False)] = 0
    return Z[m:], y, Z[:m], lab[:m]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_online.py needs an MI355X: there is nothing to time without one")
    from rlvi_amd import online, ops
    dev = torch.device("cuda", torch.cuda.current_device())
    to = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)      # noqa: E731
    rows_out = []

    def emit(row):
        rows_out.append(row)
        print(json.dumps(row), flush=True)

    def timed(calls, reps, warm):
        """{name: (median us, min us)} of device time, one of each call per round"""
        for fn in calls.values():
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        for _ in range(reps):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                t[k].append(1e3 * e0.elapsed_time(e1))
        return {k: (round(float(np.median(v)), 1), round(float(np.min(v)), 1)) for k, v in t.items()}

    # ---- one step, from the state two batches leave behind
    rng = np.random.default_rng(25)
    for n in (100, 256):
        d, m = 60, n
        u = direction(rng, d)
        data = [tuple(to(v) for v in batch(rng, n, m, d, u)) for _ in range(3)]
        order = to(online.sgd_order(n))
        calls = {}
        for name in METHODS:
            state = torch.zeros(d + 2, dtype=torch.float64, device=dev)
            for k in range(2):
                ops.online_step(data[k][0], data[k][1], state, method=name, eps=EPS, first=k == 0, order=order)
            scratch, sw = state.clone(), torch.empty(n, dtype=torch.float64, device=dev)
            counts, info = torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
            X, y, Xt, yt = data[2]

            def step(name=name, state=state, scratch=scratch, sw=sw, counts=counts, info=info):
                scratch.copy_(state)              # (the same step every time: a 62-double device copy inside the clock)
                ops.online_step(X, y, scratch, method=name, eps=EPS, order=order, X_test=Xt, y_test=yt,
                                sample_weight=sw, counts=counts, info=info)
            calls[name] = step
        t = timed(calls, a.reps, a.warm)
        emit({"step": f"{n} x {d}, {m} test rows", "device_us_median_min": t})

    # ---- the stream: 54 batches, three classifiers
    T, n, m, d = 54, 100, 100, 60
    rng = np.random.default_rng(26)
    u = direction(rng, d)
    bs = [batch(rng, n, m, d, u) for _ in range(T)]
    X, y, Xt, yt = (to(np.stack([b[j] for b in bs])) for j in range(4))
    orders = to(np.stack([online.sgd_order(n)] * T))
    S = len(METHODS)
    hist = torch.empty((S, T, d + 2), dtype=torch.float64, device=dev)
    counts = torch.zeros((S, T, 4), dtype=torch.int32, device=dev)
    weights = torch.zeros((S, T, n), dtype=torch.float64, device=dev)
    info = torch.zeros((S, T, 4), dtype=torch.int32, device=dev)
    states = torch.zeros((S, d + 2), dtype=torch.float64, device=dev)
    c1 = torch.zeros((S, T, 4), dtype=torch.int32, device=dev)
    w1 = torch.zeros((S, T, n), dtype=torch.float64, device=dev)
    i1 = torch.zeros((S, T, 4), dtype=torch.int32, device=dev)

    def one_launch():
        ops.online_stream(X, y, Xt, yt, methods=METHODS, eps=EPS, orders=orders, weights=weights, state_hist=hist,
                          counts=counts, info=info)

    def single_steps():
        for k in range(T):
            for s, name in enumerate(METHODS):
                ops.online_step(X[k], y[k], states[s], method=name, eps=EPS, first=k == 0, order=orders[k],
                                X_test=Xt[k], y_test=yt[k], sample_weight=w1[s, k], counts=c1[s, k], info=i1[s, k])
    one_launch()
    single_steps()
    torch.cuda.synchronize()
    same = bool(torch.equal(hist[:, -1], states) and torch.equal(counts, c1) and torch.equal(weights, w1))
    t = timed({"one_launch": one_launch, "single_steps": single_steps}, max(5, a.reps // 2), 1)
    ok = t["one_launch"][0] <= t["single_steps"][0]
    emit({"stream": f"{T} batches of {n} + {m} rows x {d}, {S} classifiers", "device_us_median_min": t,
          "same_bits": same, "stream_not_slower": ok,
          "test_accuracy_last_batch": {name: float((counts[s, -1, 0] + counts[s, -1, 1]).item()) / m
                                       for s, name in enumerate(METHODS)}})
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n## Device times (tools/time_online.py; HIP events, microseconds, median and smallest)\n\n```\n")
            for row in rows_out:
                f.write(json.dumps(row) + "\n")
            f.write("```\n")
    if not (ok and same):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
