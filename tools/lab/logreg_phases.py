"""Lab: where the one-launch logistic_regression spends its time.

    python tools/lab/logreg_phases.py [n d]                               call times, newton against liblinear
    RLVI_LIB_PATH=rlvi_amd/librlvi_stamps.so python tools/lab/logreg_phases.py [n d]     ... and the phase stamps

Call times: medians of 30 calls after 5 of standard.logistic_regression with both solvers (numpy in, numpy out).
With a -DRLVI_STAMPS=1 build (tools/build_variants.py stamps=-DRLVI_STAMPS=1): logreg.hip's thread 0 leaves
(100 MHz wall clock, phase code) pairs at the start of the workspace scratch; printed are the device time per
Newton step and per inner E-step iteration.  Data: G5's logreg/* at 200 x 2, else G15's Gaussian design of that
shape (tests/golden)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from rlvi_amd import ops, standard  # noqa: E402

n, d = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (200, 2)
if (n, d) == (200, 2):
    g = np.load(os.path.join(ROOT, "tests", "golden", "g5_standard.npz"))
    X, y = g["logreg/X"], g["logreg/y"]
else:
    g = np.load(os.path.join(ROOT, "tests", "golden", "g15_logreg.npz"))
    X, y = g[f"gauss_{n}x{d}_eps0.1/X"].astype(np.float64), g[f"gauss_{n}x{d}_eps0.1/y"]


def median_us(fn, calls=30, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts))


t_newton = median_us(lambda: standard.logistic_regression(X, y, solver="newton"))
t_lib = median_us(lambda: standard.logistic_regression(X, y))          # (the same call, the default solver)
_, _, outer = standard.logistic_regression(X, y, solver="newton", return_info=True)
print(f"{n} x {d}: newton {t_newton:9.1f} us   liblinear {t_lib:9.1f} us   per call (median of 30), outer {outer}",
      flush=True)

if os.environ.get("RLVI_LIB_PATH"):
    dev = torch.device("cuda:0")
    ws = ops.Workspace(dev, n, 0)
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    _, _, info = ops.logistic_regression(Xd, yd, ws=ws)
    torch.cuda.synchronize()
    info = info.cpu().numpy()
    off = ops.debug_scratch_offset()
    raw = ws.buf[off:off + 480 * 8].cpu().numpy().view(np.uint64).reshape(-1, 2)
    ticks, codes = raw[:, 0].astype(np.int64), raw[:, 1].astype(np.int64)
    k = int(np.argmax(ticks == 0)) if (ticks == 0).any() else len(ticks)
    ticks, codes = ticks[:k], codes[:k]
    steps, esteps = [], []
    for i in range(k - 1):
        if codes[i] == 1:                                   # a Newton step: to the next step's start or the fit's end
            j = i + 1
            while j < k and codes[j] not in (1, 7):
                j += 1
            if j < k and codes[i + 1:j].tolist().count(4) == 1:      # (a step that solved: not the stop test's pass)
                steps.append((ticks[j] - ticks[i]) / 100.0)
        if codes[i] == 8 and codes[i + 1] == 9:
            esteps.append((ticks[i + 1] - ticks[i]) / 100.0)
    print(f"info {info.tolist()}: {k} stamps, launch {(ticks[-1] - ticks[0]) / 100.0:.1f} us on the device")
    if steps:
        print(f"Newton step: median {np.median(steps):.2f} us (min {np.min(steps):.2f}, max {np.max(steps):.2f}, "
              f"{len(steps)} steps stamped)")
    names = {(1, 2): "objective + coefficients", (2, 3): "Hessian + gradient (Gram pass)", (3, 4): "L D L^T solve",
             (4, 5): "Z.delta", (5, 6): "Armijo trials", (6, 1): "accept", (3, 7): "final Z.v (behind the stop test)"}
    for (a, b), name in names.items():
        ds = [(ticks[i + 1] - ticks[i]) / 100.0 for i in range(k - 1) if codes[i] == a and codes[i + 1] == b]
        if ds:
            print(f"    {name:34s} median {np.median(ds):7.2f} us  ({len(ds)} stamped)")
    if esteps and info[1] > 0:
        print(f"last E-step: {esteps[-1]:.2f} us for {info[1]} inner iterations = {esteps[-1] / info[1]:.3f} us each")
