"""BARE's pruned cross-entropy on one MI355X: the HIP path (ops.bare_loss, rlvi_amd/csrc/bare.hip) in both kernel
forms against
(a) an eager restatement of the same formulas out of stock torch ops on the same device and inputs (`eager_bare`
    below: softmax, clamp, the gathers, mean and std down the batch, the comparison, the masked mean) -- forward, and
    forward + backward through autograd;
(b) the evaluation-form M-step (ops.evaluate_batch) on the same block: the streaming kernel that reads the same bytes
    once.  Pass 1 of the streaming form reads them once too, so its distance from (b) is the cost of the column
    statistics (plus the finishing workgroup).

    python tools/time_bare.py [--reps 200]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/time_bare.py --reps 20 --ours-only

Per shape and form one JSON line: the median time per call from device events around batches of calls (CALLS calls
between two events, so that a time of a few microseconds is not the events' own), forward alone and forward +
backward.  Small shapes (the reference's batches) run in both forms, forced through the knob RLVI_BARE_FORM; large
shapes in the streaming form only.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlvi_amd import _lib, ops, synth  # noqa: E402

SMALL = ((32, 10, "f32"), (128, 10, "f32"), (128, 100, "f32"))
LARGE = ((4096, 10, "f32"), (1024, 101, "bf16"), (65536, 100, "f32"))
EXTRA = ((512, 32, "f32"), (1024, 16, "f32"), (2048, 1500, "f32"))      # the bound of the one-workgroup form; long rows
CALLS = 20
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def eager_bare(z, y, k=1.0):
    """The formulas of WeightedCCE.forward as stock torch ops (written here, from the formulas)."""
    p = torch.softmax(z.float(), dim=1).clamp(1e-8, 1 - 1e-8)
    pt = p.gather(1, y[:, None])[:, 0]
    mu, sd = p.mean(0), p.std(0)
    keep = (pt - mu[y]) >= k * sd[y]
    ce = torch.nn.functional.cross_entropy(z.float(), y, reduction="none")
    n = keep.sum()
    kept = (ce * keep).sum() / n.clamp(min=1)
    return torch.where(n > 0, kept, ce.mean())


def per_call_us(fn, reps, warm=3):
    times = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            times.append(a.elapsed_time(b) * 1e3 / CALLS)
    return round(float(np.median(times)), 2), round(float(np.min(times)), 2)


def time_shape(B, C, dt, forms, reps, ours_only):
    dev = torch.device("cuda:0")
    zn, yn = synth.bare_dense_inputs(B, C, 0.5, seed=B + C)
    z = torch.from_numpy(zn).to(dev).to(DT[dt])
    y = torch.from_numpy(yn).to(dev)
    zg = z.clone().requires_grad_(True)
    ws = ops.workspace(dev, B, B)
    out = torch.empty(4, device=dev)
    L = _lib.load()

    def fwd():
        ops.bare_forward(z, y, 1.0, out=out, ws=ws)

    def fwd_bwd():
        zg.grad = None
        ops.bare_loss(zg, y, 1.0, ws=ws, check=False).backward()

    row = {"B": B, "C": C, "dtype": dt, "bytes": z.numel() * z.element_size()}
    for form in forms:
        L.rlvi_tune_set(b"RLVI_BARE_FORM", form)
        try:
            name = "one_wg" if L.rlvi_bare_form(B, C) == 1 else "streaming"
            row[name + "_fwd_us"], row[name + "_fwd_min_us"] = per_call_us(fwd, reps)
            row[name + "_fwd_bwd_us"], _ = per_call_us(fwd_bwd, reps)
        finally:
            L.rlvi_tune_unset(b"RLVI_BARE_FORM")
    row["by_size"] = "one_wg" if L.rlvi_bare_form(B, C) == 1 else "streaming"
    row["mstep_eval_us"], row["mstep_eval_min_us"] = per_call_us(lambda: ops.evaluate_batch(z, y, out=out, ws=ws), reps)
    ones = torch.ones(B, device=dev)
    row["mstep_fwd_bwd_us"], _ = per_call_us(
        lambda: ops.mstep_fwd_bwd(z, y, None, ones, None, inv_scale=1.0 / B, ws=ws), reps)
    if not ours_only:
        r = max(reps // 4, 5)
        row["eager_fwd_us"], _ = per_call_us(lambda: eager_bare(z, y), r)

        def eager_fwd_bwd():
            zg.grad = None
            eager_bare(zg, y).backward()
        row["eager_fwd_bwd_us"], _ = per_call_us(eager_fwd_bwd, r)
        ref = float(eager_bare(z, y))
        ops.bare_forward(z, y, 1.0, out=out, ws=ws)
        row["loss_vs_eager_rel"] = abs(float(out[0]) - ref) / abs(ref)
    ws.raise_on_status("time_bare")
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--ours-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bare.py needs an MI355X: there is nothing to time without one")
    for B, C, dt in SMALL:
        time_shape(B, C, dt, (0, 1), a.reps, a.ours_only)
    for B, C, dt in EXTRA[:2]:
        time_shape(B, C, dt, (0, 1), a.reps, a.ours_only)
    for B, C, dt in LARGE + EXTRA[2:]:
        time_shape(B, C, dt, (0,), max(a.reps // 4, 10), a.ours_only)


if __name__ == "__main__":
    main()
