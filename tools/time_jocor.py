"""JoCoR's joint loss, forward + backward, on one MI355X: the HIP path (ops.jocor_loss, rlvi_amd/csrc/jocor.hip)
against the reference's loss_jocor (deep-learning/methods/train_jocor.py:29-43) restated in stock torch on the same
device -- two log_softmax, two softmax, two kl_div, two cross_entropy, the .cpu() + np.argsort + gather + mean on
the host, and autograd's backward into both blocks.

    python tools/time_jocor.py [--reps 200]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/time_jocor.py      (per-kernel device times)

Per shape it prints one JSON line: the wall time per step from device events (a step = forward + backward, the
reference's including its device sync), the same for the three + one raw launches of the HIP path alone, and the
algorithmic bytes B (6 C s + 16) -- both blocks read twice, both gradients written once, the labels read twice --
over that raw time as a fraction of 8 TB/s.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlvi_amd import ops, synth  # noqa: E402

SHAPES = [(4096, 10, torch.float32), (1024, 101, torch.bfloat16), (65536, 100, torch.float32)]
PEAK = 8e12
FORGET = 0.2


def reference_step(z1, z2, t, forget_rate, co_lambda=0.1):
    """loss_jocor as the reference runs it (batch-mean KL terms, host argsort), then backward.  bf16 / fp16 blocks
    are taken to fp32 first, as torch.autocast runs these ops (the reference has no half-precision path)."""
    if z1.dtype != torch.float32:
        z1, z2 = z1.float(), z2.float()
    ce1 = F.cross_entropy(z1, t, reduction="none") * (1 - co_lambda)
    ce2 = F.cross_entropy(z2, t, reduction="none") * (1 - co_lambda)
    k_qp = torch.sum(F.kl_div(F.log_softmax(z1, dim=1), F.softmax(z2, dim=1), reduction="none"), 1).mean()
    k_pq = torch.sum(F.kl_div(F.log_softmax(z2, dim=1), F.softmax(z1, dim=1), reduction="none"), 1).mean()
    pick = (ce1 + ce2 + co_lambda * k_qp + co_lambda * k_pq).cpu()
    order = np.argsort(pick.data)
    k = int((1 - forget_rate) * len(pick))
    loss = torch.mean(pick[order[:k]])
    loss.backward()


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for B, C, dt in SHAPES:
        d1 = synth.mstep_inputs(B, C, N=B, seed=B + C)
        d2 = synth.mstep_inputs(B, C, N=B, seed=B + C + 1)
        z1 = torch.from_numpy(d1["logits"]).to(dev).to(dt).requires_grad_(True)
        z2 = torch.from_numpy(d2["logits"]).to(dev).to(dt).requires_grad_(True)
        t = torch.from_numpy(d1["labels"]).to(dev)
        ws = ops.Workspace(dev, B, B)

        def ours():
            z1.grad = z2.grad = None
            ops.jocor_loss(z1, z2, t, FORGET, ws=ws, check=False).backward()

        k = ops.jocor_num_remember(FORGET, B)
        x1, x2 = z1.detach(), z2.detach()
        one = torch.ones((), device=dev)

        def raw():
            _, _, sel = ops.jocor_forward(x1, x2, t, k, ws=ws)
            ops.jocor_backward(x1, x2, t, sel, k, grad_out=one)

        def ref():
            z1.grad = z2.grad = None
            reference_step(z1, z2, t, FORGET)

        us_ours = timed(ours, a.reps)
        us_raw = timed(raw, a.reps)
        us_ref = timed(ref, max(a.reps // 4, 10))
        s = torch.finfo(dt).bits // 8
        nbytes = B * (6 * C * s + 16)
        print(json.dumps({"shape": [B, C], "dtype": str(dt)[6:], "forget_rate": FORGET,
                          "ours_step_us": round(us_ours, 2), "ours_raw_launches_us": round(us_raw, 2),
                          "reference_torch_step_us": round(us_ref, 2), "speedup_step": round(us_ref / us_ours, 1),
                          "algorithmic_bytes": nbytes,
                          "raw_frac_of_8TBs": round(nbytes / (us_raw * 1e-6) / PEAK, 3)}), flush=True)
        assert ws.status() == 0


if __name__ == "__main__":
    main()
