"""fp16 against bf16 M-step launches, and the autocast plug-in's fp16 batch against the old fp32 upcast.

Run under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/profile_fp16.py` (no --pmc in the same
run): every (shape, dtype) segment is REPS accumulate-mode launches in the order printed here, so the kernel trace
splits into segments by position; the events give the wall time per launch or per batch on top.
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlvi_amd import _lib, ops, synth  # noqa: E402

REPS = 200
SHAPES = [(65536, 100), (65536, 101), (1024, 101), (16384, 1000)]


def timed(fn, reps=REPS):
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
    dev = torch.device("cuda:0")
    L = _lib.load()
    for B, C in SHAPES:
        d = synth.mstep_inputs(B, C, seed=1)
        z = torch.from_numpy(d["logits"]).to(dev)
        y, ix = torch.from_numpy(d["labels"]).to(dev), torch.from_numpy(d["idx"]).to(dev)
        w, r = torch.from_numpy(d["weights"]).to(dev), torch.zeros(B, device=dev)
        ws = ops.Workspace(dev, B, B)
        loop = ops.MStepLoop(w, r, ws)
        for dt in (torch.bfloat16, torch.float16):
            zz = z.to(dt)
            us = timed(lambda: loop(zz, y, ix))
            print(json.dumps({"shape": [B, C], "dtype": str(dt)[6:], "launches": REPS + 1, "event_us": round(us, 2),
                              "form": L.rlvi_workspace_last_mstep_form(ws.ptr)}), flush=True)
        ops.mstep_reduce(ws=ws)
    # one batch of the plug-in at 65 536 x 100 under autocast(fp16): native fp16 against the fp32 upcast the
    # Python layer did before (fp32 copy of the logits, fp32 kernel, autograd's cast of the gradient back to fp16)
    B, C = 65536, 100
    d = synth.mstep_inputs(B, C, seed=2)
    z16 = torch.from_numpy(d["logits"]).to(dev).half()
    y, ix = torch.from_numpy(d["labels"]).to(dev), torch.from_numpy(d["idx"]).to(dev)
    w, r = torch.from_numpy(d["weights"]).to(dev), torch.zeros(B, device=dev)
    ws = ops.Workspace(dev, B, B)
    loop = ops.MStepLoop(w, r, ws)
    native = timed(lambda: loop(z16, y, ix))
    upcast = timed(lambda: loop(z16.float(), y, ix).to(torch.float16))
    ops.mstep_reduce(ws=ws)
    print(json.dumps({"plugin_batch": [B, C], "native_fp16_us": round(native, 2), "fp32_upcast_us": round(upcast, 2),
                      "launches_each": REPS + 1}), flush=True)
    assert ws.status() == 0


if __name__ == "__main__":
    main()
