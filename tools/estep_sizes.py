"""E-step latency by population size (eager launches, warm workspace, rotating inputs).

usage: python tools/estep_sizes.py N [N ...]     (RLVI_TJ_DEBUG=1 adds the in-kernel stamps)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import stamps  # noqa: E402
from rlvi_amd import ops, synth  # noqa: E402

dev = torch.device("cuda:0")
for N in [int(a) for a in sys.argv[1:]]:
    ws = ops.Workspace(dev, N, 0)
    rs = [torch.from_numpy(synth.residual_vector("bimodal", N, seed=s)).to(dev) for s in range(4)]
    iters = torch.zeros(1, dtype=torch.int32, device=dev)

    def pair(k):
        return rs[k % 4].clone(), torch.ones(N, device=dev)

    for k in range(3):
        rt, wt = pair(k)
        ops.estep_deep(rt, wt, iters=iters, ws=ws)
    torch.cuda.synchronize()
    bufs = [pair(k) for k in range(20)]
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for rt, wt in bufs:
        ops.estep_deep(rt, wt, iters=iters, ws=ws)
    e1.record()
    torch.cuda.synchronize()
    print(N, "it", int(iters), "us/call %.1f" % (e0.elapsed_time(e1) * 1000 / 20), "status", ws.status(),
          flush=True)
    if os.environ.get("RLVI_TJ_DEBUG"):
        S = stamps.read(ws)
        print("   stamps us:", stamps.us(S.seq("SOLVE_SEQ", "SOLVE_COUNT"))[:24])
        print("   rounds (Ke, it, delta):", stamps.rounds(S)[:12])
        rn, rnew = S.f32_pair("TJ_NODES")
        rn = rn.astype(np.float64)
        tot = S.f64("TJ_TOTALS").reshape(8, 3)
        e = np.exp(-bufs[-1][0].cpu().numpy().astype(np.float64))
        print("   scale", stamps.f32(stamps.lo(S["TJ_SCALE"])))
        for k in range(4):
            r = rn[k]
            print("   node", k, "rn", r, "rnew", rnew[k], "kernel S,P,Q", tot[k], "numpy S,P,Q",
                  np.sum(r * e / (1 + r * e)), np.sum(e / (1 + r * e) ** 2), np.sum(e * e / (1 + r * e) ** 3))
        a, b = (v.astype(np.float64).reshape(-1, 64)[:, :24] for v in S.f32_pair("TJ_ROUND_NODES"))
        for xs in range(3):
            print("   round", xs, "rel change per node:", np.array2string(np.abs(b[xs] - a[xs]) / a[xs], precision=2, max_line_width=250))
