"""Lab (a -DRLVI_STAMPS=1 build, RLVI_TJ_DEBUG=1): in-kernel stamps of ONE cold E-step (workspace option cold_start)."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import stamps  # noqa: E402
from rlvi_amd import ops, synth  # noqa: E402

dev = torch.device("cuda:0")
N = 65536
r = torch.from_numpy(synth.residual_vector("bimodal", N, seed=5)).to(dev)
w = torch.ones(N, device=dev)
it = torch.zeros(1, dtype=torch.int32, device=dev)
ws = ops.Workspace(dev, N, 0)
ws.set_option("cold_start", 1)
for _ in range(3):
    ops.estep_deep(r.clone(), w, iters=it, ws=ws)
torch.cuda.synchronize()
S = stamps.read(ws)
print("iters", int(it), "stamps (us since kernel start):", stamps.us(S.seq("SOLVE_SEQ", "SOLVE_COUNT")))
print("recurrence wave of round 0 [entry, prepared, chain, trust/tail(+global model), acceptance, out] us:",
      stamps.us(S.ticks("CHAIN_SEQ")))
print("rounds (Ke, it, delta):", stamps.rounds(S)[:6])
