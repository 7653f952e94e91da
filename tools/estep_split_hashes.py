#!/usr/bin/env python3
"""Bits of the E-step over the branches around its first round, one line per call, for comparing two builds of
the library (the case list of tests/test_estep_split_gpu.py):

    RLVI_LIB_PATH=<parent .so> python tools/estep_split_hashes.py parent.txt
    python tools/estep_split_hashes.py new.txt
    python tools/estep_split_hashes.py --compare parent.txt new.txt [--dumps DIR_A DIR_B]

Per call: status, iteration count and the SHA-256 of pi, of the shifted residuals and of the warm-start state
the call leaves in the workspace (the stored trajectory nodes, the shift, the count); for the in-batch E+M also
of the gradient, the loss rows and the four scalars.  Seeded inputs from rlvi_amd.synth, a fresh workspace per
case.  --compare: the two files line for line, and the arrays of two `bench.py --dump-outputs` directories
with np.array_equal; exit status 1 on any difference."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def compare(argv):
    a, b = argv[0], argv[1]
    la, lb = open(a).read().splitlines(), open(b).read().splitlines()
    bad = [i for i, (x, y) in enumerate(zip(la, lb)) if x != y]
    if len(la) != len(lb):
        bad.append(min(len(la), len(lb)))
    for i in bad[:20]:
        print("DIFF line", i + 1, "\n  ", la[i] if i < len(la) else "-", "\n  ", lb[i] if i < len(lb) else "-")
    print(f"{a} / {b}: {len(la)} / {len(lb)} lines, {len(bad)} differ")
    if "--dumps" in argv:
        da, db = argv[argv.index("--dumps") + 1], argv[argv.index("--dumps") + 2]
        names = sorted(n for n in os.listdir(da) if n.endswith(".npy"))
        if names != sorted(n for n in os.listdir(db) if n.endswith(".npy")) or not names:
            print("dump directories hold different files:", names, sorted(os.listdir(db)))
            bad.append(-1)
        for n in names:
            same = np.array_equal(np.load(os.path.join(da, n)), np.load(os.path.join(db, n)))
            print(f"dump {n}: {'equal' if same else 'DIFFERENT'}")
            if not same:
                bad.append(-1)
    sys.exit(1 if bad else 0)


def main():
    if sys.argv[1] == "--compare":
        compare(sys.argv[2:])
    import torch
    from rlvi_amd import _lib, ops, synth
    dev = torch.device("cuda:0")
    L = _lib.load()
    lines = []

    def estep(tag, N, calls, options=None, knobs=None):
        for k, v in (knobs or {}).items():
            _lib.check(L.rlvi_tune_set(k.encode(), int(v)), "rlvi_tune_set")
        try:
            ws = ops.Workspace(dev, N, 0)
            for k, v in (options or {}).items():
                ws.set_option(k, v)
            off, nb = ws.region("warm")
            for i, (r, w, kw) in enumerate(calls):
                maxiter = kw.get("maxiter", 40)
                rt, wt = torch.from_numpy(r.copy()).to(dev), torch.from_numpy(w.copy()).to(dev)
                iters = torch.zeros(1, dtype=torch.int32, device=dev)
                tr = torch.zeros(2 * maxiter, device=dev) if kw.get("trace") else None
                ops.estep_deep(rt, wt, maxiter=maxiter, iters=iters, trace=tr, ws=ws)
                torch.cuda.synchronize()
                st = ws.status()
                ws.clear_status()
                lines.append(f"{tag} call {i} status {st} iters {int(iters)} pi {sha(wt.cpu().numpy())} "
                             f"res {sha(rt.cpu().numpy())} warm {sha(ws.buf[off:off + nb].cpu().numpy())}"
                             + (f" trace {sha(tr.cpu().numpy())}" if tr is not None else ""))
        finally:
            for k in (knobs or {}):
                L.rlvi_tune_unset(k.encode())

    def vec(N, kind="bimodal", seed=None):
        return synth.residual_vector(kind, N, seed=N if seed is None else seed)

    def ones(N):
        return np.ones(N, np.float32)

    for N, kind in [(64, "bimodal"), (300, "bimodal"), (4096, "bimodal"), (54000, "bimodal"), (65536, "bimodal"),
                    (65537, "bimodal"), (75750, "zeros10"), (131072, "bimodal"), (262144, "bimodal")]:
        r = vec(N, kind)
        estep(f"size {N} {kind}", N, [(r, ones(N), {}), (r, ones(N), {}),
                                      (r, np.random.default_rng(N).random(N).astype(np.float32), {})])
    N = 65536
    estep("warm", N, [(vec(N, seed=1), ones(N), {})] * 5)
    rng = np.random.default_rng(11)
    base = vec(N, seed=0)
    dr = [(base * np.float32(1.02 ** k) + np.float32(0.01) * rng.random(N).astype(np.float32)).astype(np.float32)
          for k in range(5)]
    estep("drift", N, [(dr[k], ones(N), {}) for k in [0, 1, 2, 3, 4, 3, 2, 1] * 2])
    # a rougher walk (scale 0.93 .. 1.07, a shift, noise): first rounds that are not accepted and trust regions left
    rng = np.random.default_rng(77)
    r = vec(N, seed=7)
    rough = []
    for _ in range(16):
        r = np.abs(r * np.float32(rng.uniform(0.93, 1.07)) + np.float32(rng.uniform(0.0, 0.05))
                   + (0.02 * rng.standard_normal(N)).astype(np.float32) * (r > 1.0)).astype(np.float32)
        rough.append(r)
    estep("rough walk", N, [(v, ones(N), {}) for v in rough])
    estep("cold_start", N, [(vec(N, seed=2), ones(N), {})] * 3, options={"cold_start": 1})
    r = vec(N, seed=3)
    estep("trace", N, [(r, ones(N), {}), (r, ones(N), {"trace": True}), (r, ones(N), {}), (r, ones(N), {"trace": True})])
    for m in (1, 2, 3):
        estep(f"maxiter {m}", N, [(vec(N, seed=4), ones(N), {"maxiter": m})] * 3)
    estep("verify", N, [(vec(N, seed=5), ones(N), {})] * 3, knobs={"RLVI_TJ_VERIFY": 1})
    for cap in (64, 128):
        estep(f"coop cap {cap}", N, [(vec(N, seed=6), ones(N), {})] * 3, knobs={"RLVI_COOP_CAP": cap})
    for B, C in [(65536, 100), (16384, 100), (4096, 10)]:
        d = synth.mstep_inputs(B, C, seed=B + C)
        zt, yt = torch.from_numpy(d["logits"]).to(dev), torch.from_numpy(d["labels"]).to(dev)
        ws = ops.Workspace(dev, B, B)
        off, nb = ws.region("warm")
        for i in range(3):
            pit = torch.ones(B, device=dev)
            out, grad, rows, iters = ops.fused_em(zt, yt, pit, ws=ws)
            torch.cuda.synchronize()
            st = ws.status()
            ws.clear_status()
            lines.append(f"fused_em {B}x{C} call {i} status {st} iters {int(iters)} pi {sha(pit.cpu().numpy())} "
                         f"grad {sha(grad.cpu().numpy())} rows {sha(rows.cpu().numpy())} out {sha(out.cpu().numpy())} "
                         f"warm {sha(ws.buf[off:off + nb].cpu().numpy())}")
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} lines -> {sys.argv[1]}  (library {_lib.LIB_PATH})")


if __name__ == "__main__":
    main()
