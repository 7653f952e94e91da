#!/usr/bin/env python3
"""Times single legs of the hot path (HIP events, hipGraph of K launches, rotating buffers).
Used for kernel tuning sweeps:  RLVI_MSTEP_U=2 python tools/time_parts.py --what mstep"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from rlvi_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--what", default="mstep", choices=["mstep", "mstep_warm", "mstep_out", "estep", "thr", "thr_fn", "fused", "mstep_fwd", "step"])
ap.add_argument("--rows", type=int, default=65536)
ap.add_argument("--classes", type=int, default=100)
ap.add_argument("--n", type=int, default=0, help="E-step / threshold vector length (default rows)")
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--dtype", default="f32", choices=["f32", "bf16", "f16"])
ap.add_argument("--tag", default="")
ap.add_argument("--seq-idx", action="store_true", help="sample indices in order instead of a permutation (lab: what the random gather / scatter costs)")
ap.add_argument("--tune", action="append", default=[], help="NAME=VALUE knob (rlvi_tune_set); repeatable")
ap.add_argument("--sweep", default="", help="NAME=v1,v2,...: time the leg once per value")
a = ap.parse_args()
dev = torch.device("cuda:0")
B, C = a.rows, a.classes
N = a.n or B
d0, labels, idx, logits, grads, weights, residuals = bench.make_inputs(torch, dev, B, C, B, 0)
if a.seq_idx:
    idx = torch.arange(B, device=dev, dtype=torch.int64)
if a.dtype in ("bf16", "f16"):
    tdt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    logits = [z.to(tdt) for z in logits]
    grads = [g.to(tdt) for g in grads]
if N != B:
    from rlvi_amd import synth
    residuals_n = torch.from_numpy(synth.residual_vector("bimodal", N, 1)).to(dev)
    weights_n = torch.rand(N, device=dev) if a.what in ("thr", "thr_fn") else torch.ones(N, device=dev)
out = torch.empty(4, device=dev)
iters = torch.zeros(1, dtype=torch.int32, device=dev)
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    ws = ops.Workspace(dev, max(N, B), B)
    if N == B:
        ops.mstep_fwd_bwd(logits[0], labels, idx, weights, residuals, out=out, grad=grads[0], ws=ws)
        res_src = residuals.clone()
    else:
        res_src = residuals_n.clone()
        residuals, weights = residuals_n, weights_n
    pi = torch.ones(B, device=dev)
    rows = torch.empty(B, device=dev)
    thr = torch.zeros(1, device=dev)

    def leg(i):
        r = i % bench.ROTATE
        if a.what == "mstep":
            ops.mstep_fwd_bwd(logits[r], labels, idx, weights, residuals, grad=grads[r], ws=ws, accumulate=True)
        elif a.what == "mstep_warm":       # one buffer pair: the block stays in the Infinity Cache
            ops.mstep_fwd_bwd(logits[0], labels, idx, weights, residuals, grad=grads[0], ws=ws, accumulate=True)
        elif a.what == "mstep_out":
            ops.mstep_fwd_bwd(logits[r], labels, idx, weights, residuals, out=out, grad=grads[r], ws=ws)
        elif a.what == "step":
            ops.mstep_fwd_bwd(logits[r], labels, idx, weights, residuals, grad=grads[r], ws=ws, accumulate=True)
            ops.epoch_end(residuals, weights, batches=1, out=out, iters=iters, ws=ws)
        elif a.what == "mstep_fwd":
            ops.mstep_fwd_bwd(logits[r], labels, idx, weights, residuals, out=out, want_grad=False, ws=ws)
        elif a.what == "estep":
            residuals.copy_(res_src)
            ops.estep_deep(residuals, weights, iters=iters, ws=ws)
        elif a.what == "thr":
            from rlvi_amd import _lib
            L = _lib.load()
            _lib.check(L.rlvi_threshold_truncate_f32(ops._ptr(weights), weights.shape[0], 0.05, ops._ptr(thr),
                                                     None, None, ws.ptr, ops._stream_ptr()), "thr")
        elif a.what == "thr_fn":           # the criterion alone: the vector is left as it is (no zeros from a truncation)
            from rlvi_amd import _lib
            L = _lib.load()
            _lib.check(L.rlvi_fn_threshold_f32(ops._ptr(weights), weights.shape[0], 0.05, ops._ptr(thr),
                                               ws.ptr, ops._stream_ptr()), "thr")
        elif a.what == "fused":
            ops.fused_em(logits[r], labels, pi, ws=ws, out=out, grad=grads[r], rows=rows, iters=iters)
    from rlvi_amd import _lib as _L
    for kv in a.tune:
        k, v = kv.split("=")
        _L.check(_L.load().rlvi_tune_set(k.encode(), int(v)), "rlvi_tune_set")

    def time_leg():
        for i in range(12):
            leg(i)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for i in range(a.steps):
                leg(i)
        torch.cuda.synchronize()
        best = 1e9
        reps = []
        for rep in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            g.replay()
            e1.record(side)
            torch.cuda.synchronize()
            reps.append(e0.elapsed_time(e1) / a.steps * 1e3)
            best = min(best, reps[-1])
        print("   reps:", " ".join(f"{r:.2f}" for r in reps), flush=True)
        return best

    def describe(best):
        extra = ""
        if a.what in ("mstep", "mstep_warm", "mstep_fwd", "mstep_out"):
            s = 2 if a.dtype in ("bf16", "f16") else 4
            byt = B * ((1 if a.what == "mstep_fwd" else 2) * C * s + 24)
            extra = f" {byt / best / 1e3:8.1f} GB/s  frac {byt / best / 1e3 / 8000:.3f}"
        if a.what in ("estep", "fused", "step"):
            extra = f" iters {int(iters)}"
        return extra

    if a.sweep:
        name, vals = a.sweep.split("=")
        for v in vals.split(","):
            _L.check(_L.load().rlvi_tune_set(name.encode(), int(v)), "rlvi_tune_set")
            best = time_leg()
            print(f"{a.tag or a.what:20s} {name}={v:>5s} B={B} C={C} N={N} {a.dtype}: {best:8.2f} us/launch"
                  f"{describe(best)}  status={ws.status()}", flush=True)
        sys.exit(0)
    best = time_leg()
    extra = describe(best)
    if a.what in ("thr", "thr_fn") and any(t.startswith("RLVI_THR_DEBUG") for t in a.tune):
        import stamps
        print("thr stamps (us since kernel start):", stamps.us(stamps.read(ws).seq("THR_SEQ", "THR_COUNT")))
    if os.environ.get("RLVI_TJ_DEBUG"):
        import stamps
        S = stamps.read(ws)
        st = S.seq("SOLVE_SEQ", "SOLVE_COUNT")
        t0 = int(st[0])

        def at(name, i=0):       # a wall-clock stamp on the solve's axis: us since its first stamp
            return stamps.us(S.word(name, i), t0)[0]
        print("stamps (us since kernel start):", stamps.us(st)[:16])
        if a.what == "fused":
            fs = S.ticks("FUSED_SEQ")
            print("fused stamps [start, tiles landed, rows done, barrier, solved, grad issued, -, out] us:",
                  [u if x else None for u, x in zip(stamps.us(fs), fs)], " solve starts at", stamps.us(t0, fs[0])[0])
        print('finite mask %x scale' % S.word("TJ_FINITE"), stamps.f32(stamps.lo(S["TJ_SCALE"])), 'totals lanes0-7 (S,P,D):', S.f64("TJ_TOTALS").reshape(8, 3))
        it, delta = S.pair("TJ_IT_DELTA")
        print('round_ok', S.word("TJ_ROUND_OK"), 'it', int(it[0]), 'delta', stamps.f32(delta))
        rn, rnew = S.f32_pair("TJ_NODES")
        print('rn  :', rn[:44])
        print('rnew:', rnew[:44])
        nq, tmin = S.pair("SOLVE_TOTALS_MIN")
        print("  wmin stored (wg0):", stamps.f32(stamps.lo(S["SOLVE_WMIN"])), " totals val[4] lanes 0..3:", stamps.f32(tmin[:4].copy()), "nq", int(nq[0]))
        sk, rho = S.f32_pair("TJ_SK_RHO")
        print("  s_k    :", sk[:24])
        print("  rho_k  :", rho[:24])
        acc, it_acc = S.pair("TJ_ACCEPT")
        print("accept-without-verification:", int(acc[0]), "it", int(it_acc[0]))
        err_est, band = S.f32_pair("TJ_ERR_BAND")
        print("  err_est:", err_est[:24])
        print("  band   :", band[:24])
        ek, slope = S.f32_pair("TJ_EK_SLOPE")
        print("  E_k    :", ek[:24])
        print("  slope  :", slope[:24])
        cs = S.ticks("CHAIN_SEQ")
        print("recurrence wave [entry, prepared, chain, trust/tail, acceptance, out] us:", stamps.us(cs))
        if S.word("HELPER") > 0:      # (the split acceptance test: the helper wave between the recurrence wave's two barriers)
            print("   helper wave [start, done] and the recurrence wave past its second barrier, us on the same axis:",
                  stamps.us(list(S.ticks("HELPER")) + [S.word("CHAIN_BARRIER2")], cs[0]))
        if S.word("RED_BARRIER") > 0 and S.word("RED_PUBLISH") > 0:
            print(f"reducer of node 0: behind its barrier at {at('RED_BARRIER'):.2f}, granule in hand at "
                  f"{at('RED_PUBLISH'):.2f} us since kernel start: combine {(S.word('RED_PUBLISH') - S.word('RED_BARRIER')) / 100.0:.2f} us")
        # the kernel's entry on the stamps' axis: stamped as its first instruction (ENTRY: entry, first data loads
        # issued, slice landed); a build without these has the kernel's length from its entry (KERNEL_TICKS), taken at the
        # last stamp, and its first two stamps sit behind the issue of the slice loads and behind their arrival
        n, ticks = len(st), S.word("KERNEL_TICKS")
        if S.word("ENTRY") > 0:
            e = [int(x) for x in S.ticks("ENTRY")]
            print(f"kernel entry at {at('ENTRY', 0):.2f}, first data loads issued at {at('ENTRY', 1):.2f}, "
                  f"slice landed at {at('ENTRY', 2):.2f} us on the stamps' axis: entry -> issued "
                  f"{(e[1] - e[0]) / 100.0:.2f} us, entry -> slice landed {(e[2] - e[0]) / 100.0:.2f} us")
        elif ticks > 0 and n > 1:
            e0 = int(st[n - 1]) - ticks
            print(f"kernel entry (last stamp - kernel length) at {(e0 - t0) / 100.0:.2f} us on the stamps' axis: entry -> first "
                  f"stamp (behind the issue of the slice loads) {(t0 - e0) / 100.0:.2f} us, entry -> slice landed "
                  f"(second stamp) {(int(st[1]) - e0) / 100.0:.2f} us")
        if S.word("SUMS_ARITH") > 0:
            print("sums of workgroup 0 / wave 0: arithmetic done at", at("SUMS_ARITH"),
                  "butterflies done at", at("SUMS_BFLY"), "us since kernel start")
        if S.word("SUMS_CYCLES") > 0 and S.word("SUMS_ARITH") > S.word("STAGED_CLOCK"):
            print(f"   shader clock from the staged slice to the end of the sums' arithmetic: "
                  f"{(S.word('SUMS_CYCLES') - S.word('STAGED_CYCLES')) / (S.word('SUMS_ARITH') - S.word('STAGED_CLOCK')) * 0.1:.2f} GHz")
        if ticks > 0:
            cycles = S.word("KERNEL_CYCLES")
            print(f"shader clock in the E-step kernel: {cycles / ticks * 0.1:.2f} GHz "
                  f"({cycles} cycles in {ticks / 100.0:.2f} us)")
        keit, delta = S.pair("SOLVE_ROUNDS")
        print("rounds (it, delta):", [(int(k), float(d)) for k, d, x in zip(keit, stamps.f32(delta), S["SOLVE_ROUNDS"]) if x][:12])
    print(f"{a.tag or a.what:28s} B={B} C={C} N={N} {a.dtype}: {best:8.2f} us/launch{extra}  status={ws.status()}")
