#!/usr/bin/env python3
"""Generate tests/golden/g12_jocor.npz by running the REFERENCE's JoCoR loss and epoch (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_jocor.py [--ref /root/reference]

G12 jocor  loss_jocor, kl_loss_compute, train_jocor   deep-learning/methods/train_jocor.py:17-76

The reference is imported read-only, as oracle/make_golden.py does (whose helpers this uses); the fixture holds
recipes (synth.mstep_inputs(B, C, N=B, seed) for model 1, seed + 1 for model 2, as G8) and the reference's
outputs.  bf16 / fp16 cases round the logits first and feed them to the reference as fp32 (it has no
half-precision path; G3 defines bf16 the same way).  Per case: the loss, K_qp, K_pq, the selection np.argsort
kept (packed bits), the k-th and (k+1)-th smallest loss_pick and their gap, and loss_pick and the gradients of
both blocks on the stored rows (all rows at small shapes, a seeded sample at large ones).  Running it again writes
the same bytes.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as MG  # noqa: E402
from rlvi_amd import synth  # noqa: E402

SHAPES = ((37, 10), (64, 10), (200, 100), (1000, 14), (1024, 101), (4096, 10))
FORGET = (0.0, 0.2, 0.45, 1.0)
EXTRA = ((200, 100, 0.2, 0.35),)          # (B, C, forget_rate, co_lambda != 0.1)
DTYPES = ("f32", "bf16", "f16")
FULL_GRAD_MAX = 1000                      # B * C up to which both gradients are stored whole
SAMPLE_ROWS = 8
LOOP = dict(seed=1212, N=256, B=64, D=16, C=10, epochs=3, forget_rate=0.2, num_gradual=2, lr=0.05, momentum=0.9,
            weight_decay=1e-4, model_seeds=(21, 22))


def case_seed(B, C):
    return 1200 + B + C


def rows_of(B, C, seed):
    """Rows whose gradients a case stores: all of them, or a seeded sample."""
    if B * C <= FULL_GRAD_MAX:
        return np.arange(B)
    return np.sort(np.random.default_rng(seed).choice(B, SAMPLE_ROWS, replace=False))


def rounded(a, dt):
    import torch
    t = torch.from_numpy(a)
    if dt == "bf16":
        t = t.to(torch.bfloat16).float()
    elif dt == "f16":
        t = t.to(torch.float16).float()
    return t.numpy().copy()


class ArgsortSpy:
    """Stands in for the reference module's `np`: records what np.argsort saw and returned."""

    def __init__(self, real):
        self.real, self.seen = real, []

    def __getattr__(self, name):
        return getattr(self.real, name)

    def argsort(self, a, *args, **kw):
        r = self.real.argsort(a, *args, **kw)
        self.seen.append((np.asarray(a, np.float32).copy(), np.asarray(r).copy()))
        return r


def gen_cases(jc):
    import torch
    out, keys = {}, []
    todo = [(B, C, fr, 0.1) for (B, C) in SHAPES for fr in FORGET] + list(EXTRA)
    for dt in DTYPES:
        for (B, C, fr, lam) in todo:
            seed = case_seed(B, C)
            d1 = synth.mstep_inputs(B, C, N=B, seed=seed, zero_frac=0.0)
            d2 = synth.mstep_inputs(B, C, N=B, seed=seed + 1, zero_frac=0.0)
            z1n, z2n = rounded(d1["logits"], dt), rounded(d2["logits"], dt)
            t = torch.from_numpy(d1["labels"])
            z1 = torch.from_numpy(z1n).requires_grad_(True)
            z2 = torch.from_numpy(z2n).requires_grad_(True)
            spy = ArgsortSpy(np)
            jc.np = spy
            try:
                loss = jc.loss_jocor(z1, z2, t, fr, None, co_lambda=lam)
            finally:
                jc.np = np
            loss.backward()
            (pick, order), = spy.seen
            k = int((1 - fr) * B)
            sel = np.zeros(B, bool)
            sel[order[:k]] = True
            s = np.sort(pick)
            gap = float(s[k]) - float(s[k - 1]) if 0 < k < B else np.inf
            with torch.no_grad():
                kqp = jc.kl_loss_compute(z1, z2, reduce='none')
                kpq = jc.kl_loss_compute(z2, z1, reduce='none')
            rows = rows_of(B, C, seed)
            key = f"{dt}_B{B}_C{C}_fr{fr}_lam{lam}"
            keys.append(key)
            out[key + "/shape"] = np.array([B, C, seed], np.int64)
            out[key + "/real"] = np.array([fr, lam], np.float64)
            out[key + "/k"] = np.array(k, np.int64)
            out[key + "/loss"] = np.array(np.float32(loss.item()))
            out[key + "/kl"] = np.array([kqp.item(), kpq.item()], np.float32)
            out[key + "/loss_pick"] = pick[rows].copy()
            out[key + "/edge"] = np.array([s[k - 1] if k > 0 else np.nan, s[k] if k < B else np.nan], np.float32)
            out[key + "/sel_bits"] = np.packbits(sel)
            out[key + "/gap"] = np.array(gap, np.float64)
            out[key + "/rows"] = rows.astype(np.int64)
            out[key + "/grad1"] = z1.grad.numpy()[rows].copy()
            out[key + "/grad2"] = z2.grad.numpy()[rows].copy()
        print(f"g12 {dt}: {len(todo)} cases", flush=True)
    out["cases"] = np.array(keys)
    return out


def gen_loop(jc):
    """Three epochs of the reference's train_jocor: two seeded nn.Linear(16, 10) through ONE SGD optimizer over both
    parameter lists (main.py:228-231), rate_schedule as main.py:172-180, batches in a fixed order."""
    import torch
    p = LOOP
    X, y = synth.jocor_loop_inputs(p["seed"], p["N"], p["D"], p["C"])
    loader = [(torch.from_numpy(X[s:s + p["B"]]), torch.from_numpy(y[s:s + p["B"]]),
               torch.arange(s, min(s + p["B"], p["N"]))) for s in range(0, p["N"], p["B"])]
    models = []
    for ms in p["model_seeds"]:
        torch.manual_seed(ms)
        models.append(torch.nn.Linear(p["D"], p["C"]))
    m1, m2 = models
    out = {"loop/init": np.concatenate([q.detach().numpy().ravel() for m in models for q in m.parameters()])}
    opt = torch.optim.SGD(list(m1.parameters()) + list(m2.parameters()), lr=p["lr"], momentum=p["momentum"],
                          weight_decay=p["weight_decay"])
    rs = synth.jocor_rate_schedule(p["forget_rate"], p["epochs"] + 1, p["num_gradual"])
    params, accs = [], []
    for epoch in range(1, p["epochs"] + 1):
        accs.append(jc.train_jocor(loader, epoch, m1, m2, opt, rs))
        params.append(np.concatenate([q.detach().numpy().ravel() for m in models for q in m.parameters()]))
    out["loop/params"] = np.stack(params)
    out["loop/train_acc"] = np.array(accs, np.float64)
    out["loop/rate_schedule"] = rs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    import torch
    torch.set_num_threads(1)                 # (the reference's reductions: one summation order)
    MG.ref_deep(a.ref)
    jc = sys.modules["methods.train_jocor"]
    out = gen_cases(jc)
    out.update(gen_loop(jc))
    # the reference's public names and argument lists (name=default), for the mirror's interface test
    import inspect
    out["ref/all"] = np.array(jc.__all__)
    for fn in ("kl_loss_compute", "loss_jocor", "train_jocor"):
        ps = inspect.signature(getattr(jc, fn)).parameters.values()
        out["ref/sig/" + fn] = np.array([q.name if q.default is q.empty else f"{q.name}={q.default!r}" for q in ps])
    MG.save_deterministic("g12_jocor", **out)


if __name__ == "__main__":
    main()
