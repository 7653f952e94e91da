#!/usr/bin/env python3
"""Generate tests/golden/g14_bare.npz by running the REFERENCE's BARE loss and the two plain loops (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_bare.py [--ref /root/reference]

G14 bare  WeightedCCE, train_bare, train_regular   deep-learning/methods/train_bare.py:15-82, train_regular.py:15-36

The reference is imported read-only, as oracle/make_golden.py does (whose helpers this uses); the fixture holds
recipes (synth.mstep_inputs / synth.bare_dense_inputs and a seed; the labels themselves only for the adversarial
cases, whose labels are built from the batch statistics) and the reference's outputs.  bf16 / fp16 cases round the
logits first and feed them to the reference as fp32 (it has no half-precision path; G3 and G12 do the same).

Per case: the rows the reference kept (packed bits; read off its torch.index_select call), their number, the fallback
flag (no index_select call: nothing was kept and the plain mean ran), the loss, the gradient of loss.mean() on the
stored rows, and the fp64 margin pt - mu[y] - k * sd[y] of every row as fp32.  A row is PINNED when its margin is
further than PIN = 2^-18 from zero (64 fp32 ulp of 1.0, the largest quantity in the comparison; fp32 rounding of pt,
mu and sd stays below 2^-22 each); a NaN margin (B = 1: the unbiased deviation of one value) is pinned too, the
comparison being false whatever the rounding.  At most 1 % of a case's rows may be unpinned; a case without any is
marked `full` and is the only kind on which loss and gradients are compared.  Running it again writes the same bytes.
"""
import argparse
import inspect
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as MG  # noqa: E402
from rlvi_amd import synth  # noqa: E402

PIN = 2.0 ** -18
UNPINNED_CAP = 0.01
SHAPES = ((37, 10), (64, 10), (200, 100), (1000, 14), (1024, 101), (4096, 10))
DENSE = ((37, 10, 0.5), (64, 10, 0.05), (200, 100, 0.5), (1000, 14, 1.0), (1024, 101, 0.2), (4096, 10, 0.02),
         (4097, 1023, 0.5))
# the dense case at 4097 x 1023 always has a few rows inside PIN (softmax entries of 1e-3, 4097 of them), and loss and
# gradients are compared on fully pinned cases only: a bimodal case gives that shape one (first seed that is)
EXTRA_BIMODAL = ((4097, 1023),)
ADVERSARIAL = ((64, 10), (1000, 14))
TINY = (1, 2)                             # B of the two smallest fallback cases, C = 10
UNBIASED_B = (3, 4, 5, 16)
DTYPES = ("f32", "bf16", "f16")
FULL_GRAD_MAX = 1000                      # B * C up to which the gradient is stored whole
SAMPLE_ROWS = 8
SEED_TRIES = 200
LOOP = dict(seed=1414, N=256, B=64, D=16, C=10, epochs=3, lr=0.05, momentum=0.9, weight_decay=1e-4, model_seed=21)


def rows_of(B, C, seed, grad, n_kept):
    """Rows whose gradients a case stores: all of them, or a seeded sample of SAMPLE_ROWS.  The sample must hold an
    entry of at least 0.1 / n_kept: the tests' absolute tolerance is 1e-5 of the largest stored entry, and the
    reference's own fp32 rounding of softmax - onehot is about 2^-24 / n_kept per entry -- a sample of confidently
    classified rows alone (entries of 1e-3 / n_kept and less) would put the bar below the reference's own error.
    The sample's seed counts up from the case's until it does."""
    if B * C <= FULL_GRAD_MAX:
        return np.arange(B)
    for s in range(seed, seed + SEED_TRIES):
        rows = np.sort(np.random.default_rng(s).choice(B, SAMPLE_ROWS, replace=False))
        if np.abs(grad[rows]).max() >= 0.1 / n_kept:
            return rows
    raise SystemExit(f"no row sample with a gradient entry of 0.1 / n_kept at {B} x {C}")


def rounded(a, dt):
    import torch
    t = torch.from_numpy(a)
    if dt == "bf16":
        t = t.to(torch.bfloat16).float()
    elif dt == "f16":
        t = t.to(torch.float16).float()
    return t.numpy().copy()


def stats64(z):
    """fp64 clamped softmax of fp32 logits and its column mean / deviations (unbiased, biased)."""
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    p = np.clip(e / e.sum(1, keepdims=True), 1e-8, 1 - 1e-8)
    B = z.shape[0]
    mu = p.mean(0)
    ss = ((p - mu) ** 2).sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return p, mu, np.sqrt(ss / (B - 1)), np.sqrt(ss / B)


def margins64(z, y, k, biased=False):
    p, mu, sd, sd0 = stats64(z)
    s = sd0 if biased else sd
    return p[np.arange(len(y)), y] - mu[y] - k * s[y]


def is_pinned(margin):
    return ~(np.abs(margin) <= PIN)       # NaN counts as pinned (see the module docstring)


class IndexSelectSpy:
    """Stands in for the reference module's `torch`: records the index of every torch.index_select."""

    def __init__(self, real):
        self.real, self.seen = real, []

    def __getattr__(self, name):
        return getattr(self.real, name)

    def index_select(self, a, dim, index):
        self.seen.append(index.detach().numpy().copy())
        return self.real.index_select(a, dim, index)


def run_reference(bare, zn, y, k, C):
    """The reference's WeightedCCE as train_bare uses it (reduction='none', then .mean()): loss, gradient, kept rows,
    fallback flag."""
    import torch
    z = torch.from_numpy(zn).requires_grad_(True)
    spy = IndexSelectSpy(torch)
    bare.torch = spy
    try:
        loss = bare.WeightedCCE(k=k, num_class=C, reduction="none")(z, torch.from_numpy(y))
    finally:
        bare.torch = torch
    loss.mean().backward()
    B = zn.shape[0]
    sel = np.zeros(B, bool)
    fallback = not spy.seen
    if fallback:
        sel[:] = True
    else:
        assert len(spy.seen) == 2 and np.array_equal(spy.seen[0], spy.seen[1])
        sel[spy.seen[0]] = True
    return float(loss.mean().item()), z.grad.numpy().copy(), sel, fallback


def adversarial_labels(z):
    p, mu, sd, _ = stats64(z)
    return np.argmin(p - mu - sd, axis=1).astype(np.int64)


def recipe(kind, B, C, scale, seed):
    """fp32 logits and labels of a case before rounding (tests/test_bare_cpu.py restates this from the stored
    kind, shape, scale and seed)."""
    if kind == "bimodal":
        d = synth.mstep_inputs(B, C, N=B, seed=seed, zero_frac=0.0)
        return d["logits"], d["labels"]
    return synth.bare_dense_inputs(B, C, scale, seed)


def gen_cases(bare):
    out, keys = {}, []

    def emit(dt, kind, B, C, scale, seed, k, zn, y, store_labels=False, expect_fallback=None):
        L, grad, sel, fallback = run_reference(bare, zn, y, k, C)
        m = margins64(zn, y, k)
        pin = is_pinned(m)
        unp = int((~pin).sum())
        assert unp <= UNPINNED_CAP * B, (dt, kind, B, C, unp)
        # on pinned rows the reference's fp32 run and the fp64 margins agree
        want = np.ones(B, bool) if fallback else (m >= 0)
        assert np.array_equal(sel[pin], want[pin]), (dt, kind, B, C)
        if expect_fallback is not None:
            assert fallback == expect_fallback, (dt, kind, B, C)
        rows = rows_of(B, C, seed, grad, B if fallback else int(sel.sum()))
        key = f"{dt}_{kind}_B{B}_C{C}" + ("" if k == 1 else f"_k{k}")
        assert key not in keys
        keys.append(key)
        out[key + "/kind"] = np.array(kind)
        out[key + "/shape"] = np.array([B, C, seed], np.int64)
        out[key + "/real"] = np.array([k, scale], np.float64)
        out[key + "/loss"] = np.array(np.float32(L))
        out[key + "/n_kept"] = np.array(B if fallback else int(sel.sum()), np.int64)
        out[key + "/fallback"] = np.array(int(fallback), np.int64)
        out[key + "/sel_bits"] = np.packbits(sel)
        out[key + "/margin"] = m.astype(np.float32)
        out[key + "/unpinned"] = np.array(unp, np.int64)
        out[key + "/full"] = np.array(int(unp == 0), np.int64)
        out[key + "/rows"] = rows.astype(np.int64)
        out[key + "/grad"] = grad[rows].copy()
        if store_labels:
            out[key + "/labels"] = y.astype(np.int16)
        return unp == 0

    for dt in DTYPES:
        n0 = len(keys)
        for (B, C) in SHAPES:
            seed = 1400 + B + C
            z, y = recipe("bimodal", B, C, 0.0, seed)
            emit(dt, "bimodal", B, C, 0.0, seed, 1, rounded(z, dt), y)
        for (B, C) in EXTRA_BIMODAL:
            for seed in range(1400 + B + C, 1400 + B + C + SEED_TRIES):
                z, y = recipe("bimodal", B, C, 0.0, seed)
                if is_pinned(margins64(rounded(z, dt), y, 1)).all():
                    break
            else:
                raise SystemExit(f"no fully pinned bimodal seed at {B} x {C} {dt}")
            assert emit(dt, "bimodal", B, C, 0.0, seed, 1, rounded(z, dt), y)
        for (B, C, scale) in DENSE:
            seed = 1450 + B + C
            z, y = recipe("dense", B, C, scale, seed)
            emit(dt, "dense", B, C, scale, seed, 1, rounded(z, dt), y)
        for B in TINY:
            seed = 1470 + B
            z, y = recipe("tiny", B, 10, 1.0, seed)
            assert emit(dt, "tiny", B, 10, 1.0, seed, 1, rounded(z, dt), y, expect_fallback=True)
        for (B, C) in ADVERSARIAL:
            seed = 1480 + B + C
            z, _ = recipe("adversarial", B, C, 3.0, seed)
            zn = rounded(z, dt)
            y = adversarial_labels(zn)
            assert margins64(zn, y, 1).max() < -0.1
            assert emit(dt, "adversarial", B, C, 3.0, seed, 1, zn, y, store_labels=True, expect_fallback=True)
        z, y = recipe("dense", 200, 100, 0.5, 1450 + 300)
        emit(dt, "khalf", 200, 100, 0.5, 1450 + 300, 0.5, rounded(z, dt), y)
        for B in UNBIASED_B:
            for seed in range(1500, 1500 + SEED_TRIES):
                z, y = recipe("unbiased", B, 10, 1.5, seed)
                zn = rounded(z, dt)
                m1, m0 = margins64(zn, y, 1), margins64(zn, y, 1, biased=True)
                kept = m1 >= 0
                # fully pinned under either divisor, a row that flips between them, and no fallback either way
                if (is_pinned(m1).all() and is_pinned(m0).all() and ((m1 >= 0) != (m0 >= 0)).any() and kept.any()
                        and (m0 >= 0).any()):
                    break
            else:
                raise SystemExit(f"no seed for the unbiased-deviation case B={B} {dt}")
            assert emit(dt, "unbiased", B, 10, 1.5, seed, 1, zn, y, expect_fallback=False)
        print(f"g14 {dt}: {len(keys) - n0} cases", flush=True)
    out["cases"] = np.array(keys)
    by_shape = {}
    for key in keys:
        by_shape.setdefault(tuple(out[key + "/shape"][:2]), []).append(int(out[key + "/full"]))
    for shape, flags in by_shape.items():
        assert any(flags), f"no fully pinned case at {shape}"
    return out


def params_of(model):
    return np.concatenate([q.detach().numpy().ravel() for q in model.parameters()])


def gen_loop(bare, regular):
    """Three epochs of the reference's train_bare and train_regular on a seeded nn.Linear(16, 10), batches in a fixed
    order.  The data seed is the first one at which every batch of the BARE run is fully pinned."""
    import torch
    p = LOOP
    for seed in range(p["seed"], p["seed"] + SEED_TRIES):
        X, y = synth.jocor_loop_inputs(seed, p["N"], p["D"], p["C"])
        loader = [(torch.from_numpy(X[s:s + p["B"]]), torch.from_numpy(y[s:s + p["B"]]),
                   torch.arange(s, min(s + p["B"], p["N"]))) for s in range(0, p["N"], p["B"])]
        res = {}
        ok = True
        for name in ("bare", "regular"):
            torch.manual_seed(p["model_seed"])
            model = torch.nn.Linear(p["D"], p["C"])
            res[name + "_init"] = params_of(model)
            opt = torch.optim.SGD(model.parameters(), lr=p["lr"], momentum=p["momentum"],
                                  weight_decay=p["weight_decay"])
            seen = []
            model.register_forward_hook(lambda mod, inp, o: seen.append(o.detach().numpy().copy()))
            params, accs = [], []
            for _ in range(p["epochs"]):
                if name == "bare":
                    accs.append(bare.train_bare(loader, model, opt, p["C"]))
                else:
                    accs.append(regular.train_regular(loader, model, opt))
                params.append(params_of(model))
            if name == "bare":
                for i, z in enumerate(seen):
                    yb = loader[i % len(loader)][1].numpy()
                    m = margins64(z, yb, 1)
                    ok = ok and bool(is_pinned(m).all()) and bool((m >= 0).any())
            res[name + "_params"] = np.stack(params)
            res[name + "_acc"] = np.array(accs, np.float64)
        if ok:
            break
    else:
        raise SystemExit("no loop seed with fully pinned batches")
    out = {"loop/seed": np.array(seed, np.int64)}
    for k, v in res.items():
        out["loop/" + k] = v
    return out


def signature_names(fn):
    ps = inspect.signature(fn).parameters.values()
    return np.array([q.name if q.default is q.empty else f"{q.name}={q.default!r}" for q in ps])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    import torch
    torch.set_num_threads(1)                 # (the reference's reductions: one summation order)
    MG.ref_deep(a.ref)
    bare, regular = sys.modules["methods.train_bare"], sys.modules["methods.train_regular"]
    out = gen_cases(bare)
    out.update(gen_loop(bare, regular))
    out["pin"] = np.array(PIN, np.float64)
    # the reference's public names and argument lists (name=default), for the mirrors' interface test
    out["ref/all"] = np.array(bare.__all__)
    out["ref/all_regular"] = np.array(regular.__all__)
    out["ref/methods"] = np.array(sorted(n for n in dir(sys.modules["methods"]) if n.startswith("train_")))
    out["ref/sig/WeightedCCE.__init__"] = signature_names(bare.WeightedCCE.__init__)
    out["ref/sig/WeightedCCE.forward"] = signature_names(bare.WeightedCCE.forward)
    out["ref/sig/train_bare"] = signature_names(bare.train_bare)
    out["ref/sig/train_regular"] = signature_names(regular.train_regular)
    MG.save_deterministic("g14_bare", **out)


if __name__ == "__main__":
    main()
