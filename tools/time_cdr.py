"""CDR's gradient masking on one MI355X: the HIP path (ops.CdrMasker, rlvi_amd/csrc/cdr.hip) against
(a) the reference's statements (deep-learning/methods/train_cdr.py:22-44) as eager torch ops on the same device and
    the same inputs -- the two torch.cat, abs(g * v), torch.topk(metric, nz), and per tensor the product, compare,
    cast, scale and multiply;
(b) rlvi_stream_copy moving the least bytes the task needs: g and v read once to select, then g and v read and g
    written to apply -- 20 P bytes for P parameters (a copy of 10 P bytes reads and writes that much).

    python tools/time_cdr.py [--reps 30] [--shapes lenet,resnet18,resnet50,seg64m] [--no-epoch]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/time_cdr.py --shapes resnet18 --no-epoch --ours-only

Per shape one JSON line: the median time per call from device events around each call (the gradients are restored
from a saved copy between calls, outside the timed span, so every call sees the same inputs), and our time as a
multiple of (b).  Then one epoch of train_cdr on the LeNet driver configuration (16 384 synthetic digits, batches of
1024) against the same statements as stock torch.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlvi_amd import driver, ops  # noqa: E402

RATIO = 0.7


def resnet50_shapes(num_classes=10):
    """The conv and fc weights of a ResNet-50 (bottlenecks 3-4-6-3, expansion 4): about 23.5 M values."""
    shapes, cin = [(64, 3, 7, 7)], 64
    for planes, n in ((64, 3), (128, 4), (256, 6), (512, 3)):
        for j in range(n):
            shapes += [(planes, cin, 1, 1), (planes, planes, 3, 3), (4 * planes, planes, 1, 1)]
            if j == 0:
                shapes.append((4 * planes, cin, 1, 1))
            cin = 4 * planes
    return shapes + [(num_classes, cin)]


def shape_list(name):
    if name == "lenet":
        return [tuple(p.shape) for p in driver.LeNet().parameters() if p.dim() in (2, 4)]
    if name == "resnet18":
        return [tuple(p.shape) for p in driver.ResNet18().parameters() if p.dim() in (2, 4)]
    if name == "resnet50":
        return resnet50_shapes()
    if name == "seg64m":
        return [(1, 64 * 1024 * 1024)]
    raise ValueError(name)


def make_params(shapes, dev, seed=0):
    gen = torch.Generator(device=dev).manual_seed(seed)
    params, saved = [], []
    for s in shapes:
        fan = int(np.prod(s[1:]))
        p = torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) / fan ** 0.5)
        g = torch.randn(s, device=dev, generator=gen) * torch.exp(2 * torch.randn(s, device=dev, generator=gen)) * 1e-3
        p.grad = g
        params.append(p)
        saved.append(g.clone())
    return params, saved


def reference_mask(params, nonzero_ratio, clip):
    """train_cdr.py:22-44 on a parameter list."""
    all_g = torch.cat([p.grad.data.view(-1) for p in params])
    all_v = torch.cat([p.data.view(-1) for p in params])
    metric = torch.abs(all_g * all_v)
    nz = int(nonzero_ratio * all_v.size(0))
    top_values, _ = torch.topk(metric, nz)
    thresh = top_values[-1]
    for p in params:
        mask = (torch.abs(p.data * p.grad.data) >= thresh).type(torch.float32)
        mask = mask * clip
        p.grad.data = mask * p.grad.data
    return thresh


def per_call_us(fn, restore, reps, warm=3):
    times = []
    for i in range(warm + reps):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times)), float(np.min(times))


def copy_us(nbytes, dev, reps):
    nbytes = (nbytes + 15) // 16 * 16
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)
    return per_call_us(lambda: ops.stream_copy(dst, src), lambda: None, reps)[0]


def time_shape(name, dev, reps, ours_only=False):
    params, saved = make_params(shape_list(name), dev)
    P = sum(p.numel() for p in params)

    def restore():
        for p, g in zip(params, saved):
            p.grad.copy_(g)

    masker = ops.CdrMasker(params)
    ours, ours_min = per_call_us(lambda: masker(RATIO, RATIO), restore, reps)
    thr_ours = float(masker.thr)
    row = {"shape": name, "tensors": len(params), "params": P, "ratio": RATIO,
           "ours_us": round(ours, 1), "ours_min_us": round(ours_min, 1), "table_uploads": masker.uploads}
    if not ours_only:
        ref_reps = max(reps // 3, 5)
        ref, _ = per_call_us(lambda: reference_mask(params, RATIO, RATIO), restore, ref_reps)
        restore()
        thr_ref = float(reference_mask(params, RATIO, RATIO))
        assert thr_ref == thr_ours, (thr_ref, thr_ours)
        cp = copy_us(10 * P, dev, reps)
        row.update({"reference_eager_us": round(ref, 1), "speedup": round(ref / ours, 1),
                    "copy_20P_bytes_us": round(cp, 1), "ours_over_copy": round(ours / cp, 2),
                    "min_bytes": 20 * P})
    print(json.dumps(row), flush=True)


def stock_epoch(loader, model, opt, clip, dev):
    import torch.nn.functional as F
    correct, total = 0, 0
    for data, labels, _ in loader:
        data, labels = data.to(dev), labels.to(dev)
        logits = model(data)
        _, pred = F.softmax(logits, dim=1).topk(5, 1, True, True)
        hit = pred.t().eq(labels.view(1, -1).expand_as(pred.t()))
        correct += hit[:1].reshape(-1).float().sum(0, keepdim=True).mul_(100.0 / labels.size(0))
        total += 1
        model.train()
        loss = torch.nn.CrossEntropyLoss()(model(data), labels)
        loss.backward()
        reference_mask([p for p in model.parameters() if p.dim() in (2, 4)], clip, clip)
        opt.step()
        opt.zero_grad()
    return float(correct) / float(total)


def time_epoch(dev, epochs=5):
    """One train_cdr epoch of the LeNet driver configuration, ours and stock, alternating; host clock around a
    synchronised epoch, the median of `epochs`."""
    import time
    from rlvi_amd.methods import train_cdr
    x, y, _, _ = driver.synthetic_digits(16384, seed=0)
    x, y = x.to(dev), y.to(dev)
    loader = driver.IndexedLoader(x, y, 1024, shuffle=False)
    rs = np.full(epochs + 1, 0.3)
    out = {}
    models = {}
    for who in ("ours", "ours_reuse_forward", "stock", "stock_again"):
        torch.manual_seed(3)
        m = driver.LeNet().to(dev)
        models[who] = (m, torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9), [])
    for e in range(epochs + 1):
        for who, (m, opt, ts) in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if who.startswith("stock"):
                stock_epoch(loader, m, opt, 1 - rs[e], dev)
            else:
                train_cdr(loader, e, m, opt, rs, reuse_forward=who != "ours")
            torch.cuda.synchronize()
            if e > 0:
                ts.append((time.perf_counter() - t0) * 1e3)
    for who, (m, opt, ts) in models.items():
        out[who + "_epoch_ms"] = round(float(np.median(ts)), 2)
    same = all(torch.equal(a, b) for a, b in zip(models["ours"][0].parameters(), models["stock"][0].parameters()))
    out["ours_equals_stock_bitwise"] = bool(same)
    # (the convolutions' backward may not repeat its own bits: two stock runs tell)
    out["stock_equals_stock_bitwise"] = all(torch.equal(a, b) for a, b in zip(models["stock"][0].parameters(),
                                                                              models["stock_again"][0].parameters()))
    print(json.dumps({"train_cdr_lenet_16384x1024": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shapes", default="lenet,resnet18,resnet50,seg64m")
    ap.add_argument("--no-epoch", action="store_true")
    ap.add_argument("--ours-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in a.shapes.split(","):
        time_shape(name, dev, a.reps, a.ours_only)
        torch.cuda.empty_cache()
    if not a.no_epoch:
        time_epoch(dev)


if __name__ == "__main__":
    main()
