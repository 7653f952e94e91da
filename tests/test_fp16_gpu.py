"""fp16 logits on the MI355X (run with -m gpu): the M-step in every kernel form, the loss scale read on the device,
precision@k, the plug-in epoch under autocast and with a GradScaler, and the driver's --amp fp16.

The target is the one the bf16 path has: the oracle fed the fp16 logits widened to fp32, its gradient rounded to
fp16 (storage precision).  Residuals and loss keep the fp32 bars; hits are exact; the gradient is within one fp16
ulp (2^-10 relative) or 2^-24 absolute (the smallest fp16 subnormal).
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from rlvi_amd import synth
from test_oracle_golden import REL, rel_pi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16_RTOL, F16_ATOL = 2 ** -10, 2 ** -24
F16_MAX, F16_MIN_NORMAL = 65504.0, 2 ** -14


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rlvi_amd import _lib, ops
    _lib.load()
    return torch, ops, torch.device("cuda:0")


@pytest.fixture(autouse=True)
def no_process_state_left_behind():
    """No test leaves a knob set, a sticky status or accumulate-mode records behind (later tests would see them)."""
    yield
    import torch
    if not torch.cuda.is_available():
        return
    from rlvi_amd import _lib, ops
    left = [n for n in _lib.tune_overrides() if n != "RLVI_DEVICE_SHARERS"]
    for name in left:
        _lib.load().rlvi_tune_unset(name.encode())
    torch.cuda.synchronize()
    dirty = []
    for key, ws in list(ops._workspaces.items()):
        st = ws.status()
        if st:
            ws.clear_status()
            dirty.append(f"workspace {key}: sticky status {st}")
        if ws.pending_records():
            ops.mstep_reduce(ws=ws)
            dirty.append(f"workspace {key}: accumulate-mode records without an epoch end")
    assert not left, f"knobs left set by this test: {left}"
    assert not dirty, "; ".join(dirty)


def f16_inputs(torch, B, C, seed, N=None):
    """synth.mstep_inputs with the logits rounded to fp16; d['logits'] holds them widened (the oracle's input)."""
    d = synth.mstep_inputs(B, C, N=B + 17 if N is None else N, seed=seed, zero_frac=0.1)
    z16 = torch.from_numpy(d["logits"]).to(torch.float16)
    d["logits"] = z16.float().numpy()
    return d, z16


def rounded_f16(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.float16).float().numpy()


def call(gpu, z, d, ws=None, grad_scale=None, want_grad=True, inv_scale=None):
    torch, ops, dev = gpu
    res = torch.from_numpy(d["residuals"].copy()).to(dev)
    out, grad = ops.mstep_fwd_bwd(z.to(dev), torch.from_numpy(d["labels"]).to(dev),
                                  torch.from_numpy(d["idx"]).to(dev), torch.from_numpy(d["weights"]).to(dev),
                                  res, inv_scale=inv_scale, want_grad=want_grad, ws=ws, grad_scale=grad_scale)
    torch.cuda.synchronize()
    return out, grad, res


def last_form(ws):
    from rlvi_amd import _lib
    return _lib.load().rlvi_workspace_last_mstep_form(ws.ptr)


# the bf16 shape list of test_mstep_dispatch_by_launch_size_vs_oracle, and the bench-sized 16-wave tile
SHAPES = [
    (1024, 101),     # 32 lanes per row, register rows
    (8195, 101),     # 16 lanes per row, register rows
    (70003, 101),    # odd rows from 32 768 rows on: the word-wise wave tile + 3 trailing rows
    (32768, 33),     # ... eight words per lane, no trailing rows
    (40000, 127),    # ... sixteen words per lane, the longest row it takes
    (36005, 9),      # ... the shortest: lane 3 of a row's group holds nothing
    (1029, 104),     # eight lanes x two 8-element vectors, register rows
    (20005, 104),    # four lanes per row, wave tiles in four-wave workgroups
    (65536, 104),    # ... wave tiles in 16-wave workgroups
    (3000, 200),
    (8200, 366),     # even rows of 129 ... 384 elements: sixteen lanes per row, pairs
    (9001, 365),     # odd rows beyond 127 elements: register rows
    (16411, 48),     # rows of five to eight 16-byte vectors from 16 384 rows on: two lanes per row
    (20003, 64),     # ... eight
    (130, 4104),     # long rows, 8-element vectors, a workgroup per row
    (257, 1001),     # long rows, single elements
    (65536, 100),    # the bench shape
]


@pytest.mark.parametrize("B,C", SHAPES)
def test_f16_mstep_every_form_vs_oracle_and_takes_the_bf16_form(B, C, gpu, oracle):
    torch, ops, dev = gpu
    d, z16 = f16_inputs(torch, B, C, seed=B + C)
    ws = ops.workspace(dev, B + 17, B)
    out, grad, res = call(gpu, z16, d, ws=ws)
    form16 = last_form(ws)
    assert grad.dtype == torch.float16
    r0 = d["residuals"].copy()
    ref = oracle.mstep(d["logits"], d["labels"], d["idx"], d["weights"], r0)
    np.testing.assert_allclose(res.cpu().numpy(), r0, rtol=REL, atol=1e-6)
    o = out.cpu().numpy()
    assert abs(float(o[0]) - float(ref["loss"])) <= REL * abs(float(ref["loss"]))
    assert float(o[3]) == float(round(float(ref["prec1"]) * B / 100.0))
    np.testing.assert_allclose(grad.float().cpu().numpy(), rounded_f16(torch, ref["grad"]), rtol=F16_RTOL,
                               atol=F16_ATOL)
    # the same launch with bf16 logits takes the same form: every 2-byte decision was tuned on bytes
    call(gpu, z16.to(torch.bfloat16), d, ws=ws)
    assert form16 == last_form(ws) and form16 > 0, (form16, last_form(ws))
    assert ws.status() == 0


def test_f16_strided_rows_and_forward_only(gpu, oracle):
    torch, ops, dev = gpu
    B, C, LD = 96, 100, 128
    d, z16 = f16_inputs(torch, B, C, seed=11, N=B)
    big = torch.zeros(B, LD, dtype=torch.float16, device=dev)
    big[:, :C] = z16.to(dev)
    out, grad, _ = call(gpu, big[:, :C], d)
    out2, none, _ = call(gpu, big[:, :C], d, want_grad=False)
    ref = oracle.mstep(d["logits"], d["labels"], d["idx"], d["weights"], d["residuals"].copy())
    assert none is None and torch.equal(out, out2)
    assert abs(float(out[0]) - float(ref["loss"])) <= REL * abs(float(ref["loss"]))
    np.testing.assert_allclose(grad.float().cpu().numpy(), rounded_f16(torch, ref["grad"]), rtol=F16_RTOL,
                               atol=F16_ATOL)


@pytest.mark.parametrize("B,C", [(3000, 37), (70003, 101), (65536, 104)])
def test_f16_evaluation_form(B, C, gpu, oracle):
    torch, ops, dev = gpu
    d, z16 = f16_inputs(torch, B, C, seed=8)
    out = ops.evaluate_batch(z16.to(dev), torch.from_numpy(d["labels"]).to(dev)).cpu().numpy()
    loss, hit = oracle.nll_rows(d["logits"], d["labels"])
    assert abs(float(out[0]) - float(loss.astype(np.float64).mean())) <= REL * float(loss.mean())
    assert float(out[3]) == float(hit.sum())
    # per_sample_ce: the forward-only call with pi = 1
    rows = ops.per_sample_ce(z16.to(dev), torch.from_numpy(d["labels"]).to(dev))
    np.testing.assert_allclose(rows.cpu().numpy(), loss, rtol=REL, atol=1e-6)


def test_f16_accumulate_and_epoch_end(gpu, oracle):
    torch, ops, dev = gpu
    N, C = 1000, 10
    d, z16 = f16_inputs(torch, N, C, seed=77, N=N)
    order = np.random.default_rng(5).permutation(N)
    res_t = torch.zeros(N, device=dev)
    w_t = torch.from_numpy(d["weights"].copy()).to(dev)
    res_o, w_o = np.zeros(N, np.float32), d["weights"].copy()
    ws = ops.Workspace(dev, N, N)
    precs, losses = [], []
    for lo, hi in ((0, 400), (400, 800), (800, 1000)):
        rows = order[lo:hi]
        _, g = ops.mstep_fwd_bwd(z16[rows].to(dev), torch.from_numpy(d["labels"][rows]).to(dev),
                                 torch.from_numpy(rows).to(dev), w_t, res_t, accumulate=True, ws=ws)
        ref = oracle.mstep(d["logits"][rows], d["labels"][rows], rows, w_o, res_o)
        precs.append(float(ref["prec1"]))
        losses.append(float(ref["loss"]))
        np.testing.assert_allclose(g.float().cpu().numpy(), rounded_f16(torch, ref["grad"]), rtol=F16_RTOL,
                                   atol=F16_ATOL)
    thr, out = ops.epoch_end(res_t, w_t, overfit=True, threshold=0, batches=3, ws=ws)
    torch.cuda.synchronize()
    oracle.update_sample_weights(res_o, w_o)
    thr_o = oracle.false_negative_criterion(w_o)
    oracle.truncate(w_o, thr_o)
    assert float(out[1]) == pytest.approx(np.mean(precs), abs=1e-4)
    assert float(out[0]) == pytest.approx(np.mean(losses), rel=1e-5)
    assert abs(float(thr) - float(thr_o)) <= REL * float(thr_o)
    rel, small = rel_pi(w_t.cpu().numpy(), w_o)
    assert rel <= REL and small <= 1e-7
    assert ws.status() == 0


# ------------------------------------------------------------------------------ the loss scale
# one shape per kernel form: register rows, four-wave tiles, 16-wave tiles, word-wise odd rows, two-lane rows,
# long rows
SCALE_SHAPES = [(1029, 104), (20005, 104), (65536, 104), (70003, 101), (16411, 48), (257, 1001)]


@pytest.mark.parametrize("B,C", SCALE_SHAPES)
def test_f16_loss_scale_read_on_the_device(B, C, gpu, oracle):
    torch, ops, dev = gpu
    d, z16 = f16_inputs(torch, B, C, seed=3 * B + C)
    out0, g0, r0 = call(gpu, z16, d)
    out1, g1, r1 = call(gpu, z16, d, grad_scale=torch.ones(1, device=dev))
    # NULL and *grad_scale == 1 give the same bits
    assert torch.equal(g0.view(torch.int16), g1.view(torch.int16))
    u = g0.float()
    ref = oracle.mstep(d["logits"], d["labels"], d["idx"], d["weights"], d["residuals"].copy())["grad"]
    for s in (2.0 ** 12, 2.0 ** 34):
        out_s, g_s, r_s = call(gpu, z16, d, grad_scale=torch.full((1,), s, device=dev))
        # the loss, out[] and the residuals never see the scale
        assert torch.equal(out_s, out0) and torch.equal(r_s, r0)
        gs = g_s.float()
        want = (u * s).half().float()
        # (u strictly above the smallest normal: u == 2^-14 may be a subnormal value rounded up to it)
        both_normal = (u.abs() > F16_MIN_NORMAL) & (gs.abs() >= F16_MIN_NORMAL) & torch.isfinite(gs) \
            & (want.abs() <= F16_MAX)
        assert torch.equal(gs[both_normal], want[both_normal])
        # an overflow is +-inf (the GradScaler's check depends on it), not the largest finite value
        xs = np.abs(ref.astype(np.float64)) * s
        over = torch.from_numpy(xs > 65520.0 * (1 + 1e-5)).to(dev)
        under = torch.from_numpy(xs < F16_MAX * (1 - 1e-5)).to(dev)
        assert torch.isinf(gs[over]).all()
        assert torch.equal(torch.sign(gs[over]).cpu(), torch.from_numpy(np.sign(ref[over.cpu().numpy()])))
        assert torch.isfinite(gs[under]).all()
        if s == 2.0 ** 34:
            assert bool(over.any())                      # (the check above is not empty)
        else:
            assert not bool(over.any())
        # against the oracle: the unscaled bars times s (the fp32 values scale exactly, so does their error)
        fin = under.cpu().numpy()                        # (the inf side is checked above)
        np.testing.assert_allclose(gs.cpu().numpy()[fin], rounded_f16(torch, ref * np.float32(s))[fin],
                                   rtol=F16_RTOL, atol=F16_ATOL * s)


def test_mstep_loop_with_a_device_scale_needs_no_host_sync(gpu, oracle):
    torch, ops, dev = gpu
    B, C = 4096, 100
    N = B + 17
    d, z16 = f16_inputs(torch, B, C, seed=21)
    w = torch.from_numpy(d["weights"]).to(dev)
    res = torch.zeros(N, device=dev)
    zd, y, ix = z16.to(dev), torch.from_numpy(d["labels"]).to(dev), torch.from_numpy(d["idx"]).to(dev)
    ws = ops.Workspace(dev, N, B)
    loop = ops.MStepLoop(w, res, ws)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)
    one = torch.ones((), device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        g = loop(zd, y, ix, None, scaler.scale(one))
        g2 = loop(zd.float(), y, ix, None, scaler.scale(one))            # fp32 logits: the buffer is multiplied
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    ref = oracle.mstep(d["logits"], d["labels"], d["idx"], d["weights"], d["residuals"].copy())
    assert g.dtype == torch.float16 and g2.dtype == torch.float32
    np.testing.assert_allclose(g.float().cpu().numpy(), rounded_f16(torch, ref["grad"] * np.float32(1024)),
                               rtol=F16_RTOL, atol=F16_ATOL)
    np.testing.assert_allclose(g2.cpu().numpy() / 1024, ref["grad"], rtol=1e-4, atol=1e-6)
    ops.mstep_reduce(ws=ws)
    assert ws.status() == 0


# ------------------------------------------------------------------------------ precision@k
@pytest.mark.parametrize("C", [1, 2, 5, 7, 33, 100, 101, 512, 513, 1000])
def test_f16_topk_hits_vs_rank_count(C, gpu):
    torch, ops, dev = gpu
    rng = np.random.default_rng(C)
    B = 3001
    # few distinct values: many exact ties, among them the label's
    z = (rng.integers(-6, 7, (B, C)) * 0.375).astype(np.float16)
    z[: B // 3] = (rng.standard_normal((B // 3, C)) * 4).astype(np.float16)
    y = rng.integers(0, C, B).astype(np.int64)
    zw = z.astype(np.float32)
    zy = zw[np.arange(B), y][:, None]
    col = np.arange(C)[None, :]
    rank = (zw > zy).sum(1) + ((zw == zy) & (col < y[:, None])).sum(1)
    ks = sorted({1, min(5, C), C})
    zt, yt = torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev)
    hits = ops.topk_hits(zt, yt, ks).cpu().numpy()
    assert hits.tolist() == [int((rank < k).sum()) for k in ks]
    assert torch.equal(ops.topk_hits(zt.float(), yt, ks).cpu(), torch.from_numpy(hits))
    # utils.accuracy on fp16 logits, unchanged
    from rlvi_amd import utils
    acc = utils.accuracy(zt, yt, topk=tuple(ks))
    assert [float(a) for a in acc] == pytest.approx([100.0 * float((rank < k).sum()) / B for k in ks], abs=1e-4)


# ------------------------------------------------------------------------------ the plug-in
def g4_setup(torch, golden, dev, head):
    g = golden("g4_epoch")
    X, y = torch.from_numpy(g["X"]), torch.from_numpy(g["y"])

    class Fp16Head(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(X.shape[1], 10)

        def forward(self, x):
            z = self.lin(x)
            return z.to(torch.float16) if head == "cast" else z           # "autocast": the caller's autocast

    model = Fp16Head()
    with torch.no_grad():
        model.lin.weight.copy_(torch.from_numpy(g["W0"]))
        model.lin.bias.copy_(torch.from_numpy(g["b0"]))
    model.to(dev)
    seen, wgrads = [], []

    def fwd_hook(_m, inp, out):
        rec = {"x": inp[0].detach().clone(), "logits": out.detach().clone()}
        out.register_hook(lambda gr, rec=rec: rec.__setitem__("grad", gr.detach().clone()))
        seen.append(rec)
    model.register_forward_hook(fwd_hook)
    model.lin.weight.register_hook(lambda gr: wgrads.append(gr.detach().clone()))
    return g, X, y, model, seen, wgrads


def g4_loader(g, X, y, ep):
    import torch
    N, B = int(g["N"]), int(g["B"])
    perm = g["orders"][ep]
    return [(X[perm[s:s + B]], y[perm[s:s + B]], torch.from_numpy(perm[s:s + B].astype(np.int64)))
            for s in range(0, N, B)]


def check_epoch_vs_oracle(torch, oracle, seen, loader, w_before, thr_before, overfit, residuals, weights,
                          threshold, acc, grad_scale=1.0):
    """Every batch's gradient handed to autograd against the oracle on the same fp16 logits (times the loss scale,
    rounded to fp16), then the epoch end: min-shifted residuals, pi, threshold and train_acc."""
    N = weights.shape[0]
    r_o = np.zeros(N, np.float32)
    precs = []
    for rec, (_, lab, idx) in zip(seen, loader):
        assert rec["logits"].dtype == torch.float16 and rec["grad"].dtype == torch.float16
        ref = oracle.mstep(rec["logits"].float().cpu().numpy(), lab.numpy(), idx.numpy(), w_before, r_o)
        precs.append(float(ref["prec1"]))
        np.testing.assert_allclose(rec["grad"].float().cpu().numpy(),
                                   rounded_f16(torch, ref["grad"] * np.float32(grad_scale)),
                                   rtol=F16_RTOL, atol=F16_ATOL)
    w_o = w_before.copy()
    oracle.update_sample_weights(r_o, w_o)
    thr_o = thr_before
    near = np.zeros(N, bool)
    if overfit:
        thr_o = max(thr_before, float(oracle.false_negative_criterion(w_o)))
        near = np.abs(w_o - np.float32(thr_o)) <= 1e-5 * max(thr_o, 1e-30)
        oracle.truncate(w_o, np.float32(thr_o))
    np.testing.assert_allclose(residuals.cpu().numpy(), r_o, rtol=REL, atol=2e-6)
    rel, small = rel_pi(weights.cpu().numpy()[~near], w_o[~near])
    assert rel <= REL and small <= 1e-7, (rel, small)
    assert abs(float(threshold) - thr_o) <= 1e-5 * max(thr_o, 1e-30) + 1e-7
    assert acc == pytest.approx(float(np.mean(precs)), abs=1e-3)


@pytest.mark.parametrize("head", ["cast", "autocast"])
def test_train_rlvi_with_fp16_logits_through_the_plugin(head, golden, gpu, oracle, monkeypatch):
    """G4's four epochs (overfit F, F, T, T) through the unchanged plug-in with fp16 logits: a head that emits fp16,
    or a plain fp32 model under torch.autocast(dtype=float16).  A generic wrapper that raises proves that every
    batch took MStepLoop's validated fast path (the native fp16 entry, no fp32 copy)."""
    torch, ops, dev = gpu
    from rlvi_amd.methods import train_rlvi

    def no_generic(*a, **k):
        raise AssertionError("a batch left MStepLoop's fast path")
    monkeypatch.setattr(ops, "mstep_fwd_bwd", no_generic)
    g, X, y, model, seen, wgrads = g4_setup(torch, golden, dev, head)
    N = int(g["N"])
    opt = torch.optim.SGD(model.parameters(), lr=float(g["lr"]), momentum=float(g["momentum"]))
    residuals = torch.zeros(N, device=dev)
    weights = torch.ones(N, device=dev)
    threshold = 0
    for ep in range(4):
        loader = g4_loader(g, X, y, ep)
        overfit = bool(g[f"ep{ep}/overfit"])
        w_before, thr_before = weights.cpu().numpy().copy(), float(threshold)
        seen.clear()
        wgrads.clear()
        model.train()
        with torch.autocast("cuda", dtype=torch.float16, enabled=head == "autocast"):
            acc, threshold = train_rlvi(loader, model, opt, residuals, weights, overfit, threshold)
        torch.cuda.synchronize()
        assert len(seen) == len(loader) == len(wgrads)
        check_epoch_vs_oracle(torch, oracle, seen, loader, w_before, thr_before, overfit, residuals, weights,
                              threshold, acc)
        if head == "cast":
            # what autograd makes of the fp16 gradient at the parameters: grad_W = grad^T x
            for rec, gw in zip(seen, wgrads):
                gw_ref = rec["grad"].float().t() @ rec["x"]
                np.testing.assert_allclose(gw.cpu().numpy(), gw_ref.cpu().numpy(), rtol=1e-4, atol=1e-7)
    assert torch.is_tensor(threshold) and threshold.dim() == 0
    assert ops.workspace(dev).status() == 0


def test_train_rlvi_amp_power_of_two_scale_matches_the_unscaled_run(golden, gpu, oracle):
    torch, ops, dev = gpu
    from rlvi_amd.methods import train_rlvi, train_rlvi_amp
    params = []
    for scaled in (False, True):
        g, X, y, model, seen, _ = g4_setup(torch, golden, dev, "cast")
        N = int(g["N"])
        opt = torch.optim.SGD(model.parameters(), lr=float(g["lr"]), momentum=float(g["momentum"]))
        residuals, weights, threshold = torch.zeros(N, device=dev), torch.ones(N, device=dev), 0
        scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10, growth_interval=1 << 20)
        for ep in range(2):
            loader = g4_loader(g, X, y, ep)
            w_before, thr_before = weights.cpu().numpy().copy(), float(threshold)
            seen.clear()
            if scaled:
                acc, threshold = train_rlvi_amp(loader, model, opt, residuals, weights, False, threshold, scaler)
            else:
                acc, threshold = train_rlvi(loader, model, opt, residuals, weights, False, threshold)
            torch.cuda.synchronize()
            check_epoch_vs_oracle(torch, oracle, seen, loader, w_before, thr_before, False, residuals, weights,
                                  threshold, acc, grad_scale=2.0 ** 10 if scaled else 1.0)
        if scaled:
            assert scaler.get_scale() == 2.0 ** 10                 # no step was skipped
        params.append([p.detach().cpu().numpy() for p in model.parameters()])
    for a, b in zip(*params):
        np.testing.assert_allclose(b, a, rtol=1e-3, atol=1e-5)
    assert ops.workspace(dev).status() == 0


def test_train_rlvi_amp_skips_every_overflowing_step(golden, gpu, oracle):
    """A scale at which every batch's gradient overflows fp16: the kernel writes inf, the scaler finds it, no step
    is taken and the scale halves once per batch.  The M-step's own results do not depend on the scale: the
    residuals and pi are the oracle's epoch end on the CE of the initial model."""
    torch, ops, dev = gpu
    from rlvi_amd.methods import train_rlvi_amp
    g, X, y, model, seen, _ = g4_setup(torch, golden, dev, "cast")
    N = int(g["N"])
    p0 = [p.detach().clone() for p in model.parameters()]
    opt = torch.optim.SGD(model.parameters(), lr=float(g["lr"]), momentum=float(g["momentum"]))
    residuals, weights = torch.zeros(N, device=dev), torch.ones(N, device=dev)
    init = 2.0 ** 48
    scaler = torch.amp.GradScaler("cuda", init_scale=init)
    loader = g4_loader(g, X, y, 0)
    acc, threshold = train_rlvi_amp(loader, model, opt, residuals, weights, False, 0, scaler)
    torch.cuda.synchronize()
    for rec in seen:
        assert bool(torch.isinf(rec["grad"]).any())
    for a, b in zip(p0, model.parameters()):
        assert torch.equal(a, b.detach())
    assert scaler.get_scale() == init * 0.5 ** len(loader)
    # the same logits every batch (the model never moved): the oracle on the initial model's CE
    w_o = np.ones(N, np.float32)
    r_o = np.zeros(N, np.float32)
    precs = []
    for (xb, lab, idx) in loader:
        z = model.lin(xb.to(dev)).to(torch.float16).float().detach().cpu().numpy()
        precs.append(float(oracle.mstep(z, lab.numpy(), idx.numpy(), np.ones(N, np.float32), r_o)["prec1"]))
    oracle.update_sample_weights(r_o, w_o)
    np.testing.assert_allclose(residuals.cpu().numpy(), r_o, rtol=REL, atol=2e-6)
    rel, small = rel_pi(weights.cpu().numpy(), w_o)
    assert rel <= REL and small <= 1e-7
    assert acc == pytest.approx(float(np.mean(precs)), abs=1e-3)
    assert threshold == 0
    assert ops.workspace(dev).status() == 0


def test_driver_amp_fp16_end_to_end(gpu, tmp_path):
    """python -m rlvi_amd.driver --amp fp16: autocast + GradScaler through train_rlvi_amp, two epochs."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "rlvi_amd.driver", "--amp", "fp16", "--n_epoch", "3", "--n_train", "2048",
           "--n_val", "512", "--n_test", "512", "--batch_size", "256", "--result_dir", str(tmp_path)]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    log = tmp_path / "mnist" / "rlvi" / "mnist_rlvi_pairflip_0.45-s1.txt"
    lines = log.read_text().strip().splitlines()
    assert len(lines) == 1 + 3                                          # header, epoch 0, two training epochs
    for line in lines[2:]:
        train_acc = float(line.split("\t")[6])
        assert math.isfinite(train_acc) and 0.0 <= train_acc <= 100.0
