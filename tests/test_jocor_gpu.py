"""JoCoR on the MI355X (run with -m gpu): ops.jocor_loss and methods.train_jocor against golden set G12 (the
reference's own outputs) and the float64 restatement of test_jocor_cpu, in fp32, bf16 and fp16.

Bars: loss and fp32 gradients as test_small_loss_baselines_golden; half gradients against the reference's fp32
gradient rounded to the same format, within one unit of that format (fp16: F16_RTOL / F16_ATOL; bf16: 2^-7).
"""
import numpy as np
import pytest

from rlvi_amd import synth
from test_jocor_cpu import case_inputs, golden, pinned, restate, selection
from test_oracle_golden import REL

pytestmark = pytest.mark.gpu

F16_RTOL, F16_ATOL = 2 ** -10, 2 ** -24
BF16_RTOL = 2 ** -7
CASES = list(golden()["cases"])


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


def tdtype(torch, dt):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dt]


def loss_close(a, ref):
    assert abs(float(a) - float(ref)) <= REL * abs(float(ref)) + 2.0 ** -24, (float(a), float(ref))


def grad_close(torch, a, ref, dt, what=""):
    """a: the kernel's gradient rows (any dtype); ref: the reference's fp32 rows."""
    a = a.float().cpu().numpy()
    base = max(1e-6 * np.abs(ref).max(), 2.0 ** -24)
    if dt == "f32":
        np.testing.assert_allclose(a, ref, rtol=1e-5, atol=base, err_msg=what)
        return
    r = torch.from_numpy(np.ascontiguousarray(ref)).to(tdtype(torch, dt)).float().numpy()
    rtol = F16_RTOL if dt == "f16" else BF16_RTOL
    np.testing.assert_allclose(a, r, rtol=rtol, atol=max(F16_ATOL, base), err_msg=what)


def run(gpu, z1n, z2n, y, fr, lam, dt, g_factor=None):
    torch, ops, dev = gpu
    z1 = torch.from_numpy(z1n).to(dev).to(tdtype(torch, dt)).requires_grad_(True)
    z2 = torch.from_numpy(z2n).to(dev).to(tdtype(torch, dt)).requires_grad_(True)
    t = torch.from_numpy(y).to(dev)
    loss = ops.jocor_loss(z1, z2, t, fr, co_lambda=lam)
    (loss if g_factor is None else g_factor * loss).backward()
    torch.cuda.synchronize()
    return loss.detach(), z1.grad, z2.grad


@pytest.mark.parametrize("key", CASES)
def test_jocor_loss_and_gradients_vs_reference(key, gpu):
    torch, ops, dev = gpu
    g = golden()
    z1n, z2n, y, k, fr, lam, dt = case_inputs(g, key)
    loss, g1, g2 = run(gpu, z1n, z2n, y, fr, lam, dt)
    assert g1.dtype == tdtype(torch, dt) and g2.dtype == tdtype(torch, dt)
    rows = torch.from_numpy(g[key + "/rows"]).to(dev)
    if k == 0:
        # torch.mean of an empty selection: NaN, and nothing flows back -- both gradients exactly zero
        assert torch.isnan(loss)
        assert not g1.float().abs().sum().item() and not g2.float().abs().sum().item()
    else:
        loss_close(loss, g[key + "/loss"])
    grad_close(torch, g1[rows], g[key + "/grad1"], dt, key + " grad1")
    grad_close(torch, g2[rows], g[key + "/grad2"], dt, key + " grad2")

    # the forward's own outputs: K_qp, K_pq, loss_pick on the stored rows, exactly k rows kept and, where the
    # reference's choice is pinned, the same rows
    zz1 = torch.from_numpy(z1n).to(dev).to(tdtype(torch, dt))
    zz2 = torch.from_numpy(z2n).to(dev).to(tdtype(torch, dt))
    out, pick, sel = ops.jocor_forward(zz1, zz2, torch.from_numpy(y).to(dev), k, lam)
    torch.cuda.synchronize()
    np.testing.assert_allclose(out[1:3].cpu().numpy(), g[key + "/kl"], rtol=REL)
    np.testing.assert_allclose(pick[rows].cpu().numpy(), g[key + "/loss_pick"], rtol=REL, atol=2.0 ** -20)
    s = sel.cpu().numpy()
    assert set(np.unique(s)) <= {0.0, 1.0}
    assert int(s.sum()) == k
    if pinned(g, key):
        assert np.array_equal(s.astype(bool), selection(g, key)), key
    if k == 0:
        assert np.isnan(out[0].item())


def test_upstream_gradient_and_loss_scale_are_read_on_the_device(gpu):
    torch, ops, dev = gpu
    g = golden()
    key = "f32_B1024_C101_fr0.45_lam0.1"
    z1n, z2n, y, k, fr, lam, dt = case_inputs(g, key)
    _, a1, a2 = run(gpu, z1n, z2n, y, fr, lam, "f32")
    _, b1, b2 = run(gpu, z1n, z2n, y, fr, lam, "f32", g_factor=3.0)
    # (g / k and g lambda / B are rounded before they multiply: a few ulp of the larger terms of an element)
    for b, a in ((b1, a1), (b2, a2)):
        ref = 3 * a.cpu().numpy()
        np.testing.assert_allclose(b.cpu().numpy(), ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())
    # a GradScaler: scaler.scale(L).backward() hands the scale in as the upstream gradient (a device tensor)
    for dt in ("f32", "f16"):
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
        z1 = torch.from_numpy(z1n).to(dev).to(tdtype(torch, dt)).requires_grad_(True)
        z2 = torch.from_numpy(z2n).to(dev).to(tdtype(torch, dt)).requires_grad_(True)
        scaler.scale(ops.jocor_loss(z1, z2, torch.from_numpy(y).to(dev), fr)).backward()
        _, c1, c2 = run(gpu, z1n, z2n, y, fr, lam, dt)
        for scaled, plain in ((z1.grad, c1), (z2.grad, c2)):
            ref = 1024.0 * plain.float().cpu().numpy()
            np.testing.assert_allclose(scaled.float().cpu().numpy(), ref, rtol=F16_RTOL if dt == "f16" else 1e-7,
                                       atol=F16_ATOL * 1024)
    # the C entry's own loss-scale pointer, beside the upstream gradient: both multiply
    zz1 = torch.from_numpy(z1n).to(dev)
    zz2 = torch.from_numpy(z2n).to(dev)
    t = torch.from_numpy(y).to(dev)
    out, _, sel = ops.jocor_forward(zz1, zz2, t, k, lam)
    two = torch.full((), 2.0, device=dev)
    eight = torch.full((), 8.0, device=dev)
    d1, d2 = ops.jocor_backward(zz1, zz2, t, sel, k, lam, grad_out=two, grad_scale=eight)
    torch.cuda.synchronize()
    np.testing.assert_allclose(d1.cpu().numpy(), 16 * a1.cpu().numpy(), rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(d2.cpu().numpy(), 16 * a2.cpu().numpy(), rtol=1e-6, atol=1e-12)


def check_vs_restatement(torch, z1, z2, y, k, lam, loss, g1, g2, dt="f32"):
    L, _, _, _, _, r1, r2 = restate(z1.float().cpu().numpy(), z2.float().cpu().numpy(), y, k, lam)
    assert abs(float(loss.detach()) - L) <= REL * abs(L)
    for mine, ref in ((g1, r1), (g2, r2)):
        grad_close(torch, mine, ref.astype(np.float32), dt)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_strided_rows(dt, gpu):
    torch, ops, dev = gpu
    B, C, pad = 300, 37, 5
    d1 = synth.mstep_inputs(B, C, N=B, seed=71)
    d2 = synth.mstep_inputs(B, C, N=B, seed=72)
    w1 = torch.zeros((B, C + pad), device=dev, dtype=tdtype(torch, dt))
    w2 = torch.zeros((B, C + 2 * pad), device=dev, dtype=tdtype(torch, dt))
    w1[:, :C] = torch.from_numpy(d1["logits"]).to(dev)
    w2[:, pad:pad + C] = torch.from_numpy(d2["logits"]).to(dev)
    z1 = w1[:, :C].detach().requires_grad_(True)
    z2 = w2[:, pad:pad + C].detach().requires_grad_(True)
    assert z1.stride(0) == C + pad and z2.stride(0) == C + 2 * pad
    y = d1["labels"]
    loss = ops.jocor_loss(z1, z2, torch.from_numpy(y).to(dev), 0.3)
    loss.backward()
    torch.cuda.synchronize()
    check_vs_restatement(torch, z1.detach(), z2.detach(), y, int(0.7 * B), 0.1, loss, z1.grad, z2.grad, dt)


def test_row_with_an_underflowed_softmax_entry(gpu):
    """exp(z - max) == 0 in fp32 for some entries: torch's kl_div gives those target entries zero gradient; the
    kernel works in log space and gets the same without a NaN."""
    torch, ops, dev = gpu
    B, C = 64, 10
    d1 = synth.mstep_inputs(B, C, N=B, seed=81)
    d2 = synth.mstep_inputs(B, C, N=B, seed=82)
    z1n, z2n = d1["logits"].copy(), d2["logits"].copy()
    z1n[3, 2] = -250.0
    z2n[3, 7] = -300.0
    z1n[10, :] = -120.0
    z1n[10, d1["labels"][10]] = 40.0
    z2n[11, 0] = 150.0
    z1 = torch.from_numpy(z1n).to(dev).requires_grad_(True)
    z2 = torch.from_numpy(z2n).to(dev).requires_grad_(True)
    y = d1["labels"]
    loss = ops.jocor_loss(z1, z2, torch.from_numpy(y).to(dev), 0.25)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(z1.grad).all() and torch.isfinite(z2.grad).all()
    check_vs_restatement(torch, z1.detach(), z2.detach(), y, int(0.75 * B), 0.1, loss, z1.grad, z2.grad)


def test_labels_out_of_range_raise(gpu):
    torch, ops, dev = gpu
    from rlvi_amd import _lib
    B, C = 128, 10
    d1 = synth.mstep_inputs(B, C, N=B, seed=91)
    z1 = torch.from_numpy(d1["logits"]).to(dev).requires_grad_(True)
    z2 = torch.from_numpy(d1["logits"][::-1].copy()).to(dev).requires_grad_(True)
    for bad in (C, -1):
        y = torch.from_numpy(d1["labels"].copy()).to(dev)
        y[17] = bad
        with pytest.raises(_lib.RlviError, match="out of range"):
            ops.jocor_loss(z1, z2, y, 0.2)
    assert ops.workspace(dev).status() == 0
    ops.jocor_loss(z1, z2, torch.from_numpy(d1["labels"]).to(dev), 0.2)       # a good batch afterwards


@pytest.mark.parametrize("B,C,dt", [(65536, 100, "f32"), (2048, 1500, "f32"), (1024, 2501, "bf16"),
                                    (4097, 1023, "f16")])
def test_large_shapes_vs_restatement(B, C, dt, gpu):
    """The bench-sized batch in one call, and rows longer than the register form (a wave per row)."""
    torch, ops, dev = gpu
    d1 = synth.mstep_inputs(B, C, N=B, seed=B + C)
    d2 = synth.mstep_inputs(B, C, N=B, seed=B + C + 1)
    z1 = torch.from_numpy(d1["logits"]).to(dev).to(tdtype(torch, dt)).requires_grad_(True)
    z2 = torch.from_numpy(d2["logits"]).to(dev).to(tdtype(torch, dt)).requires_grad_(True)
    y = d1["labels"]
    t = torch.from_numpy(y).to(dev)
    loss = ops.jocor_loss(z1, z2, t, 0.3)
    loss.backward()
    torch.cuda.synchronize()
    k = int(0.7 * B)
    check_vs_restatement(torch, z1.detach(), z2.detach(), y, k, 0.1, loss, z1.grad, z2.grad, dt)
    _, _, sel = ops.jocor_forward(z1.detach(), z2.detach(), t, k)
    assert int(sel.sum().item()) == k
    # rows left out of the selection still carry the KL gradient
    out_rows = sel == 0
    assert (z1.grad[out_rows].float().abs().sum(1) > 0).all()


def loop_setup(gpu):
    torch, ops, dev = gpu
    g = golden()
    X, y = synth.jocor_loop_inputs(1212, 256, 16, 10)
    loader = [(torch.from_numpy(X[s:s + 64]), torch.from_numpy(y[s:s + 64]), torch.arange(s, s + 64))
              for s in range(0, 256, 64)]
    init = g["loop/init"]
    models, off = [], 0
    for _ in range(2):
        m = torch.nn.Linear(16, 10).to(dev)
        with torch.no_grad():
            for q in m.parameters():
                q.copy_(torch.from_numpy(init[off:off + q.numel()].reshape(q.shape)))
                off += q.numel()
        models.append(m)
    opt = torch.optim.SGD(list(models[0].parameters()) + list(models[1].parameters()), lr=0.05, momentum=0.9,
                          weight_decay=1e-4)
    return g, loader, models, opt


def flat(models):
    return np.concatenate([q.detach().cpu().numpy().ravel() for m in models for q in m.parameters()])


def test_train_jocor_three_epochs_vs_reference(gpu):
    torch, ops, dev = gpu
    from rlvi_amd.methods import train_jocor
    g, loader, (m1, m2), opt = loop_setup(gpu)
    rs = g["loop/rate_schedule"]
    for e in range(3):
        acc = train_jocor(loader, e + 1, m1, m2, opt, rs)
        assert abs(acc - g["loop/train_acc"][e]) <= 1e-4, (e, acc)
        np.testing.assert_allclose(flat([m1, m2]), g["loop/params"][e], rtol=1e-4, atol=1e-5, err_msg=f"epoch {e}")


def test_jocor_loop_under_autocast_fp16_with_a_scaler(gpu):
    """The same three epochs with fp16 logits from autocast and a GradScaler: close to the reference's fp32 run (the
    logits carry fp16 rounding), finite, and the loss scale really reaches the kernel."""
    torch, ops, dev = gpu
    g, loader, (m1, m2), opt = loop_setup(gpu)
    rs = g["loop/rate_schedule"]
    scaler = torch.amp.GradScaler("cuda", init_scale=256.0)
    for e in range(3):
        hits = 0.0
        for images, labels, _ in loader:
            images, labels = images.to(dev), labels.to(dev)
            with torch.autocast("cuda", dtype=torch.float16):
                z1, z2 = m1(images), m2(images)
                assert z1.dtype == torch.float16
                out = torch.empty(4, device=dev)
                loss = ops.jocor_loss(z1, z2, labels, rs[e + 1], out=out)
            hits += float(out[3])
            opt.zero_grad()
            scaler.scale(loss).backward()
            assert m1.weight.grad.dtype == torch.float32
            scaler.step(opt)
            scaler.update()
        assert abs(hits / len(loader) - g["loop/train_acc"][e]) <= 5.0
        p = flat([m1, m2])
        assert np.isfinite(p).all()
        np.testing.assert_allclose(p, g["loop/params"][e], atol=3e-2, err_msg=f"epoch {e}")
    assert scaler.get_scale() >= 256.0


def test_equal_losses_are_taken_in_index_order(gpu):
    """Rows of exactly equal loss_pick across the boundary (np.argsort's choice among them is unpinned): the first
    ones in index order, exactly k of them, as select_smallest_kernel takes them."""
    torch, ops, dev = gpu
    B, C = 3000, 10
    d = synth.mstep_inputs(B, C, N=B, seed=97)
    z1n, z2n, y = d["logits"].copy(), d["logits"][::-1].copy(), d["labels"].copy()
    same = np.arange(B) % 3 == 1                   # a third of the rows identical: one loss_pick value
    z1n[same], z2n[same], y[same] = z1n[1], z2n[1], y[1]
    t = torch.from_numpy(y).to(dev)
    _, pick, _ = ops.jocor_forward(torch.from_numpy(z1n).to(dev), torch.from_numpy(z2n).to(dev), t, 0)
    p = pick.cpu().numpy()
    v = p[1]
    below = int((p < v).sum())
    for k in (below + 1, below + 17, below + int(same.sum()) - 1):
        _, pick, sel = ops.jocor_forward(torch.from_numpy(z1n).to(dev), torch.from_numpy(z2n).to(dev), t, k)
        s = sel.cpu().numpy().astype(bool)
        assert int(s.sum()) == k
        assert s[p < v].all() and not s[p > v].any()
        tied = np.nonzero(p == v)[0]
        assert s[tied[:k - below]].all() and not s[tied[k - below:]].any()
