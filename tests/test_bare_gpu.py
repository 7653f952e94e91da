"""BARE and the plain loop on the MI355X (run with -m gpu): ops.bare_forward / ops.bare_loss, methods.train_bare and
methods.train_regular against golden set G14 (the reference's own outputs) and the float64 restatement of
test_bare_cpu, in fp32, bf16 and fp16, in both kernel forms.

Bars: loss and gradients as test_jocor_gpu (loss_close; grad_close with its fp16 and bf16 units).  The selection is
compared on pinned rows only (|margin| > 2^-18); away from the golden set, loss and gradients are compared with the
restatement's for the selection the kernel made, once that selection has been checked on the pinned rows.
"""
import numpy as np
import pytest

from rlvi_amd import synth
from test_bare_cpu import (case_inputs, full, golden, loss_and_grad, pinned, pinned_rows, restate, rounded,
                           selection)
from test_jocor_gpu import F16_ATOL, F16_RTOL, grad_close, loss_close, tdtype
from test_jocor_gpu import gpu, no_process_state_left_behind  # noqa: F401  (fixtures: the device, the hygiene check)

pytestmark = pytest.mark.gpu

CASES = list(golden()["cases"])
DTYPES = ("f32", "bf16", "f16")


def set_form(form):
    from rlvi_amd import _lib
    _lib.check(_lib.load().rlvi_tune_set(b"RLVI_BARE_FORM", int(form)), "rlvi_tune_set")


def unset_form():
    from rlvi_amd import _lib
    _lib.load().rlvi_tune_unset(b"RLVI_BARE_FORM")


def run(gpu, zn, y, k, dt, g_factor=None, pitch=None):
    """ops.bare_loss with backward, then ops.bare_forward: (loss, grad, out, w, sel) as device tensors."""
    torch, ops, dev = gpu
    z = torch.from_numpy(zn).to(dev).to(tdtype(torch, dt))
    if pitch is not None:
        wide = torch.zeros((z.shape[0], pitch), device=dev, dtype=z.dtype)
        wide[:, :z.shape[1]] = z
        z = wide[:, :z.shape[1]]
        assert z.stride(0) == pitch
    z = z.detach().requires_grad_(True)
    t = torch.from_numpy(y).to(dev)
    out = torch.full((4,), -1.0, device=dev)
    loss = ops.bare_loss(z, t, k, out=out)
    (loss if g_factor is None else g_factor * loss).backward()
    out2, w, sel = ops.bare_forward(z.detach(), t, k)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and float(loss.detach()) == float(out[0])
    assert z.grad.dtype == tdtype(torch, dt) and z.grad.shape == z.shape
    return loss.detach(), z.grad, out, w, sel


def check_outputs(out, w, sel, B):
    """What holds for every call: sel is 0/1, w == sel / n_kept, n_kept counts sel, the fallback keeps every row."""
    s, wv = sel.cpu().numpy(), w.cpu().numpy()
    n_kept, fallback = float(out[1]), float(out[2])
    assert set(np.unique(s)) <= {0.0, 1.0}
    assert int(s.sum()) == int(n_kept) and fallback in (0.0, 1.0)
    if fallback:
        assert int(n_kept) == B and s.all()
    assert np.array_equal(wv, s * (np.float32(1.0) / np.float32(n_kept)))
    return s.astype(bool)


def top1_percent(zn, y):
    return 100.0 * float((np.argmax(zn, axis=1) == y).sum()) / len(y)


def check_vs_restatement(gpu, zn, y, k, dt, loss, grad, out, w, sel, rows=None, skip=None):
    """Selection on the pinned rows (minus `skip`), then loss and gradient for the selection made."""
    torch, ops, dev = gpu
    B = len(y)
    s = check_outputs(out, w, sel, B)
    L, m, ref_sel, _, fallback = restate(zn, y, k)
    pin = pinned_rows(m)
    if skip is not None:
        pin &= ~skip
    assert fallback == bool(float(out[2]))
    assert np.array_equal(s[pin], ref_sel[pin])
    L, ref_grad = loss_and_grad(zn, y, s)
    loss_close(loss, L)
    assert abs(float(out[3]) - top1_percent(zn, y)) <= 1e-4
    rows = np.arange(B) if rows is None else rows
    grad_close(torch, grad[torch.from_numpy(rows).to(dev)], ref_grad[rows].astype(np.float32), dt)
    return s


@pytest.mark.parametrize("key", CASES)
def test_bare_loss_and_gradients_vs_reference(key, gpu):
    torch, ops, dev = gpu
    g = golden()
    zn, y, k, dt = case_inputs(key)
    B = len(y)
    loss, grad, out, w, sel = run(gpu, zn, y, k, dt)
    s = check_outputs(out, w, sel, B)
    pin = pinned(g, key)
    assert np.array_equal(s[pin], selection(g, key)[pin]), key
    assert abs(int(float(out[1])) - int(g[key + "/n_kept"])) <= int(g[key + "/unpinned"]), key
    assert bool(float(out[2])) == bool(g[key + "/fallback"]), key
    assert abs(float(out[3]) - top1_percent(zn, y)) <= 1e-4, key
    assert torch.isfinite(grad.float()).all()
    if full(g, key):
        assert int(float(out[1])) == int(g[key + "/n_kept"]), key
        loss_close(loss, g[key + "/loss"])
        rows = torch.from_numpy(g[key + "/rows"]).to(dev)
        grad_close(torch, grad[rows], g[key + "/grad"], dt, key)
        # rows the reference dropped carry no gradient at all
        assert not grad[~sel.bool()].float().abs().sum().item()


def both_forms_inputs():
    cases = [("shape", 37, 10), ("shape", 128, 100)]
    cases += [("case", kind, B) for kind, Bs in (("tiny", (1, 2)), ("unbiased", (3, 4, 5, 16))) for B in Bs]
    return cases


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("what", both_forms_inputs(), ids=lambda w: "-".join(str(v) for v in w))
def test_both_forms_give_the_same_selection(what, dt, gpu):
    torch, ops, dev = gpu
    from rlvi_amd import _lib
    if what[0] == "shape":
        _, B, C = what
        zn, y = synth.bare_dense_inputs(B, C, 0.5, seed=B + C)
        zn, k = rounded(zn, dt), 1.0
    else:
        zn, y, k, _ = case_inputs(f"{dt}_{what[1]}_B{what[2]}_C10")
    B, C = zn.shape
    assert _lib.load().rlvi_bare_form(B, C) == 1
    res = []
    try:
        for form in (0, 1):
            set_form(form)
            assert _lib.load().rlvi_bare_form(B, C) == form
            res.append(run(gpu, zn, y, k, dt))
    finally:
        unset_form()
    (l0, g0, o0, w0, s0), (l1, g1, o1, w1, s1) = res
    assert torch.equal(s0, s1) and torch.equal(w0, w1)
    assert torch.equal(o0[1:], o1[1:])
    loss_close(l1, float(l0))
    grad_close(torch, g1, g0.float().cpu().numpy(), dt)
    for r in res:
        check_vs_restatement(gpu, zn, y, k, dt, *r)


@pytest.mark.parametrize("key", ["f32_dense_B4097_C1023", "bf16_dense_B1024_C101", "f16_dense_B64_C10"])
def test_two_calls_give_the_same_bits(key, gpu):
    torch, ops, dev = gpu
    zn, y, k, dt = case_inputs(key)
    a = run(gpu, zn, y, k, dt)
    b = run(gpu, zn, y, k, dt)
    for x, yv in zip(a, b):
        assert torch.equal(x, yv)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("dt", DTYPES)
def test_strided_rows(dt, form, gpu):
    B, C, pitch = 300, 37, 42
    zn, y = synth.bare_dense_inputs(B, C, 0.7, seed=71)
    zn = rounded(zn, dt)
    try:
        set_form(form)
        res = run(gpu, zn, y, 1.0, dt, pitch=pitch)
    finally:
        unset_form()
    check_vs_restatement(gpu, zn, y, 1.0, dt, *res)


# C = 10 puts 16 rows in a wave and 64 in a workgroup's sweep of pass 1, 256 in the one-workgroup form's; C = 100
# (vectors of four, 16 lanes per row) 4, 16 and 64; C = 300 a row per wave, 4 and 16
@pytest.mark.parametrize("B,C,form", [(3, 10, 0), (15, 10, 0), (65, 10, 0), (257, 10, 1), (17, 100, 0), (65, 100, 1),
                                      (5, 300, 0), (17, 300, 1), (1024, 16, 1), (16, 1024, 1)])
def test_batches_around_the_tiles(B, C, form, gpu):
    zn, y = synth.bare_dense_inputs(B, C, 0.8, seed=100 + B + C)
    try:
        set_form(form)
        res = run(gpu, zn, y, 1.0, "f32")
    finally:
        unset_form()
    check_vs_restatement(gpu, zn, y, 1.0, "f32", *res)


@pytest.mark.parametrize("form", [0, 1])
def test_a_class_without_rows_and_a_column_of_minus_sixty(form, gpu):
    torch, ops, dev = gpu
    B, C = 200, 12
    zn, y = synth.bare_dense_inputs(B, C, 0.8, seed=131)
    y = np.where(y == C - 1, 0, y)                 # no row is labelled with the last class
    try:
        set_form(form)
        res = run(gpu, zn, y, 1.0, "f32")
        check_vs_restatement(gpu, zn, y, 1.0, "f32", *res)
        # a column that is -60 in every row: its clamped probability is 1e-8 everywhere, its deviation zero, the margin
        # of the rows labelled with it a rounding artefact -- they are skipped; everything else must hold, without a NaN
        zn2, y2 = synth.bare_dense_inputs(B, C, 0.8, seed=132)
        zn2[:, 3] = -60.0
        res = run(gpu, zn2, y2, 1.0, "f32")
        assert (y2 == 3).sum() > 5
        for t in res:
            assert torch.isfinite(t.float()).all()
        check_vs_restatement(gpu, zn2, y2, 1.0, "f32", *res, skip=(y2 == 3))
    finally:
        unset_form()


@pytest.mark.parametrize("B,C", [(1024, 101), (64, 10)])
def test_upstream_gradient_and_loss_scale_stay_on_the_device(B, C, gpu):
    """(1024, 101) takes the streaming form (the gradient is the M-step's, the factor multiplies w or is the kernel's
    grad_scale), (64, 10) the one-workgroup form (the forward's gradient times the factor)."""
    torch, ops, dev = gpu
    zn, y = synth.bare_dense_inputs(B, C, 0.5, seed=B + C)
    _, a, *_ = run(gpu, zn, y, 1.0, "f32")
    _, b, *_ = run(gpu, zn, y, 1.0, "f32", g_factor=3.0)
    ref = 3 * a.cpu().numpy()
    np.testing.assert_allclose(b.cpu().numpy(), ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())
    for dt in ("f32", "f16"):
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
        z = torch.from_numpy(zn).to(dev).to(tdtype(torch, dt)).requires_grad_(True)
        scaler.scale(ops.bare_loss(z, torch.from_numpy(y).to(dev))).backward()
        _, plain, *_ = run(gpu, rounded(zn, dt), y, 1.0, dt)
        ref = 1024.0 * plain.float().cpu().numpy()
        np.testing.assert_allclose(z.grad.float().cpu().numpy(), ref, rtol=F16_RTOL if dt == "f16" else 1e-7,
                                   atol=F16_ATOL * 1024)


@pytest.mark.parametrize("B,C", [(128, 10), (4096, 10)])
def test_labels_out_of_range_raise(B, C, gpu):
    torch, ops, dev = gpu
    from rlvi_amd import _lib
    zn, y = synth.bare_dense_inputs(B, C, 0.5, seed=91)
    z = torch.from_numpy(zn).to(dev).requires_grad_(True)
    for bad in (C, -1):
        t = torch.from_numpy(y.copy()).to(dev)
        t[17] = bad
        with pytest.raises(_lib.RlviError, match="out of range"):
            ops.bare_loss(z, t)
    assert ops.workspace(dev).status() == 0
    res = run(gpu, zn, y, 1.0, "f32")                               # a good batch afterwards
    check_vs_restatement(gpu, zn, y, 1.0, "f32", *res)


@pytest.mark.parametrize("B,C,dt", [(65536, 100, "f32"), (2048, 1500, "f32"), (1024, 2501, "bf16")])
def test_large_shapes_vs_restatement(B, C, dt, gpu):
    """The bench-sized batch in one call, and rows beyond 1024 elements (vectors of four: 16 per lane; odd: 64)."""
    d = synth.mstep_inputs(B, C, N=B, seed=B + C, zero_frac=0.0)
    zn, y = rounded(d["logits"], dt), d["labels"]
    res = run(gpu, zn, y, 1.0, dt)
    rows = np.sort(np.random.default_rng(B + C).choice(B, 64, replace=False))
    s = check_vs_restatement(gpu, zn, y, 1.0, dt, *res, rows=rows)
    assert 0 < s.sum() < B


def loop_setup(gpu, name):
    torch, ops, dev = gpu
    g = golden()
    X, y = synth.jocor_loop_inputs(int(g["loop/seed"]), 256, 16, 10)
    loader = [(torch.from_numpy(X[s:s + 64]), torch.from_numpy(y[s:s + 64]), torch.arange(s, s + 64))
              for s in range(0, 256, 64)]
    init = g[f"loop/{name}_init"]
    m, off = torch.nn.Linear(16, 10).to(dev), 0
    with torch.no_grad():
        for q in m.parameters():
            q.copy_(torch.from_numpy(init[off:off + q.numel()].reshape(q.shape)))
            off += q.numel()
    opt = torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    return g, loader, m, opt


def flat(m):
    return np.concatenate([q.detach().cpu().numpy().ravel() for q in m.parameters()])


@pytest.mark.parametrize("name", ["bare", "regular"])
def test_three_epochs_vs_reference(name, gpu):
    from rlvi_amd.methods import train_bare, train_regular
    g, loader, m, opt = loop_setup(gpu, name)
    for e in range(3):
        acc = train_bare(loader, m, opt, 10) if name == "bare" else train_regular(loader, m, opt)
        assert abs(acc - g[f"loop/{name}_acc"][e]) <= 1e-4, (e, acc)
        np.testing.assert_allclose(flat(m), g[f"loop/{name}_params"][e], rtol=1e-4, atol=1e-5, err_msg=f"epoch {e}")


def test_bare_loop_under_autocast_fp16_with_a_scaler(gpu):
    """The same three epochs with fp16 logits from autocast and a GradScaler: finite, and close to the reference's fp32
    run (the logits carry fp16 rounding)."""
    torch, ops, dev = gpu
    from rlvi_amd.methods.train_bare import WeightedCCE
    g, loader, m, opt = loop_setup(gpu, "bare")
    scaler = torch.amp.GradScaler("cuda", init_scale=256.0)
    loss_fn = WeightedCCE(k=1, num_class=10, reduction="none")
    for e in range(3):
        for images, labels, _ in loader:
            images, labels = images.to(dev), labels.to(dev)
            with torch.autocast("cuda", dtype=torch.float16):
                z = m(images)
                assert z.dtype == torch.float16
                loss = loss_fn(z, labels)
            opt.zero_grad()
            scaler.scale(loss.mean()).backward()
            assert m.weight.grad.dtype == torch.float32
            scaler.step(opt)
            scaler.update()
        p = flat(m)
        assert np.isfinite(p).all()
        np.testing.assert_allclose(p, g["loop/bare_params"][e], atol=3e-2, err_msg=f"epoch {e}")
    assert scaler.get_scale() >= 256.0
