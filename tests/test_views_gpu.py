"""The row kernels on tensor views (run with -m gpu on an MI355X): every vector-width fallback against a reference.

Every kernel that reads a [B, C] block picks its vector width V and its kernel form on the host from C, the row
pitch and the block's base address.  A fresh allocation is 256-byte aligned, so the rest of the suite decides V
through C alone.  Here the blocks are views (tests/views.py): a dense block whose base is off a 16-byte boundary
(what torch.chunk along the batch gives), an odd pitch, a column offset; logits and gradient placed independently.

Reference and bars are the project's own: logit_regimes.reference (float64) on regime_inputs(..., FINITE) -- the
masked rows' -inf columns near a row's end catch a lane that reads its neighbour's row -- with nll_failures,
grad_failures and lowp_grad_failures at REL / LOWP (test_logit_range_gpu.check_mstep); JoCoR and BARE against their
float64 restatements at test_jocor_gpu's and test_bare_gpu's bars; the in-batch E+M, the E-step and the threshold
against the oracle at the bars of test_gpu_parity.

Poison: everything around a logits view is NaN (the reference never sees it: any use shows) and the logits buffer
must come back bit-unchanged; a gradient buffer is 7.0 throughout before the call and every element outside the
view must be bit-identical to 7.0 afterwards.

M-step cases: rlvi_workspace_last_mstep_shape's V must equal views.expected_vector, the form the case's table entry,
and (V, form) must differ from the dense control's -- a case cannot silently degenerate into the control.  Each case
prints (form, V, G, K) and the largest |view - control| of residuals and gradient (recorded in
profiles/r20_views.md, not asserted: vector widths may sum in different orders).
"""
import ctypes
import functools

import numpy as np
import pytest

from logit_regimes import FINITE, REL, reference, regime_inputs
from rlvi_amd import synth
from test_bare_cpu import loss_and_grad
from test_bare_cpu import rounded as rounded_to
from test_gpu_parity import gpu, no_process_state_left_behind  # noqa: F401  (fixtures: the device, the hygiene check)
from test_jocor_cpu import restate as jocor_restate
from test_jocor_gpu import grad_close, loss_close
from test_logit_range_gpu import check_mstep, tdtype
from test_oracle_golden import rel_pi
from views import KINDS, expected_vector, layout, outside, place

pytestmark = pytest.mark.gpu

DT3 = ("f32", "bf16", "f16")
SIZE = {"f32": 4, "bf16": 2, "f16": 2}
NAN = float("nan")
SEVEN = 7.0


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(torch, t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def place_logits(gpu, zn, dt, kind):
    """(view, buffer, the buffer's bits before the call): `zn` in dtype `dt`, NaN around it."""
    torch, ops, dev = gpu
    z, buf = place(torch, torch.from_numpy(np.ascontiguousarray(zn, np.float32)).to(tdtype(torch, dt)), kind, NAN, dev)
    assert z.stride(1) == 1 and int(torch.isnan(buf).sum()) == buf.numel() - z.numel()
    return z, buf, bits(torch, buf).clone()


def place_grad(gpu, B, C, dt, kind):
    """(view, buffer): a gradient block of kind `kind` in a buffer that is 7.0 throughout."""
    torch, ops, dev = gpu
    g, buf = place(torch, torch.zeros((B, C), dtype=tdtype(torch, dt)), kind, SEVEN, dev)
    buf.fill_(SEVEN)
    return g, buf


def check_poison(torch, what, logits=(), grads=()):
    """logits: (buffer, bits before) pairs that must be bit-unchanged; grads: (view, buffer) pairs whose elements
    outside the view must still be 7.0, bit for bit."""
    for buf, before in logits:
        assert torch.equal(bits(torch, buf), before), f"{what}: the logits buffer was written"
    for g, buf in grads:
        m = outside(torch, g, buf)
        left = bits(torch, buf)[m]
        seven = bits(torch, torch.full((1,), SEVEN, dtype=buf.dtype, device=buf.device))
        bad = int((left != seven).sum())
        assert bad == 0, f"{what}: {bad} gradient-buffer elements outside the view were written"
        assert not torch.isnan(g.float()).any(), f"{what}: NaN in the gradient"


# ====================================================================================================== M-step
def last_dispatch(ws):
    from rlvi_amd import _lib
    L = _lib.load()
    shape = int(L.rlvi_workspace_last_mstep_shape(ws.ptr))
    return int(L.rlvi_workspace_last_mstep_form(ws.ptr)), shape & 255, (shape >> 8) & 255, shape >> 16


@functools.lru_cache(maxsize=2)
def mstep_problem(B, C, dt):
    d = regime_inputs(B, C, dt, seed=B + C, N=B + 17, zero_frac=0.1, regimes=FINITE)
    return d, reference(d["logits"], d["labels"], d["idx"], d["weights"])


def run_mstep(gpu, d, dt, zkind, gkind, want_grad=True, what=""):
    """ops.mstep_fwd_bwd at inv_scale = 1 on a workspace of its own with the logits placed as `zkind` and the gradient
    as `gkind`; the poison checks; (out, gradient as fp32 or None, residuals, (form, V, G, K), expected V)."""
    torch, ops, dev = gpu
    B, C = d["logits"].shape
    z, zbuf, before = place_logits(gpu, d["logits"], dt, zkind)
    g, gbuf = place_grad(gpu, B, C, dt, gkind) if want_grad else (None, None)
    ws = ops.Workspace(dev, d["weights"].shape[0], B)
    res = torch.from_numpy(d["residuals"].copy()).to(dev)
    out, grad = ops.mstep_fwd_bwd(z, torch.from_numpy(d["labels"]).to(dev), torch.from_numpy(d["idx"]).to(dev),
                                  torch.from_numpy(d["weights"]).to(dev), res, inv_scale=1.0, want_grad=want_grad,
                                  grad=g, ws=ws)
    torch.cuda.synchronize()
    assert ws.status() == 0
    assert (grad is g) if want_grad else (grad is None)
    check_poison(torch, what, [(zbuf, before)], [(g, gbuf)] if want_grad else [])
    want_v = expected_vector(SIZE[dt], C, [z, g])
    return (out.cpu().numpy(), None if g is None else g.float().cpu().numpy(), res.cpu().numpy(), last_dispatch(ws),
            want_v)


# B, C, dtypes, kinds, the control's form, a view's form, {kind: (G, K)} where the case is there for one body.
# Forms (rlvi_workspace_last_mstep_form): 1 register rows, 2 four-wave tiles, 3 16-wave tiles, 4 the word-wise 2-byte
# tile, 5 long rows.  Each shape is the smallest that selects its branch.
MSTEP_TABLE = [
    (300, 104, DT3, KINDS[1:], 1, 1, {}),                                        # register rows, V from 8 / 4 down to 1
    (300, 8, ("f32",), ("elem+1", "elem+2", "pitch+1"), 1, 1, {}),
    (9001, 100, ("f32",), ("rows+1", "elem+1", "elem+2", "pitch+4", "col+1"), 2, 1, {}),     # wave tile -> register rows
    (33001, 100, ("f32",), ("elem+1", "elem+2"), 2, 1, {"elem+1": (4, 32), "elem+2": (4, 16)}),
    (57365, 100, ("f32",), ("elem+1", "pitch+4"), 3, 1, {}),                      # 16-wave form -> register rows
    (33001, 101, ("bf16", "f16"), ("rows+1", "elem+1", "pitch+1"), 4, 1, {}),     # word-wise tile -> register rows
    (20005, 104, ("bf16",), ("elem+1", "elem+2", "elem+4", "pitch+4"), 2, 1, {}),
    (70, 1000, ("f32",), ("elem+1",), 1, 5, {}),                                  # register rows -> a workgroup per row
    # (1030 rows at a row per wave are more than 512 wave tiles: the control takes the LDS tile, not register rows)
    (1030, 1000, ("f32",), ("elem+1",), 2, 5, {}),                                # wave tile -> a wave per row
    (70, 2052, ("f32",), ("elem+1", "elem+2"), 5, 5, {}),                         # long rows at V = 4 -> 1, 2
    (130, 4104, ("bf16",), ("elem+1", "elem+4"), 5, 5, {}),                       # long rows at V = 8 -> 1, 4
]


def expected_dispatch(B, C, dt, zkind, gkind, control_form, view_form):
    """(V, form) a placement must get: V from the placements' offsets and pitches in a 256-byte aligned buffer; the
    control's form while every block is dense and 16-byte aligned, else the view's."""
    s = SIZE[dt]
    blocks = [(4096 + off * s, pitch) for _, off, pitch in (layout(k, B, C) for k in (zkind, gkind) if k is not None)]
    plain = all(pitch == C and p % 16 == 0 for p, pitch in blocks)
    return expected_vector(s, C, blocks), (control_form if plain else view_form)


def mstep_cases():
    """The table's controls, and its views whose expected (V, form) differs from the control's."""
    cases = []
    for B, C, dts, kinds, cform, vform, bodies in MSTEP_TABLE:
        for dt in dts:
            control = expected_dispatch(B, C, dt, "dense", "dense", cform, vform)
            cases.append((B, C, dt, "dense", control, control, None))
            for kind in kinds:
                want = expected_dispatch(B, C, dt, kind, kind, cform, vform)
                if want != control:
                    cases.append((B, C, dt, kind, want, control, bodies.get(kind)))
    return cases


MSTEP_CASES = mstep_cases()
PAIRS = [("dense", "elem+1"), ("elem+1", "dense"), ("pitch+4", "pitch+2"), ("dense", "pitch+1")]
SUBSET = [(300, 104, dt, 1, 1) for dt in DT3] + [(9001, 100, "f32", 2, 1)]
_controls = {}


def control_run(gpu, B, C, dt):
    """The dense control of a shape: (residuals, gradient, (form, V, G, K)), kept for the shape's view cases."""
    key = (B, C, dt)
    if key not in _controls:
        _controls.clear()                                   # (one shape at a time: the blocks are large)
        d, ref = mstep_problem(B, C, dt)
        out, grad, res, took, _ = run_mstep(gpu, d, dt, "dense", "dense", what=f"{B} x {C} {dt} control")
        _controls[key] = (res, grad, took)
    return _controls[key]


def report(what, took, res, grad, control):
    with np.errstate(all="ignore"):
        dr = float(np.nanmax(np.abs(res.astype(np.float64) - control[0])))
        dg = float(np.nanmax(np.abs(grad.astype(np.float64) - control[1]))) if grad is not None else float("nan")
    print(f"\n    {what:36s} form {took[0]} V {took[1]} G {took[2]} K {took[3]}   max|view - control|: residuals "
          f"{dr:.3e} gradient {dg:.3e}")


def test_the_case_list_keeps_what_differs_from_its_control():
    """(needs no device, but belongs to this table)  Every view case expects another V or another form than its
    control; the table's views that a launcher cannot tell from the control (rows+1 where C * s is a multiple of 16,
    elem+4 and pitch+4 in fp32) are not in the list; every form is left at least once."""
    views = [c for c in MSTEP_CASES if c[3] != "dense"]
    assert len(MSTEP_CASES) - len(views) == 14 and len(views) >= 40
    assert all(want != control for _, _, _, _, want, control, _ in views)
    kept = {(b, c, dt, k) for b, c, dt, k, *_ in views}
    assert (300, 104, "f32", "rows+1") not in kept and (300, 104, "f32", "elem+4") not in kept
    assert (300, 104, "bf16", "elem+4") in kept and (300, 104, "f16", "pitch+4") in kept
    assert (9001, 100, "f32", "rows+1") not in kept                   # (+400 bytes: still 16-byte aligned)
    assert (33001, 101, "bf16", "rows+1") in kept                     # (+202 bytes)
    assert {(control[1], want[1]) for *_, want, control, _ in views} >= {(2, 1), (3, 1), (4, 1), (1, 5), (5, 5), (1, 1)}
    assert {want[0] for _, _, dt, _, want, _, _ in views if dt == "f32"} == {1, 2, 4}
    assert {want[0] for _, _, dt, _, want, _, _ in views if dt != "f32"} == {1, 2, 4}
    for B, C, dt, cform, vform in SUBSET:
        control = expected_dispatch(B, C, dt, "dense", "dense", cform, vform)
        for zk, gk in PAIRS:
            assert expected_dispatch(B, C, dt, zk, gk, cform, vform) != control


@pytest.mark.parametrize("B,C,dt,kind,want,control,body", MSTEP_CASES,
                         ids=[f"{b}x{c}-{dt}-{k}" for b, c, dt, k, *_ in MSTEP_CASES])
def test_mstep_on_a_view(B, C, dt, kind, want, control, body, gpu):
    """Logits and gradient both placed as `kind`."""
    torch, ops, dev = gpu
    d, ref = mstep_problem(B, C, dt)
    what = f"{B} x {C} {dt} {kind}"
    ctl = control_run(gpu, B, C, dt)
    out, grad, res, took, want_v = run_mstep(gpu, d, dt, kind, kind, what=what)
    report(what, took, res, grad, ctl)
    assert ctl[2][1] == control[0] and ctl[2][0] == control[1], f"{what}: the control ran {ctl[2]}, expected {control}"
    assert want_v == want[0], f"{what}: the allocation is not 16-byte aligned?"
    assert took[1] == want[0], f"{what}: V {took[1]}, expected_vector gives {want[0]}"
    assert took[0] == want[1], f"{what}: kernel form {took[0]}, this case is here for form {want[1]}"
    if kind != "dense":
        assert (took[1], took[0]) != (ctl[2][1], ctl[2][0]), f"{what}: the case degenerated into its control"
    if body is not None:
        assert took[2:] == body, f"{what}: lanes per row and slots {took[2:]}, this case is here for {body}"
    if took[0] in (4, 5):
        assert took[2:] == (0, 0)
    check_mstep(torch, d, ref, out, grad, res, dt, what)


@pytest.mark.parametrize("zkind,gkind", PAIRS, ids=[f"{z}-{g}" for z, g in PAIRS])
@pytest.mark.parametrize("B,C,dt,cform,vform", SUBSET, ids=[f"{b}x{c}-{dt}" for b, c, dt, _, _ in SUBSET])
def test_mstep_logits_and_gradient_placed_independently(B, C, dt, cform, vform, zkind, gkind, gpu):
    torch, ops, dev = gpu
    d, ref = mstep_problem(B, C, dt)
    what = f"{B} x {C} {dt} {zkind} / {gkind}"
    ctl = control_run(gpu, B, C, dt)
    want = expected_dispatch(B, C, dt, zkind, gkind, cform, vform)
    out, grad, res, took, want_v = run_mstep(gpu, d, dt, zkind, gkind, what=what)
    report(what, took, res, grad, ctl)
    assert want_v == want[0]
    assert took[1] == want[0], f"{what}: V {took[1]}, expected_vector gives {want[0]}"
    assert took[0] == want[1], f"{what}: kernel form {took[0]}, expected {want[1]}"
    assert (took[1], took[0]) != (ctl[2][1], ctl[2][0]), f"{what}: the case degenerated into its control"
    check_mstep(torch, d, ref, out, grad, res, dt, what)


@pytest.mark.parametrize("kind", ["elem+1", "elem+2", "pitch+2", "col+1"])
@pytest.mark.parametrize("B,C,dt,cform,vform", SUBSET, ids=[f"{b}x{c}-{dt}" for b, c, dt, _, _ in SUBSET])
def test_mstep_forward_only_and_evaluation_on_a_view(B, C, dt, cform, vform, kind, gpu):
    """want_grad=False on a view: out and residuals bit for bit those of the with-gradient call on the same view (as
    test_strided_forward_only_and_evaluation_forms holds for a pitch).  evaluate_batch on the view: the bits of the
    with-gradient call with pi = 1, identity rows and inv_scale = 1 / B, and the reference's plain CE."""
    torch, ops, dev = gpu
    d, ref = mstep_problem(B, C, dt)
    what = f"{B} x {C} {dt} {kind}"
    want = expected_dispatch(B, C, dt, kind, None, cform, vform)
    out, grad, res, took, _ = run_mstep(gpu, d, dt, kind, kind, what=what)
    out2, none, res2, took2, want_v = run_mstep(gpu, d, dt, kind, None, want_grad=False, what=what + " forward only")
    assert none is None and took2 == took and (took2[1], took2[0]) == want and want_v == want[0]
    assert np.array_equal(out2, out) and np.array_equal(res2, res), f"{what}: forward only differs"
    # the evaluation form
    z, zbuf, before = place_logits(gpu, d["logits"], dt, kind)
    g, gbuf = place_grad(gpu, B, C, dt, kind)
    y = torch.from_numpy(d["labels"]).to(dev)
    ws = ops.Workspace(dev, B, B)
    rows = torch.zeros(B, device=dev)
    o1, _ = ops.mstep_fwd_bwd(z, y, torch.arange(B, device=dev), torch.ones(B, device=dev), rows, inv_scale=1.0 / B,
                              grad=g, ws=ws)
    o1 = o1.cpu().numpy()
    o2 = ops.evaluate_batch(z, y, ws=ws).cpu().numpy()
    torch.cuda.synchronize()
    assert ws.status() == 0 and last_dispatch(ws) == took
    check_poison(torch, what + " evaluation", [(zbuf, before)], [(g, gbuf)])
    assert np.array_equal(o1, o2), f"{what}: evaluation form {o2} against the with-gradient call {o1}"
    ev = reference(d["logits"], d["labels"], None, None)
    assert abs(float(o2[2]) - ev["loss"]) <= REL * abs(ev["loss"]) and float(o2[3]) == float(ev["hits"])
    assert abs(float(o2[0]) - ev["loss"] / B) <= REL * abs(ev["loss"] / B)


# ---------------------------------------------------------------- ops.mstep_fwd_bwd validates grad= and out=
def test_mstep_fwd_bwd_refuses_a_gradient_or_out_it_cannot_write(gpu):
    torch, ops, dev = gpu
    B, C = 64, 12
    d = synth.mstep_inputs(B, C, N=B, seed=3)
    t = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    ws = ops.Workspace(dev, B, B)

    def call(z=None, **kw):
        res = t["residuals"].clone()
        r = ops.mstep_fwd_bwd(t["logits"] if z is None else z, t["labels"], t["idx"], t["weights"], res, ws=ws, **kw)
        torch.cuda.synchronize()
        return r

    wide = torch.zeros((B, 2 * C), device=dev)
    bad_grads = {
        "dtype": torch.zeros((B, C), dtype=torch.bfloat16, device=dev),
        "shape: rows": torch.zeros((B - 1, C), device=dev),
        "shape: columns": torch.zeros((B, C + 4), device=dev),
        "shape: flat": torch.zeros(B * C, device=dev),
        "device": torch.zeros((B, C)),
        "column stride": wide[:, ::2],
    }
    for name, g in bad_grads.items():
        with pytest.raises(ValueError, match="grad must be"):
            call(grad=g)
    # the dtype is that of the logits as the kernel gets them: fp64 logits run as fp32, bf16 logits want a bf16 gradient
    with pytest.raises(ValueError, match="grad must be"):
        call(z=t["logits"].double(), grad=torch.zeros((B, C), dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="grad must be"):
        call(z=t["logits"].bfloat16(), grad=torch.zeros((B, C), device=dev))
    bad_outs = {
        "dtype": torch.zeros(4, dtype=torch.float64, device=dev),
        "length": torch.zeros(5, device=dev),
        "stride": torch.zeros(8, device=dev)[::2],
        "device": torch.zeros(4),
    }
    for name, o in bad_outs.items():
        with pytest.raises(ValueError, match="out must be"):
            call(out=o)
    assert not wide.any(), "a refused call wrote"
    # accepted: strided rows (the pad columns stay), a caller's out; and not looked at where it is not used
    want_out, want = call()
    wide.fill_(SEVEN)
    g = wide[:, :C]
    o = torch.zeros(4, device=dev)
    got_out, got = call(grad=g, out=o)
    assert got is g and got_out is o and torch.equal(got, want) and torch.equal(o, want_out)
    assert torch.equal(wide[:, C:], torch.full((B, C), SEVEN, device=dev))
    assert call(grad=bad_grads["dtype"], want_grad=False)[1] is None
    assert ws.status() == 0


# ======================================================================================================= JoCoR
JC_COMBOS = [("dense", "dense", "dense", "dense"), ("dense", "elem+1", "dense", "dense"),
             ("elem+2", "dense", "dense", "elem+1"), ("pitch+4", "pitch+2", "pitch+1", "dense"),
             ("dense", "dense", None, "elem+1")]
JC_B, JC_LAM = 300, 0.1
JC_K = int(0.7 * JC_B)


@functools.lru_cache(maxsize=4)
def jocor_problem(C, dt):
    d1 = synth.mstep_inputs(JC_B, C, N=JC_B, seed=71 + C)
    d2 = synth.mstep_inputs(JC_B, C, N=JC_B, seed=72 + C)
    z1, z2 = rounded_to(d1["logits"], dt), rounded_to(d2["logits"], dt)
    return z1, z2, d1["labels"], jocor_restate(z1, z2, d1["labels"], JC_K, JC_LAM)


def run_jocor(gpu, C, dt, kinds):
    """ops.jocor_forward on z1 / z2 placed as kinds[0:2], the backward C entry on gradients placed as kinds[2:4]
    (None: a null pointer); the poison checks; (out, sel, g1, g2) on the host."""
    torch, ops, dev = gpu
    from rlvi_amd import _lib
    z1n, z2n, y, _ = jocor_problem(C, dt)
    what = f"JoCoR {JC_B} x {C} {dt} {kinds}"
    z1, b1, before1 = place_logits(gpu, z1n, dt, kinds[0])
    z2, b2, before2 = place_logits(gpu, z2n, dt, kinds[1])
    t = torch.from_numpy(y).to(dev)
    out, pick, sel = ops.jocor_forward(z1, z2, t, JC_K, JC_LAM)
    g = [place_grad(gpu, JC_B, C, dt, k) if k is not None else (None, None) for k in kinds[2:]]
    (g1, gb1), (g2, gb2) = g
    fn = getattr(_lib.load(), f"rlvi_jocor_bwd_{dt}")
    rc = fn(ptr(z1), z1.stride(0), ptr(z2), z2.stride(0), ptr(t), ptr(sel), JC_B, C, JC_K, JC_LAM, None, None,
            ptr(g1), g1.stride(0) if g1 is not None else 0, ptr(g2), g2.stride(0) if g2 is not None else 0, stream(torch))
    torch.cuda.synchronize()
    assert rc == 0 and ops.workspace(dev).status() == 0
    check_poison(torch, what, [(b1, before1), (b2, before2)], [p for p in g if p[0] is not None])
    return out.cpu().numpy(), sel.cpu().numpy(), g1, g2


@pytest.mark.parametrize("kinds", JC_COMBOS, ids=["-".join(str(k) for k in c) for c in JC_COMBOS])
@pytest.mark.parametrize("dt", DT3)
@pytest.mark.parametrize("C", [16, 104, 520, 1032])
def test_jocor_four_blocks_placed_independently(C, dt, kinds, gpu):
    """C = 16, 104, 520: four, sixteen and sixty-four lanes per row; 1032: the long-row kernel.  The forward picks V
    from the two logit blocks, the backward from all four: they differ for the same rows."""
    torch, ops, dev = gpu
    _, _, y, (L, _, _, _, ref_sel, r1, r2) = jocor_problem(C, dt)
    out, sel, g1, g2 = run_jocor(gpu, C, dt, kinds)
    control = run_jocor(gpu, C, dt, JC_COMBOS[0])[1] if kinds != JC_COMBOS[0] else sel
    assert np.array_equal(sel, control), "the selection differs from the dense control's"
    assert int(sel.sum()) == JC_K
    assert abs(float(out[0]) - L) <= REL * abs(L)                    # (check_vs_restatement's bars)
    for mine, want in ((g1, r1), (g2, r2)):
        if mine is not None:
            grad_close(torch, mine, want.astype(np.float32), dt)


# ======================================================================================================== BARE
BARE_SHAPES = [(64, 16, 1), (100, 104, 1), (16, 1024, 1), (300, 104, 0), (5, 2052, 0)]      # (B, C, form)
BARE_KINDS = ["dense", "elem+1", "rows+1", "pitch+1", "col+1"]


@functools.lru_cache(maxsize=4)
def bare_problem(B, C, dt):
    zn, y = synth.bare_dense_inputs(B, C, 0.8, seed=100 + B + C)
    return rounded_to(zn, dt), y


_bare_controls = {}


def run_bare(gpu, B, C, dt, kind):
    """ops.bare_loss with backward and ops.bare_forward on logits placed as `kind`: (loss, grad, out, w, sel)."""
    torch, ops, dev = gpu
    zn, y = bare_problem(B, C, dt)
    z, zbuf, before = place_logits(gpu, zn, dt, kind)
    zz = z.detach().requires_grad_(True)
    t = torch.from_numpy(y).to(dev)
    out = torch.full((4,), -1.0, device=dev)
    loss = ops.bare_loss(zz, t, 1.0, out=out)
    loss.backward()
    out2, w, sel = ops.bare_forward(z, t, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and zz.grad.shape == z.shape and zz.grad.dtype == z.dtype
    check_poison(torch, f"BARE {B} x {C} {dt} {kind}", [(zbuf, before)])
    return loss.detach(), zz.grad, out, w, sel


def bare_control(gpu, B, C, dt):
    key = (B, C, dt)
    if key not in _bare_controls:
        _bare_controls[key] = run_bare(gpu, B, C, dt, "dense")
    return _bare_controls[key]


@pytest.mark.parametrize("kind", BARE_KINDS)
@pytest.mark.parametrize("dt", DT3)
@pytest.mark.parametrize("B,C,form", BARE_SHAPES)
def test_bare_logits_on_a_view(B, C, form, dt, kind, gpu):
    from rlvi_amd import _lib
    from test_bare_gpu import check_vs_restatement
    torch, ops, dev = gpu
    assert _lib.load().rlvi_bare_form(B, C) == form
    zn, y = bare_problem(B, C, dt)
    res = bare_control(gpu, B, C, dt) if kind == "dense" else run_bare(gpu, B, C, dt, kind)
    check_vs_restatement(gpu, zn, y, 1.0, dt, *res)
    ctl = bare_control(gpu, B, C, dt)
    assert torch.equal(res[4], ctl[4]) and torch.equal(res[3], ctl[3]), "selection or w differ from the dense control's"
    assert ops.workspace(dev).status() == 0


@pytest.mark.parametrize("gkind", ["elem+1", "pitch+1"])
@pytest.mark.parametrize("dt", DT3)
@pytest.mark.parametrize("B,C", [(b, c) for b, c, f in BARE_SHAPES if f == 1])
def test_bare_one_workgroup_gradient_on_a_view(B, C, dt, gkind, gpu):
    """The C entry with dense logits (V = 4) and a gradient block that vectors of four do not fit: the one-workgroup
    form's store in single elements, which ops never asks for."""
    from rlvi_amd import _lib
    from test_bare_gpu import check_outputs
    torch, ops, dev = gpu
    zn, y = bare_problem(B, C, dt)
    what = f"BARE {B} x {C} {dt} gradient {gkind}"
    z, zbuf, before = place_logits(gpu, zn, dt, "dense")
    g, gbuf = place_grad(gpu, B, C, dt, gkind)
    assert expected_vector(SIZE[dt], C, [z]) >= 4 and expected_vector(SIZE[dt], C, [g]) == 1
    t = torch.from_numpy(y).to(dev)
    w, sel, out = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(4, device=dev)
    ws = ops.workspace(dev)
    rc = getattr(_lib.load(), f"rlvi_bare_fwd_{dt}")(ptr(z), z.stride(0), ptr(t), B, C, 1.0, ptr(w), ptr(sel), ptr(out),
                                                     ptr(g), g.stride(0), ws.ptr, stream(torch))
    torch.cuda.synchronize()
    assert rc == 0 and ws.status() == 0
    check_poison(torch, what, [(zbuf, before)], [(g, gbuf)])
    ctl = bare_control(gpu, B, C, dt)
    assert torch.equal(sel, ctl[4]) and torch.equal(w, ctl[3]) and torch.equal(out, ctl[2])
    s = check_outputs(out, w, sel, B)
    L, ref_grad = loss_and_grad(zn, y, s)
    loss_close(out[0], L)
    grad_close(torch, g, ref_grad.astype(np.float32), dt, what)


# ======================================================================================================= top-k
@pytest.mark.parametrize("dt", DT3)
@pytest.mark.parametrize("C", [8, 104, 1000])
def test_topk_hits_on_a_view(C, dt, gpu):
    torch, ops, dev = gpu
    B, ks = 300, (1, 5)
    d = regime_inputs(B, C, dt, seed=C, regimes=FINITE)
    rank = reference(d["logits"], d["labels"], None, None)["rank"]        # (ties: the lower column first)
    want = [int((rank < k).sum()) for k in ks]
    y = torch.from_numpy(d["labels"]).to(dev)
    for kind in ("dense", "elem+1", "pitch+1", "col+1"):
        z, zbuf, before = place_logits(gpu, d["logits"], dt, kind)
        got = ops.topk_hits(z, y, ks).cpu().numpy().tolist()
        check_poison(torch, f"top-k {B} x {C} {dt} {kind}", [(zbuf, before)])
        if kind == "dense":
            dense = got
        assert got == dense and got == want, (kind, got, dense, want)


# ================================================================================================== fused E+M
FUSED = [(4096, 10, "elem+1"),       # stays in one launch: the row-per-thread form checks no alignment
         (4096, 10, "pitch+2"),      # composition
         (1024, 64, "elem+1"),       # composition
         (16384, 100, "rows+1"),     # dense, 16-byte aligned: the one-launch form
         (16384, 100, "elem+2")]     # composition


@functools.lru_cache(maxsize=2)
def fused_problem(B, C):
    from oracle import rlvi_oracle as oracle
    oracle.build()
    d = synth.mstep_inputs(B, C, seed=B + C)
    loss, hit = oracle.nll_rows(d["logits"], d["labels"])
    l2, w2 = loss.copy(), np.ones(B, np.float32)
    it = oracle.update_sample_weights(l2, w2)
    ref = oracle.mstep(d["logits"], d["labels"], np.arange(B), w2, np.zeros(B, np.float32))
    return d, l2, w2, it, ref, int(hit.sum())


@pytest.mark.parametrize("B,C,kind", FUSED, ids=[f"{b}x{c}-{k}" for b, c, k in FUSED])
def test_fused_em_on_a_view(B, C, kind, gpu):
    """Logits and gradient placed as `kind`, against the oracle's composition at test_fused_em_matches_composition's
    bars."""
    torch, ops, dev = gpu
    d, l2, w2, it, ref, hits = fused_problem(B, C)
    what = f"fused E+M {B} x {C} {kind}"
    z, zbuf, before = place_logits(gpu, d["logits"], "f32", kind)
    g, gbuf = place_grad(gpu, B, C, "f32", kind)
    pit = torch.ones(B, device=dev)
    ws = ops.Workspace(dev, B, B)
    out, grad, rows, iters = ops.fused_em(z, torch.from_numpy(d["labels"]).to(dev), pit, grad=g, ws=ws)
    torch.cuda.synchronize()
    assert ws.status() == 0 and grad is g
    check_poison(torch, what, [(zbuf, before)], [(g, gbuf)])
    assert int(iters) == it
    rel, small = rel_pi(pit.cpu().numpy(), w2)
    assert rel <= REL and small <= 1e-7
    np.testing.assert_allclose(rows.cpu().numpy(), l2, rtol=REL, atol=1e-6)
    assert abs(float(out[0]) - float(ref["loss"])) <= REL * abs(float(ref["loss"]))
    assert float(out[3]) == float(hits)
    diff = g.cpu().numpy().astype(np.float64) - ref["grad"]
    assert np.sqrt((diff ** 2).sum()) <= REL * np.sqrt((ref["grad"].astype(np.float64) ** 2).sum())


# ================================================================================================ 1-D vectors
def off_by_one(torch, a, sentinel, dev):
    """(buf[1 : 1 + N], buf): `a` in a vector that is 4-byte aligned and no more, a sentinel before and behind it."""
    buf = torch.full((a.shape[0] + 2,), sentinel, dtype=torch.float32, device=dev)
    v = buf[1:-1]
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v, buf


def sentinels_kept(torch, buf, sentinel):
    want = bits(torch, torch.full((2,), sentinel, dtype=torch.float32, device=buf.device))
    return torch.equal(bits(torch, buf)[[0, -1]], want)


@pytest.mark.parametrize("N", [1025, 70001])
def test_estep_and_threshold_on_vectors_off_a_16_byte_boundary(N, gpu, oracle):
    """estep_deep and the threshold / truncation entry on residuals and weights that start 4 bytes behind a 16-byte
    boundary, at the bars of test_estep_vs_oracle_sizes and test_threshold_vs_oracle_sizes."""
    torch, ops, dev = gpu
    r = synth.residual_vector("bimodal", N, seed=N)
    w0 = np.random.default_rng(N).random(N).astype(np.float32)
    rt, rbuf = off_by_one(torch, r, -123.0, dev)
    wt, wbuf = off_by_one(torch, w0, SEVEN, dev)
    iters = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = ops.Workspace(dev, N, 0)
    ops.estep_deep(rt, wt, iters=iters, ws=ws)
    torch.cuda.synchronize()
    assert ws.status() == 0
    assert sentinels_kept(torch, rbuf, -123.0) and sentinels_kept(torch, wbuf, SEVEN)
    rr, ww = r.copy(), w0.copy()
    it, err, _ = oracle.update_sample_weights(rr, ww, trace=True)
    got = wt.cpu().numpy()
    if not np.min(np.abs(err - 1e-3)) < 1e-5 * 1e-3:          # (the stop decision is not within rounding of tol)
        assert int(iters) == it
        rel, small = rel_pi(got, ww)
        assert rel <= REL and small <= 1e-7
    assert np.array_equal(rt.cpu().numpy(), rr)
    assert got.max() == np.float32(1.0)

    rng = np.random.default_rng(N)
    w = rng.random(N).astype(np.float32)
    w[rng.random(N) < 0.2] = 1.0
    w[rng.random(N) < 0.1] = 0.0
    thr_ref, _, _ = oracle.false_negative_criterion(w, full=True)
    wt, wbuf = off_by_one(torch, w, SEVEN, dev)
    ws = ops.Workspace(dev, N, 0)
    thr = ops.fn_threshold(wt, ws=ws)
    assert float(thr) == float(thr_ref)
    prev = float(thr_ref) + 0.01 if N % 2 else 0.0
    thr2, mask, kept = ops.threshold_truncate(wt, prev, want_mask=True, ws=ws)
    expect = max(np.float32(prev), thr_ref)
    assert float(thr2) == float(expect)
    w2 = w.copy()
    m_ref = oracle.truncate(w2, expect)
    assert np.array_equal(wt.cpu().numpy(), w2)
    assert np.array_equal(mask.cpu().numpy(), m_ref)
    assert int(kept) == int(m_ref.sum())
    assert ws.status() == 0 and sentinels_kept(torch, wbuf, SEVEN)
