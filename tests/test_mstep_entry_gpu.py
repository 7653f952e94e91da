"""The 16-wave fp32 M-step form (mstep_wave_kernel, ENTRY_FIRST) computes its lane geometry behind the issue of its
tile loads and takes its load addresses as scalar base + 32-bit lane offset + immediate.  What that entry can get wrong
is checked here on the smallest launches that reach the form: it is taken only when no wave has a second tile and the
grid fills at least four fifths of the CUs, so the row counts come from the device's CU count.

Every case is checked two ways: against the CPU oracle at the suite's 1e-5 bars (loss, gradient, residuals, hits), and
bit for bit (gradient, residuals) against the four-wave form of the same launch (RLVI_MSTEP_CUWIDE=0), whose entry is
the old one.  A case whose launch did not take the 16-wave form (rlvi_workspace_last_mstep_form != 3) is skipped.
"""
import numpy as np
import pytest

from rlvi_amd import synth
from test_oracle_golden import REL

pytestmark = pytest.mark.gpu

FORM_CUWIDE = 3          # ws_note_mstep code of the 16-wave form; 2 = four-wave tiles
R = 16                   # rows of a wave tile (four lanes per row)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rlvi_amd import _lib, ops
    _lib.load()
    return torch, ops, torch.device("cuda:0")


@pytest.fixture(autouse=True)
def nothing_left_behind():
    """No knob, sticky status or accumulate-mode record outlives a test (they are process-wide)."""
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


def workgroups(torch):
    """The fewest 16-wave workgroups the launcher accepts for the form: four fifths of the CUs, rounded up."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (4 * cus + 4) // 5


def rows_for(torch, partial_workgroup=False, trailing=0):
    nb = workgroups(torch)
    tiles = 16 * nb if not partial_workgroup else 16 * (nb - 1) + 5      # (eleven waves only join the barrier)
    return tiles * R + trailing


def last_form(ops, dev, ws=None):
    from rlvi_amd import _lib
    return _lib.load().rlvi_workspace_last_mstep_form((ws or ops.workspace(dev)).ptr)


def launch(gpu, d, cuwide, idx=True, residuals=True, want_grad=True):
    """One M-step call with RLVI_MSTEP_CUWIDE = cuwide -> (out[4], grad or None, residuals or None, form)"""
    torch, ops, dev = gpu
    from rlvi_amd import _lib
    L = _lib.load()
    z = torch.from_numpy(d["logits"]).to(dev)
    lab = torch.from_numpy(d["labels"]).to(dev)
    ix = torch.from_numpy(d["idx"]).to(dev) if idx else None
    w = torch.from_numpy(d["weights"]).to(dev)
    res = torch.from_numpy(d["residuals"].copy()).to(dev) if residuals else None
    _lib.check(L.rlvi_tune_set(b"RLVI_MSTEP_CUWIDE", cuwide), "tune")
    try:
        out, grad = ops.mstep_fwd_bwd(z, lab, ix, w, res, want_grad=want_grad)
        torch.cuda.synchronize()
        form = last_form(ops, dev)
    finally:
        L.rlvi_tune_unset(b"RLVI_MSTEP_CUWIDE")
    return (out.cpu().numpy(), grad.cpu().numpy() if grad is not None else None,
            res.cpu().numpy() if res is not None else None, form)


def check_oracle(oracle, d, out, grad, res, idx=True):
    B = d["logits"].shape[0]
    r0 = d["residuals"].copy()
    ix = d["idx"] if idx else np.arange(B, dtype=np.int64)
    ref = oracle.mstep(d["logits"], d["labels"], ix, d["weights"], r0)
    assert abs(float(out[0]) - float(ref["loss"])) <= REL * abs(float(ref["loss"]))
    assert float(out[3]) == float(round(float(ref["prec1"]) * B / 100.0))
    if res is not None:
        np.testing.assert_allclose(res, r0, rtol=REL, atol=1e-6)
    if grad is not None:
        diff = grad.astype(np.float64) - ref["grad"]
        assert np.sqrt((diff ** 2).sum()) <= REL * np.sqrt((ref["grad"].astype(np.float64) ** 2).sum())
        assert np.abs(diff).max() <= 1e-6


def check_same_bits(a, b):
    """16-wave against four-wave: what the stores carry is identical; the batch scalars agree to fp64 summation order
    (the per-workgroup records group the rows differently)."""
    if a[1] is not None:
        assert np.array_equal(a[1], b[1]), "gradient"
    if a[2] is not None:
        assert np.array_equal(a[2], b[2]), "residuals"
    np.testing.assert_allclose(a[0], b[0], rtol=1e-6)
    assert a[0][3] == b[0][3]


def both_forms(gpu, d, **kw):
    new = launch(gpu, d, 1, **kw)
    if new[3] != FORM_CUWIDE:
        pytest.skip(f"the launcher took form {new[3]}, not the 16-wave form, for {d['logits'].shape}")
    old = launch(gpu, d, 0, **kw)
    assert old[3] != FORM_CUWIDE
    check_same_bits(new, old)
    return new


# C = 100: K = 7, the last slot is partial (vectors 24 .. 27 alias vector 24); C = 96: K = 6, no partial slot;
# C = 84 and C = 68: K = 6 and 5 with a partial last 1-KiB piece (336 and 272 chunks), where the clamp of the last
# piece's offset decides what is read and the bound of the last store what is written.
# C = 40: three vectors per lane in the K = 4 instantiation, the only reachable one that is not EXACT -- every piece is
# clamped and every store goes through the bounds branch; C = 64: K = 4 exact; C = 128: K = 8, eight full pieces.
@pytest.mark.parametrize("C,shape", [(100, "full"), (96, "full"), (84, "full"), (68, "full"), (40, "full"), (64, "full"),
                                     (128, "full"), (100, "trailing"), (84, "trailing"), (40, "trailing"),
                                     (100, "partial_workgroup"), (84, "partial_workgroup"), (40, "partial_workgroup")])
def test_entry_shapes_vs_oracle_and_four_wave_form(gpu, oracle, C, shape):
    """Full launch; B mod 16 = 5 trailing rows (the register-row kernel adds them to record 0); a tile count that is
    no multiple of 16 (the last workgroup has waves without a tile that only join the barrier).  Permuted idx."""
    torch, ops, dev = gpu
    B = rows_for(torch, partial_workgroup=shape == "partial_workgroup", trailing=5 if shape == "trailing" else 0)
    d = synth.mstep_inputs(B, C, N=B + 37, seed=1200 + C)
    out, grad, res, _ = both_forms(gpu, d)
    check_oracle(oracle, d, out, grad, res)
    assert ops.workspace(dev).status() == 0


def test_entry_without_idx_is_the_evaluation_form(gpu, oracle):
    """idx = None: the index load reads the labels (idxp = labels) and ix = row_base + sub."""
    torch, ops, dev = gpu
    B, C = rows_for(torch), 100
    d = synth.mstep_inputs(B, C, N=B, seed=1301)
    out, grad, res, _ = both_forms(gpu, d, idx=False)
    check_oracle(oracle, d, out, grad, res, idx=False)


def test_entry_in_order_idx(gpu, oracle):
    torch, ops, dev = gpu
    B, C = rows_for(torch), 100
    d = synth.mstep_inputs(B, C, N=B, seed=1302)
    d["idx"] = np.arange(B, dtype=np.int64)
    out, grad, res, _ = both_forms(gpu, d)
    check_oracle(oracle, d, out, grad, res)


def test_entry_without_residuals(gpu, oracle):
    torch, ops, dev = gpu
    B, C = rows_for(torch), 100
    d = synth.mstep_inputs(B, C, N=B + 3, seed=1303)
    out, grad, res, _ = both_forms(gpu, d, residuals=False)
    assert res is None
    check_oracle(oracle, d, out, grad, None)


def test_no_gradient_launch_keeps_four_wave_form(gpu, oracle):
    """grad = None.  The launcher's rule for the 16-wave form asks for a gradient (its barrier orders stores behind
    loads: without stores there is nothing to order), so this launch takes the four-wave tiles under either knob; the
    case pins that down and checks the scalars and residuals of a launch of this size."""
    torch, ops, dev = gpu
    B, C = rows_for(torch), 100
    d = synth.mstep_inputs(B, C, N=B + 3, seed=1304)
    new = launch(gpu, d, 1, want_grad=False)
    old = launch(gpu, d, 0, want_grad=False)
    assert new[3] == old[3] == 2 and new[1] is None
    check_same_bits(new, old)
    check_oracle(oracle, d, new[0], None, new[2])


def test_entry_out_of_range_label_and_index(gpu, oracle):
    """One label and one index out of range: RLVI_ST_RANGE is raised, those rows get a zero gradient, scatter no
    residual and count for nothing; every other row is what it is without them."""
    torch, ops, dev = gpu
    from rlvi_amd import _lib
    B, C = rows_for(torch), 100
    N = B + 11
    d = synth.mstep_inputs(B, C, N=N, seed=1305)
    bad_label, bad_index = 16 * 7 + 3, B - 16 * 5 - 9          # (two different tiles, neither lane 0 of its row group)
    clean_idx = d["idx"].copy()
    d["labels"][bad_label] = C
    d["idx"][bad_index] = N
    d["residuals"][:] = -1.0
    ws = ops.workspace(dev)
    try:
        new = launch(gpu, d, 1)
        st_new = ws.status()
        ws.clear_status()
        if new[3] != FORM_CUWIDE:
            pytest.skip(f"the launcher took form {new[3]}, not the 16-wave form")
        old = launch(gpu, d, 0)
        st_old = ws.status()
    finally:
        ws.clear_status()
    assert st_new == st_old and st_new & _lib.ST_RANGE
    check_same_bits(new, old)
    out, grad, res, _ = new
    bad = np.array([bad_label, bad_index])
    assert not grad[bad].any()
    assert res[clean_idx[bad_label]] == -1.0 and res[clean_idx[bad_index]] == -1.0
    good = np.setdiff1d(np.arange(B), bad)
    r0 = np.full(N, -1.0, np.float32)
    ref = oracle.mstep(d["logits"][good], d["labels"][good], d["idx"][good], d["weights"], r0, scale_div=B)
    assert abs(float(out[0]) - float(ref["loss"])) <= REL * abs(float(ref["loss"]))
    assert float(out[3]) == float(round(float(ref["prec1"]) * len(good) / 100.0))
    np.testing.assert_allclose(res, r0, rtol=REL, atol=1e-6)
    diff = grad[good].astype(np.float64) - ref["grad"]
    assert np.sqrt((diff ** 2).sum()) <= REL * np.sqrt((ref["grad"].astype(np.float64) ** 2).sum())
    assert np.abs(diff).max() <= 1e-6


def test_entry_accumulate_two_launches_then_reduce(gpu, oracle):
    """accumulate=True: two launches of the form pile their records up, mstep_reduce collects both."""
    torch, ops, dev = gpu
    from rlvi_amd import _lib
    L = _lib.load()
    B, C = rows_for(torch, trailing=5), 100
    N = 2 * B
    d = synth.mstep_inputs(2 * B, C, N=N, seed=1306)
    halves = [{k: (v[h * B:(h + 1) * B] if k in ("logits", "labels", "idx") else v) for k, v in d.items()}
              for h in range(2)]
    w = torch.from_numpy(d["weights"]).to(dev)
    got = {}
    for cuwide in (1, 0):
        ws = ops.Workspace(dev, N, B)
        res = torch.zeros(N, device=dev)
        grads, forms = [], []
        _lib.check(L.rlvi_tune_set(b"RLVI_MSTEP_CUWIDE", cuwide), "tune")
        try:
            for h in halves:
                _, g = ops.mstep_fwd_bwd(torch.from_numpy(h["logits"]).to(dev), torch.from_numpy(h["labels"]).to(dev),
                                         torch.from_numpy(h["idx"]).to(dev), w, res, ws=ws, accumulate=True)
                forms.append(last_form(ops, dev, ws))
                grads.append(g)
            out = ops.mstep_reduce(ws=ws)
            torch.cuda.synchronize()
        finally:
            L.rlvi_tune_unset(b"RLVI_MSTEP_CUWIDE")
        assert ws.status() == 0
        got[cuwide] = (out.cpu().numpy(), np.concatenate([g.cpu().numpy() for g in grads]), res.cpu().numpy(), forms)
    if got[1][3] != [FORM_CUWIDE, FORM_CUWIDE]:
        pytest.skip(f"the launcher took forms {got[1][3]}, not the 16-wave form")
    assert FORM_CUWIDE not in got[0][3]
    check_same_bits(got[1], got[0])
    out, grad, res, _ = got[1]
    r0 = np.zeros(N, np.float32)
    refs = [oracle.mstep(h["logits"], h["labels"], h["idx"], d["weights"], r0) for h in halves]
    loss = float(refs[0]["loss"]) + float(refs[1]["loss"])
    assert abs(float(out[0]) - loss) <= REL * loss
    assert float(out[3]) == float(sum(round(float(r["prec1"]) * B / 100.0) for r in refs))
    np.testing.assert_allclose(res, r0, rtol=REL, atol=1e-6)
    diff = grad.astype(np.float64) - np.concatenate([r["grad"] for r in refs])
    assert np.sqrt((diff ** 2).sum()) <= REL * np.sqrt((np.concatenate([r["grad"] for r in refs]).astype(np.float64) ** 2).sum())
    assert np.abs(diff).max() <= 1e-6
