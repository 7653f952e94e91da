"""JoCoR (deep-learning/methods/train_jocor.py) without a GPU: the mirror's interface against the reference's, golden
set G12 against a float64 restatement of the formulas, which G12 cases pin their selection, the C entries' host-side
argument checks and the fixture's size.

The restatement (`restate`) is the loss as the reference runs it: the KL terms are BATCH MEANS (kl_loss_compute's
`if reduce:` with reduce='none'), so loss_pick_i = (1-l) CE1_i + (1-l) CE2_i + l K_qp + l K_pq, L = the mean of the
k smallest, and every row receives the KL gradient.  The GPU tests (test_jocor_gpu.py) import it.
"""
import ctypes
import inspect
import os

import numpy as np
import pytest

from rlvi_amd import ops, synth
from rlvi_amd.methods import train_jocor  # noqa: F401  (the mirror these tests pin)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G12 = os.path.join(ROOT, "tests", "golden", "g12_jocor.npz")
PIN_ULPS = 16          # a selection is pinned when its gap clears this many fp32 ulp of the values at the boundary


def restate(z1, z2, y, k, lam):
    """float64 loss_jocor and its gradients: (L, K_qp, K_pq, loss_pick, sel, grad1, grad2).  Equal loss_pick are
    taken in index order (a stable sort)."""
    z1 = np.asarray(z1, np.float64)
    z2 = np.asarray(z2, np.float64)
    B, C = z1.shape

    def logsoftmax(z):
        m = z.max(1, keepdims=True)
        return z - m - np.log(np.exp(z - m).sum(1, keepdims=True))
    lp, lq = logsoftmax(z1), logsoftmax(z2)
    p, q = np.exp(lp), np.exp(lq)
    rows = np.arange(B)
    ce1, ce2 = -lp[rows, y], -lq[rows, y]
    kl_pq = (p * (lp - lq)).sum(1)            # KL(p || q) per row
    kl_qp = (q * (lq - lp)).sum(1)
    K_qp, K_pq = kl_qp.mean(), kl_pq.mean()   # kl_loss_compute(y_1, y_2), kl_loss_compute(y_2, y_1)
    pick = (1 - lam) * ce1 + (1 - lam) * ce2 + lam * K_qp + lam * K_pq
    S = np.argsort(pick, kind="stable")[:k]
    sel = np.zeros(B, bool)
    sel[S] = True
    if k == 0:
        return np.nan, K_qp, K_pq, pick, sel, np.zeros_like(z1), np.zeros_like(z2)
    L = pick[S].mean()
    hot = np.zeros_like(z1)
    hot[rows, y] = 1.0
    s = sel[:, None] * (1 - lam) / k
    g1 = s * (p - hot) + lam / B * ((p - q) + p * (lp - lq - kl_pq[:, None]))
    g2 = s * (q - hot) + lam / B * ((q - p) + q * (lq - lp - kl_qp[:, None]))
    return L, K_qp, K_pq, pick, sel, g1, g2


def golden():
    return np.load(G12)


def case_inputs(g, key):
    """(z1, z2, labels, k, forget_rate, co_lambda, dtype) of a G12 case: the recipe, rounded to the case's dtype and
    widened back (what the reference was fed)."""
    import torch
    B, C, seed = (int(v) for v in g[key + "/shape"])
    fr, lam = (float(v) for v in g[key + "/real"])
    assert ops.jocor_num_remember(fr, B) == int(g[key + "/k"])          # the mirror's k is the reference's
    dt = key.split("_")[0]
    d1 = synth.mstep_inputs(B, C, N=B, seed=seed, zero_frac=0.0)
    d2 = synth.mstep_inputs(B, C, N=B, seed=seed + 1, zero_frac=0.0)
    z1, z2 = d1["logits"], d2["logits"]
    if dt != "f32":
        tdt = torch.bfloat16 if dt == "bf16" else torch.float16
        z1 = torch.from_numpy(z1).to(tdt).float().numpy()
        z2 = torch.from_numpy(z2).to(tdt).float().numpy()
    return z1, z2, d1["labels"], int(g[key + "/k"]), fr, lam, dt


def pinned(g, key):
    """True when the case's selection is defined beyond rounding: 0 < k < B and the gap between the k-th and the
    (k+1)-th smallest loss_pick clears PIN_ULPS fp32 ulp of the values there."""
    B = int(g[key + "/shape"][0])
    k = int(g[key + "/k"])
    if not 0 < k < B:
        return False
    edge = g[key + "/edge"].astype(np.float32)
    return float(g[key + "/gap"]) > PIN_ULPS * float(np.spacing(np.abs(edge).max()))


def selection(g, key):
    B = int(g[key + "/shape"][0])
    return np.unpackbits(g[key + "/sel_bits"])[:B].astype(bool)


def test_names_argument_order_and_all_match_the_reference():
    import importlib
    g = golden()
    jc = importlib.import_module("rlvi_amd.methods.train_jocor")
    assert list(jc.__all__) == list(g["ref/all"])
    for fn in ("kl_loss_compute", "loss_jocor", "train_jocor"):
        ps = inspect.signature(getattr(jc, fn)).parameters.values()
        mine = [q.name if q.default is q.empty else f"{q.name}={q.default!r}" for q in ps]
        assert mine == list(g["ref/sig/" + fn]), fn
    import rlvi_amd.methods as methods
    assert methods.train_jocor is jc.train_jocor


def test_restatement_reproduces_the_reference():
    g = golden()
    for key in g["cases"]:
        z1, z2, y, k, fr, lam, dt = case_inputs(g, key)
        L, kqp, kpq, pick, sel, g1, g2 = restate(z1, z2, y, k, lam)
        ref_L = float(g[key + "/loss"])
        if k == 0:
            assert np.isnan(ref_L) and np.isnan(L)
        else:
            assert abs(L - ref_L) <= 1e-5 * abs(ref_L), key
        np.testing.assert_allclose([kqp, kpq], g[key + "/kl"], rtol=1e-5, err_msg=key)
        rows = g[key + "/rows"]
        np.testing.assert_allclose(pick[rows], g[key + "/loss_pick"], rtol=1e-5, err_msg=key)
        for mine, ref in ((g1, g[key + "/grad1"]), (g2, g[key + "/grad2"])):
            atol = 1e-5 * max(np.abs(ref).max(), 1e-30)
            np.testing.assert_allclose(mine[rows], ref, rtol=1e-4, atol=atol, err_msg=key)
        assert int(selection(g, key).sum()) == k
        if pinned(g, key):
            assert np.array_equal(sel, selection(g, key)), key


def test_pinned_gaps_clear_their_rounding_and_every_shape_has_pinned_cases():
    g = golden()
    by_shape = {}
    for key in g["cases"]:
        z1, z2, y, k, fr, lam, dt = case_inputs(g, key)
        B = z1.shape[0]
        if not 0 < k < B:
            continue
        _, _, _, pick, _, _, _ = restate(z1, z2, y, k, lam)
        s = np.sort(pick)
        edge = g[key + "/edge"].astype(np.float64)
        # the reference's boundary values and the restatement's agree to fp32 rounding (a few ulp)
        ulp = float(np.spacing(np.float32(np.abs(edge).max())))
        assert abs(s[k - 1] - edge[0]) <= 4 * ulp and abs(s[k] - edge[1]) <= 4 * ulp, key
        assert abs(float(g[key + "/gap"]) - (edge[1] - edge[0])) <= 1e-12, key
        if pinned(g, key):
            # the gap is larger than the rounding of both sides together, in the reference and in float64
            assert s[k] - s[k - 1] > (PIN_ULPS - 8) * ulp, key
        by_shape.setdefault(tuple(g[key + "/shape"][:2]), []).append(pinned(g, key))
    assert len(by_shape) == 6
    for shape, flags in by_shape.items():
        assert any(flags), f"no pinned case at {shape}"


def test_the_fixture_tells_the_batch_mean_kl_from_a_per_row_kl():
    """JoCoR as its paper writes it (KL per row inside loss_pick) selects other rows than the reference does on some
    pinned case: a kernel that did so fails the GPU selection test."""
    g = golden()
    differs = 0
    for key in g["cases"]:
        if not pinned(g, key):
            continue
        z1, z2, y, k, fr, lam, dt = case_inputs(g, key)
        _, _, _, pick, sel, _, _ = restate(z1, z2, y, k, lam)
        zz1, zz2 = z1.astype(np.float64), z2.astype(np.float64)
        lp = zz1 - np.log(np.exp(zz1 - zz1.max(1, keepdims=True)).sum(1, keepdims=True)) - zz1.max(1, keepdims=True)
        lq = zz2 - np.log(np.exp(zz2 - zz2.max(1, keepdims=True)).sum(1, keepdims=True)) - zz2.max(1, keepdims=True)
        per_row = (np.exp(lq) * (lq - lp)).sum(1) + (np.exp(lp) * (lp - lq)).sum(1)
        paper = pick - lam * (per_row.mean()) + lam * per_row
        paper_sel = np.zeros_like(sel)
        paper_sel[np.argsort(paper, kind="stable")[:k]] = True
        differs += int(not np.array_equal(paper_sel, selection(g, key)))
    assert differs > 0


def test_the_fixture_tells_kl_gradient_on_every_row_from_selected_rows_only():
    """Every stored row that the reference did not keep still has a gradient (the batch-mean KL's); a kernel that
    gave the KL gradient to the kept rows only would write zeros there and fail the GPU gradient test."""
    g = golden()
    seen = 0
    for key in g["cases"]:
        k = int(g[key + "/k"])
        if k == 0:
            assert not np.any(g[key + "/grad1"]) and not np.any(g[key + "/grad2"])
            continue
        dropped = ~selection(g, key)[g[key + "/rows"]]
        if dropped.any():
            for gr in (g[key + "/grad1"], g[key + "/grad2"]):
                assert np.all(np.abs(gr[dropped]).max(1) > 0), key
                # ... and it is not small against the bar of the GPU test
                assert np.abs(gr[dropped]).max() > 1e-3 * np.abs(gr).max(), key
            seen += 1
    assert seen >= 10


def test_fixture_size_and_contents():
    assert os.path.getsize(G12) < 600 * 1024
    g = golden()
    keys = list(g["cases"])
    assert len(keys) == 75
    for dt in ("f32", "bf16", "f16"):
        assert sum(k.startswith(dt + "_") for k in keys) == 25
    lams = {float(g[k + "/real"][1]) for k in keys}
    assert lams == {0.1, 0.35}
    assert g["loop/params"].shape[0] == 3 and g["loop/train_acc"].shape == (3,)


@pytest.fixture(scope="module")
def lib():
    from rlvi_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_jocor_entries_and_argument_errors_without_a_gpu(lib):
    from rlvi_amd import _lib
    for dt in ("f32", "bf16", "f16"):
        for d in ("fwd", "bwd"):
            assert f"rlvi_jocor_{d}_{dt}" in _lib.SIGNATURES and hasattr(lib, f"rlvi_jocor_{d}_{dt}")
    assert lib.rlvi_abi_version() == 3
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 255) & ~255
    for fwd in (lib.rlvi_jocor_fwd_f32, lib.rlvi_jocor_fwd_bf16, lib.rlvi_jocor_fwd_f16):
        #   z1 ld1 z2 ld2 labels B C k lam loss_pick sel out ws stream
        assert fwd(None, 10, p, 10, p, 8, 10, 4, 0.1, p, p, p, p, None) == -1
        assert fwd(p, 10, p, 10, p, 8, 10, 4, 0.1, p, p, p, None, None) == -1          # no workspace
        assert fwd(p, 4, p, 10, p, 8, 10, 4, 0.1, p, p, p, p, None) == -2             # ld1 < C
        assert fwd(p, 10, p, 10, p, 0, 10, 4, 0.1, p, p, p, p, None) == -2            # B = 0
        assert fwd(p, 10, p, 10, p, 8, 10, -1, 0.1, p, p, p, p, None) == -2           # k < 0
        assert fwd(p, 10, p, 10, p, 8, (1 << 20) + 1, 4, 0.1, p, p, p, p, None) == -2  # ld < C
        assert fwd(p, 10, p, 10, p + 4, 8, 10, 4, 0.1, p, p, p, p, None) == -3        # labels not 8-byte aligned
        assert fwd(p, 10, p, 10, p, 8, 10, 4, 0.1, p, p, p, p + 64, None) == -3       # workspace not 256-aligned
    for bwd in (lib.rlvi_jocor_bwd_f32, lib.rlvi_jocor_bwd_bf16, lib.rlvi_jocor_bwd_f16):
        #   z1 ld1 z2 ld2 labels sel B C k lam grad_out grad_scale g1 ldg1 g2 ldg2 stream
        assert bwd(p, 10, p, 10, p, None, 8, 10, 4, 0.1, p, None, p, 10, p, 10, None) == -1
        assert bwd(p, 10, p, 10, p, p, 8, 10, 4, 0.1, p, None, p, 4, p, 10, None) == -2     # ldg1 < C
        assert bwd(p, 10, p, 10, p, p, 8, 10, 4, 0.1, p + 2, None, p, 10, p, 10, None) == -3  # grad_out alignment
        assert bwd(p, 10, p, 10, p, p, 8, 10, 4, 0.1, p, None, None, 10, None, 10, None) == 0  # nothing wanted
    assert lib.rlvi_jocor_fwd_f32(p, 1 << 21, p, 1 << 21, p, 8, (1 << 20) + 1, 4, 0.1, p, p, p, p, None) == -5


def test_num_remember_is_the_reference_slice():
    for B in (37, 64, 1000):
        for fr in (0.0, 0.2, 0.45, 0.9, 1.0, np.float64(0.3)):
            k = int((1 - fr) * B)
            assert ops.jocor_num_remember(fr, B) == len(range(B)[:k])
    assert ops.jocor_num_remember(1.5, 10) == len(range(10)[:int((1 - 1.5) * 10)])
