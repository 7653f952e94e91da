"""BARE (deep-learning/methods/train_bare.py) and the plain loop (train_regular.py) without a GPU: the mirrors'
interfaces against the reference's, golden set G14 against a float64 restatement of the formulas, what the fixture
pins and what it tells apart, the C entries' host-side argument checks and the fixture's size.

The restatement (`restate`) is WeightedCCE.forward as the reference runs it: p = clamp(softmax(z), 1e-8, 1 - 1e-8),
row i kept when p[i, y_i] - mu[y_i] >= k * sd[y_i] with the batch mean and the UNBIASED batch deviation of every
column, L = the mean cross-entropy of the kept rows, or of all rows when none is kept; no gradient through the
statistics.  A row is pinned when |margin| > PIN = 2^-18 (tools/make_golden_bare.py); a NaN margin (B = 1) is pinned
too: the comparison is false whatever the rounding.  The GPU tests (test_bare_gpu.py) import all of this.
"""
import ctypes
import functools
import inspect
import os

import numpy as np
import pytest

from rlvi_amd import synth
from rlvi_amd.methods import train_bare, train_regular  # noqa: F401  (the mirrors these tests pin)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G14 = os.path.join(ROOT, "tests", "golden", "g14_bare.npz")
PIN = 2.0 ** -18
SHAPES = 13            # distinct (B, C) of the fixture's cases


def softmax64(z):
    z = np.asarray(z, np.float64)
    m = z.max(1, keepdims=True)
    lse = m + np.log(np.exp(z - m).sum(1, keepdims=True))
    return np.exp(z - lse), z - lse


def margins(z, y, k, biased=False, pt_of=None):
    """pt - mu[y] - k * sd[y] in float64.  biased: divide by B, not B - 1.  pt_of(p, logp) -> pt replaces p[i, y_i]."""
    p, logp = softmax64(z)
    B = p.shape[0]
    rows = np.arange(B)
    pc = np.clip(p, 1e-8, 1 - 1e-8)
    mu = pc.mean(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = np.sqrt(((pc - mu) ** 2).sum(0) / (B if biased else B - 1))
    pt = pc[rows, y] if pt_of is None else pt_of(p, logp)[rows, y]
    return pt - mu[y] - k * sd[y]


def loss_and_grad(z, y, sel):
    """float64 L and dL/dz for a given selection (all ones: the fallback)."""
    p, logp = softmax64(z)
    B = p.shape[0]
    rows = np.arange(B)
    n = int(sel.sum())
    hot = np.zeros_like(p)
    hot[rows, y] = 1.0
    L = float(-logp[rows, y][sel].mean())
    return L, sel[:, None] * (p - hot) / n


def restate(z, y, k):
    """float64 WeightedCCE.forward and its gradient: (L, margin, sel, grad, fallback)."""
    m = margins(z, y, k)
    with np.errstate(invalid="ignore"):
        sel = m >= 0
    fallback = not sel.any()
    if fallback:
        sel = np.ones(len(y), bool)
    L, grad = loss_and_grad(z, y, sel)
    return L, m, sel, grad, fallback


def pinned_rows(margin):
    with np.errstate(invalid="ignore"):
        return ~(np.abs(margin) <= PIN)


@functools.lru_cache(maxsize=1)
def golden():
    return dict(np.load(G14))


def rounded(z, dt):
    import torch
    if dt == "f32":
        return z
    tdt = torch.bfloat16 if dt == "bf16" else torch.float16
    return torch.from_numpy(z).to(tdt).float().numpy()


@functools.lru_cache(maxsize=None)
def case_inputs(key):
    """(z, labels, k, dtype) of a G14 case: the recipe, rounded to the case's dtype and widened back (what the
    reference was fed)."""
    g = golden()
    B, C, seed = (int(v) for v in g[key + "/shape"])
    k, scale = (float(v) for v in g[key + "/real"])
    kind = str(g[key + "/kind"])
    dt = key.split("_")[0]
    if kind == "bimodal":
        d = synth.mstep_inputs(B, C, N=B, seed=seed, zero_frac=0.0)
        z, y = d["logits"], d["labels"]
    else:
        z, y = synth.bare_dense_inputs(B, C, scale, seed)
    if kind == "adversarial":
        y = g[key + "/labels"].astype(np.int64)
    return rounded(z, dt), y, k, dt


def selection(g, key):
    B = int(g[key + "/shape"][0])
    return np.unpackbits(g[key + "/sel_bits"])[:B].astype(bool)


def pinned(g, key):
    return pinned_rows(g[key + "/margin"].astype(np.float64))


def full(g, key):
    return bool(g[key + "/full"])


def test_names_argument_order_and_all_match_the_reference():
    import importlib
    g = golden()
    tb = importlib.import_module("rlvi_amd.methods.train_bare")
    tr = importlib.import_module("rlvi_amd.methods.train_regular")
    assert list(tb.__all__) == list(g["ref/all"]) == ["train_bare"]
    assert list(tr.__all__) == list(g["ref/all_regular"]) == ["train_regular"]

    def sig(fn):
        ps = inspect.signature(fn).parameters.values()
        return [q.name if q.default is q.empty else f"{q.name}={q.default!r}" for q in ps]
    assert sig(tb.WeightedCCE.__init__) == list(g["ref/sig/WeightedCCE.__init__"])
    assert sig(tb.WeightedCCE.forward) == list(g["ref/sig/WeightedCCE.forward"])
    assert sig(tb.train_bare) == list(g["ref/sig/train_bare"])
    assert sig(tr.train_regular) == list(g["ref/sig/train_regular"])
    import torch
    assert issubclass(tb.WeightedCCE, torch.nn.Module)
    import rlvi_amd.methods as methods
    assert methods.train_bare is tb.train_bare and methods.train_regular is tr.train_regular
    # with these two the package offers every train_* plug-in of the reference
    ns = {}
    exec("from rlvi_amd.methods import *", ns)
    assert set(g["ref/methods"]) <= set(ns)
    assert len(g["ref/methods"]) == 7


def test_reductions_and_one_hot_the_mirror_does_not_provide():
    import torch
    from rlvi_amd.methods.train_bare import WeightedCCE
    z, y = torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(NotImplementedError):
        WeightedCCE(reduction="sum")(z, y)
    with pytest.raises(NotImplementedError):
        WeightedCCE()(z, y, one_hot=False)
    m = WeightedCCE(k=2, num_class=7, reduction="none")
    assert (m.k, m.num_class, m.reduction) == (2, 7, "none")


def test_restatement_reproduces_the_reference():
    g = golden()
    n_full = 0
    for key in g["cases"]:
        z, y, k, dt = case_inputs(key)
        L, m, sel, grad, fallback = restate(z, y, k)
        # the stored margins are these (fp32 storage of an fp64 value)
        np.testing.assert_allclose(m, g[key + "/margin"].astype(np.float64), rtol=1e-6, atol=1e-7, err_msg=key)
        pin = pinned(g, key)
        assert np.array_equal(sel[pin], selection(g, key)[pin]), key
        assert fallback == bool(g[key + "/fallback"]), key
        assert abs(int(sel.sum()) - int(g[key + "/n_kept"])) <= int(g[key + "/unpinned"]), key
        if not full(g, key):
            continue
        n_full += 1
        assert int(sel.sum()) == int(g[key + "/n_kept"]), key
        ref_L = float(g[key + "/loss"])
        assert abs(L - ref_L) <= 1e-5 * abs(ref_L), key
        ref = g[key + "/grad"]
        np.testing.assert_allclose(grad[g[key + "/rows"]], ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max(), err_msg=key)
    assert n_full >= 60


def test_every_case_is_within_the_cap_and_every_shape_has_a_fully_pinned_case():
    g = golden()
    by_shape = {}
    for key in g["cases"]:
        B = int(g[key + "/shape"][0])
        unp = int((~pinned(g, key)).sum())
        assert unp == int(g[key + "/unpinned"]) and unp <= 0.01 * B, key
        assert full(g, key) == (unp == 0), key
        by_shape.setdefault(tuple(int(v) for v in g[key + "/shape"][:2]), []).append(full(g, key))
    assert len(by_shape) == SHAPES
    for shape, flags in by_shape.items():
        assert any(flags), f"no fully pinned case at {shape}"
    assert float(g["pin"]) == PIN


def flips_on_pinned_rows(g, key, other_margin):
    """Rows of a case that are pinned under the reference's rule AND under the variant's, and which the variant judges
    the other way."""
    pin = pinned(g, key) & pinned_rows(other_margin)
    with np.errstate(invalid="ignore"):
        return int(((other_margin >= 0) != selection(g, key))[pin].sum())


def test_the_fixture_tells_the_unbiased_deviation_from_the_biased_one():
    """Dividing by B instead of B - 1 changes the selection on pinned rows of every case built for it (B = 3, 4, 5, 16,
    where the two differ by 22 to 3 %), in all three dtypes: a kernel that did so fails the GPU selection test."""
    g = golden()
    seen = 0
    for key in g["cases"]:
        if str(g[key + "/kind"]) != "unbiased":
            continue
        z, y, k, dt = case_inputs(key)
        assert not bool(g[key + "/fallback"]) and full(g, key)
        assert flips_on_pinned_rows(g, key, margins(z, y, k, biased=True)) > 0, key
        seen += 1
    assert seen == 12


def test_the_fixture_tells_k_one_from_k_half():
    g = golden()
    for dt in ("f32", "bf16", "f16"):
        # a k = 1 case judged with k = 0.5, and the k = 0.5 case judged with k = 1
        for key, other_k in ((f"{dt}_dense_B200_C100", 0.5), (f"{dt}_khalf_B200_C100_k0.5", 1.0)):
            z, y, k, _ = case_inputs(key)
            assert k != other_k
            assert flips_on_pinned_rows(g, key, margins(z, y, other_k)) > 0, key


def test_the_fixture_tells_the_probability_from_the_log_probability():
    """pt is the clamped softmax entry of the label; a kernel that took the (unclamped) log-probability -- the
    cross-entropy it has at hand -- selects other rows on pinned cases."""
    g = golden()
    differs = 0
    for key in g["cases"]:
        if bool(g[key + "/fallback"]):
            continue
        z, y, k, dt = case_inputs(key)
        differs += int(flips_on_pinned_rows(g, key, margins(z, y, k, pt_of=lambda p, logp: logp)) > 0)
    assert differs >= 30


def test_the_fixture_tells_dropped_rows_and_the_fallback():
    """The stored gradient of a dropped row is exactly zero (no gradient leaks through the statistics); in a fallback
    case every row has one."""
    g = golden()
    dropped_seen = fallback_seen = 0
    for key in g["cases"]:
        rows = g[key + "/rows"]
        grad = g[key + "/grad"]
        if bool(g[key + "/fallback"]):
            assert np.all(np.abs(grad).max(1) > 0), key
            assert selection(g, key).all() and int(g[key + "/n_kept"]) == int(g[key + "/shape"][0])
            fallback_seen += 1
            continue
        drop = ~selection(g, key)[rows]
        assert not np.any(grad[drop]), key
        assert np.all(np.abs(grad[~drop]).max(1) > 0), key
        dropped_seen += int(drop.any())
    assert fallback_seen == 12 and dropped_seen >= 40
    # the adversarial fallbacks are pinned as a whole: no row comes near being kept
    for key in g["cases"]:
        if str(g[key + "/kind"]) == "adversarial":
            assert float(g[key + "/margin"].max()) < -0.2, key


def test_fixture_size_and_contents():
    assert os.path.getsize(G14) < 600 * 1024
    g = golden()
    keys = list(g["cases"])
    assert len(keys) == 69
    for dt in ("f32", "bf16", "f16"):
        assert sum(k.startswith(dt + "_") for k in keys) == 23
    for name in ("bare", "regular"):
        assert g[f"loop/{name}_params"].shape == (3, 170) and g[f"loop/{name}_acc"].shape == (3,)
        assert g[f"loop/{name}_init"].shape == (170,)


@pytest.fixture(scope="module")
def lib():
    from rlvi_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_bare_entries_and_argument_errors_without_a_gpu(lib):
    from rlvi_amd import _lib
    for dt in ("f32", "bf16", "f16"):
        assert f"rlvi_bare_fwd_{dt}" in _lib.SIGNATURES and hasattr(lib, f"rlvi_bare_fwd_{dt}")
    assert "rlvi_bare_form" in _lib.SIGNATURES and hasattr(lib, "rlvi_bare_form")
    assert lib.rlvi_abi_version() == 3
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 255) & ~255
    nan = float("nan")
    for fwd in (lib.rlvi_bare_fwd_f32, lib.rlvi_bare_fwd_bf16, lib.rlvi_bare_fwd_f16):
        #   logits ld labels B C k w sel out grad ldg ws stream
        assert fwd(None, 10, p, 8, 10, 1.0, p, p, p, None, 0, p, None) == -1
        assert fwd(p, 10, None, 8, 10, 1.0, p, p, p, None, 0, p, None) == -1
        assert fwd(p, 10, p, 8, 10, 1.0, p, None, p, None, 0, p, None) == -1
        assert fwd(p, 10, p, 8, 10, 1.0, p, p, p, None, 0, None, None) == -1           # no workspace
        assert fwd(p, 4, p, 8, 10, 1.0, p, p, p, None, 0, p, None) == -2               # ld < C
        assert fwd(p, 10, p, 0, 10, 1.0, p, p, p, None, 0, p, None) == -2              # B = 0
        assert fwd(p, 10, p, 8, 10, nan, p, p, p, None, 0, p, None) == -2              # k is NaN
        assert fwd(p, 10, p, 8, 10, 1.0, p, p, p, p, 4, p, None) == -2                 # ldg < C
        assert fwd(p, 10, p + 4, 8, 10, 1.0, p, p, p, None, 0, p, None) == -3          # labels not 8-byte aligned
        assert fwd(p, 10, p, 8, 10, 1.0, p, p, p, None, 0, p + 64, None) == -3         # workspace not 256-aligned
        assert fwd(p, 10, p, 8, 10, 1.0, p + 2, p, p, None, 0, p, None) == -3          # w not 4-byte aligned
        assert fwd(p, 4097, p, 8, 4097, 1.0, p, p, p, None, 0, p, None) == -5          # C > 4096
        assert fwd(p, 10, p, (1 << 22) + 1, 10, 1.0, p, p, p, None, 0, p, None) == -5  # B beyond the fixed point
    # which form a shape takes (host side): the reference's batches in one workgroup, the bench-sized one streaming
    for B, C in ((32, 10), (128, 10), (128, 100), (1, 10), (16, 1024), (1024, 16)):
        assert lib.rlvi_bare_form(B, C) == 1, (B, C)
    for B, C in ((65536, 100), (4096, 10), (1024, 101), (129, 128), (8, 4096), (1025, 10), (8, 1025)):
        assert lib.rlvi_bare_form(B, C) == 0, (B, C)
    assert lib.rlvi_bare_form(0, 10) == -2 and lib.rlvi_bare_form(8, 4097) == -5
    assert lib.rlvi_tune_set(b"RLVI_BARE_FORM", 0) == 0
    try:
        assert lib.rlvi_bare_form(128, 10) == 0
    finally:
        assert lib.rlvi_tune_unset(b"RLVI_BARE_FORM") == 1
    assert lib.rlvi_bare_form(128, 10) == 1


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    import torch
    from rlvi_amd import _lib, ops
    with pytest.raises(_lib.RlviError, match="no CPU fallback"):
        ops.bare_loss(torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(_lib.RlviError, match="no CPU fallback"):
        ops.bare_forward(torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64))
