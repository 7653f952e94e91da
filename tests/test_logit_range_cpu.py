"""The bars of test_logit_range_gpu, made legitimate before any kernel meets them (runs with -m "not gpu").

tests/logit_regimes.py builds logits far outside the synthetic range (offsets of 16 384 ... 49 152, rows times 40, +-60
on the label, masked columns, signed zeros and subnormals, +-65504 and +-3e38, and rows with -inf / +inf / NaN) and a
float64 reference of the row softmax.  Here two correct fp32 implementations that share no code with the kernels --
the C oracle (oracle.mstep / nll_rows / accuracy) and torch on the CPU (F.cross_entropy(reduction='none') and its
autograd gradient) -- are held to the project's own bars against that reference, per row and at gain 1:

  NLL       rtol 1e-5 (REL), atol 1e-6
  gradient  max|got - ref| <= 1e-6 * pi_i + REL * max|ref| + 2^-148   per row (the last term: the fp32 subnormal grid)
  top-1 count and precision@k ranks: equal;  inf / NaN: at identical positions

Measured here (70 x 10, 70 x 101, 35 x 1000, 21 x 2052; f32, bf16, f16; every regime), the worst error in units of the
bar, oracle / torch:  NLL 0.06 / 0.21,  gradient 0.12 / 0.22.  Both stay inside the unchanged bars on every regime, so no
regime has a bar of its own.  (The figures are printed by test_bars_hold_for_two_fp32_implementations with -s.)
"""
import numpy as np
import pytest

from logit_regimes import (DTYPES, FINITE, NONFINITE, REGIME_NAMES, REL, grad_failures, modest_rows, nll_failures,
                           reference, regime_inputs, same_nonfinite)

SHAPES = [(70, 10), (70, 101), (35, 1000), (21, 2052)]
ALL = FINITE + NONFINITE
_cache = {}


def inputs(B, C, dtype, regimes=ALL):
    key = (B, C, dtype, regimes)
    if key not in _cache:
        d = regime_inputs(B, C, dtype, seed=B + C, regimes=regimes, N=B + 17)
        _cache[key] = (d, reference(d["logits"], d["labels"], d["idx"], d["weights"]))
    return _cache[key]


def worst(got, ref, bar):
    """max of |got - ref| / bar over the finite reference entries."""
    f = np.isfinite(ref) & np.isfinite(got)
    return float(np.max(np.abs(got - ref)[f] / np.broadcast_to(bar, ref.shape)[f])) if f.any() else 0.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C", SHAPES)
def test_bars_hold_for_two_fp32_implementations(B, C, dtype, oracle):
    import torch
    d, ref = inputs(B, C, dtype)
    reg, pi = d["regime"], ref["pi"]
    pinned = reg != 10                               # (top-1 of a NaN row is unpinned)
    with np.errstate(all="ignore"):
        # ---- the C oracle
        r0 = d["residuals"].copy()
        o = oracle.mstep(d["logits"], d["labels"], d["idx"], d["weights"], r0, scale_div=1)
        rows, hit = oracle.nll_rows(d["logits"], d["labels"])
        assert np.array_equal(rows, o["loss_rows"], equal_nan=True) and np.array_equal(r0[d["idx"]], rows, equal_nan=True)
        assert not nll_failures(rows, ref["nll"], reg), nll_failures(rows, ref["nll"], reg)
        assert not grad_failures(o["grad"], ref["grad"], pi, reg), grad_failures(o["grad"], ref["grad"], pi, reg)
        assert np.array_equal(hit[pinned].astype(bool), ref["hit"][pinned])
        # the loss over all finite rows (the edge rows' terms are most of it) and over the rows of a modest NLL
        for fin in (np.isfinite(ref["nll"]), modest_rows(ref)):
            o_fin = oracle.mstep(d["logits"][fin], d["labels"][fin], d["idx"][fin], d["weights"],
                                 d["residuals"].copy(), scale_div=1)
            r_fin = float(np.sum(pi[fin] * ref["nll"][fin]))
            assert 0.0 < r_fin and abs(float(o_fin["loss"]) - r_fin) <= REL * abs(r_fin)
        assert r_fin < 1e3 * B                                # (no single row's term is the whole of it)
        assert same_nonfinite(np.float32(o["loss"]), np.float32(ref["loss"]))
        ks = sorted({1, min(5, C)})
        want = [100.0 * float((ref["rank"][pinned] < k).sum()) / int(pinned.sum()) for k in ks]
        assert oracle.accuracy(d["logits"][pinned], d["labels"][pinned], topk=ks) == want
        # ---- torch on the CPU, fp32
        z = torch.from_numpy(d["logits"]).requires_grad_(True)
        ce = torch.nn.functional.cross_entropy(z, torch.from_numpy(d["labels"]), reduction="none")
        (ce * torch.from_numpy(pi.astype(np.float32))).sum().backward()
        t_rows, t_grad = ce.detach().numpy(), z.grad.numpy()
        assert not nll_failures(t_rows, ref["nll"], reg), nll_failures(t_rows, ref["nll"], reg)
        assert not grad_failures(t_grad, ref["grad"], pi, reg), grad_failures(t_grad, ref["grad"], pi, reg)
        # ---- the figures of the module docstring
        nbar = 1e-6 + REL * np.abs(ref["nll"])
        gbar = (1e-6 * pi + REL * np.abs(np.where(np.isfinite(ref["grad"]), ref["grad"], 0.0)).max(axis=1))[:, None]
        print(f"\n{B}x{C} {dtype}: worst error / bar  NLL oracle {worst(rows, ref['nll'], nbar):.3f} torch "
              f"{worst(t_rows, ref['nll'], nbar):.3f}  gradient oracle {worst(o['grad'], ref['grad'], gbar):.3f} torch "
              f"{worst(t_grad, ref['grad'], gbar):.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C", SHAPES + [(257, 1), (257, 2), (64, 7)])
def test_generator_invariants(B, C, dtype):
    import torch
    d, ref = inputs(B, C, dtype, FINITE)
    reg, z, y = d["regime"], d["logits"], d["labels"]
    assert set(d) == {"logits", "labels", "idx", "weights", "residuals", "regime"}
    assert z.dtype == np.float32 and z.shape == (B, C) and reg.shape == (B,)
    for lo in range(0, B - 15):                                          # every 16-row window holds every regime
        assert set(reg[lo:lo + 16]) == set(FINITE)
    assert np.all(reg[1:] != reg[:-1])                                   # neighbouring rows never share one
    for i in np.nonzero(reg == 4)[0]:
        finite = np.isfinite(z[i])
        assert int(finite.sum()) == min(2 + i % 5, C) and finite[y[i]]
        assert np.all(np.isneginf(z[i][~finite]))
    # 2-byte inputs survive a round trip through their type bit for bit (-0.0, subnormals and -inf included)
    tt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    back = torch.from_numpy(z).to(tt).float().numpy()
    assert np.array_equal(back.view(np.uint32), z.view(np.uint32))
    # the float64 reference is finite on the finite regimes
    assert np.isfinite(ref["nll"]).all() and np.isfinite(ref["grad"]).all() and np.isfinite(ref["loss"])
    assert np.isfinite(np.float32(ref["loss"]))
    # the regimes are what they claim to be
    big = np.abs(np.where(np.isfinite(z), z, 0.0)).max(axis=1)
    assert np.all(big[reg == 1] >= 2.0 ** 14 - 64) and np.all(big[reg == 6] >= 65000.0)
    if dtype == "f32" and B >= 21:
        assert (big[reg == 6] > 1e38).any()
    assert np.all(big[reg == 5] <= 2.0 ** -14)
    if C >= 100:
        assert ref["nll"][reg == 2].max() > 100.0
    # the masked rows' starts walk: with enough of them, some lie in each half of the row
    if C >= 100:
        first = np.array([np.nonzero(np.isfinite(z[i]) & (np.arange(C) != y[i]))[0][0] for i in np.nonzero(reg == 4)[0]])
        assert first.min() < C // 2 <= first.max()


def test_nonfinite_kinds_are_what_the_reference_says():
    d, ref = inputs(70, 101, "f32")
    reg = d["regime"]
    a, b, c, n = (reg == k for k in NONFINITE)
    assert np.all(np.isposinf(ref["nll"][a])) and np.isfinite(ref["grad"][a]).all()
    assert np.isnan(ref["nll"][b | c | n]).all() and np.isnan(ref["grad"][b | c | n]).all()
    assert np.isfinite(ref["nll"][reg < 7]).all()
    # the all -inf row: every column attains the maximum, so the label is a hit only in column 0
    assert np.array_equal(ref["hit"][c], d["labels"][c] == 0)
    assert not ref["hit"][a].any() and not ref["hit"][b].any()
    assert [REGIME_NAMES[k] for k in NONFINITE] == ["label_ninf", "pinf", "all_ninf", "nan"]


# ------------------------------------------------------------------------------ the two mutations, restated
def _softmax_rows_f32(z, labels, G, mask_dead, combine_max):
    """The register-row softmax of mstep.hip restated in fp32 numpy for one lane group of G lanes holding K slots of
    one element each: slot k of lane g holds column k * G + g; a slot past the end of the row re-reads the lane's first
    element (column g) and is masked to -inf (mask_dead) before the maximum; the lanes' maxima are combined
    (combine_max) before the exponentials; the lanes' sums are always combined.  Returns the NLL per row."""
    B, C = z.shape
    K = (C + G - 1) // G
    out = np.empty(B, np.float32)
    with np.errstate(all="ignore"):
        for i in range(B):
            v = np.empty((G, K), np.float32)
            for g in range(G):
                for k in range(K):
                    col = k * G + g
                    live = col < C
                    v[g, k] = z[i, col] if live else (-np.inf if mask_dead else z[i, min(g, C - 1)])
            m_lane = v.max(axis=1)
            m = np.full(G, m_lane.max(), np.float32) if combine_max else m_lane
            s = np.float32(np.exp(v - m[:, None]).sum(dtype=np.float32))
            out[i] = np.log(s) - (z[i, labels[i]] - m[0])
    return out


@pytest.mark.parametrize("mutation", ["none", "no_mask", "own_max"])
def test_mutations_restated_on_the_cpu(mutation):
    """What two mutations of the register-row kernel do to a lane group's arithmetic: without the -inf mask a dead slot
    adds a second copy of a live column to the sum; with the lane's own maximum the lanes' exponentials are scaled
    differently.  Both miss the NLL bar by orders of magnitude on the regimes (and, restated like this, on plain rows
    as well: profiles/r10_logit_range.md); the unmutated restatement meets the bar on every regime."""
    d, ref = inputs(70, 10, "f32", FINITE)
    nll = _softmax_rows_f32(d["logits"], d["labels"], 4, mutation != "no_mask", mutation != "own_max")
    fails = nll_failures(nll, ref["nll"], d["regime"])
    if mutation == "none":
        assert not fails, fails
    else:
        caught = {f[0] for f in nll_failures(nll, ref["nll"], d["regime"])}
        assert caught & {"masked", "offset", "wide", "edge"}, caught
