"""The softmax kernels on logits beyond the synthetic range (run with -m gpu on an MI355X).

Every other GPU test draws its logits from synth.mstep_inputs: nothing beyond about 25, every row of a tile at the same
scale.  Softmax is shift-invariant, so a kernel may subtract a wrong maximum there and still agree to 1e-5.  Here every
row of a batch is in another regime (tests/logit_regimes.py: offsets of tens of thousands, rows times 40, +-60 on the
label, masked columns, signed zeros and subnormals, +-65504 / +-3e38, and -- where named -- rows with -inf, +inf or NaN),
and every M-step kernel body, the evaluation form, the in-batch E+M, precision@k and the small-loss selection are
compared with the float64 reference of the same module.

Bars (test_logit_range_cpu holds the C oracle and torch's CPU kernels to the same ones), per row, gain 1:
  NLL / residual   rtol 1e-5 (REL), atol 1e-6
  gradient, fp32   max|got - ref| <= 1e-6 * pi_i + REL * max|ref| + 2^-148 (two steps of the fp32 subnormal grid: what an fp32
                   gradient of 1e-46 -- a pi that the E-step drove to 1e-42 -- can be held to; logit_regimes.grad_failures)
  gradient, 2-byte |got - round(ref)| <= rtol * |round(ref)| + atol + the fp32 row bar above; rtol 2^-7 (bf16, as
                   test_mstep_bf16_golden) or 2^-10 (fp16: F16_RTOL), atol 0 or 2^-24 (F16_ATOL).  The stored value is
                   the rounding of an fp32 value that meets the fp32 bar: one storage ulp where a rounding boundary
                   is straddled, plus that fp32 error where the entry cancels (the label's p - 1).  The existing
                   tests' absolute terms (1e-7, 2^-24) stand for the same fp32 error at their gain of 1 / B.
  loss             REL relative;  hit count, ranks: equal;  inf / NaN: at identical positions
Every M-step call passes inv_scale = 1 (gradient entries O(pi) whatever B), a workspace of its own, and ends with
status 0.
"""
import numpy as np
import pytest

from logit_regimes import (FINITE, NONFINITE, REGIME_NAMES, REL, grad_failures, modest_rows, nll_failures, reference,
                           regime_inputs, same_nonfinite)
from test_fp16_gpu import F16_ATOL, F16_RTOL
from test_fp16_gpu import SHAPES as F16_SHAPES
from test_gpu_parity import DISPATCH_SHAPES, tune, untune
from test_gpu_parity import gpu, no_process_state_left_behind  # noqa: F401  (fixtures: the device, the hygiene check)
from test_oracle_golden import rel_pi

pytestmark = pytest.mark.gpu

LOWP = {"bf16": (2.0 ** -7, 0.0), "f16": (F16_RTOL, F16_ATOL)}
HOLD = 16                                   # the hold bit of rlvi_workspace_last_mstep_form


def tdtype(torch, dtype):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dtype]


def last_form(ws):
    from rlvi_amd import _lib
    return int(_lib.load().rlvi_workspace_last_mstep_form(ws.ptr))


def mstep(gpu, d, dtype, ws=None, want_grad=True, pitch=None):
    """ops.mstep_fwd_bwd at inv_scale = 1 on a workspace of its own: (out[4], gradient as fp32 or None, residuals,
    the kernel form taken), all on the host."""
    torch, ops, dev = gpu
    B, C = d["logits"].shape
    N = d["weights"].shape[0]
    z = torch.from_numpy(d["logits"]).to(dev).to(tdtype(torch, dtype))
    if pitch is not None:
        wide = torch.zeros((B, pitch), device=dev, dtype=z.dtype)
        wide[:, :C] = z
        z = wide[:, :C]
    ws = ws or ops.Workspace(dev, N, B)
    res = torch.from_numpy(d["residuals"].copy()).to(dev)
    out, grad = ops.mstep_fwd_bwd(z, torch.from_numpy(d["labels"]).to(dev), torch.from_numpy(d["idx"]).to(dev),
                                  torch.from_numpy(d["weights"]).to(dev), res, inv_scale=1.0, want_grad=want_grad,
                                  ws=ws)
    torch.cuda.synchronize()
    assert ws.status() == 0
    assert grad is None or grad.dtype == z.dtype
    return (out.cpu().numpy(), None if grad is None else grad.float().cpu().numpy(), res.cpu().numpy(),
            last_form(ws))


def rounded(torch, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(tdtype(torch, dtype)).float().numpy()


def lowp_grad_failures(torch, got, ref, pi, regime, dtype, gain=1.0):
    """The 2-byte gradient bar of the module docstring, per entry; (regime name, row, error, bar) of the rows missing it."""
    rtol, atol = LOWP[dtype]
    with np.errstate(all="ignore"):
        want = rounded(torch, ref, dtype).astype(np.float64)
        fin = np.isfinite(want)
        rowbar = gain * 1e-6 * np.asarray(pi, np.float64) + REL * np.abs(np.where(np.isfinite(ref), ref, 0.0)).max(axis=1)
        bar = rtol * np.abs(want) + atol + rowbar[:, None]
        err = np.abs(got.astype(np.float64) - want)
        bad = np.where(fin, ~(err <= bar), ~((np.isnan(got) & np.isnan(want)) | (got == want)))
    rows = np.nonzero(bad.any(axis=1))[0][:8]
    out = []
    for i in rows:
        j = int(np.argmax(bad[i]))
        out.append((REGIME_NAMES[int(regime[i])], int(i), float(err[i, j]), float(bar[i, j])))
    return out


def check_grad(torch, got, ref, d, dtype, what, gain=1.0):
    reg = d["regime"]
    if dtype == "f32":
        fails = grad_failures(got, ref["grad"], ref["pi"], reg, gain=gain)
    else:
        fails = lowp_grad_failures(torch, got, ref["grad"], ref["pi"], reg, dtype, gain=gain)
    assert not fails, f"{what}: gradient rows (regime, row, error, bar) {fails}"


def check_mstep(torch, d, ref, out, grad, res, dtype, what, hits=True):
    """out / gradient / scattered residuals of one M-step call against the float64 reference (gain 1)."""
    reg, idx = d["regime"], d["idx"]
    fails = nll_failures(res[idx], ref["nll"], reg)
    assert not fails, f"{what}: NLL rows (regime, row, got, want) {fails}"
    untouched = np.ones(res.shape[0], bool)
    untouched[idx] = False
    assert np.array_equal(res[untouched], d["residuals"][untouched]), f"{what}: a residual outside idx was written"
    want = np.float32(ref["loss"])
    if np.isfinite(want):
        assert abs(float(out[0]) - ref["loss"]) <= REL * abs(ref["loss"]), (what, float(out[0]), ref["loss"])
        assert abs(float(out[2]) - ref["loss"]) <= REL * abs(ref["loss"]), (what, float(out[2]), ref["loss"])
    else:
        assert same_nonfinite(out[0], want) and same_nonfinite(out[2], want), (what, out, want)
    if hits:
        assert float(out[3]) == float(ref["hits"]), (what, float(out[3]), ref["hits"])
    if grad is not None:
        check_grad(torch, grad, ref, d, dtype, what)


def check_modest_loss(gpu, d, ref, dtype, what, form=None, ws=None, pitch=None, knobs=()):
    """The same launch again with the weights of the rows outside logit_regimes.modest_rows set to zero:
    the loss of the rows whose terms an edge row's 65 504 ... 3e38 would otherwise drown, to REL.  The same shape, so
    the same kernel body (asserted where the caller names it)."""
    keep = modest_rows(ref)
    w = d["weights"].copy()
    w[d["idx"][~keep]] = 0.0
    want = float(np.sum(ref["pi"][keep] * ref["nll"][keep]))
    assert 0.0 < want < 1e3 * keep.sum()
    try:
        for name, value in knobs:
            tune(name, value)
        out, _, _, took = mstep(gpu, dict(d, weights=w), dtype, ws=ws, pitch=pitch)
    finally:
        untune(*[name for name, _ in knobs])
    assert form is None or took == form, (what, took, form)
    assert abs(float(out[0]) - want) <= REL * want, (what, "loss of the modest rows", float(out[0]), want)
    assert abs(float(out[2]) - want) <= REL * want, (what, "loss of the modest rows", float(out[2]), want)


# ------------------------------------------------------------------------------ A: every kernel body, finite regimes
# (B, C, dtype, knobs, HBM hint, the form rlvi_workspace_last_mstep_form must report): the dispatch lists of
# test_mstep_dispatch_by_launch_size_vs_oracle and test_fp16_gpu, whose row counts are the smallest that select each
# body; the bench-sized launches that alone take the 16-wave tile (form 3) and the timed hold (form 2 + 16); and the
# small launches that the knobs send to a tile or to another lane group.  Forms: 1 register rows, 2 four-wave tiles,
# 3 16-wave tiles, 4 the word-wise 2-byte tile, 5 long rows.  A changed dispatch threshold fails the form assertion
# here instead of silently moving a case to another body.
FORMS = {
    # the f32 / bf16 dispatch list
    (70003, 10, "f32"): 2, (40001, 101, "f32"): 2, (33001, 102, "f32"): 2, (20005, 100, "f32"): 2,
    (9001, 100, "f32"): 2, (70003, 7, "f32"): 2, (1024, 101, "bf16"): 1, (8195, 101, "bf16"): 1,
    (70003, 101, "bf16"): 4, (32768, 33, "bf16"): 4, (40000, 127, "bf16"): 4, (36005, 9, "bf16"): 4,
    (1029, 104, "bf16"): 1, (20005, 104, "bf16"): 2, (3000, 200, "bf16"): 1, (20003, 365, "f32"): 2,
    (9001, 201, "f32"): 2, (8200, 366, "f32"): 2, (8200, 366, "bf16"): 2, (9001, 365, "bf16"): 1,
    (16411, 48, "bf16"): 2, (20003, 64, "bf16"): 2, (301, 3000, "f32"): 5, (70, 21841, "f32"): 5,
    (1030, 513, "f32"): 5, (1100, 2052, "f32"): 5, (130, 4104, "bf16"): 5, (257, 1001, "bf16"): 5,
    # test_fp16_gpu.SHAPES
    (1024, 101, "f16"): 1, (8195, 101, "f16"): 1, (70003, 101, "f16"): 4, (32768, 33, "f16"): 4,
    (40000, 127, "f16"): 4, (36005, 9, "f16"): 4, (1029, 104, "f16"): 1, (20005, 104, "f16"): 2,
    (65536, 104, "f16"): 3, (3000, 200, "f16"): 1, (8200, 366, "f16"): 2, (9001, 365, "f16"): 1,
    (16411, 48, "f16"): 2, (20003, 64, "f16"): 2, (130, 4104, "f16"): 5, (257, 1001, "f16"): 5,
    (65536, 100, "f16"): 2,          # (200-byte rows: 8-byte vectors, which the 16-wave tile does not take)
}
CASES_A = [(b, c, dt, (), False, f) for (b, c, dt), f in FORMS.items()] + [
    (65536, 100, "f32", (), False, 3),                         # the bench shape: 16-wave tiles
    (65536, 100, "f32", (), True, 2 + HOLD),                   # ... with ops.hint_logits_from_hbm: four-wave tiles, timed hold
    (65536, 104, "bf16", (), False, 3),
    (80, 100, "f32", (("RLVI_MSTEP_FORM", 1),), False, 2),     # wave tiles at a launch of two tiles
    (80, 100, "bf16", (("RLVI_MSTEP_FORM", 1),), False, 2),
    (80, 100, "f16", (("RLVI_MSTEP_FORM", 1),), False, 2),
    (80, 100, "f32", (("RLVI_MSTEP_FORM", 1), ("RLVI_MSTEP_G", 8)), False, 2),    # ... eight lanes per row
    (80, 100, "f32", (("RLVI_MSTEP_G", 4),), False, 1),        # register rows, four / thirty-two lanes per row
    (80, 100, "f32", (("RLVI_MSTEP_G", 32),), False, 1),
    (80, 104, "bf16", (("RLVI_MSTEP_G", 2),), False, 1),
    (80, 104, "f16", (("RLVI_MSTEP_G", 16),), False, 1),
]


def test_the_case_list_reaches_every_form_in_every_dtype():
    """(needs no device, but belongs to this table)  Forms 1, 2, 3 and 5 in fp32, bf16 and fp16, the word-wise tile (4) in
    both 2-byte types (fp32 has no such body), the hold bit in one fp32 case; bf16 and fp16 take the same form at every
    shape both lists hold."""
    assert set(FORMS) == set(DISPATCH_SHAPES) | {(b, c, "f16") for b, c in F16_SHAPES}     # both lists, whole
    for dt in ("f32", "bf16", "f16"):
        taken = {f for (_, _, d, k, h, f) in CASES_A if d == dt}
        assert {1, 2, 3, 5} <= taken and ((4 in taken) == (dt != "f32")), (dt, taken)
    assert (2 + HOLD) in {f for (_, _, d, k, h, f) in CASES_A if d == "f32"}
    for (b, c, dt), f in FORMS.items():
        if dt == "f16" and (b, c, "bf16") in FORMS:
            assert FORMS[(b, c, "bf16")] == f, (b, c)


@pytest.mark.parametrize("B,C,dtype,knobs,hint,form", CASES_A,
                         ids=[f"{b}x{c}-{dt}" + "".join(f"-{n[5:]}={v}" for n, v in k) + ("-hbm" if h else "")
                              for b, c, dt, k, h, _ in CASES_A])
def test_mstep_every_body_on_the_finite_regimes(B, C, dtype, knobs, hint, form, gpu):
    torch, ops, dev = gpu
    d = regime_inputs(B, C, dtype, seed=B + C, N=B + 17, zero_frac=0.1)
    ref = reference(d["logits"], d["labels"], d["idx"], d["weights"])
    ws = ops.Workspace(dev, B + 17, B)
    if hint:
        ops.hint_logits_from_hbm(ws)
    try:
        for name, value in knobs:
            tune(name, value)
        out, grad, res, took = mstep(gpu, d, dtype, ws=ws)
        other = None
        if dtype == "f16" and not knobs:
            other = mstep(gpu, d, "bf16", ws=ws, want_grad=True)[3]    # (fp16-rounded values: only the form is looked at)
    finally:
        untune(*[name for name, _ in knobs])
    check_mstep(torch, d, ref, out, grad, res, dtype, f"{B} x {C} {dtype} form {took}")
    check_modest_loss(gpu, d, ref, dtype, f"{B} x {C} {dtype}", form=form, ws=ws, knobs=knobs)
    assert took == form, f"{B} x {C} {dtype}: kernel form {took}, this case is here for form {form}"
    assert other is None or other == took, f"bf16 takes form {other}, fp16 form {took}"


# ------------------------------------------------------------------------------ B: masked rows
@pytest.mark.parametrize("B,C,dtype", [(70, c, dt) for c in (10, 101, 1001, 2052, 4104) for dt in ("f32", "bf16", "f16")]
                         + [(1100, c, "f32") for c in (1001, 2052, 4104)])
def test_masked_rows_equal_the_rows_without_the_masked_columns(B, C, dtype, gpu):
    """A row that is -inf but for the label and one to five other columns against the dense row of those two to six
    values: the same NLL, the same gradient on the survivors, exactly zero on every -inf column.  The other regimes share
    the masked rows' tiles.  fp32 rows of 1001, 2052 and 4104 elements are long rows: 70 of them a workgroup per row,
    1100 a wave per row."""
    torch, ops, dev = gpu
    d = regime_inputs(B, C, dtype, seed=3 * B + C, N=B)
    out, grad, res, took = mstep(gpu, d, dtype)
    if dtype == "f32" and C > 1000:
        assert took == 5
    z, y, idx, w = d["logits"], d["labels"], d["idx"], d["weights"]
    rows = np.nonzero(d["regime"] == 4)[0]
    rtol, atol = LOWP.get(dtype, (0.0, 0.0))
    seen = set()
    ws8 = ops.Workspace(dev, 8, 8)
    for i in rows:
        keep = np.nonzero(np.isfinite(z[i]))[0]
        seen.add(len(keep))
        assert np.all(grad[i][np.isneginf(z[i])] == 0.0), f"masked row {i}: a gradient on a -inf column"
        # the dense problem: this row's survivors, eight times (a launch of one row would not be a tile of rows)
        dd = dict(logits=np.tile(z[i, keep], (8, 1)), labels=np.full(8, int(np.nonzero(keep == y[i])[0][0]), np.int64),
                  idx=np.arange(8, dtype=np.int64), weights=np.full(8, w[idx[i]], np.float32),
                  residuals=np.zeros(8, np.float32))
        o2, g2, r2, _ = mstep(gpu, dd, dtype, ws=ws8)
        pi = float(w[idx[i]])
        assert abs(float(res[idx[i]]) - float(r2[0])) <= 1e-6 + REL * abs(float(r2[0])), (i, res[idx[i]], r2[0])
        bar = 1e-6 * pi + REL * np.abs(g2[0]).max() + rtol * np.abs(g2[0]) + atol
        assert np.all(np.abs(grad[i, keep] - g2[0]) <= bar), (i, grad[i, keep], g2[0])
    assert len(seen) >= 3                                    # (runs of several lengths were there)
    ref = reference(z, y, idx, w)
    check_mstep(torch, d, ref, out, grad, res, dtype, f"{B} x {C} {dtype}")
    check_modest_loss(gpu, d, ref, dtype, f"{B} x {C} {dtype}", form=took)


# ------------------------------------------------------------------------------ C: strided, forward-only, evaluation
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_strided_forward_only_and_evaluation_forms(dtype, gpu):
    torch, ops, dev = gpu
    B, C, LD = 96, 100, 128
    d = regime_inputs(B, C, dtype, seed=11, N=B + 17, zero_frac=0.1)
    ref = reference(d["logits"], d["labels"], d["idx"], d["weights"])
    out, grad, res, _ = mstep(gpu, d, dtype, pitch=LD)                       # ld > C
    check_mstep(torch, d, ref, out, grad, res, dtype, f"pitch {LD} {dtype}")
    check_modest_loss(gpu, d, ref, dtype, f"pitch {LD} {dtype}", pitch=LD)
    out2, none, res2, _ = mstep(gpu, d, dtype, want_grad=False)              # forward only, dense
    assert none is None
    check_mstep(torch, d, ref, out2, None, res2, dtype, f"forward only {dtype}")
    out3, none, res3, _ = mstep(gpu, d, dtype, want_grad=False, pitch=LD)
    assert np.array_equal(out3, out) and np.array_equal(res3, res)
    # the evaluation form and per_sample_ce: plain CE, pi = 1
    B, C = 3000, 37
    d = regime_inputs(B, C, dtype, seed=8)
    ref = reference(d["logits"], d["labels"], None, None)
    z = torch.from_numpy(d["logits"]).to(dev).to(tdtype(torch, dtype))
    y = torch.from_numpy(d["labels"]).to(dev)
    ws = ops.Workspace(dev, B, B)
    o = ops.evaluate_batch(z, y, ws=ws).cpu().numpy()
    mean = ref["loss"] / B
    assert abs(float(o[0]) - mean) <= REL * mean and abs(float(o[2]) - ref["loss"]) <= REL * ref["loss"]
    assert float(o[3]) == float(ref["hits"]) and float(o[1]) == pytest.approx(100.0 * ref["hits"] / B, abs=1e-3)
    # (one edge row's NLL is most of that sum: the batch without the rows of 65 504 and more, where every row's term counts)
    keep = modest_rows(ref)
    o = ops.evaluate_batch(z[torch.from_numpy(keep).to(dev)], y[torch.from_numpy(keep).to(dev)], ws=ws).cpu().numpy()
    want = float(ref["nll"][keep].sum())
    assert 0.0 < want < 1e3 * keep.sum()
    assert abs(float(o[2]) - want) <= REL * want and abs(float(o[0]) - want / keep.sum()) <= REL * want / keep.sum()
    assert float(o[3]) == float(ref["hit"][keep].sum())
    rows = ops.per_sample_ce(z, y, ws=ws).cpu().numpy()
    fails = nll_failures(rows, ref["nll"], d["regime"])
    assert not fails, f"per_sample_ce {dtype}: (regime, row, got, want) {fails}"
    assert ws.status() == 0


# ------------------------------------------------------------------------------ D: non-finite rows
@pytest.mark.parametrize("kinds", [NONFINITE[:3], NONFINITE[3:]], ids=["inf", "nan"])
@pytest.mark.parametrize("B,C,dtype", [(80, 10, "f32"), (80, 10, "f16"), (80, 100, "f32"), (80, 100, "f16"),
                                       (33000, 101, "bf16"), (70, 2052, "f32")])
def test_non_finite_rows_stay_in_their_rows(B, C, dtype, kinds, gpu):
    """Rows with the label at -inf (NLL +inf, a finite gradient), a +inf entry away from the label, nothing but -inf
    (both NaN) -- and, in a call of its own, a NaN entry -- among rows of every finite regime, all with pi > 0.  The
    finite rows meet the bars (nothing leaks across the rows of a tile), the others have inf / NaN exactly where the
    reference has them, in the scattered residual and in the gradient row; the batch loss is NaN as the reference's;
    the hit count is the reference's.  With a NaN row the hit count is not asserted: precision@1 of a NaN row is
    unpinned in the reference (its topk runs over an all-NaN softmax).  These are values, not bad pointers or indexes:
    every label and index is in range and the status stays 0.  M-step (80 x 10 register rows, 33 000 x 101 bf16 the
    word-wise tile, 70 x 2052 a workgroup per row; 80 x 100 also as wave tiles) and the evaluation form."""
    torch, ops, dev = gpu
    d = regime_inputs(B, C, dtype, seed=B + 7 * C, regimes=FINITE + kinds, N=B + 17)
    assert np.all(d["weights"] > 0)
    ref = reference(d["logits"], d["labels"], d["idx"], d["weights"])
    assert np.isnan(ref["loss"])
    pinned = 10 not in kinds
    runs = [("", ())] + ([("tiles", (("RLVI_MSTEP_FORM", 1),))] if (B, C) == (80, 100) else [])
    for what, knobs in runs:
        try:
            for name, value in knobs:
                tune(name, value)
            out, grad, res, took = mstep(gpu, d, dtype)
        finally:
            untune(*[name for name, _ in knobs])
        assert took == (2 if knobs else {10: 1, 100: 1, 101: 4, 2052: 5}[C]), (B, C, dtype, what, took)
        check_mstep(torch, d, ref, out, grad, res, dtype, f"{B} x {C} {dtype} {what} form {took}", hits=pinned)
    ev = reference(d["logits"], d["labels"], None, None)
    ws = ops.Workspace(dev, B, B)
    z = torch.from_numpy(d["logits"]).to(dev).to(tdtype(torch, dtype))
    o = ops.evaluate_batch(z, torch.from_numpy(d["labels"]).to(dev), ws=ws).cpu().numpy()
    assert np.isnan(o[0]) and np.isnan(o[2])
    assert not pinned or float(o[3]) == float(ev["hits"])
    rows = ops.per_sample_ce(z, torch.from_numpy(d["labels"]).to(dev), ws=ws).cpu().numpy()
    fails = nll_failures(rows, ev["nll"], d["regime"])
    assert not fails, f"per_sample_ce: (regime, row, got, want) {fails}"
    assert ws.status() == 0


# ------------------------------------------------------------------------------ E: the in-batch E+M
def fused_em(gpu, d, pi0, fused):
    torch, ops, dev = gpu
    B = pi0.shape[0]
    ws = ops.Workspace(dev, B, B)
    tune("RLVI_FUSED_EM", 1 if fused else 0)
    try:
        pit = torch.from_numpy(pi0.copy()).to(dev)
        out, grad, rows, iters = ops.fused_em(torch.from_numpy(d["logits"]).to(dev),
                                              torch.from_numpy(d["labels"]).to(dev), pit, ws=ws)
        torch.cuda.synchronize()
        assert ws.status() == 0
        return out.cpu().numpy(), grad.cpu().numpy(), rows.cpu().numpy(), pit.cpu().numpy(), int(iters)
    finally:
        untune("RLVI_FUSED_EM")


@pytest.mark.parametrize("B,C,path", [(4096, 10, "rows"), (4096, 100, "rows4"), (16384, 100, "lds"),
                                      (65536, 100, "lds"), (1000, 100, "rows4")])
def test_fused_em_on_the_finite_regimes(B, C, path, gpu, oracle):
    """ops.fused_em in one launch (a row per thread, four lanes per row, the block resident in LDS) against the
    three-launch composition (RLVI_FUSED_EM=0) and the composition against the references.  The LDS-resident launch
    promises the M-step kernel's bits: the assertions of test_fused_em_one_launch_equals_the_three_launch_composition;
    the register-row launches add a row's exponentials in another order: those of
    test_fused_em_short_rows_in_one_launch.  NLLs of several hundred (and one of 3e38) drive exp(-l) and pi to 0: that
    is the reference's behaviour and what is expected."""
    torch, ops, dev = gpu
    d = regime_inputs(B, C, "f32", seed=B + 3 * C)
    pi0 = np.random.default_rng(B + C).random(B).astype(np.float32)
    f = fused_em(gpu, d, pi0, True)
    c = fused_em(gpu, d, pi0, False)
    assert f[4] == c[4]
    if path == "lds":
        assert np.array_equal(f[2], c[2]), "loss rows"
        if (B + 255) // 256 == 256:
            assert np.array_equal(f[3], c[3]), "pi"
            assert np.array_equal(f[1], c[1]), "gradient"
        else:
            np.testing.assert_allclose(f[3], c[3], rtol=2e-6, atol=1e-30)
            np.testing.assert_allclose(f[1], c[1], rtol=4e-6, atol=4e-6 / B)
        np.testing.assert_allclose(f[0], c[0], rtol=2e-6)
    else:
        np.testing.assert_allclose(f[2], c[2], rtol=REL, atol=1e-6)
        rel, small = rel_pi(f[3], c[3])
        assert rel <= REL and small <= 1e-7
        gd = f[1].astype(np.float64) - c[1]
        assert np.sqrt((gd ** 2).sum()) <= REL * np.sqrt((c[1].astype(np.float64) ** 2).sum())
        assert np.abs(gd).max() <= 1e-6
        np.testing.assert_allclose(f[0], c[0], rtol=REL)
    assert f[0][3] == c[0][3]
    # the composition: loss rows (min-shifted NLL) and gradient against the float64 reference with the composition's pi
    out, grad, rows, pi, iters = c
    ref = reference(d["logits"], d["labels"], None, pi, gain=1.0 / B)
    fails = nll_failures(rows, ref["nll"] - ref["nll"].min(), d["regime"])
    assert not fails, f"loss rows (regime, row, got, want) {fails}"
    fails = grad_failures(grad, ref["grad"], pi, d["regime"], gain=1.0 / B)
    assert not fails, f"gradient rows (regime, row, error, bar) {fails}"
    assert abs(float(out[0]) - ref["loss"]) <= REL * abs(ref["loss"])
    assert float(out[3]) == float(ref["hits"])
    # pi and the iteration count: the oracle's E-step on the composition's own loss rows
    l2, w2 = rows.copy(), pi0.copy()
    it, err, _ = oracle.update_sample_weights(l2, w2, trace=True)
    assert np.min(np.abs(err - 1e-3)) > 1e-4 * 1e-3          # (these inputs' stop decision is not a near-tie)
    assert iters == it
    rel, small = rel_pi(pi, w2)
    assert rel <= REL and small <= 1e-7
    assert int((w2 == 0).sum()) > B // 16                     # (the wide rows' pi does underflow to 0)


# ------------------------------------------------------------------------------ F: precision@k
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", [1, 2, 7, 33, 101, 513, 1000])
def test_precision_at_k_on_the_regimes(C, dtype, gpu):
    torch, ops, dev = gpu
    B = 257
    d = regime_inputs(B, C, dtype, seed=C, regimes=FINITE + NONFINITE[:2])
    ref = reference(d["logits"], d["labels"], None, None)
    ks = sorted({1, min(5, C)})
    z = torch.from_numpy(d["logits"]).to(dev).to(tdtype(torch, dtype))
    got = ops.topk_hits(z, torch.from_numpy(d["labels"]).to(dev), ks).cpu().numpy()
    want = [int((ref["rank"] < k).sum()) for k in ks]
    if got.tolist() != want:
        per = {REGIME_NAMES[r]: [int((ref["rank"][d["regime"] == r] < k).sum()) for k in ks] for r in set(d["regime"])}
        raise AssertionError(f"hits {got.tolist()} against {want}; the reference per regime: {per}")


# ------------------------------------------------------------------------------ G: the small-loss selection
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("B", [200, 4097])
def test_small_loss_selection_on_the_regimes(B, dtype, gpu, oracle):
    """train_usdnl.loss_fn at forget rate 0.3 on the finite regimes and rows whose label column is -inf (NLL +inf): the
    kept set is the stable argsort of the kernel's own row losses (no near-tie margin needed), those meet the NLL bar,
    a row with NLL +inf is never kept (there are fewer of them than B - k) and takes nothing out of the loss of the
    rows that are; loss and gradient are the reference's for that kept set."""
    torch, ops, dev = gpu
    import importlib
    usdnl = importlib.import_module("rlvi_amd.methods.train_usdnl")
    C, fr = 100, 0.3
    k = int((1 - fr) * B)
    d = regime_inputs(B, C, dtype, seed=B, regimes=FINITE + NONFINITE[:1])
    full = reference(d["logits"], d["labels"], None, None)
    z = torch.from_numpy(d["logits"]).to(dev).to(tdtype(torch, dtype)).requires_grad_(True)
    t = torch.from_numpy(d["labels"]).to(dev)
    loss = usdnl.loss_fn(z, t, fr)
    loss.backward()
    rows_t = ops.per_sample_ce(z.detach(), t)
    mask = ops.select_smallest(rows_t, k).cpu().numpy()
    rows = rows_t.cpu().numpy()
    fails = nll_failures(rows, full["nll"], d["regime"])
    assert not fails, f"per_sample_ce (regime, row, got, want) {fails}"
    assert np.array_equal(mask, oracle.select_smallest(rows, k))            # the stable argsort's first k
    kept = mask != 0
    inf = np.isposinf(rows)
    assert 0 < int(inf.sum()) < B - k and not kept[inf].any() and int(kept.sum()) == k
    g = z.grad.float().cpu().numpy()
    assert not g[~kept].any(), "a gradient on a row that was not kept"
    ref = reference(d["logits"][kept], d["labels"][kept], None, None, gain=1.0 / k)
    # (the mean of k rows that each meet the NLL bar)
    assert abs(float(loss) - ref["loss"]) <= REL * abs(ref["loss"]) + 1e-6, (float(loss), ref["loss"])
    sub = dict(regime=d["regime"][kept])
    check_grad(torch, g[kept], ref, sub, dtype, f"usdnl {B} {dtype}", gain=1.0 / k)
    assert ops.workspace(dev).status() == 0
