"""The end of the 16-wave fp32 M-step form (mstep_wave_kernel, ENTRY_FIRST): the gradient tile leaves LDS through
global stores on a scalar base + the loads' 32-bit lane offsets, piece by piece as the LDS reads return; the residual
scatter is a global store; thread 0 asks for the sixteen waves' pairs in one go, adds them in the old order and, in
accumulate mode, adds the record with the hardware's atomic itself.

tests/test_mstep_entry_gpu.py's scheme and helpers: the smallest launches that reach the form (rows_for), every case
against the CPU oracle at the suite's REL and bit for bit (gradient, residuals) against the four-wave form of the same
launch (RLVI_MSTEP_CUWIDE=0), whose stores and record tail are the old ones; a case whose launch did not take the
16-wave form is skipped.

What each case is for:
  C = 100          the partial last slot; the last piece's store is bounded (400 chunks, 448 lanes' worth)
  C = 84, C = 68   a partial last 1-KiB piece: the clamped offset and the bound of the last store
  C = 40           not EXACT: every store goes through the bounds branch, every offset is its own register
  C = 128          eight full pieces: four immediates, four offsets past the instruction's offset field
  trailing         five rows behind the tiles (the register-row kernel adds them to record 0)
  partial wg       a last workgroup with five tile waves: eleven waves only join the barriers, and its thread 0 still
                   writes the record from what wave 0's tile path left
  no idx / no residuals (no scatter) / a grad_scale tensor / out-of-range label and index / two accumulate launches
The default launch (accumulate=False, its own finalize) is the record's plain-store branch; accumulate=True the four
fp64 adds.  For fp32 logits the library's entry has no grad_scale argument (the kernel's pointer is NULL; the scale
multiplies the gradient afterwards), so that case checks the public call, not a kernel branch.
"""
import numpy as np
import pytest

from rlvi_amd import synth
from test_mstep_entry_gpu import (FORM_CUWIDE, both_forms, check_oracle, check_same_bits, gpu,  # noqa: F401
                                  last_form, launch, nothing_left_behind, rows_for)
from test_oracle_golden import REL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("C,shape", [(100, "full"), (84, "full"), (68, "full"), (40, "full"), (128, "full"),
                                     (100, "trailing"), (68, "trailing"), (128, "trailing"),
                                     (100, "partial_workgroup"), (68, "partial_workgroup"),
                                     (128, "partial_workgroup")])
def test_tail_shapes_vs_oracle_and_four_wave_form(gpu, oracle, C, shape):
    torch, ops, dev = gpu
    B = rows_for(torch, partial_workgroup=shape == "partial_workgroup", trailing=5 if shape == "trailing" else 0)
    d = synth.mstep_inputs(B, C, N=B + 41, seed=2100 + C)
    out, grad, res, _ = both_forms(gpu, d)
    check_oracle(oracle, d, out, grad, res)
    assert ops.workspace(dev).status() == 0


def test_tail_without_idx(gpu, oracle):
    torch, ops, dev = gpu
    B, C = rows_for(torch, partial_workgroup=True), 100
    d = synth.mstep_inputs(B, C, N=B, seed=2201)
    out, grad, res, _ = both_forms(gpu, d, idx=False)
    check_oracle(oracle, d, out, grad, res, idx=False)


def test_tail_without_residuals_scatters_nothing(gpu, oracle):
    torch, ops, dev = gpu
    B, C = rows_for(torch, trailing=5), 84
    d = synth.mstep_inputs(B, C, N=B + 3, seed=2202)
    out, grad, res, _ = both_forms(gpu, d, residuals=False)
    assert res is None
    check_oracle(oracle, d, out, grad, None)


def test_tail_with_grad_scale(gpu, oracle):
    """grad_scale = 1024 (a power of two: the scaled gradient is the unscaled one's bits with another exponent)."""
    torch, ops, dev = gpu
    from rlvi_amd import _lib
    L = _lib.load()
    B, C = rows_for(torch), 100
    d = synth.mstep_inputs(B, C, N=B + 7, seed=2203)
    plain = both_forms(gpu, d)
    t = {k: torch.from_numpy(v.copy()).to(dev) for k, v in d.items()}
    scale = torch.full((1,), 1024.0, device=dev)
    _lib.check(L.rlvi_tune_set(b"RLVI_MSTEP_CUWIDE", 1), "tune")
    try:
        out, grad = ops.mstep_fwd_bwd(t["logits"], t["labels"], t["idx"], t["weights"], t["residuals"],
                                      grad_scale=scale)
        torch.cuda.synchronize()
        form = last_form(ops, dev)
    finally:
        L.rlvi_tune_unset(b"RLVI_MSTEP_CUWIDE")
    assert form == FORM_CUWIDE
    assert np.array_equal(grad.cpu().numpy(), plain[1] * np.float32(1024.0))
    assert np.array_equal(t["residuals"].cpu().numpy(), plain[2])
    assert np.array_equal(out.cpu().numpy(), plain[0])
    check_oracle(oracle, d, plain[0], plain[1], plain[2])


def test_tail_out_of_range_label_and_index(gpu, oracle):
    """Status raised, zero gradient rows, no scatter for the two rows; the rest as without them."""
    torch, ops, dev = gpu
    from rlvi_amd import _lib
    B, C = rows_for(torch, partial_workgroup=True), 100
    N = B + 13
    d = synth.mstep_inputs(B, C, N=N, seed=2204)
    bad_label, bad_index = 16 * 3 + 6, B - 16 * 2 - 5          # (the second one in the partial workgroup's tiles)
    clean_idx = d["idx"].copy()
    d["labels"][bad_label] = -1
    d["idx"][bad_index] = N + 5
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


def test_tail_accumulate_two_launches_then_reduce_is_deterministic(gpu, oracle):
    """accumulate=True twice, then mstep_reduce: the sum of two oracle calls; and `out` bit-equal between two
    identical runs on fresh workspaces (one adder per record and launch, an ordered sum inside the workgroup)."""
    torch, ops, dev = gpu
    from rlvi_amd import _lib
    L = _lib.load()
    B, C = rows_for(torch, partial_workgroup=True), 100
    N = 2 * B
    d = synth.mstep_inputs(2 * B, C, N=N, seed=2205)
    halves = [{k: (v[h * B:(h + 1) * B] if k in ("logits", "labels", "idx") else v) for k, v in d.items()}
              for h in range(2)]
    w = torch.from_numpy(d["weights"]).to(dev)
    dev_halves = [{k: torch.from_numpy(h[k]).to(dev) for k in ("logits", "labels", "idx")} for h in halves]

    def run(cuwide):
        ws = ops.Workspace(dev, N, B)
        res = torch.zeros(N, device=dev)
        grads, forms = [], []
        _lib.check(L.rlvi_tune_set(b"RLVI_MSTEP_CUWIDE", cuwide), "tune")
        try:
            for h in dev_halves:
                _, g = ops.mstep_fwd_bwd(h["logits"], h["labels"], h["idx"], w, res, ws=ws, accumulate=True)
                forms.append(last_form(ops, dev, ws))
                grads.append(g)
            out = ops.mstep_reduce(ws=ws)
            torch.cuda.synchronize()
        finally:
            L.rlvi_tune_unset(b"RLVI_MSTEP_CUWIDE")
        assert ws.status() == 0
        return out.cpu().numpy(), np.concatenate([g.cpu().numpy() for g in grads]), res.cpu().numpy(), forms

    first = run(1)
    if first[3] != [FORM_CUWIDE, FORM_CUWIDE]:
        pytest.skip(f"the launcher took forms {first[3]}, not the 16-wave form")
    again = run(1)
    assert first[0].tobytes() == again[0].tobytes(), "out differs between two identical runs"
    assert np.array_equal(first[1], again[1]) and np.array_equal(first[2], again[2])
    four = run(0)
    assert FORM_CUWIDE not in four[3]
    check_same_bits(first, four)
    out, grad, res, _ = first
    r0 = np.zeros(N, np.float32)
    refs = [oracle.mstep(h["logits"], h["labels"], h["idx"], d["weights"], r0) for h in halves]
    loss = float(refs[0]["loss"]) + float(refs[1]["loss"])
    assert abs(float(out[0]) - loss) <= REL * loss
    assert float(out[3]) == float(sum(round(float(r["prec1"]) * B / 100.0) for r in refs))
    np.testing.assert_allclose(res, r0, rtol=REL, atol=1e-6)
    ref_grad = np.concatenate([r["grad"] for r in refs])
    diff = grad.astype(np.float64) - ref_grad
    assert np.sqrt((diff ** 2).sum()) <= REL * np.sqrt((ref_grad.astype(np.float64) ** 2).sum())
    assert np.abs(diff).max() <= 1e-6
