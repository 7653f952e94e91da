"""Logits beyond the synthetic range, and a float64 reference of the row softmax (numpy only; a helper, not a test
module).

synth.mstep_inputs draws 3 * N(0, 1) with +12 on some label entries: no logit beyond about 25, every row of a tile at
the same scale.  Softmax is shift-invariant, so with such inputs a kernel may subtract a wrong maximum -- a
neighbouring row's, a masked slot's, a partial one that was never combined across lanes or waves -- and still agree to
1e-5.  regime_inputs() gives every row of a batch another regime (row i: regimes[i % len(regimes)]), so that every
16-row and 64-row tile holds all of them and neighbouring rows never share one:

  0 plain      the synthetic row
  1 offset     the row shifted by +-2^14 * (1 + i % 3) (below fp16's 65504; 2-byte spacing there is 16 ... 128: ties)
  2 wide       the row times 40: most exponentials underflow, NLLs of several hundred
  3 saturated  the label entry +60 (even occurrences of the regime) or -60 (odd ones)
  4 masked     -inf everywhere but the label and a run of 1 + i % 5 other columns whose start walks over [0, C)
  5 zeros      +-0, +-the smallest subnormal and +-the smallest normal of the storage type: a uniform softmax, tied maxima
  6 edge       up to three entries at +-65504; fp32, odd occurrences: at 3e38 instead (see below)

and the non-finite kinds, used only where a test names them:

  7 (a) label_ninf   the label column -inf, the rest finite: NLL +inf, a finite gradient
  8 (b) pinf         one +inf entry away from the label: NLL and gradient NaN
  9 (c) all_ninf     the whole row -inf: NaN
 10 (d) nan          one NaN entry: NaN

The 3e38 variant of regime 6: fp32 differences of two such entries of opposite sign overflow where float64's do not, so a
label at -3e38 beside a maximum of +3e38 would have an fp32 NLL of +inf against a finite float64 one.  The variant
therefore keeps the float64 reference, every correct fp32 evaluation and the batch's loss sum finite: its entries
are -3e38, the label's own (when it is among them) +3e38, and only the regime's FIRST such row of a batch carries
a +3e38 entry away from the label (an NLL of 3e38; two of them would overflow the fp32 loss sum).  With that, the
float64 reference is finite on all seven finite regimes and the variant was not dropped.
"""
import numpy as np

from rlvi_amd import synth

REGIME_NAMES = ("plain", "offset", "wide", "saturated", "masked", "zeros", "edge",
                "label_ninf", "pinf", "all_ninf", "nan")
FINITE = (0, 1, 2, 3, 4, 5, 6)
NONFINITE = (7, 8, 9, 10)                  # kinds (a), (b), (c), (d)
DTYPES = ("f32", "bf16", "f16")
F16_MAX = 65504.0
HUGE = 3e38

# smallest subnormal and smallest normal of each storage type
_TINY = {"f32": (2.0 ** -149, 2.0 ** -126), "bf16": (2.0 ** -133, 2.0 ** -126), "f16": (2.0 ** -24, 2.0 ** -14)}


def round_to(z, dtype):
    """fp32 array rounded to the storage type (nearest even) and widened back to fp32."""
    z = np.ascontiguousarray(z, np.float32)
    if dtype == "f32":
        return z.copy()
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return z.astype(np.float16).astype(np.float32)
    if dtype == "bf16":
        u = z.view(np.uint32).astype(np.uint64)
        r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
        r = np.where(np.isnan(z), np.uint32(0x7FC00000), r).astype(np.uint32)
        return r.view(np.float32).reshape(z.shape)
    raise ValueError(dtype)


def masked_columns(i, occ, C, label):
    """The finite columns of masked row i (the `occ`-th row of its regime): the label and a run of 1 + i % 5 other
    columns (fewer only when the row has fewer), starting at a column that walks over [0, C) with `occ`."""
    start = int((occ * 0.6180339887498949) % 1.0 * C)
    want = min(1 + i % 5, C - 1)
    run = []
    c = start
    while len(run) < want:
        if c % C != label:
            run.append(c % C)
        c += 1
    return np.array(sorted(set(run) | {int(label)}), np.int64)


def regime_inputs(B, C, dtype="f32", seed=0, regimes=FINITE, N=None, zero_frac=0.0):
    """synth.mstep_inputs(B, C, N, seed, zero_frac=zero_frac) with row i rewritten for regime regimes[i % len(regimes)];
    the logits rounded to `dtype` and widened back to fp32 (what the references are fed); plus regime[B] (int64)."""
    d = synth.mstep_inputs(B, C, N=N, seed=seed, zero_frac=zero_frac)
    rng = np.random.default_rng(seed + 977)
    z, y = d["logits"], d["labels"]
    nreg = len(regimes)
    regime = np.array([regimes[i % nreg] for i in range(B)], np.int64)
    sub, nrm = _TINY[dtype]
    tiny = np.array([0.0, -0.0, sub, -sub, nrm, -nrm], np.float32)
    huge_first = True
    for i in range(B):
        r, occ, lab = int(regime[i]), i // nreg, int(y[i])
        if r == 1:
            sign = 1.0 if occ % 2 == 0 else -1.0
            z[i] = z[i] + np.float32(sign * 2.0 ** 14 * (1 + i % 3))
        elif r == 2:
            z[i] = z[i] * np.float32(40.0)
        elif r == 3:
            z[i, lab] += np.float32(60.0 if occ % 2 == 0 else -60.0)
        elif r == 4:
            keep = masked_columns(i, occ, C, lab)
            row = np.full(C, -np.inf, np.float32)
            row[keep] = z[i, keep]
            z[i] = row
        elif r == 5:
            z[i] = tiny[rng.integers(0, len(tiny), C)]
        elif r == 6:
            cols = rng.choice(C, size=min(3, C), replace=False)
            if dtype == "f32" and occ % 2 == 1:
                z[i, cols] = np.float32(-HUGE)
                if lab in cols:
                    z[i, lab] = np.float32(HUGE)
                elif huge_first:
                    z[i, cols[0]] = np.float32(HUGE)
                    huge_first = False
            else:
                z[i, cols] = np.where(np.arange(len(cols)) % 2 == occ % 2, F16_MAX, -F16_MAX).astype(np.float32)
        elif r == 7:
            z[i, lab] = -np.inf
        elif r == 8:
            if C > 1:
                z[i, (lab + 1 + occ % (C - 1)) % C] = np.inf
        elif r == 9:
            z[i] = -np.inf
        elif r == 10:
            z[i, (7 * occ + 3) % C] = np.nan
    d["logits"] = round_to(z, dtype)
    d["regime"] = regime
    return d


def reference(logits, labels, idx, weights, gain=1.0):
    """Float64 restatement on fp32-valued logits: per-row NLL -((z_y - m) - log sum exp(z - m)) as torch evaluates it,
    gradient rows gain * pi_i * (softmax - onehot), loss = gain * sum pi_i l_i, top-1 (the label is the FIRST column
    that attains the row maximum: hit[B], hits), and rank[B] as oracle/rlvi_oracle.c defines it for precision@k.
    idx None: identity; weights None: pi = 1.  inf / NaN results are wanted where the arithmetic gives them."""
    z = np.asarray(logits).astype(np.float64)
    y = np.asarray(labels).astype(np.int64)
    B, C = z.shape
    rows = np.arange(B)
    if weights is None:
        pi = np.ones(B)
    else:
        pi = np.asarray(weights).astype(np.float64)[rows if idx is None else np.asarray(idx)]
    with np.errstate(all="ignore"):
        m = z.max(axis=1)
        zy = z[rows, y]
        d = z - m[:, None]
        lse = np.log(np.exp(d).sum(axis=1))
        nll = -((zy - m) - lse)
        grad = np.exp(d - lse[:, None])
        grad[rows, y] -= 1.0
        grad *= (gain * pi)[:, None]
        loss = float(gain * np.sum(pi * nll))
        col = np.arange(C)[None, :]
        first = (zy == m) & ~((z == m[:, None]) & (col < y[:, None])).any(axis=1)
        rank = (z > zy[:, None]).sum(axis=1) + ((z == zy[:, None]) & (col < y[:, None])).sum(axis=1)
    return dict(nll=nll, grad=grad, loss=loss, hit=first, hits=int(first.sum()), rank=rank.astype(np.int64), pi=pi)


NLL_MODEST = 1e3            # rows below it: every regime but the +-65504 / 3e38 rows (and the non-finite kinds)


def modest_rows(ref):
    """Rows whose NLL is below NLL_MODEST.  One edge row's term (65 504 ... 3e38) is most or all of a batch's loss, and
    a relative bar on that total says nothing about the other rows' terms: the loss is ALSO compared over these rows
    alone, with the others' weights set to zero (the same launch shape, so the same kernel body)."""
    with np.errstate(all="ignore"):
        return np.isfinite(ref["nll"]) & (ref["nll"] < NLL_MODEST)


# ------------------------------------------------------------------------------ the bars
REL = 1e-5                  # test_oracle_golden.REL, the project's relative bar


def same_nonfinite(got, ref):
    """inf (with its sign) and NaN at identical positions."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool(np.array_equal(np.isnan(got), np.isnan(ref)) and
                np.array_equal(np.isposinf(got), np.isposinf(ref)) and
                np.array_equal(np.isneginf(got), np.isneginf(ref)))


def nll_failures(got, ref, regime, rtol=REL, atol=1e-6):
    """Rows whose NLL misses rtol / atol or whose inf / NaN differ, as a list of (regime name, row, got, want)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        bad = np.where(fin, ~(np.abs(got - ref) <= atol + rtol * np.abs(ref)),
                       ~((np.isnan(got) & np.isnan(ref)) | (got == ref)))
    return [(REGIME_NAMES[int(regime[i])], int(i), float(got[i]), float(ref[i])) for i in np.nonzero(bad)[0][:8]]


F32_QUANTA = 2.0 ** -148   # two steps of the fp32 subnormal grid


def grad_failures(got, ref, pi, regime, gain=1.0, rel=REL, floor=1e-6):
    """Rows whose gradient misses  max|got - ref| <= gain * floor * pi_i + rel * max|ref| + 2^-148  or whose inf / NaN
    differ, as a list of (regime name, row, error, bar).  The last term is the fp32 format's own: a pi that the E-step
    has driven into the subnormal range (1e-42) gives gradient entries of 1e-46, which an fp32 result can only hold
    to its subnormal grid of 2^-149 -- pi * gain, the division by the sum and the product with the exponential each
    round to it, half a step each at the most."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(all="ignore"):
        fin_row = np.isfinite(ref).all(axis=1)
        err = np.abs(got - ref).max(axis=1)
        bar = gain * floor * np.asarray(pi, np.float64) + rel * np.abs(ref).max(axis=1) + F32_QUANTA
        ok = np.where(fin_row, err <= bar, True)               # (a NaN or inf in `got` fails a finite row)
    for i in np.nonzero(~fin_row)[0]:
        f = np.isfinite(ref[i])
        with np.errstate(all="ignore"):
            b = gain * floor * float(np.asarray(pi)[i]) + rel * (np.abs(ref[i][f]).max() if f.any() else 0.0) + F32_QUANTA
            err[i], bar[i] = (np.abs(got[i][f] - ref[i][f]).max() if f.any() else 0.0), b
        ok[i] = same_nonfinite(got[i], ref[i]) and (not f.any() or err[i] <= b)
    return [(REGIME_NAMES[int(regime[i])], int(i), float(err[i]), float(bar[i])) for i in np.nonzero(~ok)[0][:8]]
