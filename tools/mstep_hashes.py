#!/usr/bin/env python3
"""Bits of the M-step over its forms, one line per case, for comparing two builds of the library:

    RLVI_LIB_PATH=<parent .so> python tools/mstep_hashes.py parent.txt
    python tools/mstep_hashes.py new.txt
    python tools/mstep_hashes.py --compare parent.txt new.txt

Per case: the form code (rlvi_workspace_last_mstep_form), the status word and the SHA-256 of the gradient, of the
residuals and of the four scalars.  The forms of profiles/r06_mstep_cleanup.md: fp32, bf16 and fp16; four- and
16-wave tiles (the second under the caller's HBM hint, with the timed hold); register rows; the word-wise tile of odd
2-byte rows; long rows; trailing rows behind a tile form; a padded pitch; no gradient; no weights; accumulate on
(three launches closed by ops.mstep_reduce) and off.  Seeded inputs from rlvi_amd.synth, N = 2 B, a fresh
workspace per case.  --compare: the two files line for line; exit status 1 on any difference."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def sha(t):
    import torch
    a = t.detach().cpu().contiguous().view(-1)
    return hashlib.sha256(a.view(torch.uint8).numpy().tobytes()).hexdigest()[:24]


def compare(a, b):
    la, lb = open(a).read().splitlines(), open(b).read().splitlines()
    bad = [i for i, (x, y) in enumerate(zip(la, lb)) if x != y]
    if len(la) != len(lb):
        bad.append(min(len(la), len(lb)))
    for i in bad[:20]:
        print("DIFF line", i + 1, "\n  ", la[i] if i < len(la) else "-", "\n  ", lb[i] if i < len(lb) else "-")
    print(f"{a} / {b}: {len(la)} / {len(lb)} lines, {len(bad)} differ")
    sys.exit(1 if bad else 0)


def main():
    if len(sys.argv) < 2 or (sys.argv[1] == "--compare" and len(sys.argv) < 4) or sys.argv[1] in ("-h", "--help"):
        sys.exit(__doc__)
    if sys.argv[1] == "--compare":
        compare(sys.argv[2], sys.argv[3])
    import torch
    from rlvi_amd import _lib, ops, synth
    dev = torch.device("cuda:0")
    L = _lib.load()
    DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
    lines = []

    def case(tag, B, C, dts=("f32", "bf16", "f16"), hint=False, pitch=0, grad=True, weights=True, accumulate=0):
        d = synth.mstep_inputs(B, C, N=2 * B, seed=B + C)
        for dt in dts:
            z = torch.from_numpy(d["logits"]).to(dev).to(DT[dt])
            if pitch:
                zp = torch.zeros(B, pitch, dtype=DT[dt], device=dev)
                zp[:, :C] = z
                z = zp[:, :C]
            y, ix = torch.from_numpy(d["labels"]).to(dev), torch.from_numpy(d["idx"]).to(dev)
            w = torch.from_numpy(d["weights"]).to(dev)
            res = torch.zeros(2 * B, device=dev)
            ws = ops.Workspace(dev, 2 * B, B)
            if hint:
                ops.hint_logits_from_hbm(ws, True)
            g = None
            if grad:
                g = torch.zeros(B, pitch, dtype=DT[dt], device=dev)[:, :C] if pitch else torch.zeros_like(z)
            if not weights:
                out = ops.evaluate_batch(z, y, ws=ws)
            elif accumulate:
                for _ in range(accumulate):
                    ops.mstep_fwd_bwd(z, y, ix, w, res, grad=g, want_grad=grad, ws=ws, accumulate=True)
                out = ops.mstep_reduce(scale=1.0 / accumulate, ws=ws)
            else:
                out, g2 = ops.mstep_fwd_bwd(z, y, ix, w, res, grad=g, want_grad=grad, ws=ws)
                g = g2 if grad else None
            torch.cuda.synchronize()
            form = L.rlvi_workspace_last_mstep_form(ws.ptr)
            st = ws.status()
            lines.append(f"{tag} {B}x{C} {dt} form {form} status {st} grad {sha(g) if g is not None else '-'} "
                         f"res {sha(res)} out {sha(out)}")

    case("default", 65536, 100)
    case("hinted", 65536, 100, hint=True)
    case("hinted", 131072, 100, hint=True)
    case("trailing", 57365, 100)
    case("half", 32768, 100)
    case("small", 4096, 10)
    case("small", 4096, 100)
    case("odd", 65536, 101)
    case("places", 65536, 365)
    for C in (64, 48, 104, 136):
        case("two-byte", 65536, C, dts=("bf16", "f16"))
    case("two-byte", 4096, 4096, dts=("bf16", "f16"))
    case("wide", 16384, 1000)
    case("long", 4096, 4100)
    case("long wide", 256, 21841)
    case("pitch 104", 65536, 100, pitch=104)
    case("no grad", 65536, 100, grad=False)
    case("no weights", 65536, 100, weights=False, grad=False)
    case("accumulate", 65536, 100, accumulate=3)
    case("accumulate odd", 57365, 101, dts=("bf16", "f16"), accumulate=3)
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} lines -> {sys.argv[1]}  (library {_lib.LIB_PATH})")


if __name__ == "__main__":
    main()
