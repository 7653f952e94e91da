#!/usr/bin/env python3
"""Is the product build's gfx950 assembly the same, instruction for instruction, as another checkout's?

    python tools/isa_same.py [--against DIR] [--jobs N] [source.hip ...]

Compiles every .hip of rlvi_amd/csrc (or the given sources) of this checkout and of DIR to assembly, each with the
flags of its own checkout's rlvi_amd/_build.py (tools/prologue_check.py's compile_isa), and compares the text per
file after dropping what names the compilation and not the code: the `.ident` line and the lines of the
`__hip_cuid_<hash>` symbol, a hash over the source's path.  Prints one line per file; for a file that differs, the
first kernel or function whose text differs.  Exit status 1 on any difference, a file missing on one side included.
Without --against: one digest per file, for comparing two runs by hand.
A refactor that may not change what users run is done when this says so; no timing is needed then."""
import argparse
import glob
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from prologue_check import ROOT, compile_isa  # noqa: E402

LABEL = re.compile(r"^([A-Za-z_][\w$.]*):")


def code_lines(asm):
    return [l for l in asm.split("\n") if not l.lstrip().startswith(".ident") and "__hip_cuid_" not in l]


def first_difference(a, b):
    """(symbol the first differing line belongs to, that line in a, in b)"""
    sym = "(file header)"
    for i in range(max(len(a), len(b))):
        la, lb = (a[i] if i < len(a) else "<end>"), (b[i] if i < len(b) else "<end>")
        m = LABEL.match(la)
        if m and not m.group(1).startswith(".L"):
            sym = m.group(1)
        if la != lb:
            out = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
            return out or sym, la.strip(), lb.strip()
    return None


def sources_of(root):
    return {os.path.relpath(p, root) for p in glob.glob(os.path.join(root, "rlvi_amd", "csrc", "*.hip"))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("sources", nargs="*", help="paths relative to the checkout (default: every rlvi_amd/csrc/*.hip)")
    ap.add_argument("--against", help="another checkout of the repository")
    ap.add_argument("--jobs", type=int, default=4)
    a = ap.parse_args()
    other = os.path.abspath(a.against) if a.against else None
    srcs = sorted(a.sources or (sources_of(ROOT) | (sources_of(other) if other else set())))

    def one(src):
        texts = []
        for root in [ROOT] + ([other] if other else []):
            texts.append(code_lines(compile_isa(root, src)) if os.path.exists(os.path.join(root, src)) else None)
        return src, texts

    bad = 0
    with ThreadPoolExecutor(max_workers=max(1, a.jobs)) as ex:
        for src, texts in ex.map(one, srcs):
            if other is None:
                print(f"{src:40s} {hashlib.sha256(chr(10).join(texts[0]).encode()).hexdigest()[:16]}", flush=True)
            elif texts[0] is None or texts[1] is None:
                print(f"{src:40s} MISSING in {'this checkout' if texts[0] is None else a.against}", flush=True)
                bad += 1
            elif texts[0] == texts[1]:
                print(f"{src:40s} identical ({len(texts[0])} lines)", flush=True)
            else:
                sym, la, lb = first_difference(texts[0], texts[1])
                print(f"{src:40s} DIFFERS, first in {sym}\n    this:  {la}\n    other: {lb}", flush=True)
                bad += 1
    if other is not None:
        print("every file identical" if not bad else f"{bad} file(s) differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
