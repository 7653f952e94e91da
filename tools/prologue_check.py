#!/usr/bin/env python3
"""What a kernel does between its first instruction and its first request for data, read off the ISA.

    python tools/prologue_check.py [--against DIR] [--kernel REGEX] [--all] [--stamps] [source.hip ...]

Compiles the sources (default: estep_trajb.hip and mstep.hip) to gfx950 assembly with the flags of
rlvi_amd/_build.py and reports per kernel:
  preload   .amdhsa_user_sgpr_kernarg_preload_length: SGPRs of kernel arguments that arrive with the wave
  instr     instructions from the entry to the first global_load (behind the compatibility header that
            fetches the preloaded arguments the old way on firmware that does not preload)
  last      instructions from the entry to the LAST global_load of the first burst, and the burst's size: the loads
            up to the first s_barrier, s_waitcnt vmcnt(..) or branch behind the first one.  For the M-step's bench
            kernel that is label, index and the seven tile pieces; a SIMD's last wave asks for its tile only when
            every wave in front of it has issued this many instructions
  waits     s_waitcnt lgkmcnt(..) in that stretch -- each one a stall on the argument block or on a scalar load
  rcp       whether a v_rcp_f32 (the software integer division) occurs in it
  state     E-step only: the slice loads (the first global_load) are issued before ANY scalar load that does not go
            through the argument pointer (the warm-start state) and before the first s_waitcnt lgkmcnt behind one
  vgpr / sgpr / scratch / lds / waves per SIMD
  phase C   wave-tile M-step only: instructions from the first ds_read_b128 of the gradient tile's way out of LDS to
            the last gradient store (the *_store_dwordx4 ... nt), and how many flat instructions lie in between
  behind last barrier   instructions from the last s_barrier to the s_endpgm behind it: the record's tail, which
            every CU's last wave has on its path
The stretch is read in layout order, so a side block that the first load's path jumps over is counted too: the
figures are upper bounds.  Without --all only the two bench instantiations are listed.
--against DIR: the same for another checkout of the repository (its own sources, its own flags), side by side.
--stamps: also compiles the lab builds (-DRLVI_STAMPS=1 for the E-step, -DRLVI_MSTEP_STAMPS for the M-step) and checks
that s_memrealtime comes before every s_load and every s_waitcnt behind the header in the bench instantiations.
Exit status 1 when a bench instantiation misses an entry rule (preload, waits, rcp, state) or a resource bound (E-step:
at most 168 VGPRs, the bound of three waves per SIMD; M-step: four waves per SIMD; no scratch), when --stamps finds
the entry stamp late, or when --against shows a listed kernel that gains scratch or drops a wave per SIMD."""
import argparse
import os
import re
import runpy
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = r"estep_trajb_kernel<1, 256>|mstep_wave_kernel<float, 4, 4, 7, 16, true>"
DEFAULT = ["rlvi_amd/csrc/estep_trajb.hip", "rlvi_amd/csrc/mstep.hip"]


STAMP_FLAG = {"estep_trajb.hip": "-DRLVI_STAMPS=1", "mstep.hip": "-DRLVI_MSTEP_STAMPS"}


def compile_isa(root, src, extra=()):
    b = runpy.run_path(os.path.join(root, "rlvi_amd", "_build.py"))
    flags = [f for f in b["FLAGS"] if f != "-fPIC"] + list(extra)
    cmd = [b["HIPCC"]] + flags + ["--cuda-device-only", "-S", "-o", "-", os.path.join(root, src)]
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(.*\)$", "", d).replace("void rlvi::", "") for n, d in zip(names, out)}


def instructions(body):
    """(mnemonic, operands) of the lines of a function body that are instructions"""
    for line in body:
        t = line.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        parts = t.split(None, 1)
        yield parts[0], parts[1] if len(parts) > 1 else ""


def analyse(asm):
    lines = asm.split("\n")
    desc = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S):
        d = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
        desc[m.group(1)] = d
    sets = {}
    for m in re.finditer(r"\.set (\S+?)\.(num_vgpr|num_agpr|numbered_sgpr|private_seg_size), (\d+)", asm):
        sets.setdefault(m.group(1), {})[m.group(2)] = int(m.group(3))
    rows = {}
    for name, d in desc.items():
        start = lines.index(next(l for l in lines if l.startswith(name + ":")))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        ins = list(instructions(lines[start + 1:end]))
        preload = int(d.get("user_sgpr_kernarg_preload_length", 0))
        if preload:
            # the header: loads of the preloaded arguments through s[0:1], one wait, a branch (then padding up to
            # 256 bytes) -- and nothing else
            k = next(i for i, (op, _) in enumerate(ins) if op == "s_branch")
            if not all(op.startswith("s_load") or op == "s_waitcnt" for op, _ in ins[:k]):
                raise SystemExit(f"{name}: no compatibility header where one was expected")
            ins = ins[k + 1:]
        first = next((i for i, (op, _) in enumerate(ins) if op.startswith("global_load")), len(ins))
        head = ins[:first]
        last, burst = first, 0
        for i in range(first, len(ins)):
            op, a = ins[i]
            if op == "s_barrier" or op.startswith("s_cbranch") or op == "s_branch" or (op == "s_waitcnt" and "vmcnt" in a):
                break
            if op.startswith("global_load"):
                last, burst = i, burst + 1
        waits = sum(1 for op, a in head if op == "s_waitcnt" and "lgkmcnt" in a)
        rcp = any(op.startswith("v_rcp_f32") for op, _ in head)
        # kernarg pointer: s[0:1] without preload, s[0:1] as well with it (the preloaded SGPRs follow it)
        state = None
        if "estep" in name:
            other = [i for i, (op, a) in enumerate(ins) if op.startswith("s_load") and not re.search(r"s\[0:1\],", a)]
            if other:
                w = next((j for j in range(other[0], len(ins)) if ins[j][0] == "s_waitcnt" and "lgkmcnt" in ins[j][1]), None)
                state = first < other[0] and w is not None and first < w
        # the lab builds: is the wall clock read before anything is asked for or waited for?
        clock = next((i for i, (op, _) in enumerate(ins) if op == "s_memrealtime"), None)
        early = next((i for i, (op, _) in enumerate(ins) if op.startswith("s_load") or op == "s_waitcnt"), len(ins))
        stamp_first = clock is not None and clock < early
        # the kernel's end (wave-tile M-step): phase C from its first LDS read to the last gradient store, and what
        # runs behind the workgroup's last barrier
        nt = [i for i, (op, a) in enumerate(ins) if op.endswith("_store_dwordx4") and re.search(r"\bnt\b", a)]
        phase_c = flat_c = None
        if nt and "mstep_wave" in name:
            k = nt[0]
            # (back to phase B's last LDS write or the hold's loop; the stores of a form that is not EXACT sit in
            #  branches of their own, so a branch does not end the stretch)
            while k > 0 and not (ins[k - 1][0].startswith("ds_write") or ins[k - 1][0] in ("s_sleep", "s_barrier")):
                k -= 1
            reads = [i for i in range(k, nt[0]) if ins[i][0] == "ds_read_b128"]
            if reads:
                phase_c = nt[-1] - reads[0] + 1
                flat_c = sum(1 for op, _ in ins[reads[0]:nt[-1] + 1] if op.startswith("flat_"))
        bars = [i for i, (op, _) in enumerate(ins) if op == "s_barrier"]
        tail = None
        if bars:
            end = next((i for i in range(bars[-1], len(ins)) if ins[i][0] == "s_endpgm"), None)
            tail = None if end is None else end - bars[-1]
        s = sets.get(name, {})
        vg, ag = s.get("num_vgpr", 0), s.get("num_agpr", 0)
        alloc = max((vg + ag + 7) // 8 * 8, 8)
        rows[name] = dict(phase_c=phase_c, flat_c=flat_c, tail=tail, preload=preload, instr=first, last=last, burst=burst, waits=waits, rcp=rcp, state=state, stamp_first=stamp_first,
                          vgpr=vg + ag,
                          sgpr=int(d.get("next_free_sgpr", s.get("numbered_sgpr", 0))),
                          scratch=s.get("private_seg_size", int(d.get("private_segment_fixed_size", 0))),
                          lds=int(d.get("group_segment_fixed_size", 0)), waves=min(8, 512 // alloc))
    dm = demangle(list(rows))
    return {dm[n]: r for n, r in rows.items()}


def fmt(r):
    if r is None:
        return "(no such kernel)"
    st = "-" if r["state"] is None else ("yes" if r["state"] else "NO")
    end = ""
    if r["phase_c"] is not None:
        end = f"  phase C {r['phase_c']:3d} ({r['flat_c']} flat)  behind last barrier {r['tail']:3d}"
    return (f"preload {r['preload']:2d}  instr {r['instr']:4d}  last {r['last']:4d} ({r['burst']} loads)  waits {r['waits']}  rcp {'YES' if r['rcp'] else 'no':3s}  "
            f"state {st:3s}  vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} scratch {r['scratch']} lds {r['lds']:5d} waves {r['waves']}" + end)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("sources", nargs="*", default=DEFAULT)
    ap.add_argument("--against", help="another checkout of the repository to compare with")
    ap.add_argument("--kernel", default=None, help="regular expression on the demangled kernel name")
    ap.add_argument("--all", action="store_true", help="every kernel of the sources")
    ap.add_argument("--stamps", action="store_true", help="check the entry stamp of the lab builds as well")
    a = ap.parse_args()
    pat = re.compile(a.kernel if a.kernel else (".*" if a.all else BENCH))
    bad = 0
    for src in a.sources:
        new = analyse(compile_isa(ROOT, src))
        old = analyse(compile_isa(os.path.abspath(a.against), src)) if a.against else None
        print(f"== {src}")
        for k in sorted(new):
            if not pat.search(k):
                continue
            print(k)
            if old is not None:
                print("   other:", fmt(old.get(k)))
            print("   this: ", fmt(new[k]))
            r = new[k]
            if old is not None and old.get(k) is not None:
                o = old[k]
                if (r["scratch"] > 0 and o["scratch"] == 0) or r["waves"] < o["waves"]:
                    print("   WORSE than the other checkout: scratch", o["scratch"], "->", r["scratch"], " waves",
                          o["waves"], "->", r["waves"])
                    bad += 1
            if re.search(BENCH, k):
                ok = r["preload"] > 0 and r["waits"] == 0 and not r["rcp"] and r["state"] is not False
                res_ok = r["scratch"] == 0 and (r["vgpr"] <= 168 if "estep" in k else r["waves"] >= 4)
                print("   bench instantiation: entry rules", "ok" if ok else "FAIL", " resource bounds", "ok" if res_ok else "FAIL")
                bad += 0 if ok and res_ok else 1
        flag = STAMP_FLAG.get(os.path.basename(src))
        if a.stamps and flag:
            lab = analyse(compile_isa(ROOT, src, [flag]))
            for k in sorted(lab):
                if re.search(BENCH, k):
                    print(f"{k} with {flag}: s_memrealtime before every s_load / s_waitcnt:",
                          "yes" if lab[k]["stamp_first"] else "NO")
                    bad += 0 if lab[k]["stamp_first"] else 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
