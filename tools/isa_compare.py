#!/usr/bin/env python3
"""Instruction-by-instruction comparison of kernels between two builds of libgreb_hip.so, and their register table.

  python tools/isa_compare.py PARENT.so [BRANCH.so] [--pattern member_kernel --pattern physics_step_kernel] [--drop-last N]

Runs without a GPU: the gfx950 code objects are taken out of both libraries (codesha.gfx950_code_objects) and disassembled
with llvm-objdump.  A kernel of the branch is matched to the parent's kernel of the same demangled name; where the branch
added trailing template parameters, --drop-last N strips the last N of them (all `false`) before matching.  Branch targets
and pc-relative literals are compared as written, so a kernel whose instructions are the parent's prints "identical" or
lists the few that differ; a differing instruction whose mnemonic is floating-point arithmetic is flagged "FP".
Then, for every matching kernel of the branch: VGPRs, SGPRs, scratch bytes and spill counts from the code object's notes."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from greb_climate_model_amd import build, codesha  # noqa: E402

LLVM = "/opt/rocm/lib/llvm/bin"
FP = re.compile(r"^v_(pk_)?(add|sub|subrev|mul|fma|fmac|mac|mad|div|rcp|rsq|sqrt|exp|log|min|max|ldexp|frexp|trunc|floor|ceil|rndne|cvt|fract)\w*_(f16|f32|f64|bf16)")


def tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else name


def pretty(mangled):
    """_ZN4greb13member_kernelILb0ELb1EEEv... -> member_kernel<false, true> (the kernels compared here take bools only)"""
    m = re.match(r"^_ZN4greb\d+(\w+?)I((?:Lb[01]E)+)E", mangled)
    if not m:
        return mangled
    return m.group(1) + "<" + ", ".join("true" if b == "1" else "false" for b in re.findall(r"Lb([01])E", m.group(2))) + ">"


def kernels(lib, patterns):
    """{demangled name: (instructions, notes)} of the kernels whose name contains one of `patterns`."""
    out = {}
    with tempfile.TemporaryDirectory(prefix="greb_isa_") as d:
        for i, co in enumerate(codesha.gfx950_code_objects(lib)):
            path = os.path.join(d, f"co{i}.co")
            open(path, "wb").write(co)
            txt = subprocess.run([tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", path],
                                 check=True, capture_output=True, text=True).stdout
            notes = subprocess.run([tool("llvm-readelf"), "--notes", path], check=True, capture_output=True, text=True).stdout
            meta = {}
            for blk in re.split(r"\n\s+- \.", notes):
                sym = re.search(r"\.symbol:\s+(\S+)\.kd", blk)
                if sym and ".vgpr_count" in blk:
                    meta[sym.group(1)] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                                          for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count",
                                                    "sgpr_spill_count")}
            meta = {pretty(n): v for n, v in meta.items()}
            cur = None
            for line in txt.splitlines():
                m = re.match(r"^<(.*)>:\s*$", line)
                if m:
                    name = pretty(m.group(1))
                    cur = None
                    if any(p in name for p in patterns) and not name.startswith("__"):
                        cur = out.setdefault(name, ([], meta.get(name, {})))[0]
                    continue
                if cur is not None and line.strip():
                    cur.append(re.sub(r"\s+", " ", line.split("//")[0].strip()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch", nargs="?", default=build.LIB)
    ap.add_argument("--pattern", action="append")
    ap.add_argument("--drop-last", type=int, default=0)
    a = ap.parse_args()
    pats = a.pattern or ["member_kernel<", "physics_step_kernel<"]
    old, new = kernels(a.parent, pats), kernels(a.branch, pats)
    n_diff = n_fp = 0
    for name in sorted(new):
        key = name
        for _ in range(a.drop_last):
            key = re.sub(r", false>$", ">", key)
        if key == name and a.drop_last or key not in old:
            continue
        x, y = old[key][0], new[name][0]
        if len(x) != len(y):
            print(f"{name}: {len(x)} -> {len(y)} instructions: NOT the parent's code")
            n_diff += 1
            continue
        d = [(i, p, q) for i, (p, q) in enumerate(zip(x, y)) if p != q]
        print(f"{name}: {len(y)} instructions, " + ("identical" if not d else f"{len(d)} differ"))
        for i, p, q in d:
            fp = bool(FP.match(p) or FP.match(q))
            n_fp += fp
            print(f"    [{i}] {p}   ->   {q}" + ("   FP" if fp else ""))
        n_diff += bool(d)
    print(f"\n{'kernel':84s} VGPR SGPR scratch vgpr_spill sgpr_spill")
    for name in sorted(new):
        m = new[name][1]
        if m:
            print(f"{name:84s} {m['vgpr_count']:4d} {m['sgpr_count']:4d} {m['private_segment_fixed_size']:7d} {m['vgpr_spill_count']:10d} "
                  f"{m['sgpr_spill_count']:10d}")
    print(f"\nkernels with differing instructions: {n_diff}; floating-point instructions among the differences: {n_fp}")
    return 1 if n_fp else 0


if __name__ == "__main__":
    sys.exit(main())
