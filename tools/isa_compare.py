#!/usr/bin/env python3
"""Instruction-by-instruction comparison of kernels between two builds of libgreb_hip.so, and their register table.

  python tools/isa_compare.py PARENT.so [BRANCH.so] [--pattern member_kernel --pattern physics_step_kernel] [--drop-last N]

Runs without a GPU: the gfx950 code objects are taken out of both libraries (codesha.gfx950_code_objects) and disassembled
with llvm-objdump.  A kernel of the branch is matched to the parent's kernel of the same demangled name (the step kernels'
variants in one canonical form: see pretty); where the branch added trailing template parameters to another kernel,
--drop-last N strips the last N of them (all `false`) before matching.  Branch targets
are compared as written; pc-relative literals, which move with the kernel's place in the object, are counted apart.  A
kernel whose instructions are the parent's prints "identical", else the instructions that differ are listed; a differing instruction whose mnemonic is floating-point arithmetic is flagged "FP".
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
PCREL = re.compile(r"^(s_add_u32 (s\d+), \2, )0x[0-9a-f]+$")
FP = re.compile(r"^v_(pk_)?(add|sub|subrev|mul|fma|fmac|mac|mad|div|rcp|rsq|sqrt|exp|log|min|max|ldexp|frexp|trunc|floor|ceil|rndne|cvt|fract)\w*_(f16|f32|f64|bf16)")


def tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else name


VARIANT_BITS = ("FLUX", "EXP", "BUDGET", "FORCE", "BOUND")  # greb_kernels.h: kVFlux ... kVBound, bit 0 first
VARIANT_KERNELS = ("member_kernel", "physics_step_kernel")


def pretty(mangled):
    """_ZN4greb13some_kernelILb0ELb1EEEv... -> some_kernel<false, true>.  The step kernels come out in one canonical form
    whichever way the build spells their variant -- <bool STRICT, unsigned V> (ILb0ELj18EE) or, in builds before that, bools
    for STRICT, FLUX, EXP and up to three trailing BUDGET, FORCE, BOUND: member_kernel<fast, EXP|FORCE|BOUND>."""
    m = re.match(r"^_ZN4greb\d+(\w+?)I((?:Lb[01]E|Lj\d+E)+)E", mangled)
    if not m:
        return mangled
    name, args = m.group(1), re.findall(r"L([bj])(\d+)E", m.group(2))
    if name in VARIANT_KERNELS and args[0][0] == "b":
        strict, rest = args[0][1] == "1", args[1:]
        if len(rest) == 1 and rest[0][0] == "j":
            mask = int(rest[0][1])
        elif rest and all(t == "b" for t, _ in rest) and len(rest) <= len(VARIANT_BITS):
            mask = sum(1 << i for i, (_, b) in enumerate(rest) if b == "1")
        else:
            mask = None
        if mask is not None and mask < 1 << len(VARIANT_BITS):
            bits = "|".join(n for i, n in enumerate(VARIANT_BITS) if mask >> i & 1) or "0"
            return f"{name}<{'strict' if strict else 'fast'}, {bits}>"
    return name + "<" + ", ".join(("true" if v == "1" else "false") if t == "b" else v + "u" for t, v in args) + ">"


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
                if cur is not None and line.strip() and line.strip() != "...":  # (...: padding behind the section's last kernel)
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
        # the low half of a pc-relative address (s_getpc_b64, s_add_u32, s_addc_u32): it moves with the code's place in the object
        moved = [t for t in d if PCREL.match(t[1]) and PCREL.match(t[2]) and PCREL.match(t[1]).group(1) == PCREL.match(t[2]).group(1)]
        d = [t for t in d if t not in moved]
        print(f"{name}: {len(y)} instructions, " + ("identical" if not d else f"{len(d)} differ") +
              (f" ({len(moved)} pc-relative literals moved)" if moved else ""))
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
