#!/usr/bin/env python3
"""Mint tests/golden/switch_words_g96.npz: 24 switch words on the oracle (tests/switch_words.py: set A, the word set
before the flux-correction year; set B, the word set after a flux-correction year under word 0), each 1 + 1 years at
680 ppm on the synthetic 96x48 workload with abi.default_params(ipx=95, ipy=38).  CPU only; about three minutes.

Everything comes from oracle/greb_oracle.c, this project's own restatement; nothing of the reference is read.  That the
restatement with its branches keyed on switch bits is still the upstream variant for the ten pinned experiments is what
tests/test_logexp_cpu.py shows, unchanged.

Arrays, one row per case in the order of switch_words.CASES (data only):

  case_set  [24] 'a' / 'b'          case_word [24] the switch word
  field_index [24][5]               the five fields of the last scenario month: which of the distinct fields below
  fields_byteplanes [4][U*48*96]    the U distinct ones among those 120 fields, float32 as byte planes (switch_words.pack_fields)
  means     [24][12][5] float64     field mean of every scenario month and variable
  yearly    [24][2][2]  float32     the two console values of the flux-correction year and of the scenario year
  sha256    [24][32]    uint8       of the scenario year's monthly array [12][5][48][96]
  noise     [24][5]     float64     the yardstick: the largest monthly RMS per variable between the oracle and THE SAME SOURCE
                                    built with -ffp-contract=fast -mfma (made here in a temporary directory, never kept)

The noise table also goes into profiles/switch_words_numbers.txt (section 1; later sections of that file are kept).
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import switch_words as SW  # noqa: E402
from greb_climate_model_amd import abi, workload  # noqa: E402
from oracle import oracle as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
NUMBERS = os.path.join(ROOT, "profiles", "switch_words_numbers.txt")
CONTRACTED = ["-O3", "-ffp-contract=fast", "-mfma", "-fno-fast-math", "-fPIC", "-std=c11"]


def contracted_oracle(tmp: str) -> str:
    so = os.path.join(tmp, "liboracle_greb_contracted.so")
    subprocess.run(["gcc", *CONTRACTED, "-shared", "-o", so, os.path.join(ROOT, "oracle", "greb_oracle.c"), "-lm"], check=True)
    return so


def numbers_text(noise) -> str:
    tol = np.asarray(SW.TOL)
    lines = ["# Switch words against the oracle (tests/switch_words.py; tests/test_switch_words_cpu.py, tests/test_gpu_switch_words.py).",
             "# 96x48, synthetic workload, default_params(ipx=95, ipy=38), 1 flux-correction year + 1 scenario year at 680 ppm.",
             "#",
             "# 1. The oracle's own sensitivity to contraction (tests/golden/make_golden_switch_words.py): the largest monthly RMS per",
             "#    variable between oracle/greb_oracle.c as built (-ffp-contract=off) and the same source built with",
             "#    " + " ".join(CONTRACTED) + ", in units of TOL = " + repr(SW.TOL) + ".",
             "#    The bar of the GPU tests is max(TOL, 3 x this) per case and variable.",
             "#",
             "#  set word   " + "  ".join(f"{v:>8s}" for v in SW.VARS) + "    bar / TOL where it is above 1"]
    for (s, w), row in zip(SW.CASES, noise):
        u = row / tol
        over = "  ".join(f"{v} {3 * x:.2f}" for v, x in zip(SW.VARS, u) if 3 * x > 1)
        lines.append(f"   {s}   0x{w:02x}   " + "  ".join(f"{x:8.3f}" for x in u) + ("    " + over if over else ""))
    lines.append("   worst      " + "  ".join(f"{x:8.3f}" for x in (noise / tol).max(0)))
    lines.append("#")
    return "\n".join(lines) + "\n"


def main():
    O.build(ref=False)
    inp, params = workload.make_inputs(), abi.default_params(ipx=95, ipy=38)
    n = len(SW.CASES)
    last = np.empty((n, 5, inp.ny, inp.nx), np.float32)
    means, yearly = np.empty((n, 12, 5), np.float64), np.empty((n, 2, 2), np.float32)
    sha, noise = np.empty((n, 32), np.uint8), np.empty((n, 5), np.float64)
    with tempfile.TemporaryDirectory() as tmp:
        so, plain = contracted_oracle(tmp), O.ORACLE_SO
        for i, (which, word) in enumerate(SW.CASES):
            mon, yr = SW.oracle_case(O, inp, params, which, word)
            O.ORACLE_SO = so
            try:
                mon_c, _ = SW.oracle_case(O, inp, params, which, word)
            finally:
                O.ORACLE_SO = plain
            assert np.isfinite(mon).all() and np.isfinite(mon_c).all() and np.isfinite(yr).all(), (which, hex(word))
            mon = mon[0]
            d = mon.astype(np.float64) - mon_c[0]
            noise[i] = np.sqrt((d * d).mean(axis=(2, 3))).max(axis=0)
            last[i], yearly[i] = mon[-1], yr
            means[i] = mon.astype(np.float64).mean(axis=(2, 3))
            sha[i] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(mon).tobytes()).digest(), np.uint8)
            print(f"{which} 0x{word:02x}  noise / TOL " + " ".join(f"{x:.3f}" for x in noise[i] / np.asarray(SW.TOL)), flush=True)
    planes, index = SW.pack_fields(last)
    np.savez_compressed(os.path.join(OUT, SW.FIXTURE), case_set=np.asarray([s for s, _ in SW.CASES]),
                        case_word=np.asarray([w for _, w in SW.CASES], np.int32), fields_byteplanes=planes, field_index=index,
                        means=means, yearly=yearly, sha256=sha, noise=noise)
    mp = os.path.join(OUT, "MANIFEST.json")
    with open(mp) as f:
        manifest = json.load(f)
    manifest["items"]["switch_words_g96"] = {
        "recipe": "tests/golden/make_golden_switch_words.py", "source": "oracle/greb_oracle.c (nothing of the reference is read)",
        "time_flux": 1, "time_scnr": 1, "co2_ppm": SW.CO2, "ipx": 95, "ipy": 38,
        "set_a_own_spin_up": [f"0x{w:02x}" for w in SW.SET_A], "set_b_shared_spin_up": [f"0x{w:02x}" for w in SW.SET_B],
        "noise_build": " ".join(CONTRACTED), "noise_over_tol_worst": [float(f"{x:.3f}") for x in (noise / np.asarray(SW.TOL)).max(0)]}
    with open(mp, "w") as f:
        json.dump(manifest, f, indent=1)
    rest = ""
    if os.path.exists(NUMBERS):
        text = open(NUMBERS).read()
        at = text.find("# 2. ")
        rest = text[at:] if at >= 0 else ""
    with open(NUMBERS, "w") as f:
        f.write(numbers_text(noise) + rest)
    print(f"wrote {SW.FIXTURE} ({os.path.getsize(os.path.join(OUT, SW.FIXTURE))} bytes), updated MANIFEST.json and {os.path.relpath(NUMBERS, ROOT)}")


if __name__ == "__main__":
    main()
