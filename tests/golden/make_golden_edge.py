#!/usr/bin/env python3
"""Golden vectors for the edge inputs (tests/edge_workload.py: z_topo == 0 on land and ocean, glacier on ocean points, a
mixed layer that stands still on warm ocean points).  BUILD CONTAINER ONLY.
Runs oracle/_ref/greb_ref with time_flux = 1, time_scnr = 1 at 680 ppm on those inputs and writes
tests/golden/edge_g96.npz: the point lists, all 12 months and the console values; asserts the oracle reproduces the
monthly output and the console values bit for bit.  (The reference program cannot take edited corrections: the year with
the humidity clamp is pinned through tests/budget_mirror.py, tests/test_edge_cpu.py.)"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import edge_workload  # noqa: E402
from greb_climate_model_amd import abi  # noqa: E402
from oracle import oracle as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def main():
    inp, pts = edge_workload.make_edge_inputs()
    mon, out, _ = O.run_reference_binary(inp, 1, 1, (680.0,))
    o = O.Oracle(inp, abi.default_params(ipx=95, ipy=38))
    yf = o.flux_correction(1)
    mo, yr = o.run(1, 680.0)
    o.close()
    same = bool(np.array_equal(mon, mo.reshape(mon.shape)))
    assert same, "oracle differs from the reference on the edge inputs"
    rows = O.parse_ref_stdout(out)
    yearly = rows[:, 2:4].astype(np.float32)
    ours = np.concatenate([yf, yr])  # (the program prints enough digits to give the fp32 values back)
    assert np.array_equal(yearly, ours), (yearly, ours)
    assert np.isfinite(mon).all()
    np.savez_compressed(os.path.join(OUT, "edge_g96.npz"), monthly=mon, yearly=yearly, **pts)
    mp = os.path.join(OUT, "MANIFEST.json")
    with open(mp) as f:
        manifest = json.load(f)
    manifest["items"]["edge_g96"] = {"time_flux": 1, "time_scnr": 1, "co2_ppm": 680.0,
                                     "inputs": "tests/edge_workload.py make_edge_inputs(), seed %d" % edge_workload.SEED,
                                     "points": {k: int(len(v)) for k, v in pts.items()}, "oracle_bit_identical": same,
                                     "sha256": hashlib.sha256(np.ascontiguousarray(mon).tobytes()).hexdigest()}
    with open(mp, "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote edge_g96.npz")


if __name__ == "__main__":
    main()
