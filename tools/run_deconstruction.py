#!/usr/bin/env python3
"""The ten pinned experiments of the upstream deconstruction (greb.original.model.f90 log_exp 5, 6, 8-15: process switches
AND changed boundary data) as ONE engine -- one member per experiment, one boundary set per distinct combination of
changed fields (original.run_deconstruction) -- and one by one (original.run_original, an engine per experiment).

  python tools/run_deconstruction.py [years]

Runs 1 flux-correction year + 1 control year + `years` scenario years (default 2) per experiment both ways and prints a
JSON line: member-yr/s of both (all model years of all experiments over the wall time, engine creation included) and the
largest difference between the two in any monthly record."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PINNED = (5, 6, 8, 9, 10, 11, 12, 13, 14, 15)


def main():
    years = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    from greb_climate_model_amd import engine, original, workload

    inp = workload.make_inputs()
    warm = engine.Engine(inp, original.original_params())  # the first launch of a process pays for loading the code objects
    warm.flux_correction(1)
    warm.close()
    model_years = len(PINNED) * (2 + years)
    t0 = time.perf_counter()
    together = original.run_deconstruction(inp, PINNED, 1, 1, years)
    dt = time.perf_counter() - t0
    t0 = time.perf_counter()
    alone = [original.run_original(inp, le, 1, 1, years) for le in PINNED]
    dt1 = time.perf_counter() - t0
    diff = max(float(np.abs(a.astype(np.float64) - b).max()) for x, y in zip(together, alone) for a, b in zip(x, y))
    print(json.dumps({"experiments": list(PINNED), "years": [1, 1, years],
                      "one_engine": {"seconds": round(dt, 3), "member_years_per_s": round(model_years / dt, 1)},
                      "one_by_one": {"seconds": round(dt1, 3), "member_years_per_s": round(model_years / dt1, 1)},
                      "ratio": round(dt1 / dt, 2), "largest_difference": diff,
                      "finite": bool(all(np.isfinite(a).all() for x in together for a in x))}))


if __name__ == "__main__":
    main()
