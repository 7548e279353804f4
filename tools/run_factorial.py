#!/usr/bin/env python3
"""The full factorial of the eight process switches (GREB_X_*) as ONE engine: 256 members, one per compute unit of an
MI355X, each with its own switch word (engine.Engine(members=...), ensemble.switch_factorial) -- the deconstruction of
the climate response by switching processes off, in one launch per model year.

  python tools/run_factorial.py [years] [--one-by-one N]

Runs 1 flux-correction year + `years` scenario years (default 3) at 2xCO2 and prints a JSON line with member-yr/s (all
1 + years model years of all members over the wall time of flux_correction + run) and describe().  --one-by-one N
times the same work the way it had to be done before members could differ in their switches -- a one-member engine per
switch word, one after another -- for the first N words of the factorial, scaled to 256."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("years", type=int, nargs="?", default=3)
    ap.add_argument("--one-by-one", type=int, default=0, metavar="N")
    args = ap.parse_args()
    from greb_climate_model_amd import abi, engine, ensemble, workload

    inp = workload.make_inputs()
    p = abi.default_params(ipx=95, ipy=38)
    sw = ensemble.switch_factorial()
    warm = engine.Engine(inp, p)  # the first launch of a process pays for loading the code objects
    warm.flux_correction(1)
    warm.close()

    e = engine.Engine(inp, p, members=[{"switches": int(s)} for s in sw])
    out = np.empty((len(sw), args.years, 12, 5, inp.ny, inp.nx), np.float32)
    t0 = time.perf_counter()
    e.flux_correction(1)
    _, yearly = e.run(args.years, 680.0, out=out)
    dt = time.perf_counter() - t0
    res = {"members": len(sw), "years": [1, args.years], "seconds": round(dt, 4),
           "member_years_per_s": round(len(sw) * (1 + args.years) / dt, 1), "finite": bool(np.isfinite(out).all()),
           "global_mean_last_year_min_max": [round(float(yearly[:, -1, 0].min()), 3), round(float(yearly[:, -1, 0].max()), 3)],
           "describe": e.describe()}
    e.close()
    if args.one_by_one > 0:
        n = min(args.one_by_one, len(sw))
        buf = np.empty((1, args.years, 12, 5, inp.ny, inp.nx), np.float32)
        t0 = time.perf_counter()
        for s in sw[:n]:
            one = engine.Engine(inp, p)
            one.set_experiment(int(s))
            one.flux_correction(1)
            one.run(args.years, 680.0, out=buf)
            one.close()
        dt1 = (time.perf_counter() - t0) * len(sw) / n
        res["one_by_one"] = {"engines_timed": n, "seconds_scaled_to_256": round(dt1, 3),
                             "member_years_per_s": round(len(sw) * (1 + args.years) / dt1, 1),
                             "ratio": round(dt1 / dt, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
