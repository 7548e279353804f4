#!/usr/bin/env python3
"""A CO2-sweep ensemble that hands back only its diagnostics: regional means, zonal means and annual-mean maps made on
the device year by year (Engine.run_diag, csrc/greb_diag.hip) over the standard regions (diag.standard_regions).

  python tools/run_diag.py [members] [years] [--grid NX NY] [--compare] [--passes N]

Runs 1 flux-correction year, then `years` scenario years (default 512 members, 3 years; member m holds CO2 constant at
its level of the 280 ... 1120 ppm sweep) and prints one JSON line: per region the warming of the last year against the
first (annual means of Tsurf) for the lowest and the highest member, and the ensemble-years/s of the run_diag call
(best of --passes timed calls after one untimed).  --compare also times, in the same process on the same box,
Engine.run(..., monthly_dev_ptr=...) over the same years: the device-out path that delivers nothing to the host and
reduces nothing -- what the reduction and the delivery of its products cost on top of the integration."""
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
    ap.add_argument("members", type=int, nargs="?", default=512)
    ap.add_argument("years", type=int, nargs="?", default=3)
    ap.add_argument("--grid", type=int, nargs=2, default=(96, 48), metavar=("NX", "NY"))
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--passes", type=int, default=2)
    args = ap.parse_args()
    import torch
    from greb_climate_model_amd import abi, diag, engine, ensemble, workload

    nx, ny = args.grid
    M, Y = args.members, args.years
    inp = workload.make_inputs(nx, ny)
    p = abi.default_params(ipx=nx - 1, ipy=(38 * ny) // 48)
    plan = diag.Plan(nx, ny, diag.standard_regions(inp))
    co2 = np.repeat(ensemble.co2_sweep(M)[:, None], Y, axis=1).astype(np.float32)
    e = engine.Engine(inp, p, n_members=M)
    e.flux_correction(1)
    _, start = e.get_corrections(0)  # every timed call starts from the spun-up state

    def timed(fn):
        best, out = None, None
        for i in range(1 + max(1, args.passes)):  # the first call pays for allocations and code loading
            e.set_corrections(None, start)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if i > 0:
                best = dt if best is None else min(best, dt)
        return best, out

    dt, res = timed(lambda: e.run_diag(Y, co2, plan))
    ts = diag.annual_from_monthly(res.regions)[..., 0, :]  # [member][year][region]: annual-mean Tsurf
    warming = ts[:, -1] - ts[:, 0]
    out = {"grid": [nx, ny], "members": M, "years": Y, "co2_ppm": [float(co2[0, 0]), float(co2[-1, 0])],
           "warming_last_minus_first_year_K": {n: [round(float(warming[0, r]), 4), round(float(warming[-1, r]), 4)]
                                               for r, n in enumerate(res.names)},
           "finite": bool(all(np.isfinite(a).all() for a in (res.regions, res.zonal, res.annual))),
           "run_diag": {"seconds": round(dt, 4), "ensemble_years_per_s": round(M * Y / dt, 1)},
           "products_bytes_per_ensemble_year": int((res.regions.nbytes + res.zonal.nbytes + res.annual.nbytes) // Y),
           "monthly_bytes_per_ensemble_year": int(M) * 12 * 5 * ny * nx * 4}
    if args.compare:
        buf = torch.empty((M, Y, 12, 5, ny, nx), dtype=torch.float32, device="cuda")
        dt0, _ = timed(lambda: e.run(Y, co2, monthly_dev_ptr=buf.data_ptr()))
        out["run_device_out"] = {"seconds": round(dt0, 4), "ensemble_years_per_s": round(M * Y / dt0, 1)}
        out["run_diag_over_run_device_out"] = round(dt / dt0, 4)
    out["describe"] = e.describe()
    e.close(); plan.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
