#!/usr/bin/env python3
"""A CO2-sweep ensemble that hands back only the regional means of its net fluxes: the surface and the atmospheric net
flux (budget.SURFACE_NET, budget.ATMOS_NET: the right-hand sides of src/greb.f90:258 and :260) formed from the budget
terms and reduced on the device, year by year (Engine.run_diag(records=budget.combo(...)), greb_engine_run_budget_diag).

  python tools/run_fluxes.py [members] [years] [--compare] [--passes N]

Runs 1 flux-correction year, then `years` scenario years at 96x48 (default 512 members, 5 years; member m holds CO2
constant at its level of the 280 ... 1120 ppm sweep).  What leaves the device per member and year is [12][2][9] floats:
the monthly means of the two fluxes over the globe and the eight standard regions (diag.standard_regions).  Prints one
JSON line: for the lowest and the highest member the annual means of the last year (W/m2), the bytes that left the device
beside what the full budget records of the same run would take, and the ensemble-years/s of --passes timed calls after
one untimed.

--compare: also the same numbers made on the host from Engine.run_budget's full records for the first members (at most
four) -- budget.combine_reference, then diag.reduce_reference in fp64 -- under "compare": "device" and "host"
[members][years][12][2][9], and "host_abs", the same weighted means of |x|, which bound the rounding of a sum that
cancels (tests/test_gpu_budget_reduced.py holds the two to each other)."""
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
    ap.add_argument("years", type=int, nargs="?", default=5)
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--compare", action="store_true")
    args = ap.parse_args()
    from greb_climate_model_amd import abi, budget, diag, engine, ensemble, workload
    nx, ny = 96, 48
    M, Y = args.members, args.years
    inp = workload.make_inputs(nx, ny)
    p = abi.default_params(ipx=nx - 1, ipy=38)
    co2 = np.repeat(ensemble.co2_sweep(M)[:, None], Y, axis=1).astype(np.float32)
    cb = budget.combo({"surface_net": budget.SURFACE_NET, "atmos_net": budget.ATMOS_NET})
    regions = diag.standard_regions(inp)
    plan = diag.Plan(nx, ny, regions, n_vars=len(cb.names))
    e = engine.Engine(inp, p, n_members=M)
    e.flux_correction(1)
    corr, start = e.get_corrections(0)  # every call starts from the spun-up state
    secs, res = [], None
    for i in range(1 + max(1, args.passes)):  # the first call pays for allocations and code loading
        e.set_corrections(None, start)
        t0 = time.perf_counter()
        res = e.run_diag(Y, co2, plan, abi.D_REGIONS, records=cb)
        if i > 0:
            secs.append(time.perf_counter() - t0)
    annual = diag.annual_from_monthly(res.regions)  # [M][Y][2][9]
    out = {"grid": [nx, ny], "members": M, "years": Y, "fluxes": list(res.vars), "regions": list(res.names),
           "finite": bool(np.isfinite(res.regions).all()), "members_shown": {},
           "bytes_from_device": int(res.regions.nbytes + res.yearly.nbytes),
           "bytes_of_full_budget": int(M) * Y * 12 * abi.NBUDGET * ny * nx * 4,
           "seconds": [round(s, 4) for s in secs], "ensemble_years_per_s": [round(M * Y / s, 1) for s in secs]}
    for m in sorted({0, M - 1}):
        out["members_shown"][str(m)] = {
            "co2_ppm": float(co2[m, 0]),
            "annual_mean_last_year_W_m2": {v: {r: round(float(annual[m, -1, k, j]), 4) for j, r in enumerate(res.names)}
                                           for k, v in enumerate(res.vars)}}
    if args.compare:
        k = min(M, 4)
        twin = engine.Engine(inp, p, n_members=k)
        twin.set_corrections(corr, start)
        _, bud, _ = twin.run_budget(Y, co2[:k], want_monthly=False)
        twin.close()
        x = budget.combine_reference(cb, bud)  # [k][Y][12][2][ny][nx]
        w = np.stack(list(regions.values()))
        host = diag.reduce_reference(x, w)[0]
        host_abs = diag.reduce_reference(np.abs(x), w)[0]
        out["compare"] = {"members": k, "points": nx * ny, "device": res.regions[:k].astype(np.float64).tolist(),
                          "host": host.tolist(), "host_abs": host_abs.tolist()}
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
