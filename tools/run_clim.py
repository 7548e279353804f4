#!/usr/bin/env python3
"""A CO2-sweep ensemble with member 0 as the control that hands back only its climatology: multi-year monthly means,
seasonal means, trends and the responses to the control, summed on the device year by year (Engine.run_clim,
csrc/greb_clim.hip).

  python tools/run_clim.py [members] [years] [--window N] [--grid NX NY] [--compare] [--passes N] [--pass-timing]

Runs 1 flux-correction year, then `years` scenario years (default 512 members, 3 years; member m holds CO2 constant at
its level of the 280 ... 1120 ppm sweep) with one averaging period, the last --window years (default: all), and prints
one JSON line: the ensemble-years/s of the run_clim call (best of --passes timed calls after one untimed), per member
the area-weighted global mean of the annual (ANN) Tsurf response map, and the bytes delivered.  --compare also times, in
the same process on the same box, Engine.run_diag(ANNUAL) over the same years: the run whose per-year annual maps a host
would otherwise average.  --pass-timing times the add-year pass alone (with and without the trend sums) on a year of
synthetic records of the same ensemble, beside torch's device-to-device copy rate taken in the same session."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pass_timing(M, nx, ny, reps=20):
    """ms and GB/s of clim_add_year_kernel (20 B per element and year, 36 B with the trend) and of a torch copy (8 B)."""
    import torch
    from greb_climate_model_amd import abi, build, clim, codesha
    x = torch.rand((M, 12, 5, ny, nx), dtype=torch.float32, device="cuda") * 90.0 + 220.0
    n = x.numel()
    out = {"elements_per_year": int(n)}

    def timed(fn):
        fn(); torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record()
        for i in range(reps):
            fn(); ev[i + 1].record()
        torch.cuda.synchronize()
        return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]))

    for name, what, nbytes in (("add_year", abi.C_MEAN, 20), ("add_year_trend", abi.C_MEAN | abi.C_TREND, 36)):
        plan = clim.Plan(nx, ny, M, what=what)
        clim.add_year_dev(plan, x, 0)
        k = [1]

        def one():
            clim.add_year_dev(plan, x, k[0]); k[0] += 1
        ms = timed(one)
        out[name] = {"ms": round(ms, 4), "bytes_per_element": nbytes, "GB_per_s": round(n * nbytes / ms / 1e6, 1)}
        clim.finish_dev(plan, k[0]); torch.cuda.synchronize()
        plan.close()
    y = torch.empty_like(x)
    ms = timed(lambda: y.copy_(x))
    out["torch_copy"] = {"ms": round(ms, 4), "bytes_per_element": 8, "GB_per_s": round(n * 8 / ms / 1e6, 1)}
    out["code"] = codesha.record(build.LIB, "clim_add_year_kernel")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("members", type=int, nargs="?", default=512)
    ap.add_argument("years", type=int, nargs="?", default=3)
    ap.add_argument("--window", type=int, default=None, help="years of the averaging period, the last of the run (default: all)")
    ap.add_argument("--grid", type=int, nargs=2, default=(96, 48), metavar=("NX", "NY"))
    ap.add_argument("--compare", action="store_true", help="also time run_diag(ANNUAL) over the same years")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--pass-timing", action="store_true", help="also time the add-year pass alone, beside a torch copy")
    args = ap.parse_args()
    import torch
    from greb_climate_model_amd import abi, clim, diag, engine, ensemble, workload

    nx, ny = args.grid
    M, Y = args.members, args.years
    W = Y if args.window is None else args.window
    if not 1 <= W <= Y:
        ap.error("--window must lie in 1 ... years")
    inp = workload.make_inputs(nx, ny)
    p = abi.default_params(ipx=nx - 1, ipy=(38 * ny) // 48)
    plan = clim.Plan(nx, ny, M, control=[-1] + [0] * (M - 1))
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

    dt, res = timed(lambda: e.run_clim(Y, co2, plan, [(Y - W, W)]))
    area = np.cos(np.deg2rad(diag.latitudes(ny)))[:, None] * np.ones((ny, nx))
    ann = res.season("ANN", response=True)[:, 0, 0].astype(np.float64)  # [member][ny][nx]: annual Tsurf minus the control's
    response = (ann * area).sum(axis=(1, 2)) / area.sum()
    products = [a for a in (res.mean, res.seasons, res.trend, res.mean_resp, res.seasons_resp) if a is not None]
    out = {"grid": [nx, ny], "members": M, "years": Y, "period": [Y - W, W], "co2_ppm": [float(c) for c in co2[:, 0]],
           "global_mean_annual_tsurf_response_K": [None if np.isnan(r) else round(float(r), 4) for r in response],
           "finite": bool(all(np.isfinite(a).all() for a in (res.mean, res.seasons, res.trend)) and  # (the control's own
                          all(np.isfinite(a[1:]).all() for a in (res.mean_resp, res.seasons_resp))),   # response is NaN)
           "run_clim": {"seconds": round(dt, 4), "ensemble_years_per_s": round(M * Y / dt, 1)},
           "bytes_delivered": int(sum(a.nbytes for a in products)),
           "monthly_bytes_of_the_run": int(M) * Y * 12 * 5 * ny * nx * 4}
    if args.compare:
        dplan = diag.Plan(nx, ny)
        dt0, ref = timed(lambda: e.run_diag(Y, co2, dplan, what=abi.D_ANNUAL))
        out["run_diag_annual"] = {"seconds": round(dt0, 4), "ensemble_years_per_s": round(M * Y / dt0, 1),
                                  "bytes_delivered": int(ref.annual.nbytes)}
        out["run_clim_over_run_diag_annual"] = round(dt / dt0, 4)
        host = ref.annual[:, Y - W:, 0].astype(np.float64).mean(axis=1)  # the same product formed on the host
        host = ((host - host[0]) * area).sum(axis=(1, 2)) / area.sum()
        out["max_abs_difference_to_host_average_K"] = float(np.abs(host[1:] - response[1:]).max()) if M > 1 else 0.0
        dplan.close()
    if args.pass_timing:
        out["pass_timing"] = pass_timing(M, nx, ny)
    out["describe"] = e.describe()
    e.close(); plan.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
