#!/usr/bin/env python3
"""An initial-condition ensemble as ONE engine with one flux correction: identical members that differ only in the seed of
their stochastic surface heat flux (Engine.set_noise_tables / set_member_noise; greb_climate_model_amd/noise.py), beside one
noise-free member -- Hasselmann's stochastic climate model: weather noise in the heat flux, integrated by the mixed layer.

  python tools/run_noise.py [members] [years] [--sigma W] [--cell X Y] [--hold H] [--compare]
  python tools/run_noise.py --cost plain|forced|noisy [members] [--cell X Y] [--hold H]

1 flux-correction year, then `years` scenario years (default 10) at 340 ppm of `members` noisy members (default 31) and one
noise-free member, the last.  sigma (default 30 W/m2) holds over ocean, a third of it over land; cell (default 2 3) and hold
(default 6 steps: three days) give the noise its scales in space and time.  The years are integrated twice from the same
start: as run_ens (the variance across the noisy members of every monthly record, made on the device) and as run_diag
(every member's annual-mean maps and global-mean series).  The scenario clock runs on between the two, so the second pass
is another realisation of the same ensemble.  Prints the ensemble standard deviation of December Tsurf (run_ens, last year) and
of annual-mean Tsurf (run_diag, last year), each as an RMS over ocean and over land; the lag-1-year autocorrelation of the
members' annual global-mean Tsurf anomalies; member-years/s of the run_ens call; and one JSON line with all of it.

--compare: the numpy mirror's numbers beside the device's -- the RMS of the heat flux N itself over ocean and over land at the
first and the last step of the run, from noise.field and from Engine.noise, which must be equal bit for bit -- and the
noise-free member again as a plain one-member engine, whose run_diag products must equal the member's bit for bit (exit
status 1 otherwise).

--cost: what the noise costs, one kind of launch per process: `members` members (default 512), one scenario year per call,
records staying on the device, three timed calls after a first one -- a plain launch, a forced launch without any noisy member
(tools/run_forcing.py --cost's members), or that forced launch with every member noisy at --cell and --hold.  One JSON line
per process.  (Not yet run on a GPU: DESIGN.md 4.2.15 has no measured cost.)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CO2 = 340.0


def area_rms(field, mask, ny):
    """RMS of [ny][nx] over the points of `mask`, area-weighted, in fp64."""
    lat = (np.arange(ny, dtype=np.float64) + 0.5) * 180.0 / ny - 90.0
    w = np.cos(np.deg2rad(lat))[:, None] * mask
    return float(np.sqrt((np.asarray(field, np.float64) ** 2 * w).sum() / w.sum()))


def tables(inp, sigma):
    return np.where(np.asarray(inp.z_topo) < 0, np.float32(sigma), np.float32(sigma / 3.0)).astype(np.float32)


def cost(members, which, cell, hold):
    import torch
    from greb_climate_model_amd import abi, engine, ensemble, forcing, noise, workload
    inp = workload.make_inputs()
    p = abi.default_params(ipx=95, ipy=38)
    M = members
    co2 = ensemble.co2_sweep(M)[:, None].astype(np.float32)
    e = engine.Engine(inp, p, n_members=M)
    if which in ("forced", "noisy"):
        _, space, season = forcing.partial_co2_patterns(inp)
        e.set_forcing_tables(space, season, forcing.scaled_solar(inp, 0.99)[None])
        e.set_member_forcing([{"co2_pattern": m % 8, "co2_ref": 340.0, "solar_table": 0, "solar_scale": 1.01} for m in range(M)])
    elif which != "plain":
        raise SystemExit("--cost: plain, forced or noisy")
    if which == "noisy":
        e.set_noise_tables(tables(inp, 30.0), None, cell, hold)
        e.set_member_noise([{"pattern": 0, "seed": s} for s in noise.seeds(M, 1)])
    e.flux_correction(1)
    _, start = e.get_corrections(0)
    mon = torch.empty((M, 1, 12, 5, inp.ny, inp.nx), dtype=torch.float32, device="cuda")
    rates = []
    for i in range(4):
        e.set_corrections(None, start)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.run(1, co2, monthly_dev_ptr=mon.data_ptr())
        torch.cuda.synchronize()
        if i > 0:
            rates.append(M / (time.perf_counter() - t0))
    d = e.describe()
    finite = bool(torch.isfinite(mon).all().item())
    e.close()
    print(json.dumps({"launch": which, "members": M, "cell": list(cell) if which == "noisy" else None, "hold": hold if which == "noisy" else None,
                      "kernel_family": d["kernel_family"]["scenario"], "noisy_members": d["noise"]["noisy_members"],
                      "member_years_per_s": [round(r, 1) for r in rates], "mean": round(float(np.mean(rates)), 1), "finite": finite}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="*", help="[members] [years]; with --cost: [members]")
    ap.add_argument("--sigma", type=float, default=30.0)
    ap.add_argument("--cell", type=int, nargs=2, default=(2, 3), metavar=("X", "Y"))
    ap.add_argument("--hold", type=int, default=6)
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--cost", default=None, metavar="LAUNCH", help="time one kind of launch: plain, forced or noisy")
    args = ap.parse_args()
    cell = tuple(args.cell)
    if args.cost:
        cost(args.n[0] if args.n else 512, args.cost, cell, args.hold)
        return
    if len(args.n) > 2:
        ap.error("expected [members] [years]")
    N = args.n[0] if args.n else 31
    years = args.n[1] if len(args.n) == 2 else 10
    if N < 2 or years < 1:
        ap.error("at least two noisy members and one year")

    from greb_climate_model_amd import abi, diag, engine, ens, noise, workload
    inp = workload.make_inputs()
    p = abi.default_params(ipx=95, ipy=38)
    ny, nx = inp.ny, inp.nx
    ocean = np.asarray(inp.z_topo) < 0
    sigma = tables(inp, args.sigma)
    seeds = noise.seeds(N, 1)
    M = N + 1
    members = [{"pattern": 0, "seed": s} for s in seeds] + [{}]
    co2 = np.full((M, years), CO2, np.float32)

    e = engine.Engine(inp, p, n_members=M)
    e.set_noise_tables(sigma, None, cell, args.hold)
    e.set_member_noise(members)
    e.flux_correction(1)
    corr, start = e.get_corrections(0)
    plan = ens.Plan(nx, ny, M, [0] * N + [-1], what=abi.S_MEAN | abi.S_VAR)
    t0 = time.perf_counter()
    res = e.run_ens(years, co2, plan)
    dt = time.perf_counter() - t0
    std_dec = np.sqrt(res.var[0, years - 1, 11, 0])            # [ny][nx]: December Tsurf of the last year
    # the same years again as annual maps and regional series: steps years * 730 ... of the clock, another realisation
    e.set_corrections(None, start)
    dplan = diag.Plan(nx, ny)
    dres = e.run_diag(years, co2, dplan, abi.D_REGIONS | abi.D_ANNUAL)
    std_ann = dres.annual[:N, years - 1, 0].astype(np.float64).std(axis=0, ddof=1)
    gm = diag.annual_from_monthly(dres.regions[:N, :, :, 0, 0], axis=-1)  # [N][years]: annual global-mean Tsurf
    anom = gm - gm.mean(axis=0, keepdims=True)
    a, b = anom[:, :-1].ravel(), anom[:, 1:].ravel()
    lag1 = float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum())) if years > 1 else float("nan")
    describe = e.describe()
    finite = bool(np.isfinite(res.var).all() and np.isfinite(dres.annual).all() and np.isfinite(dres.regions).all())

    status = 0
    compared = {}
    if args.compare:
        last = 2 * years * abi.NSTEP_YR - 1
        rows = []
        for step in (0, last):
            want = noise.field(sigma, None, cell, args.hold, seeds[0], 1.0, (step,))[0]
            got = e.noise(0, step)
            same = bool(np.array_equal(got, want))
            rows.append({"step": step, "bit_equal": same, "mirror_rms_ocean_land": [area_rms(want, ocean, ny), area_rms(want, ~ocean, ny)],
                         "device_rms_ocean_land": [area_rms(got, ocean, ny), area_rms(got, ~ocean, ny)]})
            print(f"compare: N of member 0 at step {step}: RMS over ocean / land, mirror {rows[-1]['mirror_rms_ocean_land'][0]:.4f} / "
                  f"{rows[-1]['mirror_rms_ocean_land'][1]:.4f} W/m2, device {rows[-1]['device_rms_ocean_land'][0]:.4f} / "
                  f"{rows[-1]['device_rms_ocean_land'][1]:.4f} W/m2: {'equal bit for bit' if same else 'DIFFERENT'}")
            status |= 0 if same else 1
        q = engine.Engine(inp, p)
        q.set_corrections(corr, start)
        qplan = diag.Plan(nx, ny)
        qres = q.run_diag(years, co2[:1], qplan, abi.D_REGIONS | abi.D_ANNUAL)
        family = q.describe()["kernel_family"]["scenario"]
        q.close(); qplan.close()
        same = bool(np.array_equal(qres.annual[0], dres.annual[N]) and np.array_equal(qres.regions[0], dres.regions[N]) and
                    np.array_equal(qres.yearly[0], dres.yearly[N]))
        print(f"compare: the noise-free member {'equals' if same else 'DIFFERS FROM'} a plain one-member engine ({family} kernels)")
        status |= 0 if same else 1
        compared = {"noise": rows, "plain_bit_equal": same}
    e.close(); plan.close(); dplan.close()

    so, sl = area_rms(std_dec, ocean, ny), area_rms(std_dec, ~ocean, ny)
    ao, al = area_rms(std_ann, ocean, ny), area_rms(std_ann, ~ocean, ny)
    print(f"{N} noisy members + 1 noise-free, {years} years, {nx}x{ny}, sigma {args.sigma:g} W/m2 over ocean, cell {cell}, hold {args.hold}")
    print(f"ensemble std of December Tsurf, year {years}: ocean {so:.4f} K, land {sl:.4f} K")
    print(f"ensemble std of annual-mean Tsurf, year {years}: ocean {ao:.4f} K, land {al:.4f} K")
    print(f"lag-1-year autocorrelation of the annual global-mean Tsurf: {lag1:.3f}")
    print(f"member-years/s: {M * years / dt:.1f}")
    print(json.dumps({"grid": [nx, ny], "years": years, "members": M, "noisy": N, "sigma_W_m2": args.sigma, "cell": list(cell), "hold": args.hold,
                      "finite": finite, "std_december_tsurf_K": {"ocean": round(so, 5), "land": round(sl, 5)},
                      "std_annual_tsurf_K": {"ocean": round(ao, 5), "land": round(al, 5)}, "lag1_year_autocorrelation": None if lag1 != lag1 else round(lag1, 4),
                      "member_years_per_s": round(M * years / dt, 1), "compare": compared, "describe": describe}))
    if not finite:
        status |= 2
    sys.exit(status)


if __name__ == "__main__":
    main()
