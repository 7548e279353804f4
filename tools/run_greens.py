#!/usr/bin/env python3
"""A Green's-function experiment as ONE engine with one flux correction: the response of the atmosphere to SST patches
(Engine.set_sst_tables / set_member_sst; greb_climate_model_amd/forcing.py: sst_patch_lattice).

  python tools/run_greens.py [nlat nlon] [years] [--amp K] [--compare]
  [GREB_LIB=other/libgreb_hip.so] python tools/run_greens.py --cost plain|forced|sst [members]

1 flux-correction year, then `years` scenario years (default 3) at 340 ppm of 2 + nlat * nlon members (default 4 x 8) whose
whole ocean surface is prescribed (no weight table: weight 1 everywhere):
  member 0            the control: amp 0, SST held at the climatology;
  members 1 ... n     one per patch of the lattice: climatology + amp (default 2 K) x patch;
  member n + 1        climatology + amp x the sum of all patches.
The run is run_clim over all years with the control as everyone's control (annual-mean responses made on the device), then
the same years again as run_diag(REGIONS) from the same start: the global-mean series, which must tell the same story.
Prints the sensitivity map -- annual global-mean Tair response in mK per K of patch amplitude, one number per patch, north
on top --, the additivity ratio (sum of the patch responses / response to the sum pattern), member-years/s of the run_clim
call, and one JSON line with all of it.

--compare: three of the patches again as one-member engines from the same start; their annual means must equal the
ensemble's members bit for bit (exit status 1 otherwise).

--cost: what the hook costs, one kind of launch per process so that two builds of the library can alternate (GREB_LIB): the
timing of tools/run_forcing.py --cost -- `members` members (default 512), one scenario year per call, records staying on the
device -- of a plain launch, a forced launch without any prescribed member, or a launch whose members are all prescribed
(anomaly, weight and season tables).  profiles/sst_cost.txt is made of these lines."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CO2 = 340.0


def global_mean(field, ny):
    """[..][ny][nx] -> [..]: area-weighted mean in fp64."""
    lat = (np.arange(ny, dtype=np.float64) + 0.5) * 180.0 / ny - 90.0
    w = np.cos(np.deg2rad(lat))
    return (np.asarray(field, np.float64).mean(axis=-1) * w).sum(axis=-1) / w.sum()


def cost(members, which):
    """One JSON line: member-years/s of one scenario year per call, 96x48, records staying on the device, `members` members,
    four timed calls after a first one that pays for allocations and code loading."""
    import torch
    from greb_climate_model_amd import abi, engine, ensemble, forcing, workload
    if os.environ.get("GREB_LIB"):  # another build of the library (the parent commit's: the forced launch before this hook)
        engine._lib_path = os.path.abspath(os.environ["GREB_LIB"])
    inp = workload.make_inputs()
    p = abi.default_params(ipx=95, ipy=38)
    M = members
    co2 = ensemble.co2_sweep(M)[:, None].astype(np.float32)
    e = engine.Engine(inp, p, n_members=M)
    if which == "forced":  # tools/run_forcing.py --cost's forced members; no prescribed member
        _, space, season = forcing.partial_co2_patterns(inp)
        e.set_forcing_tables(space, season, forcing.scaled_solar(inp, 0.99)[None])
        e.set_member_forcing([{"co2_pattern": m % 8, "co2_ref": 340.0, "solar_table": 0, "solar_scale": 1.01} for m in range(M)])
    elif which == "sst":   # every member prescribed: a patch of its own where there are enough, a weight table, a season
        _, patches = forcing.sst_patch_lattice(inp, 8, 16)
        weight = np.stack([forcing.basin_weight(inp, (-60.0, 60.0, 0.0, 360.0), 10.0)] * len(patches))
        season = np.stack([np.cos(2.0 * np.pi * np.arange(abi.NSTEP_YR) / abi.NSTEP_YR).astype(np.float32)] * len(patches))
        e.set_sst_tables(patches, weight, season)
        e.set_member_sst([{"pattern": m % len(patches), "amp": 2.0} for m in range(M)])
    elif which != "plain":
        raise SystemExit("--cost: plain, forced or sst")
    e.flux_correction(1)
    _, start = e.get_corrections(0)
    mon = torch.empty((M, 1, 12, 5, inp.ny, inp.nx), dtype=torch.float32, device="cuda")
    rates = []
    for i in range(5):
        e.set_corrections(None, start)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.run(1, co2, monthly_dev_ptr=mon.data_ptr())
        torch.cuda.synchronize()
        if i > 0:
            rates.append(M / (time.perf_counter() - t0))
    family = e.describe()["kernel_family"]["scenario"]
    finite = bool(torch.isfinite(mon).all().item())
    e.close()
    print(json.dumps({"launch": which, "library": os.path.basename(engine._lib_path), "members": M, "kernel_family": family,
                      "member_years_per_s": [round(r, 1) for r in rates], "mean": round(float(np.mean(rates)), 1), "finite": finite}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="*", help="[nlat nlon] [years]; with --cost: [members]")
    ap.add_argument("--amp", type=float, default=2.0)
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--cost", default=None, metavar="LAUNCH", help="time one kind of launch: plain, forced or sst")
    args = ap.parse_args()
    if args.cost:
        cost(args.n[0] if args.n else 512, args.cost)
        return
    if len(args.n) not in (0, 1, 2, 3):
        ap.error("expected [nlat nlon] [years]")
    nlat, nlon = (args.n[0], args.n[1]) if len(args.n) >= 2 else (4, 8)
    years = args.n[2] if len(args.n) == 3 else (args.n[0] if len(args.n) == 1 else 3)

    from greb_climate_model_amd import abi, clim, diag, engine, forcing, workload
    inp = workload.make_inputs()
    p = abi.default_params(ipx=95, ipy=38)
    centres, patches = forcing.sst_patch_lattice(inp, nlat, nlon)
    n = len(patches)
    anom = np.concatenate([patches, patches.astype(np.float64).sum(axis=0, keepdims=True).astype(np.float32)])  # pattern n: the sum
    M = n + 2
    sst = [{"pattern": 0, "amp": 0.0}] + [{"pattern": k, "amp": args.amp} for k in range(n + 1)]
    co2 = np.full((M, years), CO2, np.float32)

    e = engine.Engine(inp, p, n_members=M)
    e.set_sst_tables(anom)
    e.set_member_sst(sst)
    e.flux_correction(1)
    corr, start = e.get_corrections(0)
    plan = clim.Plan(inp.nx, inp.ny, M, control=[-1] + [0] * (M - 1), what=abi.C_SEASONS | abi.C_RESPONSE)
    t0 = time.perf_counter()
    res = e.run_clim(years, co2, plan, [(0, years)])
    dt = time.perf_counter() - t0
    ann = clim.SEASONS.index("ANN")
    resp = global_mean(res.seasons_resp[1:, 0, ann, 1], inp.ny)  # [n + 1]: annual global-mean Tair response, K
    # the same years as regional series
    e.set_corrections(None, start)
    dplan = diag.Plan(inp.nx, inp.ny)
    series = e.run_diag(years, co2, dplan, abi.D_REGIONS).regions[:, :, :, 1, 0]  # [M][years][12]: global-mean Tair
    tair = diag.annual_from_monthly(series, axis=-1).mean(axis=-1)                 # [M]
    resp_diag = tair[1:] - tair[0]
    describe = e.describe()
    finite = bool(np.isfinite(res.seasons_resp[1:]).all() and np.isfinite(series).all())
    ratio = float(resp[:n].sum() / resp[n])

    status = 0
    compared = []
    if args.compare:
        for k in sorted({0, n // 2, n - 1}):
            a = engine.Engine(inp, p)
            a.set_corrections(corr, start)
            a.set_sst_tables(anom)
            a.set_member_sst([sst[1 + k]])
            aplan = clim.Plan(inp.nx, inp.ny, 1, what=abi.C_SEASONS)
            r1 = a.run_clim(years, co2[:1], aplan, [(0, years)])
            a.close(); aplan.close()
            same = bool(np.array_equal(r1.seasons[0], res.seasons[1 + k]) and np.array_equal(r1.yearly[0], res.yearly[1 + k]))
            compared.append({"patch": int(k), "bit_equal": same})
            print(f"compare: patch {k} as a one-member engine {'equals' if same else 'DIFFERS FROM'} member {1 + k} of the ensemble")
            status |= 0 if same else 1
    e.close(); plan.close(); dplan.close()

    sens = 1000.0 * resp[:n].reshape(nlat, nlon) / args.amp
    print(f"sensitivity of annual global-mean Tair to local SST, mK per K of patch amplitude ({years} years, {inp.nx}x{inp.ny}); "
          "columns: patch longitudes " + " ".join(f"{c:6.1f}" for c in centres[:nlon, 1]))
    for j in range(nlat - 1, -1, -1):
        print(f"  lat {centres[j * nlon, 0]:6.1f}: " + " ".join(f"{v:8.2f}" for v in sens[j]))
    print(f"response to the sum pattern: {resp[n]:.4f} K; sum of the patch responses: {resp[:n].sum():.4f} K")
    print(f"additivity ratio: {ratio:.4f}")
    print(f"member-years/s: {M * years / dt:.1f}")
    print(json.dumps({"grid": [inp.nx, inp.ny], "years": years, "lattice": [nlat, nlon], "amp_K": args.amp, "members": M,
                      "finite": finite, "sensitivity_mK_per_K": np.round(sens, 3).tolist(),
                      "sum_pattern_response_K": round(float(resp[n]), 5), "additivity_ratio": round(ratio, 5),
                      "largest_clim_minus_diag_response_K": float(np.abs(resp - resp_diag).max()),
                      "member_years_per_s": round(M * years / dt, 1), "compare": compared, "describe": describe}))
    if not finite or not np.isfinite(ratio):
        status |= 2
    sys.exit(status)


if __name__ == "__main__":
    main()
