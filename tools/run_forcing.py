#!/usr/bin/env python3
"""Partial-forcing experiments as ONE engine with one flux correction (Engine.set_forcing_tables / set_member_forcing;
greb_climate_model_amd/forcing.py).

  python tools/run_forcing.py [years]
  python tools/run_forcing.py --cost [members] [--out FILE]
  python tools/run_forcing.py --compare [--out FILE]

Default: 1 flux-correction year, then `years` scenario years (default 3) of eleven members -- control (340 ppm), global
2 x CO2 (680 ppm), the eight partial cases of forcing.partial_co2_patterns (680 ppm where the pattern's weight is 1, 340
elsewhere) and the solar constant times 1.02 at 340 ppm.  Prints one JSON line: the area-weighted annual global-mean Tsurf
response of each member against the control in the last year, the additivity residual of each complementary pair
(response A + response B - response of the global case), and member-years/s of the run call.

--cost: what forcing costs next to a plain member.  `members` members (default 512) of 96x48, one scenario year per call,
records staying on the device, alternating in one session: no member forced (the default kernels) against every member
forced with a pattern, a table and a scale; then the same pair for run_budget in STRICT arithmetic at 64 members (the one
forcing-aware kernel that takes more scratch than its twin).  Written to profiles/forcing_cost.txt (or --out).

--compare: the forced run of tests/test_gpu_forcing.py case 3 against tests/forcing_mirror.py, STRICT then FAST, two scenario
years: RMS of the monthly records per field, the console values, and the largest |engine - mirror| of the four radiative
budget terms.  Written to profiles/forcing_parity_numbers.txt (or --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def global_mean(field, ny):
    """[..][ny][nx] -> [..]: area-weighted mean in fp64."""
    lat = (np.arange(ny, dtype=np.float64) + 0.5) * 180.0 / ny - 90.0
    w = np.cos(np.deg2rad(lat))
    return (np.asarray(field, np.float64).mean(axis=-1) * w).sum(axis=-1) / w.sum()


def experiments(args):
    from greb_climate_model_amd import abi, diag, engine, forcing, workload
    inp = workload.make_inputs()
    p = abi.default_params(ipx=95, ipy=38)
    names, space, season = forcing.partial_co2_patterns(inp)
    members = ["control", "2xCO2"] + list(names) + ["solar x1.02"]
    M, Y = len(members), args.years
    co2 = np.full((M, Y), 340.0, np.float32)
    co2[1:1 + 1 + len(names)] = 680.0
    force = [{}, {}] + [{"co2_pattern": k, "co2_ref": 340.0} for k in range(len(names))] + [{"solar_scale": 1.02}]
    e = engine.Engine(inp, p, n_members=M)
    e.set_forcing_tables(space, season)
    e.set_member_forcing(force)
    e.flux_correction(1)
    t0 = time.perf_counter()
    mon, yr = e.run(Y, co2)
    dt = time.perf_counter() - t0
    ann = diag.annual_from_monthly(global_mean(mon[:, -1, :, 0], inp.ny), axis=-1)  # [M]: last year's global-mean Tsurf
    resp = ann - ann[0]
    out = {"grid": [inp.nx, inp.ny], "years": Y, "members": members, "finite": bool(np.isfinite(mon).all()),
           "global_mean_tsurf_response_K": {n: round(float(r), 4) for n, r in zip(members, resp)},
           "additivity_residual_K": {f"{names[a]} + {names[b]} - 2xCO2": round(float(resp[2 + a] + resp[2 + b] - resp[1]), 4)
                                     for a, b in forcing.PARTIAL_PAIRS},
           "member_years_per_s": round(M * Y / dt, 1), "describe": e.describe()}
    e.close()
    print(json.dumps(out))


def cost(args):
    import torch
    from greb_climate_model_amd import abi, engine, ensemble, forcing, workload
    inp = workload.make_inputs()
    p = abi.default_params(ipx=95, ipy=38)
    _, space, season = forcing.partial_co2_patterns(inp)
    solar = forcing.scaled_solar(inp, 0.99)[None]
    lines = ["# member-years/s of one scenario year per call, 96x48, records staying on the device; unforced = the default kernels,",
             "# forced = every member with a CO2 pattern (one of eight), an insolation table and a scale (tools/run_forcing.py --cost)",
             f"# device: {json.dumps(engine.device_info())}"]

    def pair(M, strict, budget, passes):
        co2 = ensemble.co2_sweep(M)[:, None].astype(np.float32)
        e = engine.Engine(inp, p, n_members=M, strict=strict)
        e.set_forcing_tables(space, season, solar)
        e.flux_correction(1)
        _, start = e.get_corrections(0)
        mon = torch.empty((M, 1, 12, 5, inp.ny, inp.nx), dtype=torch.float32, device="cuda")
        bud = torch.empty((M, 1, 12, abi.NBUDGET, inp.ny, inp.nx), dtype=torch.float32, device="cuda") if budget else None
        force = [{"co2_pattern": m % 8, "co2_ref": 340.0, "solar_table": 0, "solar_scale": 1.01} for m in range(M)]
        rates = {"unforced": [], "forced": []}
        for i in range(1 + passes):  # alternating; the first round pays for allocations and code loading
            for k in ("unforced", "forced"):
                e.set_member_forcing(force if k == "forced" else None)
                e.set_corrections(None, start)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if budget:
                    e.run_budget(1, co2, monthly_dev_ptr=mon.data_ptr(), budget_dev_ptr=bud.data_ptr())
                else:
                    e.run(1, co2, monthly_dev_ptr=mon.data_ptr())
                torch.cuda.synchronize()
                if i > 0:
                    rates[k].append(M / (time.perf_counter() - t0))
        finite = bool(torch.isfinite(mon).all().item())
        e.close()
        label = f"{'STRICT' if strict else 'FAST'} {'run_budget' if budget else 'run'} {M} members"
        for k in rates:
            lines.append(f"{label:36s} {k:9s} " + " ".join(f"{r:8.1f}" for r in rates[k]) + f"   mean {np.mean(rates[k]):8.1f}")
        lines.append(f"{label:36s} forced / unforced time {np.mean(rates['unforced']) / np.mean(rates['forced']):.4f}   finite {finite}")

    pair(args.members, False, False, 3)
    pair(64, True, True, 2)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = args.out or os.path.join(ROOT, "profiles", "forcing_cost.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write(text)


def compare(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import budget_mirror
    import forcing_mirror
    from greb_climate_model_amd import abi, engine, workload
    from oracle import oracle as O
    O.build(ref=False)
    inp = workload.make_inputs()
    p = abi.default_params(ipx=95, ipy=38)
    o = O.Oracle(inp, p)
    o.flux_correction(1)
    start = budget_mirror.MirrorStart(o)
    space, season, solar, f3 = forcing_mirror.case3(inp)
    y1 = forcing_mirror.run_year(o, start, 340.0, f3, inp.sw_solar)
    y2 = forcing_mirror.run_year(o, forcing_mirror.next_start(start, y1[2]), 680.0, f3, inp.sw_solar)
    o.close()
    want_mon, want_bud, want_yr = np.stack([y1[0], y2[0]]), np.stack([y1[1], y2[1]]), np.stack([y1[4], y2[4]])
    rms = lambda a, b: float(np.sqrt(np.mean((np.asarray(a, np.float64) - b) ** 2)))
    terms = ("sw", "LW_surf", "LWair_down", "LW_abs")
    lines = ["# forced run against tests/forcing_mirror.py, 96x48 fused member kernel, two scenario years (340, 680 ppm) from the oracle's",
             "# spun-up state: space weights {0, 0.25, 1}, season weights {0, 0.5, 1}, perturbed insolation table x 1.02, co2_ref 298",
             "# (tools/run_forcing.py --compare; the case of tests/test_gpu_forcing.py::test_forced_run_against_the_mirror)",
             f"# device: {json.dumps(engine.device_info())}"]
    for strict in (True, False):
        e = engine.Engine(inp, p, strict=strict)
        e.set_corrections(start.corr, start.state5)
        e.set_forcing_tables(space, season, solar)
        e.set_member_forcing([{"co2_pattern": 0, "co2_ref": 298.0, "solar_table": 0, "solar_scale": 1.02}])
        mon, bud, yr = e.run_budget(2, np.asarray([[340.0, 680.0]], np.float32))
        e.close()
        tag = "STRICT" if strict else "FAST"
        for y in range(2):
            lines.append(f"{tag:6s} year {y} monthly RMS   Tsurf {rms(mon[0, y, :, 0], want_mon[y, :, 0]):.3e}  Tair {rms(mon[0, y, :, 1], want_mon[y, :, 1]):.3e}  "
                         f"Tocean {rms(mon[0, y, :, 2], want_mon[y, :, 2]):.3e}  q {rms(mon[0, y, :, 3], want_mon[y, :, 3]):.3e}  "
                         f"albedo {rms(mon[0, y, :, 4], want_mon[y, :, 4]):.3e}")
            d = [float(np.abs(bud[0, y, :, abi.BUDGET_NAMES.index(t)].astype(np.float64) - want_bud[y, :, abi.BUDGET_NAMES.index(t)]).max()) for t in terms]
            lines.append(f"{tag:6s} year {y} budget max |difference|   " + "  ".join(f"{t} {x:.3e}" for t, x in zip(terms, d)))
            lines.append(f"{tag:6s} year {y} console values   engine {yr[0, y, 0]:.6f} {yr[0, y, 1]:.6f}   mirror {want_yr[y, 0]:.6f} {want_yr[y, 1]:.6f}   "
                         f"|difference| {abs(float(yr[0, y, 0]) - float(want_yr[y, 0])):.3e} {abs(float(yr[0, y, 1]) - float(want_yr[y, 1])):.3e}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = args.out or os.path.join(ROOT, "profiles", "forcing_parity_numbers.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=None, help="years (default 3), or members with --cost (default 512)")
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.compare:
        compare(args)
    elif args.cost:
        args.members = args.n or 512
        cost(args)
    else:
        args.years = args.n or 3
        experiments(args)


if __name__ == "__main__":
    main()
