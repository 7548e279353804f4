#!/usr/bin/env python3
"""A CO2-sweep ensemble with budget output: the monthly means of the thirteen flux terms of the update
(Engine.run_budget, greb_engine_run_budget; abi.BUDGET_NAMES).

  python tools/run_budget.py [members] [years] [--passes N]
  python tools/run_budget.py --compare [--out FILE]

Runs 1 flux-correction year, then `years` scenario years (default 512 members, 4 years; member m holds CO2 constant at
its level of the 280 ... 1120 ppm sweep), records staying on the device.  Prints one JSON line: for the lowest and the
highest member the area-weighted annual global means of the thirteen terms in the last year and the surface, atmosphere
and top-of-atmosphere imbalances derived from them (W/m2; the surface one excludes the flux correction TF), and the
ensemble-years/s of run_budget beside a plain run of the same engine -- alternating, --passes timed calls each after one
untimed.

--compare: the per-term largest |engine - mirror| over one scenario year at 96x48, STRICT then FAST, against
tests/budget_mirror.py (the oracle's routines stepped from Python), both from the oracle's spun-up state; written to
profiles/budget_parity_numbers.txt (or --out).  These are the numbers behind the bounds of tests/test_gpu_budget.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def global_means(bud_year, ny):
    """[..][12][13][ny][nx] (torch) -> [..][13]: area- and day-weighted annual global means, in fp64."""
    import torch
    from greb_climate_model_amd import abi
    lat = (torch.arange(ny, dtype=torch.float64, device=bud_year.device) + 0.5) * (180.0 / ny) - 90.0
    w = torch.cos(torch.deg2rad(lat))
    zonal = bud_year.double().mean(dim=-1)                               # [..][12][13][ny]
    glob = (zonal * w).sum(dim=-1) / w.sum()                             # [..][12][13]
    days = torch.tensor(abi.JDAY_MON, dtype=torch.float64, device=bud_year.device)
    return (glob * days[:, None]).sum(dim=-2) / 365.0


def imbalances(g):
    from greb_climate_model_amd import abi as a
    surf = g[a.B_SW] + g[a.B_LW_SURF] - g[a.B_LWAIR_DOWN] + g[a.B_Q_LAT] + g[a.B_Q_SENS]                  # :258 without TF
    atm = 2.0 * g[a.B_LWAIR_DOWN] - g[a.B_LW_ABS] + g[a.B_Q_LAT_AIR] - g[a.B_Q_SENS]                     # :260
    return {"surface_W_m2": surf, "atmosphere_W_m2": atm, "top_of_atmosphere_W_m2": surf + atm}


def sweep(args):
    import torch
    from greb_climate_model_amd import abi, engine, ensemble, workload
    nx, ny = 96, 48
    M, Y = args.members, args.years
    inp = workload.make_inputs(nx, ny)
    p = abi.default_params(ipx=nx - 1, ipy=38)
    co2 = np.repeat(ensemble.co2_sweep(M)[:, None], Y, axis=1).astype(np.float32)
    e = engine.Engine(inp, p, n_members=M)
    e.flux_correction(1)
    _, start = e.get_corrections(0)  # every timed call starts from the spun-up state
    mon = torch.empty((M, Y, 12, 5, ny, nx), dtype=torch.float32, device="cuda")
    bud = torch.empty((M, Y, 12, abi.NBUDGET, ny, nx), dtype=torch.float32, device="cuda")
    calls = {"run_budget": lambda: e.run_budget(Y, co2, monthly_dev_ptr=mon.data_ptr(), budget_dev_ptr=bud.data_ptr()),
             "run": lambda: e.run(Y, co2, monthly_dev_ptr=mon.data_ptr())}
    secs = {k: [] for k in calls}
    for i in range(1 + max(1, args.passes)):  # alternating; the first round pays for allocations and code loading
        for k in ("run", "run_budget"):
            e.set_corrections(None, start)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls[k]()
            torch.cuda.synchronize()
            if i > 0:
                secs[k].append(time.perf_counter() - t0)
    g = global_means(bud[:, -1], ny).cpu().numpy()  # [M][13]
    out = {"grid": [nx, ny], "members": M, "years": Y, "finite": bool(torch.isfinite(bud).all().item()), "members_shown": {}}
    for m in sorted({0, M - 1}):
        terms = {n: float(f"{g[m, i]:.6g}") for i, n in enumerate(abi.BUDGET_NAMES)}
        out["members_shown"][str(m)] = {"co2_ppm": float(co2[m, 0]), "annual_global_mean_last_year": terms,
                                        "imbalance": {k: round(float(v), 4) for k, v in imbalances(g[m]).items()}}
    for k in calls:
        out[k] = {"seconds": [round(s, 4) for s in secs[k]],
                  "ensemble_years_per_s": [round(M * Y / s, 1) for s in secs[k]]}
    out["run_budget_over_run"] = round(float(np.mean(secs["run_budget"]) / np.mean(secs["run"])), 4)
    out["describe"] = e.describe()
    e.close()
    print(json.dumps(out))


def compare(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import budget_mirror
    from greb_climate_model_amd import abi, engine, workload
    from oracle import oracle as O
    O.build(ref=False)
    inp = workload.make_inputs()
    p = abi.default_params(ipx=95, ipy=38)
    co2 = 680.0
    o = O.Oracle(inp, p)
    o.flux_correction(1)
    start = budget_mirror.MirrorStart(o)
    _, want, _ = budget_mirror.run_year(o, start, co2)
    o.close()
    lines = ["# largest |engine - mirror| of the monthly-mean budget terms, 96x48 fused member kernel, one scenario year at",
             f"# {co2:g} ppm from the oracle's spun-up state and corrections (tools/run_budget.py --compare)",
             f"# device: {json.dumps(engine.device_info())}",
             f"# {'term':>10s} {'largest |value|':>16s} {'STRICT':>12s} {'FAST':>12s}"]
    d = {}
    for strict in (True, False):
        e = engine.Engine(inp, p, strict=strict)
        e.set_corrections(start.corr, start.state5)
        _, bud, _ = e.run_budget(1, co2)
        e.close()
        d[strict] = np.abs(bud[0, 0].astype(np.float64) - want).reshape(12, abi.NBUDGET, -1).max(axis=(0, 2))
    scale = np.abs(want).reshape(12, abi.NBUDGET, -1).max(axis=(0, 2))
    for i, n in enumerate(abi.BUDGET_NAMES):
        lines.append(f"  {n:>10s} {scale[i]:16.6e} {d[True][i]:12.3e} {d[False][i]:12.3e}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("members", type=int, nargs="?", default=512)
    ap.add_argument("years", type=int, nargs="?", default=4)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "budget_parity_numbers.txt"))
    args = ap.parse_args()
    compare(args) if args.compare else sweep(args)


if __name__ == "__main__":
    main()
