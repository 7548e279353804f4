#!/usr/bin/env python3
"""WHEN a perturbed-physics ensemble passes 1.5 K and 2 K, and when September's albedo falls to 0.4, from ONE engine that
hands back only the crossing maps of its members (Engine.run_cross, csrc/greb_cross.hip).

  python tools/run_crossing.py [pairs] [years] [--compare] [--passes N] [--kernel-timing]

Members 0 ... pairs-1 are ensemble.perturbed_physics members at constant CO2 (340 ppm), members pairs ... 2 pairs - 1 the
same physics under CO2 rising by 1 % per year (defaults: 256 pairs, 70 years).  Events: the annual-mean Tsurf response
(member minus its control) >= 1.5 K and >= 2 K, and September's albedo (variable 4) <= 0.4.  Runs 1 flux-correction year,
then `years` scenario years, and prints one JSON line: per event, by the end of every decade, the median and the 5-95 %
range across the rising members of the area-weighted share of the globe that has crossed (FIRST), the share where it holds
to the end (STAY), the bytes returned against those of Engine.run, and the ensemble-years/s of the run_cross call (--passes
timed calls after one untimed).
--compare also runs Engine.run over the same years, the two legs alternating, prints the same shares from its records
through cross.reference, and asserts equal products on a handful of pairs.
--kernel-timing times the update kernel alone on a synthetic 60-record year of 512 members with 4 events on 2 variables
(median of 20 launches of a year k > 0), states the bytes it moves -- the months read, the state words read and written --
over that time, and times clim.add_year_dev on the same data."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shares(first, stay, area, decades):
    """first, stay [members][ny][nx] of one event -> per decade's last year d the crossed share of each member's globe."""
    out = {}
    for d in decades:
        s = (((first >= 0) & (first <= d)) * area).sum(axis=(1, 2))
        out[f"by_year_{d}"] = {"median": round(float(np.median(s)), 4), "p05": round(float(np.percentile(s, 5)), 4),
                               "p95": round(float(np.percentile(s, 95)), 4)}
    held = ((stay >= 0) * area).sum(axis=(1, 2))
    out["holds_to_the_end"] = {"median": round(float(np.median(held)), 4), "p05": round(float(np.percentile(held, 5)), 4),
                               "p95": round(float(np.percentile(held, 95)), 4)}
    return out


def kernel_timing(nx, ny, reps=20):
    import torch
    from greb_climate_model_amd import build, clim, codesha, cross
    M, U = 512, 256

    def timed(fn):
        fn(); torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record()
        for i in range(reps):
            fn(); ev[i + 1].record()
        torch.cuda.synchronize()
        return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]))

    x = torch.rand((M, 12, 5, ny, nx), dtype=torch.float32, device="cuda") * 90.0 + 220.0
    events = [cross.Event(0, cross.ANN, 1.5, rel=True), cross.Event(0, cross.ANN, 2.0, rel=True), cross.Event(4, cross.SEP, 250.0, dir=-1),
              cross.Event(4, cross.MAR, 280.0)]
    control = [-1] * U + list(range(U))
    plan = cross.Plan(nx, ny, M, events, control=control, what=cross.MAPS)
    cross.add_year_dev(plan, x, 0)
    k = [0]

    def update():
        k[0] += 1
        cross.add_year_dev(plan, x, k[0])

    ms = timed(update)
    cross.finish_dev(plan, k[0] + 1)
    torch.cuda.synchronize()
    plan.close()
    np_ = ny * nx
    months_own, months_ctl = 12 + 2, 12                            # variable 0: ANN, of the member and of its control; variable 4: Mar, Sep
    records = (M * months_own + U * months_ctl) * np_ * 4
    state = M * len(events) * np_ * 6 * 4 * 2                      # six words, read and written
    cplan = clim.Plan(nx, ny, M, what=1)
    clim.add_year_dev(cplan, x, 0)
    ck = [0]

    def cadd():
        ck[0] += 1
        clim.add_year_dev(cplan, x, ck[0])

    cms = timed(cadd)
    clim.finish_dev(cplan, ck[0] + 1)
    torch.cuda.synchronize()
    cplan.close()
    cbytes = M * 60 * np_ * (4 + 16)                               # the year read, the fp64 sums read and written
    return {"members": M, "events": 4, "variables": 2, "update_ms": round(ms, 4), "record_bytes": records, "state_bytes": state,
            "bytes_per_s": round((records + state) / ms * 1e3, 0), "clim_add_year_ms": round(cms, 4), "clim_bytes": cbytes,
            "clim_bytes_per_s": round(cbytes / cms * 1e3, 0),
            "code": {n: codesha.record(build.LIB, n) for n in ("cross_update_kernel", "cross_fraction_kernel", "cross_finish_kernel")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pairs", type=int, nargs="?", default=256)
    ap.add_argument("years", type=int, nargs="?", default=70)
    ap.add_argument("--compare", action="store_true", help="also run Engine.run: the same shares from cross.reference, equal products")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--kernel-timing", action="store_true", help="also time the update kernel alone")
    args = ap.parse_args()
    import torch
    from greb_climate_model_amd import abi, cross, diag, engine, ensemble, workload

    pairs, Y = args.pairs, args.years
    M = 2 * pairs
    inp = workload.make_inputs()
    nx, ny = inp.nx, inp.ny
    p = abi.default_params(ipx=95, ipy=38)
    ov = ensemble.perturbed_physics(pairs, p)
    overrides = [{k: float(ov[m % pairs, j]) for j, k in enumerate(ensemble.PERTURBED)} for m in range(M)]
    control, group = list(range(pairs)) * 2, [-1] * pairs + [0] * pairs
    events = [cross.Event(0, cross.ANN, 1.5, rel=True), cross.Event(0, cross.ANN, 2.0, rel=True), cross.Event(4, cross.SEP, 0.4, dir=-1)]
    names = ["tsurf_response_ge_1.5K", "tsurf_response_ge_2K", "september_albedo_le_0.4"]
    plan = cross.Plan(nx, ny, M, events, control=control, group=group)
    rise = np.float32(340.0) * np.float32(1.01) ** np.arange(1, Y + 1, dtype=np.float32)
    co2 = np.concatenate([np.full((pairs, Y), 340.0, np.float32), np.repeat(rise[None, :], pairs, axis=0)]).astype(np.float32)
    w = np.cos(np.deg2rad(np.asarray(diag.latitudes(ny), np.float64)))[:, None] * np.ones((ny, nx))
    area = w / w.sum()
    decades = sorted({d for d in range(9, Y, 10)} | {Y - 1})
    e = engine.Engine(inp, p, n_members=M, overrides=overrides)
    e.flux_correction(1)
    start = [e.state(m) for m in range(M)]  # every timed call starts from the spun-up state

    legs = {"run_cross": lambda: e.run_cross(Y, co2, plan)}
    if args.compare:  # the path run_cross replaces
        legs = {"run": lambda: e.run(Y, co2), **legs}
    times, last = {k: [] for k in legs}, {}
    for i in range(1 + max(1, args.passes)):  # the legs alternate; the first call of each pays for allocations and code loading
        for k, fn in legs.items():
            for m in range(M):
                e.set_corrections(None, start[m], member=m)
            last[k] = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = fn()
            torch.cuda.synchronize()
            if i > 0:
                times[k].append(time.perf_counter() - t0)

    def rate(k):
        r = [M * Y / t for t in times[k]]
        return {"seconds": [round(t, 4) for t in times[k]], "ensemble_years_per_s": [round(x, 1) for x in r],
                "mean": round(float(np.mean(r)), 1), "spread": round(max(r) - min(r), 1)}

    res = last["run_cross"]
    delivered = sum(getattr(res, n).nbytes for n in cross.PRODUCTS)
    out = {"grid": [nx, ny], "members": M, "pairs": pairs, "years": Y, "plan": plan.describe(),
           "crossed_share_of_the_globe": {n: shares(res.first[pairs:, i], res.stay[pairs:, i], area, decades) for i, n in enumerate(names)},
           "members_above_at_the_end_global_mean": {n: round(float((res.fraction[-1, 0, i] * area).sum()), 4) for i, n in enumerate(names)},
           "run_cross": rate("run_cross"), "bytes_delivered": int(delivered),
           "monthly_bytes_of_the_run": int(M) * Y * 12 * 5 * ny * nx * 4}
    if args.compare:
        mon, yearly = last["run"]
        some = sorted({0, 1, pairs // 2, pairs - 1} & set(range(pairs)))
        rows = some + [pairs + j for j in some]                       # the controls in front, as in the run
        k = len(some)
        x = np.ascontiguousarray(np.moveaxis(mon[rows], 1, 0))
        ref = cross.reference(x, events, list(range(k)) * 2, [-1] * k + [0] * k)
        differ = 0
        for n in cross.PRODUCTS[:6]:
            got, want = np.ascontiguousarray(getattr(res, n)[rows]), getattr(ref, n)
            differ += int((got.view(np.uint32) != want.view(np.uint32)).sum())
        if k == pairs:  # the group is whole: the exceedance probabilities too
            differ += int((res.fraction.view(np.uint32) != ref.fraction.view(np.uint32)).sum())
        out["compared_pairs"] = some
        out["values_that_differ_from_the_reference"] = differ
        out["reference_crossed_share_of_the_globe"] = {n: shares(ref.first[k:, i], ref.stay[k:, i], area, decades) for i, n in enumerate(names)}
        out["equal_products"] = differ == 0 and bool(np.array_equal(yearly.view(np.uint32), res.yearly.view(np.uint32)))
        out["run"] = rate("run")
        # not slower than the path it replaces, allowing three times that leg's run-to-run spread
        out["run_cross_minus_run"] = round(out["run_cross"]["mean"] - out["run"]["mean"], 1)
        out["not_slower_than_run"] = bool(out["run_cross"]["mean"] >= out["run"]["mean"] - 3 * out["run"]["spread"])
    if args.kernel_timing:
        out["kernel_timing"] = kernel_timing(nx, ny)
        yr = M / out["run_cross"]["mean"] * 1e3  # ms of a model year of this ensemble inside run_cross
        out["kernel_timing"]["share_of_a_model_year"] = round(out["kernel_timing"]["update_ms"] / yr, 4)
    out["describe"] = e.describe()
    e.close(); plan.close()
    print(json.dumps(out))
    if args.compare:
        assert out["equal_products"], "run_cross differs from cross.reference of Engine.run's records"


if __name__ == "__main__":
    main()
