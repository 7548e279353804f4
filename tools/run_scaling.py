#!/usr/bin/env python3
"""Pattern scaling of a perturbed-physics ensemble under a CO2 ramp -- the local change per degree of each member's OWN
global-mean warming -- from ONE engine that hands back only the regression maps of its members (Engine.run_reg,
csrc/greb_reg.hip).

  python tools/run_scaling.py [members] [years] [--compare] [--passes N] [--kernel-timing]

Engine members 0 ... members-1 are ensemble.perturbed_physics members at constant CO2 (340 ppm), members members ...
2 members - 1 the same physics under CO2 rising by 1 % per year (defaults: 256 members, 70 years).  Terms, each the member
minus its control: the annual mean and the four seasons of Tsurf, the annual mean of q and September's albedo.  Index: the
annual global-mean Tsurf response.  Runs 1 flux-correction year, then `years` scenario years, and prints one JSON line: per
rising member the Arctic, land and ocean means of the slope of every term (Arctic amplification, the land / ocean warming
contrast, humidity and albedo per degree), their median and 5-95 % range across the members, the index at the end, the bytes
returned against those of Engine.run, and the ensemble-years/s of the run_reg call (--passes timed calls after one untimed).
--compare also runs Engine.run over the same years followed by regress.reference on the host, the two legs alternating, with
the bytes each leg delivers, and asserts equal products on a handful of members (the mirror fed diag.reduce_dev's regional
means of their years).
--kernel-timing times regress.add_year_dev (the index pass and the update kernel) on a synthetic 60-record year of 512
members with 4 terms and with 16 terms (median of 20 calls of a year k > 0), diag.reduce_dev of the regions alone -- the
index pass but for its one tiny kernel --, and clim.add_year_dev on the same year; the update kernel's own time is given
only as the difference of the first two, a derived figure."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ["tsurf_ann", "tsurf_djf", "tsurf_mam", "tsurf_jja", "tsurf_son", "q_ann", "albedo_sep"]


def make_terms():
    from greb_climate_model_amd import cross, regress
    sels = [(0, cross.ANN), (0, cross.DJF), (0, cross.MAM), (0, cross.JJA), (0, cross.SON), (3, cross.ANN), (4, cross.SEP)]
    return [regress.Index(0, cross.ANN, 0, True)], [regress.Term(v, s, 0, True) for v, s in sels]


def regional(slope, masks):
    """slope [members][terms][ny][nx] -> {region: [members][terms]}, the area-weighted means over each mask (a NaN in a
    member's map makes its mean NaN)."""
    return {k: (slope.astype(np.float64) * w).sum(axis=(2, 3)) / w.sum() for k, w in masks.items()}


def summary(means):
    out = {}
    for region, a in means.items():
        out[region] = {n: {"median": round(float(np.median(a[:, t])), 5), "p05": round(float(np.percentile(a[:, t], 5)), 5),
                           "p95": round(float(np.percentile(a[:, t], 95)), 5)} for t, n in enumerate(NAMES)}
    return out


def kernel_timing(nx, ny, reps=20):
    import torch
    from greb_climate_model_amd import abi, build, clim, codesha, cross, diag, regress
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
    control = [-1] * U + list(range(U))
    np_ = ny * nx
    out = {"members": M}
    index, seven = make_terms()
    four = [seven[0], seven[3], seven[5], seven[6]]
    sixteen = seven + [regress.Term(v, s, 0, True) for v, s in ((1, cross.ANN), (2, cross.ANN), (4, cross.MAR), (4, cross.JUN), (4, cross.DEC),
                                                                 (3, cross.JJA), (3, cross.DJF), (1, cross.JUL), (1, cross.JAN))]
    for name, terms in (("4_terms", four), ("16_terms", sixteen)):
        plan = regress.Plan(nx, ny, M, index, terms, control=control, what=regress.MAPS)
        regress.add_year_dev(plan, x, 0)
        k = [0]

        def update():
            k[0] += 1
            regress.add_year_dev(plan, x, k[0])

        ms = timed(update)
        regress.finish_dev(plan, k[0] + 1)
        torch.cuda.synchronize()
        state = M * len(terms) * np_ * (4 + 3 * 16)  # y0 read, three fp64 sums read and written
        out[name] = {"add_year_ms": round(ms, 4), "state_bytes_moved": state, "plan": plan.describe()}
        plan.close()
    dplan = diag.Plan(nx, ny)
    dms = timed(lambda: diag.reduce_dev(dplan, x, abi.D_REGIONS))
    dplan.close()
    out["index_pass_ms"] = round(dms, 4)  # diag over all five variables; the index kernel behind it is one thread per member
    for name in ("4_terms", "16_terms"):
        # add_year_dev minus reduce_dev: a DERIVED figure that also holds the index kernel and the launch gaps (a kernel trace
        # times the update kernel itself: profiles/reg_numbers.txt)
        out[name]["update_ms_by_difference"] = round(out[name]["add_year_ms"] - dms, 4)
    cplan = clim.Plan(nx, ny, M, what=1)
    clim.add_year_dev(cplan, x, 0)
    ck = [0]

    def cadd():
        ck[0] += 1
        clim.add_year_dev(cplan, x, ck[0])

    out["clim_add_year_ms"] = round(timed(cadd), 4)
    clim.finish_dev(cplan, ck[0] + 1)
    torch.cuda.synchronize()
    cplan.close()
    out["code"] = {n: codesha.record(build.LIB, n) for n in ("reg_update_kernel", "reg_index_kernel", "reg_finish_kernel")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("members", type=int, nargs="?", default=256)
    ap.add_argument("years", type=int, nargs="?", default=70)
    ap.add_argument("--compare", action="store_true", help="also run Engine.run + regress.reference: equal products, both legs timed")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--kernel-timing", action="store_true", help="also time the index pass and the update kernel alone")
    args = ap.parse_args()
    import torch
    from greb_climate_model_amd import abi, diag, engine, ensemble, regress, workload

    U, Y = args.members, args.years
    M = 2 * U
    inp = workload.make_inputs()
    nx, ny = inp.nx, inp.ny
    p = abi.default_params(ipx=95, ipy=38)
    ov = ensemble.perturbed_physics(U, p)
    overrides = [{k: float(ov[m % U, j]) for j, k in enumerate(ensemble.PERTURBED)} for m in range(M)]
    control = list(range(U)) * 2
    indices, terms = make_terms()
    plan = regress.Plan(nx, ny, M, indices, terms, control=control)
    rise = np.float32(340.0) * np.float32(1.01) ** np.arange(1, Y + 1, dtype=np.float32)
    co2 = np.concatenate([np.full((U, Y), 340.0, np.float32), np.repeat(rise[None, :], U, axis=0)]).astype(np.float32)
    area = np.cos(np.deg2rad(np.asarray(diag.latitudes(ny), np.float64)))[:, None] * np.ones((ny, nx))
    std = diag.standard_regions(inp)
    masks = {k: std[k].astype(np.float64) * area for k in ("Arctic", "land", "ocean")}
    masks["globe"] = area
    e = engine.Engine(inp, p, n_members=M, overrides=overrides)
    e.flux_correction(1)
    start = [e.state(m) for m in range(M)]  # every timed call starts from the spun-up state

    def run_and_reference():
        mon, yearly = e.run(Y, co2)
        ref = regress.reference(np.moveaxis(mon, 1, 0), indices, terms, control)
        return mon, yearly, ref

    legs = {"run_reg": lambda: e.run_reg(Y, co2, plan)}
    if args.compare:  # the path run_reg replaces
        legs = {"run_and_reference": run_and_reference, **legs}
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

    res = last["run_reg"]
    means = regional(res.slope[U:], masks)
    delivered = sum(getattr(res, n).nbytes for n in regress.PRODUCTS)
    out = {"grid": [nx, ny], "engine_members": M, "members": U, "years": Y, "plan": plan.describe(), "terms": NAMES,
           "index": "annual global-mean Tsurf response [K]",
           "index_at_the_end": {"median": round(float(np.median(res.index[U:, -1, 0])), 4), "min": round(float(res.index[U:, -1, 0].min()), 4),
                                "max": round(float(res.index[U:, -1, 0].max()), 4)},
           "slope_per_K": summary(means),
           "median_r2": {n: round(float(np.nanmedian(res.r2[U:, t])), 4) for t, n in enumerate(NAMES)},
           "per_member": {k: np.round(a, 5).tolist() for k, a in means.items() if k != "globe"},
           "run_reg": rate("run_reg"), "bytes_delivered": int(delivered),
           "monthly_bytes_of_the_run": int(M) * Y * 12 * 5 * ny * nx * 4}
    if args.compare:
        mon, yearly, ref_all = last["run_and_reference"]
        some = sorted({0, 1, U // 2, U - 1} & set(range(U)))
        rows = some + [U + j for j in some]                           # the controls in front, as in the run
        k = len(some)
        x = np.ascontiguousarray(np.moveaxis(mon[rows], 1, 0))
        dplan = diag.Plan(nx, ny)
        reg = [diag.reduce_dev(dplan, torch.tensor(xk).cuda(), abi.D_REGIONS).regions for xk in x]
        torch.cuda.synchronize()
        reg = np.stack([r.cpu().numpy() for r in reg])
        dplan.close()
        ref = regress.reference(x, indices, terms, list(range(k)) * 2, regions=reg)
        differ = 0
        for n in regress.PRODUCTS:
            got, want = np.ascontiguousarray(getattr(res, n)[rows]), getattr(ref, n)
            gn, wn = np.isnan(got), np.isnan(want)
            differ += int(((gn != wn) | (~gn & ~wn & (got.view(np.uint32) != want.view(np.uint32)))).sum())
        out["compared_members"] = some
        out["values_that_differ_from_the_reference"] = differ
        out["reference_slope_per_K"] = summary(regional(ref_all.slope[U:], masks))  # (the numpy regional means: last bits may differ)
        out["equal_products"] = differ == 0 and bool(np.array_equal(yearly.view(np.uint32), res.yearly.view(np.uint32)))
        out["run_and_reference"] = rate("run_and_reference")
        out["run_and_reference_bytes_delivered"] = int(mon.nbytes + yearly.nbytes)
        out["run_reg_minus_run_and_reference"] = round(out["run_reg"]["mean"] - out["run_and_reference"]["mean"], 1)
    if args.kernel_timing:
        out["kernel_timing"] = kernel_timing(nx, ny)
        yr = 512 / out["run_reg"]["mean"] * 1e3  # ms of a model year of a 512-member ensemble at this run's rate
        for name in ("4_terms", "16_terms"):
            out["kernel_timing"][name]["share_of_a_model_year"] = round(out["kernel_timing"][name]["add_year_ms"] / yr, 5)
    out["describe"] = e.describe()
    e.close(); plan.close()
    print(json.dumps(out))
    if args.compare:
        assert out["equal_products"], "run_reg differs from regress.reference of Engine.run's records"


if __name__ == "__main__":
    main()
