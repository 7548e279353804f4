#!/usr/bin/env python3
"""A perturbed-physics ensemble at control CO2 beside the same members at 2 x CO2, as ONE engine, that hands back only
the statistics of the response across the pairs (Engine.run_ens, csrc/greb_ens.hip).

  python tools/run_ens.py [pairs] [years] [--grid NX NY] [--compare] [--passes N] [--kernel-timing]

Members 0 ... pairs-1 are ensemble.perturbed_physics members at 340 ppm, members pairs ... 2 pairs - 1 the same physics
at 680 ppm.  The control members are in no group; group 0 is the 2 x CO2 members, each as the difference to its partner,
with mean, variance, range and the 5 / 25 / 50 / 75 / 95 % quantiles.  (A plan has one control map for all its groups, and
every grouped member needs a control: the raw statistics of the control members are a second plan without a map.)
Runs 1 flux-correction year, then `years` scenario years (default 256 pairs, 3 years) and prints one JSON line: the
area-weighted global mean of the median and of the 5 / 95 % maps of the December Tsurf response (last year), the bytes
returned against those of Engine.run, and the ensemble-years/s of the run_ens call (best of --passes timed calls after
one untimed).  --compare also runs Engine.run over the same years and checks every product for equal bits against
ens.reference, and times Engine.run_diag (all products) in the same process on the same box.  --kernel-timing times, on a
year of synthetic records of the same ensemble, the moments launch and the quantile launch of this layout, and the
moments kernel on ONE group of all members without a control beside greb_ensemble_moments_dev on the same data."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROBS = (0.05, 0.25, 0.5, 0.75, 0.95)


def layout(pairs):
    """group and control of the 2 * pairs members."""
    return [-1] * pairs + [0] * pairs, [-1] * pairs + list(range(pairs))


def kernel_timing(pairs, nx, ny, reps=20):
    import torch
    from greb_climate_model_amd import abi, build, codesha, ens, ensemble
    M = 2 * pairs
    x = torch.rand((M, 12, 5, ny, nx), dtype=torch.float32, device="cuda") * 90.0 + 220.0
    n = x.numel()

    def timed(fn):
        fn(); torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record()
        for i in range(reps):
            fn(); ev[i + 1].record()
        torch.cuda.synchronize()
        return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]))

    out = {"elements_per_year": int(n)}
    group, control = layout(pairs)
    for name, what, probs in (("response_moments", ens.MOMENTS, ()), ("response_quantiles", abi.S_QUANTILES, PROBS)):
        plan = ens.Plan(nx, ny, M, group, control=control, probs=probs, what=what)
        out[name] = {"ms_per_year": round(timed(lambda: ens.reduce_dev(plan, x)), 4)}  # (includes torch.empty of the outputs)
        torch.cuda.synchronize()
        plan.close()
    out["response_moments"]["GB_per_s_of_member_data"] = round(n * 4 / out["response_moments"]["ms_per_year"] / 1e6, 1)
    plan = ens.Plan(nx, ny, M, [0] * M)  # one group of all members, no control: mean + variance + range
    new = timed(lambda: ens.reduce_dev(plan, x))
    torch.cuda.synchronize()
    plan.close()
    old = timed(lambda: ensemble.local_moments(x))
    out["all_members_one_group"] = {"ens_moments_ms": round(new, 4), "ensemble_moments_dev_ms": round(old, 4),
                                    "rate_new_over_old": round(old / new, 4),
                                    "GB_per_s_new": round(n * 4 / new / 1e6, 1), "GB_per_s_old": round(n * 4 / old / 1e6, 1)}
    out["code"] = codesha.record(build.LIB, "ens_moments_kernel")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pairs", type=int, nargs="?", default=256, help="perturbed-physics members; the engine has 2 * pairs")
    ap.add_argument("years", type=int, nargs="?", default=3)
    ap.add_argument("--grid", type=int, nargs=2, default=(96, 48), metavar=("NX", "NY"))
    ap.add_argument("--compare", action="store_true", help="also run Engine.run (equal bits against ens.reference) and time run_diag")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--kernel-timing", action="store_true", help="also time the moments and quantile launches alone")
    args = ap.parse_args()
    import torch
    from greb_climate_model_amd import abi, diag, engine, ens, ensemble, workload

    nx, ny = args.grid
    pairs, Y = args.pairs, args.years
    M = 2 * pairs
    inp = workload.make_inputs(nx, ny)
    p = abi.default_params(ipx=nx - 1, ipy=(38 * ny) // 48)
    ov = ensemble.perturbed_physics(pairs, p)
    overrides = [{k: float(ov[m % pairs, j]) for j, k in enumerate(ensemble.PERTURBED)} for m in range(M)]
    group, control = layout(pairs)
    plan = ens.Plan(nx, ny, M, group, control=control, probs=PROBS)
    co2 = np.repeat(np.asarray([340.0] * pairs + [680.0] * pairs, np.float32)[:, None], Y, axis=1)
    e = engine.Engine(inp, p, n_members=M, overrides=overrides)
    e.flux_correction(1)
    start = [e.state(m) for m in range(M)]  # every timed call starts from the spun-up state

    def timed(fn):
        best, out = None, None
        for i in range(1 + max(1, args.passes)):  # the first call pays for allocations and code loading
            for m in range(M):
                e.set_corrections(None, start[m], member=m)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if i > 0:
                best = dt if best is None else min(best, dt)
        return best, out

    dt, res = timed(lambda: e.run_ens(Y, co2, plan))
    area = np.cos(np.deg2rad(diag.latitudes(ny)))[:, None] * np.ones((ny, nx))
    gm = lambda a: round(float((a.astype(np.float64) * area).sum() / area.sum()), 4)
    dec = res.quant[0, Y - 1, :, 11, 0]  # [n_probs][ny][nx]: December Tsurf response of the last year
    products = [getattr(res, n) for n in ens.PRODUCTS]
    out = {"grid": [nx, ny], "pairs": pairs, "members": M, "years": Y, "probs": list(PROBS),
           "global_mean_december_tsurf_response_K": {"q05": gm(dec[0]), "median": gm(dec[2]), "q95": gm(dec[4]),
                                                     "mean": gm(res.mean[0, Y - 1, 11, 0]), "std": gm(res.std[0, Y - 1, 11, 0])},
           "finite": bool(all(np.isfinite(a).all() for a in products)),
           "run_ens": {"seconds": round(dt, 4), "ensemble_years_per_s": round(M * Y / dt, 1)},
           "bytes_delivered": int(sum(a.nbytes for a in products)),
           "monthly_bytes_of_the_run": int(M) * Y * 12 * 5 * ny * nx * 4}
    if args.compare:
        dt_run, (mon, yearly) = timed(lambda: e.run(Y, co2))
        differ = {}
        for y in range(Y):
            ref = ens.reference(mon[:, y], group, control, PROBS)
            for name in ens.PRODUCTS:
                got = getattr(res, name)[:, y]
                differ[name] = differ.get(name, 0) + int((got.view(np.uint32) != getattr(ref, name).view(np.uint32)).sum())
        out["values_that_differ_from_the_reference"] = differ
        out["equal_bits"] = not any(differ.values()) and bool(np.array_equal(yearly, res.yearly))
        out["run"] = {"seconds": round(dt_run, 4), "ensemble_years_per_s": round(M * Y / dt_run, 1)}
        dplan = diag.Plan(nx, ny)
        dt0, _ = timed(lambda: e.run_diag(Y, co2, dplan))
        out["run_diag"] = {"seconds": round(dt0, 4), "ensemble_years_per_s": round(M * Y / dt0, 1)}
        out["run_ens_over_run_diag"] = round(dt / dt0, 4)
        dplan.close()
    if args.kernel_timing:
        out["kernel_timing"] = kernel_timing(pairs, nx, ny)
    out["describe"] = e.describe()
    e.close(); plan.close()
    print(json.dumps(out))
    if args.compare and not out["equal_bits"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
