#!/usr/bin/env python3
"""The full factorial of the eight process switches (GREB_X_*) as ONE engine that hands back only the linear model across
its 256 members: the mean, the main effect of each process and the interactions between processes, per monthly record
(Engine.run_lin, csrc/greb_lin.hip), and the residual map of what higher interactions leave.

  python tools/run_effects.py [years] [--order N] [--bits MASK] [--compare] [--passes N] [--kernel-timing]

Runs 1 flux-correction year, then `years` scenario years (default 3) at 2 x CO2 and prints one JSON line: the
area-weighted global-mean annual-mean Tsurf main effect of each process (last year; +-1 coding: half the mean difference
between the members with the switch and those without), the largest interactions, the bytes returned against those of
Engine.run, and the ensemble-years/s of the run_lin call (--passes timed calls after one untimed).  --order N:
interactions of up to N switches (default 2: 37 terms; at most 64 terms fit a plan).  --compare also runs Engine.run over
the same years, forms the same numbers on the host with lin.reference and checks every value for equal bits, and times
Engine.run and Engine.run_ens (GREB_S_MEAN of all members) in the same process, the three legs alternating.
--bits MASK: the factorial of the switches in MASK only (default 0xff, all eight).  The 32 members that combine
GREB_X_LW_LINEAR_VAPOR and GREB_X_NO_CIRCULATION with the hydrology left on run away in the second scenario year at
2 x CO2 (NaN in their records, from Engine.run as from here).  That is the model's behaviour under LW_LINEAR_VAPOR without
circulation and with hydrology, not the port's: the oracle, asked for the same switch word, is finite in year 1 and non-finite
from year 2 as well (tests/test_switch_words_cpu.py, tests/test_gpu_switch_words.py).  A contrast over all members is NaN
wherever one of its members is: `non_finite_values` counts them, and --bits 0xf7 (without the linearised vapour feedback: 128 members, 29
terms) gives finite effects everywhere.  Where records are NaN the comparison of --compare asks for NaN on both sides
(an operation that makes a NaN gives it another sign bit on the host than on the device), for equal bits elsewhere.
--kernel-timing times, on a year of synthetic records of the same ensemble, the two launches of this plan beside
ens_moments_kernel on the same data, and states the fp64 multiply-add rate they achieve."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_timing(weight, design, nx, ny, reps=20):
    import torch
    from greb_climate_model_amd import abi, build, codesha, ens, lin
    K, M = weight.shape
    x = torch.rand((M, 12, 5, ny, nx), dtype=torch.float32, device="cuda") * 90.0 + 220.0
    n = x.numel() // M

    def timed(fn):
        fn(); torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record()
        for i in range(reps):
            fn(); ev[i + 1].record()
        torch.cuda.synchronize()
        return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]))

    out = {"members": int(M), "terms": int(K), "elements_per_member": int(n)}
    kp = 16 * ((K + 15) // 16)  # the terms the kernels carry: chunks of 16
    for name, what, pairs, issued in (("coef", abi.L_COEF, M * K, M * kp), ("rss", abi.L_RSS, 2 * M * K + M, 2 * M * kp + M),
                                      ("both", abi.L_COEF | abi.L_RSS, 3 * M * K + M, 3 * M * kp + M)):
        plan = lin.Plan(nx, ny, M, weight, design=design, what=what)
        ms = timed(lambda: lin.reduce_dev(plan, x))  # (includes torch.empty of the outputs)
        torch.cuda.synchronize()
        plan.close()
        # a multiply-add = one fp64 multiply and one fp64 add, two instructions (not fused): of the model, and as issued
        out[name] = {"ms": round(ms, 4), "fp64_multiply_adds_per_s": round(pairs * n / ms * 1e3, 0),
                     "issued_incl_padding_per_s": round(issued * n / ms * 1e3, 0)}
    plan = ens.Plan(nx, ny, M, [0] * M, what=abi.S_MEAN | abi.S_VAR | abi.S_RANGE)
    ms = timed(lambda: ens.reduce_dev(plan, x))
    torch.cuda.synchronize()
    plan.close()
    out["ens_moments_kernel_ms"] = round(ms, 4)
    out["code"] = {k: codesha.record(build.LIB, k) for k in ("lin_coef_kernel", "lin_rss_kernel")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("years", type=int, nargs="?", default=3)
    ap.add_argument("--order", type=int, default=2, help="interactions of up to this many switches (default 2: 37 terms)")
    ap.add_argument("--bits", type=lambda v: int(v, 0), default=0xff, help="the switches of the factorial (default 0xff: all eight)")
    ap.add_argument("--compare", action="store_true", help="also run Engine.run: equal bits against lin.reference; time run and run_ens")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--kernel-timing", action="store_true", help="also time the two launches alone")
    args = ap.parse_args()
    import torch
    from greb_climate_model_amd import abi, diag, engine, ens, ensemble, lin, workload

    Y = args.years
    inp = workload.make_inputs()
    nx, ny = inp.nx, inp.ny
    p = abi.default_params(ipx=95, ipy=38)
    sw = ensemble.switch_factorial(args.bits)
    M = len(sw)
    names, weight, design = lin.factorial(sw, args.bits, order=args.order)
    plan = lin.Plan(nx, ny, M, weight, design=design)
    e = engine.Engine(inp, p, members=[{"switches": int(s)} for s in sw])
    e.flux_correction(1)
    start = [e.state(m) for m in range(M)]  # every timed call starts from the spun-up state

    eplan = ens.Plan(nx, ny, M, [0] * M, what=abi.S_MEAN) if args.compare else None
    legs = {"run_lin": lambda: e.run_lin(Y, 680.0, plan)}
    if args.compare:  # the path run_lin replaces, and the nearest existing reducer
        legs = {"run": lambda: e.run(Y, 680.0), "run_ens_mean": lambda: e.run_ens(Y, 680.0, eplan), **legs}
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

    res = last["run_lin"]
    area = np.cos(np.deg2rad(diag.latitudes(ny)))[:, None] * np.ones((ny, nx))
    gm = lambda a: float((a.astype(np.float64) * area).sum() / area.sum())
    tsurf = res.coef[:, Y - 1, :, 0].astype(np.float64).mean(axis=1)  # [n_terms][ny][nx]: annual-mean Tsurf of the last year
    effect = {name: round(gm(tsurf[k]), 4) for k, name in enumerate(names)}
    inter = sorted((n for n in names if ":" in n), key=lambda n: -abs(effect[n]))[:6]
    out = {"grid": [nx, ny], "members": M, "years": Y, "bits": args.bits, "order": args.order, "terms": len(names),
           "global_mean_annual_tsurf_K": {"mean": effect["mean"],
                                          "main_effects": {n: effect[n] for n in names[1:] if ":" not in n},
                                          "largest_interactions": {n: effect[n] for n in inter}},
           "global_mean_annual_tsurf_rss_K2": round(gm(res.rss[Y - 1, :, 0].astype(np.float64).mean(axis=0)), 4),
           "non_finite_values": int((~np.isfinite(res.coef)).sum() + (~np.isfinite(res.rss)).sum()),
           "run_lin": rate("run_lin"),
           "bytes_delivered": int(res.coef.nbytes + res.rss.nbytes),
           "monthly_bytes_of_the_run": int(M) * Y * 12 * 5 * ny * nx * 4}
    if args.compare:
        mon, yearly = last["run"]
        differ = {"coef": 0, "rss": 0}
        unequal = lambda a, b: int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())
        for y in range(Y):
            ref = lin.reference(mon[:, y], weight, design=design)
            differ["coef"] += unequal(res.coef[:, y], ref.coef)
            differ["rss"] += unequal(res.rss[y], ref.rss)
        out["values_that_differ_from_the_reference"] = differ
        out["members_with_non_finite_records"] = int((~np.isfinite(mon)).reshape(M, -1).any(axis=1).sum())
        out["equal_bits"] = not any(differ.values()) and bool(np.array_equal(yearly.view(np.uint32), res.yearly.view(np.uint32)))
        out["run"], out["run_ens_mean"] = rate("run"), rate("run_ens_mean")
        # not slower than the path it replaces, allowing three times that leg's run-to-run spread
        out["run_lin_minus_run"] = round(out["run_lin"]["mean"] - out["run"]["mean"], 1)
        out["not_slower_than_run"] = bool(out["run_lin"]["mean"] >= out["run"]["mean"] - 3 * out["run"]["spread"])
        eplan.close()
    if args.kernel_timing:
        out["kernel_timing"] = kernel_timing(weight, design, nx, ny)
    out["describe"] = e.describe()
    e.close(); plan.close()
    print(json.dumps(out))
    if args.compare and not out["equal_bits"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
