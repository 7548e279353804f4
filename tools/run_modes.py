#!/usr/bin/env python3
"""The leading modes of spread of a perturbed-physics ensemble's CO2 response, from ONE engine that hands back only the
Gram matrices across its members (Engine.run_gram, csrc/greb_gram.hip).

  python tools/run_modes.py [pairs] [years] [--compare] [--passes N] [--kernel-timing]

Members 0 ... pairs-1 are ensemble.perturbed_physics members at 340 ppm, members pairs ... 2 pairs - 1 the same physics at
680 ppm (defaults: 256 pairs, 3 years).  The plan uses the 2 x CO2 members, each against its control, one block per
variable, under gram.area_scale: G[year][variable][pairs][pairs], the area-weighted inner products of the members'
response patterns over the year's twelve months.  Runs 1 flux-correction year, then `years` scenario years, and prints
one JSON line: the explained variance of the leading modes of the last year's Tsurf response (gram.eof), the largest and
the median distance between two members' responses, the bytes returned against those of Engine.run, and the ensemble-years/s
of the run_gram call (--passes timed calls after one untimed).
--compare also runs Engine.run over the same years and checks G for equal bits against gram.reference of its records --
for a subset of the used members (both sides of every edge of the kernel's 64-member tiles and a few between: the mirror
takes one numpy step per element and is quadratic in the members; a subset's matrix is the full one's rows and columns) --
and times Engine.run and Engine.run_ens (GREB_S_MEAN of the used members) in the same process, the three legs alternating.
--kernel-timing times reduce_dev alone on a year of synthetic records of 256 and 512 used members (median of 20 launches),
states its fp64 multiply-add rate against the 39.3e12/s of the data sheet, and times lin_coef_kernel (16 terms) on the
same data."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP64_FMA = 39.3e12  # vector fp64 multiply-adds per second of one MI355X (78.6 TFLOP/s)
TILE = 64                # greb_gram.h: kGramTile


def kernel_timing(nx, ny, reps=20):
    import torch
    from greb_climate_model_amd import build, codesha, gram, lin
    out = {}

    def timed(fn):
        fn(); torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record()
        for i in range(reps):
            fn(); ev[i + 1].record()
        torch.cuda.synchronize()
        return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]))

    for U in (256, 512):
        M = 2 * U
        x = torch.rand((M, 60, ny, nx), dtype=torch.float32, device="cuda") * 90.0 + 220.0
        n = 60 * ny * nx
        plan = gram.Plan(nx, ny, M, 60, gram.blocks_by_var(5), use=[0] * U + [1] * U, control=list(range(U)) * 2,
                         scale=gram.area_scale(ny, nx))
        ms = timed(lambda: gram.reduce_dev(plan, x))  # (includes torch.empty of the output)
        torch.cuda.synchronize()
        plan.close()
        tiles = (U + TILE - 1) // TILE
        model = U * (U + 1) // 2 * n                         # the multiply-adds of the lower triangle, diagonal included
        issued = tiles * (tiles + 1) // 2 * TILE * TILE * n  # ... as the tiles perform them (diagonal tiles form both halves)
        w = np.full((16, M), 1.0 / U)
        lplan = lin.Plan(nx, ny, M, w, use=[0] * U + [1] * U, control=list(range(U)) * 2)
        lms = timed(lambda: lin.reduce_dev(lplan, x))
        torch.cuda.synchronize()
        lplan.close()
        out[f"used_{U}"] = {"ms": round(ms, 4), "fp64_multiply_adds_per_s": round(model / ms * 1e3, 0),
                            "issued_per_s": round(issued / ms * 1e3, 0),
                            "issued_fraction_of_39.3e12": round(issued / ms * 1e3 / PEAK_FP64_FMA, 4),
                            "scratch_bytes": 60 * U * U * 8, "lin_coef_kernel_16_terms_ms": round(lms, 4)}
        del x
    out["code"] = {k: codesha.record(build.LIB, k) for k in ("gram_tile_kernel", "gram_sum_kernel")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pairs", type=int, nargs="?", default=256)
    ap.add_argument("years", type=int, nargs="?", default=3)
    ap.add_argument("--compare", action="store_true", help="also run Engine.run: equal bits against gram.reference; time run and run_ens")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--kernel-timing", action="store_true", help="also time reduce_dev alone")
    ap.add_argument("--modes", type=int, default=5)
    args = ap.parse_args()
    import torch
    from greb_climate_model_amd import abi, engine, ens, ensemble, gram, workload

    pairs, Y = args.pairs, args.years
    M = 2 * pairs
    inp = workload.make_inputs()
    nx, ny = inp.nx, inp.ny
    p = abi.default_params(ipx=95, ipy=38)
    ov = ensemble.perturbed_physics(pairs, p)
    overrides = [{k: float(ov[m % pairs, j]) for j, k in enumerate(ensemble.PERTURBED)} for m in range(M)]
    use, control = [0] * pairs + [1] * pairs, list(range(pairs)) * 2
    block, scale = gram.blocks_by_var(5), gram.area_scale(ny, nx)
    plan = gram.Plan(nx, ny, M, 60, block, use=use, control=control, scale=scale)
    co2 = np.repeat(np.asarray([340.0] * pairs + [680.0] * pairs, np.float32)[:, None], Y, axis=1)
    e = engine.Engine(inp, p, n_members=M, overrides=overrides)
    e.flux_correction(1)
    start = [e.state(m) for m in range(M)]  # every timed call starts from the spun-up state

    eplan = ens.Plan(nx, ny, M, [-1] * pairs + [0] * pairs, control=control, what=abi.S_MEAN) if args.compare else None
    legs = {"run_gram": lambda: e.run_gram(Y, co2, plan)}
    if args.compare:  # the path run_gram replaces, and the nearest existing reducer
        legs = {"run": lambda: e.run(Y, co2), "run_ens_mean": lambda: e.run_ens(Y, co2, eplan), **legs}
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

    res = last["run_gram"]
    G = res.G[Y - 1, 0]  # the last year's Tsurf responses
    k = min(args.modes, pairs)
    lam, frac, weight = gram.eof(G, k, plan)
    D = gram.distance(G)[np.triu_indices(pairs, 1)] if pairs > 1 else np.zeros(1)
    area = float((scale.astype(np.float64) ** 2).sum()) * 12  # the weights of a year's twelve maps
    out = {"grid": [nx, ny], "members": M, "used": pairs, "years": Y, "blocks": list(res.vars),
           "tsurf_response_modes": {"explained_fraction": [round(float(f), 5) for f in frac],
                                    "rms_amplitude_K": [round(float(np.sqrt(max(l, 0.0) / pairs / area)), 5) for l in lam]},
           "tsurf_response_rms_K": round(float(np.sqrt(np.trace(G) / pairs / area)), 4),
           "tsurf_response_distance_rms_K": {"max": round(float(np.sqrt(max(D.max(), 0.0) / area)), 4),
                                             "median": round(float(np.sqrt(max(np.median(D), 0.0) / area)), 4)},
           "non_finite_values": int((~np.isfinite(res.G)).sum()),
           "run_gram": rate("run_gram"),
           "bytes_delivered": int(res.G.nbytes),
           "monthly_bytes_of_the_run": int(M) * Y * 12 * 5 * ny * nx * 4}
    if args.compare:
        mon, yearly = last["run"]
        edges = sorted({u for t in range(TILE, pairs, TILE) for u in (t - 1, t)} | {0, pairs - 1} | set(range(0, pairs, max(1, pairs // 5))))
        differ = 0
        for y in range(Y):
            ref = gram.reference(mon[:, y].reshape(M, 60, ny, nx), block, use=use, control=control, scale=scale, members=edges)
            got = res.G[y][:, edges][:, :, edges]
            differ += int(((got.view(np.uint64) != ref.view(np.uint64)) & ~(np.isnan(got) & np.isnan(ref))).sum())
        symmetric = bool(np.array_equal(res.G.view(np.uint64), np.swapaxes(res.G, -1, -2).view(np.uint64)))
        out["compared_members"] = [int(u) for u in edges]
        out["values_that_differ_from_the_reference"] = differ
        out["symmetric_bit_for_bit"] = symmetric
        out["equal_bits"] = differ == 0 and symmetric and bool(np.array_equal(yearly.view(np.uint32), res.yearly.view(np.uint32)))
        out["run"], out["run_ens_mean"] = rate("run"), rate("run_ens_mean")
        # not slower than the path it replaces, allowing three times that leg's run-to-run spread
        out["run_gram_minus_run"] = round(out["run_gram"]["mean"] - out["run"]["mean"], 1)
        out["not_slower_than_run"] = bool(out["run_gram"]["mean"] >= out["run"]["mean"] - 3 * out["run"]["spread"])
        eplan.close()
    if args.kernel_timing:
        out["kernel_timing"] = kernel_timing(nx, ny)
        yr = M / out["run_gram"]["mean"] * 1e3  # ms of a model year of this ensemble inside run_gram
        out["kernel_timing"]["share_of_a_model_year"] = round(out["kernel_timing"][f"used_{256 if pairs <= 256 else 512}"]["ms"] / yr, 4)
    out["describe"] = e.describe()
    e.close(); plan.close()
    print(json.dumps(out))
    if args.compare and not out["equal_bits"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
