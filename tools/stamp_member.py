#!/usr/bin/env python3
"""In-kernel stamps of the fused member kernel (diagnostic -DGREB_TUNING build only; the release kernel contains no
stamp code).  Prints, as medians over the members (= workgroups = CUs):
  * the in-kernel shader clock: delta s_memtime / delta s_memrealtime x 100 MHz (MI355X_MICROARCH.md, DVFS item 6)
  * cycles per model step spent in wind staging / the 24 circulation sub-steps / point physics + accumulation
  * per wave: busy cycles per sub-step (barrier release -> arrival at the next barrier) and the share of the
    sub-step it waits at the barrier -- which wave is the critical path
  python tools/stamp_member.py [members=512] [years=2] [budget] [tail] [deal=WORKGROUPS[,SCHEDULE]] [nodeal]
`budget`: the stamped years run through Engine.run_budget (the budget instantiation: its physics phase includes the
accumulation pre-pass).
`tail`: the end of the launch, from the record every (member, chunk) item leaves -- start and end in s_memrealtime ticks,
XCC and hardware ids, shader cycles of the item and of its prologue: per XCD the median clock and the median item
duration, and the IDLE SHARE of the launch = sum over CUs of (launch end - the CU's last item end) / (CUs x launch length),
a CU being an (XCC id, SE / SH / CU id) pair.  `deal=` / `nodeal`: Engine.set_dealing for the stamped engine (default:
the engine's own default)."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from greb_climate_model_amd import engine, ensemble, workload

engine.use_tuning_build()
if os.environ.get("GREB_LIB"):  # a variant build of the tuning library (deal experiments)
    engine._lib_path = os.path.abspath(os.environ["GREB_LIB"])
M = int(sys.argv[1]) if len(sys.argv) > 1 else 512
years = int(sys.argv[2]) if len(sys.argv) > 2 else 2
budget = "budget" in sys.argv[3:]
tail = "tail" in sys.argv[3:]
deal = [a for a in sys.argv[3:] if a.startswith("deal=")]
CH = 10  # kMaxChunks (greb_kernels.h)
inp = workload.make_inputs()
p = engine.params_default(); p.ipx, p.ipy = 95, 38
e = engine.Engine(inp, p, n_members=M)
if "nodeal" in sys.argv[3:]:
    e.set_dealing(workgroups=-1)
elif deal:
    w = [int(x) for x in deal[0][5:].split(",")]
    e.set_dealing(workgroups=w[0], schedule=w[1] if len(w) > 1 else 0)
e.flux_correction(1)
levels = ensemble.co2_sweep(M)
mon = torch.empty((M, 1, 12, 5, e.np), dtype=torch.float32, device="cuda")
for _ in range(max(1, int(2.5 * 3800 / M / 1) // 20 if M >= 256 else 1)):  # >= 2 s of back-to-back launches first
    e.run(1, levels[:, None], monthly_dev_ptr=mon.data_ptr())
st = torch.zeros((M * 8 + M * CH, 8), dtype=torch.int64, device="cuda")  # the wave records, then the item records
f = engine.lib().greb_tuning_set_stamps
f.argtypes = [C.c_void_p, C.c_void_p]
assert f(e.h, st.data_ptr()) == 0
tot = np.zeros((M, 8, 8), np.float64)
bud = torch.empty((M, 1, 12, 13, e.np), dtype=torch.float32, device="cuda") if budget else None
for _ in range(years):
    if budget:
        e.run_budget(1, levels[:, None], monthly_dev_ptr=mon.data_ptr(), budget_dev_ptr=bud.data_ptr())
    else:
        e.run(1, levels[:, None], monthly_dev_ptr=mon.data_ptr())
    torch.cuda.synchronize()
    raw = st.cpu().numpy()
    tot += raw[:M * 8].reshape(M, 8, 8).astype(np.float64)
    items = raw[M * 8:].reshape(M, CH, 8).astype(np.uint64)  # (the last stamped year's)
    st.zero_()
dealt = e.describe()["dealing"]["dealt_launches"]
f(e.h, None)
e.close()
tot /= years
cyc, rt, wind, circ, busy, phys, nsteps, nsub = [tot[:, :, i] for i in range(8)]
clk = np.median(cyc[:, 0] / rt[:, 0]) * 100.0  # MHz
ns, nsb = nsteps[0, 0], nsub[0, 0]
print(f"{'run_budget' if budget else 'run'}: members {M}: launch = {np.median(cyc[:, 0]) / 1e6:.1f} Mcycles = {np.median(rt[:, 0]) / 1e5:.2f} ms; "
      f"in-kernel clock {clk:.0f} MHz (median over workgroups; min {np.min(cyc[:, 0] / rt[:, 0]) * 100:.0f}, max {np.max(cyc[:, 0] / rt[:, 0]) * 100:.0f})")
w0 = lambda x: np.median(x[:, 0]) / ns
print(f"per model step (wave 0): wind staging {w0(wind):.0f} cyc, circulation {w0(circ):.0f} cyc ({w0(circ) / nsb:.0f} per sub-step), "
      f"physics+accumulation {w0(phys):.0f} cyc; total {np.median(cyc[:, 0]) / ns:.0f} cyc = {np.median(cyc[:, 0]) / ns / clk:.2f} us")
sub = np.median(circ[:, 0]) / ns / nsb
print(f"sub-step = {sub:.0f} cycles = {sub / clk:.3f} us; per wave busy cycles per sub-step and barrier wait share:")
for w in range(8):
    b = np.median(busy[:, w]) / ns / nsb
    print(f"  wave {w} (SIMD {w % 4}, {'polar chains' if w == 6 else 'bulk'}): busy {b:6.0f} cyc  waits {100 * (1 - b / sub):4.1f} %")
print(f"member-years/s at this launch time: {M / (np.median(rt[:, 0]) / 1e8) / max(1, -(-M // 256)):.0f}")
if tail:
    rec = items.reshape(-1, 8)
    rec = rec[rec[:, 1] > 0]
    start, end = rec[:, 0].astype(np.int64), rec[:, 1].astype(np.int64)
    xcc, hw = (rec[:, 2] >> np.uint64(32)).astype(np.int64) & 15, rec[:, 2].astype(np.int64) & 0xffffffff
    cu = xcc * 256 + ((hw >> 8) & 255)  # XCC id; CU, SH and SE ids of HW_REG_HW_ID
    cyc, pro, steps = rec[:, 3].astype(np.float64), rec[:, 4].astype(np.float64), (rec[:, 6] - rec[:, 5]).astype(np.float64)
    t0, t1 = start.min(), end.max()
    cus = np.unique(cu)
    last = np.array([end[cu == c].max() for c in cus])
    per_cu = np.array([(cu == c).sum() for c in cus])
    idle = float((t1 - last).sum()) / (len(cus) * float(t1 - t0))
    print(f"tail: {'dealt' if dealt else 'not dealt'}: {len(rec)} items on {len(cus)} CUs ({per_cu.min()} .. {per_cu.max()} items per CU), "
          f"launch {float(t1 - t0) / 1e5:.3f} ms; IDLE SHARE of the launch {100 * idle:.2f} % (a CU's last end to the launch's end: "
          f"median {np.median(t1 - last) / 1e5:.3f} ms, max {float((t1 - last).max()) / 1e5:.3f} ms)")
    busy = np.array([(end[cu == c] - start[cu == c]).sum() for c in cus])
    print(f"tail: CU time inside items {100 * float(busy.sum()) / (len(cus) * float(t1 - t0)):.2f} % of CUs x launch; "
          f"prologue {np.median(pro):.0f} cycles per item (median; max {pro.max():.0f}); cycles per step over items {np.median(cyc / steps):.0f}")
    for x in np.unique(xcc):
        k = xcc == x
        clk = cyc[k] / (end[k] - start[k]) * 100.0
        print(f"  XCD {x}: {k.sum():4d} items on {len(np.unique(cu[k])):3d} CUs  clock median {np.median(clk):.0f} MHz (min {clk.min():.0f}, max {clk.max():.0f})  "
              f"item duration per step median {np.median((end[k] - start[k]) / steps[k]) / 100:.2f} us  last end {float(end[k].max() - t0) / 1e5:.3f} ms")
