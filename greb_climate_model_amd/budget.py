"""Budget output through the plans: the flux terms of the update and sums of them, reduced on the device.

Engine.run_budget hands back the thirteen flux terms of every month of every member -- [n_members][years][12][13][ny][nx],
which a many-member run cannot hold.  What is wanted of them is small: the global-mean imbalance per member and year, the
surface and the atmospheric net flux, evaporation plus rain.  Those are sums of terms, the right-hand sides of
src/greb.f90:258, :260 and :263, and they go through the same four plans as the state records (csrc/greb_fluxes.hip;
include/greb_engine.h: greb_budget_combine_dev, greb_engine_run_budget_diag / _clim / _ens / _lin):

    cb = budget.combo({"surface_net": budget.SURFACE_NET, "atmos_net": budget.ATMOS_NET})
    plan = diag.Plan(inp.nx, inp.ny, diag.standard_regions(inp), n_vars=len(cb.names))
    res = engine.Engine(inp, p, n_members=512).run_diag(100, co2, plan, abi.D_REGIONS, records=cb)
    res.regions[..., res.vars.index("surface_net"), 0]            # [512][100][12]: the global-mean surface imbalance

records="budget" reduces the thirteen terms themselves.  A sum is formed BEFORE the reduction, so variances, ranges,
quantiles and residuals are those of the sum.  combine_reference() is the numpy float32 statement of the combination stage,
one IEEE operation per rounding as the kernel performs them: the tests hold the device to it bit for bit.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _plan, abi

TERMS = abi.BUDGET_NAMES  # the thirteen terms in record order (greb_budget_name)
STATE_NAMES = ("Tsurf", "Tair", "Tocean", "q", "albedo")  # the five state records, src/greb.f90:978-982
# the right-hand sides of the update as term -> coefficient:
SURFACE_NET = {"sw": 1, "LW_surf": 1, "LWair_down": -1, "Q_lat": 1, "Q_sens": 1}   # :258, W/m2 into the surface layer
ATMOS_NET = {"LWair_down": 2, "LW_abs": -1, "Q_lat_air": 1, "Q_sens": -1}          # :260 (LWair_up equals LWair_down, :432)
DQ_PHYS = {"dq_eva": 1, "dq_rain": 1}                                              # :263, 1/s
STANDARD = {"surface_net": SURFACE_NET, "atmos_net": ATMOS_NET, "dq_phys": DQ_PHYS}


@dataclass
class Combo:
    """Linear combinations of the budget terms: matrix [n_out][13] float32 (row k: the coefficients of output k) and the
    outputs' names."""
    matrix: np.ndarray
    names: tuple

    def __iter__(self):  # matrix, names = budget.combo(...)
        return iter((self.matrix, self.names))

    def rows(self) -> dict:
        """The dict of dicts combo() was made of (zero coefficients left out)."""
        return {n: {TERMS[j]: float(c) for j, c in enumerate(row) if c != 0} for n, row in zip(self.names, self.matrix)}


def combo(rows: dict) -> Combo:
    """{"surface_net": {"sw": 1, "LW_surf": 1, "LWair_down": -1, ...}, ...} -> Combo (matrix, names), outputs in the dict's
    order.  An unknown term, no output, more than abi.MAX_RECORD_VARS outputs, an output without a non-zero coefficient or
    with one that is not finite is a GrebError(-1) naming the offender."""
    from . import engine
    rows = dict(rows)
    if not 1 <= len(rows) <= abi.MAX_RECORD_VARS:
        raise engine.GrebError(-1, f"budget.combo: {len(rows)} outputs (1 ... {abi.MAX_RECORD_VARS})")
    m = np.zeros((len(rows), abi.NBUDGET), np.float32)
    for k, (name, terms) in enumerate(rows.items()):
        for t, c in dict(terms).items():
            if t not in TERMS:
                raise engine.GrebError(-1, f"budget.combo: output {name!r}: unknown term {t!r} (one of {', '.join(TERMS)})")
            m[k, TERMS.index(t)] = c
            if not np.isfinite(m[k, TERMS.index(t)]):
                raise engine.GrebError(-1, f"budget.combo: output {name!r}: the coefficient of {t!r} is not finite")
        if not m[k].any():
            raise engine.GrebError(-1, f"budget.combo: output {name!r} has no non-zero coefficient")
    return Combo(m, tuple(str(n) for n in rows))


def as_combo(records):
    """What Engine.run_*(records=...) takes, "budget" aside "state": None for "budget" (the thirteen terms), a Combo for a
    Combo, a (matrix, names) pair or a dict of dicts."""
    from . import engine
    if isinstance(records, str):
        if records == "budget":
            return None
        raise engine.GrebError(-1, f'records = {records!r}: "state", "budget" or a budget.combo(...) expected')
    if isinstance(records, Combo):
        cb = records
    elif isinstance(records, dict):
        cb = combo(records)
    else:
        try:
            m, names = records
        except (TypeError, ValueError):
            raise engine.GrebError(-1, 'records: "state", "budget" or a budget.combo(...) expected') from None
        cb = Combo(m, tuple(names))
    m = np.ascontiguousarray(cb.matrix, np.float32)
    if m.ndim != 2 or m.shape[1] != abi.NBUDGET or m.shape[0] != len(cb.names):
        raise engine.GrebError(-1, f"records: a combination matrix [{len(cb.names)}][{abi.NBUDGET}] expected, got {list(m.shape)}")
    return Combo(m, tuple(cb.names))


def record_names(records) -> tuple:
    """The names of the variables a reduced run over `records` delivers: the axis its shapes call [5]."""
    from . import derive
    if isinstance(records, str) and records == "state":
        return STATE_NAMES
    if isinstance(records, derive.Program):
        return records.names
    cb = as_combo(records)
    return TERMS if cb is None else cb.names


def combine_reference(matrix, budget) -> np.ndarray:
    """The combination stage in numpy float32, operation by operation as csrc/greb_fluxes.hip performs it: budget
    [..][13][ny][nx] (or any [..][13][...] with the terms on axis `-3`) float32 -> [..][n_out][ny][nx].  Per output, over the
    terms in ascending order, skipping zero coefficients: the first gives acc = c * b, every later one acc = acc + c * b,
    each a float32 multiply and a float32 add."""
    m = np.asarray(getattr(matrix, "matrix", matrix), np.float32)
    b = np.asarray(budget)
    if b.dtype != np.float32 or b.ndim < 3 or b.shape[-3] != abi.NBUDGET:
        raise ValueError("combine_reference: float32 budget [..][13][ny][nx] expected")
    if m.ndim != 2 or m.shape[1] != abi.NBUDGET:
        raise ValueError("combine_reference: matrix [n_out][13] expected")
    out = np.empty(b.shape[:-3] + (m.shape[0],) + b.shape[-2:], np.float32)
    for k in range(m.shape[0]):
        acc = None
        for j in range(abi.NBUDGET):
            c = m[k, j]
            if c == 0:
                continue
            t = c * b[..., j, :, :]
            assert t.dtype == np.float32
            acc = t if acc is None else acc + t
        if acc is None:
            raise ValueError(f"combine_reference: row {k} is zero everywhere")
        out[..., k, :, :] = acc
    return out


def combine_dev(matrix, budget_year):
    """One model year of budget records on the GPU, a contiguous float32 torch tensor [n_members][12][13][ny][nx], turned
    into [n_members][12][n_out][ny][nx] (greb_budget_combine_dev) on torch's current stream, without synchronising."""
    import torch
    from . import engine
    m = np.ascontiguousarray(getattr(matrix, "matrix", matrix), np.float32)
    if m.ndim != 2 or m.shape[1] != abi.NBUDGET:
        raise engine.GrebError(-1, f"budget.combine_dev: a matrix [n_out][{abi.NBUDGET}] expected, got {list(m.shape)}")
    x = budget_year
    dev = _plan.gpu_tensor_check(x, x.dim() == 5 and tuple(x.shape[1:3]) == (12, abi.NBUDGET), "budget.combine_dev",
                                 f"[n][12][{abi.NBUDGET}][ny][nx]")
    n, ny, nx = x.shape[0], x.shape[3], x.shape[4]
    out = torch.empty((n, 12, m.shape[0], ny, nx), dtype=torch.float32, device=x.device)
    _plan.call_on_current_stream(dev, engine.lib().greb_budget_combine_dev, abi.fptr(m), int(m.shape[0]), _plan.ptr(x), int(n),
                                 int(ny * nx), _plan.ptr(out))
    return out
