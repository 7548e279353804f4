"""Python mirror of the C ABI (include/greb_engine.h) over libgreb_hip.so.

Host-side plumbing only: every number is produced by the HIP library.  There is no CPU
fallback -- if the library is missing or there is no GPU, calls raise GrebError.
"""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

from . import abi, build, workload

_lib = None


class GrebError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"greb engine error {code}: {msg}")
        self.code = code


_lib_path = build.LIB


def use_tuning_build() -> None:
    """tools/ only: load libgreb_hip_tuning.so (-DGREB_TUNING, the build in which the GREB_DEBUG_* / tile-size
    environment knobs exist) instead of the release library.  Must be called before the first engine call."""
    global _lib_path
    if _lib is not None:
        raise GrebError(-100, "use_tuning_build() after the library was loaded")
    _lib_path = build.LIB_TUNING


def lib() -> C.CDLL:
    """Load libgreb_hip.so (never builds implicitly on the GPU box; fails loudly if absent)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_lib_path):
            raise GrebError(-100, f"{_lib_path} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(_lib_path)
        L.greb_engine_last_error.restype = C.c_char_p
        L.greb_engine_last_error.argtypes = [C.c_void_p]
        L.greb_device_info.restype = C.c_char_p
        L.greb_params_default.restype = None
        abi.ens_prototypes(L)
        abi.lin_prototypes(L)
        abi.budget_prototypes(L)
        abi.gram_prototypes(L)
        abi.cross_prototypes(L)
        abi.reg_prototypes(L)
        abi.derive_prototypes(L)
        abi.noise_prototypes(L)
        _lib = L
    return _lib


EXPORTS = ["greb_params_default", "greb_engine_create", "greb_engine_flux_correction", "greb_engine_run",
           "greb_engine_get_corrections", "greb_engine_set_corrections", "greb_engine_get_state",
           "greb_engine_last_error", "greb_engine_destroy", "greb_device_info", "greb_diffusion_batched",
           "greb_advection_batched", "greb_circulation_batched", "greb_diffusion_batched_dev",
           "greb_engine_point_physics", "greb_log_exp_switches", "greb_engine_set_experiment",
           "greb_ensemble_moments_dev", "greb_ensemble_quantiles_dev", "greb_engine_set_state", "greb_release_caches", "greb_diffusion_launch_order",
           "greb_substep_launch_order", "greb_circulation_launch_plan", "greb_engine_describe",
           "greb_engine_create_members", "greb_engine_set_member_experiments", "greb_diag_create", "greb_diag_destroy",
           "greb_diag_reduce_dev", "greb_engine_run_diag", "greb_engine_run_budget", "greb_budget_name",
           "greb_member_deal_cover", "greb_member_lds_table", "greb_member_lds_map", "greb_engine_set_forcing_tables", "greb_engine_set_member_forcing",
           "greb_engine_add_boundary_set", "greb_engine_set_member_boundary", "greb_step_variant", "greb_step_variants",
           "greb_clim_create", "greb_clim_destroy", "greb_clim_add_year_dev", "greb_clim_finish_dev", "greb_engine_run_clim",
           "greb_ens_create", "greb_ens_destroy", "greb_ens_reduce_dev", "greb_engine_run_ens",
           "greb_lin_create", "greb_lin_destroy", "greb_lin_reduce_dev", "greb_engine_run_lin",
           "greb_forcing_record_offset", "greb_forcing_record_field_bytes", "greb_forcing_record_step_floats",
           "greb_forcing_record_bytes", "greb_forcing_record_field_name", "greb_engine_get_forcing_record",
           "greb_forcing_record_field_static", "greb_forcing_record_static_floats",
           "greb_diag_create_vars", "greb_clim_create_vars", "greb_budget_combine_dev", "greb_engine_run_budget_diag",
           "greb_engine_run_budget_clim", "greb_engine_run_budget_ens", "greb_engine_run_budget_lin",
           "greb_gram_create", "greb_gram_destroy", "greb_gram_reduce_dev", "greb_engine_run_gram", "greb_engine_run_budget_gram",
           "greb_cross_create", "greb_cross_destroy", "greb_cross_add_year_dev", "greb_cross_finish_dev", "greb_engine_run_cross",
           "greb_engine_run_budget_cross",
           "greb_reg_create", "greb_reg_destroy", "greb_reg_add_year_dev", "greb_reg_finish_dev", "greb_engine_run_reg",
           "greb_engine_run_budget_reg",
           "greb_derive_create", "greb_derive_destroy", "greb_derive_uses_budget", "greb_derive_apply_dev",
           "greb_engine_run_derived_diag", "greb_engine_run_derived_clim", "greb_engine_run_derived_ens", "greb_engine_run_derived_lin",
           "greb_engine_run_derived_gram", "greb_engine_run_derived_cross", "greb_engine_run_derived_reg",
           "greb_engine_set_dealing", "greb_member_chunk_table", "greb_member_queue_capacity",
           "greb_engine_set_sst_tables", "greb_engine_set_member_sst",
           "greb_engine_set_noise_tables", "greb_engine_set_member_noise", "greb_engine_get_noise"]


def _check(rc: int, h=None):
    if rc != 0:
        msg = lib().greb_engine_last_error(h)
        raise GrebError(rc, msg.decode() if msg else "")


def device_info(device: int = 0) -> dict:
    return json.loads(lib().greb_device_info(device).decode())


def budget_name(i: int) -> str | None:
    """greb_budget_name: the library's name of budget term i (abi.BUDGET_NAMES mirrors them), None outside 0 ... 12."""
    f = lib().greb_budget_name
    f.restype = C.c_char_p
    s = f(int(i))
    return None if s is None else s.decode()


def log_exp_switches(log_exp: int) -> int:
    """Process switches of the upstream variant's experiment number (greb.original.model.f90:60)."""
    f = lib().greb_log_exp_switches
    f.restype = C.c_uint
    return int(f(int(log_exp)))


def member_configs(params: abi.GrebParams, members):
    """A list of dicts -> (greb_member_config * n).  Keys: any float field of greb_params (p_emi: ten values), plus
    `switches` (GREB_X_* bits) or `log_exp` (mapped through log_exp_switches); missing keys take the engine-wide value."""
    floats = set(abi.GrebParams.PHYSICS_NAMES) | {"co2_flux"}
    arr = (abi.GrebMemberConfig * len(members))()
    for c, d in zip(arr, members):
        C.memmove(C.byref(c.p), C.byref(params), C.sizeof(abi.GrebParams))
        c.switches = 0
        if "switches" in d and "log_exp" in d:
            raise GrebError(-1, "members: give `switches` or `log_exp`, not both")
        for k, v in d.items():
            if k == "switches":
                c.switches = int(v)
            elif k == "log_exp":
                c.switches = log_exp_switches(int(v))
            elif k == "p_emi":
                if len(v) != 10:
                    raise GrebError(-1, "members: p_emi takes ten values")
                for i, x in enumerate(v):
                    c.p.p_emi[i] = float(x)
            elif k in floats:
                setattr(c.p, k, float(v))
            else:
                raise GrebError(-1, f"members: unknown key {k!r}")
    return arr


def boundary_fields(nx: int, ny: int, fields: dict) -> dict:
    """The keyword arguments of Engine.add_boundary_set, checked: names are those of greb_fields that a boundary set may
    replace (abi.BOUNDARY_FIELDS), arrays real-valued with shape [ny][nx] (z_topo, glacier) or [730][ny][nx]; returns
    them as C-contiguous float32.  None values are dropped (inherit)."""
    out = {}
    for name, x in fields.items():
        if name == "sw_solar":
            raise GrebError(-1, "add_boundary_set: sw_solar is not part of a boundary set: insolation tables are per-member "
                                "forcing (set_forcing_tables, set_member_forcing)")
        if name not in abi.BOUNDARY_FIELDS:
            raise GrebError(-1, f"add_boundary_set: unknown field {name!r} (one of {', '.join(abi.BOUNDARY_FIELDS)})")
        if x is None:
            continue
        x = np.asarray(x)
        if x.dtype.kind not in "fiu":
            raise GrebError(-1, f"add_boundary_set: {name} has dtype {x.dtype}, expected real numbers (float32)")
        want = (ny, nx) if abi.BOUNDARY_FIELDS[name] == 2 else (abi.NSTEP_YR, ny, nx)
        if x.shape != want:
            raise GrebError(-1, f"add_boundary_set: {name} has shape {x.shape}, expected {list(want)}")
        out[name] = np.ascontiguousarray(x, np.float32)
    if not out:
        raise GrebError(-1, "add_boundary_set: no field given: the set would be the engine's own data (set 0)")
    return out


def params_default() -> abi.GrebParams:
    p = abi.GrebParams()
    lib().greb_params_default(C.byref(p))
    return p


class Engine:
    """greb_engine_* handle.  Mirrors the reference's run structure: flux_correction() is
    qflux_correction (src/greb.f90:311-364), run() is the scenario loop (:228-234)."""

    def __init__(self, inp: workload.Inputs, params: abi.GrebParams | None = None, n_members: int = 1,
                 overrides=None, device: int = 0, strict: bool = False, multilaunch: bool = False,
                 row_strips: bool = False, persistent: bool | None = None, members=None):
        """members: one dict per member (member_configs: any float field of greb_params, `switches` or `log_exp`), for
        ensembles whose members differ in more than the four `overrides` slots; mutually exclusive with `overrides`.
        persistent (384-wide grids): True = the circulation call as one launch (GREB_F_PERSISTENT), False = one launch per
        sub-step (GREB_F_NO_PERSISTENT), None = the engine times both and keeps the faster."""
        L = lib()
        self.params = params or params_default()
        if members is not None:
            if overrides is not None:
                raise GrebError(-1, "Engine: give `members` or `overrides`, not both")
            members = list(members)
            n_members = len(members)
        self.nx, self.ny, self.np, self.nm = inp.nx, inp.ny, inp.nx * inp.ny, n_members
        fields, self._keep = abi.make_fields(inp)
        ov = None
        if overrides is not None:
            ov = (abi.GrebMemberOverrides * n_members)()
            for i, o in enumerate(overrides):
                for k in ("da_ice", "a_no_ice", "a_cloud", "kappa"):
                    setattr(ov[i], k, float(o.get(k, float("nan"))))
        self.h = C.c_void_p()
        flags = ((abi.F_STRICT if strict else 0) | (abi.F_MULTILAUNCH if multilaunch else 0) |
                 (abi.F_ROW_STRIPS if row_strips else 0) |
                 (0 if persistent is None else (abi.F_PERSISTENT if persistent else abi.F_NO_PERSISTENT)))
        if members is not None:
            rc = L.greb_engine_create_members(C.byref(self.params), inp.nx, inp.ny, C.byref(fields), n_members,
                                              member_configs(self.params, members), device, flags, C.byref(self.h))
        else:
            rc = L.greb_engine_create(C.byref(self.params), inp.nx, inp.ny, C.byref(fields), n_members, ov, device, flags,
                                      C.byref(self.h))
        if rc != 0:
            msg = L.greb_engine_last_error(self.h).decode()
            if self.h:
                L.greb_engine_destroy(self.h)
                self.h = None
            raise GrebError(rc, msg)

    def set_dealing(self, workgroups: int = 0, schedule: int = abi.CHUNKS_HALVING, force: bool = False) -> None:
        """greb_engine_set_dealing (fused 96x48 engine): launches of more members than `workgroups` (0: the device's compute
        units) deal (member, chunk) items to that many workgroups from a ready queue; workgroups < 0 switches dealing off;
        force deals also where the members do not outnumber the workgroups.  Results do not depend on it."""
        _check(lib().greb_engine_set_dealing(self.h, int(workgroups), int(schedule), int(bool(force))), self.h)

    def describe(self) -> dict:
        """greb_engine_describe: grid, members, arithmetic, which circulation form runs (and the trial's timings)."""
        f = lib().greb_engine_describe
        f.restype = C.c_char_p
        return json.loads(f(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            lib().greb_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def flux_correction(self, years: int) -> np.ndarray:
        yearly = np.zeros((self.nm, max(years, 1), 2), np.float32)
        _check(lib().greb_engine_flux_correction(self.h, int(years), abi.fptr(yearly)), self.h)
        return yearly[:, :years]

    def _run_arrays(self, years: int, co2_ppm):
        """What every run* call hands the library: co2 [n_members][years] and the zeroed yearly [n_members][years][2]."""
        co2 = np.ascontiguousarray(np.broadcast_to(np.asarray(co2_ppm, np.float32), (self.nm, years)))
        return co2, np.zeros((self.nm, years, 2), np.float32)

    def run(self, years: int, co2_ppm, monthly_dev_ptr: int | None = None, out: np.ndarray | None = None):
        """co2_ppm: scalar, [years] or [n_members][years].  Returns (monthly, yearly); with
        monthly_dev_ptr (a device address) the monthly means stay on the GPU and monthly is None.
        out: caller-owned host buffer for the monthly means (float32, C-contiguous, n_members*years*12*5*np
        elements -- e.g. the numpy view of a pinned torch tensor, which makes the delivery a true DMA)."""
        co2, yearly = self._run_arrays(years, co2_ppm)
        if monthly_dev_ptr is None:
            shape = (self.nm, years, 12, 5, self.ny, self.nx)
            if out is None:
                monthly = np.empty(shape, np.float32)
            else:
                if out.dtype != np.float32 or not out.flags.c_contiguous or out.size != int(np.prod(shape)):
                    raise GrebError(-1, "run: `out` must be C-contiguous float32 with n_members*years*12*5*ny*nx elements")
                monthly = out.reshape(shape)
            _check(lib().greb_engine_run(self.h, int(years), abi.fptr(co2), abi.fptr(monthly), abi.fptr(yearly), 0), self.h)
            return monthly, yearly
        _check(lib().greb_engine_run(self.h, int(years), abi.fptr(co2), C.c_void_p(monthly_dev_ptr), abi.fptr(yearly),
                                     abi.RUN_DEVICE_OUT), self.h)
        return None, yearly

    def run_budget(self, years: int, co2_ppm, want_monthly: bool = True, monthly_dev_ptr: int | None = None,
                   budget_dev_ptr: int | None = None):
        """The scenario run of run() that also hands back the monthly means of the thirteen flux terms of the update
        (abi.BUDGET_NAMES; greb_engine_run_budget).  Returns (monthly, budget, yearly) with budget
        [n_members][years][12][13][ny][nx]; monthly is None with want_monthly=False (a budget-only run).  State, clock,
        monthly and yearly are those of run() over the same years.  With budget_dev_ptr (a device address) the records
        stay on the GPU (GREB_RUN_DEVICE_OUT: monthly then goes to monthly_dev_ptr, or nowhere) and both are None."""
        co2, yearly = self._run_arrays(years, co2_ppm)
        f = lib().greb_engine_run_budget
        if budget_dev_ptr is not None:
            _check(f(self.h, int(years), abi.fptr(co2), None if monthly_dev_ptr is None else C.c_void_p(monthly_dev_ptr),
                     C.c_void_p(budget_dev_ptr), abi.fptr(yearly), abi.RUN_DEVICE_OUT), self.h)
            return None, None, yearly
        if monthly_dev_ptr is not None:
            raise GrebError(-1, "run_budget: monthly_dev_ptr needs budget_dev_ptr (one run delivers to one side)")
        monthly = np.empty((self.nm, years, 12, 5, self.ny, self.nx), np.float32) if want_monthly else None
        budget = np.empty((self.nm, years, 12, abi.NBUDGET, self.ny, self.nx), np.float32)
        _check(f(self.h, int(years), abi.fptr(co2), None if monthly is None else abi.fptr(monthly), abi.fptr(budget),
                 abi.fptr(yearly), 0), self.h)
        return monthly, budget, yearly

    def _reduced(self, name: str, records, co2, plan, *args):
        """Call the reduced run `name` ("diag", "clim", "ens", "lin", "gram", "cross", "reg") over `records`: "state" -- the year's five state
        records (greb_engine_run_<name>) --, "budget" -- its thirteen flux terms -- or a budget.Combo -- sums of them
        (greb_engine_run_budget_<name>) -- or a derive.Program -- per-point expressions of either
        (greb_engine_run_derived_<name>).  `args`: what follows the plan in the C call."""
        from . import budget, derive
        if isinstance(records, str) and records == "state":
            _check(getattr(lib(), "greb_engine_run_" + name)(self.h, int(co2.shape[1]), abi.fptr(co2), plan.h, *args), self.h)
            return
        if isinstance(records, derive.Program):
            _check(getattr(lib(), "greb_engine_run_derived_" + name)(self.h, int(co2.shape[1]), abi.fptr(co2),
                                                                     records.handle(self.nx, self.ny), plan.h, *args), self.h)
            return
        cb = budget.as_combo(records)
        _check(getattr(lib(), "greb_engine_run_budget_" + name)(self.h, int(co2.shape[1]), abi.fptr(co2),
                                                                None if cb is None else abi.fptr(cb.matrix),
                                                                0 if cb is None else len(cb.names), plan.h, *args), self.h)

    def run_diag(self, years: int, co2_ppm, plan, what: int | None = None, records="state"):
        """The scenario run of run() that hands back only the reduced products of `plan` (diag.Plan): regional means,
        zonal means and annual-mean maps made on the device year by year (greb_engine_run_diag).  what: abi.D_* bits,
        default all three.  Returns a diag.Result (regions, zonal, annual, yearly, region names; a product that was
        not selected is None).  State, clock and yearly are those of run() over the same years.
        records: "state" (the five state records), "budget" (the thirteen flux terms of run_budget), a budget.combo(...)
        (sums of them) or a derive.program(...) (per-point expressions of either); the plan's n_vars must be that count, which stands where the shapes say 5, and the result
        carries the variables' names (Result.vars)."""
        from . import budget, diag
        what = diag.ALL if what is None else int(what)
        co2, yearly = self._run_arrays(years, co2_ppm)
        names = budget.record_names(records)
        nv = len(names)
        regions = np.empty((self.nm, years, 12, nv, plan.nr), np.float32) if what & abi.D_REGIONS else None
        zonal = np.empty((self.nm, years, 12, nv, self.ny), np.float32) if what & abi.D_ZONAL else None
        annual = np.empty((self.nm, years, nv, self.ny, self.nx), np.float32) if what & abi.D_ANNUAL else None
        ptr = [None if a is None else abi.fptr(a) for a in (regions, zonal, annual)]
        self._reduced("diag", records, co2, plan, C.c_uint(what), *ptr, abi.fptr(yearly))
        return diag.Result(regions, zonal, annual, yearly, plan.names, names)

    def run_clim(self, years: int, co2_ppm, plan, periods, records="state"):
        """The scenario run of run() that hands back only the climatology products of `plan` (clim.Plan) over `periods`, a
        list of (first_year, n_years) inside this call's years -- ascending, not overlapping; years outside every period
        are integrated but not summed (greb_engine_run_clim).  Returns a clim.Result of arrays [n_members][n_periods]...
        (a product the plan does not select is None).  State, clock and yearly are those of run() over the same years.
        records: as in run_diag."""
        from . import budget, clim
        co2, yearly = self._run_arrays(years, co2_ppm)
        names = budget.record_names(records)
        per = np.ascontiguousarray(periods, np.int32).reshape(-1, 2)
        first, count = np.ascontiguousarray(per[:, 0]), np.ascontiguousarray(per[:, 1])
        out = clim.empty_products(plan.what, (self.nm, len(per)), self.ny, self.nx, len(names))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        self._reduced("clim", records, co2, plan, len(per), ip(first), ip(count),
                      *[None if a is None else abi.fptr(a) for a in out], abi.fptr(yearly))
        return clim.Result(*out, yearly, names)

    def run_ens(self, years: int, co2_ppm, plan, records="state"):
        """The scenario run of run() that hands back only the statistics across the members of each group of `plan`
        (ens.Plan), of every monthly record of every year: made on the device year by year, of the records or of each
        member's difference to its control member (greb_engine_run_ens).  Returns an ens.Result of arrays
        [n_groups][years][12][5][ny][nx], quant [n_groups][years][n_probs][12][5][ny][nx] (a product the plan does not
        select is None).  State, clock and yearly are those of run() over the same years.
        records: as in run_diag (an ens plan serves any variable count)."""
        from . import budget, ens
        co2, yearly = self._run_arrays(years, co2_ppm)
        names = budget.record_names(records)
        out = ens.empty_products(plan, (years,), (12, len(names), self.ny, self.nx))
        self._reduced("ens", records, co2, plan, *[None if a is None else abi.fptr(a) for a in out], abi.fptr(yearly))
        return ens.Result(*out, yearly, names)

    def run_lin(self, years: int, co2_ppm, plan, records="state"):
        """The scenario run of run() that hands back only the linear model of `plan` (lin.Plan) across the members, of every
        monthly record of every year: made on the device year by year (greb_engine_run_lin).  Returns a lin.Result: coef
        [n_terms][years][12][5][ny][nx] -- effects, slopes, whatever the plan's weights state -- and rss
        [years][12][5][ny][nx], the residual sum of squares of the fit (a product the plan does not select is None).
        State, clock and yearly are those of run() over the same years.  records: as in run_diag (a lin plan serves any
        variable count)."""
        from . import budget, lin
        co2, yearly = self._run_arrays(years, co2_ppm)
        names = budget.record_names(records)
        coef, rss = lin.empty_products(plan, (years,), (12, len(names), self.ny, self.nx))
        self._reduced("lin", records, co2, plan, None if coef is None else abi.fptr(coef), None if rss is None else abi.fptr(rss),
                      abi.fptr(yearly))
        return lin.Result(coef, rss, yearly, names)

    def run_gram(self, years: int, co2_ppm, plan, records="state"):
        """The scenario run of run() that hands back only the Gram matrices of `plan` (gram.Plan) across the members: per
        year and block of records G[a][c] = sum v_a v_c in float64, made on the device year by year (greb_engine_run_gram).
        Returns a gram.Result: G [years][n_blocks][U][U].  State, clock and yearly are those of run() over the same years.
        records: as in run_diag; the plan's n_records must be 12 times that variable count."""
        from . import budget, gram
        co2, yearly = self._run_arrays(years, co2_ppm)
        names = budget.record_names(records)
        G = np.empty((years, plan.nb, plan.U, plan.U), np.float64)
        self._reduced("gram", records, co2, plan, G.ctypes.data_as(C.POINTER(C.c_double)), abi.fptr(yearly))
        return gram.Result(G, yearly, names)

    def run_cross(self, years: int, co2_ppm, plan, records="state"):
        """The scenario run of run() that hands back only the crossing products of `plan` (cross.Plan): per member, event and
        point the first and the last year that hits the event's threshold, the year from which it holds to the end, the
        number of years that hit, the peak and its year, and per year the share of each group's members that hit -- made on
        the device year by year (greb_engine_run_cross).  Years are 0-based within this call (cross.as_year turns them into
        calendar years).  Returns a cross.Result: the maps [n_members][n_events][ny][nx], fraction
        [years][n_groups][n_events][ny][nx] (a product the plan does not select is None).  State, clock and yearly are those
        of run() over the same years.  records: as in run_diag; the plan's n_vars must be that variable count."""
        from . import budget, cross
        co2, yearly = self._run_arrays(years, co2_ppm)
        names = budget.record_names(records)
        out = cross.empty_products(plan, years)
        i32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
        f32 = lambda a: None if a is None else abi.fptr(a)
        self._reduced("cross", records, co2, plan, i32(out[0]), i32(out[1]), i32(out[2]), i32(out[3]), f32(out[4]), i32(out[5]),
                      f32(out[6]), abi.fptr(yearly))
        return cross.Result(*out, yearly, names)

    def run_reg(self, years: int, co2_ppm, plan, records="state"):
        """The scenario run of run() that hands back only the regression products of `plan` (regress.Plan): per member, term
        and point the slope, the intercept and R2 of the least-squares line of the term's yearly quantity on the member's own
        yearly index -- a regional mean of its records, e.g. its annual global-mean warming -- and the index series itself,
        made on the device year by year (greb_engine_run_reg).  Returns a regress.Result: the maps
        [n_members][n_terms][ny][nx], index [n_members][years][n_indices] (a product the plan does not select is None).  State,
        clock and yearly are those of run() over the same years.  records: as in run_diag; the plan's n_vars must be that
        variable count."""
        from . import budget, regress
        co2, yearly = self._run_arrays(years, co2_ppm)
        names = budget.record_names(records)
        out = regress.empty_products(plan, years)
        self._reduced("reg", records, co2, plan, *[None if a is None else abi.fptr(a) for a in out], abi.fptr(yearly))
        return regress.Result(*out, yearly, names)

    def state(self, member: int = 0) -> np.ndarray:
        s = np.empty((5, self.ny, self.nx), np.float32)
        _check(lib().greb_engine_get_state(self.h, member, abi.fptr(s)), self.h)
        return s

    def get_corrections(self, member: int = 0):
        corr = np.empty((3, abi.NSTEP_YR, self.ny, self.nx), np.float32)
        st = np.empty((5, self.ny, self.nx), np.float32)
        _check(lib().greb_engine_get_corrections(self.h, member, abi.fptr(corr), abi.fptr(st)), self.h)
        return corr, st

    def set_corrections(self, corr, state5, member: int = -1):
        """Either argument may be None (left unchanged); member -1 = every member."""
        corr = None if corr is None else np.ascontiguousarray(corr, np.float32)
        state5 = None if state5 is None else np.ascontiguousarray(state5, np.float32)
        _check(lib().greb_engine_set_corrections(self.h, member, None if corr is None else abi.fptr(corr),
                                                 None if state5 is None else abi.fptr(state5)), self.h)

    def set_experiment(self, switches: int):
        """Sensitivity-experiment switches (abi.X_*; log_exp_switches() maps the original's log_exp)."""
        _check(lib().greb_engine_set_experiment(self.h, C.c_uint(int(switches))), self.h)

    def set_member_experiments(self, switches):
        """One switch word per member.  Members that shared one flux-correction set and now differ each get a copy of
        it (spin up once under the complete model, then let the members diverge)."""
        sw = np.ascontiguousarray(switches, np.uint32)
        if sw.shape != (self.nm,):
            raise GrebError(-1, f"set_member_experiments: {self.nm} switch words expected")
        _check(lib().greb_engine_set_member_experiments(self.h, sw.ctypes.data_as(C.POINTER(C.c_uint32))), self.h)

    def set_forcing_tables(self, space, season=None, solar=None):
        """The forcing tables every member shares (greb_engine_set_forcing_tables; replaces the ones set before):
        space [n_patterns][ny][nx] CO2 weights in [0, 1] (or None: no patterns), season [n_patterns][730] their seasonal
        factor in [0, 1] (None: 1 everywhere), solar [n_solar][730][ny] insolation tables in W/m2 (None: none)."""
        def arr(x, tail, what):
            if x is None:
                return None
            x = np.ascontiguousarray(x, np.float32)
            if x.ndim == len(tail):
                x = x[None]
            if x.shape[1:] != tail:
                raise GrebError(-1, f"set_forcing_tables: {what} has shape {x.shape}, expected [n]{list(tail)}")
            return x
        space = arr(space, (self.ny, self.nx), "space")
        season = arr(season, (abi.NSTEP_YR,), "season")
        solar = arr(solar, (abi.NSTEP_YR, self.ny), "solar")
        if season is not None and (space is None or len(season) != len(space)):
            raise GrebError(-1, "set_forcing_tables: season needs one row of 730 per pattern of space")
        ptr = lambda x: None if x is None else abi.fptr(x)
        _check(lib().greb_engine_set_forcing_tables(self.h, 0 if space is None else len(space), ptr(space), ptr(season),
                                                    0 if solar is None else len(solar), ptr(solar)), self.h)

    def set_member_forcing(self, forcing):
        """One dict per member (greb_engine_set_member_forcing), keys co2_pattern (default -1: none), co2_ref (340),
        solar_table (-1: the engine's own), solar_scale (1); None: no member is forced.  Acts in run / run_budget /
        run_diag from the next call; flux_correction ignores it."""
        if forcing is None:
            _check(lib().greb_engine_set_member_forcing(self.h, None), self.h)
            return
        forcing = list(forcing)
        if len(forcing) != self.nm:
            raise GrebError(-1, f"set_member_forcing: {self.nm} entries expected")
        arr = (abi.GrebMemberForcing * self.nm)()
        for f, d in zip(arr, forcing):
            d = dict(d or {})
            f.co2_pattern = int(d.pop("co2_pattern", -1)); f.co2_ref = float(d.pop("co2_ref", 340.0))
            f.solar_table = int(d.pop("solar_table", -1)); f.solar_scale = float(d.pop("solar_scale", 1.0))
            if d:
                raise GrebError(-1, f"set_member_forcing: unknown key {sorted(d)[0]!r}")
        _check(lib().greb_engine_set_member_forcing(self.h, arr), self.h)

    def set_sst_tables(self, anom, weight=None, season=None):
        """The prescribed-SST tables every member shares (greb_engine_set_sst_tables; replaces the ones set before):
        anom [n_patterns][ny][nx] anomalies in K (or None: no patterns), weight [n_patterns][ny][nx] nudging weights in
        [0, 1] (None: 1 everywhere), season [n_patterns][730] the anomalies' seasonal factor (None: 1 everywhere)."""
        def arr(x, tail, what):
            if x is None:
                return None
            x = np.ascontiguousarray(x, np.float32)
            if x.ndim == len(tail):
                x = x[None]
            if x.shape[1:] != tail:
                raise GrebError(-1, f"set_sst_tables: {what} has shape {x.shape}, expected [n]{list(tail)}")
            return x
        anom = arr(anom, (self.ny, self.nx), "anom")
        weight = arr(weight, (self.ny, self.nx), "weight")
        season = arr(season, (abi.NSTEP_YR,), "season")
        for x, what in ((weight, "weight"), (season, "season")):
            if x is not None and (anom is None or len(x) != len(anom)):
                raise GrebError(-1, f"set_sst_tables: {what} needs one entry per pattern of anom")
        ptr = lambda x: None if x is None else abi.fptr(x)
        _check(lib().greb_engine_set_sst_tables(self.h, 0 if anom is None else len(anom), ptr(anom), ptr(weight), ptr(season)), self.h)

    def set_member_sst(self, sst):
        """One dict per member (greb_engine_set_member_sst), keys pattern (default -1: none, the ocean surface is free)
        and amp (1); None: no member is prescribed.  Acts in every run* call from the next one; flux_correction ignores it."""
        if sst is None:
            _check(lib().greb_engine_set_member_sst(self.h, None), self.h)
            return
        sst = list(sst)
        if len(sst) != self.nm:
            raise GrebError(-1, f"set_member_sst: {self.nm} entries expected")
        arr = (abi.GrebMemberSst * self.nm)()
        for s, d in zip(arr, sst):
            d = dict(d or {})
            s.pattern = int(d.pop("pattern", -1)); s.amp = float(d.pop("amp", 1.0))
            if d:
                raise GrebError(-1, f"set_member_sst: unknown key {sorted(d)[0]!r}")
        _check(lib().greb_engine_set_member_sst(self.h, arr), self.h)

    def set_noise_tables(self, sigma, season=None, cell=(1, 1), hold=1):
        """The stochastic heat-flux tables every member shares (greb_engine_set_noise_tables; replaces the ones set before):
        sigma [n_patterns][ny][nx] standard deviations in W/m2 (or None: no patterns), season [n_patterns][730] their seasonal
        factor (None: 1 everywhere), cell (cell_x, cell_y) and hold for all patterns, or one pair / one value per pattern."""
        if sigma is None:
            _check(lib().greb_engine_set_noise_tables(self.h, 0, None, None, None, None, None), self.h)
            return
        sigma = np.ascontiguousarray(sigma, np.float32)
        if sigma.ndim == 2:
            sigma = sigma[None]
        if sigma.shape[1:] != (self.ny, self.nx):
            raise GrebError(-1, f"set_noise_tables: sigma has shape {sigma.shape}, expected [n]{[self.ny, self.nx]}")
        n = len(sigma)
        if season is not None:
            season = np.ascontiguousarray(season, np.float32)
            if season.ndim == 1:
                season = season[None]
            if season.shape != (n, abi.NSTEP_YR):
                raise GrebError(-1, f"set_noise_tables: season has shape {season.shape}, expected {[n, abi.NSTEP_YR]}")
        cell = np.asarray(cell, np.int32)
        if cell.ndim == 1:
            cell = np.broadcast_to(cell, (n, 2))
        hold = np.broadcast_to(np.asarray(hold, np.int32), (n,)) if np.ndim(hold) == 0 else np.asarray(hold, np.int32)
        if cell.shape != (n, 2) or hold.shape != (n,):
            raise GrebError(-1, "set_noise_tables: cell needs one (cell_x, cell_y) and hold one value, for all patterns or per pattern")
        cx, cy, hold = (np.ascontiguousarray(a, np.int32) for a in (cell[:, 0], cell[:, 1], hold))
        iptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        _check(lib().greb_engine_set_noise_tables(self.h, n, abi.fptr(sigma), None if season is None else abi.fptr(season), iptr(cx), iptr(cy),
                                                  iptr(hold)), self.h)

    def set_member_noise(self, noise):
        """One dict per member (greb_engine_set_member_noise), keys pattern (default -1: none, the member is deterministic),
        amp (1) and seed (0; a 64-bit integer, noise.seeds makes distinct ones); None: no member is noisy.  Acts in every run*
        call from the next one; flux_correction ignores it."""
        if noise is None:
            _check(lib().greb_engine_set_member_noise(self.h, None), self.h)
            return
        noise = list(noise)
        if len(noise) != self.nm:
            raise GrebError(-1, f"set_member_noise: {self.nm} entries expected")
        arr = (abi.GrebMemberNoise * self.nm)()
        for s, d in zip(arr, noise):
            d = dict(d or {})
            seed = int(d.pop("seed", 0)) & 0xFFFFFFFFFFFFFFFF
            s.pattern = int(d.pop("pattern", -1)); s.amp = float(d.pop("amp", 1.0))
            s.seed_lo, s.seed_hi = seed & 0xFFFFFFFF, seed >> 32
            if d:
                raise GrebError(-1, f"set_member_noise: unknown key {sorted(d)[0]!r}")
        _check(lib().greb_engine_set_member_noise(self.h, arr), self.h)

    def noise(self, member: int, step: int) -> np.ndarray:
        """The heat flux N [ny][nx] in W/m2 that noisy member `member` takes at scenario step `step` (0-based, any step >= 0;
        greb_engine_get_noise): evaluated on the device by the function the step kernels call."""
        out = np.empty((self.ny, self.nx), np.float32)
        _check(lib().greb_engine_get_noise(self.h, int(member), int(step), abi.fptr(out)), self.h)
        return out

    def add_boundary_set(self, **fields) -> int:
        """A boundary set (greb_engine_add_boundary_set): the given fields -- keyword names as in greb_fields, arrays
        [ny][nx] (z_topo, glacier) or [730][ny][nx] -- replace the engine's own for the members that name the set; the
        others are inherited.  Returns the set's id, 1 ... abi.MAX_BOUNDARY_SETS (0 is the engine's own data)."""
        arrs = boundary_fields(self.nx, self.ny, fields)
        f = abi.GrebFields()
        for name, x in arrs.items():
            setattr(f, name, abi.fptr(x))
        sid = C.c_int(0)
        _check(lib().greb_engine_add_boundary_set(self.h, C.byref(f), C.byref(sid)), self.h)
        return int(sid.value)

    def set_member_boundary(self, sets, reinit: bool = False):
        """One set id per member (greb_engine_set_member_boundary; 0 = the engine's own data, None = every member 0),
        from the next flux_correction / run call.  reinit: every member also starts from the initial state of its set
        (call it before flux_correction); without it the state stays -- spin up under the control data, then change a
        member's boundary data.  Members whose sets differ each get their own flux-correction set."""
        flags = abi.BS_REINIT if reinit else 0
        if sets is None:
            _check(lib().greb_engine_set_member_boundary(self.h, None, C.c_uint(flags)), self.h)
            return
        ids = np.ascontiguousarray(sets, np.int32)
        if ids.shape != (self.nm,):
            raise GrebError(-1, f"set_member_boundary: {self.nm} set ids expected")
        _check(lib().greb_engine_set_member_boundary(self.h, ids.ctypes.data_as(C.POINTER(C.c_int32)), C.c_uint(flags)), self.h)

    def forcing_record(self, step: int, set_id: int = 0) -> np.ndarray:
        """Debug read-back (greb_engine_get_forcing_record): step `step` (1 ... 730) of the packed forcing record of
        boundary set `set_id` together with the record's static part, as [row][field][longitude] (fields:
        forcing_record_layout().names)."""
        lay = forcing_record_layout()
        out = np.empty(lay.static_floats + lay.step_floats, np.float32)
        _check(lib().greb_engine_get_forcing_record(self.h, int(set_id), int(step), abi.fptr(out)), self.h)
        ns = sum(lay.static)
        return np.concatenate([out[:lay.static_floats].reshape(lay.ny, ns, lay.nx),
                               out[lay.static_floats:].reshape(lay.ny, len(lay.names) - ns, lay.nx)], axis=1)

    def point_physics(self, ityr: int, co2: float, in5) -> np.ndarray:
        in5 = np.ascontiguousarray(in5, np.float32)
        out = np.empty((15, self.ny, self.nx), np.float32)
        _check(lib().greb_engine_point_physics(self.h, int(ityr), C.c_float(co2), abi.fptr(in5), abi.fptr(out)), self.h)
        return out


POINT_FIELDS = ("albedo", "sw", "LWsurf", "LWair_down", "em", "Q_sens", "Qlat", "Qlat_air", "dq_eva", "dq_rain",
                "dT_ocean", "dTo", "cap_surf_new")


def _batched(fn_name, params, arrays, strict, device):
    arrs = [np.ascontiguousarray(a, np.float32) for a in arrays]
    shape = arrs[0].shape
    if arrs[0].ndim == 2:
        arrs = [a[None] for a in arrs]
    b, ny, nx = arrs[0].shape
    out = np.empty((b, ny, nx), np.float32)
    p = params or params_default()
    fn = getattr(lib(), fn_name)
    _check(fn(C.byref(p), nx, ny, b, *[abi.fptr(a) for a in arrs], abi.fptr(out), int(bool(strict)), device))
    return out.reshape(shape)


def diffusion(T1, wz, params=None, strict=False, device=0):
    """Batched mirror of diffusion(T1,dX,h_scl,wz), src/greb.f90:556-723."""
    return _batched("greb_diffusion_batched", params, (T1, wz), strict, device)


def advection(T1, wz, u, v, params=None, strict=False, device=0):
    """Batched mirror of advection(T1,dX,h_scl,wz), src/greb.f90:726-915 (u, v: raw wind slice)."""
    return _batched("greb_advection_batched", params, (T1, wz, u, v), strict, device)


def circulation(X, wz, u, v, params=None, strict=False, device=0):
    """Batched mirror of circulation(X_in,dX,h_scl,wz), src/greb.f90:528-553."""
    return _batched("greb_circulation_batched", params, (X, wz, u, v), strict, device)


def diffusion_launch_order(params, nx, ny, batch):
    """Host-only diagnostic: the task list of the 384-wide diffusion sweep, arrays (field, k0, k1, up); empty when the
    grid does not take that kernel (include/greb_engine.h: greb_diffusion_launch_order)."""
    params = params if params is not None else params_default()
    f = lib().greb_diffusion_launch_order
    n = f(C.byref(params), nx, ny, batch, None, None, None, None, 0)
    if n < 0:
        _check(n)
    out = [np.zeros(n, np.int32) for _ in range(4)]
    if n:
        ptr = [a.ctypes.data_as(C.POINTER(C.c_int)) for a in out]
        assert f(C.byref(params), nx, ny, batch, *ptr, n) == n
    return out


def substep_launch_order(params, nx, ny, n_members, kappa=None):
    """Host-only diagnostic: the task list of the engine's row-strip circulation sub-step, arrays (field, k0, k1) with
    field = 2 * member + tracer (include/greb_engine.h: greb_substep_launch_order)."""
    params = params if params is not None else params_default()
    kap = None if kappa is None else np.ascontiguousarray(kappa, np.float32)
    kp = None if kap is None else kap.ctypes.data_as(C.POINTER(C.c_float))
    f = lib().greb_substep_launch_order
    n = f(C.byref(params), nx, ny, n_members, kp, None, None, None, 0)
    if n < 0:
        _check(n)
    out = [np.zeros(n, np.int32) for _ in range(3)]
    if n:
        ptr = [a.ctypes.data_as(C.POINTER(C.c_int)) for a in out]
        assert f(C.byref(params), nx, ny, n_members, kp, *ptr, n) == n
    return out


def member_chunk_table(schedule: int = abi.CHUNKS_HALVING, nsteps: int = abi.NSTEP_YR) -> list[int]:
    """Host only: the chunks a dealt launch of the fused member kernel cuts `nsteps` steps into, as the index one past each
    chunk's last step (include/greb_engine.h: greb_member_chunk_table)."""
    end = (C.c_int * abi.MAX_CHUNKS)()
    n = lib().greb_member_chunk_table(int(schedule), int(nsteps), end, abi.MAX_CHUNKS)
    if n < 0:
        _check(n)
    return [int(end[i]) for i in range(n)]


def member_queue_capacity(members: int, schedule: int = abi.CHUNKS_HALVING, nsteps: int = abi.NSTEP_YR) -> int:
    """Host only: the item words of the ready queue of such a launch of `members` members (greb_member_queue_capacity)."""
    f = lib().greb_member_queue_capacity
    f.restype = C.c_longlong
    n = int(f(int(members), int(schedule), int(nsteps)))
    if n < 0:
        _check(n)
    return n


def member_deal_cover(strict=False):
    """Host-only diagnostic: how often a sub-step of the fused 96x48 member kernel computes each row-quad, int array
    (48, 24) (include/greb_engine.h: greb_member_deal_cover)."""
    out = np.zeros((48, 24), np.int32)
    _check(lib().greb_member_deal_cover(int(bool(strict)), out.ctypes.data_as(C.POINTER(C.c_int))))
    return out


LDS_KINDS = ("column", "side", "wind", "store", "const")


def member_lds_map():
    """greb_member_lds_map as a dict: RS (row stride) and the float offsets at which X0, X1, W, WX, WY, ROWK begin; END."""
    w = (C.c_int * 8)()
    _check(lib().greb_member_lds_map(w))
    return dict(zip(("RS", "X0", "X1", "W", "WX", "WY", "ROWK", "END"), (int(x) for x in w)))


def member_lds_table(strict=False):
    """Host-only diagnostic: the LDS accesses of the bulk waves in one sub-step of the fused 96x48 member kernel, int array
    (n, 7): wave, pass slot, instruction, lane, kind (index into LDS_KINDS), bytes per lane, float offset or -1
    (include/greb_engine.h: greb_member_lds_table); member_lds_map() says where the arrays lie."""
    f = lib().greb_member_lds_table
    n = f(int(bool(strict)), None, 0)
    if n < 0:
        _check(n)
    out = np.zeros((n, 7), np.int32)
    assert f(int(bool(strict)), out.ctypes.data_as(C.POINTER(C.c_int)), n) == n
    return out


class RecordLayout:
    """forcing_record_layout(): the packed forcing record of the FAST fused member kernel as the library lays it out."""

    def __init__(self, names, static, offsets, field_bytes, static_floats, step_floats, record_bytes):
        self.names, self.static, self.offsets, self.field_bytes = names, static, offsets, field_bytes
        self.static_floats, self.step_floats, self.record_bytes = static_floats, step_floats, record_bytes
        self.ny, _, self.nx = offsets.shape


def forcing_record_layout(nx: int = 96, ny: int = 48) -> RecordLayout:
    """Host-only diagnostic (include/greb_engine.h: greb_forcing_record_*): field names, which of them are static, the
    offset in floats of every (row, field, longitude) inside the field's part (the static part or one step's slice) as an
    int64 array [ny][fields][nx], every field's immediate offset in bytes, the floats of the static part and of a slice
    and the bytes of a record."""
    L = lib()
    for f in (L.greb_forcing_record_offset, L.greb_forcing_record_field_bytes, L.greb_forcing_record_static_floats,
              L.greb_forcing_record_step_floats, L.greb_forcing_record_bytes):
        f.restype = C.c_longlong
    L.greb_forcing_record_field_name.restype = C.c_char_p
    names = []
    while L.greb_forcing_record_field_name(len(names)) is not None:
        names.append(L.greb_forcing_record_field_name(len(names)).decode())
    nf = len(names)
    off = np.array([[[L.greb_forcing_record_offset(k, f, i) for i in range(nx)] for f in range(nf)] for k in range(ny)], np.int64)
    return RecordLayout(tuple(names), tuple(bool(L.greb_forcing_record_field_static(f)) for f in range(nf)), off,
                        [int(L.greb_forcing_record_field_bytes(f)) for f in range(nf)], int(L.greb_forcing_record_static_floats()),
                        int(L.greb_forcing_record_step_floats()), int(L.greb_forcing_record_bytes()))


def step_variant(flux_phase=False, switches=False, budget=False, forced=False, on_sets=False):
    """Host-only diagnostic: the variant mask of the step kernels a launch with these properties takes, or None where no
    launch carries the combination (include/greb_engine.h: greb_step_variant)."""
    v = C.c_uint(0xFFFFFFFF)
    rc = lib().greb_step_variant(int(bool(flux_phase)), int(bool(switches)), int(bool(budget)), int(bool(forced)),
                                 int(bool(on_sets)), C.byref(v))
    return v.value if rc == 0 else None


def step_variants():
    """Host-only diagnostic: the variant masks that are built (include/greb_engine.h: greb_step_variants)."""
    n = lib().greb_step_variants(None, 0)
    out = (C.c_uint * n)()
    assert lib().greb_step_variants(out, n) == n
    return list(out)


def circulation_launch_plan(params, nx, ny, n_members, kappa=None, slots=2048):
    """Host-only diagnostic: the tasks of the one-launch circulation call for `slots` wavefront slots: arrays
    (field, k0, k1, chain, dep[n][4]) (include/greb_engine.h: greb_circulation_launch_plan)."""
    params = params if params is not None else params_default()
    kap = None if kappa is None else np.ascontiguousarray(kappa, np.float32)
    kp = None if kap is None else kap.ctypes.data_as(C.POINTER(C.c_float))
    f = lib().greb_circulation_launch_plan
    n = f(C.byref(params), nx, ny, n_members, kp, slots, None, None, None, None, None, 0)
    if n < 0:
        _check(n)
    out = [np.zeros(n, np.int32) for _ in range(4)] + [np.zeros((n, 4), np.int32)]
    if n:
        ptr = [a.ctypes.data_as(C.POINTER(C.c_int)) for a in out]
        assert f(C.byref(params), nx, ny, n_members, kp, slots, *ptr, n) == n
    return out


def diffusion_dev(params, nx, ny, batch, T1_ptr, wz_ptr, dX_ptr, strict=False, sweeps=1, stream=0):
    """Device-pointer diffusion sweeps for the roofline bench (no sync)."""
    _check(lib().greb_diffusion_batched_dev(C.byref(params), nx, ny, batch, C.c_void_p(T1_ptr), C.c_void_p(wz_ptr),
                                            C.c_void_p(dX_ptr), int(bool(strict)), int(sweeps), C.c_void_p(stream)))
