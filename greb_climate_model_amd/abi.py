"""ctypes mirror of include/greb_engine.h (structs + defaults).  Pure host-side plumbing."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

NSTEP_YR = 730
NVAR_OUT = 5
F_STRICT = 1
F_MULTILAUNCH = 2
F_ROW_STRIPS = 4
F_NO_PERSISTENT = 8
F_PERSISTENT = 16
RUN_DEVICE_OUT = 1
MAX_CHUNKS, CHUNKS_HALVING, CHUNKS_EQUAL, CHUNKS_QUARTERS = 10, 0, 1, 2  # GREB_MAX_CHUNKS, GREB_CHUNKS_* of include/greb_engine.h
D_REGIONS, D_ZONAL, D_ANNUAL = 1, 2, 4  # reduced-output products, GREB_D_* of include/greb_engine.h
D_MAX_REGIONS = 15
C_MEAN, C_SEASONS, C_TREND, C_RESPONSE = 1, 2, 4, 8  # climatology products, GREB_C_* of include/greb_engine.h
S_MEAN, S_VAR, S_RANGE, S_QUANTILES = 1, 2, 4, 8  # ensemble-output products, GREB_S_* of include/greb_engine.h
ENS_MAX_GROUPS, ENS_MAX_PROBS, ENS_MAX_SORTED = 64, 16, 4096  # GREB_ENS_MAX_*
L_COEF, L_RSS = 1, 2  # linear-model products, GREB_L_* of include/greb_engine.h
LIN_MAX_TERMS = 64    # GREB_LIN_MAX_TERMS
GRAM_MAX_BLOCKS, GRAM_MAX_USED = 16, 1024  # GREB_GRAM_MAX_*: blocks of records and used members of a covariance plan
# the names of the switches, GREB_X_* of include/greb_engine.h, bit 0 first
X_NAMES = ("GREB_X_NO_ICE", "GREB_X_NO_HYDRO", "GREB_X_NO_DEEP_OCEAN", "GREB_X_LW_LINEAR_VAPOR", "GREB_X_NO_CIRCULATION",
           "GREB_X_NO_VAPOR_TRANSPORT", "GREB_X_VAPOR_DIFFUSION_ONLY", "GREB_X_SST_PLUS1")
# budget output, GREB_NBUDGET / GREB_B_* of include/greb_engine.h: the flux terms of the update in its order, sign and unit
BUDGET_NAMES = ("sw", "LW_surf", "LWair_down", "LW_abs", "Q_sens", "Q_lat", "Q_lat_air", "dq_eva", "dq_rain", "dT_ocean",
                "dTo", "dTa_crcl", "dq_crcl")
NBUDGET = len(BUDGET_NAMES)
(B_SW, B_LW_SURF, B_LWAIR_DOWN, B_LW_ABS, B_Q_SENS, B_Q_LAT, B_Q_LAT_AIR, B_DQ_EVA, B_DQ_RAIN, B_DT_OCEAN, B_DTO,
 B_DTA_CRCL, B_DQ_CRCL) = range(NBUDGET)
JDAY_MON = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)  # src/greb.f90:42
# sensitivity-experiment switches, GREB_X_* of include/greb_engine.h
X_NO_ICE, X_NO_HYDRO, X_NO_DEEP_OCEAN, X_LW_LINEAR_VAPOR = 1, 2, 4, 8
X_NO_CIRCULATION, X_NO_VAPOR_TRANSPORT, X_VAPOR_DIFFUSION_ONLY, X_SST_PLUS1 = 16, 32, 64, 128

c_float_p = C.POINTER(C.c_float)

_PHYS = ["pi", "sig", "rho_ocean", "rho_land", "rho_air", "cp_ocean", "cp_land", "cp_air", "eps",
         "d_ocean", "d_land", "d_air", "ct_sens", "da_ice", "a_no_ice", "a_cloud",
         "Tl_ice1", "Tl_ice2", "To_ice1", "To_ice2",
         "co_turb", "kappa", "ce", "cq_latent", "cq_rain", "z_air", "z_vapor", "r_qviwv"]


class GrebParams(C.Structure):
    """struct greb_params: physics_par in declaration order (src/greb.f90:68-101,128-132)."""
    _fields_ = ([(n, C.c_float) for n in _PHYS] + [("p_emi", C.c_float * 10), ("co2_flux", C.c_float),
                ("ipx", C.c_int32), ("ipy", C.c_int32), ("year0", C.c_int32),
                ("dt", C.c_int32), ("dt_crcl", C.c_int32)])

    PHYSICS_NAMES = tuple(_PHYS)


class GrebFields(C.Structure):
    _fields_ = [(n, c_float_p) for n in ("z_topo", "glacier", "sw_solar", "tclim", "qclim", "uclim",
                                         "vclim", "mldclim", "cldclim", "swetclim")]


class GrebMemberOverrides(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("da_ice", "a_no_ice", "a_cloud", "kappa")]


class GrebMemberConfig(C.Structure):
    """struct greb_member_config: a member as a full namelist plus its GREB_X_* switches."""
    _fields_ = [("p", GrebParams), ("switches", C.c_uint32)]


MAX_BOUNDARY_SETS = 16  # GREB_MAX_BOUNDARY_SETS: boundary sets of one engine besides its own data (set 0)
BS_REINIT = 1           # GREB_BS_REINIT: set_member_boundary also puts every member into the initial state of its set
# the fields of greb_fields a boundary set may replace, with their rank (sw_solar is forcing, not boundary data)
BOUNDARY_FIELDS = {"z_topo": 2, "glacier": 2, "tclim": 3, "qclim": 3, "uclim": 3, "vclim": 3, "mldclim": 3, "cldclim": 3,
                   "swetclim": 3}
MAX_FORCING_TABLES = 16  # GREB_MAX_FORCING_TABLES: CO2 patterns, and insolation tables, of one engine


class GrebMemberForcing(C.Structure):
    """struct greb_member_forcing: a member's CO2 pattern (-1: none) and reference, insolation table (-1: the engine's) and scale."""
    _fields_ = [("co2_pattern", C.c_int32), ("co2_ref", C.c_float), ("solar_table", C.c_int32), ("solar_scale", C.c_float)]


MAX_SST_PATTERNS = 1024  # GREB_MAX_SST_PATTERNS: prescribed-SST patterns of one engine


class GrebMemberSst(C.Structure):
    """struct greb_member_sst: a member's SST pattern (-1: none, the ocean surface is free) and the amplitude on its anomaly."""
    _fields_ = [("pattern", C.c_int32), ("amp", C.c_float)]


MAX_NOISE_PATTERNS = 16  # GREB_MAX_NOISE_PATTERNS: stochastic heat-flux patterns of one engine


class GrebMemberNoise(C.Structure):
    """struct greb_member_noise: a member's noise pattern (-1: none, the member is deterministic), the amplitude on its sigma
    and the member's 64-bit seed as two words."""
    _fields_ = [("pattern", C.c_int32), ("amp", C.c_float), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32)]


# what a member may NOT change (it feeds data every member shares): greb_engine_create_members rejects a difference
MEMBER_SHARED = ("pi", "z_air", "z_vapor", "dt", "dt_crcl", "ipx", "ipy", "year0")


def default_params(**over) -> GrebParams:
    """Reference defaults (src/greb.f90:49-53,68-104), constants folded in fp32 like the compiler."""
    f = np.float32
    p = GrebParams()
    vals = dict(pi=3.1416, sig=5.6704e-8, rho_ocean=999.1, rho_land=2600., rho_air=1.2, cp_ocean=4186.,
                cp_land=926.222, cp_air=1005., eps=1., d_ocean=50., d_land=2., d_air=5000.,
                ct_sens=22.5, da_ice=0.25, a_no_ice=0.1, a_cloud=0.35,
                Tl_ice1=f(273.15) - f(10.), Tl_ice2=273.15, To_ice1=f(273.15) - f(7.),
                To_ice2=f(273.15) - f(1.7), co_turb=5.0, kappa=8e5, ce=2e-3, cq_latent=2.257e6,
                cq_rain=f(f(-0.1) / f(24.)) / f(3600.), z_air=8400., z_vapor=5000., r_qviwv=2.6736e3)
    for k, v in vals.items():
        setattr(p, k, float(f(v)))
    for i, v in enumerate((9.0721, 106.7252, 61.5562, 0.0179, 0.0028, 0.0570, 0.3462, 2.3406, 0.7032, 1.0662)):
        p.p_emi[i] = v
    p.co2_flux = 298.0
    p.ipx, p.ipy, p.year0, p.dt, p.dt_crcl = 1, 1, 1940, 12 * 3600, 1800
    for k, v in over.items():
        if k == "p_emi":
            for i, x in enumerate(v):
                p.p_emi[i] = x
        else:
            setattr(p, k, v)
    return p


def fptr(a: np.ndarray):
    """float* of a C-contiguous fp32 array (caller keeps `a` alive)."""
    assert a.dtype == np.float32 and a.flags.c_contiguous, (a.dtype, a.flags)
    return a.ctypes.data_as(c_float_p)


def make_fields(inp) -> tuple[GrebFields, list]:
    """GrebFields pointing at a workload.Inputs; returns (struct, keepalive list)."""
    keep = []
    f = GrebFields()
    for name in ("z_topo", "glacier", "sw_solar", "tclim", "qclim", "uclim", "vclim", "mldclim",
                 "cldclim", "swetclim"):
        a = np.ascontiguousarray(getattr(inp, name), dtype=np.float32)
        keep.append(a)
        setattr(f, name, fptr(a))
    return f, keep


def noise_prototypes(lib) -> None:
    """The argument types of the stochastic heat-flux calls (greb_engine_get_noise takes an int64_t step, which ctypes would
    otherwise pass as an int)."""
    vp, i32p = C.c_void_p, C.POINTER(C.c_int32)
    lib.greb_engine_set_noise_tables.argtypes = [vp, C.c_int, c_float_p, c_float_p, i32p, i32p, i32p]
    lib.greb_engine_set_member_noise.argtypes = [vp, C.POINTER(GrebMemberNoise)]
    lib.greb_engine_get_noise.argtypes = [vp, C.c_int, C.c_int64, c_float_p]
    for f in (lib.greb_engine_set_noise_tables, lib.greb_engine_set_member_noise, lib.greb_engine_get_noise):
        f.restype = C.c_int


def ens_prototypes(lib) -> None:
    """The argument types of greb_ens_* and greb_engine_run_ens (greb_ens_reduce_dev takes a size_t, which ctypes would
    otherwise pass as an int)."""
    i32p, vp = C.POINTER(C.c_int32), C.c_void_p
    lib.greb_ens_create.argtypes = [C.c_int, C.c_int, C.c_int, i32p, C.c_int, i32p, c_float_p, C.c_int, C.c_uint, C.POINTER(vp)]
    lib.greb_ens_destroy.argtypes = [vp]
    lib.greb_ens_reduce_dev.argtypes = [vp, C.c_int, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
    lib.greb_engine_run_ens.argtypes = [vp, C.c_int, c_float_p, vp] + [c_float_p] * 6
    for f in (lib.greb_ens_create, lib.greb_ens_destroy, lib.greb_ens_reduce_dev, lib.greb_engine_run_ens):
        f.restype = C.c_int


def lin_prototypes(lib) -> None:
    """The argument types of greb_lin_* and greb_engine_run_lin."""
    i32p, f64p, vp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_void_p
    lib.greb_lin_create.argtypes = [C.c_int, C.c_int, C.c_int, f64p, C.c_int, i32p, i32p, f64p, C.c_uint, C.POINTER(vp)]
    lib.greb_lin_destroy.argtypes = [vp]
    lib.greb_lin_reduce_dev.argtypes = [vp, C.c_int, vp, C.c_size_t, vp, vp, vp]
    lib.greb_engine_run_lin.argtypes = [vp, C.c_int, c_float_p, vp, c_float_p, c_float_p, c_float_p]
    for f in (lib.greb_lin_create, lib.greb_lin_destroy, lib.greb_lin_reduce_dev, lib.greb_engine_run_lin):
        f.restype = C.c_int


def gram_prototypes(lib) -> None:
    """The argument types of greb_gram_* and of the two runs that deliver Gram matrices (doubles)."""
    i32p, f64p, vp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_void_p
    lib.greb_gram_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, i32p, C.c_int, i32p, i32p, c_float_p, C.POINTER(vp)]
    lib.greb_gram_destroy.argtypes = [vp]
    lib.greb_gram_reduce_dev.argtypes = [vp, C.c_int, vp, C.c_size_t, vp, vp]
    lib.greb_engine_run_gram.argtypes = [vp, C.c_int, c_float_p, vp, f64p, c_float_p]
    lib.greb_engine_run_budget_gram.argtypes = [vp, C.c_int, c_float_p, c_float_p, C.c_int, vp, f64p, c_float_p]
    for f in (lib.greb_gram_create, lib.greb_gram_destroy, lib.greb_gram_reduce_dev, lib.greb_engine_run_gram,
              lib.greb_engine_run_budget_gram):
        f.restype = C.c_int


T_FIRST, T_LAST, T_STAY, T_COUNT, T_PEAK, T_FRACTION = 1, 2, 4, 8, 16, 32  # crossing products, GREB_T_* of include/greb_engine.h
CROSS_MAX_EVENTS = 16  # GREB_CROSS_MAX_EVENTS


class GrebCrossEvent(C.Structure):
    """struct greb_cross_event: variable, selector (0 ... 11 a month, 12 ... 16 DJF MAM JJA SON ANN), member minus control,
    direction (+1: q >= thr hits, -1: q <= thr) and threshold."""
    _fields_ = [("var", C.c_int32), ("sel", C.c_int32), ("rel", C.c_int32), ("dir", C.c_int32), ("thr", C.c_float)]


def cross_prototypes(lib) -> None:
    """The argument types of greb_cross_* and of the two runs that deliver crossing maps (int32 and float arrays)."""
    i32p, vp = C.POINTER(C.c_int32), C.c_void_p
    maps = [i32p, i32p, i32p, i32p, c_float_p, i32p]  # first, last, stay, count, peak, peak_year
    lib.greb_cross_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(GrebCrossEvent), C.c_int, i32p, i32p, C.c_int,
                                      C.c_uint, C.POINTER(vp)]
    lib.greb_cross_destroy.argtypes = [vp]
    lib.greb_cross_add_year_dev.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp]
    lib.greb_cross_finish_dev.argtypes = [vp, C.c_int, C.c_int] + [vp] * 7
    lib.greb_engine_run_cross.argtypes = [vp, C.c_int, c_float_p, vp] + maps + [c_float_p, c_float_p]
    lib.greb_engine_run_budget_cross.argtypes = [vp, C.c_int, c_float_p, c_float_p, C.c_int, vp] + maps + [c_float_p, c_float_p]
    for f in (lib.greb_cross_create, lib.greb_cross_destroy, lib.greb_cross_add_year_dev, lib.greb_cross_finish_dev,
              lib.greb_engine_run_cross, lib.greb_engine_run_budget_cross):
        f.restype = C.c_int


R_SLOPE, R_INTERCEPT, R_R2, R_INDEX = 1, 2, 4, 8  # regression products, GREB_R_* of include/greb_engine.h
REG_MAX_INDICES, REG_MAX_TERMS, REG_MAX_MEMBERS = 8, 16, 65535  # GREB_REG_MAX_INDICES, GREB_REG_MAX_TERMS, GREB_REG_MAX_MEMBERS


class GrebRegIndex(C.Structure):
    """struct greb_reg_index: variable, selector and member minus control as in GrebCrossEvent, and the region (0: the globe)."""
    _fields_ = [("var", C.c_int32), ("sel", C.c_int32), ("rel", C.c_int32), ("region", C.c_int32)]


class GrebRegTerm(C.Structure):
    """struct greb_reg_term: variable, selector, member minus control, and the index it is regressed on."""
    _fields_ = [("var", C.c_int32), ("sel", C.c_int32), ("rel", C.c_int32), ("index", C.c_int32)]


def reg_prototypes(lib) -> None:
    """The argument types of greb_reg_* and of the two runs that deliver regression maps."""
    i32p, vp = C.POINTER(C.c_int32), C.c_void_p
    out = [c_float_p] * 5  # slope, intercept, r2, index, yearly
    lib.greb_reg_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_int, i32p, C.POINTER(GrebRegIndex), C.c_int,
                                    C.POINTER(GrebRegTerm), C.c_int, C.c_uint, C.POINTER(vp)]
    lib.greb_reg_destroy.argtypes = [vp]
    lib.greb_reg_add_year_dev.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp]
    lib.greb_reg_finish_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.greb_engine_run_reg.argtypes = [vp, C.c_int, c_float_p, vp] + out
    lib.greb_engine_run_budget_reg.argtypes = [vp, C.c_int, c_float_p, c_float_p, C.c_int, vp] + out
    for f in (lib.greb_reg_create, lib.greb_reg_destroy, lib.greb_reg_add_year_dev, lib.greb_reg_finish_dev, lib.greb_engine_run_reg,
              lib.greb_engine_run_budget_reg):
        f.restype = C.c_int


MAX_RECORD_VARS = 16  # GREB_MAX_RECORD_VARS: variables per month of the records a diag or clim plan reduces


def budget_prototypes(lib) -> None:
    """The argument types of the plans with a variable count, of greb_budget_combine_dev (it takes a size_t) and of the
    four reduced runs over the budget records."""
    i32p, vp = C.POINTER(C.c_int32), C.c_void_p
    lib.greb_diag_create_vars.argtypes = [C.c_int, C.c_int, c_float_p, C.c_int, C.c_int, C.POINTER(vp)]
    lib.greb_clim_create_vars.argtypes = [C.c_int, C.c_int, C.c_int, i32p, C.c_uint, C.c_int, C.POINTER(vp)]
    lib.greb_budget_combine_dev.argtypes = [c_float_p, C.c_int, vp, C.c_int, C.c_size_t, vp, vp]
    head = [vp, C.c_int, c_float_p, c_float_p, C.c_int, vp]  # engine, years, co2_ppm, combo, n_out, plan
    lib.greb_engine_run_budget_diag.argtypes = head + [C.c_uint] + [c_float_p] * 4
    lib.greb_engine_run_budget_clim.argtypes = head + [C.c_int, i32p, i32p] + [c_float_p] * 6
    lib.greb_engine_run_budget_ens.argtypes = head + [c_float_p] * 6
    lib.greb_engine_run_budget_lin.argtypes = head + [c_float_p] * 3
    for f in (lib.greb_diag_create_vars, lib.greb_clim_create_vars, lib.greb_budget_combine_dev, lib.greb_engine_run_budget_diag,
              lib.greb_engine_run_budget_clim, lib.greb_engine_run_budget_ens, lib.greb_engine_run_budget_lin):
        f.restype = C.c_int


DERIVE_MAX_INS, DERIVE_MAX_TOTAL, DERIVE_MAX_STACK, DERIVE_MAX_LOCALS, DERIVE_MAX_FIELDS = 64, 512, 8, 4, 8  # GREB_DERIVE_MAX_*
# the ops of a derive program, GREB_DV_* of include/greb_engine.h in their numbering
DV_NAMES = ("STATE", "TERM", "FIELD", "CONST", "TEE", "GET", "ADD", "SUB", "MUL", "DIV", "MIN", "MAX", "GE", "LT", "NEG", "ABS", "SQRT",
            "EXP", "LOG", "ATAN", "SELECT")


class GrebDeriveIns(C.Structure):
    """struct greb_derive_ins: op (GREB_DV_*), arg (the index of STATE, TERM, FIELD, TEE, GET) and value (of CONST)."""
    _fields_ = [("op", C.c_int32), ("arg", C.c_int32), ("value", C.c_float)]


def derive_prototypes(lib) -> None:
    """The argument types of greb_derive_* and of the seven reduced runs over derived records: those of the budget runs with
    the derive plan in place of combo and n_out."""
    i32p, f64p, vp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_void_p
    lib.greb_derive_create.argtypes = [C.c_int, C.c_int, C.POINTER(GrebDeriveIns), i32p, C.c_int, c_float_p, C.c_int, C.POINTER(vp)]
    lib.greb_derive_destroy.argtypes = [vp]
    lib.greb_derive_uses_budget.argtypes = [vp]
    lib.greb_derive_apply_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp]
    head = [vp, C.c_int, c_float_p, vp, vp]  # engine, years, co2_ppm, derive plan, plan
    lib.greb_engine_run_derived_diag.argtypes = head + [C.c_uint] + [c_float_p] * 4
    lib.greb_engine_run_derived_clim.argtypes = head + [C.c_int, i32p, i32p] + [c_float_p] * 6
    lib.greb_engine_run_derived_ens.argtypes = head + [c_float_p] * 6
    lib.greb_engine_run_derived_lin.argtypes = head + [c_float_p] * 3
    lib.greb_engine_run_derived_gram.argtypes = head + [f64p, c_float_p]
    lib.greb_engine_run_derived_cross.argtypes = head + [i32p, i32p, i32p, i32p, c_float_p, i32p] + [c_float_p, c_float_p]
    lib.greb_engine_run_derived_reg.argtypes = head + [c_float_p] * 5
    for f in (lib.greb_derive_create, lib.greb_derive_destroy, lib.greb_derive_uses_budget, lib.greb_derive_apply_dev,
              lib.greb_engine_run_derived_diag, lib.greb_engine_run_derived_clim, lib.greb_engine_run_derived_ens,
              lib.greb_engine_run_derived_lin, lib.greb_engine_run_derived_gram, lib.greb_engine_run_derived_cross,
              lib.greb_engine_run_derived_reg):
        f.restype = C.c_int


def nan_overrides(n: int):
    arr = (GrebMemberOverrides * n)()
    for o in arr:
        o.da_ice = o.a_no_ice = o.a_cloud = o.kappa = math.nan
    return arr
