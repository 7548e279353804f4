"""A scenario year of the model stepped from Python, with the thirteen flux terms of the update accumulated beside the
five standard records.  TEST INFRASTRUCTURE, NOT PRODUCT.

Every routine is the oracle's per-routine entry point (oracle/oracle.py: swradiation, lwradiation, hydro, deep_ocean,
seaice, circulation -- pinned bit for bit to the compiled reference); the Euler update of src/greb.f90:254-268 and the
monthly accumulation of :974-984 are numpy float32, one operation per rounding, in the reference's operation order.
tests/test_budget_cpu.py checks the five records of a mirror year against Oracle.run under np.array_equal before anything
is compared with the budget: that is what makes the thirteen sums a yardstick.

The oracle instance is used for its routines and its cap_surf (which seaice() updates in place); its own state fields
are neither read after the start nor written, so `Oracle.run` can follow from the same state once cap_surf is put back
(MirrorStart.restore)."""
import numpy as np

from greb_climate_model_amd import abi

NT = abi.NSTEP_YR
f32 = np.float32


class MirrorStart:
    """What a run starts from: Ts, Ta, To, q, cap_surf and the three correction arrays of an oracle."""

    def __init__(self, oracle):
        self.state5 = oracle.state5()
        self.corr = np.stack([oracle.field(10 + i, NT).copy() for i in range(3)])  # TF, qF, ToF [3][730][ny][nx]

    def restore(self, oracle):
        """cap_surf back into the oracle (the mirror's seaice calls moved it); its state fields were never touched."""
        oracle.field(4)[:] = self.state5[4]


def run_year(oracle, start: MirrorStart, co2: float, observer=None):
    """One scenario year (steps it = 1 ... 730 of a scenario that begins at the year's first step) from `start`.
    Returns (monthly [12][5][ny][nx], budget [12][13][ny][nx], state5 at the end).
    observer: called once per step as observer(ityr, Ts, To, q, dq, Ts0) with the state the step starts from, the humidity
    increment BEFORE the clamp of :265 and the new Tsurf (what seaice sees); it reports, it changes nothing
    (tests/edge_workload.py: Census counts the points the clamp fires at and the smallest |dq + q| / q)."""
    p = oracle.params
    dt = f32(p.dt)
    cap_air = f32(p.cp_air) * f32(p.rho_air) * f32(p.d_air)  # :188
    ct_sens = f32(p.ct_sens)
    Ts, Ta, To, q = (start.state5[i].copy() for i in range(4))
    oracle.field(4)[:] = start.state5[4]
    TF, qF, ToF = start.corr
    wz_air, wz_vapor = oracle.field(5).copy(), oracle.field(6).copy()
    ny, nx = Ts.shape
    monthly = np.zeros((12, 5, ny, nx), f32)
    budget = np.zeros((12, abi.NBUDGET, ny, nx), f32)
    acc5 = np.zeros((5, ny, nx), f32)
    acc13 = np.zeros((abi.NBUDGET, ny, nx), f32)
    month_end = np.cumsum(abi.JDAY_MON)
    mon = 0
    for it in range(1, NT + 1):
        ityr = (it - 1) % NT + 1          # :252
        jday = ((it - 1) // 2) % 365 + 1  # :251
        cap = oracle.field(4).copy()
        # tendencies, :277-308
        sw, albedo = oracle.swradiation(ityr, Ts)
        LW_surf, LWair_up, LWair_down, em = oracle.lwradiation(ityr, Ts, Ta, q, co2)
        Q_sens = ct_sens * (Ta - Ts)      # :295
        Q_lat, Q_lat_air, dq_eva, dq_rain = oracle.hydro(ityr, Ts, q)
        dTa_crcl = oracle.circulation(Ta, wz_air, ityr=ityr)
        dq_crcl = oracle.circulation(q, wz_vapor, ityr=ityr)
        dT_ocean, dTo = oracle.deep_ocean(ityr, Ts, To)
        LW_abs = em * LW_surf             # the product inside :260
        # time_loop, :258-266
        Ts0 = (Ts + dT_ocean) + (dt * (((((sw + LW_surf) - LWair_down) + Q_lat) + Q_sens) + TF[ityr - 1])) / cap
        Ta0 = (Ta + dTa_crcl) + (dt * ((((LWair_up + LWair_down) - LW_abs) + Q_lat_air) - Q_sens)) / cap_air
        To0 = (To + dTo) + ToF[ityr - 1]
        dq = ((dt * (dq_eva + dq_rain)) + dq_crcl) + qF[ityr - 1]
        dq_raw = dq
        dq = np.where(dq <= -q, f32(-0.9) * q, dq).astype(f32)
        q0 = q + dq
        for a in (Ts0, Ta0, To0, q0):
            assert a.dtype == f32
        oracle.seaice(ityr, Ts0)          # :268
        if observer is not None:
            observer(ityr, Ts, To, q, dq_raw, Ts0)
        # output, :974-984, and the same rule for the thirteen terms
        for i, x in enumerate((Ts0, Ta0, To0, q0, albedo)):
            acc5[i] += x
        for i, x in enumerate((sw, LW_surf, LWair_down, LW_abs, Q_sens, Q_lat, Q_lat_air, dq_eva, dq_rain, dT_ocean, dTo,
                               dTa_crcl, dq_crcl)):
            assert x.dtype == f32
            acc13[i] += x
        if jday == month_end[mon] and it % 2 == 0:
            ndm = f32(abi.JDAY_MON[mon] * 2)
            monthly[mon] = acc5 / ndm
            budget[mon] = acc13 / ndm
            acc5[:] = 0
            acc13[:] = 0
            mon += 1
        Ts, Ta, To, q = Ts0, Ta0, To0, q0
    assert mon == 12
    return monthly, budget, np.stack([Ts, Ta, To, q, oracle.field(4).copy()])
