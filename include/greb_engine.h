/* greb_engine.h -- C ABI of the MI355X-native GREB time-integration engine.
 *
 * The reference (sieste/greb-climate-model) has no plugin / FFI interface: its routines are
 * external Fortran procedures that talk through module globals.  The drop-in boundary is
 * therefore the natural seam SURVEY.md 8(b) identifies -- the two time loops
 *     src/greb.f90:325-362   (qflux_correction: flux-correction phase)
 *     src/greb.f90:228-234   (greb_model: scenario phase, one time_loop call per step)
 * and everything the reference hands across that seam today through modules mo_numerics /
 * mo_physics / mo_diagnostics (src/greb.f90:32-158) is passed here explicitly.
 *
 * A thin Fortran host (greb_climate_model_amd/host/greb_host.f90, iso_c_binding) keeps the
 * reference's CLI / namelist / input-file / output-record conventions and calls these entry
 * points; INTEGRATION.md shows the bind(C) interface block.  Everything is plain C: pointers,
 * ints, floats; no C++ or torch types.  All arrays are IEEE fp32 in the reference's own memory
 * order (Fortran column-major == C [t][lat][lon], longitude fastest, latitude row 0 = south).
 *
 * Error convention: every entry returns int; 0 = ok, <0 = engine error (GREB_E_*), >0 = a
 * hipError_t passed through.  greb_engine_last_error() gives a message.  Nothing throws or
 * exits across the ABI.  An engine is used from one host thread at a time.
 */
#ifndef GREB_ENGINE_H
#define GREB_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GREB_NSTEP_YR 730 /* ndays_yr*ndt_days, src/greb.f90:37-41 */
#define GREB_NVAR_OUT 5   /* Tsurf, Tair, Tocean, q, albedo: src/greb.f90:978-982 */

#define GREB_E_INVALID   (-1) /* bad argument / shape */
#define GREB_E_NOGPU     (-2) /* no HIP device: the product path has no CPU fallback */
#define GREB_E_STATE     (-3) /* call order (e.g. run before create) */
#define GREB_E_UNSUPPORTED (-4)

/* namelist group physics_par in declaration order (src/greb.f90:68-101,128-132),
 * then co2_flux (:104), numerics (:51-53) and the two integer time steps (:38-39). */
typedef struct greb_params {
  float pi, sig, rho_ocean, rho_land, rho_air, cp_ocean, cp_land, cp_air, eps;
  float d_ocean, d_land, d_air, ct_sens, da_ice, a_no_ice, a_cloud;
  float Tl_ice1, Tl_ice2, To_ice1, To_ice2;
  float co_turb, kappa, ce, cq_latent, cq_rain, z_air, z_vapor, r_qviwv;
  float p_emi[10];
  float co2_flux;
  int32_t ipx, ipy;   /* 1-based diagnostic point, src/greb.f90:51-52,954 */
  int32_t year0;
  int32_t dt;         /* 43200 */
  int32_t dt_crcl;    /* 1800  */
} greb_params;

/* Fill with the reference defaults (src/greb.f90:49-53,68-104). */
void greb_params_default(greb_params* p);

/* The reference's input set, host pointers (src/greb.f90:1073-1085). */
typedef struct greb_fields {
  const float* z_topo;   /* [ny][nx]       input/topography     */
  const float* glacier;  /* [ny][nx]       input/glacier.masks  */
  const float* sw_solar; /* [730][ny]      input/solar.radiation */
  const float* tclim;    /* [730][ny][nx]  input/tsurf          */
  const float* qclim;    /*                input/vapor          */
  const float* uclim;    /*                input/zonal.wind     */
  const float* vclim;    /*                input/meridional.wind */
  const float* mldclim;  /*                input/ocean.mld      */
  const float* cldclim;  /*                input/cloud.cover    */
  const float* swetclim; /*                input/soil.moisture  */
} greb_fields;

/* Per-member physics overrides for perturbed-physics ensembles (BASELINE config 5).
 * A member is what a separate `ens_id` process is in the reference (src/greb.f90:153,1064-1068).
 * NaN in a slot = keep the engine-wide greb_params value. */
typedef struct greb_member_overrides {
  float da_ice, a_no_ice, a_cloud, kappa;
} greb_member_overrides;

/* A member as a full namelist plus its experiment switches (GREB_X_* below): everything a separate `ens_id` process of the
 * reference -- or, with `switches`, of the upstream variant's log_exp -- can change.  Per member may differ
 *   every field that reaches the point physics: sig, ct_sens, da_ice, a_no_ice, a_cloud, Tl_ice1/2, To_ice1/2, co_turb,
 *     ce, cq_latent, cq_rain, r_qviwv, p_emi[10], and rho_*, cp_*, d_land, d_air through the heat capacities;
 *   kappa (the member gets its own row tables); co2_flux; switches.
 * pi, z_air, z_vapor, dt, dt_crcl, ipx, ipy, year0 feed data every member shares (row-table geometry, wz_air / wz_vapor,
 * the clock) and must equal the engine-wide greb_params: GREB_E_INVALID otherwise, the message names field and member. */
typedef struct greb_member_config {
  greb_params p;
  uint32_t switches;
} greb_member_config;

/* engine flags */
#define GREB_F_STRICT 1u /* reference operation order, IEEE division, no FMA contraction
                            (bit-exact stencils; default is the restructured fast arithmetic) */
#define GREB_F_MULTILAUNCH 2u /* force the any-grid engine (one launch per circulation sub-step) even
                                 where the fused one-CU-per-member kernel applies (96x48); grids that
                                 do not fit one CU, e.g. 384x192, always use it */

#define GREB_F_ROW_STRIPS 4u /* 384-wide grids: FAST arithmetic takes the row-strip form of the circulation
                                (greb_step_rows.hip: one wavefront per strip of rows, no workgroup barrier) by default
                                at every member count; this flag extends it to STRICT arithmetic, which otherwise keeps
                                the band kernel (greb_kernels.hip: sweep_kernel<fused>).  The two are bit-identical in
                                STRICT (tests/test_gpu_parity.py::test_row_strip_substep_equals_band_kernel_strict) */
/* 384-wide grids, row strips: the circulation call (src/greb.f90:546-550: 24 sub-steps inside one call) runs either
 * as one launch per SUB-STEP (greb_step_rows.hip) or as ONE launch per call (greb_circ_rows.hip), whose strips hand
 * their rows to each other through memory flags and therefore need every strip of the launch resident at once (asserted
 * against the device's wavefront slots; an engine created while other engines of the process hold the slots of its device
 * takes one launch per sub-step by itself).  The two are bit-identical; which is faster depends on the member count, so
 * by default the engine times both during the first eight model steps it integrates and keeps the faster. */
#define GREB_F_NO_PERSISTENT 8u /* always one launch per sub-step */
#define GREB_F_PERSISTENT 16u   /* one launch per call wherever it can be resident, without the trial */

typedef struct greb_engine greb_engine;

/* Create an engine for n_members ensemble members on HIP device `device`.
 * Any grid with nx % 4 == 0, nx >= 12, 5 <= ny <= 192 (src/greb.f90:36 is the only thing that fixes the grid in the
 * reference).  Which kernels a grid gets:
 *   96x48 with the default sub-cycling layout   the fused member kernel (a whole member resident in one compute unit);
 *   nx = 384 or nx = 192                        the any-grid engine on wavefront-sized row strips (a lane owns six
 *                                               longitudes; a 192-wide row is laid twice around the wavefront);
 *   anything else                               the any-grid engine on latitude bands staged in LDS.
 * What bounds ny: the per-row tables (sub-cycle counts and constants, src/greb.f90:578-582, 652-654, 838-840) are
 * fixed-size arrays of 192 rows that travel by value in kernel arguments and sit in LDS, and a strip's rows are packed
 * k0 in 8 and k1 in 9 bits of a task word; ny > 192 is GREB_E_INVALID, not a slower path.
 * Copies the inputs to HBM, computes the derived fields of greb_model's preamble
 * (src/greb.f90:176-216) and Toclim (src/greb.f90:1088-1094) and sets every member's
 * state to the initial state (src/greb.f90:194-197).  overrides may be NULL. */
int greb_engine_create(const greb_params* p, int nx, int ny, const greb_fields* f, int n_members,
                       const greb_member_overrides* overrides, int device, unsigned flags,
                       greb_engine** out);

/* The same with one greb_member_config per member (greb_engine_create is this with the four override slots expanded and
 * no switches).  Members that are alike in physics, kappa, co2_flux and switches share ONE flux-correction set
 * (3 x 730 fields) and are integrated once in the flux-correction phase; otherwise every member has its own.
 * On the any-grid engine the transport kernels run all members of a launch alike: members that differ in
 * GREB_X_VAPOR_DIFFUSION_ONLY are GREB_E_UNSUPPORTED there (run the two groups as two engines beside each other); a member
 * with GREB_X_NO_CIRCULATION beside members without it is transported with the rest and drops its increments. */
int greb_engine_create_members(const greb_params* p, int nx, int ny, const greb_fields* f, int n_members,
                               const greb_member_config* members, int device, unsigned flags, greb_engine** out);

/* qflux_correction (src/greb.f90:311-364): `years`*730 steps at co2_flux; leaves the
 * correction arrays, cap_surf and the spun-up state in the engine.
 * yearly may be NULL, else [n_members][years][2] = {global-mean Tsurf, Tsurf(ipx,ipy)} in
 * deg C as printed at src/greb.f90:954. */
int greb_engine_flux_correction(greb_engine* e, int years, float* yearly);

/* What the engine is and which kernels it has settled on, as a JSON object (valid until the next call from this thread). */
const char* greb_engine_describe(greb_engine* e);

/* Scenario run (src/greb.f90:226-234 + time_loop :239-274): `years`*730 steps.
 *   co2_ppm : [n_members][years]   annual CO2, already padded (src/greb.f90:1053-1061)
 *   monthly : [n_members][years][12][5][ny][nx]  monthly means in file-record order
 *             (src/greb.f90:978-982); host memory unless GREB_RUN_DEVICE_OUT
 *   yearly  : [n_members][years][2] as above (may be NULL)
 * May be called repeatedly; the model clock (it, year, month accumulators) continues. */
#define GREB_RUN_DEVICE_OUT 1u /* `monthly` is a device pointer (e.g. for an RCCL gather) */
int greb_engine_run(greb_engine* e, int years, const float* co2_ppm, float* monthly, float* yearly,
                    unsigned run_flags);

/* ---- budget output: monthly means of the energy and water flux terms ------------------------------
 * Every step the point physics evaluates the terms of the reference's update (src/greb.f90:254-268, 277-308) and folds
 * them into the new state.  They are non-linear in the state, so the monthly mean of a flux is not the flux of the
 * monthly-mean state: only the step loop can deliver them.  GREB_NBUDGET fields per month, in the order, with the sign and
 * in the unit in which the update uses them; a monthly mean is the fp32 sum of the step values over the month divided by
 * 2 * days (the rule and the month boundaries of :974-984).  Under a member's GREB_X_* switches the terms are what the
 * update really used: 0 where a process is switched off.  The flux corrections TF, qF, ToF are not terms
 * (greb_engine_get_corrections has them per step). */
#define GREB_NBUDGET 13
#define GREB_B_SW          0  /* absorbed solar, :258                                   W/m2 */
#define GREB_B_LW_SURF     1  /* surface long-wave (negative), :258                     W/m2 */
#define GREB_B_LWAIR_DOWN  2  /* :258, :260 (LWair_up equals it, :432)                  W/m2 */
#define GREB_B_LW_ABS      3  /* em * LW_surf as formed in :260                         W/m2 */
#define GREB_B_Q_SENS      4  /* :295                                                   W/m2 */
#define GREB_B_Q_LAT       5  /*                                                        W/m2 */
#define GREB_B_Q_LAT_AIR   6  /*                                                        W/m2 */
#define GREB_B_DQ_EVA      7  /*                                                        1/s  */
#define GREB_B_DQ_RAIN     8  /*                                                        1/s  */
#define GREB_B_DT_OCEAN    9  /*                                                        K per step */
#define GREB_B_DTO         10 /*                                                        K per step */
#define GREB_B_DTA_CRCL    11 /* the Tair increment of the circulation sub-steps, :551  K per step */
#define GREB_B_DQ_CRCL     12 /* the same for q, after the switch handling              per step */
/* "sw", "LW_surf", ... for i = 0 ... GREB_NBUDGET - 1, NULL otherwise. */
const char* greb_budget_name(int i);
/* greb_engine_run that also delivers
 *   budget : [n_members][years][12][GREB_NBUDGET][ny][nx]   host memory, or device memory under GREB_RUN_DEVICE_OUT,
 *            exactly as `monthly`
 * monthly, yearly, the model clock and the state the engine is left in are those of greb_engine_run over the same years,
 * bit for bit.  monthly may be NULL (a budget-only run); a NULL budget is GREB_E_INVALID.  Scenario phase only: the
 * flux-correction phase delivers nothing, as in the reference.  Host delivery follows greb_engine_run's scheme (two
 * staging slots, year y leaves while year y + 1 integrates); device memory does not grow with `years`.  The budget sums
 * are zero at every year boundary, so run and run_budget calls may alternate freely. */
int greb_engine_run_budget(greb_engine* e, int years, const float* co2_ppm, float* monthly, float* budget, float* yearly,
                           unsigned run_flags);

/* ---- reduced output: regional, zonal and annual diagnostics made on the device ------------------
 * The reference leaves every diagnostic to R scripts over the output file (R/analyse_output_fields.R).  A big ensemble
 * cannot hand back [n_members][years][12][5][ny][nx]; what its analysis wants per member is small, and comes from ONE pass
 * over a model year of monthly records while they are still in HBM (greb_diag.hip).  Three products, chosen by flags:
 *   GREB_D_REGIONS  [..][12][5][1 + n_regions]  weighted means  sum w_r(j,i) c_j x / sum w_r(j,i) c_j;  region 0 is the
 *                   globe (w = 1), regions 1 ... n_regions are the caller's;  c_j = cos(lat_j), lat_j = (j + 0.5) 180 / ny
 *                   - 90 degrees (row 0 = south), evaluated in double with the true pi, not greb_params.pi
 *   GREB_D_ZONAL    [..][12][5][ny]             the plain mean over longitude
 *   GREB_D_ANNUAL   [..][5][ny][nx]             the day-weighted mean of the twelve records, sum jday_mon[m] X_m / 365
 *                   (src/greb.f90:42): in exact arithmetic the mean over the year's 730 steps
 * Every sum is accumulated in fp64 in an order the grid alone fixes (no atomics) and rounded to fp32 once: results are
 * deterministic, and a member's numbers do not depend on how many members are reduced with it or where it sits. */
#define GREB_D_REGIONS 1u
#define GREB_D_ZONAL   2u
#define GREB_D_ANNUAL  4u
typedef struct greb_diag greb_diag;
/* A plan: the grid and the regions.  region_w: [n_regions][ny][nx] weights in [0, 1] shared by all members (NULL with
 * n_regions = 0: the globe alone), n_regions <= 15.  Host work only -- the combined weights w_r c_j and the reciprocals of
 * their sums are made here in double -- and validated without touching a device: a grid the engine does not take,
 * n_regions > 15, a weight outside [0, 1] or not finite, a region whose weights are all zero are GREB_E_INVALID with a
 * message that names the offender (greb_engine_last_error(NULL)).  A plan serves any number of engines and calls, one at
 * a time. */
int greb_diag_create(int nx, int ny, const float* region_w, int n_regions, greb_diag** out);
int greb_diag_destroy(greb_diag* d);
/* One model year [n_members][12][5][ny][nx] on HIP device `device` -> the products whose pointer is not NULL (device
 * pointers, laid out [n_members] + the shapes above; monthly_year_dev and annual_dev 16-byte aligned).  Launches on
 * `stream` (a hipStream_t, may be NULL) and does not synchronise: e.g. ahead of an RCCL all-reduce of the small products. */
int greb_diag_reduce_dev(greb_diag* d, int device, const float* monthly_year_dev, int n_members, float* regions_dev,
                         float* zonal_dev, float* annual_dev, void* stream);
/* greb_engine_run that delivers ONLY the products selected by `what` (GREB_D_*), to host memory:
 *   regions [n_members][years][12][5][1 + n_regions]   zonal [n_members][years][12][5][ny]   annual [n_members][years][5][ny][nx]
 * (a pointer whose product is not selected is ignored and may be NULL; a selected product with a NULL pointer is
 * GREB_E_INVALID, as is a plan made for another grid).  co2_ppm, yearly, the model clock and the state the engine is left
 * in are those of greb_engine_run over the same years, bit for bit.  Each year is integrated into one of the engine's two
 * one-year staging slots and reduced there; zonal means and annual maps leave per year on the copy stream.  Device memory
 * does not grow with `years` except for the yearly scalars and the region series: a 100-year run of 512 members needs
 * what a 1-year run needs. */
int greb_engine_run_diag(greb_engine* e, int years, const float* co2_ppm, greb_diag* d, unsigned what, float* regions,
                         float* zonal, float* annual, float* yearly);

/* ---- climatology output: multi-year means, seasons, trends and responses made on the device -------
 * What an ensemble with a control member beside its other members is run for: average each calendar month over a window
 * of years, then subtract the control.  The reference leaves that to R scripts over the files of separate processes; here
 * the reduction along the time axis -- the only axis whose output grows with the length of the run -- happens in the
 * staging slot behind each model year (greb_clim.hip).  Per element the years of a period are summed in fp64 in
 * ascending year order, S = sum x and (for the trend) T = sum k x with k = 0 ... n-1 the year inside the period; of those,
 * all in fp64 and each rounded to fp32 exactly once:
 *   mean64[mo]      = S[mo] / n
 *   GREB_C_MEAN     [member][period][12][5][ny][nx]   mean64
 *   GREB_C_SEASONS  [member][period][5][5][ny][nx]    DJF, MAM, JJA, SON, ANN:  acc = 0; acc = acc + jday_mon[mo] mean64[mo]
 *                   over the season's months in calendar order (DJF = Dec, Jan, Feb of the SAME calendar years; ANN =
 *                   Jan ... Dec); acc / the season's days (90, 92, 92, 91, 365; jday_mon: src/greb.f90:42)
 *   GREB_C_TREND    [member][period][12][5][ny][nx]   per calendar month the least-squares slope per year,
 *                   (T - kbar S) / Sxx with kbar = (n-1)/2, Sxx = n(n^2-1)/12; 0 for n = 1
 *   GREB_C_RESPONSE the selected MEAN / SEASONS also as member minus its control, mean64[m] - mean64[control[m]] and the
 *                   same of the seasonal means (the difference is formed in fp64, before anything is rounded).  A member
 *                   with control[m] = -1 has a QUIET NaN in its response records -- zero would read as "no response";
 *                   control[m] = m is legal and gives zeros.
 * The order of these operations is the definition of the results (no fused multiply-add); every element has one owner
 * (no atomics), so results are deterministic and a member's numbers do not depend on the batch it is in. */
#define GREB_C_MEAN     1u
#define GREB_C_SEASONS  2u
#define GREB_C_TREND    4u
#define GREB_C_RESPONSE 8u
typedef struct greb_clim greb_clim;
/* A plan: grid, member count, each member's control (control[m] in -1 ... n_members-1, or NULL: no control map) and the
 * products.  Host data only, validated without touching a device: a grid greb_diag_create does not take, n_members < 1,
 * a control index out of range, `what` zero or with unknown bits, GREB_C_RESPONSE without GREB_C_MEAN or GREB_C_SEASONS
 * or without `control` are GREB_E_INVALID with a message that names the offender (greb_engine_last_error(NULL)).  The
 * fp64 sums (8 bytes per element of a model year, 16 with the trend) live per device and are allocated on first use.  A
 * plan sums one period at a time and serves any number of periods, calls and engines one after the other. */
int greb_clim_create(int nx, int ny, int n_members, const int32_t* control, unsigned what, greb_clim** out);
int greb_clim_destroy(greb_clim* c); /* waits for the device before it frees the sums */
/* Year k (0-based) of the current period, one model year [n_members][12][5][ny][nx] on HIP device `device` (16-byte
 * aligned), into the sums.  k must be the number of years added since the last finish: k = 0 stores, it does not add, so
 * no clearing is needed.  Launches on `stream` (a hipStream_t, may be NULL) and does not synchronise; the calls of one
 * period must be ordered among themselves (one stream, or the caller's events). */
int greb_clim_add_year_dev(greb_clim* c, int device, const float* monthly_year_dev, int k, void* stream);
/* The products of the n_years years added since the last finish (n_years must be that number) to device memory, laid out
 * [n_members] + the shapes above without [period], 16-byte aligned.  A pointer whose product the plan does not select
 * is ignored and may be NULL; a selected product with a NULL pointer is GREB_E_INVALID.  Both _dev calls check their
 * arguments before any device query; without a device they are GREB_E_NOGPU (no CPU path). */
int greb_clim_finish_dev(greb_clim* c, int device, int n_years, float* mean_dev, float* seasons_dev, float* trend_dev,
                         float* mean_resp_dev, float* seasons_resp_dev, void* stream);
/* greb_engine_run that delivers ONLY the plan's products of n_periods averaging periods, to host memory in the shapes
 * above.  Period p covers the years first_year[p] ... first_year[p] + n_years[p] - 1 of this call (0-based); periods are
 * ascending, do not overlap and lie inside 0 ... years-1 (GREB_E_INVALID otherwise, as for a plan made for another grid
 * or member count or a selected product with a NULL pointer; the message names the period at fault; all of it is decided
 * before any device work).  Years outside every period are integrated but not summed.  Each year is integrated into
 * one of the engine's two one-year staging slots and added to the sums there; at a period's last year its products are
 * written to one of two device output slots and leave on the copy stream while the following years integrate.  Device
 * memory grows neither with `years` nor with n_periods (the yearly scalars aside).  co2_ppm, yearly, the model clock, the
 * state the engine is left in and the kernels that integrate are those of greb_engine_run over the same years, bit for
 * bit: switches, member forcing and boundary sets act as they do there. */
int greb_engine_run_clim(greb_engine* e, int years, const float* co2_ppm, greb_clim* c, int n_periods, const int32_t* first_year,
                         const int32_t* n_years, float* mean, float* seasons, float* trend, float* mean_resp, float* seasons_resp,
                         float* yearly);

/* ---- ensemble output: statistics across the members of a group, made on the device -----------------
 * The member axis is what makes a many-member run's output big.  A plan puts each member into a group (group[m] in
 * -1 ... n_groups-1; -1: in no group, e.g. a pure control member) and optionally names its control member (control[m] in
 * -1 ... n_members-1); per group and per element of x[n_members][n] the statistics are taken across the group's members,
 * in ascending member index, of the samples
 *   v = x[m][i]                          without a control map
 *   v = x[m][i] - x[control[m]][i]       with one, as ONE fp32 subtraction (control[m] = m is legal and gives zeros)
 * For a group of n_g members, all in fp64 unless said otherwise, each product rounded to fp32 exactly once:
 *   GREB_S_MEAN       S = sum (double)v;  mean = S / n_g
 *   GREB_S_VAR        K = (double)v of the group's first member, d = (double)v - K, S1 = sum d, S2 = sum d d;
 *                     var = (S2 - S1 S1 / n_g) / (n_g - 1), set to 0 where that is negative and for n_g = 1: the sample
 *                     variance in one pass.  No square root is taken on the device.
 *   GREB_S_RANGE      min and max of v, in fp32
 *   GREB_S_QUANTILES  the group's v sorted ascending; for probability p (fp32): h = (double)p (n_g - 1), lo = floor(h),
 *                     t = h - lo, a = v[lo], b = v[min(lo + 1, n_g - 1)], q = a + t (b - a) as a multiply, then an add
 *                     (numpy's "linear" rule with the arithmetic pinned)
 * The order of these operations is the definition of the results (no fused multiply-add); every output element has one
 * owner (no atomics), so results are deterministic, and a group's numbers depend neither on the other groups and members
 * of the call nor on where its members sit. */
#define GREB_S_MEAN      1u
#define GREB_S_VAR       2u
#define GREB_S_RANGE     4u
#define GREB_S_QUANTILES 8u
#define GREB_ENS_MAX_GROUPS 64
#define GREB_ENS_MAX_PROBS  16
#define GREB_ENS_MAX_SORTED 4096 /* members of one group under GREB_S_QUANTILES */
typedef struct greb_ens greb_ens;
/* A plan: grid, member count, group[n_members], control[n_members] or NULL, probs[n_probs] and the products `what`
 * (GREB_S_*; probs is read only under GREB_S_QUANTILES).  Host work only, validated without touching a device.
 * GREB_E_INVALID with a message that names the offender (greb_engine_last_error(NULL)): a grid greb_diag_create does not
 * take, n_members < 1, n_groups outside 1 ... 64, a group or control index out of range, an empty group, a member of a
 * group whose control is -1 while a control map is given, `what` zero or with unknown bits, GREB_S_QUANTILES with n_probs
 * outside 1 ... 16 or a probability outside [0, 1] or not finite.  GREB_E_UNSUPPORTED: GREB_S_QUANTILES with a group of
 * more than 4096 members (the sort's tile is one compute unit's LDS).  A plan serves any number of calls and engines. */
int greb_ens_create(int nx, int ny, int n_members, const int32_t* group, int n_groups, const int32_t* control,
                    const float* probs, int n_probs, unsigned what, greb_ens** out);
int greb_ens_destroy(greb_ens* s); /* waits for the device before it frees the member lists */
/* x_dev[n_members][n] on HIP device `device` (16-byte aligned; n is arbitrary, a model year's staging slot is
 * n = 12 * 5 * ny * nx) -> mean_dev, var_dev, min_dev, max_dev [n_groups][n] and quant_dev [n_groups][n_probs][n].  A
 * pointer whose product the plan does not select is ignored and may be NULL; a selected product with a NULL pointer is
 * GREB_E_INVALID (GREB_S_RANGE needs both min_dev and max_dev).  Launches on `stream` (a hipStream_t, may be NULL) and
 * does not synchronise.  Arguments are checked before any device query; without a device: GREB_E_NOGPU (no CPU path). */
int greb_ens_reduce_dev(greb_ens* s, int device, const float* x_dev, size_t n, float* mean_dev, float* var_dev, float* min_dev,
                        float* max_dev, float* quant_dev, void* stream);
/* greb_engine_run that delivers ONLY the plan's statistics of each model year's monthly records, to host memory:
 *   mean, var, min, max  [n_groups][years][12][5][ny][nx]      quant  [n_groups][years][n_probs][12][5][ny][nx]
 * (unselected products as above; a plan made for another grid or member count is GREB_E_INVALID; all of it is decided
 * before any device work).  Each year is integrated into one of the engine's two one-year staging slots and reduced
 * there into one of two device output slots, which leaves on the copy stream while the following year integrates.
 * Device memory does not grow with `years` (the yearly scalars aside).  co2_ppm, yearly, the model clock, the state the
 * engine is left in and the kernels that integrate are those of greb_engine_run over the same years, bit for bit:
 * switches, member forcing and boundary sets act as they do there. */
int greb_engine_run_ens(greb_engine* e, int years, const float* co2_ppm, greb_ens* s, float* mean, float* var, float* min,
                        float* max, float* quant, float* yearly);

/* ---- linear-model output: effects and sensitivities across members, made on the device -------------
 * An ensemble whose members differ by design -- the factorial of the process switches, perturbed physics -- is read through
 * a linear model across its members: the main effect of each process and the interactions between them, or the regression
 * slope of the response on each parameter.  All of these are linear contrasts along the member axis, out_k = sum_m
 * w[k][m] v_m: factorial effects with weights +-1/M, least-squares coefficients with W = pinv(X), a weighted mean or a
 * difference of two group means likewise.  A plan holds weight[n_terms][n_members] (fp64), optionally use[n_members]
 * (nonzero: the member enters the sums; NULL: all do), control[n_members] (as greb_ens: -1 ... n_members-1, control[m] = m
 * is legal) and design[n_members][n_terms] (fp64; needed by GREB_L_RSS).  Per element i of x[n_members][n], over the USED
 * members in ascending member index, with the samples
 *   v = x[m][i]                          without a control map
 *   v = x[m][i] - x[control[m]][i]       with one, as ONE fp32 subtraction
 * all in fp64, each product rounded to fp32 exactly once:
 *   GREB_L_COEF  b_k = sum weight[k][m] (double)v, each term an fp64 multiply followed by an fp64 add, from +0.0;
 *                coef[k][i] = (float)b_k
 *   GREB_L_RSS   per used member, in ascending m: f = sum_k design[m][k] b_k over ascending k from +0.0 (multiply, then
 *                add; the unrounded fp64 b_k), r = (double)v - f, R = R + r r from +0.0;  rss[i] = (float)R: the residual
 *                sum of squares of the fit design * b (for W = pinv(X): what the least-squares fit leaves unexplained)
 * The order of these operations is the definition of the results (no fused multiply-add); every output element has one
 * owner (no atomics), so results are deterministic and depend neither on what else the call holds nor on the other
 * product.  A member with use[m] = 0 that is no used member's control is never read: its row may hold NaN. */
#define GREB_L_COEF 1u
#define GREB_L_RSS  2u
#define GREB_LIN_MAX_TERMS 64
typedef struct greb_lin greb_lin;
/* A plan: grid, member count, weight[n_terms][n_members], use[n_members] or NULL, control[n_members] or NULL,
 * design[n_members][n_terms] or NULL and the products `what` (GREB_L_*).  Host work only, validated without touching a
 * device.  GREB_E_INVALID with a message that names the offender (greb_engine_last_error(NULL)): a grid greb_diag_create
 * does not take, n_members < 1, n_terms outside 1 ... 64, `what` zero or with unknown bits, `weight` NULL, GREB_L_RSS
 * without `design`, a control index out of range, a used member whose control is -1 while a control map is given, no
 * used member, a weight or design entry of a used member that is not finite (the message names term and member; what
 * belongs to an unused member is not looked at).  A plan serves any number of calls and engines. */
int greb_lin_create(int nx, int ny, int n_members, const double* weight, int n_terms, const int32_t* use, const int32_t* control,
                    const double* design, unsigned what, greb_lin** out);
int greb_lin_destroy(greb_lin* l); /* waits for the device before it frees the tables */
/* x_dev[n_members][n] on HIP device `device` (16-byte aligned; n is arbitrary, a model year's staging slot is
 * n = 12 * 5 * ny * nx) -> coef_dev [n_terms][n] and rss_dev [n].  A pointer whose product the plan does not select is
 * ignored and may be NULL; a selected product with a NULL pointer is GREB_E_INVALID.  Launches on `stream` (a
 * hipStream_t, may be NULL) and does not synchronise.  Arguments are checked before any device query; without a device:
 * GREB_E_NOGPU (no CPU path). */
int greb_lin_reduce_dev(greb_lin* l, int device, const float* x_dev, size_t n, float* coef_dev, float* rss_dev, void* stream);
/* greb_engine_run that delivers ONLY the plan's products of each model year's monthly records, to host memory:
 *   coef  [n_terms][years][12][5][ny][nx]      rss  [years][12][5][ny][nx]
 * (unselected products as above; a plan made for another grid or member count is GREB_E_INVALID; all of it is decided
 * before any device work).  Each year is integrated into one of the engine's two one-year staging slots and reduced
 * there into one of two device output slots, which leaves on the copy stream while the following year integrates.
 * Device memory does not grow with `years` (the yearly scalars aside).  co2_ppm, yearly, the model clock, the state the
 * engine is left in and the kernels that integrate are those of greb_engine_run over the same years, bit for bit. */
int greb_engine_run_lin(greb_engine* e, int years, const float* co2_ppm, greb_lin* l, float* coef, float* rss, float* yearly);

/* ---- budget output through the plans: flux terms and their sums, reduced on the device --------------
 * The four plans above read a model year as [n_members][12][n_vars][ny][nx]; with n_vars = 5 that is a year of state
 * records.  The thirteen flux terms of greb_engine_run_budget exist only in the step loop and, in full, leave the device as
 * [n_members][years][12][13][ny][nx] -- which a many-member run cannot hold.  Here a year's budget records are reduced by
 * the same plans where they lie, either the thirteen terms themselves or up to GREB_MAX_RECORD_VARS linear combinations of
 * them (the surface net flux, the atmospheric net flux, evaporation plus rain: the right-hand sides of src/greb.f90:258,
 * :260, :263), formed BEFORE the reduction so that variances, ranges, quantiles and residuals are those of the sum. */
#define GREB_MAX_RECORD_VARS 16
/* greb_diag_create / greb_clim_create for records of n_vars variables per month, 1 ... GREB_MAX_RECORD_VARS (the two above
 * are these with n_vars = 5): every shape that says [5] above reads [n_vars] (seasons: [5 seasons][n_vars]), the arithmetic
 * and the order of every sum are the same.  The _dev calls take the count from the plan.  n_vars out of range is
 * GREB_E_INVALID with a message that names the value, decided on the host before any device query. */
int greb_diag_create_vars(int nx, int ny, const float* region_w, int n_regions, int n_vars, greb_diag** out);
int greb_clim_create_vars(int nx, int ny, int n_members, const int32_t* control, unsigned what, int n_vars, greb_clim** out);
/* The combination stage (greb_fluxes.hip): budget_year_dev [n_members][12][GREB_NBUDGET][np] -> out_dev
 * [n_members][12][n_out][np], np = ny * nx a multiple of four, both device pointers, 16-byte aligned and not overlapping;
 * combo[n_out][GREB_NBUDGET] is fp32 in HOST memory and travels by value in the kernel arguments.  Per element and output
 * k, over the terms j in ascending order, skipping those with combo[k][j] == 0: the first term used gives
 * acc = combo[k][j] * b_j, every later one acc = acc + combo[k][j] * b_j -- an fp32 multiply, then an fp32 add, never
 * fused.  A row with a single coefficient 1 copies the term's bits (-0.0 included).  Launches on the current device on
 * `stream` (a hipStream_t, may be NULL) and does not synchronise.  GREB_E_INVALID, with a message that names row and term:
 * n_out outside 1 ... GREB_MAX_RECORD_VARS, a row of zeros, a coefficient that is not finite.  Arguments are checked before
 * any device query; without a device: GREB_E_NOGPU (no CPU path). */
int greb_budget_combine_dev(const float* combo, int n_out, const float* budget_year_dev, int n_members, size_t np,
                            float* out_dev, void* stream);
/* greb_engine_run_diag / _clim / _ens / _lin over the year's BUDGET records instead of its state records: V variables per
 * month, V = GREB_NBUDGET with combo == NULL (the thirteen terms themselves; the combination stage does not run), else
 * V = n_out and the variables are the rows of combo.  Output shapes, delivery and device memory are those of the state
 * driver of the same name with 5 replaced by V: nothing on the device grows with `years` beyond what that driver keeps.
 * The year is integrated by the budget variant of the step kernels, as in greb_engine_run_budget (the five state records go
 * to a staging slot nobody reads); co2_ppm, yearly, the model clock and the state the engine is left in are those of
 * greb_engine_run over the same years, bit for bit, and switches, member forcing and boundary sets act as they do in
 * greb_engine_run_budget.  These calls, greb_engine_run and greb_engine_run_budget may alternate freely.
 * GREB_E_INVALID, decided before any device work and leaving the engine as it was: a diag or clim plan whose n_vars is not
 * V (the message names both numbers; likewise greb_engine_run_diag / greb_engine_run_clim with a plan whose n_vars is not
 * 5), a bad combo (as above), and whatever the state driver of the same name rejects. */
int greb_engine_run_budget_diag(greb_engine* e, int years, const float* co2_ppm, const float* combo, int n_out, greb_diag* d,
                                unsigned what, float* regions, float* zonal, float* annual, float* yearly);
int greb_engine_run_budget_clim(greb_engine* e, int years, const float* co2_ppm, const float* combo, int n_out, greb_clim* c,
                                int n_periods, const int32_t* first_year, const int32_t* n_years, float* mean, float* seasons,
                                float* trend, float* mean_resp, float* seasons_resp, float* yearly);
int greb_engine_run_budget_ens(greb_engine* e, int years, const float* co2_ppm, const float* combo, int n_out, greb_ens* s,
                               float* mean, float* var, float* min, float* max, float* quant, float* yearly);
int greb_engine_run_budget_lin(greb_engine* e, int years, const float* co2_ppm, const float* combo, int n_out, greb_lin* l,
                               float* coef, float* rss, float* yearly);

/* ---- covariance output: member-by-member Gram matrices, made on the device ------------------------
 * greb_lin reduces the members by contrasts the caller already knows.  Which contrasts are worth looking at -- the leading
 * modes of an ensemble's spread -- and how far each member's pattern lies from every other's both come from the Gram
 * matrix across the members, G[a][c] = sum_i v_a[i] v_c[i]: its eigenvectors are weight rows for greb_lin, and
 * G[a][a] + G[c][c] - 2 G[a][c] is the squared distance of two members.  It is the one reduction whose input is the whole
 * member x space x time volume and whose output is small.  A plan holds the grid and n_members; n_records, the records of
 * one member in a call (12 * n_vars for a model year); block[n_records] in -1 ... n_blocks-1 (-1: the record enters no
 * matrix); optionally use[n_members] (as greb_lin; U = the number of used members), control[n_members] (as greb_ens and
 * greb_lin; control[m] = m is legal and gives a row and a column of zeros) and scale[ny][nx] (fp32, finite, >= 0: e.g. the
 * square root of the cell area).  For record r, element i < len and used member m the sample is
 *   d = x[m][r][i]                          without a control map
 *   d = x[m][r][i] - x[control[m]][r][i]    with one, as ONE fp32 subtraction
 *   v = d  without `scale`,  v = fl32(scale[i] * d)  with it: one fp32 multiply (len must then be ny * nx)
 * and the matrices are formed in fp64, a and c counting the USED members in ascending member index:
 *   per record   P[r][a][c] = sum_i (double)v_a[i] * (double)v_c[i]   over ascending i, from +0.0, one add per element
 *   per block    G[b][a][c] = sum_{r: block[r] = b} P[r][a][c]        over ascending r, from +0.0
 * The product of two fp32 values is exact in fp64, so a fused multiply-add and a multiply followed by an add give the same
 * bits: either may be used.  What the definition forbids is reassociating the adds (no fast-math).  The output is fp64,
 * G[n_blocks][U][U], the full symmetric matrix; G[a][c] and G[c][a] carry identical bits.  (fp64 on purpose: centring
 * H G H and distances cancel 4-5 digits at climate magnitudes.)  Every output element has one owner (no atomics): results
 * are deterministic, a block's numbers depend neither on the other blocks nor on unused members, and a member with
 * use[m] = 0 that is no used member's control is never read. */
#define GREB_GRAM_MAX_BLOCKS 16
#define GREB_GRAM_MAX_USED   1024
typedef struct greb_gram greb_gram;
/* A plan.  Host work only, validated without touching a device.  GREB_E_INVALID with a message that names the offender
 * (greb_engine_last_error(NULL)): a grid greb_diag_create does not take, n_members < 1, n_records < 1, n_blocks outside
 * 1 ... 16, `block` NULL, a block index out of range (the message names the record), an empty block, a control index out
 * of range, a used member whose control is -1 while a control map is given, no used member, a scale that is negative or
 * not finite (the message names row and column).  GREB_E_UNSUPPORTED: more than GREB_GRAM_MAX_USED used members.  A plan
 * serves any number of calls and engines; its calls on one device share a scratch array (listed records x U x U doubles,
 * made with the first call there) and must not run side by side on different streams. */
int greb_gram_create(int nx, int ny, int n_members, int n_records, const int32_t* block, int n_blocks, const int32_t* use,
                     const int32_t* control, const float* scale, greb_gram** out);
int greb_gram_destroy(greb_gram* g); /* waits for the device before it frees the tables */
/* x_dev[n_members][n_records][len] on HIP device `device` (16-byte aligned; len is arbitrary without `scale`; the products
 * of greb_clim_finish_dev are valid input, e.g. seasons with n_records = 5 * n_vars) -> G_dev[n_blocks][U][U] doubles.
 * Launches on `stream` (a hipStream_t, may be NULL) and does not synchronise.  Arguments are checked before any device
 * query; without a device: GREB_E_NOGPU (no CPU path). */
int greb_gram_reduce_dev(greb_gram* g, int device, const float* x_dev, size_t len, double* G_dev, void* stream);
/* greb_engine_run that delivers ONLY the plan's matrices of each model year's monthly records, to host memory:
 *   G  [years][n_blocks][U][U] doubles
 * The plan must have n_records = 12 * 5; one made for another grid, member count or record count, or a NULL `G`, is
 * GREB_E_INVALID, decided before any device work.  Each year is integrated into one of the engine's two one-year staging
 * slots and reduced there into one of two device output slots, which leaves on the copy stream while the following year
 * integrates.  Device memory does not grow with `years` (the yearly scalars aside).  co2_ppm, yearly, the model clock, the
 * state the engine is left in and the kernels that integrate are those of greb_engine_run over the same years, bit for bit. */
int greb_engine_run_gram(greb_engine* e, int years, const float* co2_ppm, greb_gram* g, double* G, float* yearly);
/* ... over the year's BUDGET records, as greb_engine_run_budget_lin: the plan must have n_records = 12 * V. */
int greb_engine_run_budget_gram(greb_engine* e, int years, const float* co2_ppm, const float* combo, int n_out, greb_gram* g,
                                double* G, float* yearly);

/* ---- crossing output: when members pass thresholds, made on the device ------------------------------
 * greb_clim reduces the time axis linearly.  WHEN a member's annual-mean warming passes 2 K, whether it stays there, in
 * which year September's albedo first falls below 0.4, in what share of an ensemble that has happened by year y: a
 * threshold is not linear in the record, so neither the multi-year means of greb_clim nor the quantiles of greb_ens give
 * it (a mean crossing is not the years crossing, a quantile crossing is not a member crossing).  A plan holds the grid,
 * n_members, n_vars (1 ... GREB_MAX_RECORD_VARS), optionally control[n_members] (-1 ... n_members-1) and group[n_members]
 * (-1 ... n_groups-1, as greb_ens), the products `what` and 1 ... GREB_CROSS_MAX_EVENTS events:
 *   var  0 ... n_vars-1
 *   sel  0 ... 11 a calendar month; 12 ... 16 DJF, MAM, JJA, SON, ANN, the seasons of greb_clim (DJF = Dec, Jan, Feb of the
 *        SAME model year)
 *   rel  0, or 1: the member minus its control (needs a control map)
 *   dir  +1: a hit is q >= thr;  -1: a hit is q <= thr
 *   thr  a finite fp32
 * The year's quantity q of member m, event e, point i comes from one model year x[m][12][n_vars][ny][nx]:
 *   month selector   a = x[m][sel][var][i], the fp32 record itself
 *   season selector  acc = 0.0; acc = acc + jday_mon[mo] * (double)x[m][mo][var][i] over the season's months in calendar
 *                    order; a = (float)(acc / the season's days) -- greb_clim's seasons applied to one year, the same day
 *                    counts and divisors, no fused multiply-add: a has the bits of a one-year GREB_C_SEASONS
 *   rel = 0          q = a
 *   rel = 1          q = a - a_ctl as ONE fp32 subtraction (the greb_ens convention), a_ctl the same expression for
 *                    control[m]; a member with control[m] = -1 has q = a QUIET NaN; control[m] = m is legal and gives +0
 * A NaN never hits.  Over the years k = 0 ... n-1 added since the last finish, per (member, event, point):
 *   first       -1, then the first k that hits            last       -1, then the latest k that hits
 *   last_miss   -1, then the latest k that does not hit   count      the number of hits
 *   peak, peak_year   q of year 0 and 0; afterwards replaced by (q, k) when q > peak (dir = +1; q < peak for dir = -1) or when
 *                     peak is NaN and q is not: strict, so a tie keeps the earlier year
 * Year k = 0 STORES the state (no clearing pass); a plan serves any number of periods one after the other.  Products, each
 * [member][event][ny][nx] in the caller's event order:
 *   GREB_T_FIRST     int32  first                       GREB_T_LAST   int32  last
 *   GREB_T_STAY      int32  last_miss + 1 if that is <= n-1, else -1: the year from which the event holds to the end (0: always)
 *   GREB_T_COUNT     int32  count                       GREB_T_PEAK   fp32 peak and int32 peak_year: two arrays
 *   GREB_T_FRACTION  fp32 [year][group][event][ny][nx], per YEAR: (float)((double)c / (double)n_g), c the number of the
 *                    group's n_g members that hit in that year, counted in ascending member index: the group's exceedance
 *                    probability.  Needs a group map.
 * Years are 0-based within the call.  Every element has one owner (no atomics): results are deterministic and a member's
 * numbers do not depend on the batch it is in.
 * Device memory, per device on first use: only the state words the selected products need, 4 bytes each per (member,
 * event, point) -- FIRST, LAST, STAY, COUNT one word, PEAK two; all five: 24 bytes, i.e. 906 MB for 512 members x 16 events
 * at 96 x 48, 57 MB per event.  FRACTION adds one hit byte per (member, event, point) and two output slots of
 * [group][event][ny][nx].  Nothing grows with the number of years. */
#define GREB_T_FIRST    1u
#define GREB_T_LAST     2u
#define GREB_T_STAY     4u
#define GREB_T_COUNT    8u
#define GREB_T_PEAK     16u
#define GREB_T_FRACTION 32u
#define GREB_CROSS_MAX_EVENTS 16
#define GREB_CROSS_DJF 12 /* selectors behind the twelve months */
#define GREB_CROSS_MAM 13
#define GREB_CROSS_JJA 14
#define GREB_CROSS_SON 15
#define GREB_CROSS_ANN 16
typedef struct greb_cross_event {
  int32_t var, sel, rel, dir;
  float thr;
} greb_cross_event;
typedef struct greb_cross greb_cross;
/* A plan.  Host data only, validated without touching a device.  GREB_E_INVALID with a message that names the offender --
 * field, event index or member (greb_engine_last_error(NULL)): a grid greb_diag_create does not take, n_members < 1, n_vars
 * out of range, `what` zero or with unknown bits, n_events outside 1 ... 16 or `events` NULL, an event's var or sel out of
 * range, rel not 0 or 1 or rel = 1 without `control`, dir not +1 or -1, thr not finite, a control index out of range,
 * GREB_T_FRACTION without `group`; with `group`: n_groups outside 1 ... GREB_ENS_MAX_GROUPS, a group index out of range, an
 * empty group.  control and group may be NULL (n_groups is then not read). */
int greb_cross_create(int nx, int ny, int n_members, int n_vars, const greb_cross_event* events, int n_events,
                      const int32_t* control, const int32_t* group, int n_groups, unsigned what, greb_cross** out);
int greb_cross_destroy(greb_cross* c); /* waits for the device before it frees the state */
/* Year k (0-based) of the current period, one model year x_dev[n_members][12][n_vars][ny][nx] on HIP device `device` (16-byte
 * aligned), into the state; with GREB_T_FRACTION also that year's fraction_dev[n_groups][n_events][ny][nx] (16-byte aligned;
 * NULL is GREB_E_INVALID then, and the pointer is ignored otherwise).  k must be the number of years added since the last
 * finish.  Launches on `stream` (a hipStream_t, may be NULL) and does not synchronise; the calls of one period must be
 * ordered among themselves. */
int greb_cross_add_year_dev(greb_cross* c, int device, const float* x_dev, int k, float* fraction_dev, void* stream);
/* The maps of the n_years years added since the last finish (n_years must be that number) to device memory,
 * [n_members][n_events][ny][nx] each, 16-byte aligned.  A pointer whose product the plan does not select is ignored and
 * may be NULL; a selected product with a NULL pointer is GREB_E_INVALID (GREB_T_PEAK needs both peak_dev and
 * peak_year_dev).  Both _dev calls check their arguments before any device query; without a device they are GREB_E_NOGPU
 * (no CPU path). */
int greb_cross_finish_dev(greb_cross* c, int device, int n_years, int32_t* first_dev, int32_t* last_dev, int32_t* stay_dev,
                          int32_t* count_dev, float* peak_dev, int32_t* peak_year_dev, void* stream);
/* greb_engine_run that delivers ONLY the plan's products over the `years` years of this call (k = the year of the call),
 * to host memory: the maps [n_members][n_events][ny][nx], fraction [years][n_groups][n_events][ny][nx] (unselected products
 * as above).  The plan must have n_vars = 5; one made for another grid, member count or variable count, a selected
 * product with a NULL pointer or a plan with an unfinished period is GREB_E_INVALID, decided before any device work; a
 * refused call leaves the engine usable.  Each year is integrated into one of the engine's two one-year staging slots and
 * the state updated behind it on the same stream; a year's FRACTION is made in one of two device output slots and leaves
 * on the copy stream while the following year integrates; the maps are written once after the last year.  Without
 * GREB_T_FRACTION the run makes no copy stream and no events.  Device memory does not grow with `years` (the yearly
 * scalars aside).  co2_ppm, yearly, the model clock, the state the engine is left in and the kernels that integrate are
 * those of greb_engine_run over the same years, bit for bit. */
int greb_engine_run_cross(greb_engine* e, int years, const float* co2_ppm, greb_cross* c, int32_t* first, int32_t* last,
                          int32_t* stay, int32_t* count, float* peak, int32_t* peak_year, float* fraction, float* yearly);
/* ... over the year's BUDGET records, as greb_engine_run_budget_clim: the plan must have n_vars = V. */
int greb_engine_run_budget_cross(greb_engine* e, int years, const float* co2_ppm, const float* combo, int n_out, greb_cross* c,
                                 int32_t* first, int32_t* last, int32_t* stay, int32_t* count, float* peak, int32_t* peak_year,
                                 float* fraction, float* yearly);

/* ---- regression output: each member's records per unit of its own index, made on the device -----------
 * The other plans reduce along space, time, the members, into the fluxes and at thresholds; none relates a record to a
 * scalar the run itself produces.  The local change per degree of the member's OWN global-mean warming (pattern scaling),
 * polar amplification, albedo or humidity per degree: the regressor is known only once the year has been reduced in
 * space, so sum g*y over the years is not a function of any sums the other plans keep (greb_clim's TREND regresses on
 * the year number).  A plan holds the grid, n_members, n_vars (1 ... GREB_MAX_RECORD_VARS), the region weights
 * region_w[n_regions][ny][nx] as greb_diag_create takes them (region 0 is the globe), optionally control[n_members]
 * (-1 ... n_members-1), the products `what`, 1 ... GREB_REG_MAX_INDICES indices {var, sel, rel, region} and
 * 1 ... GREB_REG_MAX_TERMS terms {var, sel, rel, index}; var, sel and rel mean what they mean in greb_cross_event.
 * THE ORDER OF OPERATIONS IS THE DEFINITION:
 *   term quantity  y of year k, member m, point i: exactly greb_cross's quantity q of (var, sel, rel) -- a month selector
 *                  gives the fp32 record itself, a season selector the fp64 day-weighted sum in calendar order divided by
 *                  the season's days and rounded to fp32, rel = 1 ONE fp32 subtraction of the control's same expression,
 *                  a quiet NaN for a member without a control.
 *   index          g of year k, member m: r[mo] = the fp32 GREB_D_REGIONS value of (m, mo, var, region) under the plan's
 *                  weights, made by the device code of greb_diag_reduce_dev (the bits a greb_diag plan over the same
 *                  weights returns); a = r[sel] for a month selector, the season formula above applied to the twelve r
 *                  for a season selector; g = a for rel = 0, g = a - a_ctl as ONE fp32 subtraction for rel = 1 (a quiet
 *                  NaN without a control).
 *   state          fp64 sums of values centred on year 0.  Year k = 0 STORES y0 = y (fp32) and Sy = Sgy = Syy = 0 per
 *                  (member, term, point), g0 = g (fp32) and Sg = Sgg = 0 per (member, index): no clearing pass, a plan
 *                  serves period after period.  For k >= 1, G = (double)g - (double)g0, Y = (double)y - (double)y0 and
 *                    Sg = Sg + G    Sgg = Sgg + G*G    Sy = Sy + Y    Sgy = Sgy + G*Y    Syy = Syy + Y*Y
 *                  each one multiply, then one add, never fused.  A NaN propagates.  Centring makes a constant series
 *                  give exact zeros and loses nothing to the 288 K offset.
 *   finish         over n years, every step a separate fp64 operation:
 *                    Sxx = Sgg - Sg*Sg/n    Sxy = Sgy - Sg*Sy/n    Syc = Syy - Sy*Sy/n    b = Sxy/Sxx
 * Products, each rounded to fp32 once:
 *   GREB_R_SLOPE      [member][term][ny][nx]  (float)b
 *   GREB_R_INTERCEPT  [member][term][ny][nx]  (float)(((double)y0 + Sy/n) - b*((double)g0 + Sg/n))
 *   GREB_R_R2         [member][term][ny][nx]  (float)((Sxy*Sxy)/(Sxx*Syc))
 *   GREB_R_INDEX      per year [n_members][n_indices], the fp32 g; greb_engine_run_reg delivers [n_members][years][n_indices]
 * All three maps are a quiet NaN where n < 2 or Sxx is not > 0; R2 also where Syc is not > 0.  (No square root: its bits
 * would be the one thing numpy and the device might not share.)  Every element has one owner (no atomics): results are
 * deterministic and a member's numbers do not depend on the batch it is in.
 * Device memory, per device on first use: 20 bytes per (member, term, point) -- y0, Sy, Sgy -- and 8 more for Syy where
 * GREB_R_R2 is selected (28: 1.06 GB for 512 members x 16 terms at 96 x 48), the regional means of one year
 * [member][12][n_vars][1 + n_regions] with greb_diag's scratch, and 28 bytes per (member, index).  greb_engine_run_reg adds
 * one map [member][term][ny][nx] of floats, through which the selected maps leave one after the other, and with
 * GREB_R_INDEX the series [member][years][n_indices], the only thing that grows with the years. */
#define GREB_R_SLOPE     1u
#define GREB_R_INTERCEPT 2u
#define GREB_R_R2        4u
#define GREB_R_INDEX     8u
#define GREB_REG_MAX_INDICES 8
#define GREB_REG_MAX_TERMS   16
#define GREB_REG_MAX_MEMBERS 65535
typedef struct greb_reg_index {
  int32_t var, sel, rel, region;
} greb_reg_index;
typedef struct greb_reg_term {
  int32_t var, sel, rel, index;
} greb_reg_term;
typedef struct greb_reg greb_reg;
/* A plan.  Host data only, validated without touching a device.  GREB_E_INVALID with a message that names the offender --
 * field, index, term or member (greb_engine_last_error(NULL)): a grid greb_diag_create does not take, n_members outside
 * 1 ... GREB_REG_MAX_MEMBERS, n_vars,
 * n_regions, n_indices or n_terms out of range or their arrays NULL, `what` zero or with unknown bits, a region weight that
 * is not finite or outside [0, 1] or a region of zero weight (as greb_diag_create), an index's var, sel or region or a
 * term's var, sel or index out of range, rel not 0 or 1, rel = 1 without `control` -- of a term, of the index a term names,
 * or of an index no term names --, a control index out of range.  control may be NULL. */
int greb_reg_create(int nx, int ny, int n_members, int n_vars, const float* region_w, int n_regions, const int32_t* control,
                    const greb_reg_index* indices, int n_indices, const greb_reg_term* terms, int n_terms, unsigned what,
                    greb_reg** out);
int greb_reg_destroy(greb_reg* r); /* waits for the device before it frees the state */
/* Year k (0-based) of the current period, one model year x_dev[n_members][12][n_vars][ny][nx] on HIP device `device` (16-byte
 * aligned), into the state; with GREB_R_INDEX also that year's index_dev[n_members][n_indices] (NULL is GREB_E_INVALID
 * then, and the pointer is ignored otherwise).  k must be the number of years added since the last finish.  Launches on
 * `stream` (a hipStream_t, may be NULL) and does not synchronise; the calls of one period must be ordered among themselves. */
int greb_reg_add_year_dev(greb_reg* r, int device, const float* x_dev, int k, float* index_dev, void* stream);
/* The maps of the n_years years added since the last finish (n_years must be that number) to device memory,
 * [n_members][n_terms][ny][nx] each, 16-byte aligned.  A pointer whose product the plan does not select is ignored and
 * may be NULL; a selected product with a NULL pointer is GREB_E_INVALID.  Both _dev calls check their arguments before
 * any device query; without a device they are GREB_E_NOGPU (no CPU path). */
int greb_reg_finish_dev(greb_reg* r, int device, int n_years, float* slope_dev, float* intercept_dev, float* r2_dev, void* stream);
/* greb_engine_run that delivers ONLY the plan's products over the `years` years of this call, one period, to host memory:
 * the maps [n_members][n_terms][ny][nx], index [n_members][years][n_indices] (unselected products as above).  The plan must
 * have n_vars = 5; one made for another grid, member count or variable count, a selected product with a NULL pointer or
 * a plan with an unfinished period is GREB_E_INVALID, decided before any device work; a refused call leaves the engine
 * usable.  Each year is integrated into one of the engine's two one-year staging slots and reduced and added to the
 * state behind it on the same stream; nothing leaves before the end, and the run makes no copy stream and no events.
 * co2_ppm, yearly, the model clock, the state the engine is left in and the kernels that integrate are those of
 * greb_engine_run over the same years, bit for bit. */
int greb_engine_run_reg(greb_engine* e, int years, const float* co2_ppm, greb_reg* r, float* slope, float* intercept, float* r2,
                        float* index, float* yearly);
/* ... over the year's BUDGET records, as greb_engine_run_budget_clim: the plan must have n_vars = V. */
int greb_engine_run_budget_reg(greb_engine* e, int years, const float* co2_ppm, const float* combo, int n_out, greb_reg* r,
                               float* slope, float* intercept, float* r2, float* index, float* yearly);

/* ---- derived records: per-point expressions of state and flux terms, formed before the reduction ------
 * The three record sources above are linear in the records and have no constant term.  Relative humidity q / q_sat(T),
 * ice cover as an indicator (albedo >= 0.4), a wet-bulb temperature, the Bowen ratio, even degrees Celsius are not: their
 * mean, variance, quantile, crossing or regression cannot be made afterwards from the products of the plans, so the
 * quantity is formed from each month's record BEFORE the reduction (greb_derive.hip), where the year's records lie:
 *   state [n_members][12][5][np], budget [n_members][12][GREB_NBUDGET][np] where the program names a term
 *     ->  derived [n_members][12][n_out][np]
 * which every plan kind reduces exactly as it reduces the rows of a combo.  A plan holds the grid, n_out outputs
 * (1 ... GREB_MAX_RECORD_VARS), per output a postfix program of greb_derive_ins and up to GREB_DERIVE_MAX_FIELDS 2-D
 * fields [n_fields][ny][nx] of the caller's (exp(-z_topo / z_air), a land mask).  THE FIELDS ARE SHARED BY ALL MEMBERS: a
 * member on a boundary set that replaces z_topo still sees the field the caller passed.  Limits: per output at most
 * GREB_DERIVE_MAX_INS instructions, a stack of at most GREB_DERIVE_MAX_STACK values and GREB_DERIVE_MAX_LOCALS locals; at
 * most GREB_DERIVE_MAX_TOTAL instructions in all.  An output's program runs on an empty stack and must leave one value.
 *   push     GREB_DV_STATE i (0 ... 4: Tsurf, Tair, Tocean, q, albedo)   GREB_DV_TERM j (0 ... GREB_NBUDGET - 1)
 *            GREB_DV_FIELD f (0 ... n_fields - 1)   GREB_DV_CONST value
 *   locals   GREB_DV_TEE k: copy the top to local k, keep it on the stack   GREB_DV_GET k: push local k (set earlier in
 *            the same output)
 *   binary   pops b, then a, pushes  ADD a + b   SUB a - b   MUL a * b   DIV a / b   MIN a < b ? a : b   MAX a > b ? a : b
 *            GE a >= b ? 1 : 0   LT a < b ? 1 : 0
 *   unary    NEG (the sign bit flipped)  ABS  SQRT  EXP  LOG  ATAN
 *   ternary  GREB_DV_SELECT pops b, a, c and pushes c != 0 ? a : b
 * THE SEMANTICS ARE THE DEFINITION OF THE RESULTS: every arithmetic op is one IEEE fp32 operation with one rounding,
 * nothing is fused or reassociated; DIV and SQRT are correctly rounded; MIN and MAX are the comparisons written above, so
 * a NaN in b is taken and a NaN in a is not; GE and LT are false with a NaN, SELECT takes a for a NaN condition; EXP, LOG
 * and ATAN convert the fp32 operand to fp64, call the fp64 function and round once to fp32 (two fp64 libraries may differ
 * in the last fp64 bit, which moves the fp32 result only next to a rounding boundary).  Operands or results of DIV and
 * SQRT that are subnormal in fp32 are outside this contract.  derive.reference in Python performs the same operations. */
#define GREB_DERIVE_MAX_INS    64
#define GREB_DERIVE_MAX_TOTAL  512
#define GREB_DERIVE_MAX_STACK  8
#define GREB_DERIVE_MAX_LOCALS 4
#define GREB_DERIVE_MAX_FIELDS 8
#define GREB_DV_STATE  0
#define GREB_DV_TERM   1
#define GREB_DV_FIELD  2
#define GREB_DV_CONST  3
#define GREB_DV_TEE    4
#define GREB_DV_GET    5
#define GREB_DV_ADD    6
#define GREB_DV_SUB    7
#define GREB_DV_MUL    8
#define GREB_DV_DIV    9
#define GREB_DV_MIN    10
#define GREB_DV_MAX    11
#define GREB_DV_GE     12
#define GREB_DV_LT     13
#define GREB_DV_NEG    14
#define GREB_DV_ABS    15
#define GREB_DV_SQRT   16
#define GREB_DV_EXP    17
#define GREB_DV_LOG    18
#define GREB_DV_ATAN   19
#define GREB_DV_SELECT 20
typedef struct greb_derive_ins {
  int32_t op;  /* GREB_DV_* */
  int32_t arg; /* STATE, TERM, FIELD, TEE, GET: the index; else ignored */
  float value; /* CONST: the value; else ignored */
} greb_derive_ins;
typedef struct greb_derive greb_derive;
/* A plan: ins holds the programs of the outputs one after the other, n_ins[n_out] their lengths; fields may be NULL with
 * n_fields = 0.  Host work only, validated without touching a device.  GREB_E_INVALID with a message that names output
 * and instruction (greb_engine_last_error(NULL)): an unknown op, an index out of range, stack underflow, anything but
 * exactly one value left at the end, a stack deeper than GREB_DERIVE_MAX_STACK, a GET of a local not set earlier in the
 * same output, a CONST that is not finite, a count outside its limit, a field value that is not finite (the message names
 * field, row and column), FIELD with n_fields = 0, a grid greb_diag_create does not take. */
int greb_derive_create(int nx, int ny, const greb_derive_ins* ins, const int32_t* n_ins, int n_out, const float* fields,
                       int n_fields, greb_derive** out);
int greb_derive_destroy(greb_derive* v); /* waits for the device before it frees the program's copy */
int greb_derive_uses_budget(const greb_derive* v); /* 1: some output names a TERM; 0: none (or v is NULL) */
/* One model year on HIP device `device`: state_year_dev [n_members][12][5][ny][nx] and budget_year_dev
 * [n_members][12][GREB_NBUDGET][ny][nx] (NULL allowed if and only if no output names a TERM) -> out_dev
 * [n_members][12][n_out][ny][nx]; all 16-byte aligned, out_dev overlapping neither input.  Every input record some output
 * names is read once, every output written once.  Launches on `stream` (a hipStream_t, may be NULL) and does not
 * synchronise.  Arguments are checked before any device query; without a device: GREB_E_NOGPU (no CPU path). */
int greb_derive_apply_dev(greb_derive* v, int device, const float* state_year_dev, const float* budget_year_dev, int n_members,
                          float* out_dev, void* stream);
/* The seven reduced runs over the DERIVED records of each year: V = the plan's n_out variables per month.  Shapes,
 * delivery and device memory are those of the driver of the same name with 5 replaced by V, plus one year of derived
 * records the engine keeps.  A program without a TERM is integrated by the kernels greb_engine_run_diag, ... launch (no
 * budget instantiation, budget_runs not counted); one with a TERM as greb_engine_run_budget_diag, ... integrate.  The
 * stage is enqueued behind the year on the compute stream.  co2_ppm, yearly, the model clock and the state the engine is
 * left in are those of greb_engine_run over the same years, bit for bit.  GREB_E_INVALID, decided before any device work
 * and leaving the engine as it was: `v` NULL or of another grid, a plan whose n_vars (gram: n_records / 12) is not V, and
 * whatever the state driver of the same name rejects. */
int greb_engine_run_derived_diag(greb_engine* e, int years, const float* co2_ppm, greb_derive* v, greb_diag* d, unsigned what,
                                 float* regions, float* zonal, float* annual, float* yearly);
int greb_engine_run_derived_clim(greb_engine* e, int years, const float* co2_ppm, greb_derive* v, greb_clim* c, int n_periods,
                                 const int32_t* first_year, const int32_t* n_years, float* mean, float* seasons, float* trend,
                                 float* mean_resp, float* seasons_resp, float* yearly);
int greb_engine_run_derived_ens(greb_engine* e, int years, const float* co2_ppm, greb_derive* v, greb_ens* s, float* mean,
                                float* var, float* min, float* max, float* quant, float* yearly);
int greb_engine_run_derived_lin(greb_engine* e, int years, const float* co2_ppm, greb_derive* v, greb_lin* l, float* coef,
                                float* rss, float* yearly);
int greb_engine_run_derived_gram(greb_engine* e, int years, const float* co2_ppm, greb_derive* v, greb_gram* g, double* G,
                                 float* yearly);
int greb_engine_run_derived_cross(greb_engine* e, int years, const float* co2_ppm, greb_derive* v, greb_cross* c, int32_t* first,
                                  int32_t* last, int32_t* stay, int32_t* count, float* peak, int32_t* peak_year, float* fraction,
                                  float* yearly);
int greb_engine_run_derived_reg(greb_engine* e, int years, const float* co2_ppm, greb_derive* v, greb_reg* r, float* slope,
                                float* intercept, float* r2, float* index, float* yearly);

/* ---- per-member forcing: regional and seasonal CO2, insolation tables and scale --------------------
 * Members of one engine may differ in the forcing itself, not only in the CO2 level: CO2 raised in one hemisphere, over
 * land or ocean only or in one half of the year, a changed solar constant, a changed latitudinal or seasonal distribution
 * of insolation.  A few small tables shared by the engine, four words per member, all of it used in the point physics
 * only; members that differ only in forcing still share one flux-correction set.  For member m, point p of row j, step
 * ityr (1-based) of scenario year y, with k = co2_pattern and t = solar_table (fl: one fp32 rounding; no contraction, in
 * both arithmetic modes):
 *   k >= 0:  w   = fl(space[k][p] * season[k][ityr-1])
 *            co2 = fl( fl(w * co2_ppm[m][y]) + fl( fl(1 - w) * co2_ref[m] ) )
 *   k <  0:  co2 = co2_ppm[m][y]
 *   S     = (t >= 0 ? sw_solar[t] : the engine's greb_fields.sw_solar)[ityr-1][j]
 *   solar = fl(S * solar_scale[m]),   then sw = solar * (1 - albedo) as src/greb.f90:399
 * so that w = 1 gives co2_ppm bit for bit, w = 0 gives co2_ref, and solar_scale = 1 gives S.
 * Scope: the scenario phase -- greb_engine_run, greb_engine_run_budget, greb_engine_run_diag, whose signatures are
 * unchanged.  greb_engine_flux_correction ignores it, as it ignores GREB_X_SST_PLUS1.  A launch with any forced member
 * takes forcing-aware instantiations of the kernels for all its members; with no forced member the engine launches
 * exactly the kernels it launches without any of this.
 * GREB_E_INVALID, with a message that names the offender: n_patterns or n_solar outside 0 ... GREB_MAX_FORCING_TABLES, a
 * weight that is not finite or lies outside [0, 1], a negative or non-finite table value, an index out of range, co2_ref
 * not finite or <= 0, solar_scale not finite or < 0.  A failed call leaves the engine exactly as it was. */
#define GREB_MAX_FORCING_TABLES 16
/* Tables shared by all members; copied to the device; may be called again (replaces them).  Replacing them with fewer
 * tables than a member's current forcing names is GREB_E_INVALID: change or clear the member forcing first. */
int greb_engine_set_forcing_tables(greb_engine* e,
      int n_patterns, const float* co2_space  /* [n_patterns][ny][nx], weights in [0,1] */,
                      const float* co2_season /* [n_patterns][730] in [0,1]; NULL = 1 everywhere */,
      int n_solar,    const float* sw_solar   /* [n_solar][730][ny], W/m2, >= 0 */);
typedef struct greb_member_forcing {
  int32_t co2_pattern;  /* -1: none, CO2 is the member's scalar as today; else 0 .. n_patterns-1 */
  float   co2_ref;      /* CO2 where the weight is 0 */
  int32_t solar_table;  /* -1: the engine's own sw_solar; else 0 .. n_solar-1 */
  float   solar_scale;  /* multiplies the table; 1 = unchanged */
} greb_member_forcing;
/* f[n_members]; NULL = every member {-1, ., -1, 1}.  Cheap: four words per member.  Takes effect from the next run call.
 * A member is forced when it names a pattern or a table or its scale is not 1 (greb_engine_describe: "forcing"). */
int greb_engine_set_member_forcing(greb_engine* e, const greb_member_forcing* f);

/* ---- prescribed SST: anomaly patterns, nudging weights and seasons per member -------------------------
 * Members of one engine may differ in the ocean surface temperature they are held to: one SST patch per member beside a
 * fixed-SST control (Green's-function ensembles), SST prescribed in one basin with a buffer zone and a free ocean elsewhere
 * (pacemaker runs), an anomaly that changes sign through the year, an ocean held at its climatology under changed CO2.
 * GREB_X_SST_PLUS1 is the one case anomaly = 1 K everywhere.  A few tables shared by the engine, two words per member, all
 * of it used in the point physics only; members that differ only in this still share one flux-correction set.  For member
 * m with pattern k >= 0, in the scenario phase, at every point p with z_topo < 0 (the member's own boundary set's field)
 * and step ityr (1-based), before the step's physics, where greb.original.model.f90:226 acts (fl: one fp32 rounding; no
 * contraction, in both arithmetic modes):
 *   a      = fl( fl(anom[k][p] * season[k][ityr-1]) * amp[m] )
 *   target = fl( tclim_m[slice of the PREVIOUS step][p] + a )      tclim_m: tclim of the member's boundary set; the slice
 *                                                                  is the switch's: 730 at ityr = 1
 *   w      = weight[k][p]                                          (no weight table: 1 everywhere)
 *   Ts     = fl( fl(w * target) + fl( fl(1 - w) * Ts ) )
 * so that w = 1 gives target bit for bit and w = 0 leaves Ts bit for bit; without a weight table Ts = target.  Land points
 * are never touched.  A member that also has GREB_X_SST_PLUS1: the switch acts first, the blend on its result.  With
 * anom = 1 everywhere, no weight table and amp = 1 a member equals a member with GREB_X_SST_PLUS1 bit for bit.
 * Scope: the scenario phase -- every greb_engine_run* call, whose signatures are unchanged.  greb_engine_flux_correction
 * ignores it, as it ignores forcing and GREB_X_SST_PLUS1.  A launch with any prescribed member takes the forcing-aware
 * instantiations of the kernels for all its members (a member without a pattern pays one scalar test per step there); with
 * no prescribed and no forced member the engine launches exactly the kernels it launches without any of this.
 * GREB_E_INVALID, with a message that names the offender: n_patterns outside 0 ... GREB_MAX_SST_PATTERNS, anom NULL with
 * n_patterns > 0, an anomaly, season factor or amplitude that is not finite, a weight that is not finite or lies outside
 * [0, 1], a pattern index out of range.  A failed call leaves the engine exactly as it was. */
#define GREB_MAX_SST_PATTERNS 1024
/* Tables shared by all members; copied to the device; may be called again (replaces them).  Replacing them with fewer
 * patterns than a member's current SST names is GREB_E_INVALID: change or clear the member SST first. */
int greb_engine_set_sst_tables(greb_engine* e,
      int n_patterns, const float* anom   /* [n_patterns][ny][nx], K */,
                      const float* weight /* [n_patterns][ny][nx] in [0,1]; NULL = 1 everywhere */,
                      const float* season /* [n_patterns][730], any finite value; NULL = 1 everywhere */);
typedef struct greb_member_sst {
  int32_t pattern;  /* -1: none, the ocean surface is free as today; else 0 .. n_patterns-1 */
  float   amp;      /* multiplies the pattern's anomaly; 0 holds the weighted points at the climatology */
} greb_member_sst;
/* s[n_members]; NULL = every member {-1, .}.  Cheap: two words per member.  Takes effect from the next run call.  A member
 * is prescribed when it names a pattern (greb_engine_describe: "sst": {"patterns", "prescribed_members"}); it is not
 * counted among the forced members of "forcing". */
int greb_engine_set_member_sst(greb_engine* e, const greb_member_sst* s);

/* ---- stochastic heat flux: surface heat-flux noise per member, reproducible by seed --------------------
 * Members of one engine may differ in nothing but their weather: an initial-condition ensemble, a signal-to-noise figure
 * for the spread, range, quantile, mode, crossing and regression outputs, Hasselmann's stochastic climate model (weather
 * noise in the surface heat flux, integrated by the mixed layer into red SST variability).  The noise is generated where
 * it is used, in the point physics: a few tables shared by the engine, four words per member; members that differ only in
 * this still share one flux-correction set.  A member's realisation is a pure function of its 64-bit seed and the scenario
 * step -- not of the member index, the engine size, the workgroup that integrates it or how the years are split into run
 * calls.  For member m with pattern k >= 0, at point (j, i) (row, longitude; 0-based) and scenario step n -- the engine's
 * scenario clock, counted 0-based since creation, running on across run* calls and not advanced by flux_correction:
 *   cell  = (j / cell_y[k]) * (nx / cell_x[k]) + i / cell_x[k]               integer division
 *   b     = n / hold[k]                                                       64 bit
 *   (w0,w1,w2,w3) = Philox4x32-10( counter = (cell >> 1, low32(b), high32(b), 0), key = (seed_lo[m], seed_hi[m]) )
 *   (wa, wb) = cell even ? (w0, w1) : (w2, w3)
 *   S     = (wa & 0xffff) + (wa >> 16) + (wb & 0xffff) + (wb >> 16)           0 ... 262140, exact
 *   z     = fl( fl(float(S) - 131070.0f) * C ),  C = 0x37DDB3D7 as fp32 (2.6428997e-05 = fl(sqrt(3 / (65536^2 - 1))))
 *   N     = fl( fl( fl(sigma[k][p] * season[k][ityr-1]) * amp[m] ) * z )      W/m2
 *   TF'   = fl( TF + N )
 * (fl: one fp32 rounding; no contraction, in both arithmetic modes).  TF' takes the place of the step's flux correction in
 * the scenario update of Tsurf (src/greb.f90:258): a heat flux into the surface layer at every point where sigma is not 0,
 * land included; nothing else of the update changes.  Philox4x32-10 is the published function (multipliers 0xD2511F53,
 * 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85); integer operations only.  z is a sum of four 16-bit uniforms: mean 0,
 * variance 1, |z| <= 3.4641, excess kurtosis -0.3 -- deliberately not Gaussian: no log or cos whose bits would differ
 * between libraries, and the mixed layer sums hundreds of deviates in any case.  cell_x, cell_y give the noise a spatial
 * scale (the last cell row may be short), hold a persistence (the deviate is held for `hold` steps; 6 is three days).  The
 * pattern index is not part of the counter: two members with the same seed on different sigma maps see the same weather,
 * scaled (common random numbers).
 * Scope: the scenario phase -- every greb_engine_run* call, whose signatures are unchanged.  greb_engine_flux_correction
 * ignores it.  The noise is not a budget term (GREB_NBUDGET stays 13): the flux terms of a noisy member are those of its
 * noisy state.  A launch with any noisy member takes the forcing-aware instantiations of the kernels for all its members (a
 * member without a pattern pays one scalar test per step there); with no noisy, prescribed or forced member the engine
 * launches exactly the kernels it launches without any of this.
 * GREB_E_INVALID, with a message that names the offender: n_patterns outside 0 ... GREB_MAX_NOISE_PATTERNS, sigma NULL with
 * n_patterns > 0, a sigma or season factor that is negative or not finite, cell_x not 1, 2 or 4, cell_y outside 1 ... ny,
 * hold < 1, a pattern index out of range, an amplitude that is not finite.  A failed call leaves the engine exactly as it
 * was. */
#define GREB_MAX_NOISE_PATTERNS 16
/* Tables shared by all members; copied to the device; may be called again (replaces them).  Replacing them with fewer
 * patterns than a member's current noise names is GREB_E_INVALID: change or clear the member noise first. */
int greb_engine_set_noise_tables(greb_engine* e,
      int n_patterns, const float* sigma     /* [n_patterns][ny][nx] W/m2, finite, >= 0 */,
                      const float* season    /* [n_patterns][730] finite, >= 0; NULL = 1 everywhere */,
                      const int32_t* cell_x  /* [n_patterns] 1, 2 or 4; NULL = 1 */,
                      const int32_t* cell_y  /* [n_patterns] 1 ... ny; NULL = 1 */,
                      const int32_t* hold    /* [n_patterns] >= 1; NULL = 1 */);
typedef struct greb_member_noise {
  int32_t  pattern;           /* -1: none, the member is deterministic as today; else 0 .. n_patterns-1 */
  float    amp;               /* multiplies the pattern's sigma; 0 takes the noise path and adds +-0 */
  uint32_t seed_lo, seed_hi;  /* the member's 64-bit seed: the Philox key */
} greb_member_noise;
/* s[n_members]; NULL = every member {-1, ...}.  Cheap: four words per member.  Takes effect from the next run call.  A
 * member is noisy when it names a pattern (greb_engine_describe: "noise": {"patterns", "noisy_members"}); it is not
 * counted among the forced members of "forcing" or the prescribed members of "sst". */
int greb_engine_set_member_noise(greb_engine* e, const greb_member_noise* s);
/* N of the formula above for member `member` (which must name a pattern) at scenario step `step` (>= 0; any step, also
 * one the clock has not reached), out[ny][nx]: evaluated on the device by the function the step kernels call. */
int greb_engine_get_noise(greb_engine* e, int member, int64_t step, float* out);

/* ---- boundary sets: members of one engine on different boundary data --------------------------------
 * Members of one engine may differ in the boundary fields themselves: a changed cloud, wind, soil-moisture or vapour
 * climatology, a removed ice sheet, flat topography, a constant mixed layer -- each beside an unchanged control member.
 * A boundary set replaces some of the engine's fields; a member names one set (0 = the engine's own data).  Only the
 * replaced fields are copied to the device, the others alias the engine's.  The derived fields follow their source as
 * greb_engine_create makes them: wz_air / wz_vapor where z_topo is replaced, Toclim where tclim is, z_ocean where mldclim
 * is.  Both phases: a member integrates its flux corrections towards its own set's tclim, qclim and Toclim, and
 * GREB_X_SST_PLUS1 / GREB_X_LW_LINEAR_VAPOR read the member's set.  sw_solar is not part of a set (per-member insolation is
 * forcing: greb_engine_set_forcing_tables); a non-NULL over->sw_solar is GREB_E_INVALID.
 * A launch in which any member names a set above 0 takes boundary-aware instantiations of the kernels for all its members;
 * with every member on set 0 the engine launches exactly the kernels it launches without any of this.
 * On the any-grid engine (latitude bands, row strips) the transport kernels run all members of a launch with one pair of
 * weights and one wind slice: a member that names a set which replaces z_topo, uclim or vclim is GREB_E_UNSUPPORTED there
 * (create an engine with those fields, or ensemble.run_beside); sets of glacier, tclim, qclim, mldclim, cldclim, swetclim
 * work on every engine.
 * GREB_E_INVALID, with a message that names the offender: `over` NULL or all-NULL, more than GREB_MAX_BOUNDARY_SETS sets,
 * a value that is not finite (field and index of the first), a set index outside 0 ... sets made, unknown flag bits.
 * A failed call of either function leaves the engine exactly as it was (and consumes no set id). */
#define GREB_MAX_BOUNDARY_SETS 16
/* over: a greb_fields whose non-NULL pointers replace the engine's own field of that name for the members that name
 * this set; NULL = inherit.  Shapes as in greb_engine_create.  *set_id = 1 .. GREB_MAX_BOUNDARY_SETS (0 is the
 * engine's own data). */
int greb_engine_add_boundary_set(greb_engine* e, const greb_fields* over, int* set_id);
/* also set each member's state to the initial state of its set (src/greb.f90:190-197): Ts = Ta = tclim[729], To = Toclim,
 * q = qclim[729], cap_surf from the set's z_topo / mldclim[0] and the member's own physics.  The deconstruction use: call
 * it before flux_correction.  Without it the state is untouched -- the response use: spin up under the control data, then
 * change a member's clouds. */
#define GREB_BS_REINIT 1u
/* set[n_members], 0 = the engine's own; NULL = every member 0.  Takes effect from the next flux_correction / run call.
 * Members whose sets differ need a flux-correction set each: an engine that shared one gives every member a copy, as
 * greb_engine_set_member_experiments does; members that all name the same set keep sharing one. */
int greb_engine_set_member_boundary(greb_engine* e, const int32_t* set, unsigned flags);

/* ---- sensitivity-experiment switches -----------------------------------------
 * Runtime switches on the same kernels that reproduce the `log_exp` experiments of the upstream model
 * variant (src/greb.original.model.f90:60,162-166,394,423-430,452-453,492-495,513-515,553-571; doc in its
 * namelist_original).  greb_log_exp_switches() maps a log_exp value to the process switches below; the
 * experiment's changes to the BOUNDARY DATA (constant topography / clouds / vapour / mixed layer, :162-166) are a boundary
 * set (above) or an engine created on the changed fields; its CO2 series (A1B ramp, :939-951) and the run sequencing
 * (control run, :208-215) stay with the host (greb_climate_model_amd/original.py shows all three).  Default 0 = the complete model = src/greb.f90. */
#define GREB_X_NO_ICE            (1u << 0) /* log_exp <= 5: a_surf = a_no_ice (:394); heat capacity ignores sea ice (:492-495) */
#define GREB_X_NO_HYDRO          (1u << 1) /* <= 6, 13, 15: no latent heat, evaporation, rain (:452-453) */
#define GREB_X_NO_DEEP_OCEAN     (1u << 2) /* <= 9, 11, 14-16: dT_ocean = dTo = 0 (:513-515) */
#define GREB_X_LW_LINEAR_VAPOR   (1u << 3) /* 11: emissivity linear in q around qclim (:423,:430) */
#define GREB_X_NO_CIRCULATION    (1u << 4) /* <= 4: no transport of Tair and q (:553; the original's increment is
                                              unassigned there -- defined as 0 here) */
#define GREB_X_NO_VAPOR_TRANSPORT (1u << 5) /* 7, 16: no transport of q (:554-555; same remark) */
#define GREB_X_VAPOR_DIFFUSION_ONLY (1u << 6) /* 8: q is diffused but not advected (:560-564) */
#define GREB_X_SST_PLUS1         (1u << 7) /* 14-16: before every scenario step Tsurf(ocean) = Tclim(previous step's
                                              slice) + 1 K (:226, evaluated before time_loop updates ityr);
                                              not applied in the flux-correction phase.  The host clears it for
                                              the control run and passes CO2 = CO2_ctrl (:225) */
unsigned greb_log_exp_switches(int log_exp);
/* Takes effect from the next flux_correction / run call; every member gets `switches`. */
int greb_engine_set_experiment(greb_engine* e, unsigned switches);
/* One switch word per member, switches[n_members]; takes effect from the next call.  An engine whose members share one
 * flux-correction set gives every member a copy of it when the switches now differ (n_members sets; spin up once under
 * the complete model, then let the members diverge); if that allocation fails the HIP error is returned and the engine
 * is as it was.  greb_engine_set_experiment never does this. */
int greb_engine_set_member_experiments(greb_engine* e, const uint32_t* switches);

/* Flux-correction cache: TF/qF/ToF_correct [3][730][ny][nx] + cap_surf +
 * the four state fields Ts,Ta,To,q [5][ny][nx] of one member. */
int greb_engine_get_corrections(greb_engine* e, int member, float* corr, float* state5);
int greb_engine_set_corrections(greb_engine* e, int member, const float* corr, const float* state5);

/* Current state of one member: Ts, Ta, To, q, cap_surf [5][ny][nx]; set: member -1 = every member
 * (== greb_engine_set_corrections(e, member, NULL, state5), for hosts that cannot pass a null array). */
int greb_engine_get_state(greb_engine* e, int member, float* state5);
int greb_engine_set_state(greb_engine* e, int member, const float* state5);

const char* greb_engine_last_error(const greb_engine* e);
int greb_engine_destroy(greb_engine* e);

/* Device + build info as a static JSON string (CU count, clocks, arch). */
const char* greb_device_info(int device);

/* ---- single-routine entry points over a batch dimension (tests + roofline bench) --------
 * Mirrors of the reference routines' signatures with a leading batch count; all pointers are
 * HOST pointers unless the name ends in _dev.  `p` supplies pi/kappa/dt_crcl.
 *   diffusion  src/greb.f90:556-723   dX = wz*(dTx+dTy)
 *   advection  src/greb.f90:726-915   winds u,v are the raw climatology slice (sign split inside)
 *   circulation src/greb.f90:528-553  24 sub-steps of X += diffusion + advection
 * Shapes: T1, wz, dX, u, v : [batch][ny][nx].  strict: 0/1 as GREB_F_STRICT. */
int greb_diffusion_batched(const greb_params* p, int nx, int ny, int batch, const float* T1,
                           const float* wz, float* dX, int strict, int device);
int greb_advection_batched(const greb_params* p, int nx, int ny, int batch, const float* T1,
                           const float* wz, const float* u, const float* v, float* dX, int strict,
                           int device);
int greb_circulation_batched(const greb_params* p, int nx, int ny, int batch, const float* X,
                             const float* wz, const float* u, const float* v, float* dX, int strict,
                             int device);
/* Device-pointer form of the diffusion sweep for the HBM-roofline measurement: launches
 * `sweeps` back-to-back sweeps on `stream` (a hipStream_t, may be NULL) and returns without
 * synchronising.  Algorithmic traffic = 12 B/point/member-sweep. */
int greb_diffusion_batched_dev(const greb_params* p, int nx, int ny, int batch, const float* T1_dev,
                               const float* wz_dev, float* dX_dev, int strict, int sweeps,
                               void* stream);
/* greb_diffusion_batched_dev keeps small immutable tables per device between calls (row constants, the launch order of
 * the 384-wide sweep) so that back-to-back sweeps are not separated by an allocation.  A table is never rewritten once
 * made -- calls on different streams or threads, with different kappa or batch, do not disturb each other -- and a
 * long-lived host releases them with this (it waits for the device first).  Engines are unaffected. */
int greb_release_caches(void);
/* Diagnostic, host only (no GPU call): the launch order of the 384-wide diffusion sweep for a batch of fields, as
 * greb_diffusion_batched_dev would use it -- task i updates rows [k0[i], k1[i]) of field[i] (field < 0: an empty
 * slot), walking south to north where up[i] != 0.  Returns the number of tasks (only the first `capacity` are
 * written), 0 when the grid does not take that kernel, < 0 on a bad argument.  Any order is the same arithmetic;
 * tests check that every row of every field is written exactly once. */
int greb_diffusion_launch_order(const greb_params* p, int nx, int ny, int batch, int* field, int* k0, int* k1, int* up,
                                int capacity);
/* The same for the engine's row-strip circulation in its one-launch-per-sub-step form (384- and 192-wide grids): field = 2 * member + tracer; kappa:
 * [n_members] diffusivities (own sub-cycle tables) or NULL for p->kappa everywhere.  The order is the one an MI355X
 * (256 compute units) gets: at most one task per wavefront slot (2 048), tasks i and i + 1 024 share a SIMD. */
int greb_substep_launch_order(const greb_params* p, int nx, int ny, int n_members, const float* kappa, int* field, int* k0,
                              int* k1, int capacity);

/* The tasks of the engine's ONE-LAUNCH circulation call (greb_circ_rows.hip; src/greb.f90:546-550: the 24 sub-steps of a
 * `circulation` call inside one kernel) for `slots` wavefront slots: per task the field (2 * member + tracer), its rows
 * [k0, k1), whether it is a chain task (one row whose zonal chains stay in registers for the whole call) and up to four
 * dependencies dep4[4 * i .. 4 * i + 3] (task indices, -1 = none): the owners of rows k0-2, k0-1, k1, k1+1 of the same
 * field, whose completed sub-step s - 1 a task waits for before it starts sub-step s.  Host-only (no GPU call).
 * Returns the number of tasks -- never more than `slots` -- or 0 when the grid does not take this kernel or the slots
 * do not suffice (the engine then launches once per sub-step), or < 0. */
int greb_circulation_launch_plan(const greb_params* p, int nx, int ny, int n_members, const float* kappa, int slots,
                                 int* field, int* k0, int* k1, int* chain, int* dep4, int capacity);

/* Diagnostic, host only (no GPU call): how often one circulation sub-step of the fused 96x48 member kernel computes each
 * 4-longitude quad of each row under the kernel's static work deal (greb_member_deal.h), FAST (strict = 0) or STRICT:
 * counts[48 * 24], counts[k * 24 + q].  A complete deal has 1 for rows 1 .. 46 and 0 for the polar rows 0 and 47,
 * which have their own wave(s); the library asserts this when it is compiled, this is the same table for tests.
 * Returns 0, < 0 on a bad argument. */
int greb_member_deal_cover(int strict, int* counts);

/* Diagnostic, host only (no GPU call): the LDS accesses of one circulation sub-step of the fused 96x48 member kernel's bulk
 * waves, FAST (strict = 0) or STRICT, made from the kernel's own deal, task enumeration and LDS map (tools/lds_conflicts.py
 * applies the LDS's lane groups and bank rule to them).  One record of 7 ints per lane of every LDS instruction of every
 * dealt pass: wave, pass slot of the wave, number of the instruction within the pass, lane, kind (0 column read, 1 left /
 * right quad read, 2 wind read, 3 store, 4 row-constant read), bytes per lane, float offset into the workgroup's LDS
 * (-1: the lane has no task in this pass).  The wave(s) of the polar rows are not listed.  At most `capacity` records are
 * written (records may be NULL with capacity 0); returns the number of records there are, or < 0 on a bad argument. */
int greb_member_lds_table(int strict, int* records, int capacity);
/* The LDS map those offsets point into, 8 ints in floats: the stride of a row of X and W; where X[0], X[1] and W begin (each
 * 50 rows: 48 and a zero guard row on either side), where the winds WX and WY (48 x 96 each) and the row constants begin,
 * and where the last ends (the kernel's LDS size).  Returns 0, < 0 on a bad argument. */
int greb_member_lds_map(int* words8);

/* ---- the deal of member-year chunks (fused 96x48 member kernel) --------------------------------------
 * A launch of more members than workgroups cuts every member's steps into chunks and deals (member, chunk) items to the
 * workgroups from a ready queue on the device (greb_member.hip, greb_member_queue.h): a compute unit that is done early takes the next item
 * instead of idling until the slowest one has finished a whole member-year, and an ensemble that is no multiple of the
 * compute units does not pay a whole round for the remainder.  The results do not depend on it, bit for bit.
 * greb_engine_set_dealing: workgroups > 0: that many; 0: the device's compute units (the default); < 0: no dealing --
 * workgroup b integrates member b for the whole launch, as every launch of no more members than workgroups does anyway
 * unless force != 0 (tests: the queue with a handful of members).  schedule: GREB_CHUNKS_*.  Takes effect with the next
 * year launched.
 * greb_member_chunk_table (host only, no GPU call): the chunks `nsteps` steps of a launch are cut into, as the index one
 * past each chunk's last step (0-based steps; end[n - 1] == nsteps); at most `capacity` written; returns their number, at
 * most GREB_MAX_CHUNKS, or < 0.  greb_member_queue_capacity: the item words of the queue of such a launch of `members`
 * members = members x chunks, or < 0.
 * A workgroup that waits more than a second for an item gives the launch up; the call that waits for the year then
 * returns GREB_E_STATE. */
#define GREB_MAX_CHUNKS 10
#define GREB_CHUNKS_HALVING 0 /* 365 / 183 / 91 / 46 / 23 / 12 / 10 steps of a year's 730 */
#define GREB_CHUNKS_EQUAL   1 /* ten equal chunks */
#define GREB_CHUNKS_QUARTERS 2 /* 183 / 182 / 183 / 91 / 46 / 23 / 12 / 10: the halving schedule, its first half cut in two */
int greb_engine_set_dealing(greb_engine* e, int workgroups, int schedule, int force);
int greb_member_chunk_table(int schedule, int nsteps, int* end, int capacity);
long long greb_member_queue_capacity(int members, int schedule, int nsteps);

/* ---- forcing records (diagnostic) -------------------------------------------------------------------
 * The FAST fused 96x48 member kernel reads the boundary data of the point physics from one packed, read-only record per
 * boundary set, made on the device when the set's data is uploaded, in two parts: the static fields [row 0..47][field][96]
 * -- z_topo, glacier, z_ocean, wz_air -- and behind them the fields of every step [step 0..729][row 0..47][field][96] --
 * tclim, cldclim, mldclim, mldclim of the previous step (step 1 takes step 730), swetclim and the wind-speed term of the
 * latent heat flux (src/greb.f90:455-457) evaluated from uclim, vclim and z_topo.  greb_forcing_record_field_name gives the
 * ten in this order.  greb_engine_describe reports the bytes the records take.
 * Layout queries, host only (no GPU call): whether a field is static (1 / 0, -1 outside), the offset in floats of (row,
 * field, longitude) inside the field's part -- the static part or one step's slice (-1 outside) --, a field's offset in
 * bytes from the first field of its row and part (what the kernel folds into an instruction immediate, so at most 4 095),
 * the floats of the static part and of one step's slice, and the bytes of one record (the static part and 730 slices). */
#define GREB_FORCING_RECORD_FIELDS 10
int greb_forcing_record_field_static(int field);
long long greb_forcing_record_offset(int row, int field, int lon);
long long greb_forcing_record_field_bytes(int field);
long long greb_forcing_record_static_floats(void);
long long greb_forcing_record_step_floats(void);
long long greb_forcing_record_bytes(void);
const char* greb_forcing_record_field_name(int field); /* NULL outside 0 ... GREB_FORCING_RECORD_FIELDS - 1 */
/* Debug read-back of set `set`'s record (0 = the engine's own data): the static part, then the slice of step `step`
 * (1 ... 730), into out[greb_forcing_record_static_floats() + greb_forcing_record_step_floats()].  GREB_E_UNSUPPORTED on an
 * engine that keeps none (STRICT, any-grid). */
int greb_engine_get_forcing_record(greb_engine* e, int set, int step, float* out);

/* Diagnostic, host only (no GPU call): the variant of the step kernels -- a mask of GREB_V_* -- that a launch takes in the
 * flux-correction (flux_phase != 0) or scenario phase when the engine has experiment switches set (switches), the call is
 * greb_engine_run_budget (budget), a member is forced (forced) or a member is on a boundary set (on_sets).  This is the
 * selection the launches themselves go through.  Returns 0 and the mask in *variant; < 0, *variant untouched, for a
 * combination no launch carries (the flux-correction phase with a budget, or forced without a boundary set). */
#define GREB_V_FLUX 1u
#define GREB_V_SWITCHES 2u
#define GREB_V_BUDGET 4u
#define GREB_V_FORCING 8u
#define GREB_V_BOUNDARY 16u
int greb_step_variant(int flux_phase, int switches, int budget, int forced, int on_sets, unsigned* variant);
/* Every variant that is built: up to `capacity` masks into out; returns their number (call with capacity 0 to size). */
int greb_step_variants(unsigned* out, int capacity);

/* Point physics of one step for a batch of columns sets (tests): SWradiation :367-403,
 * LWradiation :407-434, hydro :438-469, deep_ocean :495-525, seaice :472-492 evaluated by the
 * same device functions the engine uses.  in  : Ts,Ta,To,q,cap_surf [5][ny][nx]
 *                                          out : 15 fields [15][ny][nx] in the order
 * albedo, sw, LW_surf, LWair_down, em, Q_sens, Q_lat, Q_lat_air, dq_eva, dq_rain, dT_ocean, dTo,
 * cap_surf_new(seaice(Ts)), 0, 0.   ityr is 1-based. */
int greb_engine_point_physics(greb_engine* e, int ityr, float co2, const float* in5, float* out15);

/* ---- ensemble statistics across the members resident on one GPU -------------------
 * The reference leaves ensemble statistics to its R scripts over per-`ens_id` files (src/greb.f90:153,
 * 1064-1068).  x_dev: device array [n_members][n] (e.g. the monthly means viewed per member); all output
 * pointers are device pointers of n elements (any of them may be NULL); nothing synchronises.
 *   moments  : fp64 sum and sum of squares, min, max over the members -- the partials a multi-GPU run
 *              all-reduces (greb_climate_model_amd/ensemble.py: mean, variance, range)
 *   quantiles: out_dev [n_probs][n], probabilities in [0,1] (host array, <= 16), linear interpolation of the
 *              order statistics (numpy's default); n_members <= 4096 */
int greb_ensemble_moments_dev(const float* x_dev, int n_members, size_t n, double* sum_dev, double* sumsq_dev,
                              float* min_dev, float* max_dev, void* stream);
int greb_ensemble_quantiles_dev(const float* x_dev, int n_members, size_t n, const float* probs, int n_probs,
                                float* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GREB_ENGINE_H */
