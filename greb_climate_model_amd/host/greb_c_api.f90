! greb_c_api.f90 -- iso_c_binding interface of the MI355X GREB engine (include/greb_engine.h), shared by the hosts.
module greb_c_api
  use iso_c_binding
  implicit none

  type, bind(C) :: greb_params
     real(c_float) :: pi, sig, rho_ocean, rho_land, rho_air, cp_ocean, cp_land, cp_air, eps
     real(c_float) :: d_ocean, d_land, d_air, ct_sens, da_ice, a_no_ice, a_cloud
     real(c_float) :: Tl_ice1, Tl_ice2, To_ice1, To_ice2
     real(c_float) :: co_turb, kappa, ce, cq_latent, cq_rain, z_air, z_vapor, r_qviwv
     real(c_float) :: p_emi(10)
     real(c_float) :: co2_flux
     integer(c_int32_t) :: ipx, ipy, year0, dt, dt_crcl
  end type greb_params

  ! per-member physics of a perturbed-physics ensemble; NaN = keep the engine-wide value
  type, bind(C) :: greb_member_overrides
     real(c_float) :: da_ice, a_no_ice, a_cloud, kappa
  end type greb_member_overrides

  ! a member as a full namelist plus its GREB_X_* switches (greb_engine_create_members); pi, z_air, z_vapor, dt, dt_crcl,
  ! ipx, ipy, year0 must equal the engine-wide greb_params
  type, bind(C) :: greb_member_config
     type(greb_params) :: p
     integer(c_int32_t) :: switches
  end type greb_member_config

  type, bind(C) :: greb_fields
     type(c_ptr) :: z_topo, glacier, sw_solar, tclim, qclim, uclim, vclim, mldclim, cldclim, swetclim
  end type greb_fields

  ! an event of the crossing output (greb_cross_create): variable (0-based), selector (0 ... 11 a month, 12 ... 16 DJF MAM JJA
  ! SON ANN), rel (1: member minus its control), dir (+1: q >= thr hits, -1: q <= thr), threshold
  type, bind(C) :: greb_cross_event
     integer(c_int32_t) :: var, sel, rel, dir
     real(c_float) :: thr
  end type greb_cross_event

  ! an index and a term of the regression output (greb_reg_create): variable (0-based), selector and rel as in
  ! greb_cross_event; an index is the mean over `region` (0: the globe), a term names the index it is regressed on (0-based)
  type, bind(C) :: greb_reg_index
     integer(c_int32_t) :: var, sel, rel, region
  end type greb_reg_index
  type, bind(C) :: greb_reg_term
     integer(c_int32_t) :: var, sel, rel, index
  end type greb_reg_term
  ! an instruction of a derive program (greb_derive_create): op (GREB_DV_* of greb_engine.h), arg (the 0-based index of STATE,
  ! TERM, FIELD, TEE, GET) and value (of CONST)
  type, bind(C) :: greb_derive_ins
     integer(c_int32_t) :: op, arg
     real(c_float) :: value
  end type greb_derive_ins

  interface
     subroutine greb_params_default(p) bind(C, name="greb_params_default")
       import :: greb_params
       type(greb_params), intent(out) :: p
     end subroutine
     integer(c_int) function greb_engine_create(p, nx, ny, f, n_members, overrides, device, flags, eng) &
          bind(C, name="greb_engine_create")
       import :: greb_params, greb_fields, c_int, c_ptr
       type(greb_params), intent(in) :: p
       integer(c_int), value :: nx, ny, n_members, device, flags
       type(greb_fields), intent(in) :: f
       type(c_ptr), value :: overrides
       type(c_ptr), intent(out) :: eng
     end function
     integer(c_int) function greb_engine_create_members(p, nx, ny, f, n_members, members, device, flags, eng) &
          bind(C, name="greb_engine_create_members")
       import :: greb_params, greb_fields, greb_member_config, c_int, c_ptr
       type(greb_params), intent(in) :: p
       integer(c_int), value :: nx, ny, n_members, device, flags
       type(greb_fields), intent(in) :: f
       type(greb_member_config), intent(in) :: members(*)
       type(c_ptr), intent(out) :: eng
     end function
     integer(c_int) function greb_engine_flux_correction(eng, years, yearly) bind(C, name="greb_engine_flux_correction")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng
       integer(c_int), value :: years
       real(c_float), intent(out) :: yearly(*)
     end function
     integer(c_int) function greb_engine_run(eng, years, co2_ppm, monthly, yearly, run_flags) bind(C, name="greb_engine_run")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng
       integer(c_int), value :: years, run_flags
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_float), intent(out) :: monthly(*), yearly(*)
     end function
     ! reduced output (greb_diag.hip): a plan = grid + region weights [n_regions][ny][nx] in [0,1] (c_null_ptr with 0 regions)
     integer(c_int) function greb_diag_create(nx, ny, region_w, n_regions, plan) bind(C, name="greb_diag_create")
       import :: c_int, c_ptr
       integer(c_int), value :: nx, ny, n_regions
       type(c_ptr), value :: region_w
       type(c_ptr), intent(out) :: plan
     end function
     integer(c_int) function greb_diag_destroy(plan) bind(C, name="greb_diag_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan
     end function
     ! device pointers (c_ptr); a product whose pointer is c_null_ptr is skipped; launches on `stream`, no synchronisation
     integer(c_int) function greb_diag_reduce_dev(plan, device, monthly_year_dev, n_members, regions_dev, zonal_dev, &
          annual_dev, stream) bind(C, name="greb_diag_reduce_dev")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan, monthly_year_dev, regions_dev, zonal_dev, annual_dev, stream
       integer(c_int), value :: device, n_members
     end function
     ! greb_engine_run that delivers only the products selected by `what` (1 regions, 2 zonal, 4 annual):
     ! regions(1+n_regions,5,12,years,n_members), zonal(ny,5,12,years,n_members), annual(nx,ny,5,years,n_members)
     integer(c_int) function greb_engine_run_diag(eng, years, co2_ppm, plan, what, regions, zonal, annual, yearly) &
          bind(C, name="greb_engine_run_diag")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng, plan
       integer(c_int), value :: years, what
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_float), intent(out) :: regions(*), zonal(*), annual(*), yearly(*)
     end function
     ! climatology output (greb_clim.hip): a plan = grid, member count, control(n_members) with each member's control member
     ! (0-based, -1 = none; c_null_ptr: no control map) and the products `what` (1 mean, 2 seasons, 4 trend, 8 response)
     integer(c_int) function greb_clim_create(nx, ny, n_members, control, what, plan) bind(C, name="greb_clim_create")
       import :: c_int, c_ptr
       integer(c_int), value :: nx, ny, n_members, what
       type(c_ptr), value :: control
       type(c_ptr), intent(out) :: plan
     end function
     integer(c_int) function greb_clim_destroy(plan) bind(C, name="greb_clim_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan
     end function
     ! device pointers (c_ptr); year k (0-based) of the current period into the sums; launches on `stream`, no synchronisation
     integer(c_int) function greb_clim_add_year_dev(plan, device, monthly_year_dev, k, stream) &
          bind(C, name="greb_clim_add_year_dev")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan, monthly_year_dev, stream
       integer(c_int), value :: device, k
     end function
     ! the products of the n_years years added since the last finish; a product the plan does not select may be c_null_ptr
     integer(c_int) function greb_clim_finish_dev(plan, device, n_years, mean_dev, seasons_dev, trend_dev, mean_resp_dev, &
          seasons_resp_dev, stream) bind(C, name="greb_clim_finish_dev")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan, mean_dev, seasons_dev, trend_dev, mean_resp_dev, seasons_resp_dev, stream
       integer(c_int), value :: device, n_years
     end function
     ! greb_engine_run that delivers only the plan's products of n_periods averaging periods (0-based first_year, n_years):
     ! mean, trend, mean_resp (nx,ny,5,12,n_periods,n_members); seasons, seasons_resp (nx,ny,5,5,n_periods,n_members);
     ! a product the plan does not select may be c_null_ptr
     integer(c_int) function greb_engine_run_clim(eng, years, co2_ppm, plan, n_periods, first_year, n_years, mean, seasons, &
          trend, mean_resp, seasons_resp, yearly) bind(C, name="greb_engine_run_clim")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng, plan, mean, seasons, trend, mean_resp, seasons_resp
       integer(c_int), value :: years, n_periods
       real(c_float), intent(in) :: co2_ppm(*)
       integer(c_int), intent(in) :: first_year(*), n_years(*)
       real(c_float), intent(out) :: yearly(*)
     end function
     ! ensemble output (greb_ens.hip): a plan = grid, member count, group(n_members) (0-based, -1 = in no group),
     ! control(n_members) (0-based, -1 = none; c_null_ptr: no control map), probs(n_probs) and the products `what`
     ! (1 mean, 2 variance, 4 min and max, 8 quantiles)
     integer(c_int) function greb_ens_create(nx, ny, n_members, group, n_groups, control, probs, n_probs, what, plan) &
          bind(C, name="greb_ens_create")
       import :: c_int, c_ptr
       integer(c_int), value :: nx, ny, n_members, n_groups, n_probs, what
       integer(c_int), intent(in) :: group(*)
       type(c_ptr), value :: control, probs
       type(c_ptr), intent(out) :: plan
     end function
     integer(c_int) function greb_ens_destroy(plan) bind(C, name="greb_ens_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan
     end function
     ! device pointers (c_ptr): x_dev(n,n_members) -> the statistics per group; a product the plan does not select may be
     ! c_null_ptr; launches on `stream`, no synchronisation
     integer(c_int) function greb_ens_reduce_dev(plan, device, x_dev, n, mean_dev, var_dev, min_dev, max_dev, quant_dev, &
          stream) bind(C, name="greb_ens_reduce_dev")
       import :: c_int, c_ptr, c_size_t
       type(c_ptr), value :: plan, x_dev, mean_dev, var_dev, min_dev, max_dev, quant_dev, stream
       integer(c_int), value :: device
       integer(c_size_t), value :: n
     end function
     ! greb_engine_run that delivers only the plan's statistics of every year's monthly records:
     ! mean, var, min, max (nx,ny,5,12,years,n_groups); quant (nx,ny,5,12,n_probs,years,n_groups);
     ! a product the plan does not select may be c_null_ptr
     integer(c_int) function greb_engine_run_ens(eng, years, co2_ppm, plan, mean, var, vmin, vmax, quant, yearly) &
          bind(C, name="greb_engine_run_ens")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng, plan, mean, var, vmin, vmax, quant
       integer(c_int), value :: years
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_float), intent(out) :: yearly(*)
     end function
     ! linear-model output (greb_lin.hip): a plan = grid, member count, weight(n_members,n_terms) (double), use(n_members)
     ! (nonzero = the member enters the sums; c_null_ptr: all do), control(n_members) (0-based, -1 = none; c_null_ptr: no
     ! control map), design(n_terms,n_members) (double; c_null_ptr: none) and the products `what` (1 coefficients, 2
     ! residual sum of squares, which needs the design)
     integer(c_int) function greb_lin_create(nx, ny, n_members, weight, n_terms, use, control, design, what, plan) &
          bind(C, name="greb_lin_create")
       import :: c_int, c_ptr, c_double
       integer(c_int), value :: nx, ny, n_members, n_terms, what
       real(c_double), intent(in) :: weight(*)
       type(c_ptr), value :: use, control, design
       type(c_ptr), intent(out) :: plan
     end function
     integer(c_int) function greb_lin_destroy(plan) bind(C, name="greb_lin_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan
     end function
     ! device pointers (c_ptr): x_dev(n,n_members) -> coef_dev(n,n_terms), rss_dev(n); a product the plan does not select
     ! may be c_null_ptr; launches on `stream`, no synchronisation
     integer(c_int) function greb_lin_reduce_dev(plan, device, x_dev, n, coef_dev, rss_dev, stream) &
          bind(C, name="greb_lin_reduce_dev")
       import :: c_int, c_ptr, c_size_t
       type(c_ptr), value :: plan, x_dev, coef_dev, rss_dev, stream
       integer(c_int), value :: device
       integer(c_size_t), value :: n
     end function
     ! greb_engine_run that delivers only the plan's linear model of every year's monthly records:
     ! coef (nx,ny,5,12,years,n_terms); rss (nx,ny,5,12,years); a product the plan does not select may be c_null_ptr
     integer(c_int) function greb_engine_run_lin(eng, years, co2_ppm, plan, coef, rss, yearly) &
          bind(C, name="greb_engine_run_lin")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng, plan, coef, rss
       integer(c_int), value :: years
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_float), intent(out) :: yearly(*)
     end function
     ! covariance output (greb_gram.hip): a plan = grid, member count, n_records (12 * 5 for a model year), block(n_records)
     ! (0-based, -1 = the record enters no matrix), n_blocks, use(n_members) (c_null_ptr: all), control(n_members) (0-based;
     ! c_null_ptr: no control map) and scale(nx,ny) (float; c_null_ptr: none)
     integer(c_int) function greb_gram_create(nx, ny, n_members, n_records, block, n_blocks, use, control, scale, plan) &
          bind(C, name="greb_gram_create")
       import :: c_int, c_int32_t, c_ptr
       integer(c_int), value :: nx, ny, n_members, n_records, n_blocks
       integer(c_int32_t), intent(in) :: block(*)
       type(c_ptr), value :: use, control, scale
       type(c_ptr), intent(out) :: plan
     end function
     integer(c_int) function greb_gram_destroy(plan) bind(C, name="greb_gram_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan
     end function
     ! device pointers (c_ptr): x_dev(len,n_records,n_members) -> G_dev(U,U,n_blocks) in double, U = the used members;
     ! launches on `stream`, no synchronisation
     integer(c_int) function greb_gram_reduce_dev(plan, device, x_dev, len, G_dev, stream) &
          bind(C, name="greb_gram_reduce_dev")
       import :: c_int, c_ptr, c_size_t
       type(c_ptr), value :: plan, x_dev, G_dev, stream
       integer(c_int), value :: device
       integer(c_size_t), value :: len
     end function
     ! greb_engine_run that delivers only the plan's Gram matrices of every year's monthly records: G(U,U,n_blocks,years)
     integer(c_int) function greb_engine_run_gram(eng, years, co2_ppm, plan, G, yearly) &
          bind(C, name="greb_engine_run_gram")
       import :: c_int, c_ptr, c_float, c_double
       type(c_ptr), value :: eng, plan
       integer(c_int), value :: years
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_double), intent(out) :: G(*)
       real(c_float), intent(out) :: yearly(*)
     end function
     ! ... of the year's budget records: the 13 flux terms (combo = c_null_ptr) or the n_out rows of combo(13,n_out)
     integer(c_int) function greb_engine_run_budget_gram(eng, years, co2_ppm, combo, n_out, plan, G, yearly) &
          bind(C, name="greb_engine_run_budget_gram")
       import :: c_int, c_ptr, c_float, c_double
       type(c_ptr), value :: eng, combo, plan
       integer(c_int), value :: years, n_out
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_double), intent(out) :: G(*)
       real(c_float), intent(out) :: yearly(*)
     end function
     ! crossing output (greb_cross.hip): a plan = grid, member count, variables per month, events(n_events), control(n_members)
     ! (0-based; c_null_ptr: no control map), group(n_members) (0-based, -1 = in none; c_null_ptr: no group map), n_groups and
     ! the products `what` (GREB_T_* of greb_engine.h)
     integer(c_int) function greb_cross_create(nx, ny, n_members, n_vars, events, n_events, control, group, n_groups, what, plan) &
          bind(C, name="greb_cross_create")
       import :: c_int, c_ptr, greb_cross_event
       integer(c_int), value :: nx, ny, n_members, n_vars, n_events, n_groups, what
       type(greb_cross_event), intent(in) :: events(*)
       type(c_ptr), value :: control, group
       type(c_ptr), intent(out) :: plan
     end function
     integer(c_int) function greb_cross_destroy(plan) bind(C, name="greb_cross_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan
     end function
     ! device pointers (c_ptr): year k (0-based since the last finish) x_dev(nx,ny,n_vars,12,n_members) into the state, and
     ! with GREB_T_FRACTION that year's fraction_dev(nx,ny,n_events,n_groups); launches on `stream`, no synchronisation
     integer(c_int) function greb_cross_add_year_dev(plan, device, x_dev, k, fraction_dev, stream) &
          bind(C, name="greb_cross_add_year_dev")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan, x_dev, fraction_dev, stream
       integer(c_int), value :: device, k
     end function
     ! the maps of the n_years years added, each (nx,ny,n_events,n_members): int32 but peak_dev (float); c_null_ptr where
     ! the plan does not select a product
     integer(c_int) function greb_cross_finish_dev(plan, device, n_years, first_dev, last_dev, stay_dev, count_dev, peak_dev, &
          peak_year_dev, stream) bind(C, name="greb_cross_finish_dev")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan, first_dev, last_dev, stay_dev, count_dev, peak_dev, peak_year_dev, stream
       integer(c_int), value :: device, n_years
     end function
     ! greb_engine_run that delivers only the plan's crossing products: the maps (nx,ny,n_events,n_members) -- first, last,
     ! stay, count, peak_year int32, peak float -- and fraction(nx,ny,n_events,n_groups,years); host arrays passed as
     ! c_loc(...), c_null_ptr where the plan does not select a product; years are 0-based, -1 = never
     integer(c_int) function greb_engine_run_cross(eng, years, co2_ppm, plan, first, last, stay, count, peak, peak_year, &
          fraction, yearly) bind(C, name="greb_engine_run_cross")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng, plan, first, last, stay, count, peak, peak_year, fraction
       integer(c_int), value :: years
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_float), intent(out) :: yearly(*)
     end function
     ! ... of the year's budget records: the 13 flux terms (combo = c_null_ptr) or the n_out rows of combo(13,n_out)
     integer(c_int) function greb_engine_run_budget_cross(eng, years, co2_ppm, combo, n_out, plan, first, last, stay, count, &
          peak, peak_year, fraction, yearly) bind(C, name="greb_engine_run_budget_cross")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng, combo, plan, first, last, stay, count, peak, peak_year, fraction
       integer(c_int), value :: years, n_out
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_float), intent(out) :: yearly(*)
     end function
     ! regression output (greb_reg.hip): a plan = grid, member count, variables per month, region_w(nx,ny,n_regions) as
     ! greb_diag_create takes it (c_null_ptr with n_regions = 0), control(n_members) (0-based; c_null_ptr: no control map),
     ! indices(n_indices), terms(n_terms) and the products `what` (GREB_R_* of greb_engine.h)
     integer(c_int) function greb_reg_create(nx, ny, n_members, n_vars, region_w, n_regions, control, indices, n_indices, terms, &
          n_terms, what, plan) bind(C, name="greb_reg_create")
       import :: c_int, c_ptr, greb_reg_index, greb_reg_term
       integer(c_int), value :: nx, ny, n_members, n_vars, n_regions, n_indices, n_terms, what
       type(c_ptr), value :: region_w, control
       type(greb_reg_index), intent(in) :: indices(*)
       type(greb_reg_term), intent(in) :: terms(*)
       type(c_ptr), intent(out) :: plan
     end function
     integer(c_int) function greb_reg_destroy(plan) bind(C, name="greb_reg_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan
     end function
     ! device pointers (c_ptr): year k (0-based since the last finish) x_dev(nx,ny,n_vars,12,n_members) into the state, and
     ! with GREB_R_INDEX that year's index_dev(n_indices,n_members); launches on `stream`, no synchronisation
     integer(c_int) function greb_reg_add_year_dev(plan, device, x_dev, k, index_dev, stream) bind(C, name="greb_reg_add_year_dev")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan, x_dev, index_dev, stream
       integer(c_int), value :: device, k
     end function
     ! the maps of the n_years years added, each float (nx,ny,n_terms,n_members); c_null_ptr where the plan does not select
     ! a product
     integer(c_int) function greb_reg_finish_dev(plan, device, n_years, slope_dev, intercept_dev, r2_dev, stream) &
          bind(C, name="greb_reg_finish_dev")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan, slope_dev, intercept_dev, r2_dev, stream
       integer(c_int), value :: device, n_years
     end function
     ! greb_engine_run that delivers only the plan's regression products: the float maps (nx,ny,n_terms,n_members) and
     ! index(n_indices,years,n_members); host arrays passed as c_loc(...), c_null_ptr where the plan does not select a product
     integer(c_int) function greb_engine_run_reg(eng, years, co2_ppm, plan, slope, intercept, r2, index, yearly) &
          bind(C, name="greb_engine_run_reg")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng, plan, slope, intercept, r2, index
       integer(c_int), value :: years
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_float), intent(out) :: yearly(*)
     end function
     ! ... of the year's budget records: the 13 flux terms (combo = c_null_ptr) or the n_out rows of combo(13,n_out)
     integer(c_int) function greb_engine_run_budget_reg(eng, years, co2_ppm, combo, n_out, plan, slope, intercept, r2, index, &
          yearly) bind(C, name="greb_engine_run_budget_reg")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng, combo, plan, slope, intercept, r2, index
       integer(c_int), value :: years, n_out
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_float), intent(out) :: yearly(*)
     end function
     ! derived records (greb_derive.hip): a plan = grid, the outputs' postfix programs one after the other in ins(*) with their
     ! lengths n_ins(n_out), and fields(nx,ny,n_fields) shared by all members (c_null_ptr with n_fields = 0)
     integer(c_int) function greb_derive_create(nx, ny, ins, n_ins, n_out, fields, n_fields, plan) &
          bind(C, name="greb_derive_create")
       import :: c_int, c_int32_t, c_ptr, greb_derive_ins
       integer(c_int), value :: nx, ny, n_out, n_fields
       type(greb_derive_ins), intent(in) :: ins(*)
       integer(c_int32_t), intent(in) :: n_ins(*)
       type(c_ptr), value :: fields
       type(c_ptr), intent(out) :: plan
     end function
     integer(c_int) function greb_derive_destroy(plan) bind(C, name="greb_derive_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan
     end function
     ! 1: some output names a budget term
     integer(c_int) function greb_derive_uses_budget(plan) bind(C, name="greb_derive_uses_budget")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan
     end function
     ! device pointers (c_ptr): state_year_dev(nx,ny,5,12,n_members), budget_year_dev(nx,ny,13,12,n_members) (c_null_ptr where no
     ! output names a term) -> out_dev(nx,ny,n_out,12,n_members); launches on `stream`, no synchronisation
     integer(c_int) function greb_derive_apply_dev(plan, device, state_year_dev, budget_year_dev, n_members, out_dev, stream) &
          bind(C, name="greb_derive_apply_dev")
       import :: c_int, c_ptr
       type(c_ptr), value :: plan, state_year_dev, budget_year_dev, out_dev, stream
       integer(c_int), value :: device, n_members
     end function
     ! the seven reduced runs over the derived records of `derive`: the arguments of the budget run of the same name with the
     ! derive plan in place of combo and n_out; the output arrays as c_ptr (c_loc; c_null_ptr: a product not selected)
     integer(c_int) function greb_engine_run_derived_diag(eng, years, co2_ppm, derive, plan, what, regions, zonal, annual, yearly) &
          bind(C, name="greb_engine_run_derived_diag")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng, derive, plan, regions, zonal, annual
       integer(c_int), value :: years, what
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_float), intent(out) :: yearly(*)
     end function
     integer(c_int) function greb_engine_run_derived_clim(eng, years, co2_ppm, derive, plan, n_periods, first_year, n_years, &
          mean, seasons, trend, mean_resp, seasons_resp, yearly) &
          bind(C, name="greb_engine_run_derived_clim")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng, derive, plan, first_year, n_years, mean, seasons, trend, mean_resp, seasons_resp
       integer(c_int), value :: years, n_periods
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_float), intent(out) :: yearly(*)
     end function
     integer(c_int) function greb_engine_run_derived_ens(eng, years, co2_ppm, derive, plan, mean, var, vmin, vmax, quant, yearly) &
          bind(C, name="greb_engine_run_derived_ens")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng, derive, plan, mean, var, vmin, vmax, quant
       integer(c_int), value :: years
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_float), intent(out) :: yearly(*)
     end function
     integer(c_int) function greb_engine_run_derived_lin(eng, years, co2_ppm, derive, plan, coef, rss, yearly) &
          bind(C, name="greb_engine_run_derived_lin")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng, derive, plan, coef, rss
       integer(c_int), value :: years
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_float), intent(out) :: yearly(*)
     end function
     integer(c_int) function greb_engine_run_derived_gram(eng, years, co2_ppm, derive, plan, G, yearly) &
          bind(C, name="greb_engine_run_derived_gram")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng, derive, plan, G
       integer(c_int), value :: years
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_float), intent(out) :: yearly(*)
     end function
     integer(c_int) function greb_engine_run_derived_cross(eng, years, co2_ppm, derive, plan, first, last, stay, count, peak, &
          peak_year, fraction, yearly) &
          bind(C, name="greb_engine_run_derived_cross")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng, derive, plan, first, last, stay, count, peak, peak_year, fraction
       integer(c_int), value :: years
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_float), intent(out) :: yearly(*)
     end function
     integer(c_int) function greb_engine_run_derived_reg(eng, years, co2_ppm, derive, plan, slope, intercept, r2, index, yearly) &
          bind(C, name="greb_engine_run_derived_reg")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng, derive, plan, slope, intercept, r2, index
       integer(c_int), value :: years
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_float), intent(out) :: yearly(*)
     end function
     ! greb_engine_run that also delivers the monthly means of the 13 flux terms of the update (GREB_B_* of greb_engine.h):
     ! budget(nx,ny,13,12,years,n_members); monthly as in greb_engine_run, or c_null_ptr for a budget-only run
     integer(c_int) function greb_engine_run_budget(eng, years, co2_ppm, monthly, budget, yearly, run_flags) &
          bind(C, name="greb_engine_run_budget")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng, monthly
       integer(c_int), value :: years, run_flags
       real(c_float), intent(in) :: co2_ppm(*)
       real(c_float), intent(out) :: budget(*), yearly(*)
     end function
     integer(c_int) function greb_engine_get_corrections(eng, member, corr, state5) &
          bind(C, name="greb_engine_get_corrections")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng
       integer(c_int), value :: member
       real(c_float), intent(out) :: corr(*), state5(*)
     end function
     integer(c_int) function greb_engine_set_corrections(eng, member, corr, state5) &
          bind(C, name="greb_engine_set_corrections")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng
       integer(c_int), value :: member
       real(c_float), intent(in) :: corr(*), state5(*)
     end function
     integer(c_int) function greb_log_exp_switches(log_exp) bind(C, name="greb_log_exp_switches")
       import :: c_int
       integer(c_int), value :: log_exp
     end function
     integer(c_int) function greb_engine_set_experiment(eng, switches) bind(C, name="greb_engine_set_experiment")
       import :: c_int, c_ptr
       type(c_ptr), value :: eng
       integer(c_int), value :: switches
     end function
     integer(c_int) function greb_engine_set_member_experiments(eng, switches) &
          bind(C, name="greb_engine_set_member_experiments")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr), value :: eng
       integer(c_int32_t), intent(in) :: switches(*)
     end function
     integer(c_int) function greb_engine_get_state(eng, member, state5) bind(C, name="greb_engine_get_state")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng
       integer(c_int), value :: member
       real(c_float), intent(out) :: state5(*)
     end function
     integer(c_int) function greb_engine_set_state(eng, member, state5) bind(C, name="greb_engine_set_state")
       import :: c_int, c_ptr, c_float
       type(c_ptr), value :: eng
       integer(c_int), value :: member
       real(c_float), intent(in) :: state5(*)
     end function
     integer(c_int) function greb_engine_destroy(eng) bind(C, name="greb_engine_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: eng
     end function
     function greb_engine_last_error(eng) bind(C, name="greb_engine_last_error") result(msg)
       import :: c_ptr
       type(c_ptr), value :: eng
       type(c_ptr) :: msg
     end function
  end interface
contains
  subroutine engine_check(rc, eng, what)
    integer(c_int), intent(in) :: rc
    type(c_ptr), intent(in) :: eng
    character(*), intent(in) :: what
    character(kind=c_char), pointer :: cmsg(:)
    type(c_ptr) :: p
    integer :: i
    if (rc == 0) return
    write(*, '(a,a,a,i0)') 'greb_host: ', what, ' failed, code ', rc
    p = greb_engine_last_error(eng)
    if (c_associated(p)) then
       call c_f_pointer(p, cmsg, [512])
       do i = 1, 512
          if (cmsg(i) == c_null_char) exit
          write(*, '(a)', advance='no') cmsg(i)
       end do
       write(*, *)
    end if
    error stop 1
  end subroutine
end module greb_c_api
