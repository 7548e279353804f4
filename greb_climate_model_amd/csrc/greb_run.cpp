// greb_run.cpp -- scenario runs: the one driver of their years, and the records sink (greb_engine_run, greb_engine_run_budget).
#include "greb_host.h"

using namespace greb;
using namespace greb::host;

hipError_t greb::host::unit_to_host(greb_engine* e, float* host, int n, int u, const float* dev, size_t rec, size_t rows) {
  return hipMemcpy2DAsync(host + (size_t)u * rec, (size_t)n * rec * sizeof(float), dev, rec * sizeof(float), rec * sizeof(float),
                          rows ? rows : (size_t)e->nm, hipMemcpyDeviceToHost, e->copy_stream);
}

// `years` scenario years of every member; `s` says what is made of each year and where it goes.  Host delivery: a unit
// leaves over PCIe on the copy stream while the following year integrates on the compute stream (two output slots, one
// event pair each).  A pinned destination makes the copies true DMA; a pageable one is staged by the runtime and still
// overlaps the kernels.
int greb::host::run_years(greb_engine* e, int years, const float* co2_ppm, float* yearly, const RunSink& s) {
  HIP_TRY(e, hipSetDevice(e->device));
  const size_t nm = (size_t)e->nm;
  if (int rc = ensure(e, &e->co2_dev, &e->co2_cap, nm * years)) return rc;
  HIP_TRY(e, hipMemcpyAsync(e->co2_dev, co2_ppm, nm * years * sizeof(float), hipMemcpyHostToDevice, e->stream));
  if (int rc = clear_yearly(e, years)) return rc;
  const bool delivers = (bool)s.deliver;
  if (delivers) if (int rc = ensure(e, &e->monthly_dev, &e->monthly_cap, 2 * year_records(e))) return rc; // the staging slots
  if (int rc = s.prepare()) { e->last_error = g_last_error; return rc; } // (a plan reports its failure without an engine)
  if (delivers && !e->copy_stream) HIP_TRY(e, hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  for (int i = 0; delivers && i < 2; ++i) {
    if (!e->ev_done[i]) HIP_TRY(e, hipEventCreateWithFlags(&e->ev_done[i], hipEventDisableTiming));
    if (!e->ev_free[i]) HIP_TRY(e, hipEventCreateWithFlags(&e->ev_free[i], hipEventDisableTiming));
  }
  int completed = 0, delivered = 0; // units
  YearCalls calls;
  calls.integrate = [&](int y, const YearOut& o) -> int { return run_year(e, scenario_args(e, years, y, o), e->nm); };
  // called where the SINK's first write to the slot is enqueued, so that nothing before it waits: a year whose records
  // are reduced on the device does not stall its integration on the copy of unit u - 2's small products
  calls.writing = [&](int u) -> int {
    if (u >= 2) HIP_TRY(e, hipStreamWaitEvent(e->stream, e->ev_free[u & 1], 0)); // the slot's unit u - 2 has left
    return 0;
  };
  calls.complete = [&](int u) -> int {
    HIP_TRY(e, hipEventRecord(e->ev_done[u & 1], e->stream));
    completed = u + 1;
    return 0;
  };
  auto deliver = [&](int u) -> int {
    HIP_TRY(e, hipStreamWaitEvent(e->copy_stream, e->ev_done[u & 1], 0));
    if (int rc = s.deliver(u, u & 1)) return rc;
    HIP_TRY(e, hipEventRecord(e->ev_free[u & 1], e->copy_stream));
    return 0;
  };
  // an error anywhere below must not return while copies into the CALLER's buffers are still in flight (the caller
  // may free them as soon as it sees the error): the body runs in a lambda and both streams are drained on failure
  const int rc_years = [&]() -> int {
    for (int y = 0; y < years; ++y) {
      // what EARLIER years completed leaves AFTER this year's kernels are enqueued, so that even a copy the runtime
      // performs synchronously (pageable destination) runs beside a kernel
      const int before = completed;
      if (int rc = s.year(calls, y)) return rc;
      for (; delivered < before; ++delivered) if (int rc = deliver(delivered)) return rc;
    }
    for (; delivered < completed; ++delivered) if (int rc = deliver(delivered)) return rc;
    if (delivers) HIP_TRY(e, hipStreamSynchronize(e->copy_stream));
    return 0;
  }();
  if (rc_years && delivers) {
    (void)hipStreamSynchronize(e->copy_stream);
    (void)hipStreamSynchronize(e->stream);
  }
  if (rc_years) return rc_years;
  if (int rc = finish_years(e)) return rc;
  e->it_scnr += (long long)years * kNT;
  if (s.finish) if (int rc = s.finish()) return rc;
  return yearly_to_host(e, years, yearly);
}

namespace {
// The records sink: greb_engine_run (budget == nullptr) and greb_engine_run_budget (budget != nullptr, monthly may be
// nullptr).  A unit is a year: its five records and, with a budget, its budget records.  With a budget the launches take
// the BUDGET instantiations (MemberArgs::bsum set); what they leave in state, clock, monthly and yearly is what the
// default ones leave.
int run_records(greb_engine* e, int years, const float* co2_ppm, float* monthly, float* budget, float* yearly,
                unsigned run_flags) {
  const size_t np = (size_t)e->np, nm = (size_t)e->nm;
  const size_t rec_year = 12 * 5 * np, bud_year = (size_t)12 * GREB_NBUDGET * np; // floats per member-year
  const bool dev_out = (run_flags & GREB_RUN_DEVICE_OUT) != 0;
  auto budget_slot = [&](int y) { return e->budget_dev + (size_t)(y & 1) * nm * bud_year; }; // as staging_slot
  RunSink s;
  s.prepare = [&]() -> int {
    if (!budget) return 0;
    if (!e->bsum) { // zero from here on: every December ends with the sums cleared
      HIP_TRY(e, dev_alloc(&e->bsum, nm * GREB_NBUDGET * np));
      HIP_TRY(e, hipMemsetAsync(e->bsum, 0, nm * GREB_NBUDGET * np * sizeof(float), e->stream));
    }
    ++e->budget_runs;
    if (!dev_out) return ensure(e, &e->budget_dev, &e->budget_cap, 2 * nm * bud_year);
    // (a budget-only run: the kernels write their five records regardless -- into one staging slot nobody reads)
    return monthly ? 0 : ensure(e, &e->monthly_dev, &e->monthly_cap, year_records(e));
  };
  if (dev_out) { // the kernels write the caller's device arrays, [member][years]
    s.year = [&](const YearCalls& run, int y) -> int {
      return run.integrate(y, monthly ? YearOut{monthly, years, y, budget, years, y} : YearOut{e->monthly_dev, 1, 0, budget, years, y});
    };
    return run_years(e, years, co2_ppm, yearly, s);
  }
  // the staging slot IS the output slot: the year's own kernels write it, so here -- and only here -- the year itself
  // waits until the slot's year y - 2 has left
  s.year = [&](const YearCalls& run, int y) -> int {
    if (int rc = run.writing(y)) return rc;
    if (int rc = run.integrate(y, {staging_slot(e, y), 1, 0, budget ? budget_slot(y) : nullptr, 1, 0})) return rc;
    return run.complete(y);
  };
  s.deliver = [&](int y, int sl) -> int {
    if (monthly) HIP_TRY(e, unit_to_host(e, monthly, years, y, staging_slot(e, sl), rec_year));
    if (budget) HIP_TRY(e, unit_to_host(e, budget, years, y, budget_slot(sl), bud_year));
    return 0;
  };
  return run_years(e, years, co2_ppm, yearly, s);
}
} // namespace

extern "C" {

int greb_engine_run(greb_engine* e, int years, const float* co2_ppm, float* monthly, float* yearly,
                    unsigned run_flags) {
  if (!e || years < 1 || !co2_ppm || !monthly) return fail(e, GREB_E_INVALID, "run: bad argument");
  return run_records(e, years, co2_ppm, monthly, nullptr, yearly, run_flags);
}

int greb_engine_run_budget(greb_engine* e, int years, const float* co2_ppm, float* monthly, float* budget, float* yearly,
                           unsigned run_flags) {
  if (!e || years < 1 || !co2_ppm) return fail(e, GREB_E_INVALID, "run_budget: bad argument (engine, years or co2_ppm)");
  if (!budget) return fail(e, GREB_E_INVALID, "run_budget: `budget` is NULL (greb_engine_run is the run without budget output)");
  return run_records(e, years, co2_ppm, monthly, budget, yearly, run_flags);
}

const char* greb_budget_name(int i) {
  static const char* const names[GREB_NBUDGET] = {"sw", "LW_surf", "LWair_down", "LW_abs", "Q_sens", "Q_lat", "Q_lat_air",
                                                  "dq_eva", "dq_rain", "dT_ocean", "dTo", "dTa_crcl", "dq_crcl"};
  return i >= 0 && i < GREB_NBUDGET ? names[i] : nullptr;
}

} // extern "C"
