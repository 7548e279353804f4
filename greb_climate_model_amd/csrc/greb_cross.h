// greb_cross.h -- host interface of the crossing output (greb_cross.hip): per (member, event, point) the years in which a
// thresholded quantity of a model year's records hits, and per year the share of a group's members that hit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "greb_yearwalk.h"

namespace greb {

constexpr int kCrossThreads = 256;
constexpr int kCrossMaxEvents = 16;

// An event as the update kernel walks the plan's (greb_yearwalk.h: sorted by variable, then by selector).
struct CrossEv {
  int sel, rel, dir; // selector, member minus control, +1: q >= thr hits, -1: q <= thr
  float thr;
  int out;           // the event's index in the caller's order: where its state and products lie
};
using CrossTable = YearTable<CrossEv, kCrossMaxEvents>;
// (the kernels' scalar loads address the table in the kernel arguments)
static_assert(sizeof(CrossTable) == 648 && offsetof(CrossTable, vstart) == 388, "the layout greb_cross.hip was written to");

// The state words, each [n_members][n_events][np] (null: the plan's products do not need it), and the hit bytes of the
// current year, likewise (null without FRACTION).
struct CrossState {
  int32_t *first, *last, *last_miss, *count, *peak_year;
  float* peak;
  unsigned char* hit;
};

struct CrossUpdateArgs {
  const float* x;     // [n_members][12][n_vars][np], 16-byte aligned
  const int* control; // [n_members] on the device, or null: no control map
  CrossState st;
  size_t np;          // ny * nx, a multiple of four
  int n_members, n_vars, n_events;
  int k;              // the year, 0-based since the last finish; 0 stores the state
  CrossTable t;
};
// grid (blocks of 256 point quads, n_members, distinct variables)
hipError_t launch_cross_update(const CrossUpdateArgs& a, hipStream_t s);

// fraction[n_groups][n_events][np] of the hit bytes: group g is member[offs[g]] ... member[offs[g + 1] - 1], ascending.
// grid (blocks of 256 point quads, n_groups, n_events)
hipError_t launch_cross_fraction(const unsigned char* hit, const int* offs, const int* member, int n_groups, int n_members,
                                 int n_events, size_t np, float* fraction, hipStream_t s);

struct CrossFinishArgs {
  CrossState st;
  size_t n; // n_members * n_events * np
  int n_years;
  int32_t *first, *last, *stay, *count, *peak_year; // [n_members][n_events][np], 16-byte aligned; null: skipped
  float* peak;
};
hipError_t launch_cross_finish(const CrossFinishArgs& a, hipStream_t s);

} // namespace greb
