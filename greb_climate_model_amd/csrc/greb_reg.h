// greb_reg.h -- host interface of the regression output (greb_reg.hip): per (member, term, point) the least-squares line of
// a yearly quantity of the records on a yearly index that the run itself produces -- a regional mean of the same member.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "greb_yearwalk.h"

namespace greb {

constexpr int kRegThreads = 256;
constexpr int kRegMaxTerms = 16;
constexpr int kRegMaxIndices = 8;
constexpr int kRegMaxMembers = 65535; // grid.y of the update and finish kernels

// A term as the update kernel walks the plan's (greb_yearwalk.h: sorted by variable, then by selector).
struct RegTerm {
  int sel, rel; // selector, member minus control
  int index;    // the index it is regressed on
  int out;      // the term's index in the caller's order: where its state and products lie
};
using RegTable = YearTable<RegTerm, kRegMaxTerms>;
// (the kernels' scalar loads address the table in the kernel arguments)
static_assert(sizeof(RegTable) == 584 && offsetof(RegTable, vstart) == 324, "the layout greb_reg.hip was written to");

// the indices in the caller's order
struct RegIndexTable {
  struct Ix { int var, sel, rel, region; } ix[kRegMaxIndices];
};

// The state of the terms, each [n_members][n_terms][np]: year 0's quantity and the fp64 sums of the values centred on it.
struct RegState {
  float* y0;
  double *sy, *sgy, *syy; // syy null: the plan's products do not need it (no R2)
};
// ... and of the indices, each [n_members][n_indices]: year 0's value, this year's centred value G and the sums.
struct RegIndexState {
  float* g0;
  double *G, *sg, *sgg;
};

struct RegIndexArgs {
  const float* regions; // [n_members][12][n_vars][nr]: the year's regional means (launch_diag_year)
  const int* control;   // [n_members] on the device, or null: no control map
  RegIndexState ix;
  int n_members, n_vars, nr, n_indices;
  int k;                // the year, 0-based since the last finish; 0 stores the state
  float* index;         // member m's g at index + m * index_stride: [n_indices]; null: not delivered
  size_t index_stride;
  RegIndexTable t;
};
// one thread per (member, index)
hipError_t launch_reg_index(const RegIndexArgs& a, hipStream_t s);

struct RegUpdateArgs {
  const float* x;     // [n_members][12][n_vars][np], 16-byte aligned
  const int* control; // [n_members] on the device, or null
  RegState st;
  const double* G;    // [n_members][n_indices]: this year's centred index values (launch_reg_index, enqueued before)
  size_t np;          // ny * nx, a multiple of four
  int n_members, n_vars, n_terms, n_indices;
  int k;
  RegTable t;
};
// grid (blocks of 256 point quads, n_members, distinct variables)
hipError_t launch_reg_update(const RegUpdateArgs& a, hipStream_t s);

struct RegFinishArgs {
  RegState st;
  RegIndexState ix;
  size_t np;
  int n_members, n_terms, n_indices, n_years;
  int index_of[kRegMaxTerms];      // the index of each term, in the caller's order
  float *slope, *intercept, *r2;   // [n_members][n_terms][np], 16-byte aligned; null: skipped
};
// grid (blocks of 256 point quads, n_members, n_terms)
hipError_t launch_reg_finish(const RegFinishArgs& a, hipStream_t s);

} // namespace greb
