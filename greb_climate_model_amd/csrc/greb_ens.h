// greb_ens.h -- host interface of the ensemble output (greb_ens.hip): the statistics across the members of a group of each
// element of x[n_members][n], of the values themselves or of each member's difference to its control member.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace greb {

constexpr int kEnsThreads = 256;
constexpr int kEnsRows = 16;            // member rows one lane of ens_moments_kernel keeps in flight (8 with a control map)
constexpr int kEnsMaxProbs = 16;
constexpr int kEnsMaxGroups = 64;
constexpr int kEnsMaxSorted = 4096;     // members of one group the quantile tile holds (8 points x 4096 members = 128 KB)
constexpr int kEnsTileFloats = 32768;   // 128 KB of the CU's 160 KB
constexpr int kEnsMaxPoints = 64;       // points of a quantile tile: one wavefront reads one member row of it

// The plan's member lists on the device: group g is member[offs[g] ... offs[g + 1]) in ascending member index, and
// control[k] is the control member of member[k] (null: no control map).
struct EnsLists {
  const int* offs;    // [n_groups + 1]
  const int* member;  // [offs[n_groups]]
  const int* control; // [offs[n_groups]] or null
};

struct EnsMomentArgs {
  const float* x; // [n_members][n], 16-byte aligned
  size_t n;
  EnsLists l;
  float *mean, *var, *mn, *mx; // [n_groups][n] each; null = skipped
};
// grid (ceil(ceil(n / 2) / 256), n_groups): every listed member's row is read once per group it is in
hipError_t launch_ens_moments(const EnsMomentArgs& a, int n_groups, hipStream_t s);

struct EnsProbs { int n; float p[kEnsMaxProbs]; };
// one group: its n_g <= kEnsMaxSorted members member[0 ... n_g) (device), control[] beside them or null; out [n_probs][n]
hipError_t launch_ens_quantiles(const float* x, size_t n, const int* member, const int* control, int n_g, const EnsProbs& pr,
                                float* out, hipStream_t s);

} // namespace greb
