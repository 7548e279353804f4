// greb_diag.hip -- one model year of monthly records reduced on the device (include/greb_engine.h: greb_diag_*).
//
// The reference leaves every diagnostic to R scripts over the output file (R/analyse_output_fields.R: a global-mean
// series from the full records).  Here a year of an ensemble sits in HBM as [member][12][n_vars][ny][nx] -- one staging
// slot of greb_engine_run has the five state records, a budget run up to sixteen -- and what an analysis wants of it is small: area-weighted regional means, zonal means and
// the annual-mean map.  All three come out of ONE pass over the slot:
//
//   diag_year_kernel   a workgroup owns (member, variable, band of rows) across the twelve months.  A lane owns one
//                      group of four longitudes: it loads the twelve records' values with 16-byte loads (twelve loads
//                      in flight, each record read once) and keeps them in registers, so
//                        annual : the day-weighted sum of its twelve values, per point, no communication;
//                        zonal  : its four-point sums go to LDS, one thread per (month, row) adds a row's groups
//                                 west to east;
//                        regions: per region the lane's weights (fp64, made on the host) are loaded ONCE for the
//                                 twelve months, the lane sums reduced across the wavefront by shuffles and the four
//                                 wavefronts' sums left in LDS; the band's partial sums go to a scratch array.
//   diag_regions_kernel one thread per (member, month, variable, region) adds the bands' partial sums south to north,
//                      scales by the reciprocal weight sum and rounds to fp32.
//
// Everything accumulates in fp64 and is rounded to fp32 once.  The order of every sum is fixed by the grid alone (no
// atomics; a member's workgroups do not know how many members the batch has), so results are deterministic and a
// member's numbers do not depend on the batch it is in.
#include "greb_diag.h"

namespace greb {
namespace {

constexpr int kWaves = kDiagThreads / 64;
constexpr int kMaxNr = kDiagMaxRegions + 1;

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v; // every lane holds the sum, added in the same order
}

__global__ __launch_bounds__(kDiagThreads) void diag_year_kernel(DiagArgs a, int band_rows, int nbands) {
  __shared__ double zs[kDiagMonths][kDiagThreads];  // a lane's four-point sums of the twelve months
  __shared__ double red[kWaves][kDiagMonths][kMaxNr]; // the wavefronts' region sums
  const double jday[kDiagMonths] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31}; // src/greb.f90:42
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int band = blockIdx.x, var = blockIdx.y, member = blockIdx.z;
  const int nx = a.nx, gpr = nx >> 2; // groups of four longitudes per row
  const size_t np = (size_t)nx * a.ny;
  const int j0 = band * band_rows;
  const int rows = min(band_rows, a.ny - j0);
  const int band_groups = rows * gpr;
  const bool do_regions = a.regions != nullptr;
  const int nv = a.nv; // variables per month
  const float* src = a.monthly + ((size_t)member * kDiagMonths * nv + var) * np; // month m: + m * nv * np

  if (do_regions) {
    for (int t = tid; t < kWaves * kDiagMonths * kMaxNr; t += kDiagThreads) (&red[0][0][0])[t] = 0.0;
    __syncthreads();
  }
  double zcarry = 0.0; // a row wider than one chunk (nx > 1024: one row per band): its sum so far, thread = month
  for (int g0 = 0; g0 < band_groups; g0 += kDiagThreads) { // (one chunk unless nx > 1024)
    const int g = g0 + tid;
    const bool valid = g < band_groups;
    const size_t p = valid ? (size_t)(j0 + g / gpr) * nx + 4 * (size_t)(g % gpr) : 0; // first of the lane's four points
    float4 x[kDiagMonths];
#pragma unroll
    for (int m = 0; m < kDiagMonths; ++m)
      x[m] = valid ? *reinterpret_cast<const float4*>(src + (size_t)m * nv * np + p) : make_float4(0.f, 0.f, 0.f, 0.f);

    if (a.annual && valid) { // sum jday_mon[m] * X_m / 365
      double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
      for (int m = 0; m < kDiagMonths; ++m) {
        s0 = fma(jday[m], (double)x[m].x, s0); s1 = fma(jday[m], (double)x[m].y, s1);
        s2 = fma(jday[m], (double)x[m].z, s2); s3 = fma(jday[m], (double)x[m].w, s3);
      }
      *reinterpret_cast<float4*>(a.annual + ((size_t)member * nv + var) * np + p) =
          make_float4((float)(s0 / 365.0), (float)(s1 / 365.0), (float)(s2 / 365.0), (float)(s3 / 365.0));
    }

    if (a.zonal) {
#pragma unroll
      for (int m = 0; m < kDiagMonths; ++m)
        zs[m][tid] = ((double)x[m].x + (double)x[m].y) + ((double)x[m].z + (double)x[m].w);
      __syncthreads();
      const bool last = g0 + kDiagThreads >= band_groups;
      for (int t = tid; t < kDiagMonths * rows; t += kDiagThreads) {
        const int m = t / rows, row = t % rows;
        const int ga = max(row * gpr, g0), gb = min((row + 1) * gpr, min(g0 + kDiagThreads, band_groups));
        double s = 0.0;
        for (int q = ga; q < gb; ++q) s += zs[m][q - g0];
        if (band_groups > kDiagThreads) { // rows == 1: thread t = month m carries the row's sum over the chunks
          zcarry += s;
          s = zcarry;
        }
        if (last)
          a.zonal[(((size_t)member * kDiagMonths + m) * nv + var) * a.ny + j0 + row] = (float)(s / (double)nx);
      }
      __syncthreads();
    }

    if (do_regions) {
      for (int r = 0; r < a.nr; ++r) {
        double w0 = 0, w1 = 0, w2 = 0, w3 = 0;
        if (valid) {
          const double2* wp = reinterpret_cast<const double2*>(a.w + (size_t)r * np + p);
          const double2 wa = wp[0], wb = wp[1];
          w0 = wa.x; w1 = wa.y; w2 = wb.x; w3 = wb.y;
        }
#pragma unroll
        for (int m = 0; m < kDiagMonths; ++m) {
          const double v = wave_sum(fma(w3, (double)x[m].w, fma(w2, (double)x[m].z, fma(w1, (double)x[m].y, w0 * (double)x[m].x))));
          if (lane == 0) red[wave][m][r] += v; // (the slot is this lane's alone)
        }
      }
    }
  }
  if (do_regions) {
    __syncthreads();
    double* out = a.partials + (((size_t)member * nv + var) * nbands + band) * kDiagMonths * a.nr;
    for (int t = tid; t < kDiagMonths * a.nr; t += kDiagThreads) {
      const int m = t / a.nr, r = t % a.nr;
      out[t] = ((red[0][m][r] + red[1][m][r]) + red[2][m][r]) + red[3][m][r];
    }
  }
}

__global__ __launch_bounds__(kDiagThreads) void diag_regions_kernel(DiagArgs a, int nbands, int n_members) {
  const size_t per_member = (size_t)kDiagMonths * a.nv * a.nr;
  const size_t i = (size_t)blockIdx.x * kDiagThreads + threadIdx.x; // output order: [member][month][variable][region]
  if (i >= per_member * n_members) return;
  const int member = (int)(i / per_member);
  const int rest = (int)(i % per_member);
  const int r = rest % a.nr, var = (rest / a.nr) % a.nv, m = rest / (a.nr * a.nv);
  const double* part = a.partials + ((size_t)member * a.nv + var) * nbands * kDiagMonths * a.nr + (size_t)m * a.nr + r;
  double s = 0.0;
  for (int b = 0; b < nbands; ++b) s += part[(size_t)b * kDiagMonths * a.nr]; // south to north
  a.regions[(size_t)member * a.regions_stride + rest] = (float)(s * a.inv_sum[r]);
}

} // namespace

hipError_t launch_diag_year(const DiagArgs& a, int n_members, hipStream_t s) {
  if (!a.regions && !a.zonal && !a.annual) return hipSuccess;
  const int band_rows = diag_band_rows(a.nx), nbands = diag_bands(a.nx, a.ny);
  for (int m0 = 0; m0 < n_members; m0 += 65535) { // (grid.z)
    const int n = n_members - m0 < 65535 ? n_members - m0 : 65535;
    DiagArgs b = a;
    b.monthly += (size_t)m0 * kDiagMonths * a.nv * a.nx * a.ny;
    if (b.partials) b.partials += diag_partials(a.nx, a.ny, m0, a.nr, a.nv);
    if (b.regions) b.regions += (size_t)m0 * a.regions_stride;
    if (b.zonal) b.zonal += (size_t)m0 * kDiagMonths * a.nv * a.ny;
    if (b.annual) b.annual += (size_t)m0 * a.nv * a.nx * a.ny;
    hipLaunchKernelGGL(diag_year_kernel, dim3((unsigned)nbands, (unsigned)a.nv, (unsigned)n), dim3(kDiagThreads), 0, s, b, band_rows, nbands);
    if (b.regions) {
      const size_t total = (size_t)n * kDiagMonths * a.nv * a.nr;
      hipLaunchKernelGGL(diag_regions_kernel, dim3((unsigned)((total + kDiagThreads - 1) / kDiagThreads)), dim3(kDiagThreads), 0, s,
                         b, nbands, n);
    }
  }
  return hipGetLastError();
}

} // namespace greb
