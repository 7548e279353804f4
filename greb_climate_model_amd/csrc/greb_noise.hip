// greb_noise.hip -- greb_engine_get_noise: the stochastic heat flux N of one member and one scenario step at every point,
// through the device functions the step kernels call (greb_noise.h: noise_step, noise_quad).  A query, not a hot path: one
// quad per thread, as the any-grid point physics takes them.
#include "greb_kernels.h"

namespace greb {

__global__ __launch_bounds__(256) void noise_field_kernel(MemberNoise w, const float* __restrict__ n_sigma, const float* __restrict__ n_season,
                                                          const int* __restrict__ n_cells, int nx, int ny, long long step,
                                                          float* __restrict__ out) {
  const int np = nx * ny, qd = blockIdx.x * blockDim.x + threadIdx.x;
  if (qd >= np / 4) return;
  const NoiseStep S = noise_step(w, n_sigma, n_season, n_cells, np, ny, (int)(step % kNT) + 1, (unsigned long long)step);
  const int p0 = 4 * qd, row = p0 / nx; // a quad never straddles rows: nx is a multiple of 4
  st4(out + p0, noise_quad(S, S.rowcell[row], p0 - row * nx, ld4(S.sigma + p0)));
}

hipError_t launch_noise_field(const MemberNoise& w, const float* n_sigma, const float* n_season, const int* n_cells, int nx, int ny,
                              long long step, float* out, hipStream_t s) {
  if (w.pattern < 0 || step < 0 || nx <= 0 || ny <= 0 || (nx & 3)) return hipErrorInvalidValue;
  const int quads = nx * ny / 4;
  hipLaunchKernelGGL(noise_field_kernel, dim3((quads + 255) / 256), dim3(256), 0, s, w, n_sigma, n_season, n_cells, nx, ny, step, out);
  return hipGetLastError();
}

} // namespace greb
