// greb_gram.hip -- covariance output (include/greb_engine.h: greb_gram_*): the Gram matrix across the MEMBERS,
// G[b][a][c] = sum over the records r of block b, sum over the elements i of v_a[r][i] v_c[r][i], of x[member][record][len].
//
// The samples are those of greb_lin.hip: v = x[m][r][i], or x[m][r][i] - x[control[m]][r][i] as ONE fp32 subtraction, then
// optionally one fp32 multiply by scale[i].  Everything behind that is fp64.  The definition fixes the ORDER OF THE ADDS:
// P[r][a][c] runs over ascending i from +0.0 with one add per element, G[b][a][c] over the block's records in ascending
// r from +0.0.  So an accumulator's chain cannot be split along i; what runs side by side are the (a, c, r).
//
//   gram_tile_kernel  grid (listed records, 64 x 64 tiles of the lower triangle), 256 lanes.  A symmetric rank-k update:
//                     a lane owns 4 x 4 accumulators of the tile.  The tile's two member panels (one on the diagonal) go
//                     through LDS 32 elements at a time as fp64, [element][member]: the sample -- subtraction, scale,
//                     conversion -- is built once per panel, not once per pair.  The next chunk's loads are in flight while
//                     this one is multiplied.  A member row is read in 16-byte pieces where rows are 16-byte aligned (len a
//                     multiple of 4), element by element otherwise; rows behind the last used member are staged as
//                     zeros and their accumulators never stored.  Diagonal tiles form both halves: (a, c) and (c, a) see
//                     the same exact products in the same order and carry the same bits.  Writes P[q] into the plan's
//                     scratch array.
//   gram_sum_kernel   grid (elements of G / 256, blocks).  One lane per output element adds the block's P in ascending
//                     record; an element of an upper tile reads its mirror.  One owner per element, no atomics.
//
// The product of two fp32 values is exact in fp64, so a fused multiply-add rounds once exactly where a multiply followed
// by an add does: the accumulation is written as fma() and gives the bits of gram.reference, which multiplies, then adds.
// What would change them is a reassociated sum: this file is never built with fast-math (build.py: EXTRA_FLAGS gives it
// greb_lin.hip's -ffp-contract=off, which the explicit fma() does not depend on).
//
// Why two launches and a scratch array instead of one workgroup per (tile, block) looping over its records: a block's
// records would then run one after another, and a year of 60 records in 5 blocks with 256 used members is 50 workgroups
// on 256 compute units.  Per record it is 600.  The price is n_listed * U * U * 8 bytes per plan and device.
#include "greb_gram.h"

#include <cstdint>

namespace greb {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
constexpr int kStride = kGramTile + 2; // doubles of one element's row in LDS: the 8 lanes that stage one member row 4 elements
                                       // apart land in different banks, and a lane's 4 members stay 16-byte aligned
constexpr int kPass = kGramThreads / (kGramChunk / 4); // member rows staged per pass: 32
constexpr int kPasses = kGramTile / kPass;             // 2

struct GramArgs {
  const float* x; // [n_members][n_records][len]
  size_t len;
  GramTables t;
};

// elements k ... k + 3 of a row, zero from `len` on
template <bool VEC>
__device__ inline f4 load4(const float* __restrict__ row, size_t k, size_t len) {
  f4 v = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    if (k < len) v = *reinterpret_cast<const f4*>(row + k); // (len % 4 == 0: all four or none)
    return v;
  }
  if (k < len) v.x = row[k];
  if (k + 1 < len) v.y = row[k + 1];
  if (k + 2 < len) v.z = row[k + 2];
  if (k + 3 < len) v.w = row[k + 3];
  return v;
}

template <bool CTL, bool SCL, bool VEC>
__global__ __launch_bounds__(kGramThreads) void gram_tile_kernel(GramArgs a) {
  __shared__ double panel[2][kGramChunk][kStride];
  const int U = a.t.n_used;
  int ti = 0; // tile (ti, tj) of the lower triangle, tj <= ti
  while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.y) ++ti;
  const int tj = (int)blockIdx.y - ti * (ti + 1) / 2;
  const int n_panels = ti == tj ? 1 : 2;
  const int q = (int)blockIdx.x;
  const size_t rec = (size_t)a.t.record[q];
  const int tid = (int)threadIdx.x;
  const int srow = tid / (kGramChunk / 4), sk = (tid % (kGramChunk / 4)) * 4; // staging: a member row of the pass, 4 elements
  const int tx = tid % (kGramTile / kGramOwn), ty = tid / (kGramTile / kGramOwn); // multiplying: columns 4 tx ..., rows 4 ty ...

  const float* row[2][kPasses];
  const float* ctl[2][kPasses];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int h = 0; h < kPasses; ++h) {
      const int u = (p == 0 ? ti : tj) * kGramTile + h * kPass + srow;
      const bool in = p < n_panels && u < U;
      row[p][h] = in ? a.x + ((size_t)a.t.member[u] * a.t.n_records + rec) * a.len : nullptr;
      ctl[p][h] = in && CTL ? a.x + ((size_t)a.t.control[u] * a.t.n_records + rec) * a.len : nullptr;
    }

  f4 next[2][kPasses];
  auto fetch = [&](size_t k0) { // the samples of elements k0 + sk ... + 3 of this lane's rows, in fp32
    const size_t k = k0 + sk;
    f4 s = {1.f, 1.f, 1.f, 1.f};
    if (SCL) s = load4<VEC>(a.t.scale, k, a.len);
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int h = 0; h < kPasses; ++h) {
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (row[p][h]) {
          v = load4<VEC>(row[p][h], k, a.len);
          if (CTL) v = v - load4<VEC>(ctl[p][h], k, a.len);
          if (SCL) v = s * v;
        }
        next[p][h] = v;
      }
  };

  double acc[kGramOwn][kGramOwn];
#pragma unroll
  for (int i = 0; i < kGramOwn; ++i)
#pragma unroll
    for (int j = 0; j < kGramOwn; ++j) acc[i][j] = 0.0;
  auto multiply = [&](int k) {
    const double(*pa)[kStride] = panel[0];
    const double(*pc)[kStride] = panel[n_panels - 1];
    double va[kGramOwn], vc[kGramOwn];
#pragma unroll
    for (int i = 0; i < kGramOwn; ++i) { va[i] = pa[k][kGramOwn * ty + i]; vc[i] = pc[k][kGramOwn * tx + i]; }
#pragma unroll
    for (int i = 0; i < kGramOwn; ++i)
#pragma unroll
      for (int j = 0; j < kGramOwn; ++j) acc[i][j] = __builtin_fma(va[i], vc[j], acc[i][j]);
  };

  fetch(0);
  for (size_t k0 = 0; k0 < a.len; k0 += kGramChunk) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int h = 0; h < kPasses; ++h) {
        if (p >= n_panels) continue;
        const f4 v = next[p][h];
        double* col = &panel[p][sk][h * kPass + srow];
        col[0] = (double)v.x; col[kStride] = (double)v.y; col[2 * kStride] = (double)v.z; col[3 * kStride] = (double)v.w;
      }
    __syncthreads();
    if (k0 + kGramChunk < a.len) fetch(k0 + kGramChunk);
    if (a.len - k0 >= (size_t)kGramChunk) {
#pragma unroll
      for (int k = 0; k < kGramChunk; ++k) multiply(k);
    } else {
      const int kc = (int)(a.len - k0);
      for (int k = 0; k < kc; ++k) multiply(k);
    }
    __syncthreads();
  }

  double* P = a.t.partial + (size_t)q * U * U;
#pragma unroll
  for (int i = 0; i < kGramOwn; ++i) {
    const int r = ti * kGramTile + kGramOwn * ty + i;
#pragma unroll
    for (int j = 0; j < kGramOwn; ++j) {
      const int c = tj * kGramTile + kGramOwn * tx + j;
      if (r < U && c < U) P[(size_t)r * U + c] = acc[i][j];
    }
  }
}

__global__ __launch_bounds__(kGramThreads) void gram_sum_kernel(GramTables t, double* __restrict__ G) {
  const size_t U = (size_t)t.n_used, e = (size_t)blockIdx.x * kGramThreads + threadIdx.x;
  if (e >= U * U) return;
  const size_t r = e / U, c = e % U;
  const size_t at = r / kGramTile >= c / kGramTile ? e : c * U + r; // the tiles of the lower triangle hold every pair
  const int b = (int)blockIdx.y;
  double g = 0.0;
  for (int q = t.offs[b]; q < t.offs[b + 1]; ++q) g = g + t.partial[(size_t)q * U * U + at];
  G[(size_t)b * U * U + e] = g;
}

// (a scale map has ny * nx elements, a multiple of four: with one the rows are always 16-byte aligned)
template <bool CTL>
void launch_tiles(bool scaled, bool vec, dim3 grid, hipStream_t s, const GramArgs& a) {
  const dim3 block(kGramThreads);
  if (scaled) hipLaunchKernelGGL((gram_tile_kernel<CTL, true, true>), grid, block, 0, s, a);
  else if (vec) hipLaunchKernelGGL((gram_tile_kernel<CTL, false, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((gram_tile_kernel<CTL, false, false>), grid, block, 0, s, a);
}

} // namespace

hipError_t launch_gram(const float* x, size_t len, const GramTables& t, double* G, hipStream_t s) {
  if (!x || !G || len == 0 || !t.member || !t.record || !t.offs || !t.partial || t.n_used < 1 || t.n_used > kGramMaxUsed ||
      t.n_listed < 1 || t.n_listed > t.n_records || t.n_blocks < 1 || t.n_blocks > kGramMaxBlocks)
    return hipErrorInvalidValue;
  const int tiles = (t.n_used + kGramTile - 1) / kGramTile;
  const dim3 grid((unsigned)t.n_listed, (unsigned)(tiles * (tiles + 1) / 2));
  const bool vec = len % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(t.scale) & 15) == 0;
  if (t.scale && !vec) return hipErrorInvalidValue;
  const GramArgs a{x, len, t};
  if (t.control) launch_tiles<true>(t.scale != nullptr, vec, grid, s, a);
  else launch_tiles<false>(t.scale != nullptr, vec, grid, s, a);
  if (hipError_t err = hipGetLastError(); err != hipSuccess) return err;
  const size_t uu = (size_t)t.n_used * t.n_used;
  hipLaunchKernelGGL(gram_sum_kernel, dim3((unsigned)((uu + kGramThreads - 1) / kGramThreads), (unsigned)t.n_blocks),
                     dim3(kGramThreads), 0, s, t, G);
  return hipGetLastError();
}

} // namespace greb
