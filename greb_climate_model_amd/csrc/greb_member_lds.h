// greb_member_lds.h -- the fused member kernel's LDS map and the pair-quad accessors (greb_member.hip has the overview;
// the grid and the row stride RS are greb_member_grid.h's, the schedule greb_member_deal.h's; tools/lds_conflicts.py
// counts from all three)
#pragma once

#include "greb_member_grid.h"
#include "greb_pair.h"
#include "greb_stencil.h"

namespace greb {

// LDS map, in floats
// X buffers and W carry one all-zero GUARD row below row 0 and above row NY-1: the rows k-2 .. k+2 of any bulk
// row are then five rows at constant strides from ONE base address (immediate offsets of the ds_read), and the
// missing neighbours of rows 1 and NY-2 multiply to zero without selects.
constexpr int XB = (NY + 2) * RS;   // floats per guarded buffer
constexpr int kOffX = RS;           // row 0 of X[0]; X[b] row k at kOffX + b*XB + k*RS
constexpr int kOffW = 2 * XB + RS;  // row 0 of W  [NY][NX][{wz_air,wz_vapor}]
constexpr int kOffWX = 3 * XB;      // [NP]  cu*u   (raw u in rows 0, 47 and in STRICT)
constexpr int kOffWY = kOffWX + NP; // [NP]  ccy/3*v (raw v ...)
constexpr int kOffRowK = kOffWY + NP; // [NY][kRowKWords]
constexpr int kRowKCsDif = 7;        // FAST: dif_cc/20 in the spare word of a row's constants (Circ::init)
constexpr int kLdsFloats = kOffRowK + NY * kRowKWords;
constexpr size_t kLdsBytes = (size_t)kLdsFloats * sizeof(float);
// the member kernel's item words (greb_member_queue.h; the test mirror launches with kLdsBytes)
constexpr int kLdsItemWord = kLdsFloats; // behind the map above
constexpr size_t kLdsBytesLaunch = kLdsBytes + 16;
static_assert(kLdsBytesLaunch <= 160 * 1024, "the item word must fit the CU's LDS beside the member");

// split a pair-quad into the two tracers' scalar quads (STRICT path)
__device__ __forceinline__ f4 comp(const q8& q, int tr) {
  return tr == 0 ? f4{{q.v[0].x, q.v[1].x, q.v[2].x, q.v[3].x}} : f4{{q.v[0].y, q.v[1].y, q.v[2].y, q.v[3].y}};
}
// interleave two fields' quads into one pair-quad
__device__ __forceinline__ q8 zip(const f4& a, const f4& b) {
  q8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r.v[i] = v2{a.v[i], b.v[i]};
  return r;
}

// a pair-quad at a float offset p (two dwordx4: the [half][quad][4] row layout of greb_pair.h)
__device__ __forceinline__ q8 ld8p(const lfloat* p) {
  const vfloat4 a = *(const __attribute__((address_space(3))) vfloat4*)p;
  const vfloat4 b = *(const __attribute__((address_space(3))) vfloat4*)(p + kHalfRow);
  q8 r;
  r.v[0] = v2{a.x, a.y}; r.v[1] = v2{a.z, a.w}; r.v[2] = v2{b.x, b.y}; r.v[3] = v2{b.z, b.w};
  return r;
}

__device__ __forceinline__ void st8p(lfloat* o, const q8& xn) {
  vfloat4 a, b;
  a.x = xn.v[0].x; a.y = xn.v[0].y; a.z = xn.v[1].x; a.w = xn.v[1].y;
  b.x = xn.v[2].x; b.y = xn.v[2].y; b.z = xn.v[3].x; b.w = xn.v[3].y;
  *(__attribute__((address_space(3))) vfloat4*)o = a;
  *(__attribute__((address_space(3))) vfloat4*)(o + kHalfRow) = b;
}

} // namespace greb
