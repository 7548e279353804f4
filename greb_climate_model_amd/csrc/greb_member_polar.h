// greb_member_polar.h -- the polar rows 0 / 47 of the fused member kernel's sub-step: the STRICT chain of one pole per
// wave (chain_substep_strict) and the FAST form, all four (pole, tracer) chains in one wave (QuadChain)
#pragma once

#include "greb_member_lds.h"

namespace greb {

// ---------------------------------------------------------------------------------------------
// polar rows, STRICT: one wave per pole, 48 lanes x 2 longitudes x (Tair,q), the reference's expression trees
// ---------------------------------------------------------------------------------------------
// float offset, inside a [half][quad][4] row, of the longitude pair (2l, 2l+1)
__device__ __forceinline__ int pair_off(int l) { return (l & 1) * kHalfRow + (l >> 1) * 4; }
__device__ __forceinline__ void load_win10(const lfloat* row, int l, v2 t[10]) {
  // lanes l-2 .. l+2 (mod 48) -> longitudes 2l-4 .. 2l+5
  const int lm2 = l >= 2 ? l - 2 : l + 46, lm1 = l >= 1 ? l - 1 : 47, lp1 = l <= 46 ? l + 1 : 0, lp2 = l <= 45 ? l + 2 : l - 46;
  const int idx[5] = {lm2, lm1, l, lp1, lp2};
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const vfloat4 a = *(const __attribute__((address_space(3))) vfloat4*)(row + pair_off(idx[i]));
    t[2 * i] = v2{a.x, a.y}; t[2 * i + 1] = v2{a.z, a.w};
  }
}
__device__ __forceinline__ void st_pair2(lfloat* p, v2 a, v2 b) {
  vfloat4 x; x.x = a.x; x.y = a.y; x.z = b.x; x.w = b.y;
  *(__attribute__((address_space(3))) vfloat4*)p = x;
}

__device__ __forceinline__ void chain_substep_strict(lfloat* lds, int cur, int pole, int l /* lane */, bool calm_q = false) {
  if (l >= 48) return; // idle lanes (no workgroup barrier inside this function)
  const int k = pole ? NY - 1 : 0;
  const RowK rk = row_consts((const lfloat*)(lds + kOffRowK), k);
  const lfloat* Xc = lds + kOffX + cur * XB;
  const lfloat* Wc = lds + kOffW;
  v2 T0w[10], w[10];
  load_win10(Xc + k * RS, l, T0w);
  load_win10(Wc + k * RS, l, w);
  const float u0 = lds[kOffWX + k * NX + 2 * l], u1 = lds[kOffWX + k * NX + 2 * l + 1]; // raw winds
  const float v0 = lds[kOffWY + k * NX + 2 * l], v1 = lds[kOffWY + k * NX + 2 * l + 1];
  const int k1 = pole ? k - 1 : k + 1, k2 = pole ? k - 2 : k + 2; // towards the interior
  v2 T1[2], T2[2], W1[2], W2[2];
  {
    const vfloat4 a = *(const __attribute__((address_space(3))) vfloat4*)(Xc + k1 * RS + pair_off(l));
    const vfloat4 b = *(const __attribute__((address_space(3))) vfloat4*)(Xc + k2 * RS + pair_off(l));
    const vfloat4 c = *(const __attribute__((address_space(3))) vfloat4*)(Wc + k1 * RS + pair_off(l));
    const vfloat4 d = *(const __attribute__((address_space(3))) vfloat4*)(Wc + k2 * RS + pair_off(l));
    T1[0] = v2{a.x, a.y}; T1[1] = v2{a.z, a.w}; T2[0] = v2{b.x, b.y}; T2[1] = v2{b.z, b.w};
    W1[0] = v2{c.x, c.y}; W1[1] = v2{c.z, c.w}; W2[0] = v2{d.x, d.y}; W2[1] = v2{d.z, d.w};
  }
  const v2 own[2] = {T0w[4], T0w[5]};
  const bool bug_lane = (l == 46); // its 2nd point is longitude xdim-2 (1-based), :881
  // Between two Jacobi sweeps a lane needs the new values of lanes l-2 .. l+2 (mod 48).  They travel by
  // ds_bpermute_b32 -- lane to lane through the LDS crossbar, no memory, no bank conflicts, ONE hop -- instead of a
  // ds_write + s_waitcnt + ds_read round trip through a row buffer behind the bulk waves' read traffic.  The chain
  // of 8 dependent sweeps is the floor of a sub-step: 4 700 busy cycles per sub-step with the row buffers, 4 100 so.
  const int am2 = 4 * (l >= 2 ? l - 2 : l + 46), am1 = 4 * (l >= 1 ? l - 1 : 47), ap1 = 4 * (l <= 46 ? l + 1 : 0),
            ap2 = 4 * (l <= 45 ? l + 2 : l - 46);
  auto from = [](int addr, v2 x) {
    return v2{__int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(x.x))),
              __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(x.y)))};
  };
  const float uu[2] = {u0, u1};

  v2 Th[2][2]; // [diffusion, advection][point]
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    // the row constants come from LDS (per lane) but are the same in every lane: a scalar trip count keeps the
    // sweep loop free of exec-mask bookkeeping
    const int time2 = __builtin_amdgcn_readfirstlane(which ? rk.adv_time2 : rk.dif_time2);
    const float cc = which ? rk.adv_cc : rk.dif_cc;
    v2 T[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) T[i] = T0w[i];
    v2 th[2] = {own[0], own[1]};
    for (int tt = 0; tt < time2; ++tt) {
      if (tt > 0) { // T[0] and T[9] are not referenced by either stencil
        T[1] = from(am2, th[1]); T[2] = from(am1, th[0]); T[3] = from(am1, th[1]);
        T[4] = th[0]; T[5] = th[1];
        T[6] = from(ap1, th[0]); T[7] = from(ap1, th[1]); T[8] = from(ap2, th[0]);
      }
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) {
#pragma clang fp contract(off)
        const int c = 4 + pt;
        v2 dd;
        if (which) dd = adv_lon_sub_point_strict(T, w, uu[pt], cc, c, bug_lane && pt == 1);
        else dd = div20(cc * dif_S_strict(T, w, c));
        dd = clamp_e(dd, T[c]); // :715 / :907
        th[pt] = T[c] + dd;
      }
    }
    Th[which][0] = th[0]; Th[which][1] = th[1];
  }

  // ---- latitudinal terms + update (:585-590, :756-795, :721, :913, :549)
  v2 xn[2];
  const float vv[2] = {v0, v1};
#pragma unroll
  for (int pt = 0; pt < 2; ++pt) {
#pragma clang fp contract(off)
    const v2 t0 = own[pt], w0 = w[4 + pt], a1 = T1[pt], a2 = T2[pt], b1 = W1[pt], b2 = W2[pt];
    const float vm = split_m(vv[pt]), vp = split_p(vv[pt]);
    v2 dTy, aTy;
    if (pole == 0) {
      dTy = rk.dif_ccy * b1 * (-t0 + a1);                                        // :589
      aTy = div3(rk.adv_ccy * (vp * (b1 * (t0 - a1) + b2 * (t0 - a2))));         // :759-761
    } else {
      dTy = rk.dif_ccy * b1 * (a1 - t0);                                         // :590
      aTy = div3(rk.adv_ccy * (-vm * (b1 * (t0 - a1) + b2 * (t0 - a2))));        // :792-794
    }
    const v2 dd = w0 * ((Th[0][pt] - t0) + dTy); // :718, :721
    const v2 da = (Th[1][pt] - t0) + aTy;        // :910, :913
    const v2 xd = t0 + dd;
    v2 x = xd + da;                              // :549
    if (calm_q) x.y = xd.y;                      // orig :562
    xn[pt] = x;
  }
  st_pair2(lds + kOffX + (cur ^ 1) * XB + k * RS + pair_off(l), xn[0], xn[1]);
}

// ---------------------------------------------------------------------------------------------
// FAST polar rows: all four chains -- (pole, tracer) -- in ONE wave
// ---------------------------------------------------------------------------------------------
// A DPP row of 16 lanes x 6 points is one 96-point latitude circle whose periodic boundary is the row rotate
// (row_ror:1 / row_ror:15), so the four rows of a wavefront hold the four polar chains of a member: lanes 0-15
// (south pole, Tair), 16-31 (south, q), 32-47 (north, Tair), 48-63 (north, q).  The sweeps are greb_chain6.h's
// (36 instructions for all four chains; the earlier form -- one wave per pole, 48 lanes x 2 points x (Tair,q), halos
// by 12 ds_bpermute per sweep -- needed ~45 per pole and waited for the LDS crossbar in every one of the 9 sweeps:
// 4 400 busy cycles per sub-step on two waves, now ~2 100 on one).  The coefficients of the diffusion chain are fixed
// for the run and those of the advection sweep for the model step; both are rebuilt per circulation call so that
// nothing of this lives across the point-physics phase.
struct QuadChain {
  ChainK kd, ka;             // d[i] = sum_m K[i][m] e[i+m] (greb_chain6.h): zonal diffusion, zonal advection
  float w0[6], W1[6], W2[6]; // weights of the own row and of the two rows towards the interior
  float own[6];              // the lane's points: loaded once per circulation call, then carried from sub-step to sub-step
  float cv[6];               // the latitudinal advection coefficient of the point: (ccy/3) min(v,0) south, -(ccy/3) max(v,0) north
  float ccy;                 // dif_ccy
  int at[3];                 // float offsets, within a row, of the lane's three longitude pairs (+ its tracer)
  int row[3];                // float offsets, within a guarded buffer, of rows k, k1, k2
  int time2_dif, time2_adv;
  bool calm;                 // vapour lane of an experiment that diffuses vapour without advecting it
};

__device__ __forceinline__ void quad_chain_setup(const lfloat* lds, int cur, int lane, bool calm_q, QuadChain& c) {
  const int r = lane >> 4, j = lane & 15, pole = r >> 1, C = r & 1;
  const int k = pole ? NY - 1 : 0, k1 = pole ? k - 1 : k + 1, k2 = pole ? k - 2 : k + 2; // towards the interior
  const RowK rk = row_consts((const lfloat*)(lds + kOffRowK), k);
  c.time2_dif = rk.dif_time2; c.time2_adv = rk.adv_time2; c.ccy = rk.dif_ccy;
  c.calm = calm_q && C == 1;
  c.row[0] = k * RS; c.row[1] = k1 * RS; c.row[2] = k2 * RS;
#pragma unroll
  for (int t = 0; t < 3; ++t) c.at[t] = pair_off(3 * j + t) + C;
  const lfloat* Wc = lds + kOffW;
  // (static_for: compile-time indices from the start -- arrays indexed by the variable of a `#pragma unroll` loop are
  // still dynamically indexed when the compiler decides what may live in registers)
  float w[12]; // longitudes 6j-3 .. 6j+8
  static_for<12>([&](auto I) {
    constexpr int i = I;
    int x = 6 * j - 3 + i;
    x = x < 0 ? x + NX : (x >= NX ? x - NX : x);
    w[i] = Wc[c.row[0] + pair_off(x >> 1) + (x & 1) * 2 + C];
  });
  const float third = rk.adv_ccy * (1.f / 3.f), csd = rk.dif_cc * 0.05f, csa = rk.adv_cc * 0.05f;
  float Kd[6][6], Ka[6][6];
  static_for<6>([&](auto I) {
    constexpr int i = I, p = 3 + i;
    const int o = c.at[i >> 1] + (i & 1) * 2;
    c.w0[i] = w[p];
    c.own[i] = lds[kOffX + cur * XB + c.row[0] + o];
    c.W1[i] = Wc[c.row[1] + o];
    c.W2[i] = Wc[c.row[2] + o];
    const float u = lds[kOffWX + k * NX + 6 * j + i], v = lds[kOffWY + k * NX + 6 * j + i]; // raw winds in the polar rows
    // south pole: only the v<0 part couples (rows 1,2); north pole: only the v>=0 part (rows 46,45)  (:759-761, :792-794)
    c.cv[i] = pole == 0 ? third * fminf(v, 0.f) : -third * fmaxf(v, 0.f);
    // 6(Pp[c] - Pm[c-1]) + 3(Pp[c+1] - Pm[c-2]) + (Pp[c+2] - Pm[c-3]), :595-600 in edge-flux form
    Kd[i][0] = -csd * w[p - 3]; Kd[i][1] = (-3.f * csd) * w[p - 2]; Kd[i][2] = (-6.f * csd) * w[p - 1];
    Kd[i][3] = (6.f * csd) * w[p + 1]; Kd[i][4] = (3.f * csd) * w[p + 2]; Kd[i][5] = csd * w[p + 3];
    // -up (10 Pp[c] + 4 Pp[c+1] + Pp[c+2]) - um (10 Pm[c-1] + 4 Pm[c-2] + Pm[c-3]), :845-851
    const float um = csa * fmaxf(u, 0.f), up = csa * fminf(u, 0.f);
    Ka[i][0] = -um * w[p - 3]; Ka[i][1] = (-4.f * um) * w[p - 2]; Ka[i][2] = (-10.f * um) * w[p - 1];
    Ka[i][3] = (-10.f * up) * w[p + 1]; Ka[i][4] = (-4.f * up) * w[p + 2]; Ka[i][5] = -up * w[p + 3];
    if (i == 3 && j == 15) { // longitude xdim-2 (1-based), :881: the 4* term vanishes, the 1* term is w(1)*(T(xdim-1)-T(1))
      Ka[i][4] = -up * w[p + 3]; Ka[i][5] = -up * w[p + 3];
    }
  });
  c.kd = chain_pack(Kd);
  c.ka = chain_pack(Ka);
}

__device__ __forceinline__ void quad_chain_substep(lfloat* lds, int cur, QuadChain& c) {
  const lfloat* Xc = lds + kOffX + cur * XB;
  // (the own row is this wave's alone: what it stored last sub-step is what it would read now, so the chain starts
  // without an LDS round trip; the neighbour rows are requested here and not needed before the epilogue)
  float own[6], T1[6], T2[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int o = c.at[i >> 1] + (i & 1) * 2;
    own[i] = c.own[i];
    T1[i] = Xc[c.row[1] + o];
    T2[i] = Xc[c.row[2] + o];
  }
  float Td[6], Ta[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) { Td[i] = own[i]; Ta[i] = own[i]; }
  chain_run6<true>(Td, c.kd, c.time2_dif); // :656-717
  chain_run6<true>(Ta, c.ka, c.time2_adv); // :861-909 (one sweep at this grid)
  // ---- latitudinal terms + update (:585-590, :756-795, :721, :913, :549)
  lfloat* out = lds + kOffX + (cur ^ 1) * XB + c.row[0];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const float g1 = c.W1[i] * (T1[i] - own[i]);
    const float d2 = c.W2[i] * (own[i] - T2[i]);
    const float ddy = c.ccy * g1;
    const float day = c.cv[i] * (d2 - g1);
    const float dd = c.w0[i] * ((Td[i] - own[i]) + ddy);
    float da = (Ta[i] - own[i]) + day;
    if (c.calm) da = 0.f; // orig :562
    c.own[i] = (own[i] + dd) + da;
    out[c.at[i >> 1] + (i & 1) * 2] = c.own[i];
  }
}

} // namespace greb
