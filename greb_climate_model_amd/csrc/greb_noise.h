// greb_noise.h -- stochastic surface heat-flux forcing (include/greb_engine.h: "stochastic heat flux"): the generator, as
// one device function shared by the step kernels (greb_physics_step.h: physics_load) and the query kernel (greb_noise.hip).
// A member's realisation is a pure function of its 64-bit seed, the scenario step and the point's cell: a counter-based
// generator (Philox4x32-10, Salmon et al., SC'11) keyed by the seed, its counter the cell pair and the hold block.  Nothing
// of it depends on the member index, the engine size or the workgroup that integrates the member.
// The deviate z is a sum of four 16-bit uniforms, centred and scaled to variance 1: mean 0, |z| <= 3.4641, excess kurtosis
// -0.3.  Deliberately no Gaussian: it needs no log or cos, so there is nothing to hold bit-equal across math libraries --
// integer operations and two fp32 operations only, which greb_climate_model_amd/noise.py repeats bit for bit -- and the
// mixed layer sums hundreds of deviates in any case.
#pragma once
#include "greb_device.h"

namespace greb {

// greb_member_noise of include/greb_engine.h as the kernels read it: four words per member
struct MemberNoise {
  int pattern;               // -1: the member is noise-free; else the pattern that scales its noise
  float amp;                 // multiplies the pattern's sigma
  unsigned seed_lo, seed_hi; // the Philox key
};

// A pattern's words in MemberArgs::n_cells: [kNoiseShift] log2(cell_x), [kNoiseHold] hold, then one word per row j:
// (j / cell_y) * (nx / cell_x), the first cell of the row's cell row -- the division by cell_y done once, on the host.
enum { kNoiseShift, kNoiseHold, kNoiseRows };

// One member's noise of one model step (block-uniform, scalar registers; made per step, dead after physics_load).
struct NoiseStep {
  const float* sigma;        // the member's pattern [np], W/m2; null: the member takes no noise
  const int* rowcell;        // [ny] the pattern's row words (kNoiseRows)
  float season, amp;         // the pattern's seasonal factor of this step; the member's amplitude
  unsigned seed_lo, seed_hi; // the key
  unsigned b_lo, b_hi;       // the hold block: scenario step / hold, 64 bit
  int shift;                 // log2(cell_x): 0, 1, 2
};

struct NoiseWords { unsigned w0, w1, w2, w3; };

// Philox4x32-10 as published: ten rounds of c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key
// raised by the Weyl constants between rounds.
__device__ __forceinline__ NoiseWords philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return NoiseWords{c0, c1, c2, c3};
}

// two words -> z: the sum S of their four 16-bit halves (0 ... 262140, exact in fp32), centred, times
// C = 0x37DDB3D7 = fl(sqrt(3 / (65536^2 - 1))): two roundings
__device__ __forceinline__ float noise_deviate(unsigned wa, unsigned wb) {
#pragma clang fp contract(off)
  const unsigned S = (wa & 0xffffu) + (wa >> 16) + (wb & 0xffffu) + (wb >> 16);
  return ((float)S - 131070.0f) * __uint_as_float(0x37DDB3D7u);
}

// The deviates of the quad at row `row`, longitudes lon0 ... lon0 + 3 (lon0 a multiple of 4).  One Philox call serves the
// cell pair (2c, 2c + 1): at cell_x = 1 the quad is two whole pairs (nx is a multiple of 4, so its first cell is too), at
// cell_x = 2 one pair, at cell_x = 4 one cell, the half of the pair chosen by the cell's parity.
__device__ __forceinline__ f4 noise_deviates(const NoiseStep& S, int row_word, int lon0) {
  const unsigned cell = (unsigned)row_word + ((unsigned)lon0 >> S.shift);
  const NoiseWords A = philox4x32_10(cell >> 1, S.b_lo, S.b_hi, 0u, S.seed_lo, S.seed_hi);
  f4 z;
  if (S.shift == 0) {
    const NoiseWords B = philox4x32_10((cell >> 1) + 1u, S.b_lo, S.b_hi, 0u, S.seed_lo, S.seed_hi);
    z.v[0] = noise_deviate(A.w0, A.w1); z.v[1] = noise_deviate(A.w2, A.w3);
    z.v[2] = noise_deviate(B.w0, B.w1); z.v[3] = noise_deviate(B.w2, B.w3);
  } else if (S.shift == 1) {
    z.v[0] = z.v[1] = noise_deviate(A.w0, A.w1);
    z.v[2] = z.v[3] = noise_deviate(A.w2, A.w3);
  } else {
    const bool odd = cell & 1u;
    z.v[0] = z.v[1] = z.v[2] = z.v[3] = noise_deviate(odd ? A.w2 : A.w0, odd ? A.w3 : A.w1);
  }
  return z;
}

// N of the quad in W/m2: fl(fl(fl(sigma * season) * amp) * z), no contraction in either arithmetic mode
__device__ __forceinline__ f4 noise_quad(const NoiseStep& S, int row_word, int lon0, const f4& sigma) {
#pragma clang fp contract(off)
  const f4 z = noise_deviates(S, row_word, lon0);
  f4 n;
#pragma unroll
  for (int e = 0; e < 4; ++e) n.v[e] = ((sigma.v[e] * S.season) * S.amp) * z.v[e];
  return n;
}

// The step's NoiseStep of a member whose words are w (pattern >= 0), `step` the scenario step counted from 0.
__device__ __forceinline__ NoiseStep noise_step(const MemberNoise& w, const float* n_sigma, const float* n_season, const int* n_cells,
                                                int np, int ny, int ityr, unsigned long long step) {
  const int k = __builtin_amdgcn_readfirstlane(w.pattern);
  const int* cells = n_cells + (size_t)k * (kNoiseRows + ny);
  const unsigned long long b = step / (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(cells[kNoiseHold]);
  NoiseStep S;
  S.sigma = n_sigma + (size_t)k * np;
  S.rowcell = cells + kNoiseRows;
  S.season = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(n_season[(size_t)k * 730 + (ityr - 1)])));
  S.amp = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(w.amp)));
  S.seed_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)w.seed_lo);
  S.seed_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)w.seed_hi);
  S.b_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
  S.b_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
  S.shift = __builtin_amdgcn_readfirstlane(cells[kNoiseShift]);
  return S;
}

} // namespace greb
