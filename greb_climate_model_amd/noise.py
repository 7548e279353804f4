"""Stochastic surface heat-flux forcing (include/greb_engine.h: "stochastic heat flux"): the numpy mirror of the device
generator (csrc/greb_noise.h), bit for bit -- integer operations and fp32 operations with one rounding each.

The deviate is a sum of four 16-bit uniforms, centred and scaled: mean 0, variance 1, |z| <= 3.4641, excess kurtosis -0.3.
Deliberately not Gaussian: nothing in it goes through log or cos, so the device and this file agree in every bit.
"""
from __future__ import annotations

import numpy as np

NSTEP_YR = 730
M0, M1 = 0xD2511F53, 0xCD9E8D57           # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85           # key increments
Z_SCALE = np.array([0x37DDB3D7], np.uint32).view(np.float32)[0]  # fl(sqrt(3 / (65536^2 - 1))) = 2.6428997e-05
Z_MAX = 3.4641


def philox4x32(counter, key, rounds: int = 10):
    """Philox4x32-`rounds` (Salmon et al., SC'11).  counter: four uint32 arrays (or scalars) that broadcast against each
    other, key: two.  Returns the four output words as a tuple of uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, np.uint64) & np.uint64(0xFFFFFFFF) for c in counter])
    k0, k1 = [np.asarray(k, np.uint64) & np.uint64(0xFFFFFFFF) for k in key]
    mask, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(rounds):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # 32 x 32 -> 64 bit: exact in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return tuple(np.asarray(c, np.uint64).astype(np.uint32) for c in (c0, c1, c2, c3))


def _seed_words(seed) -> tuple[int, int]:
    """A seed as (seed_lo, seed_hi): a 64-bit integer, or the pair itself."""
    if isinstance(seed, (tuple, list)):
        lo, hi = seed
        return int(lo) & 0xFFFFFFFF, int(hi) & 0xFFFFFFFF
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def _cells(nx: int, ny: int, cell) -> np.ndarray:
    cx, cy = int(cell[0]), int(cell[1])
    if cx not in (1, 2, 4) or not 1 <= cy <= ny or nx % 4:
        raise ValueError(f"noise: cell ({cx}, {cy}) on {nx} x {ny}: cell_x is 1, 2 or 4, cell_y 1 ... ny, nx a multiple of 4")
    j, i = np.arange(ny, dtype=np.int64)[:, None], np.arange(nx, dtype=np.int64)[None, :]
    return (j // cy) * (nx // cx) + i // cx


def deviates(seed, nx: int, ny: int, cell=(1, 1), hold: int = 1, steps=(0,)) -> np.ndarray:
    """z [len(steps)][ny][nx] in fp32 for the scenario steps `steps` (0-based, any non-negative integers below 2^64)."""
    lo, hi = _seed_words(seed)
    if int(hold) < 1:
        raise ValueError("noise: hold >= 1")
    c = _cells(nx, ny, cell)
    out = np.empty((len(steps), ny, nx), np.float32)
    for t, n in enumerate(steps):
        b = int(n) // int(hold)
        w = philox4x32((c >> 1, b & 0xFFFFFFFF, (b >> 32) & 0xFFFFFFFF, 0), (lo, hi))
        even = (c & 1) == 0
        wa, wb = np.where(even, w[0], w[2]), np.where(even, w[1], w[3])
        s = (wa & np.uint32(0xFFFF)) + (wa >> np.uint32(16)) + (wb & np.uint32(0xFFFF)) + (wb >> np.uint32(16))
        out[t] = (s.astype(np.float32) - np.float32(131070.0)) * Z_SCALE
    return out


def field(sigma, season, cell, hold, seed, amp, steps) -> np.ndarray:
    """N [len(steps)][ny][nx] in W/m2: fl(fl(fl(sigma * season[step % 730]) * amp) * z), one rounding per operation.
    sigma [ny][nx]; season [730] or None (1 everywhere)."""
    sigma = np.asarray(sigma, np.float32)
    ny, nx = sigma.shape
    season = np.ones(NSTEP_YR, np.float32) if season is None else np.asarray(season, np.float32)
    z = deviates(seed, nx, ny, cell, hold, steps)
    out = np.empty_like(z)
    for t, n in enumerate(steps):
        out[t] = ((sigma * season[int(n) % NSTEP_YR]) * np.float32(amp)) * z[t]
    return out


def seeds(n: int, base: int = 0) -> list[int]:
    """n distinct 64-bit seeds from `base`: the splitmix64 finaliser of base + m + 1 -- a bijection of the 64-bit integers, so the
    seeds differ whenever n <= 2^64."""
    out = []
    for m in range(n):
        x = (int(base) + m + 1) & 0xFFFFFFFFFFFFFFFF
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        out.append(x ^ (x >> 31))
    return out
