"""Covariance output: the Gram matrix across the members, made on the device.

lin.Plan reduces the members by contrasts the caller already knows.  Which contrasts are worth looking at -- the leading
modes of a perturbed-physics ensemble's spread -- and how far each member's response pattern lies from every other's both
come from one small object, G[a][c] = sum_i v_a[i] v_c[i] over the records of a block (include/greb_engine.h: greb_gram_*,
greb_engine_run_gram; csrc/greb_gram.hip), one matrix per block of records and model year, in float64:

    M = 256                                                        # pairs: member m at 2 x CO2, member M + m its control
    plan = gram.Plan(nx, ny, 2 * M, 60, gram.blocks_by_var(5), use=[1] * M + [0] * M,
                     control=list(range(M, 2 * M)) * 2, scale=gram.area_scale(ny, nx))
    res = eng.run_gram(100, co2, plan)                             # res.G [years][5][M][M]
    lam, frac, weight = gram.eof(res.G[-1, 0], 3, plan)            # the Tsurf response's three leading modes of spread
    eng.run_lin(1, co2, lin.Plan(nx, ny, 2 * M, weight, control=plan.control))   # ... and their patterns, in one run
    gram.distance(res.G[-1, 0])                                    # squared distances between the members' responses

reference() is the numpy statement of the matrices: the same IEEE operations in the same order as the kernels, so the
tests hold the device to it bit for bit.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _plan, abi


@dataclass
class Result:
    """What run_gram hands back: G [years][n_blocks][U][U] float64 (U used members in ascending member index), yearly, and
    the names of the variables of the records where the run knows them."""
    G: object
    yearly: object = None
    vars: tuple = None


class Plan(_plan.Handle):
    """greb_gram handle: grid, member count, the records of one member in a call (12 * n_vars for a model year), block
    [n_records] (-1 ... n_blocks - 1; -1: the record enters no matrix; n_blocks = max + 1 unless given), which members are
    used (None: all), each member's control member (None: no control map) and scale [ny][nx] (float32; None: none).  Host
    data only; creating one needs no GPU, and every argument error is a GrebError naming the offender."""
    _destroy = "greb_gram_destroy"

    def __init__(self, nx: int, ny: int, n_members: int, n_records: int, block, use=None, control=None, scale=None,
                 n_blocks: int | None = None):
        from . import engine
        self.nx, self.ny, self.nm, self.nrec = int(nx), int(ny), int(n_members), int(n_records)

        def ints(name, a, n, what):
            a = np.asarray(a)
            if a.shape != (max(n, 0),) or (a.size and a.dtype.kind not in "iub"):
                raise engine.GrebError(-1, f"gram.Plan: {name} must hold {n} integers, one per {what}")
            return np.ascontiguousarray(a, np.int32)

        self.block = ints("block", block, self.nrec, "record")
        self.nb = int(n_blocks) if n_blocks is not None else (int(self.block.max()) + 1 if self.block.size else 0)
        self.use = None if use is None else ints("use", use, self.nm, "member")
        self.control = None if control is None else ints("control", control, self.nm, "member")
        self.scale = None
        if scale is not None:
            s = np.asarray(scale)
            if s.shape != (self.ny, self.nx):
                raise engine.GrebError(-1, f"gram.Plan: scale must be [{self.ny}][{self.nx}]")
            self.scale = np.ascontiguousarray(s, np.float32)
        self.used = np.arange(max(self.nm, 0)) if self.use is None else np.flatnonzero(self.use)
        self.U = len(self.used)
        ip = lambda a: None if a is None or not a.size else a.ctypes.data_as(C.POINTER(C.c_int32))
        self._create("greb_gram_create", self.nx, self.ny, self.nm, self.nrec, ip(self.block), self.nb, ip(self.use), ip(self.control),
                     None if self.scale is None else abi.fptr(self.scale))


def reduce_dev(plan: Plan, x):
    """The plan's matrices of a contiguous float32 GPU tensor [n_members][n_records][...] (any trailing shape; [ny][nx] with
    a scale), as a float64 torch tensor [n_blocks][U][U] on the same device, on torch's current stream, without
    synchronising (greb_gram_reduce_dev)."""
    import torch
    from . import engine
    dev = _plan.gpu_tensor_check(x, x.dim() >= 2 and x.shape[0] == plan.nm and x.shape[1] == plan.nrec and x.numel() > 0,
                                 "gram.reduce_dev", f"[{plan.nm}][{plan.nrec}][...]")
    G = torch.empty((plan.nb, plan.U, plan.U), dtype=torch.float64, device=f"cuda:{dev}")
    _plan.call_on_current_stream(dev, engine.lib().greb_gram_reduce_dev, plan.h, int(dev), _plan.ptr(x), x.numel() // (plan.nm * plan.nrec),
                                 _plan.ptr(G))
    return G


def reference(x, block, use=None, control=None, scale=None, n_blocks: int | None = None, members=None) -> np.ndarray:
    """The matrices in numpy, operation by operation as include/greb_engine.h states them: x [n_members][n_records][...]
    float32, block [n_records], use / control [n_members] or None, scale [...] or None.  Returns G [n_blocks][U][U]
    float64.  One pass over the elements in ascending order, every record's matrix taking one add per element; then the
    records of a block in ascending order.  members: positions among the used members (ascending) -- the matrices of those
    alone, which are the corresponding rows and columns of the full ones.  Rows of unused members that are nobody's
    control are not touched."""
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim < 2:
        raise ValueError("reference: float32 x [n_members][n_records][...] expected")
    M, R = x.shape[:2]
    blk = np.asarray(block, np.int64)
    if blk.shape != (R,):
        raise ValueError("reference: block [n_records] expected")
    nb = int(n_blocks) if n_blocks is not None else int(blk.max()) + 1
    ctl = None if control is None else np.asarray(control, np.int64)
    used = np.arange(M) if use is None else np.flatnonzero(np.asarray(use))  # ascending
    if members is not None:
        used = used[np.asarray(members, np.int64)]
    if not len(used):
        raise ValueError("reference: no used member")
    xs = x.reshape(M, R, -1)
    listed = np.flatnonzero(blk >= 0)
    sc = None if scale is None else np.ascontiguousarray(scale, np.float32).reshape(-1)
    if sc is not None and sc.shape[0] != xs.shape[2]:
        raise ValueError("reference: scale must have the shape of a record")
    v = np.empty((len(listed), len(used), xs.shape[2]), np.float32)
    for k, m in enumerate(used):
        d = xs[m, listed] if ctl is None else xs[m, listed] - xs[ctl[m], listed]  # one fp32 subtraction
        v[:, k] = d if sc is None else sc * d                                      # one fp32 multiply
    assert v.dtype == np.float32
    vt = np.ascontiguousarray(np.moveaxis(v, 2, 0).astype(np.float64))  # [len][listed][U]
    P = np.zeros((len(listed), len(used), len(used)), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(vt.shape[0]):
            P = P + vt[i][:, :, None] * vt[i][:, None, :]  # the product is exact; one add per element
        G = np.zeros((nb, len(used), len(used)), np.float64)
        for q, r in enumerate(listed):  # ascending record
            G[blk[r]] = G[blk[r]] + P[q]
    return G


# ---- helpers ---------------------------------------------------------------------------------------------------------
def area_scale(ny: int, nx: int, mask=None) -> np.ndarray:
    """sqrt(cos(lat) * mask) [ny][nx], formed in double and rounded to float32 once: with it G is the area-weighted (and
    masked: mask in [0, 1], e.g. land only) inner product."""
    from . import diag
    w = np.cos(np.deg2rad(np.asarray(diag.latitudes(ny), np.float64)))[:, None] * np.ones((ny, nx), np.float64)
    if mask is not None:
        m = np.asarray(mask, np.float64)
        if m.shape != (ny, nx) or not (np.isfinite(m).all() and (m >= 0).all()):
            raise ValueError(f"area_scale: mask must be [{ny}][{nx}], finite and >= 0")
        w = w * m
    return np.sqrt(w).astype(np.float32)


def blocks_by_var(n_vars: int, months=None) -> np.ndarray:
    """The block map of a model year's 12 * n_vars records with one block per variable; months: the months (0 ... 11) that
    enter, None: all twelve (the others get -1)."""
    take = np.ones(12, bool) if months is None else np.isin(np.arange(12), np.asarray(months))
    b = np.where(take[:, None], np.arange(int(n_vars))[None, :], -1)
    return np.ascontiguousarray(b.reshape(-1), np.int32)


def center(G) -> np.ndarray:
    """H G H with H = I - 1 1^T / U over the last two axes: the Gram matrix of the members' deviations from their mean."""
    G = np.asarray(G, np.float64)
    return G - G.mean(axis=-1, keepdims=True) - G.mean(axis=-2, keepdims=True) + G.mean(axis=(-2, -1), keepdims=True)


def distance(G) -> np.ndarray:
    """The squared distances between the members, D[a][c] = G[a][a] + G[c][c] - 2 G[a][c], over the last two axes."""
    G = np.asarray(G, np.float64)
    d = np.diagonal(G, axis1=-2, axis2=-1)
    return d[..., :, None] + d[..., None, :] - 2.0 * G


def eof(G, k: int, plan: Plan | None = None, centered: bool = True):
    """The k leading modes of one matrix G [U][U]: (eigenvalues [k], explained fractions [k], weight [k][n_members]).  The
    modes are those of the centred matrix (centered=False: of G itself).  Row j of weight is what lin.Plan takes to return
    pattern j: e_j = sum_m weight[j][m] v_m with unit norm under the plan's scale (squared).  The centring is folded into
    the weights; they sit at the plan's used members (plan None: every member is used) and are zero elsewhere.  Modes whose
    eigenvalue is not positive get zero weights."""
    G = np.asarray(G, np.float64)
    U = G.shape[-1]
    if G.shape != (U, U) or not 1 <= int(k) <= U:
        raise ValueError("eof: one matrix [U][U] and 1 <= k <= U expected")
    Cm = center(G) if centered else G
    lam, V = np.linalg.eigh((Cm + Cm.T) * 0.5)
    order = np.argsort(lam)[::-1][:int(k)]
    lam, V = lam[order], V[:, order]
    total = float(np.trace(Cm))
    frac = lam / total if total > 0 else np.zeros_like(lam)
    if centered:
        V = V - V.mean(axis=0, keepdims=True)  # H V: the weights act on the members themselves
    w = np.where(lam > 0, V / np.sqrt(np.where(lam > 0, lam, 1.0)), 0.0).T  # [k][U]
    used = np.arange(U) if plan is None else plan.used
    nm = U if plan is None else plan.nm
    if len(used) != U:
        raise ValueError(f"eof: G is [{U}][{U}], the plan has {len(used)} used members")
    weight = np.zeros((int(k), nm), np.float64)
    weight[:, used] = w
    return lam, frac, weight
