"""Linear-model output: effects and sensitivities across the members, made on the device along the member axis.

An ensemble whose members differ by design is read through a linear model across them: for the factorial of the process
switches the main effect of each process and the interactions between processes, for perturbed physics the regression
slope of the response on each parameter and what the fit leaves unexplained.  All of these are linear contrasts
out_k = sum_m w[k][m] v_m; csrc/greb_lin.hip takes K <= 64 of them in one pass over the staging slot a model year was
integrated into, and the residual sum of squares of the fit design @ out (include/greb_engine.h: greb_lin_*,
greb_engine_run_lin):

    sw = ensemble.switch_factorial()                          # 256 switch words
    names, weight, design = lin.factorial(sw, 0xff, order=2)  # the mean, 8 main effects, 28 two-way interactions
    plan = lin.Plan(nx, ny, len(sw), weight, design=design)
    res = engine.Engine(inp, p, members=[{"switches": int(s)} for s in sw]).run_lin(100, 680.0, plan)
    res.coef[names.index("GREB_X_NO_ICE"), :, :, 0]           # [years][12][ny][nx]: the Tsurf main effect of the ice switch
    res.rss                                                   # what three-way and higher interactions leave

    names, weight, design = lin.regression(ensemble.perturbed_physics(256, p), ensemble.PERTURBED)
    lin.Plan(nx, ny, 256, weight, design=design)              # coef[1 + j]: the slope on parameter j; coef[0]: the intercept

reference() is the numpy statement of the products: the same IEEE operations in the same order as the kernels, so the
tests hold the device to it bit for bit.
"""
from __future__ import annotations

import ctypes as C
import itertools
from dataclasses import dataclass

import numpy as np

from . import _plan, abi

PRODUCTS = ("coef", "rss")


def selected(what: int) -> tuple:
    """Which of PRODUCTS the flags `what` (abi.L_*) deliver, as two booleans."""
    return (bool(what & abi.L_COEF), bool(what & abi.L_RSS))


def empty_products(plan, lead: tuple, rec: tuple) -> list:
    """Host arrays for the plan's products: coef [n_terms] + lead + rec, rss lead + rec; None where not selected."""
    c, r = selected(plan.what)
    return [np.empty((plan.nk,) + tuple(lead) + tuple(rec), np.float32) if c else None,
            np.empty(tuple(lead) + tuple(rec), np.float32) if r else None]


@dataclass
class Result:
    """What run_lin / reduce_dev / reference hand back; a product that was not selected is None.  coef [n_terms][..],
    rss [..] (`..` = [years][12][5][ny][nx] from Engine.run_lin, the record's shape from reduce_dev and reference)."""
    coef: object
    rss: object
    yearly: object = None
    vars: tuple = None  # the names of the variables (the axis the shapes call [5]) where the run knows them


class Plan(_plan.Handle):
    """greb_lin handle: grid, member count, weight [n_terms][n_members] (float64), which members are used (None: all), each
    member's control member (None: no control map), design [n_members][n_terms] (float64, None: none) and the products
    (abi.L_* bits; default: COEF, and RSS when a design is given).  Host data only; creating one needs no GPU, and every
    argument error is a GrebError(-1) naming the offender."""
    _destroy = "greb_lin_destroy"

    def __init__(self, nx: int, ny: int, n_members: int, weight, use=None, control=None, design=None, what: int | None = None):
        from . import engine
        self.nx, self.ny, self.nm = int(nx), int(ny), int(n_members)
        w = np.asarray(weight, np.float64)
        if w.ndim != 2 or w.shape[1] != max(self.nm, 0):
            raise engine.GrebError(-1, f"lin.Plan: weight must be [n_terms][{self.nm}], one row per term")
        self.weight = np.ascontiguousarray(w)
        self.nk = int(w.shape[0])
        self.design = None
        if design is not None:
            d = np.asarray(design, np.float64)
            if d.shape != (max(self.nm, 0), self.nk):
                raise engine.GrebError(-1, f"lin.Plan: design must be [{self.nm}][{self.nk}], one row per member")
            self.design = np.ascontiguousarray(d)
        if what is None:
            what = abi.L_COEF | (abi.L_RSS if design is not None else 0)
        self.what = int(what)

        def members(name, a):
            a = np.asarray(a)
            if a.shape != (max(self.nm, 0),) or (a.size and a.dtype.kind not in "iub"):
                raise engine.GrebError(-1, f"lin.Plan: {name} must hold {self.nm} integers, one per member")
            return np.ascontiguousarray(a, np.int32)

        self.use = None if use is None else members("use", use)
        self.control = None if control is None else members("control", control)
        ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
        dp = lambda a: None if a is None or not a.size else a.ctypes.data_as(C.POINTER(C.c_double))
        self._create("greb_lin_create", self.nx, self.ny, self.nm, dp(self.weight), self.nk, ip(self.use), ip(self.control),
                     dp(self.design), self.what & 0xFFFFFFFF)


def reduce_dev(plan: Plan, x) -> Result:
    """The plan's products of a contiguous float32 GPU tensor [n_members][...] (any trailing shape), as torch tensors coef
    [n_terms][...] and rss [...] on the same device, on torch's current stream, without synchronising
    (greb_lin_reduce_dev)."""
    import torch
    from . import engine
    dev = _plan.gpu_tensor_check(x, x.dim() >= 1 and x.shape[0] == plan.nm and x.numel() > 0, "lin.reduce_dev", f"[{plan.nm}][...]")
    rec = tuple(x.shape[1:])
    n = x.numel() // plan.nm
    c, r = selected(plan.what)
    coef = torch.empty((plan.nk,) + rec, dtype=torch.float32, device=f"cuda:{dev}") if c else None
    rss = torch.empty(rec, dtype=torch.float32, device=f"cuda:{dev}") if r else None
    _plan.call_on_current_stream(dev, engine.lib().greb_lin_reduce_dev, plan.h, int(dev), _plan.ptr(x), n, _plan.ptr(coef), _plan.ptr(rss))
    return Result(coef, rss)


def reference(x, weight, use=None, control=None, design=None, what: int | None = None) -> Result:
    """The products in numpy, operation by operation as csrc/greb_lin.hip performs them (include/greb_engine.h states
    them): x [n_members][...] float32, weight [n_terms][n_members], use [n_members] or None, control [n_members] or None,
    design [n_members][n_terms] or None.  Returns a Result of float32 arrays coef [n_terms][...] and rss [...]; products
    not in `what` are None.  Loops over the used members in ascending order and over the terms, vectorised over the
    elements; the rows of unused members that are nobody's control are not touched."""
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim < 1:
        raise ValueError("reference: float32 x [n_members][...] expected")
    w = np.asarray(weight, np.float64)
    M = x.shape[0]
    if w.ndim != 2 or w.shape[1] != M:
        raise ValueError("reference: weight [n_terms][n_members] expected")
    K = w.shape[0]
    d = None if design is None else np.asarray(design, np.float64)
    if d is not None and d.shape != (M, K):
        raise ValueError("reference: design [n_members][n_terms] expected")
    ctl = None if control is None else np.asarray(control, np.int64)
    used = np.arange(M) if use is None else np.flatnonzero(np.asarray(use))  # ascending
    if what is None:
        what = abi.L_COEF | (abi.L_RSS if d is not None else 0)
    want_c, want_r = selected(what)
    if want_r and d is None:
        raise ValueError("reference: GREB_L_RSS needs a design")
    if not len(used):
        raise ValueError("reference: no used member")
    rec = x.shape[1:]
    sample = lambda m: x[m] if ctl is None else x[m] - x[ctl[m]]  # one fp32 subtraction
    b = np.zeros((K,) + rec, np.float64)
    for m in used:
        v = sample(m)
        assert v.dtype == np.float32
        v64 = v.astype(np.float64)
        for k in range(K):
            b[k] = b[k] + w[k, m] * v64  # a multiply, then an add
    coef = b.astype(np.float32) if want_c else None
    rss = None
    if want_r:
        R = np.zeros(rec, np.float64)
        for m in used:
            f = np.zeros(rec, np.float64)
            for k in range(K):
                f = f + d[m, k] * b[k]
            r = sample(m).astype(np.float64) - f
            R = R + r * r
        rss = R.astype(np.float32)
    return Result(coef, rss)


def factorial(switch_words, bits: int = 0xff, order: int = 2):
    """The linear model of a full factorial of the switches in `bits` (abi.X_*) up to interactions of `order` switches,
    under +-1 coding: s_b(m) = +1 where member m has switch b set, -1 where not.  switch_words [n_members]: each member's
    switch word (ensemble.switch_factorial(bits)).  Returns (names, weight [n_terms][n_members], design [n_members][n_terms]):
    term S, a set of switches, has design[m] = prod_{b in S} s_b(m) and weight = design / n_members (exact in binary for
    the 2^n members of a factorial), so coef of the empty set ("mean") is the mean over the members, coef of one switch
    half the mean difference between the members with and without it, and so on; names are the GREB_X_* names of S joined
    by ":".  With order = the number of switches the model is saturated and its residual is zero."""
    sw = np.asarray(switch_words, np.int64).reshape(-1)
    which = [b for b in range(len(abi.X_NAMES)) if int(bits) >> b & 1]
    if int(bits) & ~0xff or not which:
        raise ValueError("factorial: `bits` must name some of the eight switches")
    if not 0 <= int(order) <= len(which):
        raise ValueError(f"factorial: order = {order} with {len(which)} switches")
    sign = {b: np.where(sw >> b & 1, 1.0, -1.0) for b in which}
    names, cols = [], []
    for r in range(int(order) + 1):
        for S in itertools.combinations(which, r):
            names.append(":".join(abi.X_NAMES[b] for b in S) if S else "mean")
            col = np.ones(len(sw), np.float64)
            for b in S:
                col = col * sign[b]
            cols.append(col)
    if len(names) > abi.LIN_MAX_TERMS:
        raise ValueError(f"factorial: {len(names)} terms (at most {abi.LIN_MAX_TERMS})")
    design = np.ascontiguousarray(np.stack(cols, axis=1))
    weight = np.ascontiguousarray(design.T / np.float64(len(sw)))
    return names, weight, design


def regression(predictors, names, intercept: bool = True):
    """The least-squares model of the response on `predictors` [n_members][n_predictors] (e.g. ensemble.perturbed_physics):
    design = [1, predictors] (without the column of ones when intercept is False), weight = pinv(design) in float64.
    Returns (names, weight, design) as factorial() does, the intercept's name being "intercept": coef[k] is the
    regression coefficient of term k, rss what the fit leaves unexplained."""
    X = np.asarray(predictors, np.float64)
    if X.ndim != 2 or X.shape[1] != len(names):
        raise ValueError("regression: predictors [n_members][n_predictors] and one name per predictor expected")
    design = np.ascontiguousarray(np.concatenate([np.ones((X.shape[0], 1)), X], axis=1) if intercept else X)
    if design.shape[1] > abi.LIN_MAX_TERMS:
        raise ValueError(f"regression: {design.shape[1]} terms (at most {abi.LIN_MAX_TERMS})")
    weight = np.ascontiguousarray(np.linalg.pinv(design))
    return (["intercept"] if intercept else []) + [str(n) for n in names], weight, design
