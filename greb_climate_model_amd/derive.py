"""Derived records: per-point expressions of the state records and the flux terms, formed on the device before the reduction.

The plans reduce records that are linear in what the model writes: the five state records, the thirteen flux terms, sums of
them.  Relative humidity, ice cover as an indicator, a wet-bulb temperature, the Bowen ratio, even degrees Celsius are not,
and a mean, a variance, a quantile, a crossing or a regression of such a quantity cannot be made from the plans' products
afterwards.  A derive program forms it from each month's record where the year's records lie (csrc/greb_derive.hip;
include/greb_engine.h: greb_derive_create, greb_derive_apply_dev, greb_engine_run_derived_diag / ... / _reg):

    prog = derive.program({"ice": derive.ice_cover(0.4), "rh": derive.rel_humidity(inp, p)})
    plan = diag.Plan(inp.nx, inp.ny, diag.standard_regions(inp), n_vars=len(prog.names))
    res = engine.Engine(inp, p, n_members=512).run_diag(100, co2, plan, abi.D_REGIONS, records=prog)
    res.regions[..., res.vars.index("ice"), 1:]                 # [512][100][12][regions]: the ice extent

Expressions are built with operators: derive.state("Tsurf") - 273.15, derive.term("Q_sens") / derive.term("Q_lat"),
a >= b, a < b, derive.where(c, a, b), minimum, maximum, exp, log, atan, sqrt, abs.  program() compiles them to the postfix
form the library takes; a subtree used more than once (the same Python object) is computed once and kept in a local.
reference() is the numpy float32 statement of the stage, one IEEE operation per rounding as the kernel performs them: the
tests hold the device to it bit for bit (EXP, LOG and ATAN, which go through a float64 library, to the last bit but one).

Fields are shared by all members: rel_humidity() and wet_bulb() take the topography factor exp(-z_topo / z_air) of the
inputs given, also for members on a boundary set that replaces z_topo.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _plan, abi

STATE_NAMES = ("Tsurf", "Tair", "Tocean", "q", "albedo")  # the five state records, src/greb.f90:978-982
OP_NAMES = ("STATE", "TERM", "FIELD", "CONST", "TEE", "GET", "ADD", "SUB", "MUL", "DIV", "MIN", "MAX", "GE", "LT", "NEG", "ABS",
            "SQRT", "EXP", "LOG", "ATAN", "SELECT")  # GREB_DV_* of include/greb_engine.h, in their numbering
(STATE, TERM, FIELD, CONST, TEE, GET, ADD, SUB, MUL, DIV, MIN, MAX, GE, LT, NEG, ABS, SQRT, EXP, LOG, ATAN,
 SELECT) = range(len(OP_NAMES))
_BINARY, _UNARY = range(ADD, LT + 1), range(NEG, ATAN + 1)


def _error(msg: str):
    from . import engine
    return engine.GrebError(-1, msg)


class Expr:
    """A node of an expression: an op of OP_NAMES, its operand nodes and, for a leaf, its index, name or value."""
    __slots__ = ("op", "args", "index", "name", "value", "values")
    __hash__ = object.__hash__  # (a node is itself: == is not overloaded, the same object is the same subtree)

    def __init__(self, op, args=(), index=0, name=None, value=0.0, values=None):
        self.op, self.args, self.index, self.name, self.value, self.values = op, tuple(args), index, name, value, values

    def __add__(self, o): return Expr(ADD, (self, as_expr(o)))
    def __radd__(self, o): return Expr(ADD, (as_expr(o), self))
    def __sub__(self, o): return Expr(SUB, (self, as_expr(o)))
    def __rsub__(self, o): return Expr(SUB, (as_expr(o), self))
    def __mul__(self, o): return Expr(MUL, (self, as_expr(o)))
    def __rmul__(self, o): return Expr(MUL, (as_expr(o), self))
    def __truediv__(self, o): return Expr(DIV, (self, as_expr(o)))
    def __rtruediv__(self, o): return Expr(DIV, (as_expr(o), self))
    def __ge__(self, o): return Expr(GE, (self, as_expr(o)))
    def __lt__(self, o): return Expr(LT, (self, as_expr(o)))
    def __le__(self, o): return Expr(GE, (as_expr(o), self))
    def __gt__(self, o): return Expr(LT, (as_expr(o), self))
    def __neg__(self): return Expr(NEG, (self,))
    def __abs__(self): return Expr(ABS, (self,))

    def __bool__(self):
        raise TypeError("a derive expression has no truth value: use derive.where(c, a, b)")


def as_expr(x) -> Expr:
    """An expression as it is, a number as a constant (rounded to float32 here)."""
    if isinstance(x, Expr):
        return x
    try:
        return Expr(CONST, value=float(np.float32(x)))
    except (TypeError, ValueError):
        raise _error(f"derive: {x!r} is neither an expression nor a number") from None


def state(name) -> Expr:
    """A state record by name (STATE_NAMES) or index."""
    if isinstance(name, str):
        if name not in STATE_NAMES:
            raise _error(f"derive.state: unknown record {name!r} (one of {', '.join(STATE_NAMES)})")
        name = STATE_NAMES.index(name)
    return Expr(STATE, index=int(name))


def term(name) -> Expr:
    """A budget term by name (abi.BUDGET_NAMES) or index."""
    if isinstance(name, str):
        if name not in abi.BUDGET_NAMES:
            raise _error(f"derive.term: unknown term {name!r} (one of {', '.join(abi.BUDGET_NAMES)})")
        name = abi.BUDGET_NAMES.index(name)
    return Expr(TERM, index=int(name))


def field(name: str, values=None) -> Expr:
    """A 2-D field [ny][nx] of the caller's, the same for every member: named here, given to program(fields={name: array}) --
    or with the node itself (values)."""
    return Expr(FIELD, name=str(name), values=values)


def const(value) -> Expr:
    return as_expr(float(value))


def where(c, a, b) -> Expr:
    """c != 0 ? a : b per point (a for a NaN c)."""
    return Expr(SELECT, (as_expr(c), as_expr(a), as_expr(b)))


def minimum(a, b) -> Expr:
    """a < b ? a : b"""
    return Expr(MIN, (as_expr(a), as_expr(b)))


def maximum(a, b) -> Expr:
    """a > b ? a : b"""
    return Expr(MAX, (as_expr(a), as_expr(b)))


def exp(a) -> Expr: return Expr(EXP, (as_expr(a),))
def log(a) -> Expr: return Expr(LOG, (as_expr(a),))
def atan(a) -> Expr: return Expr(ATAN, (as_expr(a),))
def sqrt(a) -> Expr: return Expr(SQRT, (as_expr(a),))
def abs(a) -> Expr: return Expr(ABS, (as_expr(a),))  # noqa: A001 (derive.abs, beside the operator)


# ---- ready-made expressions
def celsius(name) -> Expr:
    """A temperature record in degrees Celsius: one subtraction of 273.15."""
    return state(name) - 273.15


def ice_cover(threshold: float = 0.4) -> Expr:
    """1 where the albedo is at least `threshold`, else 0: its regional mean is the ice and snow extent."""
    return state("albedo") >= threshold


def bowen() -> Expr:
    """Q_sens / Q_lat, 0 where Q_lat is zero."""
    return where(term("Q_lat"), term("Q_sens") / term("Q_lat"), 0.0)


def topo_factor(inputs, params) -> np.ndarray:
    """exp(-z_topo / z_air) in float32: what the saturation humidity of the point physics is scaled by (src/greb.f90:201)."""
    z = np.asarray(inputs.z_topo, np.float32)
    return np.exp(-(z / np.float32(params.z_air))).astype(np.float32)


def rel_humidity(inputs, params) -> Expr:
    """q over the saturation humidity of the point physics (csrc/greb_device.h: hydro; src/greb.f90:458-459):
    qs = 3.75e-3 * exp(17.08085 * (Tsurf - 273.15) / (Tsurf - 273.15 + 234.175)) * exp(-z_topo / z_air).  A fraction."""
    tc = celsius("Tsurf")
    qs = 3.75e-3 * exp(17.08085 * tc / (tc + 234.175)) * field("wz_air", topo_factor(inputs, params))
    return state("q") / qs


def wet_bulb(inputs, params) -> Expr:
    """The wet-bulb temperature in degrees Celsius by Stull (2011, J. Appl. Meteor. Climatol. 50, 2267-2269) from the
    surface temperature T in degrees Celsius and the relative humidity R in per cent:
    T atan(0.151977 sqrt(R + 8.313659)) + atan(T + R) - atan(R - 1.676331) + 0.00391838 R^1.5 atan(0.023101 R) - 4.686035."""
    t = celsius("Tsurf")
    r = 100.0 * rel_humidity(inputs, params)
    return (t * atan(0.151977 * sqrt(r + 8.313659)) + atan(t + r) - atan(r - 1.676331)
            + 0.00391838 * (r * sqrt(r)) * atan(0.023101 * r) - 4.686035)


# ---- the compiler
def _compile(name: str, root: Expr, field_index) -> list:
    """One output's postfix program [(op, arg, value), ...].  A node that is not a leaf and is reached more than once becomes a
    local: TEE where it is first computed, GET afterwards."""
    uses: dict = {}
    order = [root]
    while order:  # (no recursion: a long sum is a deep tree)
        n = order.pop()
        uses[id(n)] = uses.get(id(n), 0) + 1
        if uses[id(n)] == 1:
            order.extend(n.args)
    local: dict = {}
    ins: list = []
    depth = deepest = 0
    work = [(root, False)]
    while work:
        n, done = work.pop()
        if not done and id(n) in local:
            ins.append((GET, local[id(n)], 0.0))
            depth += 1
        elif not done and n.args:
            work.append((n, True))
            work.extend((a, False) for a in reversed(n.args))
        else:
            if n.op in (STATE, TERM):
                ins.append((n.op, n.index, 0.0))
            elif n.op == FIELD:
                ins.append((FIELD, field_index(n), 0.0))
            elif n.op == CONST:
                if not np.isfinite(n.value):
                    raise _error(f"derive.program: output {name!r}: the constant {n.value} is not finite")
                ins.append((CONST, 0, n.value))
            else:
                ins.append((n.op, 0, 0.0))
            depth += 1 - len(n.args)
            if n.args and uses[id(n)] > 1:
                if len(local) == abi.DERIVE_MAX_LOCALS:
                    raise _error(f"derive.program: output {name!r} has more than {abi.DERIVE_MAX_LOCALS} subtrees used more than once")
                local[id(n)] = len(local)
                ins.append((TEE, local[id(n)], 0.0))
        deepest = max(deepest, depth)
    if deepest > abi.DERIVE_MAX_STACK:
        raise _error(f"derive.program: output {name!r} needs a stack of {deepest} values (at most {abi.DERIVE_MAX_STACK})")
    if len(ins) > abi.DERIVE_MAX_INS:
        raise _error(f"derive.program: output {name!r} compiles to {len(ins)} instructions (at most {abi.DERIVE_MAX_INS})")
    return ins


class Program:
    """A derive program: the outputs' names, per output its instructions [(op, arg, value), ...], and the fields
    [n_fields][ny][nx] with their names.  The library's plan is made per grid on first use (handle)."""

    def __init__(self, names, instructions, fields=None, field_names=()):
        self.names = tuple(str(n) for n in names)
        self.instructions = [[(int(o), int(a), float(v)) for o, a, v in ins] for ins in instructions]
        self.fields = None if fields is None else np.ascontiguousarray(fields, np.float32)
        self.field_names = tuple(field_names)
        self._plans: dict = {}

    @property
    def n_out(self) -> int:
        return len(self.names)

    @property
    def uses_budget(self) -> bool:
        return any(op == TERM for ins in self.instructions for op, _, _ in ins)

    def ins_array(self):
        flat = [i for ins in self.instructions for i in ins]
        arr = (abi.GrebDeriveIns * max(len(flat), 1))()
        for w, (op, arg, value) in zip(arr, flat):
            w.op, w.arg, w.value = op, arg, value
        counts = np.array([len(ins) for ins in self.instructions], np.int32)
        return arr, counts

    def handle(self, nx: int, ny: int):
        """The library's plan for the grid nx x ny (greb_derive_create); an error is a GrebError with its message."""
        key = (int(nx), int(ny))
        if key not in self._plans:
            if self.fields is not None and tuple(self.fields.shape[1:]) != (ny, nx):
                raise _error(f"derive: the program's fields are {list(self.fields.shape[1:])}, the grid is [{ny}, {nx}]")
            arr, counts = self.ins_array()
            h = _plan.Handle()
            h._destroy = "greb_derive_destroy"
            h._create("greb_derive_create", int(nx), int(ny), arr, counts.ctypes.data_as(C.POINTER(C.c_int32)), len(self.names),
                      None if self.fields is None else abi.fptr(self.fields), 0 if self.fields is None else len(self.fields))
            self._plans[key] = h
        return self._plans[key].h

    def close(self):
        for h in self._plans.values():
            h.close()
        self._plans = {}

    def listing(self) -> list:
        """Per output the instructions as text: "STATE 0", "CONST 273.15", "SUB", ..."""
        out = []
        for ins in self.instructions:
            out.append([OP_NAMES[op] + (f" {arg}" if op in (STATE, TERM, FIELD, TEE, GET) else f" {value:g}" if op == CONST else "")
                        if 0 <= op < len(OP_NAMES) else f"? {op}" for op, arg, value in ins])
        return out


def program(outputs: dict, fields: dict | None = None) -> Program:
    """{"name": expression, ...} -> Program, outputs in the dict's order.  fields: {"name": array [ny][nx]} for the
    derive.field(name) nodes that do not carry their own.  No output, more than abi.MAX_RECORD_VARS outputs, an unknown field,
    more than abi.DERIVE_MAX_LOCALS shared subtrees, a stack deeper than abi.DERIVE_MAX_STACK or an output longer than
    abi.DERIVE_MAX_INS is a GrebError(-1) naming the output."""
    outputs = dict(outputs)
    if not 1 <= len(outputs) <= abi.MAX_RECORD_VARS:
        raise _error(f"derive.program: {len(outputs)} outputs (1 ... {abi.MAX_RECORD_VARS})")
    given = {str(k): np.asarray(v, np.float32) for k, v in (fields or {}).items()}
    used: dict = {}  # name -> array, in the order of first use

    def make_index(out_name):
        def field_index(n: Expr) -> int:
            if n.name not in used:
                a = given.get(n.name, None if n.values is None else np.asarray(n.values, np.float32))
                if a is None:
                    raise _error(f"derive.program: output {out_name!r}: no field {n.name!r} (given: {', '.join(given) or 'none'})")
                if a.ndim != 2 or (used and a.shape != next(iter(used.values())).shape):
                    raise _error(f"derive.program: output {out_name!r}: field {n.name!r} has shape {list(a.shape)} ([ny][nx], all alike)")
                if len(used) == abi.DERIVE_MAX_FIELDS:
                    raise _error(f"derive.program: output {out_name!r}: more than {abi.DERIVE_MAX_FIELDS} fields")
                used[n.name] = a
            return list(used).index(n.name)
        return field_index

    ins = [_compile(str(k), as_expr(e), make_index(str(k))) for k, e in outputs.items()]
    total = sum(len(i) for i in ins)
    if total > abi.DERIVE_MAX_TOTAL:
        raise _error(f"derive.program: {total} instructions in all (at most {abi.DERIVE_MAX_TOTAL})")
    return Program(outputs.keys(), ins, np.stack(list(used.values())) if used else None, tuple(used))


# ---- the numpy mirror
def reference(prog: Program, state, budget=None) -> np.ndarray:
    """The derive stage in numpy float32, operation by operation as csrc/greb_derive.hip performs it: state [..][5][ny][nx]
    float32 and, where the program names a term, budget [..][13][ny][nx] -> [..][n_out][ny][nx].  Every arithmetic op is one
    float32 operation; MIN is np.where(a < b, a, b), MAX np.where(a > b, a, b); EXP, LOG and ATAN take the operand to float64,
    call numpy's function there and round once to float32."""
    s = np.asarray(state)
    if s.dtype != np.float32 or s.ndim < 3 or s.shape[-3] != abi.NVAR_OUT:
        raise ValueError("derive.reference: float32 state [..][5][ny][nx] expected")
    b = None
    if prog.uses_budget:
        if budget is None:
            raise ValueError("derive.reference: the program names a budget term: budget [..][13][ny][nx] expected")
        b = np.asarray(budget)
        if b.dtype != np.float32 or b.shape[-3] != abi.NBUDGET or b.shape[:-3] + b.shape[-2:] != s.shape[:-3] + s.shape[-2:]:
            raise ValueError("derive.reference: float32 budget [..][13][ny][nx] beside the state expected")
    one, zero = np.float32(1), np.float32(0)
    f64 = {EXP: np.exp, LOG: np.log, ATAN: np.arctan}
    binary = {ADD: np.add, SUB: np.subtract, MUL: np.multiply, DIV: np.divide,
              MIN: lambda x, y: np.where(x < y, x, y), MAX: lambda x, y: np.where(x > y, x, y),
              GE: lambda x, y: np.where(x >= y, one, zero), LT: lambda x, y: np.where(x < y, one, zero)}
    out = np.empty(s.shape[:-3] + (prog.n_out,) + s.shape[-2:], np.float32)
    with np.errstate(all="ignore"):
        for k, ins in enumerate(prog.instructions):
            stack, local = [], {}
            for op, arg, value in ins:
                if op == STATE:
                    stack.append(s[..., arg, :, :])
                elif op == TERM:
                    stack.append(b[..., arg, :, :])
                elif op == FIELD:
                    stack.append(prog.fields[arg])
                elif op == CONST:
                    stack.append(np.float32(value))
                elif op == TEE:
                    local[arg] = stack[-1]
                elif op == GET:
                    stack.append(local[arg])
                elif op in binary:
                    y = stack.pop()
                    x = stack.pop()
                    stack.append(binary[op](x, y))
                elif op == NEG:
                    stack.append(np.negative(stack.pop()))
                elif op == ABS:
                    stack.append(np.abs(stack.pop()))
                elif op == SQRT:
                    stack.append(np.sqrt(stack.pop()))
                elif op in f64:
                    stack.append(f64[op](np.asarray(stack.pop(), np.float32).astype(np.float64)).astype(np.float32))
                elif op == SELECT:
                    y = stack.pop()
                    x = stack.pop()
                    c = stack.pop()
                    stack.append(np.where(c != 0, x, y))
                else:
                    raise ValueError(f"derive.reference: unknown op {op}")
                assert np.asarray(stack[-1]).dtype == np.float32, OP_NAMES[op]
            (r,) = stack
            out[..., k, :, :] = r
    return out


def apply_dev(prog: Program, state_year, budget_year=None):
    """One model year on the GPU: contiguous float32 torch tensors state_year [n_members][12][5][ny][nx] and, where the program
    names a term, budget_year [n_members][12][13][ny][nx], turned into [n_members][12][n_out][ny][nx] (greb_derive_apply_dev) on
    torch's current stream, without synchronising."""
    import torch
    from . import engine
    x = state_year
    dev = _plan.gpu_tensor_check(x, x.dim() == 5 and tuple(x.shape[1:3]) == (12, abi.NVAR_OUT), "derive.apply_dev",
                                 f"[n][12][{abi.NVAR_OUT}][ny][nx]")
    n, ny, nx = x.shape[0], x.shape[3], x.shape[4]
    if budget_year is not None:
        bshape = (n, 12, abi.NBUDGET, ny, nx)
        if _plan.gpu_tensor_check(budget_year, tuple(budget_year.shape) == bshape, "derive.apply_dev", f"budget_year {list(bshape)}") != dev:
            raise engine.GrebError(-1, "derive.apply_dev: state_year and budget_year are on different devices")
    h = prog.handle(nx, ny)
    out = torch.empty((n, 12, prog.n_out, ny, nx), dtype=torch.float32, device=x.device)
    _plan.call_on_current_stream(dev, engine.lib().greb_derive_apply_dev, h, int(dev), _plan.ptr(x), _plan.ptr(budget_year), int(n),
                                 _plan.ptr(out))
    return out
