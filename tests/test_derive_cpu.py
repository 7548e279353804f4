"""CPU: derived records -- the header, abi.py and the library agree; the expression compiler (greb_climate_model_amd/derive.py)
and every refusal of greb_derive_create; derive.reference against formulas written out directly in numpy.  No GPU call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from greb_climate_model_amd import abi, budget, build, derive, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["greb_derive_create", "greb_derive_destroy", "greb_derive_uses_budget", "greb_derive_apply_dev"] + [
    "greb_engine_run_derived_" + k for k in ("diag", "clim", "ens", "lin", "gram", "cross", "reg")]


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return engine.lib()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_header_abi_and_library_agree(lib):
    hdr = open(os.path.join(ROOT, "include", "greb_engine.h")).read()
    f90 = open(os.path.join(ROOT, "greb_climate_model_amd", "host", "greb_c_api.f90")).read()
    for n in SYMBOLS:
        assert n in engine.EXPORTS and hasattr(lib, n), n
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert f'name="{n}"' in f90, n
    defines = dict(re.findall(r"#define\s+(GREB_D(?:V|ERIVE)_\w+)\s+(\d+)", hdr))
    for i, name in enumerate(abi.DV_NAMES):
        assert int(defines["GREB_DV_" + name]) == i == getattr(derive, name), name
    assert len([k for k in defines if k.startswith("GREB_DV_")]) == len(abi.DV_NAMES) == len(derive.OP_NAMES) == 21
    assert derive.OP_NAMES == abi.DV_NAMES and derive.STATE_NAMES == budget.STATE_NAMES
    for name in ("INS", "TOTAL", "STACK", "LOCALS", "FIELDS"):
        assert int(defines["GREB_DERIVE_MAX_" + name]) == getattr(abi, "DERIVE_MAX_" + name), name
    assert (abi.DERIVE_MAX_INS, abi.DERIVE_MAX_TOTAL, abi.DERIVE_MAX_STACK, abi.DERIVE_MAX_LOCALS, abi.DERIVE_MAX_FIELDS) == (64, 512, 8, 4, 8)
    assert C.sizeof(abi.GrebDeriveIns) == 12
    assert "greb_derive.hip" in build.SOURCES and "greb_derive.h" in build.HEADERS
    assert build.EXTRA_FLAGS["greb_derive.hip"] == build.EXTRA_FLAGS["greb_fluxes.hip"] == ["-ffp-contract=off"]
    assert not any("fast-math" in f or f == "-Ofast" for f in build.HIPCC_FLAGS + build.EXTRA_FLAGS["greb_derive.hip"])


# ---------------------------------------------------------------- the compiler
def test_each_op_round_trips():
    """One output per op: the instructions the compiler emits, and what the mirror makes of them on a few values."""
    a, b, c = derive.state("Tsurf"), derive.term("Q_lat"), derive.field("mask")
    cases = {"add": (a + b, "ADD", np.add), "sub": (a - b, "SUB", np.subtract), "mul": (a * b, "MUL", np.multiply),
             "div": (a / b, "DIV", np.divide), "min": (derive.minimum(a, b), "MIN", lambda x, y: np.where(x < y, x, y)),
             "max": (derive.maximum(a, b), "MAX", lambda x, y: np.where(x > y, x, y)),
             "ge": (a >= b, "GE", lambda x, y: (x >= y).astype(np.float32)), "lt": (a < b, "LT", lambda x, y: (x < y).astype(np.float32))}
    prog = derive.program({k: v[0] for k, v in cases.items()}, fields={"mask": np.ones((5, 12), np.float32)})
    assert prog.listing() == [["STATE 0", "TERM 5", v[1]] for v in cases.values()]
    assert prog.uses_budget and prog.names == tuple(cases)
    rng = np.random.default_rng(1)
    s, t = rng.standard_normal((2, 5, 5, 12)).astype(np.float32), rng.standard_normal((2, 13, 5, 12)).astype(np.float32)
    s[0, 0, 0, :4], t[0, 5, 0, :4] = (0.0, np.nan, 1.0, np.inf), (-0.0, 1.0, np.nan, np.inf)
    got = derive.reference(prog, s, t)
    with np.errstate(all="ignore"):
        for k, v in enumerate(cases.values()):
            assert np.array_equal(bits(got[:, k]), bits(v[2](s[:, 0], t[:, 5]))), v[1]
    assert got[0, 4, 0, 1] == 1.0 and np.isnan(got[0, 4, 0, 2])  # MIN: a NaN in b is taken, a NaN in a is not
    assert got[0, 6, 0, 1] == 0.0 and got[0, 7, 0, 2] == 0.0 and got[0, 6, 0, 0] == 1.0  # GE, LT false with a NaN; 0 >= -0
    unary = {"neg": (-a, "NEG", np.negative), "abs": (abs(a), "ABS", np.abs), "abs2": (derive.abs(a), "ABS", np.abs),
             "sqrt": (derive.sqrt(a), "SQRT", np.sqrt), "exp": (derive.exp(a), "EXP", np.exp), "log": (derive.log(a), "LOG", np.log),
             "atan": (derive.atan(a), "ATAN", np.arctan)}
    prog = derive.program({k: v[0] for k, v in unary.items()})
    assert prog.listing() == [["STATE 0", v[1]] for v in unary.values()] and not prog.uses_budget
    got = derive.reference(prog, s)
    with np.errstate(all="ignore"):
        for k, v in enumerate(unary.values()):
            ref = v[2](s[:, 0].astype(np.float64)).astype(np.float32) if v[1] in ("EXP", "LOG", "ATAN") else v[2](s[:, 0])
            assert np.array_equal(bits(got[:, k]), bits(ref)), v[1]
    other = derive.program({"sel": derive.where(c, a, 2.5), "rev": 1.0 - a, "gt": a > 0.0, "le": a <= 0.0, "k": derive.const(3)},
                           fields={"mask": (np.arange(60).reshape(5, 12) % 2).astype(np.float32)})
    assert other.listing() == [["FIELD 0", "STATE 0", "CONST 2.5", "SELECT"], ["CONST 1", "STATE 0", "SUB"], ["CONST 0", "STATE 0", "LT"],
                               ["CONST 0", "STATE 0", "GE"], ["CONST 3"]]
    got = derive.reference(other, s)
    assert np.array_equal(bits(got[:, 0]), bits(np.where(other.fields[0] != 0, s[:, 0], np.float32(2.5))))
    assert np.array_equal(bits(got[:, 1]), bits(np.float32(1) - s[:, 0])) and (got[:, 4] == 3).all()
    assert other.field_names == ("mask",)


def test_a_shared_subtree_becomes_a_local():
    t = derive.state("Tsurf") - 273.15
    prog = derive.program({"x": t * t + t, "y": derive.state("q") * derive.state("q")})
    assert prog.listing() == [["STATE 0", "CONST 273.15", "SUB", "TEE 0", "GET 0", "MUL", "GET 0", "ADD"],
                              ["STATE 3", "STATE 3", "MUL"]]  # (a leaf is pushed again: no local)
    s = np.random.default_rng(2).uniform(250, 300, (5, 4, 8)).astype(np.float32)
    tc = s[0] - np.float32(273.15)
    assert np.array_equal(bits(derive.reference(prog, s)[0]), bits(tc * tc + tc))
    # the same expression built twice is two objects: computed twice
    twice = derive.program({"x": (derive.state(0) - 1.0) * (derive.state(0) - 1.0)})
    assert "TEE 0" not in twice.listing()[0] and len(twice.listing()[0]) == 7


def test_compiler_limits_name_the_output():
    a = derive.state("Tsurf")
    shared = [a + float(k) for k in range(5)]
    e = shared[0] * shared[0]
    for n in shared[1:]:
        e = e + n * n
    with pytest.raises(engine.GrebError) as ei:
        derive.program({"ok": a, "five_locals": e})
    assert ei.value.code == -1 and "'five_locals'" in str(ei.value) and "more than 4" in str(ei.value), str(ei.value)
    deep = a
    for _ in range(8):
        deep = a + deep  # right-nested: nine values on the stack
    with pytest.raises(engine.GrebError) as ei:
        derive.program({"deep": deep})
    assert ei.value.code == -1 and "'deep'" in str(ei.value) and "stack of 9" in str(ei.value), str(ei.value)
    eight = a
    for _ in range(7):
        eight = a + eight
    assert len(derive.program({"eight": eight}).listing()[0]) == 15
    long = a
    for _ in range(32):
        long = long + 1.0  # 1 + 2 * 32 = 65 instructions
    with pytest.raises(engine.GrebError) as ei:
        derive.program({"long": long})
    assert ei.value.code == -1 and "'long'" in str(ei.value) and "65 instructions" in str(ei.value), str(ei.value)
    sixty_three = a
    for _ in range(31):
        sixty_three = sixty_three + 1.0
    with pytest.raises(engine.GrebError) as ei:
        derive.program({f"o{k}": sixty_three for k in range(9)})  # 9 * 63 = 567 > 512
    assert ei.value.code == -1 and "567 instructions in all" in str(ei.value), str(ei.value)
    for bad, words in (({}, "0 outputs"), ({f"o{k}": a for k in range(17)}, "17 outputs"),
                       ({"f": derive.field("nowhere")}, "no field 'nowhere'"), ({"c": a * float("inf")}, "not finite")):
        with pytest.raises(engine.GrebError) as ei:
            derive.program(bad)
        assert ei.value.code == -1 and words in str(ei.value), str(ei.value)
    for call, words in ((lambda: derive.state("Tskin"), "unknown record 'Tskin'"), (lambda: derive.term("Q_x"), "unknown term 'Q_x'")):
        with pytest.raises(engine.GrebError) as ei:
            call()
        assert ei.value.code == -1 and words in str(ei.value), str(ei.value)
    with pytest.raises(TypeError):
        bool(a >= 1.0)


# ---------------------------------------------------------------- greb_derive_create
def raw(outputs, fields=None, nx=12, ny=5):
    """greb_derive_create on raw instructions [[(op, arg, value), ...], ...]: (return code, message)."""
    prog = derive.Program([f"o{k}" for k in range(len(outputs))], outputs, fields)
    try:
        prog.handle(nx, ny)
    except engine.GrebError as err:
        return err.code, str(err)
    prog.close()
    return 0, ""


S, T, F, K, TEE, GET = derive.STATE, derive.TERM, derive.FIELD, derive.CONST, derive.TEE, derive.GET


def test_create_accepts_what_the_compiler_emits(lib, inputs, params):
    prog = derive.program({"rh": derive.rel_humidity(inputs, params), "tw": derive.wet_bulb(inputs, params), "ice": derive.ice_cover(),
                           "bowen": derive.bowen()})
    h = prog.handle(inputs.nx, inputs.ny)
    assert h and prog.handle(inputs.nx, inputs.ny) is h and lib.greb_derive_uses_budget(h) == 1
    plain = derive.program({"c": derive.celsius("Tair")})
    assert lib.greb_derive_uses_budget(plain.handle(12, 5)) == 0 and lib.greb_derive_uses_budget(None) == 0
    with pytest.raises(engine.GrebError) as ei:  # the fields are of the 96 x 48 grid
        prog.handle(12, 5)
    assert ei.value.code == -1 and "[48, 96]" in str(ei.value)
    prog.close(); plain.close()
    assert lib.greb_derive_destroy(None) == 0
    assert budget.record_names(prog) == ("rh", "tw", "ice", "bowen")


@pytest.mark.parametrize("outputs,fields,words", [
    ([[(S, 0, 0)], [(S, 0, 0), (21, 0, 0)]], None, ("output 1, instruction 1", "unknown op 21")),
    ([[(-1, 0, 0)]], None, ("output 0, instruction 0", "unknown op -1")),
    ([[(S, 5, 0)]], None, ("output 0, instruction 0", "state record 5", "0 ... 4")),
    ([[(T, 13, 0)]], None, ("output 0, instruction 0", "budget term 13", "0 ... 12")),
    ([[(T, -1, 0)]], None, ("output 0, instruction 0", "budget term -1")),
    ([[(F, 1, 0)]], np.ones((1, 5, 12), np.float32), ("output 0, instruction 0", "field 1", "0 ... 0")),
    ([[(F, 0, 0)]], None, ("output 0, instruction 0", "FIELD 0", "n_fields = 0")),
    ([[(S, 0, 0), (TEE, 4, 0)]], None, ("output 0, instruction 1", "local 4", "0 ... 3")),
    ([[(S, 0, 0), (TEE, 0, 0)], [(GET, 0, 0)]], None, ("output 1, instruction 0", "GET of local 0")),  # set in ANOTHER output
    ([[(S, 0, 0), (GET, 1, 0), (derive.ADD, 0, 0)]], None, ("output 0, instruction 1", "GET of local 1")),
    ([[(S, 0, 0), (derive.ADD, 0, 0)]], None, ("output 0, instruction 1", "stack underflow", "takes 2")),
    ([[(derive.NEG, 0, 0)]], None, ("output 0, instruction 0", "stack underflow", "takes 1")),
    ([[(TEE, 0, 0)]], None, ("output 0, instruction 0", "stack underflow")),
    ([[(S, 0, 0), (S, 1, 0), (derive.SELECT, 0, 0)]], None, ("output 0, instruction 2", "stack underflow", "takes 3")),
    ([[(S, 0, 0), (S, 1, 0)]], None, ("output 0, instruction 1", "leaves 2 values")),
    ([[(S, 0, 0)] * 9 + [(derive.ADD, 0, 0)] * 8], None, ("output 0, instruction 8", "hold 9 values", "at most 8")),
    ([[(K, 0, float("inf"))]], None, ("output 0, instruction 0", "CONST inf is not finite")),
    ([[(S, 0, 0), (K, 0, float("nan")), (derive.ADD, 0, 0)]], None, ("output 0, instruction 1", "CONST nan is not finite")),
    ([[(S, 0, 0)], []], None, ("output 1 has 0 instructions", "1 ... 64")),
    ([[(S, 0, 0)] + [(derive.NEG, 0, 0)] * 64], None, ("output 0 has 65 instructions", "1 ... 64")),
    ([[(S, 0, 0)] + [(derive.NEG, 0, 0)] * 63] * 9, None, ("576 instructions in all", "at most 512")),
    ([[(S, 0, 0)]] * 17, None, ("n_out = 17", "1 ... 16")),
    ([[(S, 0, 0)]], np.ones((9, 5, 12), np.float32), ("n_fields = 9", "0 ... 8")),
], ids=lambda v: None)
def test_create_refusals_name_the_offender(lib, outputs, fields, words):
    code, msg = raw(outputs, fields)
    assert code == -1, msg
    for w in ("derive_create",) + words:
        assert w in msg, (w, msg)


def test_create_refuses_fields_and_grids(lib):
    f = np.ones((2, 5, 12), np.float32)
    f[1, 3, 7] = np.inf
    code, msg = raw([[(S, 0, 0)]], f)
    assert code == -1 and "field 1" in msg and "row 3, column 7" in msg and "not finite" in msg, msg
    code, msg = raw([[(S, 0, 0)]], nx=13)
    assert code == -1 and "grid 13 x 5" in msg, msg
    assert raw([[(S, 0, 0)] * 8 + [(derive.ADD, 0, 0)] * 7]) == (0, "")  # a stack of exactly eight
    assert raw([[(S, 0, 0)] + [(derive.NEG, 0, 0)] * 63] * 8) == (0, "")  # exactly 64 each, 512 in all
    out = C.c_void_p(1)
    ins = (abi.GrebDeriveIns * 1)()
    n = (C.c_int32 * 1)(1)
    assert lib.greb_derive_create(12, 5, None, n, 1, None, 0, C.byref(out)) == -1 and out.value is None
    assert lib.greb_derive_create(12, 5, ins, n, 1, None, 1, C.byref(out)) == -1  # n_fields > 0 with fields NULL
    assert "`fields` is NULL" in lib.greb_engine_last_error(None).decode()
    assert lib.greb_derive_create(12, 5, ins, n, 1, None, 0, None) == -1
    # _dev arguments are checked before any device query
    assert lib.greb_derive_apply_dev(None, 0, None, None, 1, None, None) == -1


# ---------------------------------------------------------------- the mirror against formulas written out
def physical_year(inputs, seed=3):
    """[2][12][5][48][96] state and [2][12][13][48][96] budget records in physical ranges."""
    rng = np.random.default_rng(seed)
    shape = (2, 12, 48, 96)
    t = rng.uniform(230.0, 315.0, shape).astype(np.float32)
    s = np.stack([t, t - np.float32(2.0), rng.uniform(271.0, 300.0, shape).astype(np.float32),
                  rng.uniform(1e-4, 0.02, shape).astype(np.float32), rng.uniform(0.05, 0.7, shape).astype(np.float32)], axis=2)
    b = (rng.standard_normal((2, 12, 13, 48, 96)) * 50.0).astype(np.float32)
    b[:, :, abi.B_Q_LAT][rng.random(shape) < 0.1] = 0.0
    b[:, :, abi.B_Q_LAT][rng.random(shape) < 0.05] = -0.0
    return s, b


def test_reference_against_formulas(inputs, params):
    s, b = physical_year(inputs)
    f32 = np.float32
    prog = derive.program({"tc": derive.celsius("Tocean"), "ice": derive.ice_cover(0.4), "bowen": derive.bowen()})
    got = derive.reference(prog, s, b)
    assert got.shape == (2, 12, 3, 48, 96) and got.dtype == np.float32
    assert np.array_equal(bits(got[:, :, 0]), bits(s[:, :, 2] - f32(273.15)))
    ice = (s[:, :, 4] >= f32(0.4)).astype(np.float32)
    assert np.array_equal(bits(got[:, :, 1]), bits(ice)) and 0 < ice.mean() < 1
    ql, qs = b[:, :, abi.B_Q_LAT], b[:, :, abi.B_Q_SENS]
    with np.errstate(all="ignore"):
        bow = np.where(ql != 0, qs / ql, f32(0))
    assert np.array_equal(bits(got[:, :, 2]), bits(bow)) and (ql == 0).any() and np.isfinite(got[:, :, 2]).all()
    # rel_humidity and wet_bulb: the same float32 operations in the same order, exp and atan through float64: equal bits
    prog = derive.program({"rh": derive.rel_humidity(inputs, params), "tw": derive.wet_bulb(inputs, params)})
    got = derive.reference(prog, s)
    wz = np.exp(-(np.asarray(inputs.z_topo, np.float32) / f32(params.z_air))).astype(np.float32)
    assert np.array_equal(bits(prog.fields[0]), bits(wz)) and prog.field_names == ("wz_air",)
    e64 = lambda x: np.exp(x.astype(np.float64)).astype(np.float32)
    at = lambda x: np.arctan(x.astype(np.float64)).astype(np.float32)
    tc = s[:, :, 0] - f32(273.15)
    qsat = f32(3.75e-3) * e64(f32(17.08085) * tc / (tc + f32(234.175))) * wz
    rh = s[:, :, 3] / qsat
    assert rh.dtype == np.float32 and np.array_equal(bits(got[:, :, 0]), bits(rh))
    r = f32(100.0) * rh
    tw = (tc * at(f32(0.151977) * np.sqrt(r + f32(8.313659))) + at(tc + r) - at(r - f32(1.676331))
          + f32(0.00391838) * (r * np.sqrt(r)) * at(f32(0.023101) * r) - f32(4.686035))
    assert tw.dtype == np.float32 and np.array_equal(bits(got[:, :, 1]), bits(tw))
    # Stull's own check value: 20 C and 50 % give 13.7 C
    one = derive.program({"tw": derive.wet_bulb(inputs, params)})
    st = np.zeros((5, 48, 96), np.float32)
    st[0] = 293.15
    st[3] = 0.5 * qsat_of(293.15, wz)
    assert abs(float(derive.reference(one, st)[0, 0, 0]) - 13.7) < 0.05


def qsat_of(t, wz):
    tc = np.float64(t) - 273.15
    return (3.75e-3 * np.exp(17.08085 * tc / (tc + 234.175)) * wz).astype(np.float32)


def test_reference_refuses_bad_input(inputs):
    prog = derive.program({"b": derive.bowen()})
    s = np.zeros((12, 5, 4, 8), np.float32)
    with pytest.raises(ValueError):
        derive.reference(prog, s)  # a term without the budget
    with pytest.raises(ValueError):
        derive.reference(prog, s.astype(np.float64), np.zeros((12, 13, 4, 8), np.float32))
    with pytest.raises(ValueError):
        derive.reference(prog, s, np.zeros((12, 13, 4, 9), np.float32))


def test_unknown_records_string_keeps_its_message():
    for bad in ("nonsense", "derived"):
        with pytest.raises(engine.GrebError) as ei:
            budget.record_names(bad)
        assert ei.value.code == -1
        assert str(ei.value) == f'greb engine error -1: records = {bad!r}: "state", "budget" or a budget.combo(...) expected'
