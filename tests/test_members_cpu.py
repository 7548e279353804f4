"""CPU: per-member configurations (greb_member_config, greb_engine_create_members, greb_engine_set_member_experiments)
-- struct layout, exports, the argument checks that come before the device query, and the host-side helpers
(ensemble.switch_factorial, ensemble.perturbed_physics with any field names).  No compute call is made here."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from greb_climate_model_amd import abi, build, engine, ensemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return engine.lib()


def test_member_config_layout():
    """sizeof and field offsets of the ctypes mirror: by arithmetic (greb_params is 44 four-byte words), and against
    what a C compiler makes of include/greb_engine.h where one is present."""
    assert C.sizeof(abi.GrebParams) == (28 + 10 + 1) * 4 + 5 * 4
    assert abi.GrebMemberConfig.p.offset == 0
    assert abi.GrebMemberConfig.switches.offset == C.sizeof(abi.GrebParams)
    assert C.sizeof(abi.GrebMemberConfig) == C.sizeof(abi.GrebParams) + 4
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        return
    fields = ["p", "switches", "p.kappa", "p.p_emi", "p.co2_flux", "p.ipx", "p.dt_crcl"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "greb_engine.h"\nint main(void) {\n'
           '  printf("%zu\\n", sizeof(greb_member_config));\n' +
           "".join(f'  printf("%zu\\n", offsetof(greb_member_config, {f}));\n' for f in fields) + "  return 0;\n}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "layout.c"), "w").write(src)
        exe = os.path.join(d, "layout")
        subprocess.run([cc, "-std=c11", "-I" + os.path.join(ROOT, "include"), os.path.join(d, "layout.c"), "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    P = abi.GrebParams
    want = [C.sizeof(abi.GrebMemberConfig), 0, abi.GrebMemberConfig.switches.offset, P.kappa.offset, P.p_emi.offset,
            P.co2_flux.offset, P.ipx.offset, P.dt_crcl.offset]
    assert got == want, (got, want)


def test_new_entries_exported_and_library_reads_no_environment(lib):
    for n in ("greb_engine_create_members", "greb_engine_set_member_experiments"):
        assert n in engine.EXPORTS and hasattr(lib, n), n
    dyn = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True, check=True).stdout
    assert "greb_engine_create_members" in dyn and "greb_engine_set_member_experiments" in dyn
    und = subprocess.run(["nm", "-D", "--undefined-only", build.LIB], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und


def _create(lib, inputs, members, p=None):
    p = p or engine.params_default()
    out = C.c_void_p()
    f, keep = abi.make_fields(inputs)
    rc = lib.greb_engine_create_members(C.byref(p), inputs.nx, inputs.ny, C.byref(f), len(members),
                                        engine.member_configs(p, members), 0, 0, C.byref(out))
    msg = lib.greb_engine_last_error(out if out else None).decode()
    if out:
        lib.greb_engine_destroy(out)
    return rc, msg


@pytest.mark.parametrize("field,value", [("z_vapor", 4000.0), ("dt", 21600), ("ipx", 7)])
def test_fields_shared_by_every_member_must_equal_the_engines(lib, inputs, field, value):
    """Reached before the device query: GREB_E_INVALID (-1), not GREB_E_NOGPU (-2), also without a GPU."""
    p = engine.params_default()
    cfg = engine.member_configs(p, [{}, {"ce": 1e-3}, {}])
    setattr(cfg[2].p, field, value)
    out = C.c_void_p()
    f, keep = abi.make_fields(inputs)
    rc = lib.greb_engine_create_members(C.byref(p), inputs.nx, inputs.ny, C.byref(f), 3, cfg, 0, 0, C.byref(out))
    msg = lib.greb_engine_last_error(None).decode()
    assert rc == -1 and not out, (rc, msg)
    assert field in msg and "member 2" in msg, msg


def test_unknown_switch_bits_and_bad_arguments(lib, inputs):
    rc, msg = _create(lib, inputs, [{}, {"switches": 0x100}])
    assert rc == -1 and "switch" in msg and "member 1" in msg, (rc, msg)
    p = engine.params_default()
    out = C.c_void_p()
    f, keep = abi.make_fields(inputs)
    assert lib.greb_engine_create_members(C.byref(p), 96, 48, C.byref(f), 1, None, 0, 0, C.byref(out)) == -1
    cfg = engine.member_configs(p, [{}])
    assert lib.greb_engine_create_members(C.byref(p), 95, 48, C.byref(f), 1, cfg, 0, 0, C.byref(out)) == -1
    assert lib.greb_engine_create_members(C.byref(p), 96, 48, C.byref(f), 0, cfg, 0, 0, C.byref(out)) == -1
    assert lib.greb_engine_set_member_experiments(None, None) == -1


def test_valid_members_reach_the_device_query(lib, inputs):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    rc, msg = _create(lib, inputs, [{}, {"ct_sens": 20.0, "p_emi": [1.0] * 10, "co2_flux": 340.0, "log_exp": 13}])
    assert rc == -2 and "no CPU path" in msg, (rc, msg)


def test_member_configs_from_dicts(lib):
    p = abi.default_params(ipx=95, ipy=38)
    cfg = engine.member_configs(p, [{}, {"kappa": 7e5, "switches": abi.X_NO_ICE}, {"log_exp": 8, "cp_land": 900.0}])
    assert cfg[0].switches == 0 and cfg[0].p.kappa == p.kappa and cfg[0].p.ipx == 95
    assert cfg[1].switches == abi.X_NO_ICE and cfg[1].p.kappa == np.float32(7e5) and cfg[1].p.ce == p.ce
    assert cfg[2].switches == abi.X_VAPOR_DIFFUSION_ONLY | abi.X_NO_DEEP_OCEAN and cfg[2].p.cp_land == 900.0
    with pytest.raises(engine.GrebError):
        engine.member_configs(p, [{"dt": 3600}])  # not a float field: shared by every member
    with pytest.raises(engine.GrebError):
        engine.member_configs(p, [{"switches": 1, "log_exp": 5}])


def test_switch_factorial():
    s = ensemble.switch_factorial()
    assert s.dtype == np.uint32 and s.shape == (256,)
    assert len(set(s.tolist())) == 256 and s.min() == 0 and s.max() == 255
    assert np.all(np.diff(s.astype(np.int64)) > 0)
    s = ensemble.switch_factorial(0x0f)
    assert s.tolist() == list(range(16))
    s = ensemble.switch_factorial(abi.X_NO_ICE | abi.X_NO_CIRCULATION)
    assert s.tolist() == [0, 1, 16, 17]


# sha256 of perturbed_physics(n, abi.default_params()).tobytes() before `names` existed (float32 [n][4])
PERTURBED_BEFORE = {1: "aff349aa9ff6eb84f39901acbfc151bb8b7f4e183add6e919ee0c8a0b567112c",
                    8: "5b05a2b56fb5491e4c7d722bd393c4d662b5c7e52005701f658ec988ec40bdd5",
                    64: "cae7ef362ff73be1766e6c4021cfb3969df72192ab40f854feee4c8631988429"}


@pytest.mark.parametrize("n", [1, 8, 64])
def test_perturbed_physics_default_names_draw_what_they_drew(n):
    a = ensemble.perturbed_physics(n, abi.default_params())
    assert a.dtype == np.float32 and a.shape == (n, 4)
    assert hashlib.sha256(a.tobytes()).hexdigest() == PERTURBED_BEFORE[n]


def test_perturbed_physics_any_names():
    p = abi.default_params()
    names = ("ct_sens", "ce", "cq_rain")
    a = ensemble.perturbed_physics(16, p, names=names)
    assert a.shape == (16, 3) and np.array_equal(a, ensemble.perturbed_physics(16, p, names=names))
    base = np.asarray([getattr(p, k) for k in names], np.float64)
    r = a.astype(np.float64) / base[None]
    assert r.min() >= 0.9 - 1e-6 and r.max() <= 1.1 + 1e-6, (r.min(), r.max())
    assert len(np.unique(a[:, 0])) == 16
    # same stream positions as the definition: u = splitmix64(seed, len(names) * n).reshape(n, len(names))
    u = ensemble.splitmix64(20261004, 3 * 16).reshape(16, 3)
    assert np.array_equal(a, (base[None] * (0.9 + 0.2 * u)).astype(np.float32))
