"""Guards on the BUILT derive kernel (CPU only: the gfx950 code objects are pulled out of libgreb_hip.so and read with
llvm-readelf / llvm-objdump).  The interpreter of csrc/greb_derive.hip keeps a value stack of eight and four locals per
lane; indexed at run time as registers they would land in scratch memory, and the stage would run at a fraction of its rate
without a single wrong number.  The top of the stack is a register, the rest and the locals an LDS column per lane: no
scratch, no spills, 16-byte LDS accesses, the program read through the scalar cache, the inputs by 16-byte non-temporal
loads."""
import os
import re
import shutil
import struct
import subprocess
import tempfile

import pytest

from greb_climate_model_amd import build

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


@pytest.fixture(scope="module")
def code_objects():
    """Every gfx950 code object of the release library (one offload bundle per source file), as temp files."""
    objcopy, objdump = _tool("llvm-objcopy"), _tool("llvm-objdump")
    if not (objcopy and objdump and _tool("llvm-readelf")):
        pytest.skip("llvm binutils not present")
    lib = build.build_lib()
    d = tempfile.mkdtemp(prefix="greb_derive_isa_")
    fat = os.path.join(d, "fat.bin")
    subprocess.run([objcopy, "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
    blob = open(fat, "rb").read()
    out, pos = [], blob.find(MAGIC)
    while pos >= 0:
        n = struct.unpack_from("<Q", blob, pos + len(MAGIC))[0]
        q = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, q)
            triple = blob[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" in triple and size:
                path = os.path.join(d, f"co{len(out)}.co")
                open(path, "wb").write(blob[pos + off:pos + off + size])
                out.append(path)
        pos = blob.find(MAGIC, pos + 1)
    assert out
    yield out
    shutil.rmtree(d, ignore_errors=True)


def _kernel_notes(path):
    txt = subprocess.run([_tool("llvm-readelf"), "--notes", path], check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in re.split(r"\n\s+- \.", txt):
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name and ".vgpr_count" in blk:
            out[name.group(1)] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                                  for k in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
    return out


def _functions(path):
    """{demangled name: [instruction text, ...]} of one code object."""
    txt = subprocess.run([_tool("llvm-objdump"), "-d", "--demangle", path], check=True, capture_output=True, text=True).stdout
    fns, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:\s*$", line)
        if m:
            cur = fns.setdefault(m.group(1), [])
            continue
        if cur is not None and line.startswith("\t"):
            ins = line.split("//")[0].strip()
            if ins:
                cur.append(ins)
    return fns


def test_derive_kernels_keep_stack_and_locals_in_registers(code_objects):
    notes = {}
    for path in code_objects:
        notes.update(_kernel_notes(path))
    derive = {k: v for k, v in notes.items() if "derive_kernel" in k}
    assert len(derive) == 2, sorted(derive)  # derive_kernel<4> and derive_kernel<26>
    for k, v in derive.items():
        print(k, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        assert v["vgpr_count"] <= 256, (k, v)
    few = [v for k, v in derive.items() if "ILi4E" in k]
    assert few and few[0]["vgpr_count"] <= 64, few  # eight wavefronts per SIMD for programs of up to four inputs


def test_derive_kernels_read_program_and_records_as_designed(code_objects):
    seen = 0
    for path in code_objects:
        for name, body in _functions(path).items():
            if "derive_kernel<" not in name or name.startswith("__"):
                continue
            seen += 1
            nin = int(re.search(r"derive_kernel<(\d+)>", name).group(1))
            assert not [i for i in body if i.startswith("scratch_") or re.match(r"^v_movrel|^s_movrel", i)], name
            loads = [i for i in body if re.match(r"^(global|flat|buffer)_load", i)]
            # the records and the fields: one 16-byte non-temporal load per input slot, and no other vector load
            nt = [i for i in loads if i.startswith("global_load_dwordx4") and i.rstrip().endswith(" nt")]
            assert len(nt) == nin and loads == nt, (name, loads)
            stores = [i for i in body if re.match(r"^(global|flat|buffer)_store", i)]
            assert len(stores) == 1 and stores[0].startswith("global_store_dwordx4"), (name, stores)
            # the program's words come through the scalar cache: a scalar load inside the interpreter's loop, i.e. behind
            # the record loads
            last_nt = max(k for k, i in enumerate(body) if i in nt)
            assert any(i.startswith("s_load_dwordx2") for i in body[last_nt:]), name
            # the stack below its top and the locals: 16 bytes per lane and access, no barrier (no lane reads another's)
            assert any(i.startswith("ds_read_b128") for i in body) and any(i.startswith("ds_write_b128") for i in body), name
            assert not [i for i in body if re.match(r"^ds_(read|write)_b(8|16|32|64|96)\b", i) or i.startswith("s_barrier")], name
            # division and square root are the correctly rounded expansions
            assert any(i.startswith("v_div_fixup_f32") for i in body) and any(i.startswith("v_div_fmas_f32") for i in body), name
    assert seen == 2, seen
