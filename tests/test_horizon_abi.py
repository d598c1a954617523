"""CPU: the ABI of cgmres_hip_horizon_device — the header declares struct cgmres_hip_horizon_out with exactly the fields
the ctypes mirror has, in the C layout; the entry point is declared, listed and exported, and refuses a null handle.  The
ABI version stays 3: the plugin contract is unchanged, the plugin's horizon symbol is optional."""
import ctypes
import os
import re

import cgmres_cpp_amd as cg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["struct_size", "reserved", "xtau_dev", "ltau_dev", "F_dev", "fnorm_dev"]


def _header():
    return open(os.path.join(ROOT, "include", "cgmres_hip.h")).read()


def test_header_declares_the_struct():
    hdr = _header()
    assert "#define CGMRES_HIP_ABI_VERSION 3" in hdr and cg.ABI_VERSION == 3
    m = re.search(r"typedef struct cgmres_hip_horizon_out \{(.*?)\} cgmres_hip_horizon_out;", hdr, flags=re.S)
    assert m, "struct cgmres_hip_horizon_out not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"(int32_t|void\*)\s+(\w+);", body) == [("int32_t", "struct_size"), ("int32_t", "reserved"),
                                                               ("void*", "xtau_dev"), ("void*", "ltau_dev"),
                                                               ("void*", "F_dev"), ("void*", "fnorm_dev")]
    assert [s.strip() for s in body.split(";") if s.strip()] == [
        "int32_t struct_size", "int32_t reserved", "void* xtau_dev", "void* ltau_dev", "void* F_dev", "void* fnorm_dev"]
    assert ("int cgmres_hip_horizon_device(cgmres_hip_handle h, const void* x_dev, const cgmres_hip_horizon_out* out);"
            in hdr)
    assert "cgmres.hpp:113-162" in hdr


def test_ctypes_mirror_has_the_c_layout():
    assert [name for name, _ in cg.Horizon._fields_] == FIELDS
    assert [getattr(cg.Horizon, name).offset for name in FIELDS] == [0, 4, 8, 16, 24, 32]
    # int32 x2, then four pointers: the last one ends at 32 + 8.  (The issue that asked for this call wrote 48 beside
    # these offsets; the six fields it lists, and the offsets it lists, give 40 under the C layout rules, and 40 is what
    # the library compares struct_size with: tests/test_gpu_horizon.py::test_refusals sends 48 and is refused.)
    assert ctypes.sizeof(cg.Horizon) == 40


def test_symbol_is_declared_listed_and_exported():
    assert "cgmres_hip_horizon_device" in cg.SYMBOLS
    if not os.path.exists(cg.lib_path()):
        from cgmres_cpp_amd import build
        build.build()
    assert hasattr(cg.load(), "cgmres_hip_horizon_device")


def test_entry_point_refuses_a_null_handle():
    if not os.path.exists(cg.lib_path()):
        from cgmres_cpp_amd import build
        build.build()
    lib = cg.load()
    out = cg.Horizon(struct_size=ctypes.sizeof(cg.Horizon))
    assert lib.cgmres_hip_horizon_device(None, None, ctypes.byref(out)) == -1
    assert b"null handle" in lib.cgmres_hip_last_error()
    assert lib.cgmres_hip_horizon_device(None, None, None) == -1


def test_python_surface():
    for name in ("horizon_device", "horizon", "opt_error"):
        assert callable(getattr(cg.CgmresBatch, name))
