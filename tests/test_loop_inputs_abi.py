"""CPU: the ABI of cgmres_hip_closed_loop_device_ex — the ctypes mirror of struct cgmres_hip_loop_inputs has the C
layout, the entry point is exported and refuses a null handle, and the header declares the struct under ABI version 3
(model plugins built against version 2 implement the old closed_loop virtual and must be refused)."""
import ctypes
import os
import re

import cgmres_cpp_amd as cg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_loop_inputs_struct_layout():
    # int32 x4, then three pointers: 16 + 3 * 8
    assert ctypes.sizeof(cg.LoopInputs) == 40
    offs = [getattr(cg.LoopInputs, name).offset for name, _ in cg.LoopInputs._fields_]
    assert [name for name, _ in cg.LoopInputs._fields_] == [
        "struct_size", "ptau_per_instance", "dist_per_instance", "meas_per_instance", "ptau_seq_dev", "dist_seq_dev",
        "meas_seq_dev"]
    assert offs == [0, 4, 8, 12, 16, 24, 32]


def test_entry_point_refuses_a_null_handle():
    if not os.path.exists(cg.lib_path()):
        from cgmres_cpp_amd import build
        build.build()
    lib = cg.load()
    li = cg.LoopInputs(struct_size=ctypes.sizeof(cg.LoopInputs))
    assert lib.cgmres_hip_closed_loop_device_ex(None, None, None, 3, ctypes.byref(li)) == -1
    assert lib.cgmres_hip_closed_loop_device_ex(None, None, None, 3, None) == -1
    assert lib.cgmres_hip_last_error()


def test_header_declares_the_struct_and_abi_3():
    hdr = open(os.path.join(ROOT, "include", "cgmres_hip.h")).read()
    assert "#define CGMRES_HIP_ABI_VERSION 3" in hdr and cg.ABI_VERSION == 3
    m = re.search(r"typedef struct cgmres_hip_loop_inputs \{(.*?)\} cgmres_hip_loop_inputs;", hdr, flags=re.S)
    assert m, "struct cgmres_hip_loop_inputs not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(int32_t|const void\*)\s+(\w+);", body)
    assert fields == [("int32_t", "struct_size"), ("int32_t", "ptau_per_instance"), ("int32_t", "dist_per_instance"),
                      ("int32_t", "meas_per_instance"), ("const void*", "ptau_seq_dev"), ("const void*", "dist_seq_dev"),
                      ("const void*", "meas_seq_dev")]
    assert "cgmres_hip_closed_loop_device_ex(cgmres_hip_handle h, void* x_dev, void* u_dev, int32_t n_ticks," in hdr
    assert "main.cpp:63-73" in hdr
