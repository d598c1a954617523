"""CPU: the launch cut of a recorded closed loop (cgmres_hip_record_plan) and the layout of the two new structs.

The rule, stated here independently of the library: each stride window is cut exactly as a fresh call of `stride` ticks is
cut today (CGMRES_HIP_TICKS_PER_LAUNCH, ..., then the remainder), and the tail behind the last record as a fresh call of
the remaining ticks."""
import ctypes
import os
import shutil
import subprocess

import pytest

import cgmres_cpp_amd as cg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSE = 10


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(cg.lib_path()):
        from cgmres_cpp_amd import build
        build.build()
    return cg.load()


def fresh_cut(n):
    """How a call of n ticks is cut today (ctx_wg.hip.h before the record existed)."""
    return [min(FUSE, n - i) for i in range(0, n, FUSE)]


def plan(lib, n_ticks, stride, cap=64):
    n_rec, n_l = ctypes.c_int32(-1), ctypes.c_int32(-1)
    sizes = (ctypes.c_int32 * cap)()
    rc = lib.cgmres_hip_record_plan(n_ticks, stride, ctypes.byref(n_rec), sizes, cap, ctypes.byref(n_l))
    return rc, n_rec.value, list(sizes[:max(0, n_l.value)])


def test_cut_for_every_length_and_stride(lib):
    assert cg.TICKS_PER_LAUNCH == FUSE
    for n in range(0, 46):
        for stride in range(1, 28):
            rc, n_rec, sizes = plan(lib, n, stride)
            assert rc == 0, (n, stride)
            assert sum(sizes) == n and all(1 <= s <= FUSE for s in sizes), (n, stride, sizes)
            assert n_rec == n // stride
            ends, k = set(), 0
            for s in sizes:
                k += s
                ends.add(k - 1)  # the last tick of a launch
            for tick in range(n):
                if (tick + 1) % stride == 0:
                    assert tick in ends, (n, stride, tick, sizes)
            want = []
            for _ in range(n // stride):
                want += fresh_cut(stride)
            want += fresh_cut(n % stride)
            assert sizes == want, (n, stride, sizes, want)
            if stride % FUSE == 0:
                assert sizes == fresh_cut(n), (n, stride, sizes)
            assert cg.record_plan(n, stride) == (n_rec, sizes)


def test_counts_without_a_buffer_and_refusals(lib):
    n_rec, n_l = ctypes.c_int32(), ctypes.c_int32()
    assert lib.cgmres_hip_record_plan(53, 4, ctypes.byref(n_rec), None, 0, ctypes.byref(n_l)) == 0
    assert (n_rec.value, n_l.value) == (13, 14)
    assert lib.cgmres_hip_record_plan(53, 4, None, None, 0, None) == 0
    rc, _, _ = plan(lib, 53, 4, cap=13)
    assert rc == -1 and b"cap" in lib.cgmres_hip_last_error()
    assert plan(lib, 53, 4, cap=14)[0] == 0
    rc, _, _ = plan(lib, 5, 0)
    assert rc == -1 and b"stride" in lib.cgmres_hip_last_error()
    rc, _, _ = plan(lib, -1, 3)
    assert rc == -1 and b"n_ticks" in lib.cgmres_hip_last_error()


PROBE = r"""
#include <cstddef>
#include <cstdio>
#include "cgmres_hip.h"
#define F(S, f) printf(#S "." #f " %zu\n", offsetof(S, f))
int main() {
  printf("cgmres_hip_ensemble_out %zu\n", sizeof(cgmres_hip_ensemble_out));
  F(cgmres_hip_ensemble_out, struct_size); F(cgmres_hip_ensemble_out, reserved); F(cgmres_hip_ensemble_out, centre_dev);
  F(cgmres_hip_ensemble_out, moments_dev); F(cgmres_hip_ensemble_out, counts_dev);
  printf("cgmres_hip_loop_record %zu\n", sizeof(cgmres_hip_loop_record));
  F(cgmres_hip_loop_record, struct_size); F(cgmres_hip_loop_record, stride); F(cgmres_hip_loop_record, reserved);
  F(cgmres_hip_loop_record, x_log_dev); F(cgmres_hip_loop_record, u_log_dev); F(cgmres_hip_loop_record, n_ax_log_dev);
  F(cgmres_hip_loop_record, reason_log_dev); F(cgmres_hip_loop_record, t_host); F(cgmres_hip_loop_record, centre_dev);
  F(cgmres_hip_loop_record, moments_log_dev); F(cgmres_hip_loop_record, counts_log_dev);
  printf("CGMRES_HIP_RECORD_BLOCK %d\n", CGMRES_HIP_RECORD_BLOCK);
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text(PROBE)
    subprocess.run(["g++", "-std=c++17", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    c_side = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    py_side = {"CGMRES_HIP_RECORD_BLOCK": str(cg.RECORD_BLOCK)}
    for name, S in (("cgmres_hip_ensemble_out", cg.EnsembleOut), ("cgmres_hip_loop_record", cg.LoopRecord)):
        py_side[name] = str(ctypes.sizeof(S))
        for f, _ in S._fields_:
            py_side[f"{name}.{f}"] = str(getattr(S, f).offset)
    assert py_side == c_side
    assert ctypes.sizeof(cg.EnsembleOut) == 32 and ctypes.sizeof(cg.LoopRecord) == 80


def test_entry_points_refuse_a_null_handle(lib):
    out = cg.EnsembleOut(struct_size=ctypes.sizeof(cg.EnsembleOut))
    assert lib.cgmres_hip_ensemble_device(None, None, None, ctypes.byref(out)) == -1
    rec = cg.LoopRecord(struct_size=ctypes.sizeof(cg.LoopRecord), stride=1)
    assert lib.cgmres_hip_closed_loop_device_rec(None, None, None, 3, None, ctypes.byref(rec)) == -1
    assert lib.cgmres_hip_last_error()
