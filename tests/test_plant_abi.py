"""CPU: the ABI of the plant of a closed loop — the three entry points are declared, listed and exported; the ctypes mirror
of struct cgmres_hip_loop_plant has the C layout; cgmres_hip_plant_info gives the constants the state equations read, in
the order of theta; the numpy plant of the GPU tests (tests/plant_harness.py) at nominal theta IS the oracle's plant; and
what the entry points refuse without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import cgmres_cpp_amd as cg
import plant_harness as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cgmres_hip_plant_info", "cgmres_hip_plant_step_device", "cgmres_hip_closed_loop_device_plant")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(cg.lib_path()):
        from cgmres_cpp_amd import build
        build.build()
    return cg.load()


def test_header_exports_and_binding_agree(lib):
    hdr = open(os.path.join(ROOT, "include", "cgmres_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in cg.SYMBOLS and hasattr(lib, name), name
    assert "#define CGMRES_HIP_ABI_VERSION 3" in hdr and cg.ABI_VERSION == 3
    assert re.search(r"enum \{ CGMRES_HIP_PLANT_EULER = 0, CGMRES_HIP_PLANT_RK4 = 1 \};", code)
    assert (cg.PLANT_EULER, cg.PLANT_RK4) == (0, 1) and cg.PLANT_INTEGRATORS == {"euler": 0, "rk4": 1}


def test_loop_plant_struct_layout():
    hdr = open(os.path.join(ROOT, "include", "cgmres_hip.h")).read()
    m = re.search(r"typedef struct cgmres_hip_loop_plant \{(.*?)\} cgmres_hip_loop_plant;", hdr, flags=re.S)
    assert m, "struct cgmres_hip_loop_plant not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(int32_t|const void\*)\s+(\w+)(\[2\])?;", body)
    assert fields == [("int32_t", "struct_size", ""), ("int32_t", "integrator", ""), ("int32_t", "substeps", ""),
                      ("int32_t", "theta_per_instance", ""), ("const void*", "theta_dev", ""), ("int32_t", "reserved", "[2]")]
    # int32 x4, a pointer, int32 x2
    assert ctypes.sizeof(cg.LoopPlant) == 32
    assert [name for name, _ in cg.LoopPlant._fields_] == [f[1] for f in fields]
    assert [getattr(cg.LoopPlant, name).offset for name, _ in cg.LoopPlant._fields_] == [0, 4, 8, 12, 16, 24]


def test_plant_info_tables(lib):
    pend, msd, semi = cg.plant_info("pendulum"), cg.plant_info("msd"), cg.plant_info("semiactive")
    assert pend["n_theta"] == 7 and msd["n_theta"] == 6 and semi["n_theta"] == 2
    # As, Bs, A52, C22, A32a, A32, A32b of arm_type_inverted_pendulum/model.hpp
    assert np.array_equal(pend["nominal"], [6.25, 15.6, 39.1111, 0.0407448, 5.65635, 0.905016, 14.1183])
    assert np.array_equal(msd["nominal"], np.ones(6))     # m1, m2, d1, d2, k1, k2
    assert np.array_equal(semi["nominal"], [-1.0, -1.0])  # a, b
    for m in (ph.PENDULUM, ph.MSD, ph.SEMIACTIVE):
        assert np.array_equal(cg.plant_info(m)["nominal"], ph.NOMINAL[m])
    n = ctypes.c_int32(-1)
    assert lib.cgmres_hip_plant_info(17, ctypes.byref(n), None, 0) == -1 and b"unknown model_id 17" in lib.cgmres_hip_last_error()
    nom = (ctypes.c_double * 7)()
    assert lib.cgmres_hip_plant_info(cg.PENDULUM, ctypes.byref(n), nom, 6) == -1 and b"cap = 6" in lib.cgmres_hip_last_error()
    assert lib.cgmres_hip_plant_info(cg.PENDULUM, None, nom, 7) == 0 and nom[6] == 14.1183
    assert lib.cgmres_hip_plant_info(cg.MSD, ctypes.byref(n), None, 0) == 0 and n.value == 6


@pytest.mark.parametrize("model", [0, 1, 2])
def test_numpy_plant_at_nominal_theta_is_the_oracle_plant(orc, model):
    nx, nu = ph.DIMS[model]
    rng = np.random.default_rng(3)
    x, u = rng.uniform(-4, 4, (40, nx)), rng.uniform(-3, 3, (40, nu))
    r = orc.Controller(model, 50, 10)
    f = ph.rhs(model, x, u, np.tile(ph.NOMINAL[model], (40, 1)))
    worst = max(float(np.max(np.abs(f[i] - r.plant(x[i], u[i])))) for i in range(40))
    print(f"max |numpy dxdt - oracle plant| = {worst}")
    assert worst == 0.0
    # one Euler step of dt is the plant statement of the oracle's closed loop (oracle/orc.py: closed_loop)
    step = ph.plant(model, x, u, np.tile(ph.NOMINAL[model], (40, 1)), "euler", 1, r.dt)
    assert all(np.array_equal(step[i], x[i] + r.plant(x[i], u[i]) * r.dt) for i in range(40))


def test_numpy_plant_sees_theta_substeps_and_integrator():
    """The figures the loop tests lean on: RK4/4 against Euler/1 and the theta draw against nominal both move one tick's
    state by far more than the loop bound of 1e-9 scaled to a tick."""
    for model in (0, 1, 2):
        nx, nu = ph.DIMS[model]
        rng = np.random.default_rng(5)
        x, u = rng.uniform(-4, 4, (83, nx)), rng.uniform(-3, 3, (83, nu))
        nom, th = np.tile(ph.NOMINAL[model], (83, 1)), ph.theta_draw(model, 83)
        a = ph.plant(model, x, u, nom, "euler", 1, 1e-3)
        assert np.max(np.abs(ph.plant(model, x, u, nom, "rk4", 4, 1e-3) - a)) > 1e-7
        assert np.max(np.abs(ph.plant(model, x, u, nom, "euler", 4, 1e-3) - a)) > 1e-7
        assert np.max(np.abs(ph.plant(model, x, u, th, "euler", 1, 1e-3) - a)) > 1e-5


def test_refusals_that_need_no_device(lib):
    lp = cg.LoopPlant(struct_size=ctypes.sizeof(cg.LoopPlant), integrator=cg.PLANT_RK4, substeps=4)
    li = cg.LoopInputs(struct_size=ctypes.sizeof(cg.LoopInputs))
    assert lib.cgmres_hip_plant_step_device(None, None, None, ctypes.byref(lp)) == -1
    assert b"null handle" in lib.cgmres_hip_last_error()
    assert lib.cgmres_hip_closed_loop_device_plant(None, None, None, 3, ctypes.byref(li), None, ctypes.byref(lp)) == -1
    assert b"null handle" in lib.cgmres_hip_last_error()
    assert lib.cgmres_hip_closed_loop_device_plant(None, None, None, 3, None, None, None) == -1
    p = cg.Plant()
    assert (p.integrator, p.substeps, p.theta) == ("rk4", 4, None)
