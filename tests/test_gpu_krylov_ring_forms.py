"""GPU parity of the STREAMING form of the Krylov row walk (csrc/wg_gmres.hip.h: ring_request + ring_walk<true> over two
row buffers from row 0, in the Gram-Schmidt rounds and in x += V y, followed by drain_stream) at sizes of a few
milliseconds.  The rest of the suite reaches this form only at workload size (fp32, N = 100, k_max = 20, B = 8192); the
compact ring of the row-Newton kernel is pinned by test_gpu_gs_ring.py.

    pendulum fp64 dv = 20, variant 2, k_max 13, 14   the full-plan kernel leaves its twelve straight-line cases beyond
                                                     KRING = 12 rows: the streaming walk and its drain inside a kernel
                                                     that also carries the register ring; basis lengths 0 ... 13, i.e.
                                                     tails of none and of one round
    pendulum fp64 dv = 20, variant 3, k_max 1, 2, 3  the lean kernel: a request that clamps both buffers to the single
                                                     row, the tail alone, the first full trip
    two-mass system fp64, variant 3, k_max 3         dv = 20 and dv = 27.  At dv = 20 a row is 120 elements (80 bytes per
                                                     lane) and the planner grants the short-vector lean kernel, which
                                                     keeps v_k in registers; the nearest horizon whose lean kernel
                                                     streams v_k back from its row (VK_IN_REGS false: more than 160
                                                     elements, the long-vector kernel), so that the walk runs to row k
                                                     inclusive, is dv = 27 (162 elements).  Both are run.

Every case: B = 20 (one full workgroup and a last one with 4 of 16 rows valid), tol = 0 and 1e-6, 12 device-resident
ticks from the scenario's own start (a launch fuses at most 10: one launch boundary) against the free-running oracle:
x and u within 1e-7, the last tick's Arnoldi counts and exit reasons equal — helper and bounds of
test_gpu_gs_ring.py."""
import numpy as np
import pytest

import cgmres_cpp_amd as cg
from gpu_helpers import _oracle_free_run

pytestmark = pytest.mark.gpu

B = 20
TICKS = 12  # as in test_gpu_gs_ring.py: one launch fuses at most 10 ticks, the 11th starts a second launch
PENDULUM, MSD = 0, 1
CASES = [(PENDULUM, 20, 2, 13), (PENDULUM, 20, 2, 14),
         (PENDULUM, 20, 3, 1), (PENDULUM, 20, 3, 2), (PENDULUM, 20, 3, 3),
         (MSD, 20, 3, 3), (MSD, 27, 3, 3)]


@pytest.mark.parametrize("model,dv,variant,km", CASES)
def test_streaming_walk_free_running_vs_oracle(orc, model, dv, variant, km):
    name = ("pendulum", "msd")[model]
    x0, u0, p = orc.batch_scenario(model, B)
    for tol in (0.0, 1e-6):
        xo, uo, ko, ro = _oracle_free_run(orc, dv, km, tol, x0, u0, p, TICKS, model)
        c = cg.CgmresBatch(name, batch=B, dv=dv, k_max=km, tol=tol, variant=variant)
        vn = c.variant_name
        if variant == 2:
            assert vn.startswith("wg") and not vn.startswith("wg-lean") and "row-newton" not in vn, (dv, km, vn)
        else:
            assert vn.startswith("wg-lean"), (dv, km, vn)
        c.set_ptau_repeat(p), c.init_u0(u0), c.init_u0_newton(u0, x0, p, 10)
        xd, ud = c.device_buffer(x0.shape).upload(x0), c.device_buffer(u0.shape)
        c.closed_loop_device(xd, ud, TICKS)
        c.synchronize()
        x, u = xd.download(), ud.download()
        n_ax, reason = c.get_status()
        c.close()
        print(f"{name} {vn} dv {dv} k_max {km} tol {tol}: |du| {np.max(np.abs(u - uo)):.3e} |dx| {np.max(np.abs(x - xo)):.3e}")
        assert np.array_equal(n_ax, ko[:, -1]) and np.array_equal(reason, ro[:, -1]), (name, dv, km, tol, n_ax, ko[:, -1])
        assert np.max(np.abs(u - uo)) <= 1e-7 and np.max(np.abs(x - xo)) <= 1e-7, (name, dv, km, tol)
