"""The independent reference of the horizon tests (tests/horizon_ref.cpp), built with g++ into a directory the caller
names and driven over ctypes.  A plain module: nothing from conftest."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)


class HorizonRef:
    """ref(model, dtype, dv, Tf, alpha, t, x, U, ptau) -> (xtau [dv+1, dim_x], ltau [dv+1, dim_x], F [dim_u*dv]) of one
    instance, computed in dtype ("f64" | "f32"), returned as float64.  header / cls: a user model instead of the three
    oracle models (model and dtype are then ignored: fp64)."""

    def __init__(self, out_dir, header=None, cls=None):
        so = os.path.join(str(out_dir), f"libhorizon_ref_{cls or 'oracle'}.so")
        cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", ROOT]
        if header:
            cmd += [f'-DMODEL_HEADER="{header}"', f"-DMODEL_CLASS={cls}"]
        subprocess.run(cmd + [os.path.join(ROOT, "tests", "horizon_ref.cpp"), "-o", so], check=True)
        self._lib = C.CDLL(so)
        self._lib.horizon_ref.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double] + [_dp] * 6

    def __call__(self, model, dtype, dv, Tf, alpha, t, x, U, ptau):
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        U = np.ascontiguousarray(U, dtype=np.float64).ravel()
        ptau = np.ascontiguousarray(ptau, dtype=np.float64).ravel()
        ptau = ptau if ptau.size else np.zeros(1)
        nx = x.size
        xtau, ltau, F = np.empty((dv + 1, nx)), np.empty((dv + 1, nx)), np.empty(U.size)
        rc = self._lib.horizon_ref(int(model), 1 if dtype == "f32" else 0, int(dv), float(Tf), float(alpha), float(t),
                                   *[a.ctypes.data_as(_dp) for a in (x, U, ptau, xtau, ltau, F)])
        assert rc == 0, f"horizon_ref: unknown model {model}"
        return xtau, ltau, F

    def batch(self, model, dtype, dv, Tf, alpha, t, x, U, ptau):
        """The same for [B, ...] arrays; ptau [B, dim_p*(dv+1)] (or [B, 0])."""
        out = [self(model, dtype, dv, Tf, alpha, t, x[b], U[b], ptau[b]) for b in range(len(x))]
        return tuple(np.array(a) for a in zip(*out))
