"""The oracle's generic controller on a user model header (tests/user_models/user_oracle.cpp) as a plain module: build
the executable with g++, run one of its forms, parse what it prints.  Shared by tests/test_user_model_plugin.py,
tests/test_gpu_user_kernel_classes.py and tools/user_case_admission.py; nothing is imported from conftest."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "user_models", "user_oracle.cpp")
PLAIN, FAST = ("-ffp-contract=off",), ("-ffp-contract=fast", "-mfma")
# where __graft_entry__.build() leaves the plain-flavour executables of the shape models (beside the plugins)
PREBUILT_DIR = os.path.join(ROOT, "cgmres_cpp_amd", "lib", "plugins")


def prebuilt(cls):
    return os.path.join(PREBUILT_DIR, f"user_oracle_{cls}")


def build(header, cls, exe, flavour=PLAIN):
    """g++ build of user_oracle.cpp for class `cls` of `header` into `exe` (kept when it is newer than its sources)."""
    exe = str(exe)
    deps = [SRC, header, os.path.join(ROOT, "oracle", "cgmres_oracle.hpp"), os.path.join(ROOT, "oracle", "models.hpp")]
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
        return exe
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    rel = os.path.relpath(header, ROOT)
    subprocess.run(["g++", "-O2", "-std=c++17", *flavour, f"-I{ROOT}", f'-DMODEL_HEADER="{rel}"', f"-DMODEL_CLASS={cls}", SRC,
                    "-o", exe], check=True)
    return exe


def have_gxx():
    return shutil.which("g++") is not None


def _rows(exe, args):
    out = subprocess.run([str(exe)] + [a if isinstance(a, str) else repr(a) for a in args], check=True, capture_output=True,
                         text=True).stdout
    return np.array([[float(v) for v in l.split()] for l in out.strip().split("\n")]), out


def run(exe, nx, nu, B, ticks, dv, kmax, tol, with_state=False):
    """u [B, ticks, nu], x [B, ticks, nx], k [B, ticks]; with with_state also (t [B, ticks], U [B, ticks, L],
    dUdt [B, ticks, L]): the controller state each tick started from."""
    rows, _ = _rows(exe, [B, ticks, dv, kmax, float(tol)] + (["state"] if with_state else []))
    base = (rows[:, 3:3 + nu].reshape(B, ticks, nu), rows[:, 3 + nu:3 + nu + nx].reshape(B, ticks, nx),
            rows[:, 2].astype(int).reshape(B, ticks))
    if not with_state:
        return base
    L, o = nu * dv, 3 + nu + nx
    return base + ((rows[:, o].reshape(B, ticks), rows[:, o + 1:o + 1 + L].reshape(B, ticks, L),
                    rows[:, o + 1 + L:o + 1 + 2 * L].reshape(B, ticks, L)),)


def run_full(exe, nx, nu, B, ticks, dv, kmax, tol, forced_from=None):
    """The "full" form as a dict of arrays [B, ticks, ...]: k, u, x, t, U, d (the state the tick started from), reason,
    t1, U1, d1 (the state after it); and the text, which another build takes as `forced_from` (a file path)."""
    rows, text = _rows(exe, [B, ticks, dv, kmax, float(tol), "full"] + ([str(forced_from)] if forced_from else []))
    L, o = nu * dv, 3 + nu + nx
    assert rows.shape == (B * ticks, o + 3 + 4 * L), rows.shape
    cut = lambda a, b: rows[:, a:b].reshape(B, ticks, b - a)
    return dict(k=rows[:, 2].astype(int).reshape(B, ticks), u=cut(3, 3 + nu), x=cut(3 + nu, o), t=rows[:, o].reshape(B, ticks),
                U=cut(o + 1, o + 1 + L), d=cut(o + 1 + L, o + 1 + 2 * L), reason=rows[:, o + 1 + 2 * L].astype(int).reshape(B, ticks),
                t1=rows[:, o + 2 + 2 * L].reshape(B, ticks), U1=cut(o + 3 + 2 * L, o + 3 + 3 * L),
                d1=cut(o + 3 + 3 * L, o + 3 + 4 * L)), text


def run_hooks(exe, nx, nu, B, dv, kmax, tol):
    """The "hooks" form: dict of F, b, Ax, v [B, L], t (a float), U, d [B, L], x [B, nx]."""
    out = subprocess.run([str(exe), str(B), "1", str(dv), str(kmax), repr(float(tol)), "hooks"], check=True, capture_output=True,
                         text=True).stdout
    lines = [[float(v) for v in l.split()] for l in out.strip().split("\n")]
    L = nu * dv
    assert len(lines) == 6 * B
    r = {k: np.array([lines[6 * b + 1 + i] for b in range(B)]) for i, k in enumerate(("F", "b", "Ax", "v"))}
    st = np.array([lines[6 * b + 5] for b in range(B)])
    assert st.shape == (B, 1 + 2 * L + nx) and np.all(st[:, 0] == st[0, 0])
    r.update(t=float(st[0, 0]), U=st[:, 1:1 + L], d=st[:, 1 + L:1 + 2 * L], x=st[:, 1 + 2 * L:])
    return r


def scenario(B, nx, nu, np_):
    """x0, u0 guess and p of user_oracle.cpp's instances"""
    b = np.arange(B)[:, None]
    return (0.3 + 0.05 * b - 0.11 * np.arange(nx)[None, :], np.full((B, nu), 0.1),
            0.2 + 0.03 * b + 0.01 * np.arange(np_)[None, :])
