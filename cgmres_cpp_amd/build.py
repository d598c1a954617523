"""Builds libcgmres_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python -m cgmres_cpp_amd.build [--force]

Every .hip file under csrc/ is one translation unit (the kernel instantiations are split per model and
scalar type so they compile in parallel); objects go to csrc/_obj/, the library to lib/.

compile() is the one compile step of the project: the library's objects, the model and operator plugins
(plugin.py), the planner probes of the tests and the diagnostic builds under tools/ all go through it.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OBJ_DIR = os.path.join(CSRC, "_obj")
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libcgmres_hip.so")
INCLUDE = os.path.join(ROOT, "include")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CFLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function"]
LDFLAGS = ["--offload-arch=gfx950", "-shared", "-fPIC", "-fno-gpu-rdc"]


def sources(csrc=CSRC):
    srcs = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hip"))
    hdrs = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h"))
    return srcs, hdrs + [os.path.join(os.path.dirname(os.path.dirname(csrc)), "include", "cgmres_hip.h")]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(not os.path.exists(d) or os.path.getmtime(d) > t for d in deps)


def up_to_date():
    srcs, hdrs = sources()
    return not _stale(LIB_PATH, srcs + hdrs)


def read_deps(out):
    """The files `out` was compiled from, as its record <out>.d names them (absolute paths), or None without a record.
    The record holds one name per line: relative to the repository root for a file inside it, so that a tree copied
    to another place with its artefacts still finds its own headers there, absolute for any other file."""
    try:
        with open(out + ".d") as f:
            return [os.path.join(ROOT, n) for n in f.read().splitlines() if n]
    except OSError:
        return None


def record_name(path):
    """What a record calls `path`: relative to the repository root inside it, its absolute path elsewhere."""
    path, root = os.path.realpath(path), os.path.realpath(ROOT) + os.sep
    return path[len(root):] if path.startswith(root) else path


def _record_deps(out, rule):
    """Rewrites the make rule the compiler left in the file `rule` (`out: dep dep \\` ...) as the record <out>.d that
    read_deps() reads, and puts it in place in one step (two processes may be building the same artefact)."""
    with open(rule) as f:
        body = f.read().replace("\\\n", " ").split(": ", 1)[1]
    # (make's escapes: a blank inside a name is written `\ `, a `#` as `\#`, a `$` as `$$`)
    names = [re.sub(r"\\([ #])", r"\1", n).replace("$$", "$") for n in re.findall(r"(?:\\.|\S)+", body)]
    with open(rule, "w") as f:
        f.write("".join(record_name(n) + "\n" for n in names))
    os.replace(rule, out + ".d")


def needs_compile(out, src):
    """The staleness rule of compile(): `out` is kept when it is not older than `src` or any file its record names;
    a missing record, or a recorded file that no longer exists, makes it stale."""
    deps = read_deps(out)
    return deps is None or _stale(out, [src] + deps)


def compile(out, src, flags=(), link_only=False, force=False, verbose=False):
    """hipcc with CFLAGS and `flags` (the caller's -c or -shared among them) of `src` into `out`, unless `out` is up to
    date (needs_compile); link_only: `src` is the list of objects of a shared library.  Returns `out`."""
    if link_only:
        cmd, stale = [HIPCC] + LDFLAGS + list(flags) + ["-o", out] + list(src), _stale(out, src)
    else:
        rule = f"{out}.d.{os.getpid()}"
        cmd = [HIPCC] + CFLAGS + list(flags) + ["-MMD", "-MF", rule, "-o", out, src]
        stale = needs_compile(out, src)
    if not force and not stale:
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        # (the first error names the cause; the tail names the command)
        err = r.stderr if len(r.stderr) <= 6000 else r.stderr[:3000] + "\n[...]\n" + r.stderr[-3000:]
        raise RuntimeError(f"hipcc failed for {os.path.basename(out)}:\n" + err)
    sys.stderr.write(r.stderr)
    if not link_only:
        _record_deps(out, rule)
    return out


def build(force=False, verbose=False, jobs=None, lib=LIB_PATH, obj_dir=OBJ_DIR, flags=(), csrc=CSRC):
    """The library: every .hip of `csrc` compiled with `flags` into `obj_dir` and linked into `lib`.  The defaults are
    the product build; a diagnostic build (tools/) names its own lib, obj_dir and flags."""
    if not force and lib == LIB_PATH and csrc == CSRC and up_to_date():
        return lib  # (also where the objects did not travel with the tree)
    srcs, _ = sources(csrc)
    jobs = jobs or min(len(srcs), max(1, len(os.sched_getaffinity(0))))
    with ThreadPoolExecutor(jobs) as ex:
        objs = list(ex.map(lambda s: compile(os.path.join(obj_dir, os.path.basename(s)[:-4] + ".o"), s,
                                             ["-c"] + list(flags), force=force, verbose=verbose), srcs))
    return compile(lib, objs, link_only=True, force=force, verbose=verbose)


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="-v" in sys.argv))
