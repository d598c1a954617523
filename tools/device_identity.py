#!/usr/bin/env python3
"""Is the device code of this tree that of a parent commit?  (the procedure of profiles/*_identity.md)

    python tools/device_identity.py <parent> [--work DIR] [--out FILE.md]

The parent's cgmres_cpp_amd/ and include/ are exported with git into a temporary directory (--work DIR: there, and
kept: a parent already compiled there is not compiled again).  The translation units of those documents (every .hip of
csrc/, inst_pendulum_f64.hip -DCGM_STAMPS, the user model Shape431 with and without -DCGM_DEBUG_LDS, the operator
ConvDiffRowOp) are compiled on both sides with build.py's CFLAGS plus --cuda-device-only -S, the __hip_cuid_ lines (a
hash of the unit's path) are dropped, and each unit is classified as
    identical
    identical up to commutative source order   (commutative_swap)
    different                                  (the first differing lines are printed)
The table goes to stdout, or to --out.  Exit status 1 if any unit is different.
"""
import argparse, hashlib, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# Two-source commutative VALU operations; the operands are plain registers, so no source carries a modifier
# (neg, abs) and none follows (DPP, SDWA, clamp, omod).
COMMUTATIVE = re.compile(r"v_(add|mul|min|max|and|or|xor)_[fiub]\d+(_e32|_e64)?")
REGISTER = re.compile(r"[vs](\d+|\[\d+:\d+\])")


def commutative_swap(a, b):
    """Lines a and b are the same commutative VALU instruction with the same destination and the two register
    sources exchanged."""
    pa, pb = a.split(None, 1), b.split(None, 1)
    if len(pa) != 2 or len(pb) != 2 or pa[0] != pb[0] or not COMMUTATIVE.fullmatch(pa[0]):
        return False
    oa, ob = [s.strip() for s in pa[1].split(",")], [s.strip() for s in pb[1].split(",")]
    if len(oa) != 3 or len(ob) != 3 or not all(REGISTER.fullmatch(s) for s in oa + ob):
        return False
    return oa[0] == ob[0] and oa[1] == ob[2] and oa[2] == ob[1] and oa[1] != oa[2]


def classify(a, b):
    """(class, detail) of two lists of lines: ("identical", None), ("commutative", {mnemonic: count}) or
    ("different", [first differing (line number, a, b) ...])."""
    if a == b:
        return "identical", None
    pairs = [(n + 1, x, y) for n, (x, y) in enumerate(zip(a, b)) if x != y]
    if len(a) == len(b) and all(commutative_swap(x, y) for _, x, y in pairs):
        count = {}
        for _, x, _ in pairs:
            count[x.split()[0]] = count.get(x.split()[0], 0) + 1
        return "commutative", count
    if len(a) != len(b):
        pairs.append((min(len(a), len(b)) + 1, f"<{len(a)} lines>", f"<{len(b)} lines>"))
    return "different", sorted(pairs)[:5]


def units(side_root, work):
    """(label, source, flags) of the units, the generated ones written under `work`."""
    from cgmres_cpp_amd import plugin
    csrc = os.path.join(side_root, "cgmres_cpp_amd", "csrc")
    um = os.path.join(ROOT, "tests", "user_models")
    out = [(f"`{f}`", os.path.join(csrc, f), []) for f in sorted(os.listdir(csrc)) if f.endswith(".hip")]
    out.append(("`inst_pendulum_f64.hip -DCGM_STAMPS`", os.path.join(csrc, "inst_pendulum_f64.hip"), ["-DCGM_STAMPS"]))
    gen = [("user model Shape431", "shape_models.hpp", "user_model.hip.h", "CGMRES_HIP_DEFINE_PLUGIN", "Shape431", []),
           ("user model Shape431 -DCGM_DEBUG_LDS", "shape_models.hpp", "user_model.hip.h", "CGMRES_HIP_DEFINE_PLUGIN",
            "Shape431", ["-DCGM_DEBUG_LDS"]),
           ("operator ConvDiffRowOp (gmres_row_ops.hpp)", "gmres_row_ops.hpp", "user_operator.hip.h",
            "CGMRES_HIP_DEFINE_OPERATOR", "ConvDiffRowOp", [])]
    for label, hpp, glue, macro, cls, flags in gen:
        src = os.path.join(work, cls + ".hip")  # (the same text and name on both sides)
        with open(src, "w") as f:
            f.write(plugin.TEMPLATE.format(origin="tests/user_models/" + hpp, header=hpp, glue=glue, macro=macro, cls=cls))
        out.append((f"`{label}`", src, flags + ["-iquote", um, "-iquote", csrc]))
    return out


def assembly(side_root, work, reuse):
    """The units of one side compiled to <work>/<n>.s; returns [(label, lines)]."""
    from cgmres_cpp_amd import build
    os.makedirs(work, exist_ok=True)
    us = units(side_root, work)

    def one(n):
        _, src, flags = us[n]
        out = os.path.join(work, f"{n}.s")
        if not (reuse and os.path.exists(out)):
            cmd = [build.HIPCC] + build.CFLAGS + flags + ["-I" + os.path.join(side_root, "include"),
                                                          "--cuda-device-only", "-S", "-o", out + ".tmp", src]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(" ".join(cmd) + "\n" + r.stderr[-4000:])
            sys.stderr.write(r.stderr)
            os.replace(out + ".tmp", out)
        with open(out) as f:
            return [l.rstrip("\n") for l in f if "__hip_cuid_" not in l]

    with ThreadPoolExecutor(min(16, len(os.sched_getaffinity(0)))) as ex:
        return [(us[n][0], lines) for n, lines in enumerate(ex.map(one, range(len(us))))]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("--work")
    ap.add_argument("--out")
    a = ap.parse_args()
    from cgmres_cpp_amd import build
    tmp = None if a.work else tempfile.TemporaryDirectory()
    work = os.path.abspath(a.work or tmp.name)
    git = lambda *c: subprocess.run(["git", "-C", ROOT] + list(c), check=True, capture_output=True, text=True).stdout
    commit = git("rev-parse", "--short", a.parent).strip()
    proot = os.path.join(work, commit)
    if not os.path.isdir(proot):
        os.makedirs(proot)
        tar = subprocess.Popen(["git", "-C", ROOT, "archive", commit, "cgmres_cpp_amd", "include"], stdout=subprocess.PIPE)
        subprocess.run(["tar", "-x", "-C", proot], stdin=tar.stdout, check=True)
        if tar.wait() != 0:
            raise RuntimeError("git archive failed")
    old = assembly(proot, os.path.join(work, commit + "_s"), reuse=True)
    new = assembly(ROOT, os.path.join(work, "tree_s"), reuse=False)
    sha = lambda lines: hashlib.sha256("".join(l + "\n" for l in lines).encode()).hexdigest()
    version = subprocess.run([build.HIPCC, "--version"], capture_output=True, text=True).stdout.splitlines()[:2]
    doc = [f"Parent: commit {commit}.  `{' '.join(build.CFLAGS)}` plus `--cuda-device-only -S`.", "", "```"] + version + \
          ["```", "", "| translation unit | lines | sha256, parent | sha256, this change | |", "|---|---|---|---|---|"]
    notes, bad = [], 0
    parent_units = dict(old)
    for label, lb in new:  # (by label: a unit this change adds has no parent)
        if label not in parent_units:
            doc.append(f"| {label} | {len(lb)} | — | `{sha(lb)}` | new in this change |")
            continue
        la = parent_units[label]
        cls, detail = classify(la, lb)
        word = {"identical": "identical", "commutative": "identical up to commutative source order",
                "different": "DIFFERENT"}[cls]
        doc.append(f"| {label} | {len(lb)} | `{sha(la)}` | `{sha(lb)}` | {word} |")
        if cls == "commutative":
            notes.append(f"- {label}: sources exchanged in " + ", ".join(f"{n} `{m}`" for m, n in sorted(detail.items())))
        if cls == "different":
            bad += 1
            notes += [f"- {label}: first differing lines"] + [f"  - {n}: `{x.strip()}` / `{y.strip()}`" for n, x, y in detail]
    text = "\n".join(doc + [""] + notes) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
