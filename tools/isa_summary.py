#!/usr/bin/env python3
"""ISA summary of every tick kernel instantiation (no GPU needed): registers, spills, scratch, and WHERE the scratch
traffic and AGPR copies sit — inside a loop block (the stage loops, the Gram-Schmidt rounds) or in straight-line code.

    python tools/isa_summary.py [--out profiles/r02_isa_summary.md] [pattern]
    python tools/isa_summary.py --operator tests/user_models/gmres_row_ops.hpp ConvDiffRowOp150
    python tools/isa_summary.py --blocks "PendulumDev<double>, double, 16, 10, false, 1, 1" [--csrc DIR] [--out FILE]

The second form summarises the two kernels of an OPERATOR plugin (csrc/user_operator.hip.h: gmres_wave_kernel,
gmres_op_kernel) for the struct named: per loop depth (1 = the Arnoldi loop, 2 = the Gram-Schmidt rounds and whatever
loops the operator brings) the instruction count and how many of them are ds_ (LDS), flat_ (an LDS or HBM access whose
address space the compiler could not prove: an operand that left LDS addressing), scratch_ and global_ accesses.

The third form lists ONE kernel (the first whose demangled name contains the substring) basic block by basic block, in
program order: loop depth, instruction count and how many of the instructions are v_accvgpr_* copies, v_readlane /
v_writelane, DPP moves, ds_* (LDS), global_* accesses and floating-point arithmetic with a literal-zero operand (an
operation the compiler could not fold: no fast-math).  --csrc points it at the sources of another checkout (the parent
of a change), so that two listings can be set side by side.

For every inst_*.hip translation unit: hipcc -S --cuda-device-only -Rpass-analysis=kernel-resource-usage, then per
kernel: VGPR / AGPR / SGPR, VGPR+SGPR spill counts, scratch bytes per lane (compiler remarks), the number of
scratch_load/scratch_store and v_accvgpr_read/write instructions in the whole kernel and inside blocks the compiler
marks as loops (`; %bb... Loop Header/ in Loop:` annotations), listed per loop with its instruction count."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cgmres_cpp_amd", "csrc")
TMP = os.environ.get("ISA_TMP", "/tmp/asm")


def compile_tu(src):
    os.makedirs(TMP, exist_ok=True)
    out = os.path.join(TMP, os.path.basename(src) + ".s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", out, src] + EXTRA, capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr[-3000:])
    return open(out).read(), r.stderr


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.strip().split("\n")))


def remarks(rp):
    out = {}
    for m in re.finditer(r"Function Name: (\S+) \[.*?(?=Function Name:|\Z)", rp, re.S):
        blk = m.group(0)

        def g(key):
            mm = re.search(key + r": (\d+)", blk)
            return int(mm.group(1)) if mm else None
        out[m.group(1)] = dict(sgpr=g("TotalSGPRs"), vgpr=g("VGPRs"), agpr=g("AGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"),
                               sgpr_spill=g("SGPRs Spill"), vgpr_spill=g("VGPRs Spill"), occ=g(r"Occupancy \[waves/SIMD\]"))
    return out


def scan(body):
    """Counts of scratch and AGPR-copy instructions per loop nest level.
    The tick kernel is one big loop over the fused ticks (depth 1); depth 2 = code that runs once per Arnoldi
    iteration (Gram-Schmidt rounds, Hessenberg column) and the stage loops of the preamble; depth >= 3 = the stage
    loops inside the Arnoldi loop (the critical path).  Loops that contain v_trig_preop_f64 (library
    sincos inlined) or a call (library sincos out of line, lean kernels) are the redo of a chunk whose arguments left
    the fast trig range: counted separately as `slow`.  Only a loop of depth >= 3 can be such a redo: the row-parallel
    kernels (NWT) inline sincos straight into the Arnoldi loop (no stage loop around it), and there only the blocks that
    hold the library path themselves are `slow` — the rest of the Arnoldi loop is `iter` like everywhere else."""
    blocks, cur = [], None
    for line in body.split("\n"):
        t = line.strip()
        mm = re.match(r"^(\.LBB\d+_\d+):", t)
        if mm:
            cur = dict(label=mm.group(1)[2:], header=None, depth=0, ops=[])
            blocks.append(cur)
            continue
        if cur is None:
            continue
        if t.startswith(";"):
            d = re.search(r"Loop Header: Depth=(\d+)", t)
            if d:
                cur["header"], cur["depth"] = cur["label"], max(cur["depth"], int(d.group(1)))
            d = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", t)
            if d and int(d.group(2)) >= cur["depth"]:
                cur["header"], cur["depth"] = d.group(1), int(d.group(2))
            continue
        if not t or t.startswith("."):
            continue
        cur["ops"].append(t.split()[0])
    is_slow = lambda b: any(o in ("v_trig_preop_f64", "s_swappc_b64") for o in b["ops"])
    slow_headers = {b["header"] for b in blocks if b["header"] and b["depth"] >= 3 and is_slow(b)}
    levels = {k: dict(n=0, scratch=0, acc=0, lane=0) for k in ("tick", "iter", "stage", "slow", "outside")}
    loops = {}
    for b in blocks:
        key = ("slow" if b["header"] in slow_headers or (b["depth"] in (1, 2) and is_slow(b)) else
               "outside" if b["depth"] == 0 else "tick" if b["depth"] == 1 else "iter" if b["depth"] == 2 else "stage")
        sc = sum(o.startswith("scratch_") for o in b["ops"])
        ac = sum(o.startswith("v_accvgpr") for o in b["ops"])
        lv = levels[key]
        lv["n"] += len(b["ops"]); lv["scratch"] += sc; lv["acc"] += ac
        lv["lane"] += sum(o.startswith(("v_readlane", "v_writelane")) for o in b["ops"])
        if key == "stage":
            l = loops.setdefault(b["header"], dict(n=0, scratch=0, acc=0, ds=0, vmem=0))
            l["n"] += len(b["ops"]); l["scratch"] += sc; l["acc"] += ac
            l["ds"] += sum(o.startswith("ds_") for o in b["ops"])
            l["vmem"] += sum(o.startswith(("global_", "buffer_", "flat_")) for o in b["ops"])
    return levels, loops


EXTRA = []

FP_ARITH = re.compile(r"^v_(pk_)?(fma|fmac|mad|mac|add|sub|mul|max|min)\w*_f(16|32|64)")


def block_listing(asm, name, short, r):
    """One line per basic block of the kernel `name`, in program order."""
    m = re.search(r"^" + re.escape(name) + r":.*?\.end_amdhsa_kernel", asm, re.S | re.M)
    kinds = ("acc", "lane", "dpp", "ds", "global", "zero")
    blocks, cur = [], dict(label="(entry)", depth=0, n=0, **{k: 0 for k in kinds})
    blocks.append(cur)
    n_scratch = len(re.findall(r"^\s*scratch_", m.group(0), re.M))
    for line in m.group(0).split("\n")[1:]:
        t = line.split(";")[0].strip() if not line.strip().startswith(";") else line.strip()
        mm = re.match(r"^\.(LBB\d+_\d+):", t)
        if mm:
            cur = dict(label="_" + mm.group(1).split("_")[1], depth=0, n=0, **{k: 0 for k in kinds})
            blocks.append(cur)
            continue
        if t.startswith(";"):
            d = re.search(r"Depth=(\d+)", t)
            if d:
                cur["depth"] = max(cur["depth"], int(d.group(1)))
            continue
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        if t.startswith("s_endpgm"):
            cur["n"] += 1
            break
        op = t.split()[0]
        operands = [o.strip() for o in t[len(op):].split(",")]
        cur["n"] += 1
        cur["acc"] += op.startswith("v_accvgpr")
        cur["lane"] += op.startswith(("v_readlane", "v_writelane"))
        cur["dpp"] += op.startswith("v_mov") and any(k in t for k in ("row_", "quad_perm", "wave_", "_dpp"))
        cur["ds"] += op.startswith("ds_")
        cur["global"] += op.startswith("global_")
        cur["zero"] += bool(FP_ARITH.match(op)) and "0" in operands[1:]
    tot = {k: sum(b[k] for b in blocks) for k in ("n",) + kinds}
    lines = [f"# Basic blocks of `{short}` (gfx950, hipcc -O3; tools/isa_summary.py --blocks)", "",
             "Program order.  depth: loop nest level (1 = ticks, 2 = Arnoldi iterations, 3+ = loops inside one).  acc = v_accvgpr_*,",
             "lane = v_readlane/v_writelane, dpp = DPP moves, zero0 = fp arithmetic with a literal-zero operand.", "",
             f"VGPR {r.get('vgpr')}, AGPR {r.get('agpr')}, VGPR spill {r.get('vgpr_spill')}, SGPR spill {r.get('sgpr_spill')}, "
             f"scratch {r.get('scratch')} B/lane, scratch_ instructions {n_scratch}", "",
             f"total: {tot['n']} instructions, acc {tot['acc']}, lane {tot['lane']}, dpp {tot['dpp']}, ds {tot['ds']}, "
             f"global {tot['global']}, zero0 {tot['zero']}", "",
             "block  depth  instrs    acc   lane    dpp     ds global  zero0"]
    for b in blocks:
        lines.append(f"{b['label']:<6} {b['depth']:>5} {b['n']:>7} " + " ".join(f"{b[k]:>6}" for k in kinds))
    return "\n".join(lines) + "\n"


def blocks_main(sub, out_path):
    srcs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.startswith("inst_") and f.endswith(".hip"))
    with ThreadPoolExecutor(min(6, len(os.sched_getaffinity(0)))) as ex:
        res = list(ex.map(compile_tu, srcs))
    for asm, rp in res:
        names = [m.group(1) for m in re.finditer(r"^(_Z\w+):", asm, re.M) if "_kernel" in m.group(1)]
        dm = demangle(names) if names else {}
        for name in names:
            if sub in dm[name]:
                short = re.sub(r"cgm::|void |\(cgm::WgParams<\w+>\)|\(cgm::LaneParams<\w+>\)", "", dm[name])
                text = block_listing(asm, name, short, remarks(rp).get(name, {}))
                if out_path:
                    open(os.path.join(ROOT, out_path) if not os.path.isabs(out_path) else out_path, "w").write(text)
                print(text)
                return
    sys.exit(f"no kernel whose name contains {sub!r}")


def operator_summary(header, cls):
    from cgmres_cpp_amd.plugin import TEMPLATE
    os.makedirs(TMP, exist_ok=True)
    src = os.path.join(TMP, "op_" + re.sub(r"\W", "_", cls) + ".hip")
    with open(src, "w") as f:
        f.write(TEMPLATE.format(origin=header, header=os.path.abspath(header), glue=os.path.join(CSRC, "user_operator.hip.h"),
                                macro="CGMRES_HIP_DEFINE_OPERATOR", cls=cls))
    asm, rp = compile_tu(src)
    rm = remarks(rp)
    names = [m.group(1) for m in re.finditer(r"^(_Z\w+):", asm, re.M) if "gmres_" in m.group(1)]
    dm = demangle(names) if names else {}
    kinds = ("ds_", "flat_", "scratch_", "global_")
    lines = [f"# ISA summary of the operator plugin of `{cls}` ({os.path.basename(header)}; gfx950, hipcc -O3)", "",
             "Per loop depth: instructions, of which ds_/flat_/scratch_/global_ accesses (depth 0 = straight-line code, "
             "1 = the Arnoldi loop, 2+ = loops inside it).", "",
             "| kernel | VGPR | SGPR | scratch B/lane | instrs | depth 0 | depth 1 | depth 2+ |", "|---|---|---|---|---|---|---|---|"]
    for name in names:
        m = re.search(r"^" + re.escape(name) + r":.*?\.end_amdhsa_kernel", asm, re.S | re.M)
        if not m:
            continue
        lv = [dict(n=0, **{k: 0 for k in kinds}) for _ in range(3)]
        depth = 0
        for line in m.group(0).split("\n"):
            t = line.strip()
            if re.match(r"^\.LBB\d+_\d+:", t):
                depth = 0
            elif t.startswith(";"):
                d = re.search(r"Depth=(\d+)", t)
                if d:
                    depth = max(depth, int(d.group(1)))
            elif t and not t.startswith(".") and not t.endswith(":"):
                c = lv[min(depth, 2)]
                c["n"] += 1
                for k in kinds:
                    c[k] += t.startswith(k)
        r = rm.get(name, {})
        short = re.sub(r"cgm::|void |\(.*", "", dm.get(name, name))
        cell = lambda c: f"{c['n']} (" + "/".join(str(c[k]) for k in kinds) + ")"
        lines.append(f"| `{short}` | {r.get('vgpr')} | {r.get('sgpr')} | {r.get('scratch')} | {sum(c['n'] for c in lv)} | "
                     f"{cell(lv[0])} | {cell(lv[1])} | {cell(lv[2])} |")
    return "\n".join(lines) + "\n"


def main():
    args = [a for a in sys.argv[1:]]
    out_path = None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    if "--csrc" in args:
        global CSRC
        i = args.index("--csrc")
        CSRC = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    for a in list(args):
        if a.startswith("-D"):
            EXTRA.append(a)
            args.remove(a)
    if "--blocks" in args:
        i = args.index("--blocks")
        blocks_main(args[i + 1], out_path)
        return
    if "--operator" in args:
        i = args.index("--operator")
        sys.path.insert(0, ROOT)
        text = operator_summary(args[i + 1], args[i + 2])
        if out_path:
            open(os.path.join(ROOT, out_path) if not os.path.isabs(out_path) else out_path, "w").write(text)
        print(text)
        return
    pat = args[0] if args else "tick_wg_kernel"
    srcs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.startswith("inst_") and f.endswith(".hip"))
    with ThreadPoolExecutor(min(6, len(os.sched_getaffinity(0)))) as ex:
        res = list(ex.map(compile_tu, srcs))
    lines = ["# ISA summary of the tick kernels (gfx950, hipcc -O3; generated by tools/isa_summary.py)", "",
             "Per kernel: registers and spill counts from the compiler remarks, then WHERE scratch_load/store instructions and",
             "VGPR<->AGPR copies (v_accvgpr_*, one issue slot each) sit, by loop nest level: `stage` = the stage loops inside the",
             "Arnoldi loop (state / coefficient / costate sweeps: the critical path), `iter` = once per Arnoldi iteration",
             "(Gram-Schmidt rounds, Hessenberg column) and the preamble's stage loops, `tick` = once per control tick,",
             "`slow` = the library-sincos redo of a chunk of stages (arguments beyond the fast trig range; never taken in the benchmarks).",
             "Entries are `scratch/acc/lane` instruction counts (static; lane = v_readlane + v_writelane) of `instrs` instructions.", "",
             "| kernel | VGPR | AGPR | VGPR spill | SGPR spill | scratch B/lane | instrs | stage | iter | tick | slow |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    detail = []
    for (asm, rp), src in zip(res, srcs):
        rm = remarks(rp)
        names = [m.group(1) for m in re.finditer(r"^(_Z\w+):", asm, re.M) if pat in m.group(1)]
        dm = demangle(names) if names else {}
        for name in names:  # (by name: a device FUNCTION ahead of a kernel must not swallow it)
            m = re.search(r"^" + re.escape(name) + r":.*?\.end_amdhsa_kernel", asm, re.S | re.M)
            if not m:
                continue
            lv, loops = scan(m.group(0))
            r = rm.get(name, {})
            short = re.sub(r"cgm::|void |\(cgm::WgParams<\w+>\)|\(cgm::LaneParams<\w+>\)", "", dm.get(name, name))
            cell = lambda k: f"{lv[k]['scratch']}/{lv[k]['acc']}/{lv[k]['lane']} of {lv[k]['n']}"
            lines.append(f"| `{short}` | {r.get('vgpr')} | {r.get('agpr')} | {r.get('vgpr_spill')} | {r.get('sgpr_spill')} | "
                         f"{r.get('scratch')} | {sum(v['n'] for v in lv.values())} | {cell('stage')} | {cell('iter')} | "
                         f"{cell('tick')} | {cell('slow')} |")
            hot = {h: l for h, l in loops.items() if l["scratch"] or l["acc"]}
            if hot:
                detail.append(f"\n`{short}` — stage loops with scratch / AGPR copies: " +
                              "; ".join(f"{h}: {l['n']} instrs (ds {l['ds']}, vmem {l['vmem']}) scratch {l['scratch']} acc {l['acc']}"
                                        for h, l in hot.items()))
    text = "\n".join(lines + [""] + detail) + "\n"
    if out_path:
        open(os.path.join(ROOT, out_path) if not os.path.isabs(out_path) else out_path, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
