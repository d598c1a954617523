#!/usr/bin/env python3
"""Evidence and A/B measurement of the row-Newton kernel's Gram-Schmidt rounds, on the GPU box (this script itself never
opens the GPU: every step is a fresh child process under a time limit, and the first step that faults, aborts or runs
out of time ends the job).

    python tools/gs_evidence.py --out DIR --libs name=path[,stamps=path] ... [--rounds 3] [--budget 600] [--skip pmc,stamps,ab,trace]
                                [--pmc-libs a,b] [--pmc-counters SQ_INSTS_VALU,SQ_INSTS_SALU,...]

For every library (the first one is the base of the comparisons):
  pmc     two rocprofv3 --pmc passes of the plain bench command, each a run of its own with the program directly after
          `--` and no tracing: the instruction-cache / instruction-fetch group, then the L2 (TCC) hit / miss / request
          counters the available-counter list offers.  Reduced to per wave and tick for the tick kernel.
          With --pmc-counters: ONE pass of exactly the counters named instead (two, half the names each, if the SQ does
          not hold them in one), per wave and tick — the instructions a wave actually issues.
  stamps  tools/phase_stamps.py on the library's -DCGM_STAMPS twin (stamps=...), with the split of the MGS rounds.
  ab      bench.py --steps 200 --warmup 50 --reps 5, the libraries interleaved, --rounds runs each; the first round also
          dumps the outputs, which are compared with == against the base library's.
  trace   rocprofv3 --kernel-trace --stats of the plain bench command: kernel time per launch.
Everything lands in DIR/gs_evidence.json (+ the raw outputs next to it)."""
import csv
import glob
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"]
PLAIN = ["--steps", "100", "--warmup", "20", "--reps", "1"]  # multiples of the 10 ticks a launch advances
ICACHE = ["SQC_ICACHE_REQ", "SQC_ICACHE_HITS", "SQC_ICACHE_MISSES", "SQC_ICACHE_MISSES_DUPLICATE", "SQ_IFETCH", "SQ_WAIT_INST_ANY",
          "SQ_WAVE_CYCLES"]
FATAL = (124, 137, 134, 139, -6, -9, -11)
TICKS_PER_LAUNCH = 10


def opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = os.path.abspath(opt("--out", os.path.join(ROOT, "_diag", "gs_evidence")))  # (_diag/ is git-ignored)
RESULT = {}


def save():
    with open(os.path.join(OUT, "gs_evidence.json"), "w") as fh:
        json.dump(RESULT, fh, indent=1)


DEADLINE = time.time() + float(opt("--budget", "600"))  # seconds for the whole job: the step limits are cut to what is left


def run(cmd, log, limit, env=None):
    """One GPU step.  Returns (rc, stdout); a fault, abort or time-out ends the whole job."""
    e = dict(os.environ, **(env or {}))
    limit = int(min(limit, DEADLINE - time.time()))
    if limit < 30:
        RESULT["stopped_at"] = dict(step=log, rc=None, stderr="out of the job's time budget before this step")
        save()
        sys.exit(f"{log}: not started, the job's time budget is used up")
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=e, cwd="/tmp")
    with open(os.path.join(OUT, log), "w") as fh:
        fh.write(r.stdout + "\n--- stderr ---\n" + r.stderr)
    print(f"[{log}] rc {r.returncode}", flush=True)
    if r.returncode in FATAL or "illegal memory access" in r.stderr:
        RESULT["stopped_at"] = dict(step=log, rc=r.returncode, stderr=r.stderr[-2000:])
        save()
        sys.exit(f"{log}: rc {r.returncode} — nothing more is started on the GPU")
    return r.returncode, r.stdout


def sha16(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def counters(d):
    """{counter: (launches, per-launch mean, waves per launch)} of the tick kernel from a --pmc output directory"""
    acc = {}
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "tick_wg" not in r["Kernel_Name"]:
                continue
            a = acc.setdefault(r["Counter_Name"], [0, 0.0, 0])
            a[0] += 1
            a[1] += float(r["Counter_Value"])
            a[2] = int(r.get("Grid_Size") or 0) // 64
    return {k: dict(launches=n, per_launch=v / n, waves=w) for k, (n, v, w) in acc.items() if n}


def pmc_pass(tag, names, lib):
    d = os.path.join(OUT, tag)
    rc, _ = run(["rocprofv3", "--pmc"] + names + ["-d", d, "--output-format", "csv", "--"] + BENCH + PLAIN, tag + ".log", 240,
                {"CGMRES_HIP_LIB": lib})
    return counters(d) if rc == 0 else None


def pmc(name, lib, tcc):
    got = pmc_pass(f"pmc_{name}_icache", ICACHE, lib)
    if got is None:  # more counters than one pass of the SQ holds: the same names in two runs
        got = {}
        for i, grp in enumerate((ICACHE[:4], ICACHE[4:])):
            got.update(pmc_pass(f"pmc_{name}_icache{i}", grp, lib) or {})
    l2 = pmc_pass(f"pmc_{name}_l2", tcc, lib) or {}
    per = lambda c, src: src[c]["per_launch"] / max(1, src[c]["waves"]) / TICKS_PER_LAUNCH if c in src else None
    out = dict(raw_per_launch={k: v["per_launch"] for k, v in {**got, **l2}.items()},
               waves_per_launch=next((v["waves"] for v in got.values()), None),
               icache_misses_per_wave_tick=per("SQC_ICACHE_MISSES", got),
               icache_requests_per_wave_tick=per("SQC_ICACHE_REQ", got),
               ifetch_per_wave_tick=per("SQ_IFETCH", got),
               wait_inst_any_per_wave_tick=per("SQ_WAIT_INST_ANY", got),
               wave_cycles_per_wave_tick=per("SQ_WAVE_CYCLES", got))
    if "SQ_WAIT_INST_ANY" in got and "SQ_WAVE_CYCLES" in got:
        out["wait_inst_any_over_wave_cycles"] = got["SQ_WAIT_INST_ANY"]["per_launch"] / got["SQ_WAVE_CYCLES"]["per_launch"]
    hit = next((l2[c]["per_launch"] for c in l2 if c.startswith("TCC_HIT")), None)
    miss = next((l2[c]["per_launch"] for c in l2 if c.startswith("TCC_MISS")), None)
    if hit is not None and miss is not None and hit + miss > 0:
        out["l2_hit_rate"] = hit / (hit + miss)
    return out


def pmc_named(name, lib, names):
    got = pmc_pass(f"pmc_{name}_named", names, lib)
    if got is None:
        got = {}
        h = (len(names) + 1) // 2
        for i, grp in enumerate((names[:h], names[h:])):
            got.update(pmc_pass(f"pmc_{name}_named{i}", grp, lib) or {})
    return dict(library_sha256_16=sha16(lib), launches=next((v["launches"] for v in got.values()), None),
                waves_per_launch=next((v["waves"] for v in got.values()), None),
                per_wave_and_tick={k: v["per_launch"] / max(1, v["waves"]) / TICKS_PER_LAUNCH for k, v in got.items()})


def stamps(name, lib):
    rc, txt = run([sys.executable, os.path.join(ROOT, "tools", "phase_stamps.py"), "--variant=2", "--lib=" + lib], f"stamps_{name}.txt", 240)
    rows = {}
    for m in re.finditer(r"^  (.+?)\s+(\d+) cyc/tick\s+([\d.]+)%\s+\((\d+) visits\)", txt, re.M):
        rows[m.group(1).strip()] = dict(cycles_per_tick=int(m.group(2)), percent=float(m.group(3)), visits=int(m.group(4)))
    head = re.search(r"shader cycles/tick (\d+), wall ([\d.]+) us/tick", txt)
    return dict(library_sha256_16=sha16(lib), cycles_per_tick=int(head.group(1)) if head else None,
                wall_us_per_tick=float(head.group(2)) if head else None,
                split={k: v for k, v in rows.items() if k.startswith("MGS")}, all=rows)


def main():
    os.makedirs(OUT, exist_ok=True)
    libs, twins = [], {}
    i = sys.argv.index("--libs") + 1
    while i < len(sys.argv) and not sys.argv[i].startswith("--"):
        parts = sys.argv[i].split(",")
        name, path = parts[0].split("=")
        libs.append((name, os.path.abspath(path)))
        for p in parts[1:]:
            if p.startswith("stamps="):
                twins[name] = os.path.abspath(p[7:])
        i += 1
    skip = set((opt("--skip", "") or "").split(","))
    rounds = int(opt("--rounds", "3"))
    RESULT["libraries"] = {n: dict(path=os.path.relpath(p, ROOT), library_sha256_16=sha16(p)) for n, p in libs}
    base = libs[0][0]

    pmc_libs = [l for l in libs if l[0] in (opt("--pmc-libs") or ",".join(n for n, _ in libs[:2])).split(",")]
    if "pmc" not in skip and opt("--pmc-counters"):
        RESULT["counters"] = {}
        for name, lib in pmc_libs:
            RESULT["counters"][name] = pmc_named(name, lib, opt("--pmc-counters").split(","))
            save()
    elif "pmc" not in skip:
        _, avail = run(["rocprofv3", "--list-avail"], "avail.log", 120)
        open(os.path.join(OUT, "avail.txt"), "w").write(avail)
        names = set(re.findall(r"\bTCC_(?:HIT|MISS|REQ)[A-Za-z_]*\b", avail))
        tcc = [("TCC_%s_sum" % k) if ("TCC_%s_sum" % k) in names else "TCC_" + k for k in ("HIT", "MISS", "REQ")]
        RESULT["tcc_counters_offered"] = sorted(names)
        RESULT["counters"] = {}
        for name, lib in pmc_libs:
            RESULT["counters"][name] = pmc(name, lib, tcc)
            save()

    if "stamps" not in skip:
        RESULT["stamps"] = {}
        for name, _ in libs:
            if name in twins:
                RESULT["stamps"][name] = stamps(name, twins[name])
                save()

    if "ab" not in skip:
        ms = {n: [] for n, _ in libs}
        lines = {}
        for rnd in range(rounds):
            for name, lib in libs:
                extra = ["--dump-outputs", os.path.join(OUT, "dump_" + name)] if rnd == 0 else []
                rc, txt = run(BENCH + ["--steps", "200", "--warmup", "50", "--reps", "5"] + extra, f"ab_{name}_{rnd}.log", 300,
                              {"CGMRES_HIP_LIB": lib})
                if rc:
                    sys.exit(f"bench failed on {name}")
                line = json.loads(txt.strip().split("\n")[-1])
                ms[name].append(line["ms_per_step"])
                lines[name] = line
        import numpy as np
        ab = {}
        for name, _ in libs:
            v = ms[name]
            ab[name] = dict(us_per_tick_runs=[1e3 * x for x in v], median_us=1e3 * statistics.median(v), spread_us=1e3 * (max(v) - min(v)),
                            variant_name=lines[name].get("config", {}).get("variant_name"),
                            bound_observed=lines[name].get("roofline", {}).get("bound_observed"),
                            library_sha256_16=lines[name].get("roofline", {}).get("library_sha256_16"))
            same = {}
            for f in sorted(glob.glob(os.path.join(OUT, "dump_" + base, "*.npy"))):
                a, b = np.load(f), np.load(os.path.join(OUT, "dump_" + name, os.path.basename(f)))
                same[os.path.basename(f)] = bool(a.shape == b.shape and np.all((a == b) | (np.isnan(a) & np.isnan(b))))
            ab[name]["outputs_equal_to_" + base] = same
        for name, _ in libs[1:]:
            d = ab[base]["median_us"] - ab[name]["median_us"]
            bar = 3 * max(ab[base]["spread_us"], ab[name]["spread_us"])
            ab[name]["gain_us_vs_" + base] = d
            ab[name]["bar_us"] = bar
            ab[name]["verdict"] = "gain" if d > bar else ("slower" if -d > bar else "no difference beyond 3x spread")
        RESULT["ab"] = ab
        save()

    if "trace" not in skip:
        RESULT["kernel_trace"] = {}
        for name, lib in libs:
            d = os.path.join(OUT, "trace_" + name)
            rc, _ = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + BENCH + PLAIN,
                        f"trace_{name}.log", 240, {"CGMRES_HIP_LIB": lib})
            for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if "tick_wg" in r["Name"]:
                        RESULT["kernel_trace"][name] = dict(calls=int(r["Calls"]), average_ns=float(r["AverageNs"]),
                                                            us_per_tick=float(r["AverageNs"]) / 1e3 / TICKS_PER_LAUNCH)
            save()
    save()
    print(json.dumps({k: v for k, v in RESULT.items() if k in ("ab", "kernel_trace")}, indent=1))


if __name__ == "__main__":
    main()
