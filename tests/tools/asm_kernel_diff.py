#!/usr/bin/env python3
"""Kernel by kernel comparison of two gfx950 assembly listings of one translation unit (CPU side, no GPU):
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Idi-hpc_amd/csrc --cuda-device-only -S unit.hip -o new.s
    tests/tools/asm_kernel_diff.py parent.s new.s [--only names.txt] [--all]
Per kernel: VGPRs, SGPRs, scratch bytes, LDS bytes, occupancy, instruction count, and whether the sequence of vector memory
operations (global / scratch loads and stores, with their nt modifier), barriers and vmcnt waits is the same in program order.
Prints the kernels in which any of these moves (--all: every kernel) and a summary.  --only: a file of substrings of demangled
names, one per line; the summary is then given for the kernels that match one of them and for the rest separately."""
import re
import subprocess
import sys

META = {"NumVgprs": "vgpr", "TotalNumSgprs": "sgpr", "ScratchSize": "scratch", "LDSByteSize": "lds", "Occupancy": "occ"}


def parse(path):
    kernels, cur, body = {}, None, False
    for ln in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m:
            cur, body = {"insts": 0, "mem": []}, True
            kernels[m.group(1)] = cur
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            body = False
            continue
        if body:
            m = re.match(r"\s+([a-z][a-z0-9_]+)\b(.*)", ln)
            if not m:
                continue
            op, rest = m.group(1), m.group(2).split(";")[0]
            cur["insts"] += 1
            if re.match(r"(global|scratch|buffer|flat)_(load|store|atomic)", op):
                cur["mem"].append(op + (" nt" if re.search(r"\bnt\b", rest) else ""))
            elif op == "s_barrier":
                cur["mem"].append(op)
            elif op == "s_waitcnt":
                w = re.search(r"vmcnt\(\d+\)", rest)
                if w:
                    cur["mem"].append(w.group(0))
        else:
            m = re.match(r";\s*(\w+):\s*(\d+)", ln)
            if m and m.group(1) in META:
                cur.setdefault(META[m.group(1)], int(m.group(2)))
    return {k: v for k, v in kernels.items() if "occ" in v}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {n: re.sub(r"hpc_rll::\(anonymous namespace\)::|hpc_rll::|void ", "", d).split("(")[0] for n, d in zip(names, out)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    only = None
    if "--only" in sys.argv:
        only = [l.strip() for l in open(sys.argv[sys.argv.index("--only") + 1]) if l.strip()]
        args.remove(sys.argv[sys.argv.index("--only") + 1])
    a, b = parse(args[0]), parse(args[1])
    print(f"kernels: {len(a)} -> {len(b)}; only in the first: {sorted(set(a) - set(b))}; only in the second: {sorted(set(b) - set(a))}")
    names = demangle(sorted(set(a) & set(b)))
    keys = ("vgpr", "sgpr", "scratch", "lds", "occ", "insts")
    tally = {}
    for n, dem in sorted(names.items(), key=lambda x: x[1]):
        x, y = a[n], b[n]
        moved = [k for k in keys if x[k] != y[k]] + (["mem"] if x["mem"] != y["mem"] else [])
        grp = "listed" if only is None or any(dem.startswith(o) or o in dem for o in only) else "other"
        t = tally.setdefault(grp, {"n": 0, "same": 0, **{k: 0 for k in keys}, "mem": 0, "worse": 0})
        t["n"] += 1
        t["same"] += not moved
        for k in moved:
            t[k] += 1
        worse = y["occ"] < x["occ"] or y["scratch"] > x["scratch"]
        t["worse"] += worse
        if moved or "--all" in sys.argv:
            cells = " ".join(f"{k} {x[k]}" + (f"->{y[k]}" if x[k] != y[k] else "") for k in keys)
            print(f"{grp:6s} {dem:58s} {cells} mem-seq {'MOVED' if x['mem'] != y['mem'] else 'same'} ({len(x['mem'])} ops)"
                  + ("  WORSE: occupancy lost or scratch grown" if worse else ""))
    for grp, t in tally.items():
        print(f"{grp}: {t['n']} kernels, {t['same']} unchanged in every column; moved: " +
              ", ".join(f"{k} {t[k]}" for k in keys + ("mem",)) + f"; occupancy lost or scratch grown: {t['worse']}")


if __name__ == "__main__":
    main()
