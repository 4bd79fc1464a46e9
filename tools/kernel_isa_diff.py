#!/usr/bin/env python3
"""Did a refactor change the code of a kernel?  Compiles the named .hip files of two trees to gfx950 assembly (the Makefile's
flags + --cuda-device-only -S; cross-compiles, no GPU needed) and compares every kernel symbol: VGPRs, AGPRs, LDS and scratch
bytes from its .amdhsa_* lines, its instruction count, and the opcodes whose counts differ.

    git archive --prefix=parent/ HEAD~1 | tar -x -C /tmp
    python3 tools/kernel_isa_diff.py /tmp/parent . pwconv.hip pwgrad.hip [--json profiles/NAME.json]

Exit status 1 when a kernel exists in one tree only or a resource differs; opcode differences are reported, not judged.
"""
import argparse
import collections
import concurrent.futures as cf
import json
import os
import re
import subprocess
import sys

FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize", "--cuda-device-only", "-S"]
RES = {"vgpr": ".amdhsa_next_free_vgpr", "agpr": ".amdhsa_accum_offset", "sgpr": ".amdhsa_next_free_sgpr",
       "lds": ".amdhsa_group_segment_fixed_size", "scratch": ".amdhsa_private_segment_fixed_size"}
EQUAL = ("vgpr", "agpr", "lds", "scratch")


def kernels(tree, name):
    """-> {demangled kernel: dict(resources, n = instructions, ops = Counter of opcodes, text = the instruction stream)}"""
    csrc = os.path.join(tree, "ppea-depth_amd", "csrc")
    asm = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [name, "-o", "-"], cwd=csrc, capture_output=True, text=True, check=True).stdout
    bodies, res, cur = {}, {}, None
    for line in asm.splitlines():
        s = line.split(";")[0].strip()
        m = re.match(r"^(\w+):$", s)
        if m and cur is None and re.search(r"^\s*\.type\s+%s,@function" % re.escape(m.group(1)), asm, re.M):
            cur = bodies.setdefault(m.group(1), [])
        elif s.startswith(".amdhsa_kernel "):
            cur = res.setdefault(s.split()[1], {})
        elif s in (".end_amdhsa_kernel",) or s.startswith(".Lfunc_end"):
            cur = None
        elif isinstance(cur, dict) and s.split()[:1] and s.split()[0] in RES.values():
            cur[s.split()[0]] = int(s.split()[1])
        elif isinstance(cur, list) and s and not s.startswith(".") and not s.endswith(":"):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", s)))
    names = sorted(res)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    out = {}
    for sym, d in zip(names, dem):
        d = re.sub(r"\(.*$", "", re.sub(r"^void ", "", d.replace("(anonymous namespace)::", "")))
        k = {key: res[sym].get(field, 0) for key, field in RES.items()}
        k["agpr"] = max(0, k["vgpr"] - k["agpr"])                          # accum_offset = first AGPR
        k.update(n=len(bodies[sym]), ops=collections.Counter(i.split()[0] for i in bodies[sym]), text=bodies[sym])
        out[d] = k
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--json", help="write the full report here")
    args = ap.parse_args()
    with cf.ThreadPoolExecutor(8) as ex:
        got = list(ex.map(lambda a: kernels(*a), [(t, f) for f in args.files for t in (args.old, args.new)]))
    report, bad = {}, 0
    for f, old, new in zip(args.files, got[0::2], got[1::2]):
        rows = report[f] = {}
        for name in sorted(set(old) | set(new)):
            o, n = old.get(name), new.get(name)
            if o is None or n is None:
                rows[name] = {"only_in": "new" if o is None else "old"}
                bad += 1
                continue
            ops = {op: [o["ops"][op], n["ops"][op]] for op in sorted(set(o["ops"]) | set(n["ops"])) if o["ops"][op] != n["ops"][op]}
            moved = sum(a != b for a, b in zip(o["text"], n["text"])) if o["n"] == n["n"] else None      # same length: lines that differ
            rows[name] = {"identical": o["text"] == n["text"], "instructions": [o["n"], n["n"]], "opcodes": ops, "lines_differing": moved,
                          **{k: [o[k], n[k]] for k in RES}}
            bad += any(o[k] != n[k] for k in EQUAL)
        same = sum(r.get("identical", False) for r in rows.values())
        print(f"{f}: {len(rows)} kernels, {same} with an identical instruction stream")
        for name, r in rows.items():
            if "only_in" in r:
                print(f"  {name}: only in the {r['only_in']} tree")
            elif not r["identical"]:
                res = " ".join(f"{k} {r[k][0]}->{r[k][1]}" for k in RES if r[k][0] != r[k][1])
                ops = (" ".join(f"{op} {a}->{b}" for op, (a, b) in r["opcodes"].items())
                       or f"same opcodes, other order or operands ({r['lines_differing']} lines)")
                print(f"  {name}: {r['instructions'][0]}->{r['instructions'][1]} instructions; {res + '; ' if res else ''}{ops}")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1, sort_keys=True)
            fh.write("\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
