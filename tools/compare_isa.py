#!/usr/bin/env python3
"""Compare two sets of gfx950 assembly files kernel by kernel (one-off analysis for a refactor that must not move generated code).

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S old.hip -o old.s        (likewise new.s)
    tools/compare_isa.py --old old_a.s old_b.s --new new.s [--rename REGEX REPL]...

A kernel is matched by its demangled name without the parameter list; --rename rewrites the old names first (in the order given) when
the refactor renamed kernels.  The instruction stream of a kernel is its lines between the symbol's label and .Lfunc_end with comments
and directives stripped and label numbers erased.  Prints one row per kernel: instructions old / new, identical or differs, VGPR /
SGPR / private segment / static LDS bytes from the kernel's metadata, waves per SIMD by registers old / new
(min(8, floor(512 / (ceil(VGPR / 8) * 8)))) and `ok` when the new kernel has no private segment, the old one's LDS size and no fewer
waves.  Exit status 1 when a kernel of one side has no partner.
"""
import argparse
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {m: re.sub(r"^void ", "", d.split("(")[0]) for m, d in zip(names, out)}


def kernels(path):
    """{mangled name: {"ins": [instruction lines], "vgpr": .., "sgpr": .., "priv": .., "lds": ..}} for the kernels (.amdhsa_kernel) of one file"""
    lines = open(path).read().split("\n")
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    res = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.split(";")[0].strip() == name + ":")
        ins = []
        for l in lines[start + 1:]:
            l = l.split(";")[0].strip()
            if l.startswith(".Lfunc_end"):
                break
            if not l or (l.startswith(".") and not l.endswith(":")):
                continue
            ins.append(re.sub(r"\.L([A-Za-z_]+)\d+(_\d+)?", r".L\1", l))
        desc = lines.index("\t.amdhsa_kernel " + name)          # the kernel descriptor: static LDS size
        lds = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", "\n".join(lines[desc:desc + 8]))
        res[name] = {"ins": ins, "lds": int(lds.group(1))}
    meta = "\n".join(lines[lines.index("amdhsa.kernels:"):]) if "amdhsa.kernels:" in lines else ""
    for entry in re.split(r"\n\s*- ", meta):
        n = re.search(r"\.name:\s*(\S+)", entry)
        if n and n.group(1) in res:
            for key, field in (("vgpr", "vgpr_count"), ("sgpr", "sgpr_count"), ("priv", "private_segment_fixed_size")):
                v = re.search(r"\." + field + r":\s*(\d+)", entry)
                if v:
                    res[n.group(1)][key] = int(v.group(1))
    return res


def load(paths, renames=()):
    allk = {}
    for p in paths:
        allk.update(kernels(p))
    names = demangle(list(allk))
    out = {}
    for m, k in allk.items():
        d = names[m]
        for rx, repl in renames:
            d = re.sub(rx, repl, d)
        out[d] = k
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPL"))
    a = ap.parse_args()
    old, new = load(a.old, a.rename), load(a.new)
    print("%-44s %8s %8s  %-9s  %-22s %-22s %-5s %s" % ("kernel (new name)", "ins old", "ins new", "stream", "VGPR/SGPR/priv/LDS old", "VGPR/SGPR/priv/LDS new", "waves", "resources"))
    waves = lambda k: min(8, 512 // (-(-k["vgpr"] // 8) * 8))
    kept = 0
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name), new.get(name)
        if o is None or n is None:
            print("%-44s %s" % (name, "only in --new" if o is None else "only in --old"))
            continue
        res = lambda k: "%d/%d/%d/%d" % (k.get("vgpr", -1), k.get("sgpr", -1), k.get("priv", -1), k.get("lds", -1))
        ok = n["priv"] == 0 and n["lds"] == o["lds"] and waves(n) >= waves(o)
        kept += ok
        print("%-44s %8d %8d  %-9s  %-22s %-22s %-5s %s" % (name, len(o["ins"]), len(n["ins"]), "identical" if o["ins"] == n["ins"] else "differs", res(o), res(n),
                                                          "%d/%d" % (waves(o), waves(n)), "ok" if ok else "WORSE"))
    print("%d kernels, resources kept by %d" % (len(set(old) & set(new)), kept))
    return 1 if set(old) != set(new) else 0


if __name__ == "__main__":
    sys.exit(main())
