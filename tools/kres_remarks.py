"""Kernel resources of two builds compared from their -Rpass-analysis=kernel-resource-usage remarks.
usage: make -C conditional-ude_amd/csrc CXXFLAGS="<flags.mk's> -Rpass-analysis=kernel-resource-usage"      (each tree)
       kres_remarks.py OLD NEW
OLD / NEW: a log of the compiler's standard error, or a directory of such logs.  A parallel build interleaves the remarks
of its compiler processes line by line, and a kernel's figures are then attributed to its neighbours: build with -j1, or
give every compiler process a log of its own (HIPCC = a wrapper that redirects standard error by output name).
Prints every kernel present in both logs whose VGPRs, AGPRs, SGPR / VGPR spills, scratch, LDS or occupancy differ, the
kernels only the new build has, and a summary line.  A kernel compiled in several translation units is compared as the
sorted list of its units' figures.  A kernel template that gained a trailing boolean parameter is matched to the old
build's instantiation through its `false` value (cpep_kernel<..., 0> against cpep_kernel<..., 0, false>)."""
import os
import re
import subprocess
import sys

FIELDS = ("VGPRs", "AGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
          "Occupancy [waves/SIMD]")


def load(path):
    out = {}
    paths = sorted(os.path.join(path, f) for f in os.listdir(path)) if os.path.isdir(path) else [path]
    for p in paths:
        load_one(p, out)
    return out


def load_one(path, out):
    cur = None
    for line in open(path, errors="replace"):
        m = re.match(r"(\S+?):\d+:\d+: remark: Function Name: (\S+)", line)
        if m:
            cur = {}
            out.setdefault(m.group(2), []).append(cur)
            continue
        m = re.match(r"\S+: remark:\s+([^:]+): (\S+) \[-Rpass", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[m.group(1)] = m.group(2)
    return out


def demangle(names):
    try:
        txt = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, txt.split("\n")))
    except Exception:
        return {n: n for n in names}


def by_name(raw):
    names = demangle(sorted(raw))
    return {names[k]: sorted(tuple(u.get(f) for f in FIELDS) for u in v) for k, v in raw.items()}


def main():
    old, new = by_name(load(sys.argv[1])), by_name(load(sys.argv[2]))
    for k in sorted(new):                             # ROWS = false of a kernel that gained the switch: the old kernel
        short = re.sub(r", false>\(", ">(", k)
        if k not in old and short != k and short in old and short not in new:
            new[short] = new.pop(k)
    both = sorted(set(old) & set(new))
    names = {k: k for k in set(old) | set(new)}
    changed = [k for k in both if old[k] != new[k]]
    print(f"{len(old)} kernels in the old build, {len(new)} in the new, {len(both)} in both; "
          f"{len(changed)} of those differ in {', '.join(FIELDS)}")
    for k in changed:
        print("CHANGED", names[k])
        print(f"    {old[k]} -> {new[k]}")
    gone = sorted(set(old) - set(new))
    for k in gone:
        print("GONE   ", names[k])
    added = sorted(set(new) - set(old))
    print(f"{len(added)} kernels only in the new build:")
    for k in added:
        print("NEW    ", names[k], " ".join(f"{f.split()[0]}={v}" for f, v in zip(FIELDS, new[k][0])))


if __name__ == "__main__":
    main()
