#!/usr/bin/env python3
"""Compare two sets of device assembly listings kernel by kernel: a plain listing differ for re-cuts of the kernel units.

usage: isa_diff.py OLD.s[,OLD2.s ...] NEW.s[,NEW2.s ...]

The listings are what the build's flags plus ``--cuda-device-only -S`` give for a unit.  For every kernel (matched by symbol
across all files of a side) the table shows
  * the metadata that must not move: .vgpr_count, .agpr_count, .group_segment_fixed_size, .private_segment_fixed_size,
    .max_flat_workgroup_size (the launch bound), and the occupancy the compiler states,
  * whether the multiset of non-scalar mnemonics (everything not starting ``s_``) is the same, with the differences listed, and
    whether they also come in the same order,
  * the scalar differences (reported only).
Exit status 1 when a kernel is missing on one side, or a metadata item or a non-scalar count differs.
"""
import collections
import re
import subprocess
import sys

META = (".vgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".max_flat_workgroup_size")


def kernels_of(path):
    """{symbol: (metadata dict, Counter of mnemonics, the non-scalar mnemonics in order)} of one listing."""
    lines = open(path).read().split("\n")
    bodies, order, cur, occupancy = {}, {}, None, {}
    for ln in lines:
        m = re.match(r"^(\w+):\s*(;.*)?$", ln)
        if m and not ln.startswith(".L") and cur is None:
            cur = m.group(1)
            bodies[cur], order[cur] = collections.Counter(), []
            continue
        if cur is not None:
            if ln.startswith(".Lfunc_end"):
                cur = None
                continue
            t = ln.strip()
            if not t or t[0] in ".;" or t.endswith(":"):
                continue
            bodies[cur][t.split()[0]] += 1
            if not t.startswith("s_"):
                order[cur].append(t.split()[0])
    last = None
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel (\w+)", ln)
        if m:
            last = m.group(1)
        m = re.match(r"; Occupancy: (\d+)", ln)
        if m and last:
            occupancy.setdefault(last, m.group(1))
    meta, entry = {}, None
    at = lines.index("amdhsa.kernels:") if "amdhsa.kernels:" in lines else len(lines)
    for ln in lines[at:]:
        if ln.startswith("  - "):
            entry = {}
            ln = "    " + ln[4:]
        m = re.match(r"^    (\.\w+):\s+(\S+)\s*$", ln)
        if m and entry is not None:
            entry[m.group(1)] = m.group(2)
            if m.group(1) == ".symbol":
                meta[m.group(2)[:-3]] = entry              # "<name>.kd"
    out = {}
    for name, e in meta.items():
        md = {k: e.get(k, "?") for k in META}
        md["occupancy"] = occupancy.get(name, "?")
        out[name] = (md, bodies.get(name, collections.Counter()), order.get(name, []))
    return out


def demangle(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(sig):
    sig = re.sub(r"^void ", "", sig)
    return re.sub(r"\(.*$", "", sig)


def delta(a, b, scalar):
    keys = sorted(k for k in set(a) | set(b) if k.startswith("s_") == scalar and a[k] != b[k])
    return ", ".join("%s %+d" % (k, b[k] - a[k]) for k in keys)


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = {}, {}
    for side, arg in ((old, sys.argv[1]), (new, sys.argv[2])):
        for p in arg.split(","):
            for k, v in kernels_of(p).items():
                side[k] = v + (p.rsplit("/", 1)[-1],)
    names = demangle(sorted(set(old) | set(new)))
    bad = 0
    print("%d kernels before, %d after" % (len(old), len(new)))
    print("%-44s %-20s %5s %5s %6s %8s %6s %4s  %s" % ("kernel", "unit", "vgpr", "agpr", "lds", "scratch", "bound", "occ", "instructions"))
    for sym in sorted(names, key=lambda s: names[s]):
        label = short(names[sym])
        if sym not in old or sym not in new:
            print("%-44s only %s" % (label, "before" if sym in old else "after"))
            bad += 1
            continue
        (mo, co, oo, _), (mn, cn, on, unit) = old[sym], new[sym]
        cells = []
        for k in META + ("occupancy",):
            cells.append(mo[k] if mo[k] == mn[k] else "%s>%s" % (mo[k], mn[k]))
            bad += mo[k] != mn[k]
        vec, sca = delta(co, cn, False), delta(co, cn, True)
        bad += bool(vec)
        nv = sum(n for k, n in cn.items() if not k.startswith("s_"))
        note = "%d non-scalar, %s" % (nv, ("same sequence" if oo == on else "same multiset, other order") if not vec else "NON-SCALAR DIFFERS: " + vec)
        if sca:
            note += "; scalar: " + sca
        print("%-44s %-20s %5s %5s %6s %8s %6s %4s  %s" % tuple([label[:44], unit] + cells + [note]))
    print("hard items that differ: %d" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
