#!/usr/bin/env python3
"""Do the kernels of this tree compile to the machine code another tree's do?  (no GPU needed)
    python3 tools/kernel_text_equal.py <other tree> [unit ...]         (units: rerank scan query ...; default: all of them)
Compiles each unit of both trees for gfx950 with the build's own flags plus `--cuda-device-only -S` and compares, kernel by
kernel, the instruction lines: comments, directives and blank lines dropped, the function's number taken out of its local labels
(.LBB<n>_<i>).  Kernels are paired by demangled name, without the namespaces (a type that moves between an unnamed namespace and
`lshrs::` renames a kernel, not its code).  Prints `N kernels, N identical`, names those that differ or exist on one side only,
and exits 1 if there are any.  It compares and nothing else."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lshrs_amd._native import HIPCC_FLAGS, UNITS      # noqa: E402


def kernels(tree, unit):
    """{demangled kernel name: [instruction lines]} of one unit of one tree"""
    csrc = os.path.join(tree, "lshrs_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *HIPCC_FLAGS, "-I" + os.path.join(tree, "include"), "-I" + csrc,
           "--cuda-device-only", "-S", os.path.join(csrc, unit + ".hip"), "-o", "-"]
    asm = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    entry = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    found, name = {}, None
    for ln in asm.splitlines():
        ln = ln.split(";")[0].strip()
        m = re.fullmatch(r"([A-Za-z_$][\w$.]*):", ln)
        if m and m.group(1) in entry:
            name = m.group(1)
            found[name] = []
        elif ln.startswith(".Lfunc_end"):
            name = None
        elif name and ln and (not ln.startswith(".") or ln.startswith(".LBB")):
            found[name].append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
    names = subprocess.run(["c++filt"], input="\n".join(found), check=True, capture_output=True, text=True).stdout.splitlines()
    plain = [n.replace("(anonymous namespace)::", "").replace("lshrs::", "") for n in names]
    assert len(set(plain)) == len(found), "two kernels of %s share a name" % unit
    return dict(zip(plain, found.values()))


def main(argv):
    if not argv or argv[0].startswith("-"):
        sys.exit(__doc__)
    other, units = os.path.abspath(argv[0]), argv[1:] or list(UNITS)
    total, same, bad = 0, 0, []
    with ThreadPoolExecutor(max_workers=4) as pool:      # (the compilations are independent: a few at a time)
        built = list(pool.map(lambda job: kernels(*job), [(tree, unit) for unit in units for tree in (other, ROOT)]))
    for i, unit in enumerate(units):
        theirs, ours = built[2 * i], built[2 * i + 1]
        for name in sorted(set(theirs) | set(ours)):
            total += 1
            if name not in ours or name not in theirs:
                bad.append("%s: %s (only in %s)" % (unit, name, "the other tree" if name in theirs else "this tree"))
            elif theirs[name] != ours[name]:
                bad.append("%s: %s (%d / %d instruction lines)" % (unit, name, len(theirs[name]), len(ours[name])))
            else:
                same += 1
    print("%d kernels, %d identical" % (total, same))
    for b in bad:
        print("  differs  " + b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
