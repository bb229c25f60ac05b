#!/usr/bin/env python3
"""What one trip of stage 1's k-loop executes.  sig16_kernel runs at the package power cap, so its time follows the number
of instructions a wave executes per vector (profiles/HISTORY.md, section 5): this counts them.  It cross-compiles sig16.hip
as tools/check_mfma_hazards.py does, finds in every sig16_kernel instantiation the k-loop - the block that branches back to
its own label and holds matrix instructions; one trip = two k-tiles - and prints the instructions of that block by class,
the most frequent opcodes of the vector ALU that are not matrix instructions, and the kernel's register figures (with the
number of distinct VGPRs the loop names: hipcc allocates all 128 either way).  It reports the instruction mix and judges
nothing (tests/test_stage1_loop_census.py holds the figures it must show).  No GPU:
    python tools/stage1_loop_census.py            -> one paragraph per instantiation
    python tools/stage1_loop_census.py --json     -> the same as one JSON object, keyed by the demangled kernel name"""
import collections
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_mfma_hazards import assembly          # noqa: E402  (the same cross-compile)

UNIT = "sig16.hip"
CLASSES = ("mfma", "valu", "lds_read", "lds_write", "lds_dma", "vmem", "s_nop", "salu", "control")


def classify(op: str, operands: str) -> str:
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds_read" if "read" in op or "load" in op else "lds_write"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        lds = op.startswith("global_load_lds") or re.search(r"(^|\s)lds(\s|$)", operands) is not None
        return "lds_dma" if lds else "vmem"
    if op == "s_nop":
        return "s_nop"
    if op.startswith(("s_waitcnt", "s_barrier", "s_cbranch", "s_branch", "s_setprio", "s_sleep", "s_endpgm")):
        return "control"
    return "salu"


def demangle(names):
    out = subprocess.run(["c++filt", *names], capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: d.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "") for n, d in zip(names, out)}


def kernels(text: str):
    """-> {mangled name: list of (label or None, opcode, operands)} for the sig16_kernel instantiations"""
    out, cur = {}, None
    for raw in text.splitlines():
        line = raw.split(";")[0].strip()
        if not line:
            continue
        if line.endswith(":") and not line.startswith("."):
            cur = out.setdefault(line[:-1], []) if "sig16_kernel" in line else None
            continue
        if cur is None:
            continue
        if re.fullmatch(r"\.LBB\d+_\d+:", line):
            cur.append((line[:-1], None, None))
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif not line.startswith(".") and not line.endswith(":"):
            op, _, rest = line.partition(" ")
            cur.append((None, op, rest.strip()))
    return out


def k_loop(body):
    """the instructions of the self-looping block with the most matrix instructions"""
    best, block, label = [], [], None
    for lab, op, rest in body:
        if lab is not None:
            block, label = [], lab
            continue
        block.append((op, rest))
        if op.startswith("s_cbranch") and label is not None and rest.split(",")[-1].strip() == label:
            if sum(o.startswith("v_mfma") for o, _ in block) > sum(o.startswith("v_mfma") for o, _ in best):
                best = list(block)
    return best


def vgprs_named(loop) -> int:
    """distinct architectural VGPRs the block names (what is live across it without being touched is not in it)"""
    used = set()
    for _, rest in loop:
        for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", rest):
            used |= set(range(int(a), int(b) + 1))
        used |= {int(a) for a in re.findall(r"\bv(\d+)\b", rest)}
    return len(used)


def metadata(text: str):
    """-> {mangled name: register figures} from the .amdhsa_ directives and the code-object notes"""
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        d = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
        out[m.group(1)] = {"arch_vgprs": int(d.get("accum_offset", 0)), "next_free_vgpr": int(d.get("next_free_vgpr", 0))}
    for m in re.finditer(r"- \.agpr_count:\s+(\d+)(.*?)\.wavefront_size", text, re.S):
        d = dict(re.findall(r"\.(\w+):\s+(\S+)", m.group(2)))
        if d.get("name") in out:
            out[d["name"]].update(agpr_count=int(m.group(1)), scratch_bytes=int(d["private_segment_fixed_size"]),
                                  vgpr_spill_count=int(d["vgpr_spill_count"]), sgpr_spill_count=int(d["sgpr_spill_count"]))
    return out


def census(text: str = None):
    text = assembly(UNIT) if text is None else text
    ks, meta = kernels(text), metadata(text)
    names = demangle(list(ks))
    out = {}
    for mangled, body in ks.items():
        loop = k_loop(body)
        classes = collections.Counter(classify(op, rest) for op, rest in loop)
        ops = collections.Counter(op for op, _ in loop)
        valu = collections.Counter(op for op, rest in loop if classify(op, rest) == "valu")
        out[names[mangled]] = {"classes": {c: classes.get(c, 0) for c in CLASSES}, "valu_opcodes": dict(valu.most_common()),
                               "opcodes": dict(ops.most_common()),
                               "registers": dict(meta.get(mangled, {}), k_loop_vgprs_named=vgprs_named(loop))}
    return out


def main() -> int:
    res = census()
    if "--json" in sys.argv[1:]:
        print(json.dumps(res, indent=1, sort_keys=True))
        return 0
    for name in sorted(res):
        r = res[name]
        print(name)
        print("  k-loop, one trip (two k-tiles): " + ", ".join(f"{c} {n}" for c, n in r["classes"].items() if n))
        print("  vector ALU besides the matrix instructions: " + ", ".join(f"{o} {n}" for o, n in list(r["valu_opcodes"].items())[:12]))
        print("  registers: " + ", ".join(f"{k} {v}" for k, v in sorted(r["registers"].items())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
