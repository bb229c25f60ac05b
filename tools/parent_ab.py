#!/usr/bin/env python3
"""A change to the native code against its parent, on one box in one session: two builds of liblshrs_hip.so (the parent's
sources built with tools/ab_build.py, selected through LSHRS_HIP_LIBRARY), a fresh child process per measurement, A and B
alternating.  Every child runs under its own time limit and the sequence ends at the first one that fails.
    python tools/parent_ab.py PARENT.so [CHANGE.so] [--pairs 4] [--noise-pairs 2] [--steps 200] [--no-extras]
A = PARENT.so, B = CHANGE.so (default: the tree's own library).  Printed: lshrs_build_flags() of both libraries; per pair the
headline `value` and `roofline.kernel_ms_mean` of `python bench.py --steps K`; the parent against itself (--noise-pairs) for
the noise; then - unless --no-extras - one pair each of bench.py's sustained block (the function `--full` runs:
in_kernel_clock_GHz), `bench.py --only c5` and stage 1 at 16 x 16 x 300 (tools/half_rows_ab.py's child).  The verdict: a gain
if B is faster than A in every pair and the median gain in kernel_ms_mean is at least three times the median absolute
difference of the parent-against-parent pairs."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 300        # seconds a child may take


def run(lib, cmd, limit=LIMIT):
    env = {k: v for k, v in os.environ.items() if k != "LSHRS_SIG16_HALF_MAX_TILES"}
    env["LSHRS_HIP_LIBRARY"] = lib
    out = subprocess.run([sys.executable, *cmd], cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
    if out.returncode != 0:
        print(f"child {cmd} with {lib} ended with status {out.returncode}:\n{out.stderr[-3000:]}", flush=True)
        raise SystemExit(1)
    return out.stdout


def last_json(text):
    return json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])


def bench(lib, steps):
    r = last_json(run(lib, ["bench.py", "--gpus", "1", "--steps", str(steps)]))
    return float(r["value"]), float(r["roofline"]["kernel_ms_mean"])


def sustained_child():
    sys.path.insert(0, ROOT)
    import torch

    import bench as B
    from lshrs_amd import LSHHasher

    n = 1_000_000
    x = torch.randn(n, B.DIM, device="cuda", generator=torch.Generator("cuda").manual_seed(20240101))
    h = LSHHasher(B.BANDS, B.ROWS, B.DIM, seed=42)
    keys = h.hash_device(x)
    for _ in range(40):
        h.hash_device(x, out=keys)
    s = B.bench_sustained(torch, h, x, keys, 2.0, lambda: None)
    print(json.dumps({k: s.get(k) for k in ("value", "stage1_kernel_ms_mean", "in_kernel_clock_GHz", "power_mid_run")}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("change", nargs="?", default=os.path.join(ROOT, "lshrs_amd", "csrc", "liblshrs_hip.so"))
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--noise-pairs", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--no-extras", action="store_true")
    a = ap.parse_args()
    A, B = os.path.abspath(a.parent), os.path.abspath(a.change)
    flags = "from lshrs_amd import _native; print(hex(int(_native.load().lshrs_build_flags())))"
    print(f"A = {os.path.relpath(A, ROOT)} (parent), lshrs_build_flags() = {run(A, ['-c', flags]).strip()}")
    print(f"B = {os.path.relpath(B, ROOT)} (change), lshrs_build_flags() = {run(B, ['-c', flags]).strip()}", flush=True)
    noise = []
    for i in range(a.noise_pairs):
        (v0, k0), (v1, k1) = bench(A, a.steps), bench(A, a.steps)
        noise.append(abs(k1 - k0) / k0)
        print(f"A/A pair {i}: value {v0 / 1e6:.2f} / {v1 / 1e6:.2f} M vec/s, stage-1 kernel_ms_mean {k0:.4f} / {k1:.4f} (|diff| {100 * noise[-1]:.2f} %)", flush=True)
    gains, faster = [], []
    for i in range(a.pairs):
        (v0, k0), (v1, k1) = bench(A, a.steps), bench(B, a.steps)
        gains.append((k0 - k1) / k0)
        faster.append(k1 < k0)
        print(f"A/B pair {i}: value {v0 / 1e6:.2f} -> {v1 / 1e6:.2f} M vec/s ({100 * (v1 / v0 - 1):+.2f} %), "
              f"stage-1 kernel_ms_mean {k0:.4f} -> {k1:.4f} ({-100 * gains[-1]:+.2f} %)", flush=True)
    if gains and noise:
        g, nz = statistics.median(gains), statistics.median(noise)
        won = all(faster) and g >= 3 * nz
        print(f"median gain in kernel_ms_mean {100 * g:.2f} %, median |A/A difference| {100 * nz:.2f} %, B faster in "
              f"{sum(faster)} of {len(faster)} pairs: {'A GAIN' if won else 'NOT a gain'} by the three-times-the-noise rule", flush=True)
    if a.no_extras:
        return
    me = os.path.abspath(__file__)
    for name, lib in (("A", A), ("B", B)):
        print(f"sustained {name}: {run(lib, [me, '--sustained-child']).strip().splitlines()[-1]}", flush=True)
    for name, lib in (("A", A), ("B", B)):
        c5 = last_json(run(lib, ["bench.py", "--only", "c5", "--no-check"], limit=600))["c5"]
        print(f"c5 {name}: value {c5.get('value', 0) / 1e6:.3f} M vec/s, stage-1 kernel_ms_mean {(c5.get('roofline') or {}).get('kernel_ms_mean')}", flush=True)
    for name, lib in (("A", A), ("B", B)):
        s1, step, rate, frac, digest, route, flagged = run(lib, ["tools/half_rows_ab.py", "--child", "300", "16", "16"]).split()[-7:]
        print(f"16x16x300 {name}: stage 1 {s1} ms, step {step} ms, {rate} M vec/s, keys {digest}, {route}, flagged {flagged}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--sustained-child":
        sustained_child()
    else:
        main()
