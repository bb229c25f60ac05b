"""What sig16_kernel's k-loop executes per trip (two k-tiles), from a cross-compile - no GPU (tools/stage1_loop_census.py).
Stage 1 runs at the package power cap: its time follows the instructions a wave executes per vector, and the vector-ALU
port is the one that is nearly full.  The floors: 192 matrix instructions, 72 LDS reads (64 fragment + 8 x), 16 LDS-DMA
pieces (8 waves) or 24 (4 waves); the split as written is 144 vector-ALU instructions (32 conversions, 32 residuals, 32 to
widen the high halves again, 32 dot products for the two norms, 16 for max |x|), addresses 8 more (one per stage for the
fragments, two per k-tile for x).  Before the LDS-DMA went through buffer descriptors and the ring positions through
rotating scalars the loop had 188 (8 waves) / 304 (4 waves) and the 4-wave kernels spilled four registers."""

from __future__ import annotations

import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = ("sig16_kernel<false, false, 8>", "sig16_kernel<true, false, 8>")
HALF = ("sig16_kernel<false, false, 4>", "sig16_kernel<true, false, 4>", "sig16_kernel<false, true, 4>", "sig16_kernel<true, true, 4>")


@pytest.fixture(scope="module")
def census():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import stage1_loop_census
    finally:
        sys.path.pop(0)
    return stage1_loop_census.census()


def test_every_instantiation_has_its_k_loop(census):
    assert len(census) == 8
    for name, c in census.items():
        assert c["classes"]["mfma"] == 192 and c["classes"]["lds_read"] == 72, (name, c["classes"])
        assert c["classes"]["lds_dma"] == (16 if name.endswith("8>") else 24), (name, c["classes"])
        assert c["registers"]["agpr_count"] == 128 and c["registers"]["arch_vgprs"] <= 128, (name, c["registers"])   # two waves per SIMD


@pytest.mark.parametrize("name", TARGETS)
def test_k_loop_of_the_256_row_workgroups(census, name):
    c = census[name]
    print(name, c["classes"], c["valu_opcodes"], c["registers"])
    ops = c["opcodes"]
    assert c["classes"]["mfma"] == 192 and c["classes"]["lds_read"] == 72 and c["classes"]["lds_dma"] == 16, c["classes"]
    wide_adds = [o for o in ops if o.startswith("v_") and (o.endswith("_u64") or o.startswith("v_addc_co"))]
    assert not wide_adds, wide_adds                                    # no 64-bit vector integer add: addresses are 32-bit offsets
    assert ops.get("v_cvt_pk_bf16_f32", 0) <= 32, ops                  # one conversion per bf16 pair
    assert c["classes"]["valu"] <= 160, (c["classes"], c["valu_opcodes"])
    assert not [o for o in ops if o.startswith("s_and_saveexec")], ops  # no waterfall loop round a descriptor
    assert not [o for o in ops if o.startswith("scratch_")] and c["registers"]["scratch_bytes"] == 0, (ops, c["registers"])
    assert c["registers"]["vgpr_spill_count"] == 0 and c["registers"]["sgpr_spill_count"] == 0, c["registers"]


@pytest.mark.parametrize("name", HALF)
def test_128_row_workgroups_spill_no_more_than_they_did(census, name):
    """Four registers (16 bytes, outside the loop) before the change."""
    c = census[name]
    print(name, c["classes"], c["registers"])
    assert c["registers"]["vgpr_spill_count"] <= 4 and c["registers"]["sgpr_spill_count"] == 0, c["registers"]
    assert not [o for o in c["opcodes"] if o.startswith("scratch_")], c["opcodes"]
    assert not [o for o in c["opcodes"] if o.startswith("s_and_saveexec")], c["opcodes"]


def test_a_forced_workgroup_shape_shows_in_the_build_flags():
    """LSHRS_SIG16_HALF_MAX_TILES is read once per process: a child with it set, one without."""
    code = "from lshrs_amd import _native; print(int(_native.load().lshrs_build_flags()))"
    env = {k: v for k, v in os.environ.items() if k not in ("LSHRS_SIG16_HALF_MAX_TILES", "LSHRS_HIP_LIBRARY")}
    plain = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    forced = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, LSHRS_SIG16_HALF_MAX_TILES="0"),
                            capture_output=True, text=True)
    assert plain.returncode == 0 and forced.returncode == 0, plain.stderr + forced.stderr
    assert int(plain.stdout.split()[-1]) == 0
    assert int(forced.stdout.split()[-1]) == 0x2 | (1 << 25)
