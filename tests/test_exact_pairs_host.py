"""Host side of the self-join (lshrs_amd.exact_pairs_above, lshrs_scan_pairs_*): the exports, the workspace's arithmetic, the C
entry's argument checks and what exact_pairs_above decides before any GPU call.  No GPU."""

from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

PAIRS_EXPORTS = ("lshrs_scan_pairs_workspace_bytes", "lshrs_scan_pairs_f32", "lshrs_scan_pairs_bf16", "lshrs_scan_pairs_f16",
                 "lshrs_scan_pairs_i8", "lshrs_scan_pairs_f8e4m3")


def _lib():
    from lshrs_amd import _native

    _native.build()
    return _native.load()


def test_names_are_exported():
    import lshrs_amd
    from lshrs_amd import DeviceVectors, LSHRS, _exact

    assert callable(lshrs_amd.exact_pairs_above) and "exact_pairs_above" in lshrs_amd.__all__
    assert callable(_exact.scan_pairs) and "scan_pairs" in _exact.__all__
    assert callable(DeviceVectors.pairs_above) and callable(LSHRS.pairs_exact_above)


def test_the_six_exports_are_in_the_header_the_binding_and_the_library():
    from lshrs_amd import _native

    lib = _lib()
    header = open(os.path.join(_native.INCLUDE, "lshrs_hip.h")).read()
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _native.LIBRARY], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (lshrs_\w+)", dynamic))
    for name in PAIRS_EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _native.EXPORTS and name in exported and hasattr(lib, name), name
    assert lib.lshrs_abi_version() == 7 == _native.ABI_VERSION
    assert len(_native.EXPORTS) == 75 == len(set(_native.EXPORTS))


def test_workspace_bytes():
    from lshrs_amd import _native

    size = _lib().lshrs_scan_pairs_workspace_bytes
    # a forced block: its image (16 KiB per tile of 64 rows and chunk of 64 elements - the size knows no element type, so it
    # is the two-term image's; the one-term types use half of it) + a norm per row of the block + 16, whatever m is
    assert size(700, 100, 64) == 1 * 2 * 16384 + 64 * 4 + 16
    assert size(700, 100, 128) == 2 * 2 * 16384 + 128 * 4 + 16
    assert size(5, 100, 128) == 2 * 2 * 16384 + 128 * 4 + 16
    assert size(20011, 772, 1024) == 16 * 13 * 16384 + 1024 * 4 + 16
    assert size(1, 1, 64) == 16384 + 256 + 16
    # the planned block: 8192 rows, no more than the rows (in whole tiles), no more tiles than an image of 256 MiB holds
    assert size(700, 100, 0) == 11 * 2 * 16384 + 704 * 4 + 16
    assert size(1, 16, 0) == size(64, 16, 0) == 16384 + 256 + 16
    assert size(200000, 768, 0) == size(8192, 768, 0) == 128 * 12 * 16384 + 8192 * 4 + 16
    assert size(1 << 20, 16384, 0) == 64 * 256 * 16384 + 4096 * 4 + 16         # (4 MiB a tile: 64 tiles are 256 MiB)
    assert size(1 << 20, 16384, 0) - 4096 * 4 - 16 == 256 << 20
    assert size(1 << 20, 8191, 0) - 8192 * 4 - 16 == 256 << 20                 # (128 chunks: 128 tiles, the whole block)
    # what it refuses
    assert size(0, 16, 0) == _native.E_BADARG and size(-3, 16, 64) == _native.E_BADARG
    assert size(10, 0, 0) == _native.E_BADARG and size(10, -1, 0) == _native.E_BADARG
    assert size(10, 16384, 0) > 0 and size(10, 16385, 0) == _native.E_TOOLARGE
    assert size((1 << 31) - 1, 16, 0) > 0 and size(1 << 31, 16, 0) == _native.E_TOOLARGE
    for qblock in (1, 63, 65, 100, -64, -1):
        assert size(10, 16, qblock) == _native.E_BADARG, qblock
    assert size(10, 16, 65535 * 64) > 0 and size(10, 16, 65536 * 64) == _native.E_TOOLARGE


def test_c_entry_checks_its_arguments_on_the_host():
    """Status codes of lshrs_scan_pairs_*: those of lshrs_scan_above_*, decided before anything touches a device."""
    from lshrs_amd import _native

    lib = _lib()
    buf = np.zeros(80, dtype=np.int64)
    p = (buf.ctypes.data + 15) // 16 * 16              # (16-byte aligned, with room behind it)
    assert p % 16 == 0
    for dt in _native.SCAN_ELEMS:
        fn = getattr(lib, "lshrs_scan_pairs_" + dt)
        #        corpus m  ldc dim row_ids bar qblock capacity a  b  approx total ws err stream
        assert fn(p, 10, 16, 16385, None, 0.5, 0, 0, None, None, None, p, p, None, None) == _native.E_TOOLARGE
        assert fn(p, 1 << 31, 16, 16, None, 0.5, 0, 0, None, None, None, p, p, None, None) == _native.E_TOOLARGE
        assert fn(p, 0, 16, 16, None, 0.5, 0, 0, None, None, None, p, p, None, None) == _native.E_BADARG       # no rows
        assert fn(p, 10, 16, 0, None, 0.5, 0, 0, None, None, None, p, p, None, None) == _native.E_BADARG
        assert fn(p, 10, 16, 16, None, 0.5, 100, 0, None, None, None, p, p, None, None) == _native.E_BADARG    # qblock % 64
        assert fn(p, 10, 16, 16, None, 0.5, -64, 0, None, None, None, p, p, None, None) == _native.E_BADARG
        assert fn(p, 10, 16, 16, None, 0.5, 0, -1, None, None, None, p, p, None, None) == _native.E_BADARG     # capacity < 0
        assert fn(None, 10, 16, 16, None, 0.5, 0, 0, None, None, None, p, p, None, None) == _native.E_BADARG   # no corpus
        assert fn(p, 10, 16, 16, None, 0.5, 0, 0, None, None, None, None, p, None, None) == _native.E_BADARG   # no total
        assert fn(p, 10, 16, 16, None, 0.5, 0, 0, None, None, None, p, None, None, None) == _native.E_BADARG   # no workspace
        assert fn(p, 10, 16, 16, None, 0.5, 0, 5, None, None, None, p, p, None, None) == _native.E_BADARG      # slots, no arrays
        assert fn(p, 10, 16, 16, None, 0.5, 0, 5, p, None, p, p, p, None, None) == _native.E_BADARG            # ... no out_b
        assert fn(p, 10, 16, 16, None, 0.5, 0, 0, None, None, None, p + 4, p, None, None) == _native.E_BADARG  # total misaligned
        assert fn(p, 10, 16, 16, None, 0.5, 0, 0, None, None, None, p, p + 8, None, None) == _native.E_BADARG  # workspace
        assert fn(p, 10, 16, 16, None, 0.5, 0, 5, p + 4, p, p, p, p, None, None) == _native.E_BADARG           # out_a misaligned
        assert fn(p, 10, 16, 16, None, 0.5, 0, 5, p, p + 4, p, p, p, None, None) == _native.E_BADARG           # out_b misaligned
        assert fn(p, 10, 16, 16, None, 0.5, 0, 5, p, p, p + 2, p, p, None, None) == _native.E_BADARG           # out_approx
        assert fn(p, 10, 16, 16, p + 4, 0.5, 0, 0, None, None, None, p, p, None, None) == _native.E_BADARG     # row_ids
        assert fn(p, 10, 8, 16, None, 0.5, 0, 0, None, None, None, p, p, None, None) == _native.E_BADARG       # ldc < dim


@pytest.mark.parametrize("threshold", ([0.2, 0.3], [0.5], np.zeros((1, 1)), float("nan"), float("inf"), -float("inf"), 1.0000001,
                                       -1.5, "high", None))
def test_bad_thresholds_raise_before_any_gpu_call(threshold, monkeypatch):
    from lshrs_amd import _exact, _native

    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were checked")

    monkeypatch.setattr(_native, "require_gpu", no_gpu)
    monkeypatch.setattr(_native, "load", no_gpu)
    with pytest.raises(ValueError, match="threshold"):
        _exact.exact_pairs_above(None, threshold)


def test_negative_max_pairs_raises_before_any_gpu_call(monkeypatch):
    from lshrs_amd import _exact, _native

    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were checked")

    monkeypatch.setattr(_native, "require_gpu", no_gpu)
    monkeypatch.setattr(_native, "load", no_gpu)
    with pytest.raises(ValueError, match="max_pairs"):
        _exact.exact_pairs_above(None, 0.5, max_pairs=-1)
    # good arguments get as far as the GPU
    for threshold in (0.5, -1.0, 1.0, np.float32(0.2), np.array(0.3)):
        with pytest.raises(AssertionError, match="the GPU was asked for"):
            _exact.exact_pairs_above(None, threshold, max_pairs=0)


def test_the_planned_block_is_read_out_of_the_workspace_size():
    from lshrs_amd._exact import _pairs_block

    lib = _lib()
    assert _pairs_block(lib, 700, 100) == 704 and _pairs_block(lib, 1, 7) == 64
    assert _pairs_block(lib, 200000, 768) == 8192 and _pairs_block(lib, 1 << 20, 16384) == 4096
