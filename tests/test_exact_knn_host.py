"""Host side of the k-NN self-join (lshrs_amd.exact_knn, lshrs_scan_knn_*): the exports and where they are declared, the
workspace's arithmetic, the C entries' argument checks and what exact_knn decides before any GPU call.  No GPU."""

from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

KNN_EXPORTS = ("lshrs_scan_knn_workspace_bytes", "lshrs_scan_knn_f32", "lshrs_scan_knn_bf16", "lshrs_scan_knn_f16",
               "lshrs_scan_knn_i8", "lshrs_scan_knn_f8e4m3")


def _lib():
    from lshrs_amd import _native

    _native.build()
    return _native.load()


def test_names_are_exported():
    import lshrs_amd
    from lshrs_amd import DeviceVectors, LSHRS, _exact

    assert callable(lshrs_amd.exact_knn) and "exact_knn" in lshrs_amd.__all__
    assert callable(_exact.scan_knn) and "scan_knn" in _exact.__all__ and "exact_knn" in _exact.__all__
    assert callable(DeviceVectors.neighbors) and callable(LSHRS.neighbors_exact)


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lshrs_[a-z0-9_]+)\s*\(", text)))


def test_the_six_entries_are_in_their_header_their_tuple_and_the_library():
    from lshrs_amd import _native

    lib = _lib()
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _native.LIBRARY], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (lshrs_\w+)", dynamic))
    assert _declared(os.path.join(_native.INCLUDE, "lshrs_knn.h")) == sorted(KNN_EXPORTS) == sorted(_native.EXPORTS_KNN)
    assert '#include "lshrs_hip.h"' in open(os.path.join(_native.INCLUDE, "lshrs_knn.h")).read()
    for name in KNN_EXPORTS:
        assert name in exported and hasattr(lib, name), name
        assert name not in _native.EXPORTS
    # the first header and its tuple are what they were
    assert _declared(os.path.join(_native.INCLUDE, "lshrs_hip.h")) == sorted(_native.EXPORTS)
    assert len(_native.EXPORTS) == 75 == len(set(_native.EXPORTS)) and len(set(_native.EXPORTS_KNN)) == 6
    assert lib.lshrs_abi_version() == 7 == _native.ABI_VERSION


def _slices(m, qtiles, window):
    """The slices of m rows one block of `qtiles` query tiles scans: one round of the workgroups resident at a time - 256 CUs,
    two per CU while their LDS (a 16 KiB chunk of the image, 64 buffers of cap = max(64, the power of two at or above 2 x
    window) 8-byte items, 12 bytes per query) fits twice into 160 KiB, else one - at least 1024 rows each, no more than a merge
    workgroup sorts (8192 items / window); in whole passes of 256."""
    cap = 64
    while cap < 2 * window:
        cap <<= 1
    resident = 512 if 2 * (16384 + 64 * cap * 8 + 768) <= 160 * 1024 else 256
    want = max(1, min(resident // qtiles, -(-m // 1024), 8192 // window))
    rps = -(-(-(-m // 256)) // want) * 256
    return -(-m // rps)


def _want_bytes(q_count, m, dim, window, qblock):
    """lshrs_scan_knn_workspace_bytes restated: the image of one block (16 KiB per tile and chunk), a norm per row of it, the
    slices' winners of the block that has most (block rows x slices x window x 8), and 16."""
    chunks = -(-dim // 64)
    if qblock:
        tiles = qblock // 64
    else:
        tiles = min(8192 // 64, (256 << 20) // (chunks * 16384), -(-max(q_count, 1) // 64))
    block = tiles * 64
    parts = 0
    for qn in (min(q_count, block), q_count % block):
        if qn:
            parts = max(parts, qn * _slices(m, -(-qn // 64), window) * window * 8)
    return tiles * chunks * 16384 + block * 4 + parts + 16


def test_workspace_bytes():
    from lshrs_amd import _native

    size = _lib().lshrs_scan_knn_workspace_bytes
    # by hand: one block of 11 tiles, one slice (700 rows are less than 1024)
    assert size(700, 700, 100, 16, 0) == 11 * 2 * 16384 + 704 * 4 + 700 * 1 * 16 * 8 + 16
    # a forced block of 64: the first block has the most winners (64 rows; the last has 60)
    assert size(700, 700, 100, 16, 64) == 2 * 16384 + 256 + 64 * 16 * 8 + 16
    # 200 000 x 768: blocks of 8192 rows, 128 tiles, four slices at two workgroups per CU; the last block (3392 rows, 53
    # tiles) has nine, still fewer winners; a window of 64 leaves room for one workgroup per CU: two slices
    assert _slices(200000, 128, 32) == 4 and _slices(200000, 53, 32) == 9 and _slices(200000, 128, 64) == 2
    assert size(200000, 200000, 768, 32, 0) == 128 * 12 * 16384 + 8192 * 4 + 8192 * 4 * 32 * 8 + 16
    assert size(200000, 200000, 768, 64, 0) == 128 * 12 * 16384 + 8192 * 4 + 8192 * 2 * 64 * 8 + 16
    for shape in ((700, 700, 100, 16, 0), (700, 700, 100, 16, 64), (700, 700, 100, 128, 128), (100, 257, 17, 1, 0),
                  (100, 257, 17, 1, 64), (1, 1, 1, 1, 0), (2, 2, 64, 128, 0), (33, 33, 768, 16, 0), (200000, 200000, 768, 32, 0),
                  (8192, 200000, 768, 32, 0), (200000, 200000, 768, 128, 0), (5000, 1 << 20, 16384, 64, 0),
                  (70000, 1 << 20, 8191, 8, 0), (3000, 100000, 100, 128, 1024), (64, 5000, 64, 64, 64), (0, 10, 16, 16, 0)):
        assert size(*shape) == _want_bytes(*shape), shape
    # what it refuses
    assert size(-1, 10, 16, 16, 0) == _native.E_BADARG and size(11, 10, 16, 16, 0) == _native.E_BADARG
    assert size(5, 0, 16, 16, 0) == _native.E_BADARG and size(0, 0, 16, 16, 0) == _native.E_BADARG
    assert size(5, 10, 0, 16, 0) == _native.E_BADARG and size(5, 10, -1, 16, 0) == _native.E_BADARG
    for window in (0, -1, 129):
        assert size(5, 10, 16, window, 0) == _native.E_BADARG, window
    assert size(5, 10, 16, 128, 0) > 0
    for qblock in (1, 63, 65, 100, -64, -1):
        assert size(5, 10, 16, 16, qblock) == _native.E_BADARG, qblock
    assert size(5, 10, 16384, 16, 0) > 0 and size(5, 10, 16385, 16, 0) == _native.E_TOOLARGE
    assert size(5, (1 << 31) - 1, 16, 16, 0) > 0 and size(5, 1 << 31, 16, 16, 0) == _native.E_TOOLARGE
    assert size(5, 10, 16, 16, 65535 * 64) > 0 and size(5, 10, 16, 16, 65536 * 64) == _native.E_TOOLARGE


def test_c_entries_check_their_arguments_on_the_host():
    """Status codes of lshrs_scan_knn_*: those of lshrs_scan_topk_* / lshrs_scan_pairs_*, decided before anything touches a
    device (there is none here)."""
    from lshrs_amd import _native

    lib = _lib()
    buf = np.zeros(80, dtype=np.int64)
    p = (buf.ctypes.data + 15) // 16 * 16              # (16-byte aligned, with room behind it)
    for dt in _native.SCAN_ELEMS:
        fn = getattr(lib, "lshrs_scan_knn_" + dt)
        #        corpus m  ldc dim row_ids q_begin q_count window qblock rows approx count ws err stream
        assert fn(p, 10, 16, 16385, None, 0, 5, 16, 0, p, p, p, p, None, None) == _native.E_TOOLARGE
        assert fn(p, 1 << 31, 16, 16, None, 0, 5, 16, 0, p, p, p, p, None, None) == _native.E_TOOLARGE
        assert fn(p, 10, 16, 16, None, 0, 5, 16, 65536 * 64, p, p, p, p, None, None) == _native.E_TOOLARGE
        assert fn(p, 0, 16, 16, None, 0, 0, 16, 0, p, p, p, p, None, None) == _native.E_BADARG          # no rows
        assert fn(p, 10, 16, 0, None, 0, 5, 16, 0, p, p, p, p, None, None) == _native.E_BADARG
        assert fn(p, 10, 16, 16, None, 0, -1, 16, 0, p, p, p, p, None, None) == _native.E_BADARG        # q_count < 0
        assert fn(p, 10, 16, 16, None, -1, 5, 16, 0, p, p, p, p, None, None) == _native.E_BADARG        # q_begin < 0
        assert fn(p, 10, 16, 16, None, 6, 5, 16, 0, p, p, p, p, None, None) == _native.E_BADARG         # a range beyond m
        assert fn(p, 10, 16, 16, None, 0, 11, 16, 0, p, p, p, p, None, None) == _native.E_BADARG
        assert fn(p, 10, 16, 16, None, 0, 5, 0, 0, p, p, p, p, None, None) == _native.E_BADARG          # window
        assert fn(p, 10, 16, 16, None, 0, 5, 129, 0, p, p, p, p, None, None) == _native.E_BADARG
        assert fn(p, 10, 16, 16, None, 0, 5, 16, 100, p, p, p, p, None, None) == _native.E_BADARG       # qblock % 64
        assert fn(p, 10, 16, 16, None, 0, 5, 16, -64, p, p, p, p, None, None) == _native.E_BADARG
        assert fn(None, 10, 16, 16, None, 0, 5, 16, 0, p, p, p, p, None, None) == _native.E_BADARG      # no corpus
        assert fn(p, 10, 16, 16, None, 0, 5, 16, 0, None, p, p, p, None, None) == _native.E_BADARG      # no out_rows
        assert fn(p, 10, 16, 16, None, 0, 5, 16, 0, p, None, p, p, None, None) == _native.E_BADARG      # no out_approx
        assert fn(p, 10, 16, 16, None, 0, 5, 16, 0, p, p, None, p, None, None) == _native.E_BADARG      # no out_count
        assert fn(p, 10, 16, 16, None, 0, 5, 16, 0, p, p, p, None, None, None) == _native.E_BADARG      # no workspace
        assert fn(p, 10, 16, 16, None, 0, 5, 16, 0, p + 4, p, p, p, None, None) == _native.E_BADARG     # out_rows misaligned
        assert fn(p, 10, 16, 16, None, 0, 5, 16, 0, p, p + 2, p, p, None, None) == _native.E_BADARG     # out_approx
        assert fn(p, 10, 16, 16, None, 0, 5, 16, 0, p, p, p + 2, p, None, None) == _native.E_BADARG     # out_count
        assert fn(p, 10, 16, 16, None, 0, 5, 16, 0, p, p, p, p + 8, None, None) == _native.E_BADARG     # workspace
        assert fn(p, 10, 16, 16, p + 4, 0, 5, 16, 0, p, p, p, p, None, None) == _native.E_BADARG        # row_ids
        assert fn(p, 10, 16, 16, None, 0, 5, 16, 0, p, p, p, p, p + 2, None) == _native.E_BADARG        # err
        assert fn(p, 10, 8, 16, None, 0, 5, 16, 0, p, p, p, p, None, None) == _native.E_BADARG          # ldc < dim
        # no query rows: nothing to do, whatever the arrays are - but the rest is still checked
        assert fn(p, 10, 16, 16, None, 0, 0, 16, 0, None, None, None, None, None, None) == 0
        assert fn(p, 10, 16, 16, None, 10, 0, 16, 0, None, None, None, None, None, None) == 0
        assert fn(p, 10, 16, 16, None, 11, 0, 16, 0, None, None, None, None, None, None) == _native.E_BADARG
        assert fn(p, 10, 16, 16, None, 0, 0, 0, 0, None, None, None, None, None, None) == _native.E_BADARG


@pytest.mark.parametrize("k, method", ((0, "auto"), (-3, "scan"), (5, "fast"), (5, None), (0, "gather")))
def test_bad_arguments_raise_before_any_gpu_call(k, method, monkeypatch):
    from lshrs_amd import _exact, _native

    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were checked")

    monkeypatch.setattr(_native, "require_gpu", no_gpu)
    monkeypatch.setattr(_native, "load", no_gpu)
    with pytest.raises(ValueError, match="k must be > 0|method must be"):
        _exact.exact_knn(None, k, method=method)


def test_good_arguments_get_as_far_as_the_gpu(monkeypatch):
    from lshrs_amd import _exact, _native

    def no_gpu():
        raise AssertionError("the GPU was asked for")

    monkeypatch.setattr(_native, "require_gpu", no_gpu)
    monkeypatch.setattr(_native, "load", no_gpu)
    for method in ("auto", "scan", "gather"):
        with pytest.raises(AssertionError, match="the GPU was asked for"):
            _exact.exact_knn(None, 3, method=method)


def test_chunks_are_whole_blocks_within_the_budget():
    from lshrs_amd import _exact

    budget = _exact._PAIRS_QUERY_BYTES
    for block, dim, window in ((8192, 768, 32), (8192, 1, 1), (4096, 16384, 128), (64, 100, 16), (8192, 16384, 128)):
        chunk = _exact._knn_chunk(block, dim, window)
        assert chunk >= block and chunk % block == 0
        assert chunk == block or chunk * (4 * dim + 16 * window) <= budget
        assert (chunk + block) * (4 * dim + 16 * window) > budget
    assert _exact._knn_chunk(8192, 768, 32) == 9 * 8192
