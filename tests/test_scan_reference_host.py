"""What of tests/_scan_reference.py needs no GPU: `expected_windows` on hand-made scores, and the geometry the GPU cases of
tests/test_gpu_scan_selection.py rely on, read out of the built library (`plan`) - so that a later change of the slice plan
cannot quietly stop those cases from reaching the clamp, the merge size or the prune form they were written for."""

from __future__ import annotations

import numpy as np
import pytest

from lshrs_amd import _native
from tests import _scan_reference as R

NEG_INF = np.float32("-inf")


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def _bits(values):
    return np.asarray(values, dtype=np.float32).view(np.uint32)


def test_scan_keys_order_the_bits_not_the_values():
    vals = np.array([np.inf, 1.0, 2.0 ** -140, 0.0, -0.0, -(2.0 ** -140), -1.0, -np.inf], dtype=np.float32)
    keys = R.scan_keys(vals.view(np.uint32)).astype(np.int64)
    assert np.all(np.diff(keys) < 0)                        # strictly descending: +0.0 above -0.0
    assert keys[3] == 0x80000000 and keys[4] == 0x7FFFFFFF and keys[-1] == 0x007FFFFF and keys.min() > 0


def test_expected_windows_ties_zeros_nan_dead_and_padding():
    nan = np.float32("nan")
    #            row: 0     1     2     3     4     5     6     7
    A = np.array([[0.5, 0.75, 0.5, 0.75, 0.25, 0.5, -1.0, 0.75],          # ties, broken by ascending row
                  [-0.0, 0.0, -0.0, 0.0, -0.5, 0.0, -0.0, 0.5],           # +0.0 ahead of -0.0
                  [0.9, nan, 0.8, nan, 0.7, nan, nan, 0.6],               # NaN left out
                  [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8],               # (dead rows below)
                  [nan, nan, nan, nan, nan, nan, nan, nan]], dtype=np.float32)
    rows, bits, count = R.expected_windows(A, None, 4)
    assert rows.dtype == np.int64 and bits.dtype == np.uint32 and count.dtype == np.int32
    assert rows[0].tolist() == [1, 3, 7, 0] and bits[0].tolist() == _bits([0.75, 0.75, 0.75, 0.5]).tolist()
    assert rows[1].tolist() == [7, 1, 3, 5] and bits[1].tolist() == _bits([0.5, 0.0, 0.0, 0.0]).tolist()
    assert rows[2].tolist() == [0, 2, 4, 7] and count[:3].tolist() == [4, 4, 4]
    assert rows[4].tolist() == [-1] * 4 and bits[4].tolist() == [R.NEG_INF_BITS] * 4 and count[4] == 0
    # the zeros one place further: -0.0 rows follow every +0.0 row, in ascending row
    rows, bits, count = R.expected_windows(A, None, 8)
    assert rows[1].tolist() == [7, 1, 3, 5, 0, 2, 6, 4]
    assert bits[1].tolist() == _bits([0.5, 0.0, 0.0, 0.0, -0.0, -0.0, -0.0, -0.5]).tolist()
    assert rows[2].tolist() == [0, 2, 4, 7, -1, -1, -1, -1] and count[2] == 4           # fewer rows than the window: padded
    assert bits[2, 4:].tolist() == [R.NEG_INF_BITS] * 4 and np.float32(NEG_INF).view(np.uint32) == R.NEG_INF_BITS
    # dead rows left out, whatever they score; a window wider than the block
    live = np.array([1, 1, 0, 1, 1, 0, 1, 0], dtype=bool)
    rows, bits, count = R.expected_windows(A, live, 3)
    assert rows[3].tolist() == [6, 4, 3] and rows[0].tolist() == [1, 3, 0] and rows[2].tolist() == [0, 4, -1]
    assert count.tolist() == [3, 3, 2, 3, 0]
    rows, bits, count = R.expected_windows(A, live, 12)
    assert rows.shape == (5, 12) and count.tolist() == [5, 5, 2, 5, 0]
    assert rows[3].tolist() == [6, 4, 3, 1, 0] + [-1] * 7 and bits[3, 5:].tolist() == [R.NEG_INF_BITS] * 7
    assert rows[1].tolist() == [1, 3, 0, 6, 4] + [-1] * 7
    # a real -inf score is an item like any other (its key is above 0): only the count tells it from padding
    B = np.array([[NEG_INF, 1.0, nan]], dtype=np.float32)
    rows, bits, count = R.expected_windows(B, None, 3)
    assert rows[0].tolist() == [1, 0, -1] and count[0] == 2 and bits[0, 1] == R.NEG_INF_BITS


def test_narrower_windows_are_the_first_columns():
    rng = np.random.default_rng(4)
    A = rng.standard_normal((9, 300)).astype(np.float32)
    A[:, ::7] = A[:, 1::7]                                  # ties
    A[3, 5:] = np.nan
    live = rng.random(300) < 0.5
    wide = R.expected_windows(A, live, 128)
    for w in (1, 2, 3, 33, 64, 100, 127, 128):
        a, b = R.narrower(wide, w), R.expected_windows(A, live, w)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), w
    rows, bits, count = wide
    for i in range(9):                                      # against a plain Python sort of (key, row)
        cand = [(-int(R.scan_keys(A[i, j:j + 1].view(np.uint32))[0]), j) for j in range(300) if live[j] and A[i, j] == A[i, j]]
        want = [j for _, j in sorted(cand)][:128]
        assert rows[i, :count[i]].tolist() == want and count[i] == min(128, len(cand))


# ------------------------------------------------------------------------------------------
# geometry: csrc/scan.hip's scan_slices / scan_plan restated, and held against the library
# ------------------------------------------------------------------------------------------
def _model(q, m, dim, window):
    """(slices, rows per slice, cap, which bound gave the slice count) as scan_plan has them."""
    cap = R.selection_cap(window)
    lds = R.CHUNK_BYTES + R.QTILE * cap * 8 + R.QTILE * 12
    resident = 256 * (2 if 2 * lds <= 160 * 1024 else 1)
    qtiles = -(-q // R.QTILE)
    bounds = {"resident": resident // qtiles, "rows": -(-m // 1024), "limit": R.MERGE_ITEMS // window}
    why = min(bounds, key=lambda k: bounds[k])
    want = bounds[why]
    if want < 1:
        want, why = 1, "floor"
    passes = -(-m // 256)
    rps = -(-passes // want) * 256
    return -(-m // rps), rps, cap, why, bounds


# (q, m, dim, window) -> slices, merge items, padded merge items: the cases of tests/test_gpu_scan_selection.py::GEOMETRY
TABLE = (((5, 81_919, 16, 128), 64, 8192, 8192),
         ((70, 81_920, 16, 127), 64, 8128, 8192),
         ((5, 131_071, 16, 64), 128, 8192, 8192),
         ((5, 131_071, 16, 33), 128, 4224, 8192),
         ((16_449, 300, 16, 128), 1, 128, 128),
         ((6_400, 3_000, 16, 128), 2, 256, 256),
         ((7, 1_025, 16, 3), 2, 6, 8))


def test_the_geometry_the_gpu_cases_rely_on(lib):
    from tests.test_gpu_scan_selection import GEOMETRY

    assert tuple(shape for shape, *_ in TABLE) == tuple(GEOMETRY)
    for shape, slices, n, npad in TABLE:
        assert R.plan(lib, *shape) == slices == _model(*shape)[0], shape
        assert R.merge_items(slices, shape[3]) == (n, npad), shape

    # 1: the `limit` clamp binds (rows and residency would both allow more); the merge runs at its full 64 KiB, above the
    #    48 KiB beyond which it asks for the attribute; the last slice is one row short of its fifth pass
    slices, rps, cap, why, bounds = _model(5, 81_919, 16, 128)
    assert why == "limit" and bounds["rows"] > 64 and bounds["resident"] > 64 and cap == 256
    assert 8192 * 8 == 64 * 1024 > 48 * 1024 and 81_919 - (slices - 1) * rps == 1279 == 5 * 256 - 1
    # 2: the same with two query tiles, the second of 6 queries; 64 zero items pad the network
    slices, rps, cap, why, bounds = _model(70, 81_920, 16, 127)
    assert why == "limit" and -(-70 // 64) == 2 and 70 - 64 == 6 and 8192 - slices * 127 == 64 and cap == 256
    # 3, 4: cap = 128 (scan_prune_n<2>), at the merge's full size and at a window that is no power of two
    for window in (64, 33):
        slices, rps, cap, why, bounds = _model(5, 131_071, 16, window)
        assert cap == 128 and slices == 128 and R.merge_items(slices, window)[1] == 8192
    assert _model(5, 131_071, 16, 64)[4]["limit"] == 128       # (the clamp and the rows agree on 128)
    # 5: more query tiles than resident workgroups: resident / qtiles is 0, raised to one slice
    slices, rps, cap, why, bounds = _model(16_449, 300, 16, 128)
    assert -(-16_449 // 64) == 258 > 256 and bounds["resident"] == 0 and why == "floor" and slices == 1
    # 6: resident / qtiles decides
    slices, rps, cap, why, bounds = _model(6_400, 3_000, 16, 128)
    assert why == "resident" and bounds["resident"] == 2 < bounds["rows"] == 3 and slices == 2
    # 7: the smallest merge; the second slice is one row past a pass
    slices, rps, cap, why, bounds = _model(7, 1_025, 16, 3)
    assert (slices, rps) == (2, 768) and 1_025 - rps == 257 and cap == 64


def test_the_plan_is_the_model_over_a_sweep(lib):
    for q in (1, 64, 65, 70, 6_400, 16_449):
        for m in (1, 255, 256, 257, 1_024, 1_025, 5_000, 6_000, 81_919, 131_071, 1_000_000):
            for window in (1, 2, 3, 31, 32, 33, 64, 65, 100, 127, 128):
                for dim in (16, 33, 200):
                    assert R.plan(lib, q, m, dim, window) == _model(q, m, dim, window)[0], (q, m, dim, window)


def test_the_geometry_of_the_small_data_sets(lib):
    """The data sets of tests/test_gpu_scan_selection.py: 5 000 (6 000) rows are five (six) slices of 1 024 rows at every
    window, so that rows 1024..2047 are exactly one slice (S5 b: a slice without winners); the windows tried cover all three
    forms of the prune (cap 64, 128, 256) and both sides of each threshold."""
    from tests.test_gpu_scan_selection import SMALL_M, WINDOWS

    for window in WINDOWS:
        assert _model(70, 5_000, 33, window)[:2] == (5, 1024) and R.plan(lib, 70, 5_000, 33, window) == 5
        assert R.plan(lib, 70, 6_000, 33, window) == 6
    caps = [R.selection_cap(w) for w in WINDOWS]
    assert set(caps) == {64, 128, 256}
    assert [R.selection_cap(w) for w in (32, 33, 64, 65)] == [64, 128, 128, 256]
    assert {32, 33, 64, 65, 1, 128} <= set(WINDOWS)
    for m in SMALL_M:
        for window in (1, 33, 128):
            assert R.plan(lib, 7, m, 16, window) == (2 if m == 1_025 else 1)
