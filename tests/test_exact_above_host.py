"""Host side of the range search (lshrs_amd.exact_above, LSHRS.recall_above): what is decided before any GPU call, the rounding
of the first pass's bars, the bookkeeping of recall_above on hand-made arrays, and the C entry's argument checks.  No GPU."""

from __future__ import annotations

import math

import numpy as np
import pytest


def test_names_are_exported():
    import lshrs_amd
    from lshrs_amd import DeviceVectors, LSHRS

    assert callable(lshrs_amd.exact_above) and "exact_above" in lshrs_amd.__all__
    assert callable(DeviceVectors.search_above) and callable(LSHRS.search_exact_above) and callable(LSHRS.recall_above)


@pytest.mark.parametrize("threshold", (float("nan"), float("inf"), -float("inf"), 1.0000001, -1.5, [0.2, float("nan"), 0.1],
                                       [0.2, 0.3], [[0.2, 0.3, 0.4]], np.zeros((3, 1)), [0.1, 0.2, 2.0]))
def test_bad_thresholds_raise_before_any_gpu_call(threshold, monkeypatch):
    from lshrs_amd import _exact, _native

    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were checked")

    monkeypatch.setattr(_native, "require_gpu", no_gpu)
    monkeypatch.setattr(_native, "load", no_gpu)
    with pytest.raises(ValueError, match="threshold"):
        _exact.exact_above(np.ones((3, 8), np.float32), None, threshold)


def test_negative_max_pairs_and_bad_queries_raise_before_any_gpu_call(monkeypatch):
    from lshrs_amd import _exact, _native

    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were checked")

    monkeypatch.setattr(_native, "require_gpu", no_gpu)
    monkeypatch.setattr(_native, "load", no_gpu)
    with pytest.raises(ValueError, match="max_pairs"):
        _exact.exact_above(np.ones((3, 8), np.float32), None, 0.5, max_pairs=-1)
    with pytest.raises(ValueError, match="queries"):
        _exact.exact_above(np.ones(8, np.float32), None, 0.5)
    # good arguments get as far as the GPU
    for threshold in (0.5, -1.0, 1.0, [0.0, 0.5, 1.0], np.float32(0.2)):
        with pytest.raises(AssertionError, match="the GPU was asked for"):
            _exact.exact_above(np.ones((3, 8), np.float32), None, threshold, max_pairs=0)


def test_thresholds_become_one_per_query():
    from lshrs_amd._exact import _check_above_args

    assert _check_above_args(4, 0.25, 10).tolist() == [0.25] * 4
    assert _check_above_args(3, [0.0, 0.5, 1.0], 0).tolist() == [0.0, 0.5, 1.0]
    assert _check_above_args(0, 0.3, 1).shape == (0,) and _check_above_args(0, [], 1).shape == (0,)


def test_bars_are_rounded_down():
    """float64(bar) <= t - margin for every threshold - also where the nearest float32 lies above - and within one float32
    step of it; the bar never lies above float32(t) - margin either, the threshold the answer is defined by."""
    from lshrs_amd._exact import above_bars, rerank_rounding

    rng = np.random.default_rng(0)
    t = np.concatenate([rng.uniform(-1.0, 1.0, 20000), [-1.0, 1.0, 0.0, 0.2, 0.75, np.nextafter(1.0, 0.0), 1e-30, -1e-30]])
    ups = 0
    for margin in (0.0, rerank_rounding(33) + 2.0 ** -13, 1e-4, 3.7e-3, 2.0 ** -7):
        bars = above_bars(t, margin)
        assert bars.dtype == np.float32 and bars.shape == t.shape
        b64 = bars.astype(np.float64)
        assert np.all(b64 <= t - margin)
        assert np.all(b64 <= t.astype(np.float32).astype(np.float64) - margin)
        step = np.spacing(np.abs(bars)).astype(np.float64)
        assert np.all(t - margin - b64 <= 4.0 * step + 2.0 ** -24)
        ups += int(np.sum((t - margin).astype(np.float32).astype(np.float64) > t - margin))
    assert ups > 1000                                   # (the nearest float32 was above for many: rounding down was exercised)
    assert above_bars(np.array([0.5]), 0.0).tolist() == [0.5]


def test_recall_above_bookkeeping():
    from lshrs_amd._exact import above_recall

    # query 0: truth {1, 2, 3}, candidates {2, 3, 9, 10}; query 1: no truth, candidates {5}; query 2: truth {7}, no candidates;
    # query 3: truth {4, 6}, candidates {6, 4}
    t_ids = np.array([3, 1, 2, 7, 4, 6], dtype=np.int64)
    t_scores = np.array([0.9, 0.8, 0.8, 1.0, 0.5, 0.0], dtype=np.float32)
    t_bounds = np.array([0, 3, 3, 4, 6], dtype=np.int64)
    c_ids = np.array([10, 2, 9, 3, 5, 6, 4], dtype=np.int64)
    c_bounds = np.array([0, 4, 5, 5, 7], dtype=np.int64)
    b, r = 4, 2
    got = above_recall(t_ids, t_scores, t_bounds, c_ids, c_bounds, b, r)
    assert got["truth_pairs"] == 6 and got["recall"] == 4 / 6 and got["precision"] == 4 / 7 and got["candidates"] == 7 / 4
    per = got["per_query"]
    assert per.dtype == np.float32 and per.shape == (4,) and math.isnan(per[1])
    assert per[[0, 2, 3]].tolist() == [np.float32(2 / 3), 0.0, 1.0]
    want = np.mean([1 - (1 - (1 - math.acos(float(s)) / math.pi) ** r) ** b for s in t_scores.tolist()])
    assert abs(got["expected"] - want) <= 1e-12 and 0.0 <= got["expected"] <= 1.0
    # the law's corners: a cosine of 1 always collides; one band of one bit at a cosine of 0 collides half the time
    assert above_recall([1], [1.0], [0, 1], [1], [0, 1], 3, 5)["expected"] == 1.0
    assert above_recall([1], [0.0], [0, 1], [], [0, 0], 1, 1)["expected"] == pytest.approx(0.5)
    assert above_recall([1], [1.0000001], [0, 1], [], [0, 0], 1, 1)["expected"] == 1.0      # (a score a rounding above 1)
    # nothing is similar: recall 1, precision 0 of what collided; nothing at all: both 1
    none = above_recall([], [], [0, 0, 0], [4, 5], [0, 1, 2], b, r)
    assert none["recall"] == 1.0 and none["precision"] == 0.0 and none["truth_pairs"] == 0 and math.isnan(none["expected"])
    assert np.isnan(none["per_query"]).all()
    empty = above_recall([], [], [0], [], [0], b, r)
    assert empty["recall"] == 1.0 and empty["precision"] == 1.0 and empty["candidates"] == 0.0 and empty["per_query"].shape == (0,)
    with pytest.raises(ValueError):
        above_recall([], [], [0, 0], [], [0], b, r)


def test_c_entry_checks_its_arguments_on_the_host():
    """Limits and status codes of lshrs_scan_above_*: those of lshrs_scan_topk_*, decided before anything touches a device."""
    from lshrs_amd import _native

    _native.build()
    lib = _native.load()
    size = lib.lshrs_scan_above_workspace_bytes
    # the query image (16 KiB per tile of 64 queries and chunk of 64 elements) + a norm per padded query + 16
    assert size(37, 6000, 100) == 1 * 2 * 16384 + 64 * 4 + 16
    assert size(65, 20011, 772) == 2 * 13 * 16384 + 128 * 4 + 16
    assert size(0, 10, 16) == 16
    assert size(1, 10, 16384) > 0 and size(1, 10, 16385) == _native.E_TOOLARGE
    assert size(1, (1 << 31) - 1, 16) > 0 and size(1, 1 << 31, 16) == _native.E_TOOLARGE
    assert size(1, 0, 16) == _native.E_BADARG and size(-1, 10, 16) == _native.E_BADARG and size(1, 10, 0) == _native.E_BADARG
    buf = np.zeros(80, dtype=np.int64)
    p = (buf.ctypes.data + 15) // 16 * 16              # (16-byte aligned, with room behind it)
    assert p % 16 == 0
    for dt in _native.SCAN_ELEMS:
        fn = getattr(lib, "lshrs_scan_above_" + dt)
        assert fn(None, 10, 16, 16, None, None, 0, None, 0, None, None, None, None, None, None, None) == 0      # q == 0
        assert fn(p, 10, 16, 16385, None, p, 3, p, 0, None, None, None, p, p, None, None) == _native.E_TOOLARGE
        assert fn(p, 1 << 31, 16, 16, None, p, 3, p, 0, None, None, None, p, p, None, None) == _native.E_TOOLARGE
        assert fn(p, 10, 16, 16, None, p, 3, p, -1, None, None, None, p, p, None, None) == _native.E_BADARG    # capacity < 0
        assert fn(None, 10, 16, 16, None, p, 3, p, 0, None, None, None, p, p, None, None) == _native.E_BADARG
        assert fn(p, 10, 16, 16, None, p, 3, None, 0, None, None, None, p, p, None, None) == _native.E_BADARG   # no bars
        assert fn(p, 10, 16, 16, None, p, 3, p, 0, None, None, None, None, p, None, None) == _native.E_BADARG   # no total
        assert fn(p, 10, 16, 16, None, p, 3, p, 5, None, None, None, p, p, None, None) == _native.E_BADARG      # slots, no arrays
        assert fn(p, 10, 16, 16, None, p, 3, p, 0, None, None, None, p + 4, p, None, None) == _native.E_BADARG  # total misaligned
        assert fn(p, 10, 16, 16, None, p, 3, p, 0, None, None, None, p, p + 8, None, None) == _native.E_BADARG  # workspace
        assert fn(p, 10, 8, 16, None, p, 3, p, 0, None, None, None, p, p, None, None) == _native.E_BADARG       # ldc < dim
