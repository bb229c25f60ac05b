"""What of the exact search needs no GPU: the settle predicate, the window choice, the C ABI's pure host functions and the
argument checks that come before any device is touched."""

from __future__ import annotations

import numpy as np
import pytest

from lshrs_amd import _exact, _native


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def test_settle_predicate():
    eps = 1e-3
    # settled by the gap: the last approximate score of the window, plus epsilon, is no more than the k-th rescored score
    assert _exact.settled([32], 32, [0.60], [0.84], eps).tolist() == [True]
    assert _exact.settled([32], 32, [0.84 - eps], [0.84], eps).tolist() == [True]         # (<=: the boundary settles)
    # unsettled by epsilon: the window's tail is closer to s_k than the bound can tell apart
    assert _exact.settled([32], 32, [0.8395], [0.84], eps).tolist() == [False]
    assert _exact.settled([32], 32, [0.84], [0.84], eps).tolist() == [False]
    assert _exact.settled([32], 32, [0.8395], [0.84], 1e-4).tolist() == [True]            # (a tighter bound settles it)
    # settled because the window was not filled: every live row was seen, whatever the scores
    assert _exact.settled([31], 32, [float("-inf")], [0.1], eps).tolist() == [True]
    assert _exact.settled([5], 32, [0.99], [float("-inf")], eps).tolist() == [True]
    # a full window that holds fewer than k rows (k beyond the window): s_k = -inf, never settled
    assert _exact.settled([128], 128, [0.2], [float("-inf")], eps).tolist() == [False]
    # per query, and the sum is evaluated in float64 (float32 would round 1 + 2^-30 to 1)
    got = _exact.settled(np.array([32, 32, 7]), 32, np.array([0.5, 0.9, 0.9], np.float32), np.array([0.9, 0.9, 0.1], np.float32), eps)
    assert got.tolist() == [True, False, True] and got.dtype == bool
    assert _exact.settled([8], 8, [1.0], [1.0], 2.0 ** -30).tolist() == [False]


def test_rerank_rounding_is_added_to_epsilon():
    u = 2.0 ** -24
    for dim in (1, 100, 768, 16384):
        first_order = (dim / 32 + 23) * u               # the rerank kernel's own rounding (the settle rule)
        assert first_order < _exact.rerank_rounding(dim) <= (dim / 16 + 32) * u
    # a row left out whose cosine ties s_k within epsilon alone is not settled once the rerank's rounding is charged
    eps, dim = 1e-3, 768
    assert _exact.settled([32], 32, [0.84 - eps], [0.84], eps + _exact.rerank_rounding(dim)).tolist() == [False]


def test_window_choice(lib):
    top = int(lib.lshrs_scan_max_window())
    assert top >= 128
    assert [_exact.choose_window(k, top) for k in (1, 10, 64, 65, top)] == [2, 32, 128, top, top]
    assert _exact.choose_window(3, top) == 8 and _exact.choose_window(16, top) == 32 and _exact.choose_window(17, top) == 64
    for k in (1, 2, 3, 10, 33, 64):                    # a power of two, at least 2 k
        w = _exact.choose_window(k, top)
        assert w & (w - 1) == 0 and 2 * k <= w < 4 * k
    with pytest.raises(ValueError):
        _exact.choose_window(0, top)


def test_scan_entries_are_bound(lib):
    names = ["lshrs_scan_topk_" + s for s in _native.SCAN_ELEMS] + ["lshrs_scan_workspace_bytes", "lshrs_scan_max_window",
                                                                    "lshrs_scan_epsilon"]
    for name in names:
        assert name in _native.EXPORTS and hasattr(lib, name), name
    assert "scan" in _native.UNITS and lib.lshrs_abi_version() == 7
    for s in _native.SCAN_ELEMS[1:]:
        assert getattr(lib, "lshrs_scan_topk_" + s).argtypes == lib.lshrs_scan_topk_f32.argtypes


def test_epsilon_and_workspace_are_host_functions(lib):
    for elem in range(5):
        last = 0.0
        for dim in (1, 33, 100, 768, 1536, 4096, 16384):
            eps = float(lib.lshrs_scan_epsilon(elem, dim))
            assert last < eps <= 2.0 ** -7, (elem, dim, eps)         # grows with dim, never beyond what a first pass can use
            last = eps
    # one bf16 term per exact element type, two for f16 / f32: the same bound within each group, a larger one for two terms
    e = [float(lib.lshrs_scan_epsilon(elem, 768)) for elem in range(5)]
    assert e[1] == e[3] == e[4] < e[0] == e[2]
    # no smaller than its two leading terms: 2^-14 for the queries' split, products * 2^-23 for the f32 sums
    assert e[1] >= 2.0 ** -14 + 2 * 768 * 2.0 ** -23
    for bad in ((-1, 100), (5, 100), (0, 0), (1, 16385)):
        assert lib.lshrs_scan_epsilon(*bad) == -1.0
    assert _exact.scan_epsilon("bfloat16", 768) == e[1]
    with pytest.raises(ValueError):
        _exact.scan_epsilon("float64", 768)
    assert lib.lshrs_scan_workspace_bytes(256, 200_000, 768, 32) > 256 * 768 * 4
    assert lib.lshrs_scan_workspace_bytes(1, 1, 1, 1) > 0
    for bad in ((1, 0, 8, 8), (1, 8, 0, 8), (1, 8, 8, 0), (1, 8, 8, 129), (-1, 8, 8, 8)):
        assert lib.lshrs_scan_workspace_bytes(*bad) == _native.E_BADARG, bad
    assert lib.lshrs_scan_workspace_bytes(1, 1 << 31, 8, 8) == _native.E_TOOLARGE
    assert lib.lshrs_scan_workspace_bytes(1, 8, 16385, 8) == _native.E_TOOLARGE
    # bad arguments are refused before anything touches a device
    assert lib.lshrs_scan_topk_f32(None, 8, 8, 8, None, None, 1, 8, None, None, None, None, None, None) == _native.E_BADARG
    assert lib.lshrs_scan_topk_bf16(None, 8, 8, 8, None, None, 0, 8, None, None, None, None, None, None) == 0      # q == 0


def test_argument_validation_without_a_device():
    from lshrs_amd import DeviceVectors, exact_top_k

    q, x = np.zeros((2, 8), np.float32), np.zeros((4, 8), np.float32)
    with pytest.raises(ValueError, match="k must be > 0"):
        exact_top_k(q, x, 0)
    with pytest.raises(ValueError, match="method must be"):
        exact_top_k(q, x, 3, method="brute")
    store = DeviceVectors(8)
    with pytest.raises(ValueError, match=r"shape \(n, 8\)"):
        store.search(np.zeros((2, 9), np.float32))
    with pytest.raises(ValueError, match=r"shape \(n, 8\)"):
        store.search(np.zeros(8, np.float32))
    assert store.last_search_stats == {}
