"""The selection of the exhaustive scan (csrc/scan.hip: the per-query buffers, the overflow / prune / retry loop, the slices'
winners, scan_merge_kernel), exact, on the GPU.

Every case: `A` = the approximate score of every (query, live row), from lshrs_scan_above_* with a bar of -inf
(tests/_scan_reference.all_pairs_approx: a kernel without selection, slices' winners or merge, on the same arithmetic); then the
rows, the score BITS and the count lshrs_scan_topk_* returns must EQUAL the windows those scores determine
(`expected_windows`: descending score, equal scores by ascending row, +0.0 ahead of -0.0).  No tolerance anywhere.  A failure
first says whether the returned scores are A's at the returned rows: if not, the two kernels' arithmetic diverged (the header's
"same arithmetic" is false); if so, the selection or the merge is wrong.

The shapes are the smallest that reach what they are for; tests/test_scan_reference_host.py holds their geometry (slices,
merge items, the prune form) against the built library."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import _scan_reference as R

pytestmark = pytest.mark.gpu

# cap 64 (1 .. 32), 128 (33 .. 64) and 256 (65 .. 128): both sides of each threshold, and windows that are no power of two
WINDOWS = (1, 2, 3, 4, 8, 16, 31, 32, 33, 63, 64, 65, 100, 127, 128)
SMALL_M = (1, 31, 32, 33, 255, 256, 257, 1_023, 1_024, 1_025)
# (q, m, dim, window): what each reaches is asserted in tests/test_scan_reference_host.py::test_the_geometry_the_gpu_cases_rely_on
GEOMETRY = ((5, 81_919, 16, 128),          # the `limit` clamp binds; the merge at 8 192 items / 64 KiB; a last slice of 1 279 rows
            (70, 81_920, 16, 127),         # the same with two query tiles; zero padding inside the 64 KiB network
            (5, 131_071, 16, 64),          # cap = 128 (scan_prune_n<2>) at the merge's full size
            (5, 131_071, 16, 33),          # cap = 128, a window that is no power of two
            (16_449, 300, 16, 128),        # 258 query tiles, more than the resident workgroups: one slice
            (6_400, 3_000, 16, 128),       # 100 query tiles: resident / qtiles decides
            (7, 1_025, 16, 3))             # the smallest merge; the second slice is one row past a pass
ASCENDING_TOO = (0, 2, 3)
M, DIM, Q = 5_000, 33, 70                  # S1 - S5: two query tiles, the second of 6 queries; five slices of 1 024 rows


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _gaussian(seed, m, dim, q):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((m, dim)).astype(np.float32), rng.standard_normal((q, dim)).astype(np.float32)


def _ascending(seed, m, dim, q):
    """Rows in ascending float64 cosine to one direction v, queries v + 0.05 noise: every pass brings every query rows that
    beat all it has seen, so every pass of every slice overflows the buffers and the prune / retry loop runs throughout."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(dim)
    X = rng.standard_normal((m, dim)).astype(np.float32)
    cos = (X.astype(np.float64) @ v) / (np.linalg.norm(X.astype(np.float64), axis=1) * np.linalg.norm(v))
    X = np.ascontiguousarray(X[np.argsort(cos, kind="stable")])
    Qs = (v[None, :] + 0.05 * rng.standard_normal((q, dim))).astype(np.float32)
    return X, Qs


def _make(torch, X, Qs, name, row_ids=None):
    stored = R._stored_form(torch, name, X)
    Qd = torch.from_numpy(Qs).cuda()
    rid = None if row_ids is None else torch.from_numpy(row_ids).cuda()
    live = np.ones(X.shape[0], dtype=bool) if row_ids is None else row_ids >= 0
    A, emitted = R.all_pairs_approx(stored, Qd, rid)
    assert emitted == Qs.shape[0] * int(live.sum())
    A.setflags(write=False)
    return {"stored": stored, "Q": Qd, "rid": rid, "live": live, "A": A}


@functools.lru_cache(maxsize=None)
def _data(kind, name="bfloat16"):
    """One data set in one stored form with its all-pairs scores and its windows of 128 (made once, never modified)."""
    torch = _torch()
    rng = np.random.default_rng(99)
    row_ids = None
    if kind == "gaussian":
        X, Qs = _gaussian(7, M, DIM, Q)
    elif kind == "ascending":
        X, Qs = _ascending(8, M, DIM, Q)
    elif kind == "descending":                              # after a slice's first pass nothing may enter
        X, Qs = _ascending(8, M, DIM, Q)
        X = np.ascontiguousarray(X[::-1])
    elif kind == "ties":                                    # 40 distinct rows, each stored 150 times as identical bits
        base, Qs = _gaussian(9, 40, DIM, Q)
        X = np.ascontiguousarray(np.repeat(base, 150, axis=0)[rng.permutation(6_000)])
    else:
        X, Qs = _gaussian(7, M, DIM, Q)
        ids = rng.permutation(1 << 20)[:M].astype(np.int64)     # (what a live row is called is not the scan's business)
        dead = np.zeros(M, dtype=bool)
        if kind == "dead-90%":
            dead[rng.permutation(M)[:M * 9 // 10]] = True
        elif kind == "dead-slice":                          # all of one slice: it hands zero items to the merge
            dead[1024:2048] = True
        elif kind == "dead-but-100":                        # count = 100 < 128: the padding
            dead[:] = True
            dead[rng.permutation(M)[:100]] = False
        else:
            raise KeyError(kind)
        row_ids = np.where(dead, -1 - ids, ids)
    case = _make(torch, X, Qs, name, row_ids)
    case["expected"] = R.expected_windows(case["A"], case["live"], max(WINDOWS))
    return case


def _windows(torch, case, window):
    from lshrs_amd._exact import scan_windows

    rows, approx, count, err = scan_windows(case["stored"], case["Q"], window, case["rid"])
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    return rows.cpu().numpy(), approx.cpu().numpy(), count.cpu().numpy()


def _assert_equal(got, want, A, what):
    rows, approx, count = got
    erows, ebits, ecount = want
    bits = approx.view(np.uint32)
    if np.array_equal(rows, erows) and np.array_equal(bits, ebits) and np.array_equal(count, ecount):
        return
    inside = (rows >= 0) & (rows < A.shape[1])
    qi = np.nonzero(inside)[0]
    same_arithmetic = np.array_equal(bits[inside], A.view(np.uint32)[qi, rows[inside]])
    bad = np.nonzero((rows != erows).any(axis=1) | (bits != ebits).any(axis=1) | (count != ecount))[0]
    i = int(bad[0])
    j = np.nonzero((rows[i] != erows[i]) | (bits[i] != ebits[i]))[0]
    at = int(j[0]) if j.shape[0] else -1
    verdict = ("the returned scores are the all-pairs scores of the returned rows: the SELECTION or the MERGE is wrong"
               if same_arithmetic else
               "the returned scores are NOT the all-pairs scores of the returned rows: the two kernels' ARITHMETIC diverged")
    raise AssertionError(f"{what}: {bad.shape[0]} of {rows.shape[0]} queries differ; {verdict}.  Query {i}: count {count[i]} "
                         f"(expected {ecount[i]}), first difference at position {at}: row {rows[i, at]} bits "
                         f"{bits[i, at]:#010x}, expected row {erows[i, at]} bits {ebits[i, at]:#010x}")


DATA_SETS = (("gaussian", "bfloat16"), ("gaussian", "float32"), ("gaussian", "int8"),
             ("ascending", "bfloat16"), ("ascending", "float32"), ("ascending", "int8"),
             ("descending", "bfloat16"), ("ties", "bfloat16"),
             ("dead-90%", "bfloat16"), ("dead-slice", "bfloat16"), ("dead-but-100", "bfloat16"))


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("kind,name", DATA_SETS, ids=[f"{k}-{n}" for k, n in DATA_SETS])
def test_every_window_is_the_all_pairs_window(kind, name, window):
    torch = _torch()
    case = _data(kind, name)
    want = R.narrower(case["expected"], window)
    _assert_equal(_windows(torch, case, window), want, case["A"], f"{kind} {name} window {window}")
    erows, ebits, ecount = want
    live = int(case["live"].sum())
    assert np.all(ecount == min(window, live))
    if kind == "ties" and window == 128:
        # one score alone fills the window, which must hold the 128 lowest of its 150 rows
        assert np.all(ebits == ebits[:, :1]) and np.all(np.diff(erows, axis=1) > 0)
    if kind == "dead-but-100" and window > 100:
        assert np.all(erows[:, 100:] == -1) and np.all(ebits[:, 100:] == R.NEG_INF_BITS)


@pytest.mark.parametrize("m", SMALL_M)
def test_small_blocks(m):
    """Fewer rows than a tile, a pass, a slice - and one more: windows wider than the block are padded."""
    torch = _torch()
    X, Qs = _gaussian(100 + m, m, 16, 7)
    case = _make(torch, X, Qs, "bfloat16")
    for window in (1, 33, 128):
        want = R.expected_windows(case["A"], None, window)
        assert np.all(want[2] == min(window, m))
        _assert_equal(_windows(torch, case, window), want, case["A"], f"m = {m}, window {window}")


@pytest.mark.parametrize("index,order", [(i, "gaussian") for i in range(len(GEOMETRY))] + [(i, "ascending") for i in ASCENDING_TOO])
def test_slice_plans_and_merge_sizes(index, order):
    torch = _torch()
    q, m, dim, window = GEOMETRY[index]
    X, Qs = (_gaussian if order == "gaussian" else _ascending)(500 + index, m, dim, q)
    case = _make(torch, X, Qs, "bfloat16")
    want = R.expected_windows(case["A"], None, window)
    assert np.all(want[2] == min(window, m))
    _assert_equal(_windows(torch, case, window), want, case["A"], f"{GEOMETRY[index]} {order}")
