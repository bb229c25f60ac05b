"""tests/_replay_reference.py on the CPU: its reference against NumPy on a host whose BLAS is a recognised order, its parameter
lists against what `_hostblas.named_model` claims, its case builder's promises - and the argument refusals of
lshrs_sig_replay_values_f32, which return before anything touches a device (the pointers handed over are small integers that
are nobody's memory and are never dereferenced)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import _replay_reference as R

P = 0x1000                 # a non-NULL, 16-byte aligned "pointer" no path below reads through
E_BADARG, E_TOOLARGE = -10001, -10002
STAGE2, TIES, SMALL = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from lshrs_amd import _native

    _native.build()
    assert (_native.E_BADARG, _native.E_TOOLARGE) == (E_BADARG, E_TOOLARGE)
    assert (_native.REPLAY_ROUTE_STAGE2, _native.REPLAY_ROUTE_TIES, _native.REPLAY_ROUTE_SMALL) == (STAGE2, TIES, SMALL)
    return _native.load()


def _all_shapes():
    """(nb, r, dim) of every GPU case, once"""
    shapes = [(R.stage2_bands(r), r, d) for r, d in R.STAGE2_SHAPES + R.TIES_TAIL_SHAPES + R.SMALL_SHAPES + R.SMALL_SHAPES_MORE]
    shapes += R.BUCKET_SHAPES + [(4, r, d) for r, d in R.TIES_BLOCK_SHAPES]
    shapes += [(3, r, d) for r in R.TIES_MODEL3_ROWS + R.TIES_MODEL2_ROWS for d in R.SMALL_DIMS]
    return sorted(set(shapes))


def test_every_gpu_parameter_is_a_shape_the_named_builds_claim():
    from lshrs_amd import _hostblas

    for nb, r, dim in _all_shapes():
        ms = R.models_of(r, dim)
        assert ms and all(m in (1, 2, 3) for _b, m in ms), (r, dim)
        for build, m in ms:
            assert _hostblas.named_model(build, r, dim) == m and R.build_of(m, r, dim) in R.BUILDS
    for r in R.TIES_MODEL3_ROWS:
        for dim in R.SMALL_DIMS:
            assert _hostblas.named_model("openblas-skylakex", r, dim) == 3
    for r in R.TIES_MODEL2_ROWS:
        for dim in R.SMALL_DIMS:
            assert _hostblas.named_model("openblas-haswell", r, dim) == (1 if dim % 4 == 0 else 2)
    for r, dim in R.SMALL_SHAPES + R.SMALL_SHAPES_MORE:
        assert R.models_of(r, dim) == [("openblas-skylakex", 1)]              # the small kernel replays model 1 only
    for r, dim in R.STAGE2_SHAPES:
        if r == 1 or dim % 4:
            assert [m for _b, m in R.models_of(r, dim)] == [1, 2]             # sdot and the scalar tail: both builds, two orders


def test_dispatch_rules_as_restated():
    assert R.stage2_kernel(16, 128) == ("fix8", 4, False) and R.stage2_kernel(16, 160) == ("fix8", 6, False)
    assert R.stage2_kernel(4, 200) == ("fix8", 6, True) and R.stage2_kernel(5, 100) == ("fix8", 4, True)
    assert R.stage2_kernel(4, 8192) == ("fix8", 6, True) and R.stage2_kernel(16, 4096) == ("fix8", 6, False)
    assert R.stage2_kernel(1, 768) == ("fixany", 0, False) and R.stage2_kernel(16, 768, buckets=True) == ("fix8-samep", 6, False)
    assert [R.row_kind(j, 7) for j in range(8)] == [0, 0, 0, 0, 1, 1, 2, 0]
    assert [R.row_kind(j, 13) for j in range(12, 16)] == [2, 0, 0, 0] and [R.row_kind(j, 10) for j in (8, 9)] == [1, 1]
    from lshrs_amd import _hostblas

    for r in (1, 3, 5, 6, 7, 10, 13, 16):
        assert [R.row_kind(j, r) for j in range(r)] == _hostblas.blas_row_kinds(r).tolist()
    assert R.small_kernel(16, 768) == (24, False) and R.small_kernel(16, 1536) == (48, False) and R.small_kernel(8, 3072) == (128, False)
    assert R.small_kernel(10, 300) == (24, True) and R.small_kernel(10, 1504) == (48, True) and R.small_kernel(6, 4088) == (128, True)
    assert R.ties_plan(7, 102, 2, True) == (0, True) and R.ties_plan(4, 4100, 1, True) == (0, True)
    assert R.ties_plan(10, 300, 1, True) == (0, False) and R.ties_plan(10, 300, 1, False) == (0, True)
    assert R.ties_plan(5, 7, 1, False) == (E_TOOLARGE, None) and R.ties_plan(4, 768, 2, True) == (E_TOOLARGE, None)
    assert R.ties_plan(1, 7, 3, False) == (E_BADARG, None)
    assert R.stage2_refusal(32, 5, 4108, 1) == E_BADARG and R.stage2_refusal(64, 4, 8192, 1) == 0
    assert R.stage2_refusal(2, 8, 768, 1) == E_TOOLARGE and R.stage2_refusal(32, 7, 102, 3) == E_BADARG


def test_case_builder_keeps_its_promises():
    for nb, r, dim in [(16, 16, 768), (32, 7, 102), (32, 1, 33), (3, 5, 1), (3, 33, 8), (4, 3, 8196)]:
        c = R.case(nb, r, dim)
        assert c is R.case(nb, r, dim)                                        # computed once, shared
        assert c.x.shape == (R.N_ROWS, dim) and c.x.dtype == np.float32
        assert np.isnan(c.x[R.ROW_NAN]).sum() == 1 and np.isposinf(c.x[R.ROW_INF]).sum() == 1
        finite = np.isfinite(c.x).all(axis=1)
        assert sorted(np.flatnonzero(~finite).tolist()) == sorted(R.NONFINITE_ROWS)
        assert not c.x[R.ROW_ZERO].any()
        grid = c.planes[c.grid_band] * 64
        assert np.array_equal(grid, np.round(grid)) and np.abs(grid).max() <= 127
        if dim >= 64:
            for row, (b, j) in zip(R.ROWS_CANCELLED, c.cancelled):             # cancelled: ~1e-7 of what a Gaussian row leaves
                p = c.planes[b][j].astype(np.float64)
                y = abs(float(p @ c.x[row].astype(np.float64)))
                assert y < 1e-5 * np.linalg.norm(p) * np.linalg.norm(c.x[row].astype(np.float64))
        entries = R.plain_list(c)
        rows, cols = R.entry_rows_cols(entries)
        pairs = set(zip(rows.tolist(), cols.tolist()))
        assert len(pairs) >= entries.size - 3 and (cols >= c.padcols).sum() == 3
        assert {(i, int(k)) for i in range(R.N_ROWS) for k in R.key_columns(c)} <= pairs
        assert entries.size % 8 != 0                                          # the list ends inside a group of eight
        assert {(i, int(k)) for i in range(R.N_ROWS) for k in R.padding_columns(c, nb - 1)[:-1]} <= pairs


def test_reference_flags_the_non_finite_rows_and_nothing_else():
    for nb, r, dim in [(16, 16, 160), (32, 7, 102), (32, 1, 100), (3, 5, 1), (3, 9, 6), (3, 17, 8)]:
        c = R.case(nb, r, dim)
        entries = R.plain_list(c)
        for _build, model in R.models_of(r, dim):
            want = R.expected_values(c.planes, c.x, entries, model, r)
            live = R.check_reference(c, entries, want, model)
            assert int(live.sum()) == entries.size - 3
            # the judge: takes the reference itself, refuses one last-place error, one value written where none may be
            got = np.where(live, want, R.SENTINEL).astype(np.float32)
            compared, nan = R.judge(c, entries, want, got, model, "self")
            assert compared + nan == int(live.sum()) and nan >= int((live & np.isin(R.entry_rows_cols(entries)[0], [R.ROW_NAN])).sum())
            off = got.copy()
            k = int(np.flatnonzero(live & np.isfinite(want) & (want != 0))[3])
            off[k] = np.nextafter(off[k], np.float32(np.inf))
            with pytest.raises(AssertionError):
                R.judge(c, entries, want, off, model, "one ulp off")
            dead = got.copy()
            dead[int(np.flatnonzero(~live)[0])] = 0.0
            with pytest.raises(AssertionError):
                R.judge(c, entries, want, dead, model, "a dead entry written")
            neg = got.copy()
            z = np.flatnonzero(live & (R.bits(want) == 0))
            neg[z] = -0.0                                                     # the sign of a zero carries no key bit
            R.judge(c, entries, want, neg, model, "-0.0")


def test_reference_is_numpy_on_a_host_with_a_recognised_blas():
    """Where this host's own BLAS is one of the named builds, expected_values IS `planes[b] @ x` of this process, bit for bit, on
    the case builder's rows (the non-finite rows: NaN where NumPy has NaN, the same bits elsewhere; the sign of a zero is not
    compared - sgemv adds its result to a y of +0.0, the model returns the sum itself - and carries no key bit)."""
    from lshrs_amd import _hostblas

    _hostblas.build()
    host = _hostblas.host_build_name()
    if host is None:
        pytest.skip("this host's BLAS is not one of the named builds: nothing to compare the reference with here")
    checked = 0
    for nb, r, dim in _all_shapes():
        model = _hostblas.named_model(host, r, dim)
        assert model
        c = R.case(nb, r, dim)
        if _hostblas.blas_order_model(np.stack(c.planes)) != model:           # (this host's licence for this very shape)
            continue
        cols = R.key_columns(c)
        entries = R.flag_entries(np.repeat(np.arange(R.N_ROWS), cols.size), np.tile(cols, R.N_ROWS))
        want = R.expected_values(c.planes, c.x, entries, model, r).reshape(R.N_ROWS, nb * r)
        with np.errstate(all="ignore"):
            host_y = np.stack([np.concatenate([p @ v for p in c.planes]) for v in c.x]).astype(np.float32)
        assert np.array_equal(np.isnan(want), np.isnan(host_y)), (nb, r, dim)
        ok = np.isnan(want) | (R.bits(want) == R.bits(host_y))                # (-0.0 as +0.0: a zero row's sign is the only place they part)
        assert ok.all(), (nb, r, dim, np.argwhere(~ok)[:8])
        checked += 1
    assert checked >= len(_all_shapes()) // 2


# ------------------------------------------------------------------------------------------------------------------
# lshrs_sig_replay_values_f32: what it refuses, without a GPU
# ------------------------------------------------------------------------------------------------------------------

def _call(lib, route, *, X=P, n=19, ldx=None, ws=P, nb=16, r=16, dim=768, model=1, keys=P, values=P, lst=P, cap=100, sort=None,
          counters=P):
    ldx = dim if ldx is None else ldx
    return lib.lshrs_sig_replay_values_f32(X, n, ldx, ws, nb, r, dim, model, route, keys, values, lst, cap,
                                           ctypes.addressof(sort) if sort is not None else None, counters, None)


def test_values_entry_refuses_what_every_route_refuses(lib):
    for route in (STAGE2, TIES, SMALL):
        lst = None if route == SMALL else P
        assert _call(lib, route, n=0, X=None, ws=None, keys=None, values=None, lst=None, counters=None) == 0      # nothing to do
        assert _call(lib, route, lst=lst, values=None) == E_BADARG
        assert _call(lib, route, lst=lst, counters=None) == E_BADARG
        assert _call(lib, route, lst=lst, X=None) == E_BADARG
        assert _call(lib, route, lst=lst, ws=None) == E_BADARG
        assert _call(lib, route, lst=lst, keys=None) == E_BADARG
        assert _call(lib, route, lst=lst, n=-1) == E_BADARG
        assert _call(lib, route, lst=lst, ldx=767) == E_BADARG                                                    # ldx < dim
        assert _call(lib, route, lst=lst, nb=0) == E_BADARG
        assert _call(lib, route, lst=lst, model=0) == E_BADARG and _call(lib, route, lst=lst, model=4) == E_BADARG
    assert _call(lib, 3) == E_BADARG and _call(lib, -1) == E_BADARG                                               # no such route


def test_values_entry_small_route_refusals(lib):
    s = lambda **kw: _call(lib, SMALL, **{"lst": None, **kw})
    assert s(lst=P) == E_BADARG                                               # the small route takes no list
    assert s(model=2) == E_BADARG and s(model=3, dim=8) == E_BADARG           # model 1 only
    assert s(dim=10, ldx=32) == E_TOOLARGE and s(dim=4, ldx=32) == E_TOOLARGE
    assert s(dim=4100, ldx=4128) == E_TOOLARGE                                # more than 128 k-tiles
    assert s(dim=300, ldx=300) == E_TOOLARGE                                  # rows not padded to whole k-tiles
    assert s(dim=300, ldx=322) == E_TOOLARGE                                  # ldx % 4
    assert s(X=P + 4) == E_TOOLARGE                                           # rows not 16-byte aligned
    assert s(n=257) == E_TOOLARGE


def test_values_entry_ties_route_refusals(lib):
    t = lambda **kw: _call(lib, TIES, **kw)
    assert t(lst=None) == E_BADARG and t(cap=0) == E_BADARG
    from lshrs_amd import _native

    sort = _native.SigSort(P, P, P, 1 << 20, thr_ptr=P)
    assert t(sort=sort) == E_BADARG                                           # segments: stage-2 route only
    assert t(model=3, dim=9, r=4) == E_BADARG and t(model=3, dim=8, r=1) == E_BADARG
    for dim in (1, 2, 3, 5, 6, 7):
        assert t(model=1, dim=dim, r=4) == E_TOOLARGE                         # a scalar tail below 9 elements: model 2 / 3 only
        assert R.ties_plan(4, dim, 1, True) == (E_TOOLARGE, None)
    assert t(model=2, dim=768) == E_TOOLARGE and t(model=2, dim=8, r=2) == E_TOOLARGE     # whole groups of four: model 1
    assert t(n=1 << 42) == E_TOOLARGE


def test_values_entry_stage2_route_refusals(lib):
    from lshrs_amd import _native

    s2 = lambda **kw: _call(lib, STAGE2, **kw)
    assert s2(lst=None) == E_BADARG and s2(cap=0) == E_BADARG
    assert s2(nb=32, r=5, dim=4108) == E_BADARG == R.stage2_refusal(32, 5, 4108, 1)      # 8 m + 4 beyond one block
    assert s2(nb=32, r=7, dim=102, model=3) == E_BADARG
    assert s2(dim=770, model=3) == E_BADARG
    assert s2(nb=32, r=4, dim=8, model=3) == E_BADARG                         # model 3 is the tie route's alone
    assert s2(model=2) == E_BADARG                                            # whole groups of four: model 1
    assert s2(nb=32, r=16, dim=16) == E_BADARG                                # below 32 elements: resident shapes only
    assert s2(nb=2, r=8, dim=768) == E_TOOLARGE == R.stage2_refusal(2, 8, 768, 1)        # fewer than 128 key columns
    assert s2(ldx=1 << 20) == E_BADARG
    assert s2(n=1 << 42) == E_TOOLARGE
    # the column segments: only a scratch the split pass itself would fill
    good = lambda **kw: _native.SigSort(P, P, P, kw.pop("cap", 256 * 83), thr_ptr=kw.pop("thr", P), mode=kw.pop("mode", 1))
    assert s2(sort=good()) == E_BADARG                                        # a list beside the segments
    b = lambda sort, **kw: s2(lst=None, cap=0, sort=sort, **kw)
    bad = good()
    bad.struct_bytes = 8
    assert b(bad) == E_BADARG
    assert b(_native.SigSort(None, P, P, 256 * 83, thr_ptr=P)) == E_BADARG
    assert b(_native.SigSort(P, None, P, 256 * 83, thr_ptr=P)) == E_BADARG
    assert b(_native.SigSort(P, P, None, 256 * 83, thr_ptr=P)) == E_BADARG
    assert b(good(thr=None)) == E_BADARG and b(good(mode=0)) == E_BADARG
    assert b(good(cap=0)) == E_BADARG and b(good(cap=256 * 63)) == E_BADARG   # segments shorter than 64 entries
    assert b(good(), dim=128) == E_BADARG                                     # four k-tiles: the short-row kernel's
    assert b(good(cap=256 * 64), nb=32, r=1, dim=768) == E_BADARG             # one-row bands: the plain-load form's
    assert b(good(cap=2048 * 64), nb=128, r=16) == E_BADARG                   # more than 1024 padded key columns
