"""The k-NN self-join over device-resident rows (lshrs_amd.exact_knn, DeviceVectors.neighbors, LSHRS.neighbors_exact) and the
kernel behind it (csrc/scan.hip, lshrs_scan_knn_*), on the GPU.  Both halves are asked for exactly:

the first pass   the range scan with a bar of -inf gives the approximate score of EVERY (row as f32 query, row)
                 (tests/_scan_reference.all_pairs_approx); with the diagonal struck out, those scores and the item order
                 determine the window of every live query row (expected_windows): rows, score bits, counts.  For the one-term
                 types that is the check that dropping the zero `mid` term's MFMA changed nothing;
the answer       exact_knn equals the oracle that predates it: exact_top_k(stored.float(), stored, k + 1) per row with the row
                 itself removed, or else the last entry dropped - the same ids, the same score bits, the documented order.

Shapes: the smallest at which the kernel can go wrong - fewer rows than a tile (1, 2, 33), more than one pass of 256 (257,
700), dims below / at / across a chunk of 64 (1, 17, 64, 100) and many chunks (768), blocks of 64 and 128 query rows so that
700 rows span many blocks.  dim = 1 makes every cosine +-1: the tie order, and the overflow / prune / retry loop under load."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import _scan_reference as R

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "bfloat16", "float16", "int8", "float8_e4m3fn")
MS = (1, 2, 33, 257, 700)
DIMS = (1, 17, 64, 100, 768)
WINDOWS = (1, 16, 128)
QBLOCKS = (0, 64, 128)
IDS = ("none", "dead", "descending")
KS = (1, 5, 70)                     # (2 x 70 is beyond the widest window: "auto" takes "gather")
METHODS = ("scan", "gather", "auto")
# the shapes of the self-join's answer test (tests/test_gpu_exact_pairs.py)
ANSWER_SHAPES = ((1, 17), (2, 1), (2, 64), (33, 1), (33, 100), (257, 64), (257, 768), (700, 17), (700, 100), (700, 768))
T = 0.75


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _rows(m, dim):
    """Seeded random rows with planted partners: exact copies, and rows at a cosine of T give or take a few float32 ulps."""
    rng = np.random.default_rng(1000 * m + dim)
    X = rng.standard_normal((m, dim)).astype(np.float32)
    if m >= 33:
        pick = rng.choice(m, 24, replace=False)
        X[pick[:6]] = X[pick[6:12]]                                     # exact copies
        for j, (src, dst) in enumerate(zip(pick[12:18], pick[18:24])):  # cosine ~ T -2 .. +3 ulps (in exact arithmetic)
            u = X[src].astype(np.float64)
            u /= np.linalg.norm(u)
            v = rng.standard_normal(dim)
            v -= (v @ u) * u
            nv = np.linalg.norm(v)
            c = T + (j - 2) * 2.0 ** -24
            X[dst] = ((c * u + np.sqrt(1.0 - c * c) * v / nv) * 3.0).astype(np.float32) if nv > 0 else X[src]
    return X


def _row_ids(mode, m):
    """None; or ids with some dead rows (row 1 and every seventh; `_case` makes the dead row 1 all zeros); or ids that descend
    while the rows ascend, with gaps."""
    if mode == "none":
        return None
    if mode == "dead":
        ids = np.arange(m, dtype=np.int64) * 3 + 5
        ids[1::7] = -1
        return ids
    return (np.arange(m, dtype=np.int64)[::-1] * 5 + 2).copy()


@functools.lru_cache(maxsize=None)
def _case(m, dim, name, mode):
    """Rows in one stored form with one kind of row_ids (made once, never modified): `stored`, `ids` (device) / `ids_h`, `live`
    and `Q`, the rows as float32 queries for the oracles - with ones in place of a dead zero row, which is nobody's query."""
    torch = _torch()
    stored = R._stored_form(torch, name, _rows(m, dim))
    ids_h = _row_ids(mode, m)
    Q = stored.float().contiguous()
    if mode == "dead" and m > 1:
        stored[1] = 0                                                   # a dead row of zero norm: it must raise nothing
        Q[1] = 1.0
    ids = None if ids_h is None else torch.from_numpy(ids_h).cuda()
    live = np.ones(m, dtype=bool) if ids_h is None else ids_h >= 0
    return {"stored": stored, "ids": ids, "ids_h": ids_h, "Q": Q, "live": live}


@functools.lru_cache(maxsize=None)
def _expected(m, dim, name, mode):
    """What lshrs_scan_knn_* must leave for every row of a case at the widest window: all_pairs_approx of the rows as f32
    queries, the diagonal struck out, cut into windows; a dead query row gets nothing.  (rows, score bits, counts), read-only."""
    c = _case(m, dim, name, mode)
    A, _ = R.all_pairs_approx(c["stored"], c["Q"], c["ids"])
    A = A.copy()
    A[np.arange(m), np.arange(m)] = np.nan
    rows, bits, count = R.expected_windows(A, c["live"], max(WINDOWS))
    dead = ~c["live"]
    rows[dead], bits[dead], count[dead] = -1, R.NEG_INF_BITS, 0
    for a in (rows, bits, count):
        a.setflags(write=False)
    return rows, bits, count


def _check_windows(got, want, what):
    rows, approx, count, err = got
    want_rows, want_bits, want_count = want
    assert int(err.item()) == 0, f"{what}: error word {int(err.item())}"
    rows, bits, count = rows.cpu().numpy(), approx.cpu().numpy().view(np.uint32), count.cpu().numpy()
    assert np.array_equal(count, want_count), f"{what}: counts differ at query rows {np.flatnonzero(count != want_count)[:5]}"
    bad = np.flatnonzero((rows != want_rows).any(axis=1))
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} windows hold other rows, first query row {bad[0]}: {rows[bad[0]]} != {want_rows[bad[0]]}"
    bad = np.flatnonzero((bits != want_bits).any(axis=1))
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} windows hold other score bits, first query row {bad[0]}"


# ------------------------------------------------------------------------------------------
# 1. the first pass, exactly
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("m", MS)
def test_first_pass_is_the_window_the_range_scans_scores_determine(m, dim, name):
    from lshrs_amd._exact import scan_knn

    for mode in IDS:
        c = _case(m, dim, name, mode)
        widest = _expected(m, dim, name, mode)
        for window in WINDOWS:
            want = R.narrower(widest, window)
            for qblock in QBLOCKS:
                _check_windows(scan_knn(c["stored"], 0, m, window, c["ids"], qblock), want,
                               f"{m} x {dim} {name}, ids {mode}, window {window}, qblock {qblock}")


@pytest.mark.parametrize("name", DTYPES)
def test_first_pass_of_a_range_of_the_rows(name):
    """Rows [37, 137) of 257 as the queries: the windows of exactly those rows, over all 257."""
    from lshrs_amd._exact import scan_knn

    m, dim, lo, n = 257, 100, 37, 100
    for mode in ("none", "dead"):
        c = _case(m, dim, name, mode)
        widest = _expected(m, dim, name, mode)
        for window in (16, 128):
            want = tuple(a[lo:lo + n] for a in R.narrower(widest, window))
            for qblock in (0, 64):
                got = scan_knn(c["stored"], lo, n, window, c["ids"], qblock)
                _check_windows(got, want, f"range {name}, ids {mode}, window {window}, qblock {qblock}")
                assert not (got[0].cpu().numpy() == (lo + np.arange(n))[:, None]).any(), "a row in its own window"
    empty = scan_knn(_case(m, dim, name, "none")["stored"], m, 0, 16)
    assert empty[0].shape == (0, 16) and empty[2].shape == (0,) and int(empty[3].item()) == 0


@pytest.mark.parametrize("name", DTYPES)
def test_first_pass_on_rows_at_any_address_and_stride(name):
    """A base one element into the allocation and an odd row stride: the element-wise loads (ALIGNED = false) of the pass and
    the prep kernels' reads; then an aligned base with a row stride larger than dim.  The windows are those of the same rows in
    a fresh allocation."""
    torch = _torch()
    from lshrs_amd._exact import scan_knn

    m, dim = 257, 100
    c = _case(m, dim, name, "dead")
    widest = _expected(m, dim, name, "dead")
    ld = dim + 3
    flat = torch.zeros(m * ld + 1, dtype=c["stored"].dtype, device="cuda")
    view = torch.as_strided(flat, (m, dim), (ld, 1), 1)
    view.copy_(c["stored"])
    assert view.stride(0) % 2 == 1 and view.data_ptr() % 16 != 0
    wide = torch.zeros((m, 128), dtype=c["stored"].dtype, device="cuda")
    if name in ("float32", "bfloat16", "float16"):
        wide[:, dim:] = float("nan")                        # (nothing is taken from behind a row's last element)
    strided = wide[:, :dim]
    strided.copy_(c["stored"])
    assert strided.stride(0) == 128 and strided.data_ptr() % 16 == 0
    for rows, what in ((view, "unaligned"), (strided, "strided")):
        for window, qblock in ((16, 0), (128, 64)):
            _check_windows(scan_knn(rows, 0, m, window, c["ids"], qblock), R.narrower(widest, window),
                           f"{what} {name}, window {window}, qblock {qblock}")


@pytest.mark.parametrize("name", ("float32", "bfloat16"))
def test_first_pass_writes_nothing_outside_its_arrays(name):
    """lshrs_scan_knn_* itself with arrays longer than (q_count, window): the guard slots behind them stay as they were."""
    torch = _torch()
    from lshrs_amd import _native
    from lshrs_amd.similarity import corpus_suffix

    lib = _native.load()
    m, dim, lo, n, window, guard = 700, 17, 64, 300, 16, 64
    c = _case(m, dim, name, "dead")
    want = tuple(a[lo:lo + n] for a in R.narrower(_expected(m, dim, name, "dead"), window))
    stored = c["stored"]
    for qblock in (0, 128):
        o_r = torch.full((n * window + guard,), -7, dtype=torch.int64, device="cuda")
        o_s = torch.full((n * window + guard,), -7.0, dtype=torch.float32, device="cuda")
        o_c = torch.full((n + guard,), -7, dtype=torch.int32, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(lib.lshrs_scan_knn_workspace_bytes(n, m, dim, window, qblock)), dtype=torch.uint8, device="cuda")
        fn = getattr(lib, "lshrs_scan_knn_" + corpus_suffix(stored))
        _native.check(fn(stored.data_ptr(), m, int(stored.stride(0)), dim, c["ids"].data_ptr(), lo, n, window, qblock,
                         o_r.data_ptr(), o_s.data_ptr(), o_c.data_ptr(), ws.data_ptr(), err.data_ptr(),
                         torch.cuda.current_stream().cuda_stream), "knn")
        torch.cuda.synchronize()
        assert bool((o_r[n * window:] == -7).all()) and bool((o_s[n * window:] == -7.0).all()) and bool((o_c[n:] == -7).all())
        _check_windows((o_r[:n * window].view(n, window), o_s[:n * window].view(n, window), o_c[:n], err), want,
                       f"range guard {name}, qblock {qblock}")


# ------------------------------------------------------------------------------------------
# 2. the public answer, exactly
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(m, dim, name, mode, k):
    """exact_top_k(rows as float32 queries, rows, k + 1) per live row, the row itself removed or else the last entry dropped;
    the rows in ascending order of id: (ids (n,), neighbors (n, kk), scores (n, kk))."""
    from lshrs_amd import exact_top_k

    c = _case(m, dim, name, mode)
    ids, scores = exact_top_k(c["Q"], c["stored"], k + 1, row_ids=c["ids"])
    own = np.arange(m, dtype=np.int64) if c["ids_h"] is None else c["ids_h"]
    n = int(c["live"].sum())
    kk = max(0, min(k, n - 1))
    assert ids.shape[1] == min(k + 1, n)
    out_n = np.empty((n, kk), dtype=np.int64)
    out_s = np.empty((n, kk), dtype=np.float32)
    order = [r for r in np.argsort(own, kind="stable") if own[r] >= 0]
    for i, r in enumerate(order):
        at = np.flatnonzero(ids[r] == own[r])
        drop = int(at[0]) if at.shape[0] else ids.shape[1] - 1
        keep = np.arange(ids.shape[1]) != drop
        out_n[i], out_s[i] = ids[r][keep][:kk], scores[r][keep][:kk]
    return own[order], out_n, out_s


@pytest.mark.parametrize("mode", IDS)
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("shape", ANSWER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_answer_is_exact_top_ks_without_the_row_itself(shape, name, mode):
    from lshrs_amd import exact_knn, scan_max_window

    m, dim = shape
    c = _case(m, dim, name, mode)
    live = int(c["live"].sum())
    for k in KS:
        want_ids, want_n, want_s = _oracle(m, dim, name, mode, k)
        for method in METHODS:
            stats = {}
            ids, nbrs, scores = exact_knn(c["stored"], k, row_ids=c["ids"], method=method, stats=stats)
            what = f"{shape} {name} ids {mode} k {k} {method}: {stats}"
            print("knn", what)
            assert ids.dtype == np.int64 and nbrs.dtype == np.int64 and scores.dtype == np.float32
            assert np.array_equal(ids, want_ids) and np.all(np.diff(ids) > 0), what
            assert nbrs.shape == scores.shape == want_n.shape == (live, max(0, min(k, live - 1))), what
            assert not (nbrs == ids[:, None]).any(), f"{what}: a row is its own neighbour"
            assert np.array_equal(nbrs, want_n), f"{what}: rows {np.flatnonzero((nbrs != want_n).any(axis=1))[:5]} differ"
            assert np.array_equal(scores.view(np.uint32), want_s.view(np.uint32)), f"{what}: scores are not the rerank's bits"
            assert np.all(np.diff(scores, axis=1) <= 0)
            # the scan path does not hide behind the gather
            scanning = method == "scan" or (method == "auto" and 2 * k <= scan_max_window())
            assert stats["rows"] == m and stats["live"] == live and 0 < stats["epsilon"] <= 2.0 ** -7
            assert stats["window"] == ((1 << (2 * k - 1).bit_length()) if scanning and k < 70 else 128 if scanning else 0)
            if live >= 2:
                assert stats["settled_first_pass"] + stats["gathered"] == live, what
                assert stats["chunks"] == 1
                if not scanning:
                    assert stats["gathered"] == live and stats["settled_first_pass"] == 0
                elif dim == 1 and m >= 257:
                    assert stats["gathered"] == live, what          # (every cosine is +-1: nothing can be told apart)
                elif k == 5 and dim >= 17 and name in ("float32", "bfloat16", "float16"):
                    assert stats["settled_first_pass"] >= 0.9 * live, what
            else:
                assert stats["settled_first_pass"] == stats["gathered"] == 0


def test_device_tensors_on_request():
    from lshrs_amd import exact_knn

    c = _case(700, 100, "float16", "descending")
    ids, nbrs, scores = exact_knn(c["stored"], 5, row_ids=c["ids"])
    t_ids, t_n, t_s = exact_knn(c["stored"], 5, row_ids=c["ids"], return_tensors=True)
    assert t_ids.is_cuda and t_n.is_cuda and t_s.is_cuda
    assert np.array_equal(t_ids.cpu().numpy(), ids) and np.array_equal(t_n.cpu().numpy(), nbrs)
    assert np.array_equal(t_s.cpu().numpy().view(np.uint32), scores.view(np.uint32))


def test_many_chunks_are_one_answer(monkeypatch):
    """A budget that cuts 700 rows into chunks of one block of 64: the same answer as in one chunk, scan and gather."""
    from lshrs_amd import _exact, exact_knn

    c = _case(700, 17, "bfloat16", "dead")
    want = {method: exact_knn(c["stored"], 5, row_ids=c["ids"], method=method) for method in ("scan", "gather")}
    monkeypatch.setattr(_exact, "_PAIRS_QUERY_BYTES", 64 * (4 * 17 + 16 * 16))
    monkeypatch.setattr(_exact, "_pairs_block", lambda lib, m, dim: 64)
    for method in ("scan", "gather"):
        stats = {}
        got = exact_knn(c["stored"], 5, row_ids=c["ids"], method=method, stats=stats)
        assert stats["chunks"] >= (11 if method == "scan" else 3) and stats["settled_first_pass"] + stats["gathered"] == stats["live"]
        for a, b in zip(got, want[method]):
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


# ------------------------------------------------------------------------------------------
# 3. the surface
# ------------------------------------------------------------------------------------------
def test_zero_rows_and_bad_arguments():
    torch = _torch()
    from lshrs_amd import exact_knn

    c = _case(257, 64, "float32", "none")
    zx = c["stored"].clone()
    zx[200] = 0
    for method in ("scan", "gather"):
        with pytest.raises(ValueError, match="Cannot normalize zero vector"):
            exact_knn(zx, 5, method=method)
        ids = torch.arange(257, device="cuda")
        ids[200] = -1                                       # (a dead zero row is nobody's business)
        got_ids, nbrs, _ = exact_knn(zx, 5, row_ids=ids, method=method)
        assert got_ids.shape == (256,) and 200 not in set(got_ids.tolist()) and not (nbrs == 200).any()
    with pytest.raises(ValueError, match="row_ids"):
        exact_knn(c["stored"], 5, row_ids=np.arange(256))
    with pytest.raises(ValueError, match="k must be > 0"):
        exact_knn(c["stored"], 0)
    with pytest.raises(ValueError, match="method"):
        exact_knn(c["stored"], 5, method="fast")
    none = {}
    ids, nbrs, scores = exact_knn(c["stored"][:0], 5, stats=none)
    assert ids.shape == (0,) and nbrs.shape == scores.shape == (0, 0) and none["rows"] == none["live"] == none["chunks"] == 0
    ids, nbrs, scores = exact_knn(c["stored"][:1], 5)
    assert ids.tolist() == [0] and nbrs.shape == scores.shape == (1, 0)


@pytest.mark.parametrize("name", ("bfloat16", "float8_e4m3fn"))
def test_store_neighbors_after_add_readd_remove_and_compact(name):
    """Superseded and erased rows stay in the block - here they are exact copies of live rows - and are nobody's neighbour; the
    answer, under the caller's ids, does not move when compact() moves the rows."""
    torch = _torch()
    from lshrs_amd import DeviceVectors, exact_knn

    m, dim = 700, 64
    X = _rows(m, dim)
    rng = np.random.default_rng(5)
    ids = rng.permutation(np.arange(m, dtype=np.int64) * 7 + 3)
    store = DeviceVectors(dim, name)
    store.add(ids, X)
    again = np.arange(0, 60, 3)
    store.add(ids[again], X[again + 100])
    gone = np.arange(300, 340)
    assert store.remove(ids[gone]) == gone.shape[0]
    got = store.neighbors(5)
    st = dict(store.last_search_stats)
    assert st["rows"] == m + again.shape[0] and st["live"] == m - gone.shape[0] == len(store)
    assert st["settled_first_pass"] + st["gathered"] == st["live"]
    final = X.copy()
    final[again] = X[again + 100]
    keep = np.setdiff1d(np.arange(m), gone)
    fresh = R._stored_form(torch, name, final[keep])
    want = exact_knn(fresh, 5, row_ids=ids[keep])
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                     b.view(np.uint32) if b.dtype == np.float32 else b)
    assert not (set(ids[gone].tolist()) & (set(got[0].tolist()) | set(got[1].ravel().tolist())))
    by_id = {i: nb for i, nb in zip(got[0].tolist(), got[1].tolist())}
    assert all(int(ids[i + 100]) in by_id[int(ids[i])] for i in again.tolist())       # (each re-added id sits next to its twin)
    store.compact()
    after = store.neighbors(5)
    assert store.last_search_stats["rows"] == m - gone.shape[0]
    for a, b in zip(after, got):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    t = store.neighbors(5, method="gather", return_tensors=True)
    assert t[0].is_cuda and np.array_equal(t[1].cpu().numpy(), got[1]) and store.last_search_stats["gathered"] == st["live"]
    with pytest.raises(ValueError, match="k must be > 0"):
        store.neighbors(0)
    empty = DeviceVectors(dim, name).neighbors(3)
    assert empty[0].shape == (0,) and empty[1].shape == (0, 0)


def test_lshrs_neighbors_exact():
    torch = _torch()
    from lshrs_amd import LSHRS, InMemoryStorage

    m, dim = 700, 64
    X = _rows(m, dim)
    ids = np.arange(m, dtype=np.int64) * 11 + 1
    idx = LSHRS(dim=dim, num_perm=128, storage=InMemoryStorage(), keep_vectors="bfloat16")
    idx.index(ids, X)
    got_ids, nbrs, scores = idx.neighbors_exact(5, return_arrays=True)
    s_ids, s_n, s_s = idx.vectors.neighbors(5)
    assert np.array_equal(got_ids, ids) and np.array_equal(got_ids, s_ids) and np.array_equal(nbrs, s_n) and np.array_equal(scores, s_s)
    assert nbrs.shape == (m, 5) and idx.last_search_stats["live"] == m
    assert idx.last_search_stats["settled_first_pass"] + idx.last_search_stats["gathered"] == m
    as_list = idx.neighbors_exact(5)
    assert [i for i, _ in as_list] == ids.tolist()
    assert [[n for n, _ in row] for _, row in as_list] == nbrs.tolist()
    assert np.array_equal(np.array([[s for _, s in row] for _, row in as_list], dtype=np.float32), scores)
    # without the vectors on the device: what search_exact raises; with an attached tensor: row i is id i
    plain = LSHRS(dim=dim, num_perm=128, storage=InMemoryStorage())
    plain.index(np.arange(m), X)
    with pytest.raises(RuntimeError, match="vector_fetch_fn must be supplied"):
        plain.neighbors_exact(5)
    plain.set_corpus(torch.from_numpy(X).cuda().to(torch.bfloat16))
    p_ids, p_n, p_s = plain.neighbors_exact(5, return_arrays=True)
    assert np.array_equal(p_ids * 11 + 1, ids) and np.array_equal(p_n * 11 + 1, nbrs) and np.array_equal(p_s, scores)
    with pytest.raises(ValueError, match="k must be > 0"):
        plain.neighbors_exact(0)
