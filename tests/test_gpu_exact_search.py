"""Exact top-k search over device-resident rows (lshrs_amd.exact_top_k, DeviceVectors.search, LSHRS.search_exact / recall) and
the scan kernel behind it (csrc/scan.hip, lshrs_scan_topk_*), on the GPU.

The reference is oracle.top_k_cosine over the rows AS STORED (upcast to float32), the judge tests/_ranking.judge_ranking with
its default tolerances.  "Planted" data gives every query exactly k near neighbours (cosine >= 0.84) and a wide gap below them
(<= 0.61): with that gap any honest epsilon settles every query in the first pass, so a pass through the gather path would
hide a broken scan - `gathered == 0` is asserted.  References are computed once per (shape, dtype) and shared."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests._ranking import cosines_f64, judge_ranking

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "bfloat16", "float16", "int8", "float8_e4m3fn")
# (n, dim, q, k): a dim that is no multiple of the MFMA k (100, 33), a dim longer than one k-chunk (100, 772), rows and queries
# that fill no tile, several row slices (6000, 20011), q below / at / above a tile of 64 (37, 65; 3), k of 1 and of 64
SHAPES = ((6000, 100, 37, 10), (20011, 64, 65, 10), (4097, 33, 5, 64), (3000, 772, 33, 10), (9000, 100, 3, 1))


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _stored_form(torch, name, x):
    """float32 rows as a device tensor of dtype `name`: torch's cast for 16 bits, quantize_rows for 8 (as
    tests/test_gpu_vector_store.py::_stored_form makes it)."""
    from lshrs_amd import quantize_rows

    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    if name == "float32":
        return xd.clone()
    if name in ("int8", "float8_e4m3fn"):
        return quantize_rows(xd, getattr(torch, name))
    return xd.to(getattr(torch, name))


def planted(seed, n, dim, q, k):
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((q, dim)).astype(np.float32)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    pos = rng.choice(n, q * k, replace=False).reshape(q, k)
    for i in range(q):
        X[pos[i]] = (Q[i] * rng.uniform(0.5, 2.0, (k, 1)) + 0.25 * rng.standard_normal((k, dim))).astype(np.float32)
    return Q, X, pos


def _reference(Q, rows_f32, k):
    from oracle import lshrs_oracle as O

    return [O.top_k_cosine(Q[i], rows_f32, k=k) for i in range(Q.shape[0])]


@functools.lru_cache(maxsize=None)
def _case(shape_index, name):
    """Planted data of one shape in one stored form, with the reference's answers (computed once, never modified)."""
    torch = _torch()
    n, dim, q, k = SHAPES[shape_index]
    Q, X, pos = planted(1, n, dim, q, k)
    stored = _stored_form(torch, name, X)
    upcast = stored.float().cpu().numpy()
    upcast.setflags(write=False)
    return {"Q": Q, "pos": pos, "stored": stored, "upcast": upcast, "k": k, "want": _reference(Q, upcast, k)}


def _judge_all(ids, scores, want, Q, cand, fetch):
    for i in range(Q.shape[0]):
        judge_ranking(list(zip(ids[i].tolist(), scores[i].tolist())), want[i], query=Q[i], candidates=cand, fetch=fetch)


def _ties_by_id(ids, scores):
    same = scores[:, 1:] == scores[:, :-1]
    assert np.all(ids[:, 1:][same] > ids[:, :-1][same]), "equal scores are not in ascending order of id"


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("shape_index", range(len(SHAPES)))
def test_scan_parity_with_the_reference(shape_index, name):
    torch = _torch()
    from lshrs_amd import exact_top_k, rerank_batch

    case = _case(shape_index, name)
    Q, k, up = case["Q"], case["k"], case["upcast"]
    n, q = up.shape[0], Q.shape[0]
    stats = {}
    ids, scores = exact_top_k(Q, case["stored"], k, method="scan", stats=stats)
    assert ids.shape == scores.shape == (q, k) and ids.dtype == np.int64 and scores.dtype == np.float32
    print("stats", SHAPES[shape_index], name, stats)
    _judge_all(ids, scores, case["want"], Q, np.arange(n), lambda c: up[np.asarray(c)])
    for i in range(q):
        assert set(ids[i].tolist()) == set(case["pos"][i].tolist()), f"query {i}: not the planted set"
    # a returned score is the rerank's score of that (query, row), bit for bit
    _, rr = rerank_batch(torch.from_numpy(Q).cuda(), case["stored"], torch.from_numpy(ids).cuda(), k=k, return_tensors=True)
    assert np.array_equal(scores.view(np.uint32), rr.cpu().numpy().view(np.uint32))
    _ties_by_id(ids, scores)
    assert stats["queries"] == q and stats["gathered"] == 0 and stats["settled_first_pass"] == q, stats
    assert 0 < stats["epsilon"] <= 2.0 ** -7 and stats["window"] == min(128, 1 << (2 * k - 1).bit_length())


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("shape_index", range(len(SHAPES)))
def test_scan_equals_gather(shape_index, name):
    from lshrs_amd import exact_top_k

    case = _case(shape_index, name)
    stats = {}
    a_ids, a_scores = exact_top_k(case["Q"], case["stored"], case["k"], method="scan")
    b_ids, b_scores = exact_top_k(case["Q"], case["stored"], case["k"], method="gather", stats=stats)
    assert stats["gathered"] == case["Q"].shape[0] and stats["settled_first_pass"] == 0
    assert np.array_equal(a_ids, b_ids)
    assert np.array_equal(a_scores.view(np.uint32), b_scores.view(np.uint32))


@pytest.mark.parametrize("name", DTYPES)
def test_dead_rows_and_sparse_ids(name):
    """Superseded and erased rows stay in the block - here they are its best-scoring rows - and must not be found."""
    torch = _torch()
    from lshrs_amd import DeviceVectors

    n, dim, q, k = SHAPES[0]
    Q, X, pos = planted(1, n, dim, q, k)
    rng = np.random.default_rng(77)
    ids = np.unique(rng.integers(0, 1 << 40, size=2 * n, dtype=np.int64))
    ids = rng.permutation(ids)[:n]
    store = DeviceVectors(dim, name)
    store.add(ids, X)
    again = pos[:, :k // 3].reshape(-1)                                 # a third of every planted set gets a fresh vector
    fresh = rng.standard_normal((again.shape[0], dim)).astype(np.float32)
    store.add(ids[again], fresh)
    gone = pos[:, k // 3:k // 3 + 2].reshape(-1)                        # two more of each leave
    assert store.remove(ids[gone]) == gone.shape[0]
    final = X.copy()
    final[again] = fresh
    keep = np.setdiff1d(np.arange(n), gone)
    live_ids = ids[keep]
    up = _stored_form(torch, name, final[keep]).float().cpu().numpy()
    want = [[(int(live_ids[p]), s) for p, s in row] for row in _reference(Q, up, k)]
    at = {int(i): j for j, i in enumerate(live_ids.tolist())}
    fetch = lambda c: up[[at[int(i)] for i in c]]                       # noqa: E731
    assert store.stats()["dead"] == again.shape[0] + gone.shape[0]
    got_ids, got_scores = store.search(Q, k)
    assert store.last_search_stats["queries"] == q
    _judge_all(got_ids, got_scores, want, Q, live_ids, fetch)
    dead = set(ids[gone].tolist())
    assert not dead & set(got_ids.reshape(-1).tolist())
    store.compact()
    assert store.stats()["dead"] == 0
    c_ids, c_scores = store.search(Q, k)
    _judge_all(c_ids, c_scores, want, Q, live_ids, fetch)
    assert np.array_equal(c_ids, got_ids) and np.array_equal(c_scores.view(np.uint32), got_scores.view(np.uint32))


@pytest.mark.parametrize("name", ("bfloat16", "int8"))
def test_ties_across_the_cut(name):
    """More equal-scoring rows than the widest window: the first pass cannot settle the query and must say so."""
    torch = _torch()
    from lshrs_amd import exact_top_k, scan_max_window

    dim, k = 100, 10
    rng = np.random.default_rng(5)
    v = rng.standard_normal(dim).astype(np.float32)
    ties = 3 * scan_max_window()
    X = np.concatenate([v[None] * rng.uniform(0.5, 2.0, (ties, 1)).astype(np.float32),
                        rng.standard_normal((2000, dim)).astype(np.float32)])
    X = X[rng.permutation(X.shape[0])]
    Q = v[None].copy()
    stored = _stored_form(torch, name, X)
    up = stored.float().cpu().numpy()
    want = _reference(Q, up, k)
    cand = np.arange(X.shape[0])
    stats = {}
    ids, scores = exact_top_k(Q, stored, k, method="scan", stats=stats)
    _judge_all(ids, scores, want, Q, cand, lambda c: up[np.asarray(c)])
    assert stats["settled_first_pass"] == 0 and stats["gathered"] == 1, stats
    _ties_by_id(ids, scores)
    g_ids, g_scores = exact_top_k(Q, stored, k, method="gather")
    _judge_all(g_ids, g_scores, want, Q, cand, lambda c: up[np.asarray(c)])
    assert np.array_equal(ids, g_ids) and np.array_equal(scores, g_scores)


def test_edges():
    torch = _torch()
    from lshrs_amd import exact_top_k, scan_max_window

    rng = np.random.default_rng(11)
    dim = 33
    X = rng.standard_normal((3000, dim)).astype(np.float32)
    Q = rng.standard_normal((7, dim)).astype(np.float32)
    xd = torch.from_numpy(X).cuda()
    cand = np.arange(3000)

    # k at or above the number of live rows: every live row, in order - through the scan (the window saw them all) ...
    small, stats = xd[:50], {}
    for k in (50, 64):
        ids, scores = exact_top_k(Q, small, k, method="scan", stats=stats)
        assert ids.shape == (7, 50) and stats["gathered"] == 0 and stats["settled_first_pass"] == 7
        _judge_all(ids, scores, _reference(Q, X[:50], 50), Q, cand[:50], lambda c: X[np.asarray(c)])
    # ... and through the gather, which "auto" takes when 2 k is beyond the widest window
    assert 2 * 300 > scan_max_window()
    for k in (300, 500):
        ids, scores = exact_top_k(Q, xd[:300], k, stats=stats)
        assert ids.shape == (7, 300) and stats["gathered"] == 7 and stats["window"] == 0
        _judge_all(ids, scores, _reference(Q, X[:300], 300), Q, cand[:300], lambda c: X[np.asarray(c)])
    ids, scores = exact_top_k(Q, xd, 100, stats=stats)
    assert stats["gathered"] == 7
    _judge_all(ids, scores, _reference(Q, X, 100), Q, cand, lambda c: X[np.asarray(c)])
    # k beyond the widest window forced through the scan: nothing settles, the gather answers
    f_ids, f_scores = exact_top_k(Q, xd, 200, method="scan", stats=stats)
    assert stats["settled_first_pass"] == 0 and stats["gathered"] == 7 and f_ids.shape == (7, 200)
    assert np.array_equal(f_ids[:, :100], ids)

    # no queries
    ids, scores = exact_top_k(np.empty((0, dim), np.float32), xd, 10, stats=stats)
    assert ids.shape == scores.shape == (0, 10) and ids.dtype == np.int64 and scores.dtype == np.float32
    assert stats["queries"] == 0 and stats["gathered"] == 0

    # zero vectors raise what the rerank raises
    zq = Q.copy()
    zq[3] = 0
    zx = xd.clone()
    zx[1234] = 0
    for method in ("scan", "gather"):
        with pytest.raises(ValueError, match="Cannot normalize zero vector"):
            exact_top_k(zq, xd, 10, method=method)
        with pytest.raises(ValueError, match="Cannot normalize zero vector"):
            exact_top_k(Q, zx, 10, method=method)
    rid = torch.arange(3000, device="cuda")
    rid[1234] = -1                                          # (a dead zero row is nobody's business)
    exact_top_k(Q, zx, 10, row_ids=rid, method="scan")

    # a row stride larger than dim: searched in place
    for dt in (torch.float32, torch.bfloat16, torch.int8):
        wide = torch.zeros((3000, dim + 31), dtype=dt, device="cuda")
        wide[:, :dim] = (xd * 20).to(dt)
        view = wide[:, :dim]
        assert view.stride(0) == dim + 31 and not view.is_contiguous()
        a = exact_top_k(Q, view, 10, method="scan", stats=stats)
        assert stats["gathered"] + stats["settled_first_pass"] == 7
        b = exact_top_k(Q, view.contiguous(), 10, method="gather")
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("method", ("auto", "scan", "gather"))
def test_rows_longer_than_the_kernels_take_raise_what_the_rerank_raises(method):
    """dim > 16 384 is beyond lshrs_scan_topk_* and beyond the rerank's own entries (lshrs_cosine_batch_* / _ragged_*): every
    method refuses such rows before any launch, with the error a rerank of them raises."""
    torch = _torch()
    from lshrs_amd import NativeLibraryError, exact_top_k, rerank_batch

    dim = 16385
    stored = torch.ones((40, dim), dtype=torch.bfloat16, device="cuda")
    Q = np.ones((3, dim), np.float32)
    with pytest.raises(NativeLibraryError, match="LSHRS_E_TOOLARGE"):
        rerank_batch(torch.from_numpy(Q).cuda(), stored, torch.arange(40, device="cuda").expand(3, 40).contiguous(), k=5)
    with pytest.raises(NativeLibraryError, match="LSHRS_E_TOOLARGE"):
        exact_top_k(Q, stored, 5, method=method)


def _f64_rows(torch, stored):
    return stored.float().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("positive", (False, True), ids=("gaussian", "positive"))
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("dim", (33, 100, 772, 1536))
def test_epsilon_is_honest(dim, name, positive):
    """lshrs_scan_topk_* called directly: every approximate score within lshrs_scan_epsilon of the float64 cosine of the stored
    row, and nothing outside a window could belong inside.  All-positive data: sum |q_i x_i| = q . x, the bound's worst case."""
    torch = _torch()
    from lshrs_amd import _native

    lib = _native.load()
    m, q, window = 5000, 33, 128
    rng = np.random.default_rng(1000 * dim + DTYPES.index(name) + 100 * positive)
    X = rng.standard_normal((m, dim)).astype(np.float32)
    Q = rng.standard_normal((q, dim)).astype(np.float32)
    if positive:
        X, Q = np.abs(X), np.abs(Q)
    stored = _stored_form(torch, name, X)
    suffix = _native.SCAN_ELEMS[DTYPES.index(name)]
    eps = float(lib.lshrs_scan_epsilon(DTYPES.index(name), dim))
    assert 0 < eps <= 2.0 ** -7
    qd = torch.from_numpy(Q).cuda()
    rows = torch.full((q, window), -7, dtype=torch.int64, device="cuda")
    approx = torch.full((q, window), float("nan"), dtype=torch.float32, device="cuda")
    count = torch.full((q,), -7, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    nbytes = int(lib.lshrs_scan_workspace_bytes(q, m, dim, window))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    fn = getattr(lib, "lshrs_scan_topk_" + suffix)
    _native.check(fn(stored.data_ptr(), m, stored.stride(0), dim, None, qd.data_ptr(), q, window, rows.data_ptr(),
                     approx.data_ptr(), count.data_ptr(), ws.data_ptr(), err.data_ptr(),
                     torch.cuda.current_stream().cuda_stream), "lshrs_scan_topk_" + suffix)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    rows, approx, count = rows.cpu().numpy(), approx.cpu().numpy().astype(np.float64), count.cpu().numpy()
    assert np.all(count == window)
    x64, q64 = _f64_rows(torch, stored), Q.astype(np.float64)
    truth = (q64 @ x64.T) / (np.linalg.norm(q64, axis=1)[:, None] * np.linalg.norm(x64, axis=1)[None, :])
    assert rows.min() >= 0 and rows.max() < m
    worst = 0.0
    for i in range(q):
        assert np.unique(rows[i]).shape[0] == window, f"query {i}: a row twice in the window"
        assert np.all(np.diff(approx[i]) <= 0), f"query {i}: approximate scores not in descending order"
        worst = max(worst, float(np.abs(approx[i] - truth[i, rows[i]]).max()))
        outside = np.ones(m, dtype=bool)
        outside[rows[i]] = False
        assert truth[i, outside].max() <= approx[i, -1] + eps, f"query {i}: a row outside the window belongs inside"
    print(f"dim {dim} {name} {'positive' if positive else 'gaussian'}: max |approx - cosine| {worst:.3e}, epsilon {eps:.3e}")
    assert worst <= eps


def test_scan_skips_dead_rows_directly():
    """row_ids at the C entry: negative entries are skipped, out_count is min(window, live rows), padding is -1 / -inf."""
    torch = _torch()
    from lshrs_amd._exact import scan_windows

    rng = np.random.default_rng(3)
    m, dim, q = 700, 64, 3
    X = torch.from_numpy(rng.standard_normal((m, dim)).astype(np.float32)).cuda()
    Q = torch.from_numpy(rng.standard_normal((q, dim)).astype(np.float32)).cuda()
    rid = torch.full((m,), -1, dtype=torch.int64, device="cuda")
    live = np.sort(rng.choice(m, 20, replace=False))
    rid[torch.from_numpy(live).cuda()] = torch.arange(20, device="cuda")
    rows, approx, count, err = scan_windows(X, Q, 32, rid)
    assert int(err.item()) == 0 and count.cpu().tolist() == [20] * q
    rows, approx = rows.cpu().numpy(), approx.cpu().numpy()
    for i in range(q):
        assert sorted(rows[i, :20].tolist()) == live.tolist()
        assert np.all(rows[i, 20:] == -1) and np.all(np.isneginf(approx[i, 20:]))
        want = cosines_f64(Q[i].cpu().numpy(), X.cpu().numpy()[rows[i, :20]])
        assert np.abs(approx[i, :20] - want).max() <= 1e-3


def test_lshrs_search_exact_and_recall():
    torch = _torch()
    from lshrs_amd import LSHRS, InMemoryStorage

    n, dim, q, k = SHAPES[0]
    Q, X, _ = planted(1, n, dim, q, k)
    rng = np.random.default_rng(9)
    ids = np.unique(rng.integers(0, 1 << 40, size=2 * n, dtype=np.int64))[:n]
    idx = LSHRS(dim=dim, num_perm=128, storage=InMemoryStorage(), keep_vectors="bfloat16")
    idx.index(ids, X)
    e_ids, e_scores = idx.search_exact(Q, k, return_arrays=True)
    s_ids, s_scores = idx.vectors.search(Q, k)
    assert np.array_equal(e_ids, s_ids) and np.array_equal(e_scores, s_scores)
    assert idx.last_search_stats["queries"] == q and idx.last_search_stats["gathered"] == 0
    as_lists = idx.search_exact(Q, k)
    assert [[i for i, _ in row] for row in as_lists] == e_ids.tolist()
    assert np.array_equal(np.array([[s for _, s in row] for row in as_lists], dtype=np.float32), e_scores)
    rec = idx.recall(Q, top_k=k)
    lsh = idx.query_many(Q, top_k=k)
    mine = np.array([len(set(lsh[i]) & set(e_ids[i].tolist())) / k for i in range(q)], dtype=np.float32)
    assert np.array_equal(rec["per_query"], mine) and rec["per_query"].dtype == np.float32
    assert rec["recall"] == float(mine.mean()) and 0.0 <= rec["recall"] <= 1.0
    assert np.array_equal(rec["exact"], e_ids) and rec["returned"] == float(np.mean([len(a) for a in lsh]))
    print("recall of 8 x 16 on the planted shape:", rec["recall"], "returned", rec["returned"])

    # an attached tensor: row i is id i
    plain = LSHRS(dim=dim, num_perm=128, storage=InMemoryStorage())
    plain.index(np.arange(n), X)
    with pytest.raises(RuntimeError, match="vector_fetch_fn must be supplied"):
        plain.search_exact(Q, k)
    with pytest.raises(RuntimeError, match="vector_fetch_fn must be supplied"):
        plain.query_many(Q, top_k=None, top_p=0.5)          # (the rerank's own error, for comparison)
    tensor = torch.from_numpy(X).cuda().to(torch.bfloat16)
    plain.set_corpus(tensor)
    t_ids, t_scores = plain.search_exact(Q, k, return_arrays=True)
    at = {int(v): j for j, v in enumerate(ids.tolist())}
    assert np.array_equal(t_ids, np.vectorize(at.get)(e_ids)) and np.array_equal(t_scores, e_scores)
    rec2 = plain.recall(Q, top_k=k, top_p=1.0)
    assert 0.0 <= rec2["recall"] <= 1.0 and np.array_equal(rec2["exact"], t_ids)
    with pytest.raises(ValueError):
        plain.search_exact(Q[:, :50], k)
    with pytest.raises(ValueError):
        plain.search_exact(Q, 0)


@functools.lru_cache(maxsize=None)
def _unplanted(dim):
    """Gaussian rows and queries with no planted neighbours (made once, never modified)."""
    rng = np.random.default_rng(2024 + dim)
    X = rng.standard_normal((5000, dim)).astype(np.float32)
    Q = rng.standard_normal((70, dim)).astype(np.float32)
    return Q, X


@functools.lru_cache(maxsize=None)
def _unplanted_case(dim, name):
    """The unplanted data in one stored form, with every query's float64 cosines of the stored rows in descending order
    (computed once, never modified)."""
    torch = _torch()
    Q, X = _unplanted(dim)
    stored = _stored_form(torch, name, X)
    upcast = stored.float().cpu().numpy()
    ranked = -np.sort(-np.stack([cosines_f64(Q[i], upcast) for i in range(Q.shape[0])]), axis=1)
    for a in (upcast, ranked):
        a.setflags(write=False)
    return {"Q": Q, "stored": stored, "upcast": upcast, "ranked": ranked}


@pytest.mark.parametrize("k,window", ((2, 4), (3, 8), (5, 16), (8, 16), (17, 64), (32, 64)))
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("dim", (33, 100))
def test_every_window_through_exact_top_k(dim, name, k, window):
    """k of 2, 3, 5, 8, 17, 32: windows of 4, 8, 16, 16, 64, 64 - the widths between those the planted shapes reach, among them
    the selection's middle form (windows 33 .. 64, any k of 17 .. 32).  The data is not planted; that the first pass must settle
    every query is established from the data itself: every query's gap between its k-th and its window-th float64 cosine exceeds
    three times what the settle rule charges (epsilon + the rerank's rounding), where twice is what the rule needs."""
    from lshrs_amd import exact_top_k
    from lshrs_amd._exact import choose_window, rerank_rounding, scan_epsilon, scan_max_window

    case = _unplanted_case(dim, name)
    Q, stored, up, ranked = case["Q"], case["stored"], case["upcast"], case["ranked"]
    q, n = Q.shape[0], up.shape[0]
    assert choose_window(k, scan_max_window()) == window
    charged = scan_epsilon(stored.dtype, dim) + rerank_rounding(dim)
    gap = float((ranked[:, k - 1] - ranked[:, window - 1]).min())
    print(f"dim {dim} {name} k {k} window {window}: smallest gap {gap:.3e}, three times the charge {3 * charged:.3e}")
    assert gap > 3 * charged, "the data does not let the first pass settle every query: take another seed"
    stats = {}
    ids, scores = exact_top_k(Q, stored, k, method="scan", stats=stats)
    g_ids, g_scores = exact_top_k(Q, stored, k, method="gather")
    assert np.array_equal(ids, g_ids) and np.array_equal(scores.view(np.uint32), g_scores.view(np.uint32))
    _judge_all(ids, scores, _reference(Q, up, k), Q, np.arange(n), lambda c: up[np.asarray(c)])
    assert stats["window"] == window and stats["settled_first_pass"] == q and stats["gathered"] == 0, stats


@pytest.mark.parametrize("name", ("float32", "bfloat16"))
def test_rows_that_are_not_finite_are_in_no_answer(name):
    """A row holding a NaN or an infinity has no cosine: with k well below the number of finite rows it is in no answer, by
    either method, and the two agree."""
    torch = _torch()
    from lshrs_amd import exact_top_k

    Q, X = _unplanted(33)
    X = X[:3000].copy()
    rng = np.random.default_rng(6)
    bad = rng.choice(3000, 9, replace=False)
    for j, value in enumerate((np.nan, np.inf, -np.inf) * 3):
        X[bad[j], rng.integers(0, 33)] = value
    X[bad[0]] = np.nan                                      # (a row of nothing but NaN)
    X[bad[1], :2] = (np.inf, -np.inf)
    stored = _stored_form(torch, name, X)
    assert int((~torch.isfinite(stored.float())).any(dim=1).sum()) == 9
    up = stored.float().cpu().numpy()
    fine = np.setdiff1d(np.arange(3000), bad)
    for k in (1, 10, 32):
        stats = {}
        ids, scores = exact_top_k(Q, stored, k, method="scan", stats=stats)
        g_ids, g_scores = exact_top_k(Q, stored, k, method="gather")
        assert not set(bad.tolist()) & set(ids.reshape(-1).tolist()) and np.isfinite(scores).all()
        assert np.array_equal(ids, g_ids) and np.array_equal(scores.view(np.uint32), g_scores.view(np.uint32))
        want = [[(int(fine[p]), s) for p, s in row] for row in _reference(Q, up[fine], k)]
        _judge_all(ids, scores, want, Q, fine, lambda c: up[np.asarray(c)])
