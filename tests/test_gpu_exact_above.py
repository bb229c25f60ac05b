"""Range search over device-resident rows (lshrs_amd.exact_above, DeviceVectors.search_above, LSHRS.search_exact_above /
recall_above) and the kernel behind it (csrc/scan.hip, lshrs_scan_above_*), on the GPU.

The answer is DEFINED by the rerank's own score: a (query, live row) belongs to it exactly when the float32
lshrs_cosine_* gives that pair reaches float32(threshold).  So the ground truth of membership is rerank_batch over ALL rows - a
kernel older than this search - and equality with it is exact, ids and score bits.  The reference for the scores is
oracle.lshrs_oracle.cosine_similarity over the rows AS STORED (upcast to float32), the judge of membership
tests/_ranking.cosines_f64: whatever is above the threshold by the project's stated cosine tolerance (1e-5) is present,
whatever is below it by as much is absent.  "Planted" data (as tests/test_gpu_exact_search.py makes it) gives every query
exactly ten rows at a cosine >= 0.84 and nothing else above 0.61."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests._ranking import cosines_f64

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "bfloat16", "float16", "int8", "float8_e4m3fn")
# (n, dim, q): a dim that is no multiple of the MFMA k (100, 33), a dim longer than one k-chunk (100, 772), rows and queries
# that fill no tile, several row slices (6000, 20011), q below / above a tile of 64 (37, 5; 65); the last one: everything at once
SHAPES = ((6000, 100, 37), (20011, 64, 65), (3000, 772, 33), (4097, 33, 5), (300, 16, 3))
K = 10
TOL = 1e-5


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _stored_form(torch, name, x):
    """float32 rows as a device tensor of dtype `name`: torch's cast for 16 bits, quantize_rows for 8."""
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


@functools.lru_cache(maxsize=None)
def _planted_case(shape_index, name):
    """Planted data of one shape in one stored form (made once, never modified)."""
    torch = _torch()
    n, dim, q = SHAPES[shape_index]
    Q, X, pos = planted(1, n, dim, q, K)
    stored = _stored_form(torch, name, X)
    upcast = stored.float().cpu().numpy()
    upcast.setflags(write=False)
    return {"Q": Q, "pos": pos, "stored": stored, "upcast": upcast}


@functools.lru_cache(maxsize=None)
def _gauss_case(dim, name):
    """Gaussian rows and queries in one stored form, with the rerank's score of EVERY (query, row): rerank_batch over all rows,
    scattered back to a (q, n) matrix (computed once, never modified)."""
    torch = _torch()
    from lshrs_amd import rerank_batch

    n, q = 8000, 37
    rng = np.random.default_rng(100 + dim)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((q, dim)).astype(np.float32)
    stored = _stored_form(torch, name, X)
    upcast = stored.float().cpu().numpy()
    everything = torch.arange(n, dtype=torch.int64, device="cuda").unsqueeze(0).expand(q, n).contiguous()
    order, ranked = rerank_batch(torch.from_numpy(Q).cuda(), stored, everything, k=n, return_tensors=True)
    scores = torch.empty((q, n), dtype=torch.float32, device="cuda")
    scores.scatter_(1, order.long(), ranked)
    scores = scores.cpu().numpy()
    cos64 = np.stack([cosines_f64(Q[i], upcast) for i in range(q)])
    for a in (upcast, scores, cos64):
        a.setflags(write=False)
    return {"Q": Q, "stored": stored, "upcast": upcast, "rerank": scores, "cos64": cos64}


def _lists(ids, scores, bounds, q):
    assert ids.dtype == np.int64 and scores.dtype == np.float32 and bounds.dtype == np.int64
    assert bounds.shape == (q + 1,) and bounds[0] == 0 and np.all(np.diff(bounds) >= 0)
    assert ids.shape == scores.shape == (int(bounds[-1]),)
    return [(ids[bounds[i]:bounds[i + 1]], scores[bounds[i]:bounds[i + 1]]) for i in range(q)]


def _check_order(lists):
    for i, (ids, scores) in enumerate(lists):
        assert np.all(np.diff(scores) <= 0), f"query {i}: scores not in descending order"
        same = scores[1:] == scores[:-1]
        assert np.all(ids[1:][same] > ids[:-1][same]), f"query {i}: equal scores are not in ascending order of id"


def _check_against_oracle(lists, Q, rows_of, cos_of, thresholds):
    """Scores within TOL of the oracle's cosine of the stored rows; membership judged in float64: every row at or above
    t + TOL is there, none below t - TOL is.  rows_of(ids) -> stored rows (float32), cos_of(i) -> (ids, float64 cosines) of
    every live row for query i."""
    from oracle import lshrs_oracle as O

    for i, (ids, scores) in enumerate(lists):
        t = float(thresholds[i])
        if ids.shape[0]:
            want = O.cosine_similarity(Q[i], rows_of(ids))
            assert np.abs(scores.astype(np.float64) - want.astype(np.float64)).max() <= TOL, f"query {i}: score off the oracle's"
        all_ids, c64 = cos_of(i)
        must = set(all_ids[c64 >= t + TOL].tolist())
        may = set(all_ids[c64 >= t - TOL].tolist())
        got = set(ids.tolist())
        assert len(got) == ids.shape[0], f"query {i}: an id twice"
        assert must <= got, f"query {i}: {len(must - got)} rows above the threshold are missing"
        assert got <= may, f"query {i}: {len(got - may)} rows below the threshold were returned"


# ------------------------------------------------------------------------------------------
# 1. planted parity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("shape_index", range(4))
def test_planted_parity(shape_index, name):
    torch = _torch()
    from lshrs_amd import exact_above, rerank_batch

    case = _planted_case(shape_index, name)
    Q, up, pos = case["Q"], case["upcast"], case["pos"]
    n, q = up.shape[0], Q.shape[0]
    stats = {}
    ids, scores, bounds = exact_above(Q, case["stored"], 0.75, stats=stats)
    print("stats", SHAPES[shape_index], name, stats)
    lists = _lists(ids, scores, bounds, q)
    for i in range(q):
        assert set(lists[i][0].tolist()) == set(pos[i].tolist()), f"query {i}: not the planted set"
    assert np.array_equal(np.diff(bounds), np.full(q, K))
    _check_order(lists)
    # a returned score is the rerank's score of that (query, row), bit for bit: reranking each answer in its own order changes nothing
    order, rr = rerank_batch(torch.from_numpy(Q).cuda(), case["stored"], torch.from_numpy(ids.reshape(q, K)).cuda(), k=K,
                             return_tensors=True)
    assert np.array_equal(rr.cpu().numpy().view(np.uint32), scores.reshape(q, K).view(np.uint32))
    assert np.array_equal(order.cpu().numpy(), np.tile(np.arange(K), (q, 1)))
    every = np.arange(n)
    _check_against_oracle(lists, Q, lambda c: up[c], lambda i: (every, cosines_f64(Q[i], up)), [0.75] * q)
    assert stats["launches"] == 1 and stats["queries"] == q and stats["kept"] == q * K and stats["emitted"] >= q * K
    assert 0 < stats["epsilon"] <= 2.0 ** -7
    # device tensors on request: the same answer
    t_ids, t_scores, t_bounds = exact_above(torch.from_numpy(Q).cuda(), case["stored"], 0.75, return_tensors=True)
    assert t_ids.is_cuda and t_scores.is_cuda and t_bounds.is_cuda
    assert np.array_equal(t_ids.cpu().numpy(), ids) and np.array_equal(t_scores.cpu().numpy().view(np.uint32), scores.view(np.uint32))
    assert np.array_equal(t_bounds.cpu().numpy(), bounds)


# ------------------------------------------------------------------------------------------
# 2. boundary honesty: hundreds of pairs within 1e-3 of the threshold, none misjudged
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_query", (False, True), ids=("scalar", "per-query"))
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("dim", (33, 100))
def test_boundary_is_the_reranks(dim, name, per_query):
    from lshrs_amd import exact_above

    case = _gauss_case(dim, name)
    Q, up, truth = case["Q"], case["upcast"], case["rerank"]
    q, n = truth.shape
    thr = np.linspace(0.0, 0.3, q) if per_query else np.full(q, 0.2)
    t32 = thr.astype(np.float32)
    near = int((np.abs(case["cos64"] - thr[:, None]) <= 1e-3).sum())
    assert near >= 200, f"only {near} pairs within 1e-3 of the threshold: the data does not test the bar"
    stats = {}
    ids, scores, bounds = exact_above(Q, case["stored"], thr if per_query else 0.2, stats=stats)
    print("boundary", dim, name, "per-query" if per_query else "scalar", stats, "pairs within 1e-3:", near)
    lists = _lists(ids, scores, bounds, q)
    _check_order(lists)
    want = truth >= t32[:, None]                       # the rerank's score of every pair against float32(threshold)
    got = np.zeros((q, n), dtype=bool)
    mine = np.zeros((q, n), dtype=np.float32)
    for i, (row_ids, row_scores) in enumerate(lists):
        assert np.unique(row_ids).shape[0] == row_ids.shape[0]
        got[i, row_ids] = True
        mine[i, row_ids] = row_scores
    assert np.array_equal(got, want), (f"{int((want & ~got).sum())} pairs of the rerank's answer missing, "
                                       f"{int((got & ~want).sum())} returned that are not in it")
    assert np.array_equal(mine[want].view(np.uint32), truth[want].view(np.uint32)), "scores are not the rerank's bits"
    assert stats["kept"] == int(want.sum()) and stats["emitted"] >= stats["kept"]
    every = np.arange(n)
    _check_against_oracle(lists, Q, lambda c: up[c], lambda i: (every, case["cos64"][i]), thr)


# ------------------------------------------------------------------------------------------
# 3. capacity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("float32", "bfloat16", "int8"))
def test_capacity_at_the_c_entry(name):
    torch = _torch()
    from lshrs_amd import _native
    from lshrs_amd._exact import scan_above

    lib = _native.load()
    case = _gauss_case(100, name)
    stored, Q = case["stored"], case["Q"]
    m, dim = stored.shape
    q = Q.shape[0]
    qd = torch.from_numpy(Q).cuda()
    bars_h = np.linspace(0.19, 0.21, q).astype(np.float32)
    bars = torch.from_numpy(bars_h).cuda()
    # ample room: the count and the pairs themselves
    a_q, a_row, a_approx, a_total, err = scan_above(stored, qd, bars, 1 << 16)
    total = int(a_total.item())
    assert int(err.item()) == 0 and 3000 <= total <= 12000, total
    all_pairs = set(zip(a_q[:total].cpu().tolist(), a_row[:total].cpu().tolist()))
    assert len(all_pairs) == total
    assert bool((a_approx[:total] >= bars[a_q[:total].long()]).all())
    # every pair well above its bar is there, none well below (|approx - cosine| <= epsilon <= 2^-7)
    cos64 = case["cos64"]
    eps = float(lib.lshrs_scan_epsilon(DTYPES.index(name), dim))
    sure = set(zip(*np.nonzero(cos64 >= bars_h[:, None].astype(np.float64) + eps + 1e-6)))
    maybe = set(zip(*np.nonzero(cos64 >= bars_h[:, None].astype(np.float64) - eps - 1e-6)))
    assert sure <= all_pairs <= maybe

    fn = getattr(lib, "lshrs_scan_above_" + _native.SCAN_ELEMS[DTYPES.index(name)])
    ws = torch.empty(int(lib.lshrs_scan_above_workspace_bytes(q, m, dim)), dtype=torch.uint8, device="cuda")
    cap, guard = 100, 64
    o_q = torch.full((cap + guard,), -7, dtype=torch.int32, device="cuda")
    o_row = torch.full((cap + guard,), -7, dtype=torch.int64, device="cuda")
    o_approx = torch.full((cap + guard,), -7.0, dtype=torch.float32, device="cuda")
    count = torch.full((1,), 123456789, dtype=torch.int64, device="cuda")        # (the entry zeroes it)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _native.check(fn(stored.data_ptr(), m, stored.stride(0), dim, None, qd.data_ptr(), q, bars.data_ptr(), cap, o_q.data_ptr(),
                     o_row.data_ptr(), o_approx.data_ptr(), count.data_ptr(), ws.data_ptr(), err.data_ptr(), stream), "above")
    torch.cuda.synchronize()
    assert int(count.item()) == total and int(err.item()) == 0
    first = list(zip(o_q[:cap].cpu().tolist(), o_row[:cap].cpu().tolist()))
    assert len(set(first)) == cap and set(first) <= all_pairs
    assert bool((o_approx[:cap] >= bars[o_q[:cap].long()]).all())
    assert bool((o_q[cap:] == -7).all()) and bool((o_row[cap:] == -7).all()) and bool((o_approx[cap:] == -7.0).all())
    # no slots at all: the same count, nothing needed to write to
    count.fill_(-1)
    _native.check(fn(stored.data_ptr(), m, stored.stride(0), dim, None, qd.data_ptr(), q, bars.data_ptr(), 0, None, None, None,
                     count.data_ptr(), ws.data_ptr(), err.data_ptr(), stream), "above")
    torch.cuda.synchronize()
    assert int(count.item()) == total


def test_capacity_through_exact_above(monkeypatch):
    from lshrs_amd import _exact, exact_above

    case = _gauss_case(100, "bfloat16")
    Q, stored = case["Q"], case["stored"]
    q = Q.shape[0]
    one = {}
    ids, scores, bounds = exact_above(Q, stored, 0.2, stats=one)
    assert one["launches"] == 1 and one["emitted"] > 64 * q
    monkeypatch.setattr(_exact, "_ABOVE_FIRST_CAPACITY", 64)
    two = {}
    ids2, scores2, bounds2 = exact_above(Q, stored, 0.2, stats=two)
    assert two["launches"] == 2 and two["emitted"] == one["emitted"] and two["kept"] == one["kept"]
    assert np.array_equal(ids, ids2) and np.array_equal(scores.view(np.uint32), scores2.view(np.uint32))
    assert np.array_equal(bounds, bounds2)
    # more pairs than the caller allows: refused by number, whatever the first capacity
    for limit in (one["emitted"] - 1, 64 * q + 1, 10, 0):
        with pytest.raises(ValueError, match=f"{one['emitted']} pairs.*max_pairs = {limit}"):
            exact_above(Q, stored, 0.2, max_pairs=limit)
    monkeypatch.undo()
    with pytest.raises(ValueError, match=f"{one['emitted']} pairs.*max_pairs = 1000"):
        exact_above(Q, stored, 0.2, max_pairs=1000)
    exactly = {}
    ids3, _, _ = exact_above(Q, stored, 0.2, max_pairs=one["emitted"], stats=exactly)
    assert np.array_equal(ids3, ids) and exactly["launches"] == 1


# ------------------------------------------------------------------------------------------
# 4. dead rows and sparse ids
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DTYPES)
def test_dead_rows_and_sparse_ids(name):
    """Superseded and erased rows stay in the block - here they are its best-scoring rows - and must not be found."""
    torch = _torch()
    from lshrs_amd import DeviceVectors, exact_above

    n, dim, q = SHAPES[0]
    Q, X, pos = planted(1, n, dim, q, K)
    rng = np.random.default_rng(77)
    ids = np.unique(rng.integers(0, 1 << 62, size=2 * n, dtype=np.int64))
    ids = rng.permutation(ids)[:n]
    stored = _stored_form(torch, name, X)
    up = stored.float().cpu().numpy()
    best = np.stack([pos[i][np.argsort(-cosines_f64(Q[i], up[pos[i]]))] for i in range(q)])
    ids[best[0, K - 1]] = 1 << 62                                       # (a row that stays live, under the largest id)
    assert np.unique(ids).shape[0] == n

    # row_ids at exact_above itself: the three best rows of every query are dead
    row_ids = ids.copy()
    row_ids[best[:, :3].reshape(-1)] = -1
    got_ids, got_scores, bounds = exact_above(Q, stored, 0.75, row_ids=row_ids)
    lists = _lists(got_ids, got_scores, bounds, q)
    _check_order(lists)
    for i in range(q):
        assert set(lists[i][0].tolist()) == set(ids[best[i, 3:]].tolist()), f"query {i}"
    assert (1 << 62) in set(lists[0][0].tolist())
    plain_ids, plain_scores, plain_bounds = exact_above(Q, stored, 0.75)
    at = {int(v): j for j, v in enumerate(ids.tolist())}
    for i in range(q):                                                  # the scores are those of the same rows without row_ids
        mine = dict(zip(lists[i][0].tolist(), lists[i][1].tolist()))
        theirs = dict(zip(plain_ids[plain_bounds[i]:plain_bounds[i + 1]].tolist(),
                          plain_scores[plain_bounds[i]:plain_bounds[i + 1]].tolist()))
        assert all(theirs[at[k]] == v for k, v in mine.items())

    # the same through a store: add, add again (the old rows are superseded), remove
    store = DeviceVectors(dim, name)
    store.add(ids, X)
    again = pos[:, :3].reshape(-1)                                      # three of every planted set get a fresh vector
    fresh = rng.standard_normal((again.shape[0], dim)).astype(np.float32)
    store.add(ids[again], fresh)
    gone = pos[:, 3:5].reshape(-1)                                      # two more of each leave
    assert store.remove(ids[gone]) == gone.shape[0]
    assert store.stats()["dead"] == again.shape[0] + gone.shape[0]
    s_ids, s_scores, s_bounds = store.search_above(Q, 0.75)
    assert store.last_search_stats["queries"] == q and store.last_search_stats["launches"] == 1
    s_lists = _lists(s_ids, s_scores, s_bounds, q)
    _check_order(s_lists)
    for i in range(q):
        assert set(s_lists[i][0].tolist()) == set(ids[pos[i, 5:]].tolist()), f"query {i}: superseded or erased rows"
    final = X.copy()
    final[again] = fresh
    keep = np.setdiff1d(np.arange(n), gone)
    live_up = _stored_form(torch, name, final[keep]).float().cpu().numpy()
    live_ids = ids[keep]
    where = {int(v): j for j, v in enumerate(live_ids.tolist())}
    _check_against_oracle(s_lists, Q, lambda c: live_up[[where[int(v)] for v in c]],
                          lambda i: (live_ids, cosines_f64(Q[i], live_up)), [0.75] * q)
    store.compact()
    c_ids, c_scores, c_bounds = store.search_above(Q, 0.75)
    assert np.array_equal(c_ids, s_ids) and np.array_equal(c_scores.view(np.uint32), s_scores.view(np.uint32))
    assert np.array_equal(c_bounds, s_bounds)
    with pytest.raises(ValueError):
        store.search_above(Q[:, :50], 0.75)


# ------------------------------------------------------------------------------------------
# 5. rows at any address and stride
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("float32", "bfloat16", "int8"))
@pytest.mark.parametrize("dim", (33, 100))
def test_unaligned_rows(dim, name):
    """An odd row stride and a base one element into the allocation: the scan's element-wise loads (ALIGNED = false).  The
    answer is the one the definition gives on that view - rerank_batch over all of its rows, cut at the threshold - and it equals
    that of an aligned copy (16-byte base, row stride a multiple of 16 elements: ALIGNED = true), ids and score bits.  The
    rerank's own kernel sums a row in another order when IT can use vector loads (dim and stride multiples of 4 / 8 / 16
    elements for 32 / 16 / 8 bits), so its scores of the two layouts - the scores returned - are the same bits only where dim
    rules that out; there the two answers are compared exactly, and elsewhere each against its own layout's rerank."""
    torch = _torch()
    from lshrs_amd import exact_above, rerank_batch

    case = _gauss_case(dim, name)
    Q, stored = case["Q"], case["stored"]
    n, q = stored.shape[0], Q.shape[0]
    ld = dim + (3 if dim % 2 == 0 else 4)
    assert ld % 2 == 1
    flat = torch.zeros(n * ld + 1, dtype=stored.dtype, device="cuda")
    view = torch.as_strided(flat, (n, dim), (ld, 1), 1)
    view.copy_(stored)
    assert view.stride(0) == ld and view.data_ptr() == flat.data_ptr() + flat.element_size() and view.data_ptr() % 16 != 0
    wide = torch.zeros((n, (dim + 15) // 16 * 16 + 16), dtype=stored.dtype, device="cuda")
    wide[:, :dim] = stored
    copy = wide[:, :dim]
    assert copy.data_ptr() % 16 == 0 and copy.stride(0) % 16 == 0 and torch.equal(copy, view)
    thr = np.linspace(0.0, 0.3, q)
    t32 = thr.astype(np.float32)
    qd = torch.from_numpy(Q).cuda()
    everything = torch.arange(n, dtype=torch.int64, device="cuda").unsqueeze(0).expand(q, n).contiguous()
    answers, reranks = [], []
    for rows in (view, copy):
        ids, scores, bounds = exact_above(Q, rows, thr)
        lists = _lists(ids, scores, bounds, q)
        _check_order(lists)
        order, ranked = rerank_batch(qd, rows, everything, k=n, return_tensors=True)
        truth = torch.empty((q, n), dtype=torch.float32, device="cuda")
        truth.scatter_(1, order.long(), ranked)
        truth = truth.cpu().numpy()
        want = truth >= t32[:, None]
        got = np.zeros((q, n), dtype=bool)
        mine = np.zeros((q, n), dtype=np.float32)
        for i, (row_ids, row_scores) in enumerate(lists):
            got[i, row_ids] = True
            mine[i, row_ids] = row_scores
        assert ids.shape[0] > 1000 and np.array_equal(got, want)
        assert np.array_equal(mine[want].view(np.uint32), truth[want].view(np.uint32))
        answers.append((ids, scores, bounds))
        reranks.append(truth)
    a, b = answers
    if dim % {"float32": 4, "bfloat16": 8, "int8": 16}[name]:          # (the rerank reads both layouts element by element)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        assert np.array_equal(a[2], b[2])
    else:
        # f32 at 100-d: the rerank's two summation orders may differ in a score's last bits, and the answers with them - but only
        # so: a pair that is in one answer alone has rerank scores of the two layouts that straddle float32(t) and lie within twice
        # the rerank's rounding bound of each other, and a pair in both has its own layout's score in each (checked above)
        ra, rb = reranks
        from lshrs_amd._exact import rerank_rounding

        assert np.abs(ra.astype(np.float64) - rb).max() <= 2 * rerank_rounding(dim)     # (each within it of the cosine)
        only_one = (ra >= t32[:, None]) != (rb >= t32[:, None])
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        assert np.all((lo < t32[:, None])[only_one] & (hi >= t32[:, None])[only_one])
        in_a = np.zeros((q, n), dtype=bool)
        in_b = np.zeros((q, n), dtype=bool)
        in_a[np.repeat(np.arange(q), np.diff(a[2])), a[0]] = True
        in_b[np.repeat(np.arange(q), np.diff(b[2])), b[0]] = True
        assert np.array_equal(in_a != in_b, only_one)


# ------------------------------------------------------------------------------------------
# 6. edges
# ------------------------------------------------------------------------------------------
def test_edges():
    torch = _torch()
    from lshrs_amd import DeviceVectors, exact_above

    n, dim, q = SHAPES[4]
    rng = np.random.default_rng(11)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((q, dim)).astype(np.float32)
    xd = torch.from_numpy(X).cuda()

    # no queries
    stats = {}
    ids, scores, bounds = exact_above(np.empty((0, dim), np.float32), xd, 0.5, stats=stats)
    assert ids.shape == scores.shape == (0,) and ids.dtype == np.int64 and scores.dtype == np.float32
    assert bounds.tolist() == [0] and bounds.dtype == np.int64 and stats["queries"] == 0 and stats["launches"] == 0
    ids, _, bounds = exact_above(np.empty((0, dim), np.float32), xd, np.empty(0))
    assert ids.shape == (0,) and bounds.tolist() == [0]

    # a threshold of 1 and no duplicate of a query among the rows: nothing
    ids, scores, bounds = exact_above(Q, xd, 1.0, stats=stats)
    assert ids.shape == scores.shape == (0,) and bounds.tolist() == [0] * (q + 1) and stats["kept"] == 0
    # ... a duplicate (up to a scale) is found by it or is not, as the rerank's rounding of that pair has it
    dup = torch.cat([xd, torch.from_numpy(2 * Q[1:2]).cuda()])
    ids, scores, bounds = exact_above(Q, dup, 1.0)
    assert set(ids.tolist()) <= {n} and bounds[1] == 0 and bounds[-1] == bounds[2]
    ids, scores, bounds = exact_above(Q, dup, 0.9999)
    assert ids.tolist() == [n] and np.diff(bounds).tolist() == [0, 1, 0] and abs(float(scores[0]) - 1.0) <= TOL

    # a threshold of -1: every pair, in order
    ids, scores, bounds = exact_above(Q, xd, -1.0, stats=stats)
    assert ids.shape == (q * n,) and bounds.tolist() == [0, n, 2 * n, 3 * n] and stats["kept"] == stats["emitted"] == q * n
    lists = _lists(ids, scores, bounds, q)
    _check_order(lists)
    for i in range(q):
        assert np.array_equal(np.sort(lists[i][0]), np.arange(n))
        want = cosines_f64(Q[i], X)[lists[i][0]]
        assert np.abs(lists[i][1] - want).max() <= TOL

    # no live row: row_ids all negative, an empty store, a store emptied
    ids, _, bounds = exact_above(Q, xd, -1.0, row_ids=np.full(n, -1, dtype=np.int64), stats=stats)
    assert ids.shape == (0,) and bounds.tolist() == [0] * (q + 1) and stats["emitted"] == 0
    store = DeviceVectors(dim, "float32")
    ids, _, bounds = store.search_above(Q, -1.0)
    assert ids.shape == (0,) and bounds.tolist() == [0] * (q + 1)
    store.add(np.arange(5), X[:5])
    assert store.search_above(Q, -1.0)[0].shape == (5 * q,)
    assert store.remove(np.arange(5)) == 5
    ids, _, bounds = store.search_above(Q, -1.0)
    assert ids.shape == (0,) and bounds.tolist() == [0] * (q + 1)

    # zero vectors raise what the rerank raises
    zq = Q.copy()
    zq[1] = 0
    zx = xd.clone()
    zx[123] = 0
    with pytest.raises(ValueError, match="Cannot normalize zero vector"):
        exact_above(zq, xd, 0.5)
    with pytest.raises(ValueError, match="Cannot normalize zero vector"):
        exact_above(Q, zx, 0.5)
    rid = torch.arange(n, device="cuda")
    rid[123] = -1                                           # (a dead zero row is nobody's business)
    assert exact_above(Q, zx, -1.0, row_ids=rid)[0].shape == (q * (n - 1),)

    # shapes that do not fit
    with pytest.raises(ValueError):
        exact_above(Q[:, :8], xd, 0.5)
    with pytest.raises(ValueError):
        exact_above(Q, xd, 0.5, row_ids=np.arange(n - 1))
    with pytest.raises(ValueError, match="threshold"):
        exact_above(Q, xd, [0.5, 0.5])


def test_negative_zero_ties_with_zero():
    """Equal scores go by ascending id, and -0.0 equals 0.0.  Row 0 scores -0.0 (a dot product of -1e-30 over norms of 1e10
    each: the quotient underflows), row 1 scores 0.0, row 2 is the query: the answer is [2, 0, 1] - an order by the scores' bits
    would put row 1 before row 0.  The same through the self-join's ordering: the pairs (0, 1) at -0.0 and (0, 2) at 0.0."""
    torch = _torch()
    from lshrs_amd import exact_above, exact_pairs_above

    q = np.array([[1e-15, 1e10, 0.0, 0.0]], dtype=np.float32)
    rows = np.array([[-1e-15, 0.0, 1e10, 0.0], [0.0, 0.0, 1e10, 0.0], [1e-15, 1e10, 0.0, 0.0]], dtype=np.float32)
    ids, scores, bounds = exact_above(q, torch.from_numpy(rows).cuda(), -0.5)
    assert bounds.tolist() == [0, 3] and scores[0] > 0.9
    assert scores[1:].tolist() == [0.0, 0.0] and np.signbit(scores[1:]).tolist() == [True, False], scores
    assert ids.tolist() == [2, 0, 1]
    pair_rows = np.array([[1e-15, 1e10, 0.0, 0.0], [-1e-15, 0.0, 1e10, 0.0], [0.0, 0.0, 0.0, 1e10]], dtype=np.float32)
    ia, ib, ps = exact_pairs_above(torch.from_numpy(pair_rows).cuda(), -0.5)
    assert ps.tolist() == [0.0, 0.0, 0.0] and np.signbit(ps).tolist() == [True, False, False], ps
    assert list(zip(ia.tolist(), ib.tolist())) == [(0, 1), (0, 2), (1, 2)]


def test_rows_longer_than_the_kernels_take_raise_what_the_rerank_raises():
    torch = _torch()
    from lshrs_amd import NativeLibraryError, exact_above, rerank_batch

    dim = 16385
    stored = torch.ones((40, dim), dtype=torch.bfloat16, device="cuda")
    Q = np.ones((3, dim), np.float32)
    with pytest.raises(NativeLibraryError, match="LSHRS_E_TOOLARGE"):
        rerank_batch(torch.from_numpy(Q).cuda(), stored, torch.arange(40, device="cuda").expand(3, 40).contiguous(), k=5)
    with pytest.raises(NativeLibraryError, match="LSHRS_E_TOOLARGE"):
        exact_above(Q, stored, 0.5)


# ------------------------------------------------------------------------------------------
# 7. LSHRS.search_exact_above / recall_above
# ------------------------------------------------------------------------------------------
def test_lshrs_search_exact_above_and_recall_above():
    torch = _torch()
    from lshrs_amd import LSHRS, InMemoryStorage

    n, dim, q = 4000, 64, 50
    Q, X, pos = planted(3, n, dim, q, K)
    rng = np.random.default_rng(9)
    ids = np.unique(rng.integers(0, 1 << 40, size=2 * n, dtype=np.int64))[:n]
    idx = LSHRS(dim=dim, num_perm=128, storage=InMemoryStorage(), keep_vectors="bfloat16")
    idx.index(ids, X)
    t = 0.75
    e_ids, e_scores, e_bounds = idx.search_exact_above(Q, t, return_arrays=True)
    s_ids, s_scores, s_bounds = idx.vectors.search_above(Q, t)
    assert np.array_equal(e_ids, s_ids) and np.array_equal(e_scores, s_scores) and np.array_equal(e_bounds, s_bounds)
    assert idx.last_search_stats["queries"] == q and idx.last_search_stats["launches"] == 1
    for i in range(q):
        assert set(e_ids[e_bounds[i]:e_bounds[i + 1]].tolist()) == set(ids[pos[i]].tolist())
    as_lists = idx.search_exact_above(Q, t)
    assert len(as_lists) == q
    assert [i for row in as_lists for i, _ in row] == e_ids.tolist()
    assert np.array_equal(np.array([s for row in as_lists for _, s in row], dtype=np.float32), e_scores)
    assert [len(row) for row in as_lists] == np.diff(e_bounds).tolist()

    thr = np.where(np.arange(q) % 5 == 0, 0.999, t)                     # every fifth query: nothing that similar
    rec = idx.recall_above(Q, thr)
    truth = idx.search_exact_above(Q, thr)
    lsh = idx.query_many(Q, top_k=None)
    tsets, csets = [set(i for i, _ in row) for row in truth], [set(row) for row in lsh]
    assert all(len(c) == len(row) for c, row in zip(csets, lsh))
    pairs, found = sum(len(s) for s in tsets), sum(len(a & b) for a, b in zip(tsets, csets))
    cands = sum(len(c) for c in csets)
    assert pairs == (q - q // 5) * K
    assert rec["truth_pairs"] == pairs and rec["recall"] == found / pairs and rec["precision"] == found / cands
    assert rec["candidates"] == cands / q
    per = rec["per_query"]
    assert per.dtype == np.float32 and per.shape == (q,)
    for i in range(q):
        if tsets[i]:
            assert per[i] == np.float32(len(tsets[i] & csets[i]) / len(tsets[i]))
        else:
            assert np.isnan(per[i])
    assert 0.0 <= rec["expected"] <= 1.0 and 0.0 <= rec["recall"] <= 1.0
    print("recall_above of 8 x 16 at 0.75 on planted rows:", rec["recall"], "expected", rec["expected"], "precision",
          rec["precision"], "candidates", rec["candidates"])
    nothing = idx.recall_above(Q, 1.0)
    assert nothing["recall"] == 1.0 and nothing["truth_pairs"] == 0 and np.isnan(nothing["per_query"]).all()

    # without the vectors on the device: what search_exact raises; with an attached tensor: row i is id i
    plain = LSHRS(dim=dim, num_perm=128, storage=InMemoryStorage())
    plain.index(np.arange(n), X)
    with pytest.raises(RuntimeError, match="vector_fetch_fn must be supplied"):
        plain.search_exact(Q, K)
    with pytest.raises(RuntimeError, match="vector_fetch_fn must be supplied"):
        plain.search_exact_above(Q, t)
    with pytest.raises(RuntimeError, match="vector_fetch_fn must be supplied"):
        plain.recall_above(Q, t)
    plain.set_corpus(torch.from_numpy(X).cuda().to(torch.bfloat16))
    t_ids, t_scores, t_bounds = plain.search_exact_above(Q, t, return_arrays=True)
    at = {int(v): j for j, v in enumerate(ids.tolist())}
    assert np.array_equal(t_bounds, e_bounds) and np.array_equal(t_scores, e_scores)
    for i in range(q):                                                  # (equal scores order by id: compare as sets)
        assert set(t_ids[t_bounds[i]:t_bounds[i + 1]].tolist()) == {at[v] for v in e_ids[e_bounds[i]:e_bounds[i + 1]].tolist()}
    with pytest.raises(ValueError):
        plain.search_exact_above(Q[:, :50], t)
    with pytest.raises(ValueError, match="threshold"):
        plain.search_exact_above(Q, 1.5)
