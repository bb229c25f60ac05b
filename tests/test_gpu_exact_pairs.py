"""The self-join over device-resident rows (lshrs_amd.exact_pairs_above, DeviceVectors.pairs_above, LSHRS.pairs_exact_above) and
the kernel behind it (csrc/scan.hip, lshrs_scan_pairs_*), on the GPU.  Both halves are asked for exactly:

the first pass   with a bar of -inf it emits EVERY pair (a < b, both live) once, and each approximate score equals the one the
                 range scan gives row b for row a as an f32 query (tests/_scan_reference.all_pairs_approx) - for the one-term
                 types that is the check that dropping the zero `mid` term's MFMA changed nothing;
the answer       exact_pairs_above equals the pairs (query id < row id) of exact_above(stored.float(), stored, t): the same set,
                 the same score bits, the documented order.  That oracle is older than the self-join.

Shapes: the smallest at which the kernel can go wrong - fewer rows than a tile (1, 2, 33), more than one pass of 256 (257,
700), dims below / at / across a chunk of 64 (1, 17, 64, 100) and many chunks (768), blocks of 64 and 128 query rows so that
700 rows span many blocks, diagonal tiles and skipped passes."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import _scan_reference as R

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "bfloat16", "float16", "int8", "float8_e4m3fn")
MS = (1, 2, 33, 257, 700)
DIMS = (1, 17, 64, 100, 768)
QBLOCKS = (0, 64, 128)
IDS = ("none", "dead", "descending")
# the public answer: every m and every dim at least twice, the 125 products are the first pass's
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
    """Rows in one stored form with one kind of row_ids (made once, never modified): `stored`, `ids` (device) / `ids_h`, and
    `Q`, the rows as float32 queries for the oracles - with ones in place of a dead zero row, which is nobody's query."""
    torch = _torch()
    stored = R._stored_form(torch, name, _rows(m, dim))
    ids_h = _row_ids(mode, m)
    Q = stored.float().contiguous()
    if mode == "dead" and m > 1:
        stored[1] = 0                                                   # a dead row of zero norm: it must raise nothing
        Q[1] = 1.0
    ids = None if ids_h is None else torch.from_numpy(ids_h).cuda()
    return {"stored": stored, "ids": ids, "ids_h": ids_h, "Q": Q}


@functools.lru_cache(maxsize=None)
def _approx(m, dim, name, mode):
    """all_pairs_approx of a case: (A (m, m) float32 - A[a, b]: row a asks, row b is scored -, live (m,) bool)."""
    c = _case(m, dim, name, mode)
    A, _ = R.all_pairs_approx(c["stored"], c["Q"], c["ids"])
    live = np.ones(m, dtype=bool) if c["ids_h"] is None else c["ids_h"] >= 0
    A.setflags(write=False)
    return A, live


def _raw_pairs(stored, bar, capacity, guard, row_ids, qblock):
    """lshrs_scan_pairs_* itself, the three arrays `guard` slots longer than `capacity` and filled with -7."""
    torch = _torch()
    from lshrs_amd import _native
    from lshrs_amd.similarity import corpus_suffix

    lib = _native.load()
    m, dim = int(stored.shape[0]), int(stored.shape[1])
    fn = getattr(lib, "lshrs_scan_pairs_" + corpus_suffix(stored))
    ws = torch.empty(int(lib.lshrs_scan_pairs_workspace_bytes(m, dim, qblock)), dtype=torch.uint8, device="cuda")
    o_a = torch.full((capacity + guard,), -7, dtype=torch.int64, device="cuda")
    o_b = torch.full((capacity + guard,), -7, dtype=torch.int64, device="cuda")
    o_s = torch.full((capacity + guard,), -7.0, dtype=torch.float32, device="cuda")
    total = torch.full((1,), 123456789, dtype=torch.int64, device="cuda")       # (the entry zeroes it)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    _native.check(fn(stored.data_ptr(), m, int(stored.stride(0)), dim, row_ids.data_ptr() if row_ids is not None else None,
                     float(bar), qblock, capacity, o_a.data_ptr(), o_b.data_ptr(), o_s.data_ptr(), total.data_ptr(),
                     ws.data_ptr(), err.data_ptr(), torch.cuda.current_stream().cuda_stream), "pairs")
    torch.cuda.synchronize()
    return o_a.cpu().numpy(), o_b.cpu().numpy(), o_s.cpu().numpy(), int(total.item()), int(err.item())


def _check_first_pass(stored, row_ids, A, live, qblock, what):
    """Everything of the first pass at a bar of -inf: the set, the count, the scores; then the same with too few slots."""
    from lshrs_amd._exact import scan_pairs

    m = int(stored.shape[0])
    n_live = int(live.sum())
    want = n_live * (n_live - 1) // 2
    a, b, s, total, err = scan_pairs(stored, float("-inf"), m * (m - 1) // 2, row_ids, qblock)
    assert int(err.item()) == 0, f"{what}: error word {int(err.item())}"
    assert int(total.item()) == want, f"{what}: total {int(total.item())}, {want} pairs of live rows"
    a, b, s = a[:want].cpu().numpy(), b[:want].cpu().numpy(), s[:want].cpu().numpy()
    assert np.all((0 <= a) & (a < b) & (b < m)), f"{what}: a pair that is not a < b within the rows"
    assert np.all(live[a] & live[b]), f"{what}: a dead row in a pair"
    assert np.unique(a * m + b).shape[0] == want, f"{what}: a pair twice"       # (want distinct pairs a < b of live rows: all)
    ref = A[a, b]
    assert not np.isnan(ref).any()
    bad = np.flatnonzero(~(s == ref))
    assert bad.shape[0] == 0, (f"{what}: {bad.shape[0]} approximate scores differ from the range scan's, first ({a[bad[0]]}, "
                               f"{b[bad[0]]}): {s[bad[0]]!r} != {ref[bad[0]]!r}")
    if want >= 2:
        cap, guard = want // 2, 64
        a2, b2, s2, total2, err2 = _raw_pairs(stored, float("-inf"), cap, guard, row_ids, qblock)
        assert total2 == want and err2 == 0, f"{what}: total {total2} with {cap} slots, {want} pairs"
        assert np.all(a2[cap:] == -7) and np.all(b2[cap:] == -7) and np.all(s2[cap:] == -7.0), f"{what}: written past capacity"
        a2, b2, s2 = a2[:cap], b2[:cap], s2[:cap]
        assert np.all((0 <= a2) & (a2 < b2) & (b2 < m)) and np.all(live[a2] & live[b2])
        assert np.unique(a2 * m + b2).shape[0] == cap and np.all(s2 == A[a2, b2]), f"{what}: the pairs that fitted"


# ------------------------------------------------------------------------------------------
# 1. the first pass, exactly
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("m", MS)
def test_first_pass_emits_every_pair_once_with_the_range_scans_score(m, dim, name):
    for mode in ("none", "dead"):
        c = _case(m, dim, name, mode)
        A, live = _approx(m, dim, name, mode)
        for qblock in QBLOCKS:
            _check_first_pass(c["stored"], c["ids"], A, live, qblock, f"{m} x {dim} {name}, ids {mode}, qblock {qblock}")


@pytest.mark.parametrize("name", DTYPES)
def test_first_pass_on_rows_at_any_address_and_stride(name):
    """A base one element into the allocation and an odd row stride: the element-wise loads (ALIGNED = false) of the pass and
    the prep kernels' reads; the scores are those of the same rows in a fresh allocation."""
    torch = _torch()
    m, dim = 257, 100
    c = _case(m, dim, name, "dead")
    A, live = _approx(m, dim, name, "dead")
    ld = dim + 3
    flat = torch.zeros(m * ld + 1, dtype=c["stored"].dtype, device="cuda")
    view = torch.as_strided(flat, (m, dim), (ld, 1), 1)
    view.copy_(c["stored"])
    assert view.stride(0) % 2 == 1 and view.data_ptr() % 16 != 0
    for qblock in (0, 64):
        _check_first_pass(view, c["ids"], A, live, qblock, f"unaligned {name}, qblock {qblock}")


@pytest.mark.parametrize("name", ("float32", "bfloat16"))
def test_first_pass_takes_nothing_from_behind_a_rows_last_element(name):
    """Rows of 70 elements at a stride of 128 (one whole chunk of 64 and a part of the next; 300 rows: one whole pass and a part
    of the next; blocks of 64: diagonal tiles and tiles off it), NaN in the 58 places behind each row.  The image of the query
    rows is zero beyond dim whatever the memory holds there: one NaN in it would make every score of its row NaN (0 * NaN), and
    no pair of that row would reach even a bar of -inf.  A two-term type and a one-term one."""
    torch = _torch()
    m, dim, ld = 300, 70, 128
    c = _case(m, dim, name, "dead")
    A, live = _approx(m, dim, name, "dead")
    flat = torch.full((m, ld), float("nan"), dtype=c["stored"].dtype, device="cuda")
    view = flat[:, :dim]
    view.copy_(c["stored"])
    assert view.stride(0) == ld and bool(torch.isnan(flat[:, dim:].float()).all())
    _check_first_pass(view, c["ids"], A, live, 64, f"NaN behind the rows, {name}")


def test_first_pass_with_a_bar():
    """A finite bar: exactly the pairs whose approximate score reaches it."""
    from lshrs_amd._exact import scan_pairs

    m, dim, name = 700, 17, "bfloat16"
    c = _case(m, dim, name, "dead")
    A, live = _approx(m, dim, name, "dead")
    bar = np.float32(0.5)
    upper = np.triu(np.ones((m, m), dtype=bool), 1) & live[:, None] & live[None, :]
    want = upper & (A >= bar)
    assert 100 <= int(want.sum()) < int(upper.sum()) // 4
    for qblock in QBLOCKS:
        a, b, s, total, err = scan_pairs(c["stored"], float(bar), int(want.sum()) + 10, c["ids"], qblock)
        n = int(total.item())
        assert n == int(want.sum()) and int(err.item()) == 0
        got = np.zeros((m, m), dtype=bool)
        got[a[:n].cpu().numpy(), b[:n].cpu().numpy()] = True
        assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------
# 2. the public answer, exactly
# ------------------------------------------------------------------------------------------
def _oracle_pairs(c, t):
    """The pairs (query id < row id) of exact_above(rows as float32 queries, rows, t), dead query rows dropped, in the documented
    order: descending score, equal scores by ascending (id_a, id_b)."""
    from lshrs_amd import exact_above

    m = int(c["stored"].shape[0])
    ids, scores, bounds = exact_above(c["Q"], c["stored"], t, row_ids=c["ids"])
    qid = np.arange(m, dtype=np.int64) if c["ids_h"] is None else c["ids_h"]
    asking = np.repeat(qid, np.diff(bounds))
    keep = (asking >= 0) & (asking < ids)
    ia, ib, s = asking[keep], ids[keep], scores[keep]
    order = np.lexsort((ib, ia, -s.astype(np.float64)))
    return ia[order], ib[order], s[order]


@pytest.mark.parametrize("mode", IDS)
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("shape", ANSWER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_answer_is_exact_aboves(shape, name, mode):
    from lshrs_amd import exact_pairs_above

    m, dim = shape
    c = _case(m, dim, name, mode)
    want_a, want_b, want_s = _oracle_pairs(c, T)
    stats = {}
    ids_a, ids_b, scores = exact_pairs_above(c["stored"], T, row_ids=c["ids"], stats=stats)
    print("pairs", shape, name, mode, stats)
    assert ids_a.dtype == np.int64 and ids_b.dtype == np.int64 and scores.dtype == np.float32
    assert ids_a.shape == ids_b.shape == scores.shape == want_a.shape, f"{ids_a.shape[0]} pairs, the oracle has {want_a.shape[0]}"
    assert np.all(ids_a < ids_b)
    assert np.array_equal(ids_a, want_a) and np.array_equal(ids_b, want_b)
    assert np.array_equal(scores.view(np.uint32), want_s.view(np.uint32)), "scores are not the rerank's bits"
    assert np.all(np.diff(scores) <= 0)
    assert stats["rows"] == m and stats["kept"] == want_a.shape[0] and stats["emitted"] >= stats["kept"]
    assert stats["launches"] == 1 and stats["blocks"] == 1 and 0 < stats["epsilon"] <= 2.0 ** -7
    if m >= 33 and dim >= 17:                               # (six planted copies; in "dead" mode some of their rows are dead)
        assert want_a.shape[0] >= (1 if mode == "dead" else 6), "the planted copies are not in the oracle's answer"


def test_device_tensors_on_request():
    from lshrs_amd import exact_pairs_above

    c = _case(700, 100, "float16", "descending")
    a, b, s = exact_pairs_above(c["stored"], T, row_ids=c["ids"])
    ta, tb, ts = exact_pairs_above(c["stored"], T, row_ids=c["ids"], return_tensors=True)
    assert ta.is_cuda and tb.is_cuda and ts.is_cuda
    assert np.array_equal(ta.cpu().numpy(), a) and np.array_equal(tb.cpu().numpy(), b)
    assert np.array_equal(ts.cpu().numpy().view(np.uint32), s.view(np.uint32))


# ------------------------------------------------------------------------------------------
# 3. plumbing
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", (-1.0, 1.0))
@pytest.mark.parametrize("name", ("float32", "int8"))
def test_threshold_extremes(name, t):
    from lshrs_amd import exact_pairs_above

    m, dim = 257, 17
    c = _case(m, dim, name, "dead")
    live = int((c["ids_h"] >= 0).sum())
    want_a, want_b, want_s = _oracle_pairs(c, t)
    stats = {}
    a, b, s = exact_pairs_above(c["stored"], t, row_ids=c["ids"], stats=stats)
    assert np.array_equal(a, want_a) and np.array_equal(b, want_b) and np.array_equal(s.view(np.uint32), want_s.view(np.uint32))
    if t == -1.0:
        assert a.shape[0] == live * (live - 1) // 2 == stats["emitted"] == stats["kept"]
    else:
        assert a.shape[0] <= 6 and np.all(s >= np.float32(1.0))         # (of the planted copies, those the rerank rounds to 1)


def test_capacity_and_max_pairs(monkeypatch):
    from lshrs_amd import _exact, exact_pairs_above

    c = _case(700, 17, "bfloat16", "none")
    one = {}
    a, b, s = exact_pairs_above(c["stored"], 0.5, stats=one)
    assert one["launches"] == 1 and one["emitted"] > 1000
    monkeypatch.setattr(_exact, "_PAIRS_FIRST_CAPACITY", 64)
    two = {}
    a2, b2, s2 = exact_pairs_above(c["stored"], 0.5, stats=two)
    assert two["launches"] == 2 and two["emitted"] == one["emitted"] and two["kept"] == one["kept"]
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(s.view(np.uint32), s2.view(np.uint32))
    for limit in (one["emitted"] - 1, 65, 10, 0):
        with pytest.raises(ValueError, match=f"{one['emitted']} pairs.*max_pairs = {limit}"):
            exact_pairs_above(c["stored"], 0.5, max_pairs=limit)
    monkeypatch.undo()
    with pytest.raises(ValueError, match=f"{one['emitted']} pairs.*max_pairs = 1000"):
        exact_pairs_above(c["stored"], 0.5, max_pairs=1000)
    exactly = {}
    a3, _, _ = exact_pairs_above(c["stored"], 0.5, max_pairs=one["emitted"], stats=exactly)
    assert np.array_equal(a3, a) and exactly["launches"] == 1


def test_zero_rows_and_bad_shapes():
    torch = _torch()
    from lshrs_amd import exact_pairs_above

    c = _case(257, 64, "float32", "none")
    zx = c["stored"].clone()
    zx[200] = 0
    with pytest.raises(ValueError, match="Cannot normalize zero vector"):
        exact_pairs_above(zx, 0.5)
    ids = torch.arange(257, device="cuda")
    ids[200] = -1                                           # (a dead zero row is nobody's business)
    a, b, _ = exact_pairs_above(zx, -1.0, row_ids=ids)
    assert a.shape[0] == 256 * 255 // 2 and 200 not in set(a.tolist()) | set(b.tolist())
    with pytest.raises(ValueError, match="row_ids"):
        exact_pairs_above(c["stored"], 0.5, row_ids=np.arange(256))
    with pytest.raises(ValueError, match="threshold"):
        exact_pairs_above(c["stored"], [0.5, 0.5])
    none = {}
    a, b, s = exact_pairs_above(c["stored"][:0], 0.5, stats=none)
    assert a.shape == b.shape == s.shape == (0,) and none["launches"] == 0 and none["rows"] == 0


@pytest.mark.parametrize("name", ("bfloat16", "float8_e4m3fn"))
def test_store_pairs_above_after_add_readd_remove_and_compact(name):
    """Superseded and erased rows stay in the block - here they are exact copies of live rows - and are in no pair; the answer,
    oriented by id, does not move when compact() moves the rows."""
    torch = _torch()
    from lshrs_amd import DeviceVectors, exact_pairs_above

    m, dim = 700, 64
    X = _rows(m, dim)
    rng = np.random.default_rng(5)
    ids = rng.permutation(np.arange(m, dtype=np.int64) * 7 + 3)
    store = DeviceVectors(dim, name)
    store.add(ids, X)
    again = np.arange(0, 60, 3)                             # twenty ids get the vector of another id: new duplicates,
    store.add(ids[again], X[again + 100])                   # and the rows they had are superseded
    gone = np.arange(300, 340)
    assert store.remove(ids[gone]) == gone.shape[0]
    assert store.stats()["dead"] == again.shape[0] + gone.shape[0]
    a, b, s = store.pairs_above(T)
    st = dict(store.last_search_stats)
    assert st["rows"] == m + again.shape[0] and st["launches"] == 1 and st["kept"] == a.shape[0]
    final = X.copy()
    final[again] = X[again + 100]
    keep = np.setdiff1d(np.arange(m), gone)
    fresh = R._stored_form(torch, name, final[keep])
    fa, fb, fs = exact_pairs_above(fresh, T, row_ids=ids[keep])
    assert np.array_equal(a, fa) and np.array_equal(b, fb) and np.array_equal(s.view(np.uint32), fs.view(np.uint32))
    pairs = set(zip(a.tolist(), b.tolist()))
    assert all((min(ids[i], ids[i + 100]), max(ids[i], ids[i + 100])) in pairs for i in again.tolist())
    assert not (set(ids[gone].tolist()) & (set(a.tolist()) | set(b.tolist())))
    store.compact()
    ca, cb, cs = store.pairs_above(T)
    assert store.last_search_stats["rows"] == m - gone.shape[0]
    assert np.array_equal(ca, a) and np.array_equal(cb, b) and np.array_equal(cs.view(np.uint32), s.view(np.uint32))
    ta, _, _ = store.pairs_above(T, return_tensors=True)
    assert ta.is_cuda and np.array_equal(ta.cpu().numpy(), a)
    with pytest.raises(ValueError, match="max_pairs"):
        store.pairs_above(T, max_pairs=0)
    assert DeviceVectors(dim, name).pairs_above(-1.0)[0].shape == (0,)


def test_lshrs_pairs_exact_above():
    torch = _torch()
    from lshrs_amd import LSHRS, InMemoryStorage

    m, dim = 700, 64
    X = _rows(m, dim)
    ids = np.arange(m, dtype=np.int64) * 11 + 1
    idx = LSHRS(dim=dim, num_perm=128, storage=InMemoryStorage(), keep_vectors="bfloat16")
    idx.index(ids, X)
    a, b, s = idx.pairs_exact_above(T, return_arrays=True)
    sa, sb, ss = idx.vectors.pairs_above(T)
    assert a.shape[0] >= 6 and np.array_equal(a, sa) and np.array_equal(b, sb) and np.array_equal(s, ss)
    assert idx.last_search_stats["rows"] == m and idx.last_search_stats["kept"] == a.shape[0]
    as_list = idx.pairs_exact_above(T)
    assert [p[0] for p in as_list] == a.tolist() and [p[1] for p in as_list] == b.tolist()
    assert np.array_equal(np.array([p[2] for p in as_list], dtype=np.float32), s)
    # without the vectors on the device: what search_exact_above raises; with an attached tensor: row i is id i
    plain = LSHRS(dim=dim, num_perm=128, storage=InMemoryStorage())
    plain.index(np.arange(m), X)
    with pytest.raises(RuntimeError, match="vector_fetch_fn must be supplied"):
        plain.pairs_exact_above(T)
    plain.set_corpus(torch.from_numpy(X).cuda().to(torch.bfloat16))
    pa, pb, ps = plain.pairs_exact_above(T, return_arrays=True)
    assert np.array_equal(pa * 11 + 1, a) and np.array_equal(pb * 11 + 1, b) and np.array_equal(ps, s)
    with pytest.raises(ValueError, match="threshold"):
        plain.pairs_exact_above(1.5)
