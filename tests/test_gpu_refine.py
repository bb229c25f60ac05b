"""The graph refinement on the GPU, the whole call (lshrs_amd.refine_knn, DeviceVectors.refine_neighbors, LSHRS.neighbors with
refine_rounds): after a round every list is exact_knn's ranking restricted to the rows within two steps, bit for bit; the exact
graph is a fixed point; a graph in which everybody is within two steps gives the exact graph; no score ever decreases; ties go
by id; what is refused; and the route through the classes."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests._knn_join_reference import desc_key, knn_join_reference
from tests._refine_reference import adjacency_of, expand_reference, restricted_reference

pytestmark = pytest.mark.gpu


def _feature():
    """The feature under test, asked for before anything is built for it: a tree without the module, or a build without the
    fourth library, fails here at once."""
    from lshrs_amd import _native, _refine

    _native.load_refine()
    return _refine


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(one, two):
    return len(one) == len(two) and all(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))
                                        for a, b in zip(one, two))


def _rows(n, dim, dtype, seed, copies=20):
    """n rows of `dtype` on the device, `copies` of them exact duplicates of other rows: ties, bit for bit."""
    import torch

    rng = np.random.default_rng(seed)
    if dtype == "int8":
        x = rng.integers(-127, 128, size=(n, dim)).astype(np.int8)
    else:
        x = rng.standard_normal((n, dim)).astype(np.float32)
    x[n - copies:] = x[rng.choice(n - copies, size=copies, replace=False)]
    x = x[rng.permutation(n)]
    return torch.from_numpy(x).cuda().to(getattr(torch, dtype))


def _random_graph(ids, k_in, seed, holes=0.1):
    """A table of ids: row i names k_in other live ids (repeats among them), some entries -1."""
    rng = np.random.default_rng(seed)
    n = len(ids)
    at = (np.arange(n)[:, None] + rng.integers(1, n, size=(n, k_in))) % n
    table = ids[at]
    table[rng.random((n, k_in)) < holes] = -1
    return table.astype(np.int64)


def _restriction(corpus, table, k, row_ids=None, max_degree=None):
    """What one round must return: exact_knn with k = n - 1, per id restricted to the ids within two steps in `table`."""
    from lshrs_amd import exact_knn

    ids, nbrs, scores = exact_knn(corpus, max(1, int(corpus.shape[0]) - 1), row_ids=row_ids)
    at = np.where(table >= 0, np.searchsorted(ids, table.clip(min=0)), -1)
    sets = expand_reference(adjacency_of(at), max_degree)
    allowed = [{int(ids[c]) for c in mine} for mine in sets]
    return (ids,) + restricted_reference(ids, nbrs, scores, allowed, k), sets


@pytest.mark.parametrize("dtype", ("float32", "bfloat16", "int8"))
def test_a_round_is_the_exact_ranking_restricted_to_two_steps(dtype):
    _feature()
    from lshrs_amd import refine_knn

    corpus = _rows(200, 32, dtype, 11)
    table = _random_graph(np.arange(200, dtype=np.int64), 3, 12)
    want, sets = _restriction(corpus, table, 5)
    stats = {}
    got = refine_knn(corpus, table, 5, stats=stats)
    assert [a.dtype for a in got] == [np.int64, np.int64, np.float32, np.int32] and got[1].shape == (200, 5)
    assert _same(got, want)
    assert stats["rounds_run"] == 1 and stats["entries"] == [sum(len(x) for x in sets)] and stats["live"] == stats["rows"] == 200
    assert stats["candidates_max"] == [max(len(x) for x in sets)] and stats["short_rows"] == sum(len(x) < 5 for x in sets)
    assert stats["torch_rows"] == [0] and stats["long_lists"] == [0] and stats["skipped_midpoints"] == [0]
    assert stats["edges"] == [sum(len(x) for x in adjacency_of(table)) // 2] and stats["changed_rows"][0] > 0
    # device tensors in, device tensors out; a cap on the midpoints
    import torch

    tensors = refine_knn(corpus, torch.from_numpy(table).cuda(), 5, return_tensors=True)
    assert all(t.is_cuda for t in tensors) and _same([t.cpu().numpy() for t in tensors], want)
    degree = sorted(len(x) for x in adjacency_of(table))
    cap = degree[len(degree) // 2]
    want, sets = _restriction(corpus, table, 5, max_degree=cap)
    got = refine_knn(corpus, table, 5, max_degree=cap, stats=stats)
    assert _same(got, want) and stats["skipped_midpoints"] == [sum(d > cap for d in degree)] and stats["skipped_midpoints"][0] > 0
    # k need not be k_in: wider than every list, and 1
    for k in (1, 150):
        assert _same(refine_knn(corpus, table, k), _restriction(corpus, table, k)[0]), k


def test_the_exact_graph_is_a_fixed_point():
    _feature()
    from lshrs_amd import exact_knn, refine_knn

    corpus = _rows(200, 32, "float32", 21)
    exact = exact_knn(corpus, 5)
    stats = {}
    got = refine_knn(corpus, exact[1], 5, rounds=3, stats=stats)
    assert _same(got[:3], exact) and np.all(got[3] == 5)
    assert stats["rounds_run"] == 1 and stats["changed_rows"] == [0] and stats["short_rows"] == 0


def test_everybody_within_two_steps_gives_the_exact_graph():
    _feature()
    from lshrs_amd import exact_knn, refine_knn

    corpus = _rows(200, 32, "bfloat16", 31)
    ids = np.arange(200, dtype=np.int64)
    table = np.zeros((200, 1), dtype=np.int64)          # every row lists row 0, which lists row 1
    table[0, 0] = 1
    for k in (5, 199, 1000):
        got = refine_knn(corpus, table, k)
        assert _same(got[:3], exact_knn(corpus, k)) and np.all(got[3] == min(k, 199)) and np.array_equal(got[0], ids)


def _keys(scores):
    return np.array([desc_key(s) for s in scores.reshape(-1)], dtype=np.int64).reshape(scores.shape)


def test_no_score_of_a_list_ever_decreases():
    _feature()
    from lshrs_amd import refine_knn

    corpus = _rows(200, 32, "float32", 41)
    table = _random_graph(np.arange(200, dtype=np.int64), 5, 42)
    stats = {}
    scored = refine_knn(corpus, table, 5, rounds=0, stats=stats)        # the input's own entries under the same rerank
    assert stats["rounds_run"] == 0 and stats["entries"] == []
    for i in range(200):
        mine = sorted(set(table[i][table[i] >= 0].tolist()))
        assert sorted(scored[1][i][:scored[3][i]].tolist()) == mine
    one = refine_knn(corpus, table, 5, rounds=1)
    two = refine_knn(corpus, table, 5, rounds=2, stats=stats)
    assert stats["rounds_run"] == 2 and len(stats["entries"]) == 2 and len(stats["changed_rows"]) == 2
    assert np.all(_keys(one[2]) <= _keys(scored[2])) and np.all(_keys(two[2]) <= _keys(one[2]))
    assert np.any(_keys(one[2]) < _keys(scored[2])) and np.any(_keys(two[2]) < _keys(one[2]))
    assert np.all(one[3] >= scored[3]) and np.all(two[3] >= one[3])
    # the second round is a round over the first one's answer
    assert _same(two, refine_knn(corpus, one[1], 5, rounds=1))


def test_a_neighbour_s_neighbour_is_found():
    _feature()
    import torch

    from lshrs_amd import refine_knn

    x = np.zeros((6, 8), dtype=np.float32)
    x[0, :2] = (1.0, 0.0)                               # a
    x[1, :2] = (1.0, 1.0)                               # b: 45 degrees off a
    x[2, :2] = (1.0, 0.1)                               # c: the true nearest of a
    x[3:, 2:5] = np.eye(3)                              # three bystanders, orthogonal to all
    table = np.array([[1], [2], [-1], [-1], [-1], [-1]], dtype=np.int64)     # a - b and b - c only
    got = refine_knn(torch.from_numpy(x).cuda(), table, 2)
    assert got[1][0].tolist() == [2, 1] and got[1][2].tolist() == [0, 1] and got[1][1].tolist() == [2, 0]
    assert got[3].tolist() == [2, 2, 2, 0, 0, 0] and np.all(got[1][3:] == -1) and np.isnan(got[2][3:]).all()
    # not through a midpoint over the cap: b has two neighbours
    capped = refine_knn(torch.from_numpy(x).cuda(), table, 2, max_degree=1)
    assert capped[1][0].tolist() == [1, -1] and capped[1][1].tolist() == [2, 0] and capped[3].tolist() == [1, 2, 1, 0, 0, 0]


def test_equal_scores_go_by_ascending_id():
    _feature()
    import torch

    from lshrs_amd import refine_knn

    rng = np.random.default_rng(51)
    x = rng.standard_normal((8, 16)).astype(np.float32)
    x[[1, 3, 4, 6]] = x[1]                              # four rows, bit for bit the same
    row_ids = np.array([500, 90, 7, 30, 2000, 11, 60, 45], dtype=np.int64)       # ids in another order than the rows
    ids = np.sort(row_ids)
    table = np.full((8, 1), 500, dtype=np.int64)        # everybody lists id 500, which lists id 7
    table[np.searchsorted(ids, 500), 0] = 7
    got = refine_knn(torch.from_numpy(x).cuda(), table, 7, row_ids=row_ids)
    assert np.array_equal(got[0], ids)
    mine = got[1][np.searchsorted(ids, 500)].tolist()
    same = [i for i in mine if i in (90, 30, 2000, 60)]
    assert same == [30, 60, 90, 2000] and mine.index(2000) - mine.index(30) == 3
    run = got[2][np.searchsorted(ids, 500)][mine.index(30):mine.index(30) + 4]
    assert len(set(run.view(np.uint32).tolist())) == 1
    # and among themselves: each of the four has the other three in front, by id
    for i in (90, 30, 2000, 60):
        assert got[1][np.searchsorted(ids, i)][:3].tolist() == sorted({90, 30, 2000, 60} - {i})


def test_sparse_ids_and_rows_without_an_id():
    _feature()
    from lshrs_amd import refine_knn

    corpus = _rows(200, 32, "bfloat16", 61)
    rng = np.random.default_rng(62)
    row_ids = ((1 << 40) + 7919 * rng.permutation(200)).astype(np.int64)
    dead = rng.choice(200, size=30, replace=False)
    removed = int(row_ids[dead[0]])
    row_ids[dead] = -1
    ids = np.sort(row_ids[row_ids >= 0])
    table = _random_graph(ids, 3, 63)
    want, _ = _restriction(corpus, table, 5, row_ids=row_ids)
    stats = {}
    got = refine_knn(corpus, table, 5, row_ids=row_ids, stats=stats)
    assert _same(got, want) and np.array_equal(got[0], ids) and stats["live"] == 170 and stats["rows"] == 200
    two = refine_knn(corpus, table, 5, row_ids=row_ids, rounds=2)
    assert _same(two, refine_knn(corpus, got[1], 5, row_ids=row_ids))
    # an id that has no row: never stored, removed (the -1 of another row is no name)
    for gone in (removed, (1 << 40) + 7919 * 200, 5, -2):
        bad = table.copy()
        bad[17, 1] = gone
        with pytest.raises(ValueError, match="has no row"):
            refine_knn(corpus, bad, 5, row_ids=row_ids)
    bad = table.copy()
    bad[17, 1] = ids[17]
    with pytest.raises(ValueError, match="lists itself"):
        refine_knn(corpus, bad, 5, row_ids=row_ids)
    for shape in (table[:-1], np.vstack((table, table[:1])), table[:, 0]):
        with pytest.raises(ValueError, match="one row per live id"):
            refine_knn(corpus, shape, 5, row_ids=row_ids)
    # nobody, and one row: nothing to refine
    assert refine_knn(corpus[:1], np.zeros((1, 3), np.int64) - 1, 5)[1].shape == (1, 0)
    assert refine_knn(corpus, np.zeros((0, 3), np.int64), 5, row_ids=np.full(200, -1))[0].shape == (0,)
    empty = refine_knn(corpus, np.full((200, 2), -1, np.int64), 5, stats=stats)
    assert np.all(empty[1] == -1) and np.all(empty[3] == 0) and stats["edges"] == [0] and stats["short_rows"] == 200


def test_more_entries_than_allowed_are_refused_before_the_rerank(monkeypatch):
    refine = _feature()
    from lshrs_amd import refine_knn

    corpus = _rows(200, 32, "float32", 71)
    table = _random_graph(np.arange(200, dtype=np.int64), 3, 72)
    stats = {}
    want = refine_knn(corpus, table, 5, stats=stats)
    entries = stats["entries"][0]
    assert _same(refine_knn(corpus, table, 5, max_entries=entries), want)

    def no_rerank(*args, **kwargs):
        raise AssertionError("the rerank was reached")

    monkeypatch.setattr(refine, "_rerank_lists", no_rerank)
    with pytest.raises(ValueError, match="max_degree") as exc:
        refine_knn(corpus, table, 5, max_entries=entries - 1)
    assert str(entries) in str(exc.value) and "max_entries" in str(exc.value)
    with pytest.raises(ValueError, match="max_degree"):
        refine_knn(corpus, table, 5, max_entries=0)


def test_a_zero_row_among_the_candidates_is_refused():
    _feature()
    from lshrs_amd import refine_knn

    corpus = _rows(50, 16, "float32", 81, copies=0)
    corpus[7] = 0
    table = _random_graph(np.arange(50, dtype=np.int64), 3, 82, holes=0.0)
    with pytest.raises(ValueError, match="Cannot normalize zero vector"):
        refine_knn(corpus, table, 5)


# ------------------------------------------------------------------------------------------
# through the classes
# ------------------------------------------------------------------------------------------
BANDS, ROWS_PER_BAND = 4, 8


def _clustered(n_centres, members, dim, sigma, seed):
    """Centres drawn from N(0, 1)^dim, each with `members` rows at centre + sigma N(0, 1)^dim: two members of one cluster have
    a cosine of about 1 / (1 + sigma^2), members of different clusters about 0."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_centres, dim)).astype(np.float32)
    x = np.repeat(centres, members, axis=0) + np.float32(sigma) * rng.standard_normal((n_centres * members, dim)).astype(np.float32)
    return x[rng.permutation(len(x))]


@functools.lru_cache(maxsize=None)
def _index():
    """600 clustered rows under scattered ids behind a 4 x 8 index, and the law's forecast for its graph - worked out on the
    CPU from the rows alone: the buckets are expected to hold SOME of the true neighbours and not all of them."""
    _feature()
    from lshrs_amd import LSHRS, InMemoryStorage
    from lshrs_amd._exact import collision_law

    x = _clustered(60, 10, 32, 0.5, 91)
    unit = x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
    cos = unit @ unit.T
    np.fill_diagonal(cos, -2.0)
    forecast = collision_law(np.sort(cos, axis=1)[:, -5:].reshape(-1), BANDS, ROWS_PER_BAND)
    assert 0.2 < forecast < 0.8, forecast
    ids = (1 << 40) + 7919 * np.random.default_rng(92).permutation(600).astype(np.int64)
    index = LSHRS(dim=32, num_perm=BANDS * ROWS_PER_BAND, num_bands=BANDS, rows_per_band=ROWS_PER_BAND, storage=InMemoryStorage(),
                  packed_ingest=True, keep_vectors="float32")
    index.index(ids, x)
    return index, forecast


def test_an_index_refines_its_own_graph():
    _feature()
    from lshrs_amd import refine_knn

    index, _ = _index()
    plain = index.neighbors(5, return_arrays=True)
    plain_stats = dict(index.last_search_stats)
    rows, row_ids = index.vectors._search_snapshot()
    stats = {}
    want = refine_knn(rows, plain[1], 5, row_ids=row_ids, stats=stats)
    got = index.neighbors(5, return_arrays=True, refine_rounds=1)
    assert _same(got, want)
    after = dict(index.last_search_stats)
    assert after.pop("refine") == stats and stats["rounds_run"] == 1
    for name in ("fold_ms", "segments_folded"):         # (the first call of the two folds the store's segments)
        after.pop(name), plain_stats.pop(name)
    assert after == plain_stats
    # the store's own method, and the lists
    assert _same(index.vectors.refine_neighbors(plain[1], 5), want) and index.vectors.last_search_stats == stats
    lists = index.neighbors(5, refine_rounds=1)
    assert [i for i, _ in lists] == got[0].tolist()
    for (_, mine), nb, sc, c in zip(lists, got[1].tolist(), got[2].astype(np.float64).tolist(), got[3].tolist()):
        assert mine == list(zip(nb[:c], sc[:c]))
    # two rounds with a cap: the function's, over the same graph
    want = refine_knn(rows, plain[1], 5, row_ids=row_ids, rounds=2, max_degree=6)
    assert _same(index.neighbors(5, return_arrays=True, refine_rounds=2, max_degree=6), want)
    assert index.last_search_stats["refine"]["skipped_midpoints"][0] > 0


def test_without_rounds_the_answer_is_the_buckets_graph():
    _feature()
    from lshrs_amd import exact_knn

    index, _ = _index()
    rows, row_ids = index.vectors._search_snapshot()
    ids, nbrs, scores = exact_knn(rows, 599, row_ids=row_ids)
    score = {}
    for a, nb, sc in zip(ids.tolist(), nbrs.tolist(), scores.tolist()):
        score.update(((a, b), np.float32(s)) for b, s in zip(nb, sc))
    want = knn_join_reference(index._storage.array_segments(1), ids, 5, lambda a, b: score[(a, b)])
    for kwargs in ({}, {"refine_rounds": 0}, {"refine_rounds": 0, "max_degree": 3}):
        got = index.neighbors(5, return_arrays=True, **kwargs)
        assert _same(got, want[:4]), kwargs
        assert "refine" not in index.last_search_stats and index.last_search_stats["short_rows"] == want[4]["short_rows"]


def test_recall_does_not_fall_with_a_round():
    _feature()
    index, forecast = _index()
    before = index.recall_neighbors(5)
    assert 0.0 < before["recall"] < 1.0 and "refine" not in index.last_search_stats
    assert abs(before["expected"] - forecast) < 0.05            # (the law over the exact scores, against the CPU's forecast)
    after = index.recall_neighbors(5, refine_rounds=1)
    assert after["recall"] >= before["recall"] and np.all(after["per_row"] >= before["per_row"])
    assert after["recall"] > before["recall"], "a round over a clustered corpus finds cluster mates the buckets missed"
    assert after["truth_entries"] == before["truth_entries"] == 3000 and after["found_entries"] >= before["found_entries"]
    assert after["short_rows"] == index.last_search_stats["refine"]["short_rows"] <= before["short_rows"]
    assert after["expected"] == before["expected"]
