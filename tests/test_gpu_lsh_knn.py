"""The LSH k-NN graph on the GPU, the whole call (lshrs_amd/_knn_join.py, LSHRS.neighbors, DeviceVectors.lsh_neighbors): equal
to exact_knn bit for bit where every pair is a candidate, equal to the plain-Python reference - exact scores restricted to the
buckets' candidates - through an index, the long-list route, what the join refuses, empty answers, the recall measure."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests._join_reference import hand_segment, join_reference
from tests._knn_join_reference import knn_join_reference

pytestmark = pytest.mark.gpu


def _feature():
    """The feature under test, asked for before anything is built for it: a tree without the module, or a build without the
    third library, fails here at once - no index, no reference and no GPU work first."""
    from lshrs_amd import _knn_join, _native

    _native.load_graph()
    return _knn_join


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(one, two):
    return len(one) == len(two) and all(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))
                                        for a, b in zip(one, two))


def _segment_on_device(seg):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda() for a in (seg.codes, seg.offsets, seg.members)]


def _rows_with_duplicates(n, dim, dtype, seed, copies=40):
    """n rows of `dtype` on the device, `copies` of them exact duplicates of other rows: ties, bit for bit."""
    import torch

    rng = np.random.default_rng(seed)
    if dtype == "int8":
        x = rng.integers(-127, 128, size=(n, dim)).astype(np.int8)
    else:
        x = rng.standard_normal((n, dim)).astype(np.float32)
    src = rng.choice(n - copies, size=copies, replace=False)
    x[n - copies:] = x[src]
    x = x[rng.permutation(n)]
    return torch.from_numpy(x).cuda().to(getattr(torch, dtype))


@pytest.mark.parametrize("dtype", ("float32", "bfloat16", "int8"))
def test_one_bucket_of_everybody_equals_the_exact_graph(dtype):
    _feature()
    import torch

    from lshrs_amd import exact_knn, lsh_knn

    n, dim = 300, 64
    corpus = _rows_with_duplicates(n, dim, dtype, 51)
    dev = _segment_on_device(hand_segment({0x07: list(range(n))}))
    want = exact_knn(corpus, 10)
    stats = {}
    got = lsh_knn(corpus, 10, *dev, 1, 1, stats=stats)
    assert [a.dtype for a in got] == [np.int64, np.int64, np.float32, np.int32]
    assert _same(got[:3], want) and np.all(got[3] == 10)
    ties = sum(len(set(row.tolist())) < 10 for row in got[2].view(np.uint32))
    assert ties > 40, "duplicates must put equal scores into the lists"
    assert stats["emitted"] == n * (n - 1) // 2 == stats["raw_pairs"] and stats["candidates_max"] == n - 1
    assert stats["short_rows"] == 0 and stats["long_lists"] == 0 and stats["live"] == stats["rows"] == n
    # ids in another order than the rows, and rows that no id points at: members of no bucket
    rng = np.random.default_rng(52)
    row_ids = (1 << 40) + 1 + 104729 * rng.permutation(n).astype(np.int64)
    row_ids[rng.choice(n, size=23, replace=False)] = -1
    live = np.flatnonzero(row_ids >= 0).astype(np.int64)
    dev = _segment_on_device(hand_segment({0x07: live[rng.permutation(live.shape[0])].tolist()}))
    want = exact_knn(corpus, 10, row_ids=row_ids)
    got = lsh_knn(corpus, 10, *dev, 1, 1, row_ids=row_ids, stats=stats)
    assert _same(got[:3], want) and np.all(got[3] == 10) and got[0].shape == (n - 23,) and stats["live"] == n - 23
    tensors = lsh_knn(corpus, 10, *dev, 1, 1, row_ids=row_ids, return_tensors=True)
    assert len(tensors) == 4 and all(isinstance(x, torch.Tensor) and x.device == corpus.device for x in tensors)
    assert [x.dtype for x in tensors] == [torch.int64, torch.int64, torch.float32, torch.int32]
    assert _same([x.cpu().numpy() for x in tensors], got)
    # k beyond the rows: the width exact_knn returns
    wide = lsh_knn(corpus, 1000, *dev, 1, 1, row_ids=row_ids)
    assert _same(wide[:3], exact_knn(corpus, 1000, row_ids=row_ids)) and wide[1].shape == (n - 23, n - 24)


def _skewed(n, dim, seed, bulk_from=100, shift=8.0, copies=30):
    """n float32 rows: the first `bulk_from` are plain noise, the others noise around one direction - their sign bits agree
    often, so they crowd into few buckets and the plain rows find few bucket mates; `copies` exact duplicates for ties."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    mu = rng.standard_normal(dim).astype(np.float32)
    x[bulk_from:] += np.float32(shift) * mu / np.linalg.norm(mu)
    x[n - copies:] = x[rng.choice(np.arange(bulk_from, n - copies), size=copies, replace=False)]
    return x


@functools.lru_cache(maxsize=None)
def _index(dtype):
    """2 000 skewed rows under scattered ids, 4 bands of 8 rows, indexed in two calls (two segments, folded by the call):
    (index, all exact scores (n, n) float32 with [i, j] = id i asking id j in ascending order of id, the sorted ids)."""
    _feature()
    import torch

    from lshrs_amd import LSHRS, InMemoryStorage, exact_top_k

    n, dim = 2000, 64
    x = _skewed(n, dim, 61)
    ids = (1 << 40) + 7919 * np.random.default_rng(62).permutation(n).astype(np.int64)
    index = LSHRS(dim=dim, num_perm=32, num_bands=4, rows_per_band=8, storage=InMemoryStorage(), packed_ingest=True,
                  keep_vectors=dtype)
    index.index(ids[:1200], x[:1200])
    index.index(ids[1200:], x[1200:])
    rows, row_ids = index.vectors._search_snapshot()
    live = torch.nonzero(row_ids >= 0).reshape(-1)
    order = live[torch.argsort(row_ids[live])]
    sorted_ids = row_ids[order].cpu().numpy()
    # the reference's scores: every stored row, as float32, asking every stored row
    t_ids, t_scores = exact_top_k(rows[order].float(), rows, n, row_ids=row_ids)
    by_id = np.argsort(t_ids, axis=1, kind="stable")
    table = np.take_along_axis(t_scores, by_id, axis=1)
    assert np.array_equal(np.take_along_axis(t_ids, by_id, axis=1)[0], sorted_ids)
    table.setflags(write=False)
    return index, table, sorted_ids


def _reference(index, table, sorted_ids, k, **kwargs):
    rank = {int(i): r for r, i in enumerate(sorted_ids.tolist())}
    return knn_join_reference(index._storage.array_segments(1), sorted_ids, k, lambda a, b: table[rank[a], rank[b]], **kwargs)


@pytest.mark.parametrize("dtype", ("float32", "bfloat16"))
def test_an_index_answers_the_exact_ranking_restricted_to_its_candidates(dtype):
    _feature()
    index, table, sorted_ids = _index(dtype)
    index._one_join = None
    want = _reference(index, table, sorted_ids, 5)
    got = index.neighbors(5, return_arrays=True)
    stats = dict(index.last_search_stats)
    assert [a.dtype for a in got] == [np.int64, np.int64, np.float32, np.int32] and got[1].shape == (2000, 5)
    assert _same(got, want[:4])
    assert stats["short_rows"] == want[4]["short_rows"] > 0, "some rows must have fewer than 5 candidates: the padding"
    assert stats["candidates_max"] == want[4]["candidates_max"] and stats["emitted"] == want[4]["emitted"]
    assert stats["raw_pairs"] == want[4]["raw_pairs"] and stats["buckets"] == want[4]["buckets"]
    assert stats["segments_folded"] == 2 and stats["live"] == 2000 and stats["long_lists"] == 0 and stats["launches"] >= 1
    padded = got[3] < 5
    assert np.all(got[1][padded, -1] == -1) and np.all(np.isnan(got[2][padded, -1])) and not np.isnan(got[2][~padded]).any()
    # the lists, without the padding
    lists = index.neighbors(5)
    assert index.last_search_stats["segments_folded"] == 0
    assert [i for i, _ in lists] == got[0].tolist()
    for (_, mine), nb, sc, c in zip(lists, got[1].tolist(), got[2].astype(np.float64).tolist(), got[3].tolist()):
        assert mine == list(zip(nb[:c], sc[:c]))
    # two collisions and more; a limit on the buckets
    for kwargs in ({"min_collisions": 2}, {"max_bucket": 8}):
        want = _reference(index, table, sorted_ids, 5, **kwargs)
        got = index.neighbors(5, return_arrays=True, **kwargs)
        assert _same(got, want[:4]), kwargs
        assert index.last_search_stats["emitted"] == want[4]["emitted"] > 0
        assert index.last_search_stats["skipped_buckets"] == want[4]["skipped_buckets"]
    assert index.last_search_stats["skipped_buckets"] > 0


@pytest.mark.parametrize("dtype", ("float32", "bfloat16"))
def test_recall_neighbors_is_what_the_two_answers_say(dtype):
    _feature()
    from lshrs_amd._exact import collision_law

    index, _, _ = _index(dtype)
    t_ids, t_nbrs, t_scores = index.neighbors_exact(10, return_arrays=True)
    ids, nbrs, _, counts = index.neighbors(10, return_arrays=True)
    assert np.array_equal(t_ids, ids)
    per = np.array([len(set(t.tolist()) & set(f[:c].tolist())) / 10 for t, f, c in zip(t_nbrs, nbrs, counts)], dtype=np.float32)
    found = sum(len(set(t.tolist()) & set(f[:c].tolist())) for t, f, c in zip(t_nbrs, nbrs, counts))
    rec = index.recall_neighbors(10)
    assert rec["truth_entries"] == 20000 and rec["found_entries"] == int(counts.sum())
    assert rec["recall"] == found / 20000 and 0.0 < rec["recall"] < 1.0
    assert rec["per_row"].dtype == np.float32 and np.array_equal(rec["per_row"], per)
    assert rec["short_rows"] == index.last_search_stats["short_rows"] == int((counts < 10).sum())
    assert rec["expected"] == collision_law(t_scores.reshape(-1), 4, 8)


def test_recall_is_one_where_everybody_shares_every_bucket():
    _feature()
    from lshrs_amd import LSHRS, InMemoryStorage

    rng = np.random.default_rng(71)
    v = rng.standard_normal(64).astype(np.float32)
    x = v[None, :] * (2.0 ** rng.integers(-3, 4, size=(50, 1))).astype(np.float32)        # one direction: one signature
    index = LSHRS(dim=64, num_perm=32, num_bands=4, rows_per_band=8, storage=InMemoryStorage(), packed_ingest=True,
                  keep_vectors="float32")
    index.index(np.arange(50, dtype=np.int64) * 5 + 3, x)
    rec = index.recall_neighbors(7)
    assert rec["recall"] == 1.0 and rec["truth_entries"] == rec["found_entries"] == 350 and rec["short_rows"] == 0
    assert np.all(rec["per_row"] == 1.0) and index.last_search_stats["candidates_max"] == 49
    exact = index.neighbors_exact(7, return_arrays=True)
    assert _same(index.neighbors(7, return_arrays=True)[:3], exact)


def test_lists_beyond_the_kernel_are_ranked_by_the_sorts(monkeypatch):
    _feature()
    import torch

    from lshrs_amd import _knn_join, exact_knn, lsh_knn

    n = _knn_join.graph_max_list() + 2
    corpus = torch.randn(n, 8, device="cuda", generator=torch.Generator("cuda").manual_seed(81))
    corpus[n - 200:] = corpus[:200]                                     # ties
    dev = _segment_on_device(hand_segment({0x05: list(range(n))}))
    calls = []
    inner = _knn_join._rank_long

    def spy(torch_, nbr, scores, row_off, row_ids, k, rows, *outs):
        calls.append(int(rows.shape[0]))
        return inner(torch_, nbr, scores, row_off, row_ids, k, rows, *outs)

    monkeypatch.setattr(_knn_join, "_rank_long", spy)
    stats = {}
    got = lsh_knn(corpus, 10, *dev, 1, 1, stats=stats)
    assert calls == [n] and stats["long_lists"] == n and stats["candidates_max"] == n - 1 and stats["launches"] == 2
    assert _same(got[:3], exact_knn(corpus, 10)) and np.all(got[3] == 10)


def test_what_the_join_refuses_is_refused_with_its_messages():
    _feature()
    import torch

    from lshrs_amd import _join, lsh_knn
    from lshrs_amd.vectors import NO_VECTOR_MSG

    corpus = torch.randn(12, 32, device="cuda", generator=torch.Generator("cuda").manual_seed(91))
    good = hand_segment({0x001: [0, 1, 2, 3], 0x002: [4, 5], 0x101: [0, 1], 0x102: [2, 4, 5]})
    pairs, ref = join_reference([good])
    assert lsh_knn(corpus, 3, *_segment_on_device(good), 2, 1)[3].tolist() == [3, 3, 3, 3, 2, 2, 0, 0, 0, 0, 0, 0]
    # a member without a row
    with pytest.raises(IndexError, match=NO_VECTOR_MSG):
        lsh_knn(corpus, 3, *_segment_on_device(hand_segment({0x001: [0, 1, -1, 3], 0x002: [4, 5]})), 2, 1)
    with pytest.raises(IndexError, match=_join.OUT_OF_RANGE_MSG):
        lsh_knn(corpus, 3, *_segment_on_device(hand_segment({0x001: [0, 1, 12, 3]})), 2, 1)
    # a row in two buckets of one band
    with pytest.raises(ValueError, match="two signatures"):
        lsh_knn(corpus, 3, *_segment_on_device(hand_segment({0x001: [0, 1, 2], 0x002: [2, 5]})), 2, 1)
    # the two limits
    with pytest.raises(ValueError, match=f"{ref['raw_pairs']} raw pairs, more than max_raw_pairs = {ref['raw_pairs'] - 1}"):
        lsh_knn(corpus, 3, *_segment_on_device(good), 2, 1, max_raw_pairs=ref["raw_pairs"] - 1)
    with pytest.raises(ValueError, match=f"more than max_pairs = {len(pairs) - 1}"):
        lsh_knn(corpus, 3, *_segment_on_device(good), 2, 1, max_pairs=len(pairs) - 1)
    assert lsh_knn(corpus, 3, *_segment_on_device(good), 2, 1, max_pairs=len(pairs), max_raw_pairs=ref["raw_pairs"])[3].sum() == 16
    # a candidate of zero norm
    corpus[4] = 0.0
    with pytest.raises(ValueError, match="Cannot normalize zero vector"):
        lsh_knn(corpus, 3, *_segment_on_device(good), 2, 1)
    # ... which is nobody's business while it is in no counted bucket
    assert lsh_knn(corpus, 3, *_segment_on_device(hand_segment({0x001: [0, 1, 2, 3], 0x002: [4]})), 2, 1)[3].sum() == 12


def test_empty_answers():
    _feature()
    import torch

    from lshrs_amd import LSHRS, InMemoryStorage, lsh_knn

    def check(got, n, kk):
        assert [a.dtype for a in got] == [np.int64, np.int64, np.float32, np.int32]
        assert [a.shape for a in got] == [(n,), (n, kk), (n, kk), (n,)]
        assert np.all(got[1] == -1) and np.isnan(got[2]).all() and not got[3].any()

    # a segment without buckets: every row, with no neighbour
    stats = {}
    got = lsh_knn(torch.ones(4, 64, device="cuda"), 2, [], [0], [], 8, 1, stats=stats)
    check(got, 4, 2)
    assert got[0].tolist() == [0, 1, 2, 3] and stats["short_rows"] == 4 and stats["emitted"] == 0
    check(lsh_knn(torch.ones(1, 64, device="cuda"), 2, [], [0], [], 8, 1), 1, 0)
    check(lsh_knn(torch.ones(0, 64, device="cuda"), 2, [], [0], [], 8, 1), 0, 0)
    check(lsh_knn(torch.ones(3, 64, device="cuda"), 2, [], [0], [], 8, 1, row_ids=[-1, -1, -1]), 0, 0)
    # buckets of one member each
    check(lsh_knn(torch.ones(4, 64, device="cuda"), 2, *_segment_on_device(hand_segment({1: [0], 2: [3]})), 8, 1), 4, 2)
    empty = LSHRS(dim=64, num_perm=64, num_bands=8, rows_per_band=8, storage=InMemoryStorage(), packed_ingest=True,
                  keep_vectors="float32")
    check(empty.neighbors(5, return_arrays=True), 0, 0)
    assert empty.neighbors(5) == [] and empty.last_search_stats["emitted"] == 0
    rec = empty.recall_neighbors(5)
    assert rec["recall"] == 1.0 and rec["truth_entries"] == 0 and rec["per_row"].shape == (0,)


@pytest.mark.parametrize("dtype", ("bfloat16", "int8"))
def test_the_store_route_after_remove_and_compact(dtype):
    _feature()
    import torch

    from lshrs_amd import DeviceVectors
    from lshrs_amd.packed_ops import _csr_host

    n, dim, nb = 600, 48, 6
    rng = np.random.default_rng(101)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    ids = (1 << 40) + 1 + 104729 * rng.permutation(n).astype(np.int64)
    gone = rng.choice(n, size=80, replace=False)
    keep = np.setdiff1d(np.arange(n), gone)
    keys = rng.integers(0, 8, size=(n, nb, 1)).astype(np.uint8)
    seg = _segment_on_device(_csr_host(ids[keep], keys[keep]))
    store = DeviceVectors(dim, dtype)
    store.add(ids, x)
    store.remove(ids[gone].tolist())
    one = store.lsh_neighbors(10, *seg, nb, 1)
    stats = dict(store.last_search_stats)
    assert stats["live"] == n - 80 and stats["rows"] == n and stats["short_rows"] == 0 and one[1].shape == (n - 80, 10)
    store.compact()
    two = store.lsh_neighbors(10, *seg, nb, 1)
    assert store.last_search_stats["rows"] == n - 80
    fresh = DeviceVectors(dim, dtype)
    fresh.add(ids[keep][::-1].copy(), x[keep][::-1].copy())
    three = fresh.lsh_neighbors(10, *seg, nb, 1)
    emitted = fresh.last_search_stats["emitted"]
    assert _same(one, three) and _same(two, three) and np.array_equal(one[0], np.sort(ids[keep]))
    tensors = fresh.lsh_neighbors(10, *seg, nb, 1, return_tensors=True, min_collisions=2)
    assert all(isinstance(t, torch.Tensor) for t in tensors) and 0 < fresh.last_search_stats["emitted"] < emitted == stats["emitted"]
