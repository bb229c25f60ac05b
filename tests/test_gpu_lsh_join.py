"""The LSH self-join on the GPU (csrc/join.hip, lshrs_amd/_join.py, LSHRS.pairs_above): the two kernels against a plain-Python
join over hand-made bucket segments (packed_ops._csr_host over small key spaces - no signature pass), then the whole call
through LSHRS against pairs_exact_above restricted to the reference's candidate pairs, bit for bit."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests._join_reference import buckets_reference, join_reference

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (3, 1), (16, 2), (33, 1), (128, 1), (8, 6), (16, 4), (2, 1), (6, 2), (10, 1))
PLANTED = (300, 129, 65, 64, 63, 3, 2, 1)          # bucket lengths of band 0, among many small ones


def _keys_of(vals, bb):
    """(n, nb) key numbers below 256 as (n, nb, bb) key bytes that use the highest byte, too."""
    vals = vals * ((1 << (8 * (bb - 1))) + 1) if bb > 1 else vals
    keys = np.zeros(vals.shape + (bb,), dtype=np.uint8)
    for j in range(bb):
        keys[:, :, j] = (vals >> (8 * j)) & 0xFF
    return keys


@functools.lru_cache(maxsize=None)
def _segment(nb, bb):
    """One segment of 830 members over `n_rows` = 837 rows (the id is the row): band 0 holds buckets of the PLANTED lengths and
    203 members spread over 240 keys; the other bands spread everybody over 200 keys; the last two members share every key."""
    from lshrs_amd.packed_ops import _csr_host

    rng = np.random.default_rng(1000 * nb + bb)
    n = sum(PLANTED) + 203
    vals = rng.integers(0, 200, size=(n, nb))
    vals[:, 0] = np.r_[np.repeat(np.arange(len(PLANTED)), PLANTED), rng.integers(len(PLANTED), 248, size=203)]
    vals[-1] = vals[-2]
    vals = vals[rng.permutation(n)]
    ids = rng.choice(n + 7, size=n, replace=False).astype(np.int64)
    seg = _csr_host(ids, _keys_of(vals, bb))
    return seg, n + 7


def _run(seg, n_rows, nb, bb, **kwargs):
    """lsh_pairs over the segment with room for everything: ({(a, b): collisions}, raw_pairs); asserts that no pair comes out
    twice and that the count is the number of pairs."""
    import torch

    from lshrs_amd import _join

    codes, offsets, members = (torch.from_numpy(a).cuda() for a in (seg.codes, seg.offsets, seg.members))
    (a, b, hits, total, err), raw = _join.lsh_pairs(codes, offsets, members, n_rows, nb, bb, capacity=1 << 19, **kwargs)
    n = int(total.item())
    assert n <= 1 << 19 and int(err.item()) == 0
    a, b, hits = a[:n].cpu().numpy(), b[:n].cpu().numpy(), hits[:n].cpu().numpy()
    assert np.all(a < b)
    got = dict(zip(zip(a.tolist(), b.tolist()), hits.tolist()))
    assert len(got) == n, "a pair came out twice"
    return got, raw


@pytest.mark.parametrize("nb, bb", SHAPES)
def test_the_kernels_equal_the_plain_join(nb, bb):
    seg, n_rows = _segment(nb, bb)
    lens = set(np.diff(seg.offsets)[seg.bands == 0].tolist())
    assert set(PLANTED) <= lens and max(lens) == 300
    want, stats = join_reference([seg])
    got, raw = _run(seg, n_rows, nb, bb)
    assert got == want and raw == stats["raw_pairs"]
    assert max(want.values()) == nb                     # (the two members that share every key)
    if nb > 1:
        assert sum(1 for c in want.values() if c > 1) > 1


def test_a_raw_range_split_across_launches(monkeypatch):
    from lshrs_amd import _join

    seg, n_rows = _segment(3, 1)
    whole, raw = _run(seg, n_rows, 3, 1)
    # slices of 1000 raw pairs: the bucket of 300 members alone holds 44 850, so boundaries fall inside buckets
    monkeypatch.setattr(_join, "_EMIT_SLICE", 1000)
    assert raw > 44850 and raw % 1000 != 0
    split, raw2 = _run(seg, n_rows, 3, 1)
    assert split == whole == join_reference([seg])[0] and raw2 == raw
    monkeypatch.setattr(_join, "_EMIT_SLICE", 44851)
    assert _run(seg, n_rows, 3, 1)[0] == whole


def test_max_bucket_counts_in_no_role():
    import torch

    from lshrs_amd import lsh_pairs_above
    from lshrs_amd.packed_ops import _csr_host

    # band 0: rows 0..9 in one bucket; band 1: rows 0, 1 in one bucket, everybody else alone; band 2: rows 2..9 in one bucket
    vals = np.zeros((12, 3), dtype=np.int64)
    vals[:, 0] = np.r_[np.full(10, 1), 2, 3]
    vals[:, 1] = np.r_[5, 5, 10 + np.arange(10)]
    vals[:, 2] = np.r_[20, 21, np.full(8, 7), 22, 23]
    seg = _csr_host(np.arange(12, dtype=np.int64), _keys_of(vals, 1))
    corpus = torch.randn(12, 32, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    dev = [torch.from_numpy(a).cuda() for a in (seg.codes, seg.offsets, seg.members)]
    for max_bucket, skipped in ((None, 0), (10, 0), (9, 1), (5, 2), (2, 2)):
        want, ref_stats = join_reference([seg], max_bucket=max_bucket)
        stats = {}
        ia, ib, _, coll = lsh_pairs_above(corpus, -1.0, *dev, 3, 1, max_bucket=max_bucket, stats=stats)
        assert dict(zip(zip(ia.tolist(), ib.tolist()), coll.tolist())) == want, max_bucket
        assert stats["skipped_buckets"] == skipped == ref_stats["skipped_buckets"]
        assert stats["raw_pairs"] == ref_stats["raw_pairs"] and stats["emitted"] == stats["kept"] == len(want)
        assert stats["buckets"] == ref_stats["buckets"]
    # at 5: the pair (0, 1) shares the oversized bucket of band 0 and the small one of band 1 - it is emitted, with the
    # oversized bucket not counted; (2, 3) shares only oversized buckets - it is not
    assert join_reference([seg])[0][(0, 1)] == 2 and join_reference([seg])[0][(2, 3)] == 2
    assert join_reference([seg], max_bucket=5)[0] == {(0, 1): 1}


@pytest.mark.parametrize("nb, bb", ((16, 2), (3, 1), (6, 2)))
def test_min_collisions_against_the_reference(nb, bb):
    seg, n_rows = _segment(nb, bb)
    for need in (2, nb):
        want = join_reference([seg], min_collisions=need)[0]
        assert _run(seg, n_rows, nb, bb, min_collisions=need)[0] == want
        assert len(want) >= 1


def test_capacity_max_pairs_and_max_raw_pairs(monkeypatch):
    import torch

    from lshrs_amd import _join, lsh_pairs_above

    seg, n_rows = _segment(3, 1)
    corpus = torch.randn(n_rows, 32, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    dev = [torch.from_numpy(a).cuda() for a in (seg.codes, seg.offsets, seg.members)]
    want, ref_stats = join_reference([seg])
    first, second = {}, {}
    one = lsh_pairs_above(corpus, -1.0, *dev, 3, 1, stats=first)
    monkeypatch.setattr(_join, "_JOIN_FIRST_CAPACITY", 64)
    two = lsh_pairs_above(corpus, -1.0, *dev, 3, 1, stats=second)
    assert first["launches"] == 1 and second["launches"] == 2 and first["emitted"] == second["emitted"] == len(want)
    for x, y in zip(one, two):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    assert dict(zip(zip(one[0].tolist(), one[1].tolist()), one[3].tolist())) == want
    assert np.all(np.diff(one[2]) <= 0)
    with pytest.raises(ValueError, match="max_pairs"):
        lsh_pairs_above(corpus, -1.0, *dev, 3, 1, max_pairs=len(want) - 1)
    assert len(lsh_pairs_above(corpus, -1.0, *dev, 3, 1, max_pairs=len(want))[0]) == len(want)
    with pytest.raises(ValueError, match="max_bucket"):
        lsh_pairs_above(corpus, -1.0, *dev, 3, 1, max_raw_pairs=ref_stats["raw_pairs"] - 1)
    assert len(lsh_pairs_above(corpus, -1.0, *dev, 3, 1, max_raw_pairs=ref_stats["raw_pairs"])[0]) == len(want)


def test_two_signatures_are_refused_and_an_id_twice_in_a_bucket_counts_once():
    from lshrs_amd.packed_ops import _csr_host, merge_csr

    nb = 3
    # id 5 under keys 1 (with 6) and then under keys 2 (with 7): in two buckets of every band
    one = _csr_host(np.array([5, 6], dtype=np.int64), _keys_of(np.full((2, nb), 1), 1))
    two = _csr_host(np.array([5, 7], dtype=np.int64), _keys_of(np.full((2, nb), 2), 1))
    with pytest.raises(ValueError, match="two signatures"):
        _run(merge_csr([one, two]), 8, nb, 1)
    # ... the same where only ONE band differs
    vals = np.full((2, nb), 1)
    vals[:, 2] = 9
    with pytest.raises(ValueError, match="two signatures"):
        _run(merge_csr([one, _csr_host(np.array([5, 7], dtype=np.int64), _keys_of(vals, 1))]), 8, nb, 1)
    # the same id under the same keys through two segments: once in its bucket
    again = _csr_host(np.array([6, 3], dtype=np.int64), _keys_of(np.full((2, nb), 1), 1))
    folded = merge_csr([one, again])
    assert np.diff(folded.offsets).tolist() == [3] * nb
    got, raw = _run(folded, 8, nb, 1)
    assert got == {(3, 5): nb, (3, 6): nb, (5, 6): nb} == join_reference([one, again])[0] and raw == 3 * nb


def _planted(n, dim, seed, copies=200):
    """n float32 rows: `copies` of them with two noisy copies each, cosines between about 0.62 and 0.95."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    src = rng.choice(n // 2, size=copies, replace=False)
    assert n // 2 + 2 * copies <= n
    for k in range(2):
        sigma = rng.uniform(0.3, 1.25, size=(copies, 1)).astype(np.float32)
        x[n // 2 + copies * k + np.arange(copies)] = x[src] * rng.uniform(0.5, 2.0, size=(copies, 1)).astype(np.float32) \
            + sigma * rng.standard_normal((copies, dim)).astype(np.float32)
    return x


def _filtered(exact, cand):
    ea, eb, es = exact
    keep = np.array([(a, b) in cand for a, b in zip(ea.tolist(), eb.tolist())], dtype=bool)
    return ea[keep], eb[keep], es[keep], keep


def _check_whole_call(index, t):
    """pairs_above(t) == pairs_exact_above(t) restricted to the reference's candidates; returns (answer, exact, stats)."""
    cand, ref_stats = join_reference(index._storage.array_segments(1))
    got = index.pairs_above(t, return_arrays=True)
    stats = dict(index.last_search_stats)
    exact = index.pairs_exact_above(t, return_arrays=True)
    ea, eb, es, keep = _filtered(exact, cand)
    assert keep.any() and not keep.all(), "the candidates must hit some of the truth and miss some"
    assert np.array_equal(got[0], ea) and np.array_equal(got[1], eb)
    assert got[2].dtype == np.float32 and np.array_equal(got[2].view(np.uint32), es.view(np.uint32))
    assert got[3].dtype == np.int32 and got[3].tolist() == [cand[p] for p in zip(ea.tolist(), eb.tolist())]
    assert stats["emitted"] == len(cand) and stats["kept"] == len(ea) and stats["raw_pairs"] == ref_stats["raw_pairs"]
    assert stats["buckets"] == ref_stats["buckets"] and stats["skipped_buckets"] == 0 and stats["launches"] >= 1
    return got, exact, stats


@pytest.mark.parametrize("dtype", ("float32", "bfloat16", "int8"))
def test_the_whole_call_from_the_index_own_vectors(dtype):
    from lshrs_amd import LSHRS, InMemoryStorage
    from lshrs_amd._exact import collision_law

    n, dim, t = 2000, 64, 0.6
    x = _planted(n, dim, 11)
    ids = (1 << 40) + 7919 * np.random.default_rng(4).permutation(n).astype(np.int64)
    index = LSHRS(dim=dim, num_perm=64, num_bands=8, rows_per_band=8, storage=InMemoryStorage(), packed_ingest=True,
                  keep_vectors=dtype)
    for lo in range(0, n, 500):
        index.index(ids[lo:lo + 500], x[lo:lo + 500])
    index.delete([int(i) for i in ids[[3, 1000, 1001, 1450, 1999]]])
    got, exact, stats = _check_whole_call(index, t)
    assert stats["segments_folded"] == 4 and stats["fold_ms"] > 0.0
    # a second call folds nothing and answers the same
    again = index.pairs_above(t, return_arrays=True)
    assert index.last_search_stats["segments_folded"] == 0 and index.last_search_stats["fold_ms"] == 0.0
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    assert index.pairs_above(t) == list(zip(got[0].tolist(), got[1].tolist(), got[2].astype(np.float64).tolist(), got[3].tolist()))
    # the measurement that goes with it: the counts of those two answers
    rec = index.recall_pairs_above(t)
    assert rec["truth_pairs"] == len(exact[0]) and rec["kept"] == len(got[0]) and rec["candidates"] == stats["emitted"]
    assert rec["recall"] == len(got[0]) / len(exact[0]) and rec["precision"] == len(got[0]) / stats["emitted"]
    assert rec["expected"] == collision_law(exact[2], 8, 8) and 0.0 < rec["recall"] < 1.0
    # min_collisions = 2: the reference's pairs of two bands and more
    cand2 = join_reference(index._storage.array_segments(1), min_collisions=2)[0]
    ea, eb, es, keep = _filtered(exact, cand2)
    two = index.pairs_above(t, min_collisions=2, return_arrays=True)
    assert np.array_equal(two[0], ea) and np.array_equal(two[1], eb) and np.array_equal(two[2].view(np.uint32), es.view(np.uint32))
    assert index.last_search_stats["emitted"] == len(cand2) and keep.any()


def test_what_the_join_refuses_and_the_empty_index():
    import torch

    from lshrs_amd import LSHRS, InMemoryStorage, lsh_pairs_above
    from lshrs_amd.vectors import NO_VECTOR_MSG

    # a segment without buckets
    none = lsh_pairs_above(torch.ones(4, 64, device="cuda"), 0.5, [], [0], [], 8, 1)
    assert [a.dtype for a in none] == [np.int64, np.int64, np.float32, np.int32] and all(a.shape == (0,) for a in none)
    # offsets that do not end where the member list does: refused before anything is launched
    with pytest.raises(ValueError, match="offsets must run"):
        lsh_pairs_above(torch.ones(4, 64, device="cuda"), 0.5, [1], [0, 3], [0, 1], 8, 1)
    x = _planted(1000, 64, 13)
    ids = np.arange(1000, dtype=np.int64) * 3 + (1 << 33)
    empty = LSHRS(dim=64, num_perm=64, num_bands=8, rows_per_band=8, storage=InMemoryStorage(), packed_ingest=True,
                  keep_vectors="float32")
    got = empty.pairs_above(0.5, return_arrays=True)
    assert [a.dtype for a in got] == [np.int64, np.int64, np.float32, np.int32] and all(a.shape == (0,) for a in got)
    assert empty.pairs_above(0.5) == [] and empty.last_search_stats["emitted"] == 0
    assert empty.recall_pairs_above(0.5)["recall"] == 1.0
    empty.index(ids, x)
    assert len(empty.pairs_above(0.6)) > 0
    # an id in the buckets whose vector is gone
    empty.vectors.remove([int(ids[7])])
    with pytest.raises(IndexError, match=NO_VECTOR_MSG):
        empty.pairs_above(0.6)
    # buckets kept as op tuples: no arrays to join on, and no host fallback
    tuples = LSHRS(dim=64, num_perm=64, num_bands=8, rows_per_band=8, storage=InMemoryStorage(), packed_ingest=False,
                   keep_vectors="float32")
    tuples.index(ids, x)
    with pytest.raises(RuntimeError, match="array"):
        tuples.pairs_above(0.6)


@pytest.mark.parametrize("dtype", ("float32", "bfloat16"))
def test_row_ids_in_another_order_than_the_rows_and_device_tensors_back(dtype):
    """lsh_pairs_above(row_ids=...): the emit delivers ROW pairs with the lower row first, the answer is oriented by ID."""
    import torch

    from lshrs_amd import exact_pairs_above, lsh_pairs_above
    from lshrs_amd.packed_ops import _csr_host

    n, dim, t, nb = 600, 48, 0.6, 6
    corpus = torch.from_numpy(_planted(n, dim, 21, copies=100)).cuda().to(getattr(torch, dtype))
    rng = np.random.default_rng(22)
    row_ids = (1 << 40) + 1 + 104729 * rng.permutation(n).astype(np.int64)
    row_ids[rng.choice(n, size=37, replace=False)] = -1            # rows no id points at: members of no bucket
    live = np.flatnonzero(row_ids >= 0).astype(np.int64)
    assert live.shape[0] == n - 37 and row_ids[live].min() > 1 << 40
    seg = _csr_host(live, rng.integers(0, 8, size=(live.shape[0], nb, 1)).astype(np.uint8))
    rows, ref_stats = join_reference([seg])
    turned = np.mean([row_ids[a] > row_ids[b] for a, b in rows])
    assert 0.4 < turned < 0.6, "about half of the row pairs have the higher id at the lower row"
    cand = {(int(min(row_ids[a], row_ids[b])), int(max(row_ids[a], row_ids[b]))): c for (a, b), c in rows.items()}
    assert len(cand) == len(rows)
    ea, eb, es, keep = _filtered(exact_pairs_above(corpus, t, row_ids=row_ids), cand)
    assert keep.any() and not keep.all(), "the candidates must hit some of the truth and miss some"
    dev = [torch.from_numpy(a).cuda() for a in (seg.codes, seg.offsets, seg.members)]
    stats = {}
    got = lsh_pairs_above(corpus, t, *dev, nb, 1, row_ids=row_ids, stats=stats)
    assert [a.dtype for a in got] == [np.int64, np.int64, np.float32, np.int32]
    assert np.array_equal(got[0], ea) and np.array_equal(got[1], eb) and np.all(got[0] < got[1])
    assert np.array_equal(got[2].view(np.uint32), es.view(np.uint32))
    assert got[3].tolist() == [cand[p] for p in zip(ea.tolist(), eb.tolist())] and max(got[3]) > 1
    assert stats["emitted"] == len(cand) and stats["kept"] == len(ea) and stats["raw_pairs"] == ref_stats["raw_pairs"]
    assert stats["buckets"] == ref_stats["buckets"] and stats["skipped_buckets"] == 0
    tensors = lsh_pairs_above(corpus, t, *dev, nb, 1, row_ids=row_ids, return_tensors=True)
    assert len(tensors) == 4 and all(isinstance(x, torch.Tensor) and x.device == corpus.device for x in tensors)
    assert [x.dtype for x in tensors] == [torch.int64, torch.int64, torch.float32, torch.int32]
    for x, y in zip(tensors, got):
        assert np.array_equal(x.cpu().numpy().view(np.uint32), y.view(np.uint32))


def _near_copy(v, rng, eps=0.045):
    """v and a little noise: a cosine of about 1 / sqrt(1 + eps^2) = 0.999 with v."""
    noise = rng.standard_normal(v.shape).astype(np.float32)
    return (v + eps * np.linalg.norm(v) / np.linalg.norm(noise) * noise).astype(np.float32)


def _store_index(dtype):
    """1500 planted rows indexed in three calls under scattered ids, the vectors kept by the index: (index, x, ids, rng)."""
    from lshrs_amd import LSHRS, InMemoryStorage

    n, dim = 1500, 64
    x = _planted(n, dim, 31)
    rng = np.random.default_rng(32)
    ids = (1 << 40) + 7919 * rng.permutation(n).astype(np.int64)
    index = LSHRS(dim=dim, num_perm=64, num_bands=8, rows_per_band=8, storage=InMemoryStorage(), packed_ingest=True,
                  keep_vectors=dtype)
    for lo in range(0, n, 500):
        index.index(ids[lo:lo + 500], x[lo:lo + 500])
    return index, x, ids, rng


def _most_collisions(got, but=()):
    """The pair of the answer `got` with the most collisions among those that involve none of `but`."""
    ok = [k for k in range(len(got[0])) if int(got[0][k]) not in but and int(got[1][k]) not in but]
    k = max(ok, key=lambda k: (int(got[3][k]), -k))
    return int(got[0][k]), int(got[1][k])


def _a_stranger(index, ids, to, but=()):
    """The first id that shares no bucket with `to` and is none of `but`."""
    cand = join_reference(index._storage.array_segments(1))[0]
    return next(int(i) for i in ids.tolist() if i != to and i not in but and (min(i, to), max(i, to)) not in cand)


def _same(one, two):
    return all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
               and a.dtype == b.dtype for a, b in zip(one, two))


@pytest.mark.parametrize("dtype", ("bfloat16", "int8"))
def test_the_store_route_after_reindexing_and_compaction(dtype):
    """DeviceVectors.lsh_pairs_above over a row block with superseded rows (map rows that stay all -1, row_ids of -1, members
    translated to the LATEST row), after compact(), after delete() and re-index, and the refusal of an id under two signatures
    through the whole LSHRS call."""
    index, x, ids, rng = _store_index(dtype)
    t = 0.6
    row_of = {int(i): r for r, i in enumerate(ids.tolist())}
    # 200 ids a second time, the SAME vectors: 200 superseded rows, the same buckets
    again = rng.choice(ids.shape[0], size=200, replace=False)
    index.index(ids[again], x[again])
    assert index.vectors.stats()["dead"] == 200 and index.vectors.stats()["live"] == 1500
    got, exact, _ = _check_whole_call(index, t)
    # compact(): other rows, the same answer, and the buckets did not change - nothing is folded again
    index.vectors.compact()
    assert index.vectors.stats()["dead"] == 0 and index.vectors.stats()["rows"] == 1500
    after = index.pairs_above(t, return_arrays=True)
    assert index.last_search_stats["segments_folded"] == 0
    assert _same(after, got) and len(got[0]) > 0
    assert _same(index.pairs_exact_above(t, return_arrays=True), exact)
    # X, which has a partner above the threshold, deleted and indexed again under a near copy of Z's vector
    big_x, partner = int(got[0][0]), int(got[1][0])
    big_z = _a_stranger(index, ids, big_x, but=(partner,))
    index.delete([big_x])
    index.index(np.array([big_x], dtype=np.int64), _near_copy(x[row_of[big_z]], rng)[None])
    assert index.vectors.stats()["dead"] == 1
    got, exact, _ = _check_whole_call(index, t)
    pairs = set(zip(got[0].tolist(), got[1].tolist()))
    assert (min(big_x, big_z), max(big_x, big_z)) in pairs
    # W indexed under a second vector WITHOUT a delete: old vector near Y's, new vector near Z2's
    special = (big_x, big_z, partner)
    big_w, big_y = _most_collisions(got, but=special)
    big_z2 = _a_stranger(index, ids, big_w, but=special + (big_y,))
    index.index(np.array([big_w], dtype=np.int64), _near_copy(x[row_of[big_z2]], rng)[None])
    segments = index._storage.array_segments(1)
    mine = {}
    for code, members in buckets_reference(segments).items():
        if big_w in members and len(members) >= 2:
            mine.setdefault(code >> 8, []).append(members)
    assert any(len(b) == 2 and any(big_y in m for m in b) and any(big_z2 in m and big_y not in m for m in b) for b in mine.values()), \
        "in some band W must share a bucket with Y under the old keys and another with Z2 under the new ones"
    cand = join_reference(segments)[0]
    assert (min(big_w, big_y), max(big_w, big_y)) in cand and (min(big_w, big_z2), max(big_w, big_z2)) in cand
    with pytest.raises(ValueError, match="two signatures"):
        index.pairs_above(t)
    with pytest.raises(ValueError, match="two signatures"):
        index.pairs_above(t, return_arrays=True, min_collisions=2)
    ea, eb, es = index.pairs_exact_above(t, return_arrays=True)
    assert (min(big_w, big_z2), max(big_w, big_z2)) in set(zip(ea.tolist(), eb.tolist()))      # (W's vector is the latest)
    # delete() cures it
    index.delete([big_w])
    _check_whole_call(index, t)


@pytest.mark.parametrize("dtype", ("bfloat16", "int8"))
def test_a_second_signature_whose_old_partner_is_gone(dtype):
    """As W above, but the old partner was deleted first: W's old buckets hold W alone, unless somebody else shares one, and a
    bucket of one member does not count - the row map does not see it.  Pinned here is what must hold either way: the call
    refuses the id, or every pair it returns is a pair of pairs_exact_above with that score, bit for bit (W is scored under
    its latest vector).  LSHRS.pairs_above's docstring says which of the two happens when.  With this corpus (1500 rows over
    256 keys a band) W's old buckets keep 4 to 13 members, old and new bucket count in every band, and the call raises today."""
    index, x, ids, rng = _store_index(dtype)
    t = 0.6
    row_of = {int(i): r for r, i in enumerate(ids.tolist())}
    got = index.pairs_above(t, return_arrays=True)
    big_w, big_y = _most_collisions(got)
    big_z = _a_stranger(index, ids, big_w, but=(big_y,))
    index.delete([big_y])
    index.index(np.array([big_w], dtype=np.int64), _near_copy(x[row_of[big_z]], rng)[None])
    codes_of_w = [code for code, members in buckets_reference(index._storage.array_segments(1)).items() if big_w in members]
    assert len(codes_of_w) > 8, "W must sit in two buckets of some band"
    ea, eb, es = index.pairs_exact_above(t, return_arrays=True)
    truth = dict(zip(zip(ea.tolist(), eb.tolist()), es.view(np.uint32).tolist()))
    assert (min(big_w, big_z), max(big_w, big_z)) in truth
    try:
        ga, gb, gs, _ = index.pairs_above(t, return_arrays=True)
    except ValueError as exc:
        assert "two signatures" in str(exc)
    else:
        assert len(ga) > 0
        for pair, bits in zip(zip(ga.tolist(), gb.tolist()), gs.view(np.uint32).tolist()):
            assert truth.get(pair) == bits, pair
