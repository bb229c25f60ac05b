"""The near-duplicate groups on the GPU (csrc/groups.hip, lshrs_amd/_groups.py, LSHRS.groups_above): the three kernels at
their ABI - through ctypes, on a label array that sits between sentinels - against a plain-Python union-find
(tests/_groups_reference.py), then the Python layers, the store and the index against the same reference over the joins' own
pairs.  Every comparison is exact array equality; err bit 1 (an iteration cap passed) is never set."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests._groups_reference import group_lists, groups_reference, labels_reference, removable

pytestmark = pytest.mark.gpu

SENTINEL = -0x5A5A5A5B
PAD = 96                      # int32 sentinels on each side of the labels


def _groups_library():
    """The library of the components, loaded.  The first statement of every test here: where it is missing the test fails
    at once, before it builds a corpus, an index or a reference."""
    from lshrs_amd import _native

    return _native.load_groups()


def _hooked(n, edge_lists, stream=None):
    """init, one hook per (a, b) of `edge_lists`, flatten - through ctypes, the label array inside a larger tensor and the
    error word inside another, sentinels around both.  Returns (labels, err bits, the forest before flatten)."""
    import torch

    lib = _groups_library()
    whole = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    errs = torch.tensor([SENTINEL, 0, SENTINEL], dtype=torch.int32, device="cuda")
    parent, err = whole[PAD:PAD + n], errs[1:2]
    dev = [(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda(),
            torch.from_numpy(np.ascontiguousarray(b, dtype=np.int64)).cuda()) for a, b in edge_lists]
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    assert lib.lshrs_cc_init_i32(parent.data_ptr(), n, s) == 0
    for a, b in dev:
        assert lib.lshrs_cc_hook_i64(a.data_ptr(), b.data_ptr(), int(a.shape[0]), parent.data_ptr(), n, err.data_ptr(), s) == 0
    if stream is not None:
        stream.synchronize()
    before = parent.cpu().numpy().copy()
    assert lib.lshrs_cc_flatten_i32(parent.data_ptr(), n, err.data_ptr(), s) == 0
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    got, outside, bits = whole.cpu().numpy(), errs.cpu().numpy(), int(errs[1].item())
    assert np.all(got[:PAD] == SENTINEL) and np.all(got[PAD + n:] == SENTINEL), "the kernels wrote outside the labels"
    assert outside[0] == SENTINEL and outside[2] == SENTINEL
    assert not bits & 2, "a lane passed its iteration cap"
    # parent[x] <= x before flatten, and the forest before flatten is the partition after it
    assert np.all(before <= np.arange(n)) and np.all(before >= 0)
    return got[PAD:PAD + n].copy(), bits, before


def _check(n, a, b, **kwargs):
    labels, bits, _ = _hooked(n, [(a, b)], **kwargs)
    assert bits == 0 and labels.dtype == np.int32
    assert np.array_equal(labels, labels_reference(a, b, n))
    return labels


def test_no_edges_and_one_edge():
    _groups_library()
    none = np.empty(0, np.int64)
    assert _check(1, none, none).tolist() == [0]
    assert _check(5, none, none).tolist() == [0, 1, 2, 3, 4]
    assert _check(5, [3], [1]).tolist() == [0, 1, 2, 1, 4]
    assert _check(5, [1], [3]).tolist() == [0, 1, 2, 1, 4]
    assert _check(2, [1, 0, 1], [1, 0, 0]).tolist() == [0, 0]
    assert _check(300, [299], [0])[299] == 0


@pytest.mark.parametrize("order", ("ascending", "descending", "shuffled"))
def test_a_path_over_every_xcd(order):
    """65 536 vertices in a path: 256 workgroups of edges, a chain that only path halving and flatten's two-level moves make
    shallow - descending is the order in which every hook lands on the top of the chain."""
    _groups_library()
    n = 65536
    low = np.arange(n - 1, dtype=np.int64)
    if order == "descending":
        low = low[::-1].copy()
    elif order == "shuffled":
        low = np.random.default_rng(7).permutation(low)
    flip = np.random.default_rng(8).random(n - 1) < 0.5 if order == "shuffled" else np.zeros(n - 1, dtype=bool)
    a, b = np.where(flip, low + 1, low), np.where(flip, low, low + 1)
    labels = _check(n, a, b)
    assert not labels.any()


def test_a_star_whose_centre_is_the_highest_vertex():
    _groups_library()
    n = 10001
    leaves = np.random.default_rng(9).permutation(n - 1).astype(np.int64)
    labels = _check(n, np.full(n - 1, n - 1, dtype=np.int64), leaves)
    assert not labels.any()
    assert not _check(n, leaves, np.full(n - 1, n - 1, dtype=np.int64)).any()


def _two_cliques():
    i, j = np.triu_indices(64, 1)
    first, second = (i + 10, j + 10), (i + 200, j + 200)
    return (np.r_[first[0], second[1]].astype(np.int64), np.r_[first[1], second[0]].astype(np.int64))


@pytest.mark.parametrize("bridge", ("first", "last", "none"))
def test_two_cliques_and_a_bridge(bridge):
    _groups_library()
    a, b = _two_cliques()
    if bridge == "first":
        a, b = np.r_[263, a], np.r_[10, b]
    elif bridge == "last":
        a, b = np.r_[a, 40], np.r_[b, 230]
    labels = _check(300, a, b)
    assert labels[10:74].tolist() == [10] * 64 and labels[200:264].tolist() == [10 if bridge != "none" else 200] * 64
    assert labels[:10].tolist() == list(range(10)) and labels[74:200].tolist() == list(range(74, 200))


def test_repeated_edges_both_orientations_and_self_loops():
    _groups_library()
    rng = np.random.default_rng(10)
    n = 500
    a, b = rng.integers(0, n, size=150), rng.integers(0, n, size=150)
    loops = rng.integers(0, n, size=50)
    many_a = np.r_[np.tile(a, 100), np.tile(b, 100), loops, loops]
    many_b = np.r_[np.tile(b, 100), np.tile(a, 100), loops, loops]
    shuffle = rng.permutation(many_a.shape[0])
    once = _check(n, a, b)
    assert np.array_equal(_check(n, many_a[shuffle], many_b[shuffle]), once)
    assert 1 < len(set(once.tolist())) < n


@functools.lru_cache(maxsize=None)
def _random_graph(degree, seed):
    n = 100_000
    rng = np.random.default_rng(1000 * seed + int(10 * degree))
    e = int(n * degree / 2)
    a, b = rng.integers(0, n, size=e), rng.integers(0, n, size=e)
    want = labels_reference(a, b, n)
    want.setflags(write=False)
    return n, a, b, want


@pytest.mark.parametrize("seed", (1, 2, 3))
@pytest.mark.parametrize("degree", (0.8, 1.0, 1.2))
def test_random_graphs_around_the_percolation_threshold(degree, seed):
    _groups_library()
    n, a, b, want = _random_graph(degree, seed)
    labels, bits, before = _hooked(n, [(a, b)])
    assert bits == 0 and np.array_equal(labels, want)
    sizes = np.bincount(want)
    assert sizes.max() > 50 and (sizes == 1).sum() > 1000          # long components and many small ones
    # the forest before flatten already is that partition: every vertex's root is its label
    roots = before.copy()
    for _ in range(17):                       # (pointer doubling: 2^17 levels, more than there are vertices)
        roots = roots[roots]
    assert np.array_equal(roots, want)


def test_hooking_in_three_calls_twice_and_on_another_stream():
    _groups_library()
    import torch

    n, a, b, want = _random_graph(1.0, 1)
    cut1, cut2 = a.shape[0] // 3, a.shape[0] // 3 * 2 + 1
    three = [(a[:cut1], b[:cut1]), (a[cut1:cut2], b[cut1:cut2]), (a[cut2:], b[cut2:])]
    labels, bits, _ = _hooked(n, three)
    assert bits == 0 and np.array_equal(labels, want)
    # the same list twice over, and two different lists: one call over all the edges
    labels, bits, _ = _hooked(n, [(a, b), (b, a)])
    assert bits == 0 and np.array_equal(labels, want)
    n2, a2, b2, _ = _random_graph(0.8, 2)
    labels, bits, _ = _hooked(n, [(a, b), (a2, b2)])
    assert bits == 0 and np.array_equal(labels, labels_reference(np.r_[a, a2], np.r_[b, b2], n))
    # the same call again, and on a stream of its own
    again, bits, _ = _hooked(n, [(a, b)])
    assert bits == 0 and np.array_equal(again, want)
    other, bits, _ = _hooked(n, [(a, b)], stream=torch.cuda.Stream())
    assert bits == 0 and np.array_equal(other, want)


def test_endpoints_outside_the_vertices_are_skipped_and_reported():
    _groups_library()
    rng = np.random.default_rng(11)
    n = 4000
    a, b = rng.integers(0, n, size=3000), rng.integers(0, n, size=3000)
    wrong_a = np.array([-1, 5, n, 7, 1 << 40, 9, -(1 << 40), n - 1, 1 << 31, (1 << 32) + 3], dtype=np.int64)
    wrong_b = np.array([3, -1, 2, n, 1, 1 << 40, 4, n, 6, 8], dtype=np.int64)
    at = rng.choice(3000, size=10, replace=False)
    all_a, all_b = np.insert(a, at, wrong_a), np.insert(b, at, wrong_b)
    labels, bits, _ = _hooked(n, [(all_a, all_b)])
    assert bits == 1
    assert np.array_equal(labels, labels_reference(a, b, n))          # the valid edges are joined, the others join nothing
    # the bit is or-ed in and stays: a clean list hooked after a bad one
    labels, bits, _ = _hooked(n, [(wrong_a, wrong_b), (a, b)])
    assert bits == 1 and np.array_equal(labels, labels_reference(a, b, n))
    labels, bits, _ = _hooked(n, [(wrong_a, wrong_b)])
    assert bits == 1 and np.array_equal(labels, np.arange(n))


# ---------------------------------------------------------------------------------------------------------------------------
# through Python
# ---------------------------------------------------------------------------------------------------------------------------
def _same_groups(got, want):
    return all(np.array_equal(g, w) and g.dtype == np.int64 for g, w in zip(got, want)) and len(got) == 2


def test_connected_labels_and_what_it_raises():
    _groups_library()
    import torch

    from lshrs_amd import _groups

    n, a, b, want = _random_graph(1.2, 3)
    labels = _groups.connected_labels(a, b, n)
    assert isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.int32
    assert np.array_equal(labels.cpu().numpy(), want)
    on_device = _groups.connected_labels(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), n)
    assert np.array_equal(on_device.cpu().numpy(), want)
    assert _groups.connected_labels([], [], 4).tolist() == [0, 1, 2, 3] and _groups.connected_labels([], [], 0).shape == (0,)
    for bad in (([4], [0]), ([0], [-1]), ([1 << 40], [0])):
        with pytest.raises(ValueError, match="outside"):
            _groups.connected_labels(*bad, 4)
    with pytest.raises(ValueError, match="outside"):
        _groups.connected_labels([0], [0], 0)


def test_hooking_in_slices(monkeypatch):
    _groups_library()
    from lshrs_amd import _groups

    n, a, b, want = _random_graph(1.0, 2)
    monkeypatch.setattr(_groups, "_HOOK_SLICE", 7001)
    assert a.shape[0] % 7001 != 0 and a.shape[0] > 7 * 7001
    assert np.array_equal(_groups.connected_labels(a, b, n).cpu().numpy(), want)


def test_group_pairs_on_arrays_and_on_device_tensors():
    _groups_library()
    import torch

    from lshrs_amd import group_pairs

    rng = np.random.default_rng(12)
    ids = rng.choice(1 << 62, size=5000, replace=False).astype(np.int64)
    ids[:3] = (0, 1 << 62, (1 << 62) - 1)
    a, b = ids[rng.integers(0, 5000, size=3500)], ids[rng.integers(0, 5000, size=3500)]
    want = groups_reference(a, b)
    assert want[0].max() == 1 << 62 and want[0].min() == 0 and 100 < want[1].shape[0] < 3000
    stats = {}
    got = group_pairs(a, b, stats=stats)
    assert _same_groups(got, want) and all(isinstance(g, np.ndarray) for g in got)
    sizes = np.diff(want[1])
    assert stats == {"pairs": 3500, "grouped": want[0].shape[0], "groups": sizes.shape[0], "largest": int(sizes.max())}
    assert _same_groups(group_pairs(a.tolist(), b.tolist()), want)
    assert _same_groups(group_pairs(b, a), want)
    tensors = group_pairs(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), return_tensors=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 for t in tensors)
    assert _same_groups([t.cpu().numpy() for t in tensors], want)
    assert _same_groups(group_pairs(torch.from_numpy(a), torch.from_numpy(b).cuda()), want)          # (a host tensor)
    # ids given in descending order, as a path: one group, ascending
    down = np.sort(ids)[::-1].copy()
    got = group_pairs(down[:-1], down[1:])
    assert _same_groups(got, groups_reference(down[:-1], down[1:])) and got[1].tolist() == [0, 5000]
    assert np.array_equal(got[0], np.sort(ids))
    # int32 ids, and pairs that are all a == b: groups of one member
    small = group_pairs(np.array([7, 7, 3], np.int32), np.array([7, 7, 3], np.int32))
    assert small[0].tolist() == [3, 7] and small[1].tolist() == [0, 1, 2]


def test_group_pairs_of_nothing():
    _groups_library()
    import torch

    from lshrs_amd import group_pairs

    stats = {"stale": 1}
    for got in (group_pairs([], [], stats=stats), group_pairs(np.empty(0, np.int64), np.empty(0, np.int64)),
                [t.cpu().numpy() for t in group_pairs(torch.empty(0, dtype=torch.int64, device="cuda"),
                                                      torch.empty(0, dtype=torch.int64, device="cuda"), return_tensors=True)]):
        assert _same_groups(got, groups_reference([], []))
        assert got[0].shape == (0,) and got[1].tolist() == [0]
    assert stats == {"pairs": 0, "grouped": 0, "groups": 0, "largest": 0}


CHAIN_COS = 0.85             # neighbours of a chain; two apart: 0.7225, three apart: 0.614
THRESHOLD = 0.8
CHAINS = (3,) * 40 + (5,) * 10 + (2,) * 30 + (9,)


def _chains(n, dim, seed):
    """n rows of which the first sum(CHAINS) are chains a ~ b ~ c ...: neighbours at a cosine of 0.85, everybody else in the
    chain below 0.73, the chains' rows scattered over the corpus by a permutation.  Returns (rows, [row numbers of a chain])."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim))
    at, chains = 0, []
    for length in CHAINS:
        basis = np.linalg.qr(rng.standard_normal((dim, length)))[0].T          # orthonormal directions
        v = [basis[0]]
        for k in range(1, length):
            v.append(CHAIN_COS * v[-1] + np.sqrt(1.0 - CHAIN_COS ** 2) * basis[k])
        x[at:at + length] = np.array(v) * rng.uniform(0.5, 3.0, size=(length, 1))
        chains.append(list(range(at, at + length)))
        at += length
    where = rng.permutation(n)
    out = np.empty_like(x)
    out[where] = x
    return out.astype(np.float32), [[int(where[r]) for r in c] for c in chains]


@functools.lru_cache(maxsize=None)
def _chain_corpus(dtype):
    """The planted corpus in `dtype` on the device, its ids, the planted groups by id - and the check, on the CPU in float64
    over the STORED values, that no score is near the threshold: the grouping does not hinge on a last bit."""
    import torch

    n, dim = 3000, 64
    x, chains = _chains(n, dim, 41)
    corpus = torch.from_numpy(x).cuda().to(getattr(torch, dtype))
    stored = corpus.float().cpu().numpy().astype(np.float64)
    unit = stored / np.linalg.norm(stored, axis=1, keepdims=True)
    scores = unit @ unit.T
    np.fill_diagonal(scores, -1.0)
    # the rerank rounds in float32 (about 1e-6 at 64 elements): 0.02 is four orders of magnitude of room
    assert np.abs(scores - THRESHOLD).min() > 0.02
    above = {(int(i), int(j)) for i, j in zip(*np.nonzero(np.triu(scores >= THRESHOLD)))}
    assert above == {(min(c[k], c[k + 1]), max(c[k], c[k + 1])) for c in chains for k in range(len(c) - 1)}
    ids = (1 << 41) + 104729 * np.random.default_rng(42).permutation(n).astype(np.int64)
    planted = sorted(sorted(int(ids[r]) for r in c) for c in chains)
    return corpus, ids, planted


@pytest.mark.parametrize("dtype", ("float32", "bfloat16"))
def test_exact_groups_on_planted_chains(dtype):
    _groups_library()
    import torch

    from lshrs_amd import exact_groups_above, exact_pairs_above

    corpus, ids, planted = _chain_corpus(dtype)
    pa, pb, _ = exact_pairs_above(corpus, THRESHOLD, row_ids=ids)
    assert pa.shape[0] == sum(c - 1 for c in CHAINS)
    want = groups_reference(pa, pb)
    stats = {}
    got = exact_groups_above(corpus, THRESHOLD, row_ids=ids, stats=stats)
    assert _same_groups(got, want)
    # ... which are the chains as they were planted: a ~ b ~ c in one group though a and c score 0.72
    assert group_lists(*got) == planted and len(planted) == len(CHAINS)
    assert stats["pairs"] == stats["kept"] == pa.shape[0] and stats["groups"] == len(CHAINS) and stats["largest"] == 9
    assert stats["grouped"] == sum(CHAINS) and stats["rows"] == 3000 and stats["launches"] == 1
    tensors = exact_groups_above(corpus, THRESHOLD, row_ids=ids, return_tensors=True)
    assert all(isinstance(t, torch.Tensor) and t.device == corpus.device for t in tensors)
    assert _same_groups([t.cpu().numpy() for t in tensors], want)
    # without ids the row is the id; above every score nothing is grouped
    rows = exact_groups_above(corpus, THRESHOLD)
    assert _same_groups(rows, groups_reference(*exact_pairs_above(corpus, THRESHOLD)[:2])) and rows[1].shape[0] == len(CHAINS) + 1
    assert _same_groups(exact_groups_above(corpus, 0.95, row_ids=ids), groups_reference([], []))
    with pytest.raises(ValueError, match="max_pairs"):
        exact_groups_above(corpus, THRESHOLD, row_ids=ids, max_pairs=10)


def test_the_store_groups_under_its_ids_and_a_removed_bridge_splits_a_group():
    _groups_library()
    from lshrs_amd import DeviceVectors

    corpus, ids, planted = _chain_corpus("float32")
    store = DeviceVectors(64, "float32")
    half = 1500
    store.add(ids[:half], corpus[:half])
    store.add(ids[half:], corpus[half:])
    got = store.groups_above(THRESHOLD)
    stats = dict(store.last_search_stats)
    assert group_lists(*got) == planted
    assert _same_groups(got, groups_reference(*store.pairs_above(THRESHOLD)[:2]))
    assert stats["groups"] == len(CHAINS) and stats["largest"] == 9 and stats["pairs"] == stats["kept"]
    # the middle of the chain of nine goes: four and four
    nine = next(g for g in planted if len(g) == 9)
    rows_of = {int(i): r for r, i in enumerate(ids.tolist())}
    _, chains = _chains(3000, 64, 41)
    chain = next(c for c in chains if len(c) == 9)
    bridge = int(ids[chain[4]])
    assert bridge in nine and rows_of[bridge] == chain[4]
    assert store.remove([bridge]) == 1
    after = store.groups_above(THRESHOLD)
    stats = dict(store.last_search_stats)
    assert _same_groups(after, groups_reference(*store.pairs_above(THRESHOLD)[:2]))
    halves = sorted([sorted(int(ids[r]) for r in chain[:4]), sorted(int(ids[r]) for r in chain[5:])])
    assert sorted([g for g in planted if g != nine] + halves) == group_lists(*after)
    assert stats["groups"] == len(CHAINS) + 1 and stats["largest"] == 5


def _noisy_copies(n, dim, seed, copies, duplicates):
    """n float32 rows: `copies` rows with two noisy copies each (cosines between about 0.62 and 0.95), and `duplicates` rows
    that are exact copies of another row.  Returns (rows, [(row, row of its exact copy)])."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    src = rng.choice(n // 2, size=copies, replace=False)
    assert n // 2 + 2 * copies + duplicates <= n
    for k in range(2):
        sigma = rng.uniform(0.3, 1.25, size=(copies, 1)).astype(np.float32)
        x[n // 2 + copies * k + np.arange(copies)] = x[src] * rng.uniform(0.5, 2.0, size=(copies, 1)).astype(np.float32) \
            + sigma * rng.standard_normal((copies, dim)).astype(np.float32)
    first = n // 2 + 2 * copies
    twins = [(int(r), first + k) for k, r in enumerate(rng.choice(n // 2, size=duplicates, replace=False))]
    for r, copy in twins:
        x[copy] = x[r]
    return x, twins


@functools.lru_cache(maxsize=None)
def _index():
    from lshrs_amd import LSHRS, InMemoryStorage

    n, dim = 2000, 64
    x, twins = _noisy_copies(n, dim, 51, copies=200, duplicates=40)
    ids = (1 << 40) + 7919 * np.random.default_rng(52).permutation(n).astype(np.int64)
    index = LSHRS(dim=dim, num_perm=64, num_bands=8, rows_per_band=8, storage=InMemoryStorage(), packed_ingest=True,
                  keep_vectors="float32")
    for lo in range(0, n, 500):
        index.index(ids[lo:lo + 500], x[lo:lo + 500])
    return index, ids, twins


def test_the_index_groups_out_of_its_buckets():
    _groups_library()
    index, ids, twins = _index()
    t = 0.6
    pa, pb, _, _ = index.pairs_above(t, return_arrays=True)
    want = groups_reference(pa, pb)
    got = index.groups_above(t, return_arrays=True)
    stats = dict(index.last_search_stats)
    assert _same_groups(got, want) and want[1].shape[0] > 100
    assert index.groups_above(t) == group_lists(*want)
    assert stats["pairs"] == stats["kept"] == pa.shape[0] and stats["groups"] == want[1].shape[0] - 1
    assert stats["grouped"] == want[0].shape[0] and stats["largest"] == int(np.diff(want[1]).max())
    assert {"buckets", "raw_pairs", "emitted", "launches", "segments_folded", "fold_ms"} <= set(stats)
    # the exact groups, from the exact pairs
    ea, eb, _ = index.pairs_exact_above(t, return_arrays=True)
    truth = groups_reference(ea, eb)
    exact = index.groups_exact_above(t, return_arrays=True)
    assert _same_groups(exact, truth) and index.groups_exact_above(t) == group_lists(*truth)
    assert index.last_search_stats["groups"] == truth[1].shape[0] - 1 and index.last_search_stats["rows"] >= 2000
    # every LSH group lies inside exactly one exact group, and the buckets miss some of the truth
    home = {}
    for k, group in enumerate(group_lists(*truth)):
        home.update((i, k) for i in group)
    for group in group_lists(*got):
        assert len({home[i] for i in group}) == 1, group
    assert pa.shape[0] < ea.shape[0] and removable(got[1]) < removable(truth[1])
    # exact duplicates always collide: each with its twin in one group
    mine = {}
    for k, group in enumerate(group_lists(*got)):
        mine.update((i, k) for i in group)
    for r, copy in twins:
        assert mine[int(ids[r])] == mine[int(ids[copy])]
    # the join's keywords go through: pairs of two bands and more
    two = index.groups_above(t, min_collisions=2, return_arrays=True)
    pa2, pb2, _, _ = index.pairs_above(t, min_collisions=2, return_arrays=True)
    assert _same_groups(two, groups_reference(pa2, pb2)) and 0 < pa2.shape[0] < pa.shape[0]


def test_recall_of_the_groups():
    _groups_library()
    index, ids, twins = _index()
    t = 0.6
    lsh = groups_reference(*index.pairs_above(t, return_arrays=True)[:2])
    truth = groups_reference(*index.pairs_exact_above(t, return_arrays=True)[:2])
    rec = index.recall_groups_above(t)
    assert set(rec) == {"groups", "truth_groups", "removable", "truth_removable", "recall", "largest", "truth_largest"}
    assert rec["groups"] == lsh[1].shape[0] - 1 and rec["truth_groups"] == truth[1].shape[0] - 1
    assert rec["removable"] == removable(lsh[1]) and rec["truth_removable"] == removable(truth[1])
    assert rec["recall"] == removable(lsh[1]) / removable(truth[1]) and 0.0 < rec["recall"] < 1.0
    assert rec["largest"] == int(np.diff(lsh[1]).max()) and rec["truth_largest"] == int(np.diff(truth[1]).max())
    assert index.last_search_stats["groups"] == rec["groups"] and "fold_ms" in index.last_search_stats
    assert len(twins) <= rec["removable"]
    # nothing reaches 1.0 but the exact duplicates, which always collide: everything is recovered
    high = index.recall_groups_above(0.9999)
    assert high["truth_removable"] == high["removable"] == len(twins) and high["recall"] == 1.0


def test_the_empty_index_and_a_store_without_bucket_arrays():
    _groups_library()
    from lshrs_amd import LSHRS, InMemoryStorage

    empty = LSHRS(dim=64, num_perm=64, num_bands=8, rows_per_band=8, storage=InMemoryStorage(), packed_ingest=True,
                  keep_vectors="float32")
    assert empty.groups_above(0.5) == [] and empty.groups_exact_above(0.5) == []
    got = empty.groups_above(0.5, return_arrays=True)
    assert _same_groups(got, groups_reference([], []))
    assert empty.last_search_stats["groups"] == 0 and empty.last_search_stats["emitted"] == 0
    rec = empty.recall_groups_above(0.5)
    assert rec["recall"] == 1.0 and rec["groups"] == rec["truth_groups"] == rec["removable"] == rec["largest"] == 0
    x, _ = _noisy_copies(600, 64, 53, copies=50, duplicates=5)
    tuples = LSHRS(dim=64, num_perm=64, num_bands=8, rows_per_band=8, storage=InMemoryStorage(), packed_ingest=False,
                   keep_vectors="float32")
    tuples.index(np.arange(600, dtype=np.int64) * 3 + (1 << 33), x)
    with pytest.raises(RuntimeError, match="array"):
        tuples.groups_above(0.6)
    assert len(tuples.groups_exact_above(0.6)) > 0          # (the exact groups need no buckets)
