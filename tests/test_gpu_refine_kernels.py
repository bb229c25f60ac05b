"""The kernels of csrc/refine.hip at their C ABI (include/lshrs_refine.h), through raw ctypes on device tensors, and the
device-level entries around them (lshrs_amd._refine.graph_edges, expand_candidates): the edges against the plain-Python rule,
the expansion against sets - per tier, at both tier boundaries, under a degree cap, under every order of its input - and every
output between guard entries that must stay untouched."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests._refine_reference import adjacency_of, bound_reference, csr_of, edges_reference, expand_reference

pytestmark = pytest.mark.gpu

GUARD = 4096


def _lib():
    from lshrs_amd import _native, _refine

    assert callable(_refine.expand_candidates)
    return _native.load_refine()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n, dtype, fill):
    """A device tensor of GUARD + n + GUARD entries, all `fill`, and the address of its entry GUARD."""
    import torch

    t = torch.full((2 * GUARD + n,), fill, dtype=dtype, device="cuda")
    return t, t.data_ptr() + GUARD * t.element_size()


def _inside(t, n, fill):
    """(the n entries between the guards, whether the guards are untouched)"""
    host = t.cpu().numpy()
    return host[GUARD:GUARD + n], bool((host[:GUARD] == fill).all() and (host[GUARD + n:] == fill).all())


def _edges(graph):
    import torch

    lib = _lib()
    graph = np.ascontiguousarray(graph, dtype=np.int64)
    n_rows, k_in = graph.shape
    keep, at = _guarded(n_rows * k_in, torch.uint8, 9)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.lshrs_refine_edges_i64(_dev(graph).data_ptr(), n_rows, k_in, at, err.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got, clean = _inside(keep, n_rows * k_in, 9)
    return got.reshape(n_rows, k_in), int(err.item()), clean


def _random_table(n, k_in, seed):
    """A table with planted mutual pairs, duplicates inside a row and -1s; no row lists itself."""
    rng = np.random.default_rng(seed)
    graph = (np.arange(n)[:, None] + rng.integers(1, n, size=(n, k_in))) % n
    for r in range(0, n, 3):                        # mutual: the first entry of r's first neighbour is r
        graph[graph[r, 0], 0] = r
    for r in range(1, n, 5):                        # a duplicate inside the row
        graph[r, k_in - 1] = graph[r, 0]
    graph[rng.random((n, k_in)) < 0.15] = -1
    assert not (graph == np.arange(n)[:, None]).any()
    return graph.astype(np.int64)


def test_edges_against_the_rule():
    _lib()                              # (first: without the library nothing below is worth making)
    graph = _random_table(64, 4, 1)
    want = edges_reference(graph)
    mutual = sum(1 for r in range(64) for g in graph[r] if g >= 0 and r in graph[g].tolist())
    assert mutual >= 20 and (graph == -1).sum() >= 20 and any(len(set(x[x >= 0].tolist())) < (x >= 0).sum() for x in graph)
    keep, err, clean = _edges(graph)
    assert err == 0 and clean and keep.dtype == np.uint8 and np.array_equal(keep, want)
    # every undirected pair of the table exactly once
    pairs = [(min(r, int(graph[r, c])), max(r, int(graph[r, c]))) for r, c in zip(*np.nonzero(keep))]
    every = {(min(r, int(g)), max(r, int(g))) for r in range(64) for g in graph[r] if g >= 0}
    assert len(pairs) == len(set(pairs)) and set(pairs) == every
    # the same through the module's entry; other shapes of the grid
    from lshrs_amd import graph_edges

    got, d_err = graph_edges(_dev(graph))
    assert np.array_equal(got.cpu().numpy(), want) and int(d_err.item()) == 0
    for n, k_in in ((1, 1), (2, 1), (65, 3), (300, 7)):
        graph = _random_table(n, k_in, n) if n > 2 else np.array([[-1]] if n == 1 else [[1], [0]], dtype=np.int64)
        keep, err, clean = _edges(graph)
        assert err == 0 and clean and np.array_equal(keep, edges_reference(graph)), (n, k_in)


@pytest.mark.parametrize("bad, bit", ((64, 1), (-2, 1), (1 << 40, 1), (-(1 << 40), 1), ("self", 2)))
def test_an_entry_that_has_no_business_in_the_table_sets_its_bit_and_is_not_read_through(bad, bit):
    _lib()                              # (first: without the library nothing below is worth making)
    graph = _random_table(64, 4, 2)
    graph[17, 1] = 17 if bad == "self" else bad
    graph[63, 3] = 63 if bad == "self" else bad         # (the table's last entry: a read through it would leave the table)
    keep, err, clean = _edges(graph)
    assert err == bit and clean and keep[17, 1] == 0 and keep[63, 3] == 0
    assert np.array_equal(keep, edges_reference(graph))


# ------------------------------------------------------------------------------------------
# expand
# ------------------------------------------------------------------------------------------
def _count(nbr, off, n_rows, max_degree=0, total=None):
    import torch

    lib = _lib()
    count, at = _guarded(n_rows, torch.int32, -9)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_nbr, d_off = _dev(nbr), _dev(off)
    size = len(nbr) if total is None else total
    assert lib.lshrs_refine_expand_count_i64(d_nbr.data_ptr() if size else None, d_off.data_ptr(), n_rows, size, max_degree,
                                             at, err.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got, clean = _inside(count, n_rows, -9)
    return got, int(err.item()), clean


def _write(nbr, off, n_rows, cand_off, max_degree=0, cand_total=None):
    import torch

    lib = _lib()
    cand_off = np.asarray(cand_off, dtype=np.int64)
    size = int(cand_off[-1]) if cand_total is None else cand_total
    cand, at = _guarded(size, torch.int64, -7)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_nbr, d_off, d_coff = _dev(nbr), _dev(off), _dev(cand_off)
    assert lib.lshrs_refine_expand_write_i64(d_nbr.data_ptr() if len(nbr) else None, d_off.data_ptr(), n_rows, len(nbr),
                                             max_degree, d_coff.data_ptr(), at if size else None, size, err.data_ptr(),
                                             None) == 0
    torch.cuda.synchronize()
    got, clean = _inside(cand, size, -7)
    return got, int(err.item()), clean


def _expand_at_the_abi(lists, max_degree=0):
    """count, prefix, write over `lists`: (the counts, [sorted list per row], err of both, guards untouched)."""
    nbr, off = csr_of(lists)
    n = len(lists)
    count, err, clean = _count(nbr, off, n, max_degree)
    cand_off = np.r_[0, np.cumsum(np.maximum(count, 0).astype(np.int64))]
    cand, err2, clean2 = _write(nbr, off, n, cand_off, max_degree)
    return count, [cand[cand_off[r]:cand_off[r + 1]].tolist() for r in range(n)], err | err2, clean and clean2


def test_expand_in_the_wave_tier():
    lib = _lib()                        # (first: without the library nothing below is worth making)
    lists = adjacency_of(_random_table(300, 4, 3))
    want = expand_reference(lists)
    assert max(bound_reference(lists)) <= lib.lshrs_refine_wave_set()
    count, got, err, clean = _expand_at_the_abi(lists)
    assert err == 0 and clean and count.dtype == np.int32
    assert count.tolist() == [len(x) for x in want]
    for r in range(300):
        assert len(set(got[r])) == len(got[r]) and r not in got[r], r
        assert sorted(got[r]) == sorted(want[r]), r
    # rows without a list, and a graph without an entry
    count, got, err, clean = _expand_at_the_abi([[1], [0], [], [], [5], [4]])
    assert err == 0 and clean and count.tolist() == [1, 1, 0, 0, 1, 1] and got == [[1], [0], [], [], [5], [4]]
    count, got, err, clean = _expand_at_the_abi([[], [], []])
    assert err == 0 and clean and count.tolist() == [0, 0, 0]


def _bipartite(t, s):
    """K(t, s): the rows 0 .. t-1 each adjacent to all of t .. t+s-1.  U = t s + s on the left, t s + t on the right."""
    left, right = list(range(t)), list(range(t, t + s))
    return [list(right) for _ in left] + [list(left) for _ in right]


def _one_above(limit):
    """(t, s) of the K(t, s) whose LEFT rows have U = s (t + 1) = limit + 1, t >= 2 the smallest there is."""
    for t in range(2, limit):
        if (limit + 1) % (t + 1) == 0:
            return t, (limit + 1) // (t + 1)
    raise AssertionError(f"{limit + 1} is prime")


@functools.lru_cache(maxsize=None)
def _boundary_graph():
    """Five complete bipartite graphs side by side.  U of a LEFT row of K(t, s) is s (t + 1), of a right row t (s + 1): left
    rows exactly at each of the two limits (t + 1 = 32 resp. 64), left rows one above each, and a K(70, 130) far above both."""
    lib = _lib()
    wave, most = lib.lshrs_refine_wave_set(), lib.lshrs_refine_max_set()
    assert wave % 32 == 0 and most % 64 == 0
    parts = [_bipartite(31, wave // 32), _bipartite(*_one_above(wave)), _bipartite(63, most // 64),
             _bipartite(*_one_above(most)), _bipartite(70, 130)]
    lists, base = [], 0
    for part in parts:
        lists += [[v + base for v in row] for row in part]
        base += len(part)
    return lists, wave, most


def test_expand_at_the_tier_boundaries():
    from lshrs_amd import expand_candidates

    lists, wave, most = _boundary_graph()
    bounds = bound_reference(lists)
    for limit in (wave, most):
        assert limit in bounds and limit + 1 in bounds
    beyond = [r for r, u in enumerate(bounds) if u > most]
    assert beyond and max(bounds) > 9000 and len(lists) < 12000
    want = expand_reference(lists)
    count, got, err, clean = _expand_at_the_abi(lists)
    assert err == 0 and clean
    for r in range(len(lists)):
        if bounds[r] > most:
            assert count[r] == -1 and got[r] == [], r
        else:
            assert count[r] == len(want[r]) and len(set(got[r])) == len(got[r]) and set(got[r]) == want[r], (r, bounds[r])
    # the module's entry finishes the rows beyond with torch
    stats = {}
    nbr, off = csr_of(lists)
    cand, cand_off, d_err = expand_candidates(_dev(nbr), _dev(off), stats=stats)
    cand, cand_off = cand.cpu().numpy(), cand_off.cpu().numpy()
    assert int(d_err.item()) == 0 and stats["torch_rows"] == len(beyond) and stats["skipped_midpoints"] == 0
    assert np.diff(cand_off).tolist() == [len(x) for x in want]
    for r in range(len(lists)):
        mine = cand[cand_off[r]:cand_off[r + 1]].tolist()
        assert len(set(mine)) == len(mine) and set(mine) == want[r], r


def test_a_row_over_the_cap_is_a_candidate_and_no_midpoint():
    from lshrs_amd import expand_candidates

    _lib()
    # a star of degree 40 (hub 0), and a path 41 - 42 - 43 beside it
    lists = [list(range(1, 41))] + [[0]] * 40 + [[42], [41, 43], [42]]
    want = expand_reference(lists, max_degree=8)
    assert want[0] == set(range(1, 41)) and all(want[r] == {0} for r in range(1, 41)) and want[41] == {42, 43}
    count, got, err, clean = _expand_at_the_abi(lists, max_degree=8)
    assert err == 0 and clean and count.tolist() == [len(x) for x in want]
    assert all(set(got[r]) == want[r] for r in range(len(lists)))
    stats = {}
    nbr, off = csr_of(lists)
    cand, cand_off, _ = expand_candidates(_dev(nbr), _dev(off), 8, stats)
    assert stats["skipped_midpoints"] == 1 and stats["torch_rows"] == 0
    assert np.diff(cand_off.cpu().numpy()).tolist() == [len(x) for x in want]
    # at the cap itself the hub connects its leaves
    count, got, err, clean = _expand_at_the_abi(lists, max_degree=40)
    assert err == 0 and all(set(got[r]) == expand_reference(lists)[r] for r in range(len(lists))) and count[1] == 40


def test_the_sets_do_not_depend_on_any_order():
    from lshrs_amd import expand_candidates
    from lshrs_amd._knn_join import pair_adjacency

    _lib()
    graph = _random_table(300, 4, 4)
    lists = adjacency_of(graph)
    want = expand_reference(lists)
    rng = np.random.default_rng(8)
    turned = [rng.permutation(x).tolist() for x in lists]
    count, got, err, clean = _expand_at_the_abi(turned)
    assert err == 0 and clean and all(set(got[r]) == want[r] and len(got[r]) == len(want[r]) for r in range(300))
    # the pairs themselves in two orders, through the adjacency kernels
    keep = edges_reference(graph)
    at = np.argwhere(keep)
    a, b = at[:, 0].astype(np.int64), graph[at[:, 0], at[:, 1]].astype(np.int64)
    for order in (np.arange(len(a)), rng.permutation(len(a))):
        flip = rng.random(len(a)) < 0.5
        pa, pb = np.where(flip, b, a)[order], np.where(flip, a, b)[order]
        nbr, row_off, _ = pair_adjacency(_dev(pa), _dev(pb), 300)
        cand, cand_off, d_err = expand_candidates(nbr, row_off)
        cand, cand_off = cand.cpu().numpy(), cand_off.cpu().numpy()
        assert int(d_err.item()) == 0
        assert all(sorted(cand[cand_off[r]:cand_off[r + 1]].tolist()) == sorted(want[r]) for r in range(300))


def test_offsets_that_do_not_belong_set_the_bit_and_nothing_leaves_the_arrays():
    _lib()
    lists = adjacency_of(_random_table(300, 4, 5))
    want = expand_reference(lists)
    nbr, off = csr_of(lists)
    lens = np.array([len(x) for x in want], dtype=np.int64)
    good = np.r_[0, np.cumsum(lens)]
    # row_off: lists beyond nbr, lists that run backwards, negative ones - they count as empty and are reported
    for wrong in (off + len(nbr), off[::-1].copy(), np.full_like(off, -5)):
        count, err, clean = _count(nbr, wrong, 300)
        assert err & 1 and clean and np.all(count >= 0)
        _, err, clean = _write(nbr, wrong, 300, good)
        assert err & 1 and clean
    # one row's list out of range: that row is empty, and is nobody's midpoint
    wrong = off.copy()
    wrong[300] = len(nbr) + 1
    count, err, clean = _count(nbr, wrong, 300)
    cut = expand_reference(lists[:299] + [[]])
    assert err == 1 and clean and len(lists[299]) and count.tolist() == [len(x) for x in cut]
    # an entry outside the rows is skipped and reported
    broken = nbr.copy()
    broken[off[7]] = 300
    count, err, clean = _count(broken, off, 300)
    assert err == 2 and clean
    ref = expand_reference([[300 if (r == 7 and i == 0) else v for i, v in enumerate(x)] for r, x in enumerate(lists)])
    assert count.tolist() == [len(x) for x in ref]
    # cand_off: every list one entry short - full, with nothing but the row's own candidates, and reported; lists beyond
    # cand, backwards, negative: nothing is written at all
    short = np.r_[0, np.cumsum(np.maximum(lens - 1, 0))]
    cand, err, clean = _write(nbr, off, 300, short)
    assert err & 1 and clean
    for r in range(300):
        mine = cand[short[r]:short[r + 1]].tolist()
        assert -7 not in mine and len(set(mine)) == len(mine) and not set(mine) - want[r], r
    for wrong in (good + good[-1], good[::-1].copy(), np.full_like(good, -5)):
        cand, err, clean = _write(nbr, off, 300, wrong, cand_total=int(good[-1]))
        assert err & 1 and clean and np.all(cand == -7)
    # the right offsets into an array that ends early: the lists beyond it are not written
    cand, err, clean = _write(nbr, off, 300, good, cand_total=int(good[150]))
    assert err & 1 and clean
    for r in range(150):
        assert sorted(cand[good[r]:good[r + 1]].tolist()) == sorted(want[r]), r


# ------------------------------------------------------------------------------------------
# expand: the workgroup tier's walk over the rows (lshrs_lists.h: walk_rows) beyond its first window
# ------------------------------------------------------------------------------------------
def _check_expansion(count, got, want, rows):
    for r in rows:
        assert count[r] == len(want[r]) and len(set(got[r])) == len(got[r]) and set(got[r]) == want[r], r


def test_expand_walks_every_window_of_the_rows():
    """Rows 0 .. 599 - two full windows of 256 and a third: workgroup rows at both ends of each, three of them and one beyond
    the limit noted in window 0, every other row empty.  A workgroup row's list is wave_set + 1 DISTINCT rows with empty lists,
    the row beyond's max_set + 1 of them: 600 rows cannot hold those, so max_set + 1 empty rows stand behind the 600 - and behind
    them one more workgroup row, the last of a ragged window."""
    lib = _lib()                        # (first: without the library nothing below is worth making)
    wave, most = lib.lshrs_refine_wave_set(), lib.lshrs_refine_max_set()
    n, over = 600 + most + 2, 50
    assert n % 256
    lists = [[] for _ in range(n)]
    for r in (0, 7, 100, 255, 256, 511, 512, 599, n - 1):
        lists[r] = list(range(600 + r % 97, 600 + r % 97 + wave + 1))
    lists[over] = list(range(600, 600 + most + 1))
    bounds = bound_reference(lists)
    assert sorted(set(bounds)) == [0, wave + 1, most + 1] and max(map(max, (x for x in lists if x))) < n - 1
    want = expand_reference(lists)
    count, got, err, clean = _expand_at_the_abi(lists)
    assert err == 0 and clean
    assert count[over] == -1 and got[over] == []
    _check_expansion(count, got, want, [r for r in range(n) if r != over])


def test_expand_comes_round_to_a_workgroup_s_second_window():
    """2 x 256 x CUs + 257 rows: one window more than the resident grid of the workgroup kernel has workgroups, and a ragged
    one behind it - all rows empty but the last, which is the workgroup's."""
    import torch

    lib = _lib()                        # (first: without the library nothing below is worth making)
    wave = lib.lshrs_refine_wave_set()
    n = 2 * 256 * torch.cuda.get_device_properties(0).multi_processor_count + 257
    own = list(range(1000, 1000 + wave + 1))
    nbr, off = np.array(own, dtype=np.int64), np.r_[np.zeros(n, np.int64), len(own)]
    small = [own] + [[]] * (1000 + wave + 1)           # (the reference of the one row, on a table it fits in)
    want = expand_reference(small)[0]
    assert bound_reference(small)[0] == wave + 1 and len(want) == len(own)
    count, err, clean = _count(nbr, off, n)
    assert err == 0 and clean and np.all(count[:n - 1] == 0) and count[n - 1] == len(want)
    cand, err, clean = _write(nbr, off, n, np.r_[np.zeros(n, np.int64), len(own)])
    assert err == 0 and clean and len(cand) == len(want) and set(cand.tolist()) == want
