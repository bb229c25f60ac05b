"""The three kernels of csrc/graph.hip at their C ABI (include/lshrs_graph.h), through raw ctypes on device tensors: degree and
fill against np.bincount and per-row multisets, the select against a NumPy ranking by (key of the score, id) - every list
handed in under two different orders, every output between guard entries that must stay untouched."""

from __future__ import annotations

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 4096
N_ROWS = 300
HUB = 7                     # the row that is an endpoint of 1000 pairs


def _lib():
    from lshrs_amd import _native

    return _native.load_graph()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n, dtype, fill):
    """A device tensor of GUARD + n + GUARD entries, all `fill`, and the address of its entry GUARD."""
    import torch

    t = torch.full((2 * GUARD + n,), fill, dtype=dtype, device="cuda")
    return t, t.data_ptr() + GUARD * t.element_size()


def _guards_untouched(t, n, fill):
    host = t.cpu().numpy()
    same = (lambda x: np.isnan(x).all()) if isinstance(fill, float) and np.isnan(fill) else (lambda x: (x == fill).all())
    return bool(same(host[:GUARD])) and bool(same(host[GUARD + n:]))


@functools.lru_cache(maxsize=None)
def _pairs():
    """Hand pairs, 5 000 random pairs over 300 rows (repeats among them), and 1 000 pairs that all end in row HUB - in runs, so
    that the lanes of a wave add to the same word."""
    rng = np.random.default_rng(5)
    hand = np.array([[0, 1], [1, 2], [2, 0], [299, 0], [5, 6], [6, 5], [5, 6]], dtype=np.int64)
    a = rng.integers(0, N_ROWS, size=5000)
    b = (a + rng.integers(1, N_ROWS, size=5000)) % N_ROWS
    other = rng.integers(0, N_ROWS - 1, size=1000)
    other[other >= HUB] += 1
    hub = np.stack((np.where(np.arange(1000) % 2 == 0, HUB, other), np.where(np.arange(1000) % 2 == 0, other, HUB)), axis=1)
    pairs = np.concatenate((hand, np.stack((a, b), axis=1), hub)).astype(np.int64)
    assert np.all(pairs[:, 0] != pairs[:, 1])
    return pairs[:, 0].copy(), pairs[:, 1].copy()


def _valid(a, b, n_rows):
    return (a >= 0) & (a < n_rows) & (b >= 0) & (b < n_rows) & (a != b)


def _lists_reference(a, b, n_rows):
    ok = _valid(a, b, n_rows)
    lists = [[] for _ in range(n_rows)]
    for x, y in zip(a[ok].tolist(), b[ok].tolist()):
        lists[x].append(y)
        lists[y].append(x)
    return [sorted(x) for x in lists]


def _degree(a, b, n_rows):
    import torch

    lib = _lib()
    degree = torch.zeros(n_rows, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    da, db = _dev(a), _dev(b)
    rc = lib.lshrs_graph_degree_i64(da.data_ptr() if len(a) else None, db.data_ptr() if len(a) else None, len(a), n_rows,
                                    degree.data_ptr(), err.data_ptr(), None)
    assert rc == 0
    return degree.cpu().numpy(), int(err.item())


def _fill(a, b, n_rows, row_off):
    """fill into a guarded nbr preset to -7: (the 2 p entries, whether the guards are untouched)."""
    import torch

    lib = _lib()
    nbr, at = _guarded(2 * len(a), torch.int64, -7)
    cursor = torch.zeros(n_rows, dtype=torch.int32, device="cuda")
    da, db, off = _dev(a), _dev(b), _dev(np.asarray(row_off, dtype=np.int64))
    rc = lib.lshrs_graph_fill_i64(da.data_ptr() if len(a) else None, db.data_ptr() if len(a) else None, len(a), n_rows,
                                  off.data_ptr(), cursor.data_ptr(), at, None)
    assert rc == 0
    torch.cuda.synchronize()
    return nbr.cpu().numpy()[GUARD:GUARD + 2 * len(a)], _guards_untouched(nbr, 2 * len(a), -7)


def _offsets(degree):
    return np.r_[0, np.cumsum(degree.astype(np.int64))]


@pytest.mark.parametrize("n_pairs", (0, 1, 63, 64, 65, None))
def test_degree_and_fill_against_bincount_and_the_multisets(n_pairs):
    _lib()                              # (first: without the library nothing below is worth making)
    a, b = _pairs()
    if n_pairs is not None:
        a, b = a[-n_pairs:] if n_pairs else a[:0], b[-n_pairs:] if n_pairs else b[:0]        # (the hub's pairs: one word)
    else:
        assert int(np.sum(a == HUB) + np.sum(b == HUB)) >= 1000
    degree, err = _degree(a, b, N_ROWS)
    assert err == 0 and degree.dtype == np.int32
    assert np.array_equal(degree, np.bincount(np.r_[a, b], minlength=N_ROWS))
    off = _offsets(degree)
    assert off[-1] == 2 * len(a)
    nbr, clean = _fill(a, b, N_ROWS, off)
    assert clean
    want = _lists_reference(a, b, N_ROWS)
    for r in range(N_ROWS):
        assert sorted(nbr[off[r]:off[r + 1]].tolist()) == want[r], r


@pytest.mark.parametrize("bad_a, bad_b, bit", ((-1, 5, 1), (5, -1, 1), (N_ROWS, 5, 1), (5, N_ROWS, 1), (1 << 40, 5, 1), (9, 9, 2)))
def test_a_bad_pair_sets_its_bit_and_adds_nothing(bad_a, bad_b, bit):
    _lib()                              # (first: without the library nothing below is worth making)
    a, b = _pairs()
    a, b = np.r_[a[:100], bad_a, a[100:200]], np.r_[b[:100], bad_b, b[100:200]]
    degree, err = _degree(a, b, N_ROWS)
    ok = _valid(a, b, N_ROWS)
    assert err == bit and int(ok.sum()) == 200
    assert np.array_equal(degree, np.bincount(np.r_[a[ok], b[ok]], minlength=N_ROWS))
    off = _offsets(degree)
    nbr, clean = _fill(a, b, N_ROWS, off)
    want = _lists_reference(a, b, N_ROWS)
    assert clean and off[-1] == 400 and np.all(nbr[400:] == -7)
    for r in range(N_ROWS):
        assert sorted(nbr[off[r]:off[r + 1]].tolist()) == want[r], r


def test_offsets_that_do_not_belong_to_the_pairs_write_nothing_outside_the_lists():
    _lib()                              # (first: without the library nothing below is worth making)
    a, b = _pairs()
    want = _lists_reference(a, b, N_ROWS)
    # the offsets of the first 2 000 pairs only: every list is too short for what arrives
    degree, _ = _degree(a[:2000], b[:2000], N_ROWS)
    off = _offsets(degree)
    nbr, clean = _fill(a, b, N_ROWS, off)
    assert clean and np.all(nbr[off[-1]:] == -7)
    for r in range(N_ROWS):
        mine = nbr[off[r]:off[r + 1]].tolist()
        assert -7 not in mine and not set(mine) - set(want[r]), r          # full, and with nothing but the row's own partners
    # no list at all; lists that run backwards; offsets beyond nbr
    for off in (np.zeros(N_ROWS + 1, np.int64), np.arange(N_ROWS, -1, -1, dtype=np.int64) * 40,
                np.arange(N_ROWS + 1, dtype=np.int64) * 40 + 2 * len(a) - 40, np.full(N_ROWS + 1, -5, np.int64)):
        nbr, clean = _fill(a, b, N_ROWS, off)
        inside = np.zeros(2 * len(a), dtype=bool)
        for r in range(N_ROWS):
            inside[max(0, off[r]):max(0, min(off[r + 1], 2 * len(a)))] = True
        assert clean and np.all(nbr[~inside] == -7)


# ------------------------------------------------------------------------------------------
# select
# ------------------------------------------------------------------------------------------
N_IDS = 5000


def _keys(scores):
    u = scores.view(np.uint32).astype(np.int64)
    k = np.where(u & 0x80000000, u, u ^ 0x7FFFFFFF)
    k[np.isnan(scores)] = 0xFFFFFFFF
    return k


def _select_reference(lists, scores, ids_of, k):
    n = len(lists)
    out_ids, out_scores = np.full((n, k), -1, np.int64), np.full((n, k), np.nan, np.float32)
    count = np.zeros(n, np.int32)
    for r, (nb, sc) in enumerate(zip(lists, scores)):
        ids = ids_of(nb)
        order = np.lexsort((ids, _keys(sc)))[:k]
        count[r] = len(order)
        out_ids[r, :len(order)], out_scores[r, :len(order)] = ids[order], sc[order]
    return out_ids, out_scores, count


def _select(lists, scores, row_ids, k, n_ids=None, total=None, row_off=None):
    """The entry over the lists laid end to end, every output between guards: (ids, scores, count, err, guards untouched)."""
    import torch

    lib = _lib()
    n = len(lists)
    lens = np.array([len(x) for x in lists], dtype=np.int64)
    off = np.r_[0, np.cumsum(lens)] if row_off is None else np.asarray(row_off, dtype=np.int64)
    nbr = _dev(np.concatenate(lists).astype(np.int64) if n else np.zeros(0, np.int64))
    sc = _dev(np.concatenate(scores).astype(np.float32) if n else np.zeros(0, np.float32))
    d_off = _dev(off)
    d_ids = _dev(row_ids) if row_ids is not None else None
    out_ids, p_ids = _guarded(n * k, torch.int64, -9)
    out_scores, p_scores = _guarded(n * k, torch.float32, 77.0)
    out_count, p_count = _guarded(n, torch.int32, -9)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    size = int(nbr.shape[0]) if total is None else total
    rc = lib.lshrs_graph_select_f32(nbr.data_ptr() if size else None, sc.data_ptr() if size else None, d_off.data_ptr(), n, size,
                                    d_ids.data_ptr() if d_ids is not None else None,
                                    (len(row_ids) if n_ids is None else n_ids) if row_ids is not None else 0, k, p_ids, p_scores,
                                    p_count, err.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    clean = _guards_untouched(out_ids, n * k, -9) and _guards_untouched(out_scores, n * k, 77.0) and \
        _guards_untouched(out_count, n, -9)
    return (out_ids.cpu().numpy()[GUARD:GUARD + n * k].reshape(n, k), out_scores.cpu().numpy()[GUARD:GUARD + n * k].reshape(n, k),
            out_count.cpu().numpy()[GUARD:GUARD + n], int(err.item()), clean)


def _contents(kind, n, rng):
    if kind == "distinct":
        return rng.permutation(n).astype(np.float32) / np.float32(max(n, 1)) - np.float32(0.5)
    if kind == "equal":
        return np.full(n, 0.25, dtype=np.float32)
    if kind == "zeros":
        return rng.choice(np.array([0.0, -0.0, 1e-3, -1e-3], dtype=np.float32), size=n)
    assert kind == "nan"
    sc = rng.integers(0, 4, size=n).astype(np.float32) / np.float32(4)          # few values: ties among the numbers too
    sc[rng.random(n) < 0.4] = np.nan
    return sc


@pytest.mark.parametrize("kind", ("distinct", "equal", "zeros", "nan"))
@pytest.mark.parametrize("k", (1, 10, 64, 100))
def test_select_against_the_ranking_by_key_and_id(k, kind):
    lib = _lib()                        # (first: without the library nothing below is worth making)
    wave, longest = lib.lshrs_graph_wave_list(), lib.lshrs_graph_max_list()
    lengths = sorted({0, 1, k - 1, k, k + 1, 63, 64, 65, wave - 1, wave, wave + 1, longest - 1, longest, longest + 1})
    assert N_IDS > longest + 1
    rng = np.random.default_rng(1000 * k + len(kind))
    # ids in another order than the rows they stand at, and lists in another order than either
    row_ids = ((1 << 40) + 3 * rng.permutation(N_IDS)).astype(np.int64)
    lists = [rng.choice(N_IDS, size=n, replace=False).astype(np.int64) for n in lengths]
    scores = [_contents(kind, n, rng) for n in lengths]
    want_ids, want_scores, want_count = _select_reference(lists, scores, lambda nb: row_ids[nb], k)
    got_ids, got_scores, got_count, err, clean = _select(lists, scores, row_ids, k)
    assert err == 0 and clean
    over = lengths.index(longest + 1)
    assert got_count[over] == -1 and np.all(got_ids[over] == -9) and np.all(got_scores[over] == 77.0)
    rest = np.arange(len(lengths)) != over
    assert np.array_equal(got_count[rest], want_count[rest]) and want_count[rest].tolist() == [min(k, n) for n in lengths if n <= longest]
    assert np.array_equal(got_ids[rest], want_ids[rest])
    assert np.array_equal(got_scores[rest].view(np.uint32), want_scores[rest].view(np.uint32))
    for r, n in enumerate(lengths):                                     # the padding, said once more in its own words
        if n <= longest:
            assert np.all(got_ids[r, min(k, n):] == -1) and np.all(got_scores[r, min(k, n):].view(np.uint32) == 0x7FC00000)
    if kind == "equal":
        full = [r for r, n in enumerate(lengths) if k <= n <= longest]
        assert all(np.array_equal(got_ids[r], np.sort(row_ids[lists[r]])[:k]) for r in full) and full
    # the same lists in another order: the same bytes
    turned = [rng.permutation(n) for n in lengths]
    again = _select([x[p] for x, p in zip(lists, turned)], [s[p] for s, p in zip(scores, turned)], row_ids, k)
    assert again[3] == 0 and again[4]
    for x, y in zip((got_ids, got_scores, got_count), again[:3]):
        assert x.tobytes() == y.tobytes()
    # without row_ids the entry is its own id
    plain = _select(lists, scores, None, k)
    want_ids, want_scores, _ = _select_reference(lists, scores, lambda nb: nb, k)
    assert plain[3] == 0 and plain[4] and np.array_equal(plain[0][rest], want_ids[rest])
    assert np.array_equal(plain[1][rest].view(np.uint32), want_scores[rest].view(np.uint32))


def test_select_reports_what_it_does_not_read():
    _lib()                              # (first: without the library nothing below is worth making)
    rng = np.random.default_rng(3)
    row_ids = (100 + np.arange(50)).astype(np.int64)
    lists = [np.array([3, 4, 60, 5, -1], dtype=np.int64), np.array([7, 8], dtype=np.int64)]
    scores = [np.array([0.5, 0.25, 0.75, 0.1, 0.6], dtype=np.float32), np.array([0.1, 0.2], dtype=np.float32)]
    # entries outside row_ids go under the id -1 and are not looked up
    ids, sc, count, err, clean = _select(lists, scores, row_ids, 3)
    assert err == 2 and clean and count.tolist() == [3, 2]
    assert ids.tolist() == [[-1, -1, 103], [108, 107, -1]] and sc[0].tolist() == [0.75, 0.6000000238418579, 0.5]
    # a list that does not lie within [0, total]: nothing of it is read, the other rows are answered
    for off in ([0, 9, 11], [-1, 5, 7], [5, 0, 2]):
        ids, sc, count, err, clean = _select(lists, scores, row_ids, 3, row_off=off)
        assert err & 1 and clean and count[0] == 0 and np.all(ids[0] == -1) and np.isnan(sc[0]).all()
    ids, sc, count, err, clean = _select(lists, scores, row_ids, 3, row_off=[5, 0, 2])
    assert count.tolist() == [0, 2] and ids[1].tolist() == [103, 104, -1]
    del rng


# ------------------------------------------------------------------------------------------
# select: the workgroup tier's walk over the rows (lshrs_lists.h: walk_rows) beyond its first window
# ------------------------------------------------------------------------------------------
def _check_rows(got, lists, scores, row_ids, k, rows):
    """Rows `rows` of a _select answer against tests/_knn_join_reference.rank_list, bit for bit."""
    from tests._knn_join_reference import rank_list

    got_ids, got_scores, got_count = got[:3]
    for r in rows:
        want = rank_list(list(zip(row_ids[lists[r]].tolist(), scores[r].tolist())), k)
        assert got_count[r] == len(want), r
        assert got_ids[r].tolist() == [e[0] for e in want] + [-1] * (k - len(want)), r
        assert np.array_equal(got_scores[r, :len(want)].view(np.uint32), np.array([e[1] for e in want], np.float32).view(np.uint32)), r
        assert np.all(got_scores[r, len(want):].view(np.uint32) == 0x7FC00000), r


def test_select_walks_every_window_of_the_rows():
    """600 rows - two full windows of 256 and a ragged third: workgroup lists at both ends of every window, three of them and
    one beyond the limit noted in window 0, every other list empty or short."""
    lib = _lib()                        # (first: without the library nothing below is worth making)
    wave, longest = lib.lshrs_graph_wave_list(), lib.lshrs_graph_max_list()
    n, k, over = 600, 10, 50
    lengths = [r % 5 for r in range(n)]
    for r in (0, 7, 100, 255, 256, 511, 512, 599):
        lengths[r] = wave + 1
    lengths[over] = longest + 1
    rng = np.random.default_rng(600)
    row_ids = ((1 << 40) + 3 * rng.permutation(N_IDS)).astype(np.int64)
    lists = [rng.choice(N_IDS, size=c, replace=False).astype(np.int64) for c in lengths]
    scores = [_contents("nan" if r % 2 else "distinct", c, rng) for r, c in enumerate(lengths)]
    got = _select(lists, scores, row_ids, k)
    assert got[3] == 0 and got[4]
    assert got[2][over] == -1 and np.all(got[0][over] == -9) and np.all(got[1][over] == 77.0)
    _check_rows(got, lists, scores, row_ids, k, [r for r in range(n) if r != over])


def test_select_comes_round_to_a_workgroup_s_second_window():
    """2 x 256 x CUs + 257 rows: one window more than the resident grid of the workgroup kernel has workgroups, and a ragged
    one behind it - all rows empty but the last, whose list is the workgroup's."""
    import torch

    lib = _lib()                        # (first: without the library nothing below is worth making)
    wave = lib.lshrs_graph_wave_list()
    n = 2 * 256 * torch.cuda.get_device_properties(0).multi_processor_count + 257
    rng = np.random.default_rng(257)
    row_ids = ((1 << 40) + 3 * rng.permutation(N_IDS)).astype(np.int64)
    none = np.zeros(0, np.int64)
    lists = [none] * (n - 1) + [rng.choice(N_IDS, size=wave + 1, replace=False).astype(np.int64)]
    scores = [none.astype(np.float32)] * (n - 1) + [_contents("distinct", wave + 1, rng)]
    got = _select(lists, scores, row_ids, 1)
    assert got[3] == 0 and got[4]
    assert np.all(got[2][:n - 1] == 0) and np.all(got[0][:n - 1] == -1) and np.all(got[1][:n - 1].view(np.uint32) == 0x7FC00000)
    _check_rows(got, lists, scores, row_ids, 1, [n - 1])
