"""The two kernels of the LSH self-join (csrc/join.hip) at their C ABI, through ctypes: the row map cell by cell and its error
bits, the emit at every width of its map loads, raw pairs whose number needs more than a float's and more than 32 bits
(reached through raw_begin), and what the emit does at and behind its capacity.  Everything compared is an integer."""

from __future__ import annotations

import functools
import re

import numpy as np
import pytest

from tests._join_reference import hand_segment, join_reference, pair_of, rowmap_reference
from tests.test_gpu_lsh_join import PLANTED, _run, _segment

pytestmark = pytest.mark.gpu

MAP_SHAPES = ((1, 1), (2, 1), (3, 2), (4, 1), (6, 2), (6, 6), (7, 3), (10, 1), (12, 4))
PAD = 0x5A
CANARY, CANARY32 = -0x0123456789ABCDEF, 0x5A5A5A5A
E_TWO, E_BAND, E_MISSING, E_BEYOND = 1, 2, 256, 512


def _upload(seg):
    import torch

    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda() for a in (seg.codes, seg.offsets, seg.members))


def _prefix(seg, max_bucket=None):
    """The exclusive prefix sum of the counted buckets' pair counts, and their total."""
    lens = np.diff(seg.offsets)
    counted = (lens >= 2) & (lens <= (1 << 62 if max_bucket is None else max_bucket))
    return np.r_[0, np.cumsum(np.where(counted, lens * (lens - 1) // 2, 0))].astype(np.int64)


def _rowmap(seg, dev, n_rows, nb, bb, max_bucket=None):
    """lshrs_join_rowmap_i64 into a workspace of 64 bytes more than it asks for, every byte preset to PAD: (cells (n_rows, nb)
    int32, the bytes behind the cells, err, the workspace on the device)."""
    import torch

    from lshrs_amd import _native

    lib = _native.load()
    nbytes = int(lib.lshrs_join_workspace_bytes(n_rows, nb))
    assert nbytes >= max(16, 4 * n_rows * nb) and nbytes % 16 == 0
    ws = torch.full((nbytes + 64,), PAD, dtype=torch.uint8, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    codes, offsets, members = dev
    _native.check(lib.lshrs_join_rowmap_i64(codes.data_ptr(), offsets.data_ptr(), int(codes.shape[0]), bb, nb, members.data_ptr(),
                                            int(members.shape[0]), n_rows, 1 << 62 if max_bucket is None else max_bucket,
                                            ws.data_ptr(), err.data_ptr(), None), "lshrs_join_rowmap_i64")
    torch.cuda.synchronize()
    raw = ws.cpu().numpy()
    return raw[:4 * n_rows * nb].view(np.int32).reshape(n_rows, nb), raw[4 * n_rows * nb:], int(err.item()), ws


def _emit(dev, prefix_dev, n_codes, n_rows, nb, ws, begin, count, need, capacity, outs, total):
    """One lshrs_join_emit_i64 launch; `outs`: (a, b, hits) device tensors, or None for three null pointers."""
    import torch

    from lshrs_amd import _native

    ptrs = (None, None, None) if outs is None else tuple(t.data_ptr() for t in outs)
    status = _native.load().lshrs_join_emit_i64(dev[1].data_ptr(), prefix_dev.data_ptr(), n_codes, dev[2].data_ptr(), n_rows, nb,
                                                ws.data_ptr(), int(begin), int(count), need, capacity, *ptrs, total.data_ptr(), None)
    torch.cuda.synchronize()
    return status


def _outputs(capacity, slack=4096):
    import torch

    return (torch.full((capacity + slack,), CANARY, dtype=torch.int64, device="cuda"),
            torch.full((capacity + slack,), CANARY, dtype=torch.int64, device="cuda"),
            torch.full((capacity + slack,), CANARY32, dtype=torch.int32, device="cuda"))


def _untouched(outs, start):
    a, b, hits = (t[start:].cpu().numpy() for t in outs)
    return bool(np.all(a == CANARY) and np.all(b == CANARY) and np.all(hits == CANARY32))


def _slots(outs, n):
    a, b, hits = (t[:n].cpu().numpy().tolist() for t in outs)
    return list(zip(a, b, hits))


# ---------------------------------------------------------------------------------------------------- 1. the row map itself
@pytest.mark.parametrize("max_bucket", (None, 64))
@pytest.mark.parametrize("nb, bb", MAP_SHAPES)
def test_the_row_map_cell_by_cell(nb, bb, max_bucket):
    seg, n_rows = _segment(nb, bb)
    lens = set(np.diff(seg.offsets)[seg.bands == 0].tolist())
    assert {63, 64, 65} <= lens and set(PLANTED) <= lens
    want = rowmap_reference(seg, n_rows, nb, bb, max_bucket)
    cells, behind, err, _ = _rowmap(seg, _upload(seg), n_rows, nb, bb, max_bucket)
    assert err == 0
    assert np.array_equal(cells, want)
    assert behind.shape[0] >= 64 and np.all(behind == PAD)
    # (the map says something: rows without a bucket, rows with one, and - with the limit - the planted 65 left out)
    assert (want == -1).any() and (want >= 0).any()
    if max_bucket is not None:
        assert (rowmap_reference(seg, n_rows, nb, bb) != want).sum() >= 65 + 129 + 300


N_HAND, NB_HAND = 48, 3
HAND = {0x001: [0, 1, 2, 3], 0x002: [4, 5], 0x003: [6], 0x004: [7, 8, 9],
        0x101: [0, 5, 9], 0x102: [1, 2], 0x103: [3], 0x1FE: [4, 6, 7, 8],
        0x207: [3, 4, 8, 10, 11], 0x208: [0, 1], 0x2FE: [2, 5]}
# what each cause adds: a member without a row; a row at n_rows (n_rows - 1 beside it is a row like any other); a bucket of
# band num_bands; row 20 in two counted buckets of band 0
CAUSES = {E_MISSING: {0x010: [12, -1, 13]}, E_BEYOND: {0x1F0: [N_HAND - 1, N_HAND, 14]}, E_BAND: {0x3F0: [15, 16]},
          E_TWO: {0x0F0: [20, 21], 0x0F1: [22, 20]}}


def _hand(causes, fill):
    """HAND with the buckets of `causes`; `fill`: 150 buckets of two rows between any two causes (300 members: the offending
    entries then lie in different workgroups of the row map's launch)."""
    buckets = dict(HAND)
    for bit in causes:
        buckets.update(CAUSES[bit])
    n_rows = N_HAND
    if fill:
        for k in range(150):
            buckets[0x020 + k] = [100 + 2 * k, 101 + 2 * k]             # band 0: between 0x010 and 0x0F0
            buckets[0x110 + k] = [101 + 2 * k, 102 + 2 * k]             # band 1: between 0x0F1 and 0x1F0
            buckets[0x210 + k] = [100 + 2 * k, 103 + 2 * k]             # band 2: between 0x1F0 and 0x3F0
        n_rows = 420
        buckets.pop(0x1F0, None)
        if E_BEYOND in causes:
            buckets[0x1F0] = [n_rows - 1, n_rows, 14]
    return hand_segment(buckets), n_rows


ERROR_CASES = (((E_MISSING,), False), ((E_BEYOND,), False), ((E_BAND,), False), ((E_TWO,), False),
               ((E_MISSING, E_BEYOND, E_BAND, E_TWO), True), ((), False), ((), True))


@pytest.mark.parametrize("causes, fill", ERROR_CASES)
def test_the_row_map_error_bits_and_the_map_under_errors(causes, fill):
    seg, n_rows = _hand(causes, fill)
    members = seg.members.tolist()
    if fill and causes:
        at = sorted([members.index(-1), members.index(n_rows), int(seg.offsets[seg.codes.tolist().index(0x3F0)]),
                     max(i for i, m in enumerate(members) if m == 20)])
        assert min(np.diff(at)) > 256, "the offending entries must lie in different workgroups"
    if E_BEYOND in causes:
        assert n_rows - 1 in members
    want = rowmap_reference(seg, n_rows, NB_HAND, 1)
    cells, behind, err, _ = _rowmap(seg, _upload(seg), n_rows, NB_HAND, 1)
    assert err == sum(causes), f"err = {err:#x}"
    if E_TWO in causes:
        codes = seg.codes.tolist()
        two = (codes.index(0x0F0), codes.index(0x0F1))
        assert want[20, 0] == two[0] and cells[20, 0] in two          # (whichever arrived first)
        want[20, 0] = cells[20, 0]
        assert want[21, 0] == two[0] and want[22, 0] == two[1]
    if E_BEYOND in causes:
        assert want[n_rows - 1, 1] == seg.codes.tolist().index(0x1F0) == want[14, 1]
    if E_MISSING in causes:
        assert want[12, 0] == want[13, 0] == seg.codes.tolist().index(0x010)
    assert np.array_equal(cells, want)
    assert behind.shape[0] >= 64 and np.all(behind == PAD)


@pytest.mark.parametrize("causes, error, message", (
    ((E_MISSING,), IndexError, "NO_VECTOR_MSG"), ((E_BEYOND,), IndexError, "OUT_OF_RANGE_MSG"),
    ((E_BAND,), ValueError, "outside the index"), ((E_TWO,), ValueError, "two signatures"),
    ((E_MISSING, E_BEYOND, E_BAND, E_TWO), IndexError, "NO_VECTOR_MSG"),
    ((E_BEYOND, E_BAND, E_TWO), IndexError, "OUT_OF_RANGE_MSG"),
    ((E_BAND, E_TWO), ValueError, "outside the index"),
    ((E_MISSING, E_TWO), IndexError, "NO_VECTOR_MSG"), ((E_BEYOND, E_TWO), IndexError, "OUT_OF_RANGE_MSG")))
def test_the_error_bits_refuse_by_message_in_their_order(causes, error, message):
    from lshrs_amd import _join
    from lshrs_amd.vectors import NO_VECTOR_MSG

    text = {"NO_VECTOR_MSG": NO_VECTOR_MSG, "OUT_OF_RANGE_MSG": _join.OUT_OF_RANGE_MSG}.get(message, message)
    seg, n_rows = _hand(causes, False)
    with pytest.raises(error, match=re.escape(text)):
        _join.lsh_pairs(*_upload(seg), n_rows, NB_HAND, 1, capacity=64)
    # ... and the same segment without a cause is joined
    seg, n_rows = _hand((), False)
    assert _run(seg, n_rows, NB_HAND, 1)[0] == join_reference([seg])[0]


# ---------------------------------------------------------------------------------- 2. the emit at every width of its loads
@pytest.mark.parametrize("nb, bb", ((2, 1), (6, 2), (10, 1), (4, 1), (7, 3), (12, 4)))
def test_the_emit_at_every_map_width(nb, bb):
    """num_bands % 4 == 2 (8-byte loads of the map), beside one more shape of each other width."""
    seg, n_rows = _segment(nb, bb)
    want, stats = join_reference([seg])
    got, raw = _run(seg, n_rows, nb, bb)
    assert got == want and raw == stats["raw_pairs"]
    assert max(want.values()) == nb and sum(1 for c in want.values() if c == nb) >= 1
    assert sum(1 for c in want.values() if c > 1) > 1
    for need in (2, nb):
        want = join_reference([seg], min_collisions=need)[0]
        assert _run(seg, n_rows, nb, bb, min_collisions=need)[0] == want and len(want) >= 1


# ------------------------------------------------------------------------- 3. large triangular indices through raw_begin
L = 100_003
WINDOW = 4099


@functools.lru_cache(maxsize=None)
def _large():
    """One segment of two bands over L + 5 rows.  Band 1 is ONE bucket of L members (about 5.0e9 raw pairs, more than 2^32),
    the member rows a permutation of the rows without five of them.  Band 0, listed first, splits those members into two
    buckets of L // 2 and L - L // 2: a pair of the band-1 bucket whose entries lie in the same half collides in band 0
    first and must not leave from band 1; a pair across the halves leaves with one collision.  The halves are drawn at
    random over the ENTRIES of the band-1 bucket - not its first L // 2 entries: a window of raw pairs spans a few values of
    j at most, and with a contiguous half every window below j = L // 2 would hold pairs of one kind only."""
    import torch

    rng = np.random.default_rng(20260)
    n_rows = L + 5
    rows = rng.permutation(n_rows)[:L].astype(np.int64)
    first = np.zeros(L, dtype=bool)
    first[rng.choice(L, size=L // 2, replace=False)] = True
    seg = hand_segment({0x001: rows[first], 0x002: rows[~first], 0x101: rows})
    assert seg.offsets.tolist() == [0, L // 2, L, 2 * L] and seg.members.dtype == np.int64
    prefix = _prefix(seg)
    assert prefix[3] - prefix[2] == L * (L - 1) // 2 > 1 << 32 and prefix[1] == (L // 2) * (L // 2 - 1) // 2 > 1 << 24
    dev = _upload(seg)
    cells, behind, err, ws = _rowmap(seg, dev, n_rows, 2, 1)
    want = np.full((n_rows, 2), -1, dtype=np.int32)
    want[rows[first], 0], want[rows[~first], 0], want[rows, 1] = 0, 1, 2
    assert err == 0 and np.array_equal(cells, want) and np.all(behind == PAD)
    assert 0.4 < float((rows[:-1] > rows[1:]).mean()) < 0.6
    return {"seg": seg, "rows": rows, "first": first, "prefix": prefix, "dev": dev, "ws": ws, "n_rows": n_rows,
            "prefix_dev": torch.from_numpy(prefix).cuda()}


def _window(big, bucket, t0, need=1):
    """The raw pairs [t0, t0 + WINDOW) of `bucket` in one launch: (set of (a, b, collisions), total)."""
    import torch

    outs = _outputs(WINDOW, slack=64)
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    begin = int(big["prefix"][bucket]) + t0
    assert big["prefix"][bucket] <= begin and begin + WINDOW <= big["prefix"][bucket + 1]
    assert _emit(big["dev"], big["prefix_dev"], 3, big["n_rows"], 2, big["ws"], begin, WINDOW, need, WINDOW, outs, total) == 0
    n = int(total.item())
    assert 0 <= n <= WINDOW and _untouched(outs, n)
    got = _slots(outs, n)
    assert len(set(got)) == n, "a pair came out twice"
    return set(got), n


def _band1_windows():
    count = L * (L - 1) // 2
    yield "first", 0
    for name, centre in (("2^24", 1 << 24), ("2^31", 1 << 31), ("2^32", 1 << 32)):
        yield name, centre - WINDOW // 2
    for j in (4097, 65536, 92682, 92683, L - 1):
        yield f"j={j}", j * (j - 1) // 2 - WINDOW // 2
    yield "last", count - WINDOW


BAND1_WINDOWS = tuple(_band1_windows())


@pytest.mark.parametrize("name, t0", BAND1_WINDOWS, ids=[w[0] for w in BAND1_WINDOWS])
def test_raw_pairs_beyond_a_float_and_beyond_32_bits(name, t0):
    big = _large()
    rows, first = big["rows"], big["first"]
    assert 0 <= t0 and t0 + WINDOW <= L * (L - 1) // 2
    want, same = set(), 0
    for t in range(t0, t0 + WINDOW):
        i, j = pair_of(t)
        assert j < L
        if first[i] == first[j]:
            same += 1                                   # (collides in band 0 first: it leaves from there, not from here)
        else:
            want.add((int(min(rows[i], rows[j])), int(max(rows[i], rows[j])), 1))
    assert same > 100 and len(want) > 100 and same + len(want) == WINDOW, "the window must hold pairs of both kinds"
    got, total = _window(big, 2, t0)
    assert total == len(want)
    assert got == want
    # two collisions and more: nothing of this bucket leaves
    assert _window(big, 2, t0, need=2) == (set(), 0)


def test_a_bucket_whose_pairs_all_leave_past_2_24():
    big = _large()
    mine = big["rows"][big["first"]]
    t0 = (1 << 24) - WINDOW // 2
    want = set()
    for t in range(t0, t0 + WINDOW):
        i, j = pair_of(t)
        want.add((int(min(mine[i], mine[j])), int(max(mine[i], mine[j])), 2))
    assert len(want) == WINDOW
    for need in (1, 2):
        got, total = _window(big, 0, t0, need=need)
        assert total == WINDOW and got == want


# ------------------------------------------------------------------- 4. capacity, the cursor and the count-only launch
@functools.lru_cache(maxsize=None)
def _small():
    import torch

    seg, n_rows = _segment(3, 1)
    want, stats = join_reference([seg])
    prefix = _prefix(seg)
    assert prefix[-1] == stats["raw_pairs"] and len(want) > 1000
    dev = _upload(seg)
    cells, _, err, ws = _rowmap(seg, dev, n_rows, 3, 1)
    assert err == 0
    return {"dev": dev, "prefix": prefix, "prefix_dev": torch.from_numpy(prefix).cuda(), "ws": ws, "n_rows": n_rows,
            "want": {(a, b, c) for (a, b), c in want.items()}, "n_codes": int(seg.codes.shape[0])}


def _emit_small(s, begin, count, capacity, outs, total):
    return _emit(s["dev"], s["prefix_dev"], s["n_codes"], s["n_rows"], 3, s["ws"], begin, count, 1, capacity, outs, total)


def test_nothing_is_stored_at_or_behind_the_capacity():
    import torch

    s = _small()
    outs = _outputs(1000)
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert _emit_small(s, 0, int(s["prefix"][-1]), 1000, outs, total) == 0
    assert int(total.item()) == len(s["want"])
    got = _slots(outs, 1000)
    assert len(set(got)) == 1000 and set(got) <= s["want"]
    assert _untouched(outs, 1000)


def test_the_count_only_launch():
    import torch

    s = _small()
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert _emit_small(s, 0, int(s["prefix"][-1]), 0, None, total) == 0
    assert int(total.item()) == len(s["want"])


def test_a_total_that_is_not_reset_continues_behind_the_first_launch():
    import torch

    s = _small()
    raw, n = int(s["prefix"][-1]), len(s["want"])
    outs = _outputs(n, slack=64)
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    half = raw // 2 + 1
    assert _emit_small(s, 0, half, n, outs, total) == 0
    n_first = int(total.item())
    first = _slots(outs, n_first)
    assert 0 < n_first < n and set(first) <= s["want"] and len(set(first)) == n_first and _untouched(outs, n_first)
    assert _emit_small(s, half, raw - half, n, outs, total) == 0
    assert int(total.item()) == n
    both = _slots(outs, n)
    assert both[:n_first] == first, "the second launch wrote into the first one's slots"
    assert len(set(both)) == n and set(both) == s["want"] and _untouched(outs, n)
