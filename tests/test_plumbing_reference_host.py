"""The references of tests/_plumbing_reference.py against independent statements of the same operations, and the argument
checks of the plumbing entry points that return before anything touches a device.  CPU only - no kernel is launched here:
every call below is one the library answers from its arguments alone, so the pointers it is handed (small integers that
are nobody's memory) are never dereferenced."""

from __future__ import annotations

import numpy as np
import pytest

from tests import _plumbing_reference as R

P = 0x1000                 # a non-NULL, 8-byte aligned "pointer" no path below reads through
E_BADARG, E_TOOLARGE = -10001, -10002


@pytest.fixture(scope="module")
def lib():
    from lshrs_amd import _native

    _native.build()
    assert (_native.E_BADARG, _native.E_TOOLARGE) == (E_BADARG, E_TOOLARGE)
    return _native.load()


# ------------------------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------------------------

def test_hex_reference_is_bytes_hex():
    every = np.arange(256, dtype=np.uint8)
    assert R.hex_reference(every).tobytes() == every.tobytes().hex().encode()
    rng = np.random.default_rng(1)
    for n in (0, 1, 15, 16, 17, 4097):
        keys = rng.integers(0, 256, size=n, dtype=np.uint8)
        assert R.hex_reference(keys).tobytes() == keys.tobytes().hex().encode()
    keys = rng.integers(0, 256, size=(5, 3, 2), dtype=np.uint8)             # any shape: the bytes in memory order
    assert R.hex_reference(keys).tobytes() == keys.tobytes().hex().encode()
    assert R.hex_reference(np.array([0x0A, 0xF0], np.uint8)).tobytes() == b"0af0"      # high nibble first, lower case


@pytest.mark.parametrize("nb,bb", [(1, 1), (5, 1), (3, 2)])
def test_bucket_reference_is_a_loop_over_rows_and_bands(nb, bb):
    rng = np.random.default_rng(10 * nb + bb)
    n = 300
    keys = rng.integers(0, 7 if bb == 1 else 256, size=(n, nb, bb), dtype=np.uint8)
    if bb == 2:
        keys[:, :, 1] = rng.integers(0, 2, size=(n, nb), dtype=np.uint8) * 255      # few distinct keys, both bytes in play
        keys[:, :, 0] &= 3
    ids = rng.integers(0, 1 << 62, size=n, dtype=np.int64)
    ids[17] = ids[3]                                                        # one id on two rows
    counts, members = R.bucket_reference(keys, ids)
    want = {}
    for row in range(n):
        for band in range(nb):
            key = int.from_bytes(keys[row, band].tobytes(), "little")
            want.setdefault((band << (8 * bb)) | key, []).append(int(ids[row]))
    assert members == {b: sorted(v) for b, v in want.items()}
    assert counts.dtype == np.int32 and counts.shape == (nb << (8 * bb),)
    flat = [b for b, v in want.items() for _ in v]
    assert np.array_equal(counts, np.bincount(flat, minlength=nb << (8 * bb)))
    assert int(counts.sum()) == n * nb and set(members) == set(np.flatnonzero(counts).tolist())


def test_bucket_reference_tells_the_two_byte_orders_apart():
    keys = np.array([[[0xFF, 0x00]], [[0x00, 0xFF]], [[0xFF, 0x00]]], dtype=np.uint8)     # 0x00ff, 0xff00, 0x00ff
    counts, members = R.bucket_reference(keys, np.array([5, 6, 7], np.int64))
    assert members == {0x00FF: [5, 7], 0xFF00: [6]}
    assert counts[0x00FF] == 2 and counts[0xFF00] == 1 and counts.sum() == 3
    keys = np.repeat(keys, 2, axis=1)                                       # band 1: the same keys, 65536 bins further on
    _, members = R.bucket_reference(keys, np.array([5, 6, 7], np.int64))
    assert members == {0x00FF: [5, 7], 0xFF00: [6], 0x100FF: [5, 7], 0x1FF00: [6]}


def test_rank_model_is_sorted_with_the_headers_key():
    neg_nan = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]
    scores = np.array([0.0, np.nan, -0.0, np.inf, 1.0, -np.inf, neg_nan, -0.0, 1.0, 0.0, -1.0, np.inf], dtype=np.float32)

    def klass(p):          # spelled out score by score: what stands ahead of what
        v = scores[p]
        if np.isnan(v):
            return 6
        if v == np.inf:
            return 0
        if v == -np.inf:
            return 5
        if v > 0:
            return 1
        if v < 0:
            return 4
        return 3 if np.signbit(v) else 2

    want = sorted(range(len(scores)), key=lambda p: (klass(p), p))          # (one value per class here: position decides the rest)
    assert want == [3, 11, 4, 8, 0, 9, 2, 7, 10, 5, 1, 6]
    assert R.rank_model(scores) == want
    assert R.rank_model(np.array([1.0, 2.0, 1.0, 2.0], np.float32)) == [1, 3, 0, 2]
    assert R.rank_model(np.array([], np.float32)) == []
    # on data without NaN and with one kind of zero it is the stable descending argsort
    rng = np.random.default_rng(3)
    s = (rng.integers(-6, 7, size=500) / 4.0).astype(np.float32)
    assert R.rank_model(s) == np.argsort(-s, kind="stable").tolist()


def test_special_scores_hold_what_they_promise():
    rng = np.random.default_rng(4)
    for n in (0, 1, 2, 3, 7, 8, 100):
        s = R.special_scores(rng, n)
        assert s.dtype == np.float32 and s.shape == (n,)
        if n >= 7:
            assert np.isnan(s).sum() == 3 and np.isposinf(s).sum() == 1 and np.isneginf(s).sum() == 1
            assert (R.bits(s) == R.bits(np.array([0xFFC00001], np.uint32).view(np.float32))[0]).sum() == 1
            zeros = np.flatnonzero(s == 0.0)
            neg = [p for p in zeros if np.signbit(s[p])]
            pos = [p for p in zeros if not np.signbit(s[p])]
            assert neg and pos and min(neg) < max(pos)                      # a -0.0 ahead of a +0.0


def test_gather_and_scatter_references_are_loops():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((11, 9)).astype(np.float32)
    rows = [10, 0, 3, 3, 10]
    got = R.gather_reference(x, 6, rows)
    assert got.shape == (5, 6) and got.flags.c_contiguous
    for t, r in enumerate(rows):
        for k in range(6):
            assert got[t, k] == x[r, k]
    tie_list = np.array([[(r << 16) | w, m] for r, w, m in [(10, 0, 1), (0, 65535, 0xFFFFFFFF), (3, 1, 1 << 31), (7, 0, 0)]],
                        dtype=np.int64).reshape(-1)
    for count, cap, want in [(0, 4, []), (1, 4, [10]), (3, 4, [10, 0, 3]), (4, 4, [10, 0, 3, 7]), (9, 4, [10, 0, 3, 7]),
                             (9, 2, [10, 0])]:
        r, d = R.tied_rows_reference(x, 9, tie_list, count, cap)
        assert r.tolist() == want and np.array_equal(d, x[want].reshape(len(want), 9))
    keys = rng.integers(0, 256, size=(6, 4, 3), dtype=np.uint8)
    prows, pbands = [5, 0, 5], [0, 3, 1]
    patch = rng.integers(0, 256, size=(3, 3), dtype=np.uint8)
    got = R.scatter_keys_reference(keys, prows, pbands, patch)
    want = keys.copy()
    for t in range(3):
        for j in range(3):
            want[prows[t], pbands[t], j] = patch[t, j]
    assert np.array_equal(got, want) and not np.array_equal(got, keys)


def test_l2_reference_and_tolerance():
    x = np.array([[3.0, 4.0, 0.0], [1e-3, 0.0, 0.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    ref = R.l2_reference(x)
    assert ref.dtype == np.float64
    assert np.allclose(ref[0], [0.6, 0.8, 0.0], rtol=0, atol=1e-16) and ref[1].tolist() == [1.0, 0.0, 0.0]
    assert np.all(np.isnan(ref[2]))
    rng = np.random.default_rng(6)
    x = rng.standard_normal((4, 1000)).astype(np.float32)
    import math
    for row, r in zip(x, R.l2_reference(x)):
        norm = math.sqrt(math.fsum(float(v) * float(v) for v in row))       # exactly rounded sum, one row at a time
        assert np.allclose(r, row.astype(np.float64) / norm, rtol=1e-14, atol=0)
    u = 2.0 ** -24
    assert [R.l2_tolerance(d) / u for d in (1, 3, 255, 256, 257, 512, 513, 1000)] == [9.0, 9.0, 9.0, 9.0, 9.5, 9.5, 10.0, 10.5]


# ------------------------------------------------------------------------------------------------------------------
# guarded(): on the CPU the same views, so the helper itself is checked where no GPU is
# ------------------------------------------------------------------------------------------------------------------

def test_guarded_views_and_their_guards():
    import torch

    cpu = torch.device("cpu")
    v = R.guarded(torch, (3, 5), torch.float32, device=cpu)
    assert v.shape == (3, 5) and v.dtype == torch.float32 and v.is_contiguous()
    assert np.all(R.bits(v.numpy()) == R.FILL_I32)
    assert R.guards_intact(v)
    v.zero_()
    assert R.guards_intact(v)
    base = v.guard_buffer
    base[R.GUARD_BYTES - 1] = 0                                             # the byte in front
    assert not R.guards_intact(v)
    base[R.GUARD_BYTES - 1] = R.GUARD_FILL
    base[R.GUARD_BYTES + 60] = 0                                            # the byte behind
    assert not R.guards_intact(v)
    base[R.GUARD_BYTES + 60] = R.GUARD_FILL
    assert R.guards_intact(v)
    odd = R.guarded(torch, 10, offset=1, device=cpu)
    assert odd.data_ptr() % 2 == 1 and odd.dtype == torch.uint8 and odd.shape == (10,)
    odd.guard_buffer[R.GUARD_BYTES] = 0                                            # the slack in front of an offset view is guard too
    assert not R.guards_intact(odd)
    R.fill_guarded(torch, odd, np.arange(10, dtype=np.uint8))
    assert odd.numpy().tolist() == list(range(10))
    with pytest.raises(AssertionError):
        R.guarded(torch, 4, torch.float32, offset=2, device=cpu)


# ------------------------------------------------------------------------------------------------------------------
# argument checks that return before anything touches a device
# ------------------------------------------------------------------------------------------------------------------

def test_size_zero_is_done_even_with_null_pointers(lib):
    assert lib.lshrs_gather_rows_f32(None, 0, 0, None, 0, None, None) == 0                              # m
    assert lib.lshrs_gather_tied_rows_f32(None, 0, 0, None, None, 0, None, None) == 0                   # tie_cap
    assert lib.lshrs_scatter_band_keys_u8(None, 0, 0, None, None, None, 0, None) == 0                   # m
    assert lib.lshrs_keys_to_hex_u8(None, 0, None, None) == 0                                           # nbytes
    assert lib.lshrs_bucket_histogram_u8(None, 0, 0, 0, None, None) == 0                                # n
    assert lib.lshrs_bucket_scatter_u8(None, None, 0, 0, 0, None, None, None, None) == 0                # n
    assert lib.lshrs_l2_normalize_f32(None, 0, 0, 0, None, None, None) == 0                             # n
    assert lib.lshrs_topk_desc_f32(None, 0, 5, 3, None, None, None, None) == 0                          # q
    assert lib.lshrs_topk_desc_f32(None, 2, 5, 0, None, None, None, None) == 0                          # k


def test_gathers_refuse_bad_arguments(lib):
    g = lib.lshrs_gather_rows_f32                  # (X, ldx, dim, rows, m, dst, stream)
    assert g(None, 8, 8, P, 1, P, None) == E_BADARG
    assert g(P, 8, 8, None, 1, P, None) == E_BADARG
    assert g(P, 8, 8, P, 1, None, None) == E_BADARG
    assert g(P, 7, 8, P, 1, P, None) == E_BADARG                            # ldx < dim
    assert g(P, 8, 0, P, 1, P, None) == E_BADARG
    assert g(P, 8, 8, P, -1, P, None) == E_BADARG
    assert g(P, 8, 8, P, 1 << 31, P, None) == E_TOOLARGE                    # m > 2^31 - 1
    assert g(P, 8, 8, P, 1 << 40, P, None) == E_TOOLARGE
    t = lib.lshrs_gather_tied_rows_f32             # (X, ldx, dim, tie_list, tie_count, tie_cap, dst, stream)
    assert t(None, 8, 8, P, P, 4, P, None) == E_BADARG
    assert t(P, 8, 8, None, P, 4, P, None) == E_BADARG
    assert t(P, 8, 8, P, None, 4, P, None) == E_BADARG
    assert t(P, 8, 8, P, P, 4, None, None) == E_BADARG
    assert t(P, 7, 8, P, P, 4, P, None) == E_BADARG                         # ldx < dim
    assert t(P, 8, 0, P, P, 4, P, None) == E_BADARG
    assert t(P, 8, 8, P, P, -4, P, None) == E_BADARG


def test_key_patch_and_hex_refuse_bad_arguments(lib):
    s = lib.lshrs_scatter_band_keys_u8             # (keys, num_bands, band_bytes, rows, bands, patch, m, stream)
    assert s(None, 4, 2, P, P, P, 3, None) == E_BADARG
    assert s(P, 4, 2, None, P, P, 3, None) == E_BADARG
    assert s(P, 4, 2, P, None, P, 3, None) == E_BADARG
    assert s(P, 4, 2, P, P, None, 3, None) == E_BADARG
    assert s(P, 0, 2, P, P, P, 3, None) == E_BADARG
    assert s(P, 4, 0, P, P, P, 3, None) == E_BADARG
    assert s(P, 4, 2, P, P, P, -3, None) == E_BADARG
    h = lib.lshrs_keys_to_hex_u8                   # (keys, nbytes, hex, stream)
    assert h(None, 16, P, None) == E_BADARG
    assert h(P, 16, None, None) == E_BADARG
    assert h(P, -16, P, None) == E_BADARG


def test_bucket_calls_refuse_bad_arguments(lib):
    h = lib.lshrs_bucket_histogram_u8              # (keys, n, num_bands, band_bytes, counts, stream)
    assert h(None, 10, 4, 1, P, None) == E_BADARG
    assert h(P, 10, 4, 1, None, None) == E_BADARG
    assert h(P, -10, 4, 1, P, None) == E_BADARG
    assert h(P, 10, 0, 1, P, None) == E_BADARG
    assert h(P, 10, 4, 0, P, None) == E_TOOLARGE
    assert h(P, 10, 4, 3, P, None) == E_TOOLARGE
    assert h(P, 10, 32769, 1, P, None) == E_TOOLARGE
    assert h(P, 10, 32769, 2, P, None) == E_TOOLARGE
    s = lib.lshrs_bucket_scatter_u8                # (keys, ids, n, num_bands, band_bytes, offsets, cursors, members, stream)
    for hole in range(5):
        ptrs = [P] * 5
        ptrs[hole] = None
        keys, ids, offsets, cursors, members = ptrs
        assert s(keys, ids, 10, 4, 1, offsets, cursors, members, None) == E_BADARG, hole
    assert s(P, P, -10, 4, 1, P, P, P, None) == E_BADARG
    assert s(P, P, 10, 0, 1, P, P, P, None) == E_BADARG
    assert s(P, P, 10, 4, 0, P, P, P, None) == E_TOOLARGE
    assert s(P, P, 10, 4, 3, P, P, P, None) == E_TOOLARGE
    assert s(P, P, 10, 32769, 1, P, P, P, None) == E_TOOLARGE
    assert s(P, P, 10, 32769, 2, P, P, P, None) == E_TOOLARGE


def test_l2_normalize_refuses_bad_arguments(lib):
    n = lib.lshrs_l2_normalize_f32                 # (X, n, ldx, dim, out, status, stream)
    assert n(None, 3, 8, 8, P, None, None) == E_BADARG
    assert n(P, 3, 8, 8, None, None, None) == E_BADARG
    assert n(P, 3, 7, 8, P, P, None) == E_BADARG                            # ldx < dim
    assert n(P, 3, 8, 0, P, P, None) == E_BADARG
    assert n(P, -3, 8, 8, P, P, None) == E_BADARG
    assert n(P, 1 << 31, 8, 8, P, P, None) == E_TOOLARGE


def test_topk_refuses_bad_arguments_and_sizes_its_workspace(lib):
    t = lib.lshrs_topk_desc_f32                    # (scores, q, c, k, order, sorted, workspace, stream)
    assert t(None, 1, 5, 3, P, P, None, None) == E_BADARG
    assert t(P, 1, 5, 3, None, P, None, None) == E_BADARG
    assert t(P, 1, 5, 3, P, None, None, None) == E_BADARG
    assert t(P, 1, 5, 6, P, P, None, None) == E_BADARG                      # k > c
    assert t(P, 1, 16384, 16385, P, P, None, None) == E_BADARG
    assert t(P, 1, 0, 1, P, P, None, None) == E_BADARG                      # c <= 0
    assert t(P, 1, -5, -6, P, P, None, None) == E_BADARG
    assert t(P, -1, 5, 3, P, P, None, None) == E_BADARG
    assert t(P, 1, 5, -3, P, P, None, None) == E_BADARG
    assert t(P, 1, 16385, 3, P, P, None, None) == E_BADARG                  # the global path needs its workspace ...
    assert t(P, 1, 16385, 3, P, P, P + 4, None) == E_BADARG                 # ... 8-byte aligned
    assert t(P, 1, 16385, 3, P, P, P + 1, None) == E_BADARG
    assert t(P, 65536, 16385, 3, P, P, P, None) == E_TOOLARGE               # q <= 65535 there
    w = lib.lshrs_topk_workspace_bytes
    for q in (1, 3, 65535):
        assert w(q, 1) == 0 and w(q, 16384) == 0
        assert w(q, 16385) == q * 32768 * 8 == w(q, 32768)
        assert w(q, 32769) == q * 65536 * 8
    assert w(0, 16385) == 0
    assert w(-1, 5) == E_BADARG and w(1, -5) == E_BADARG
