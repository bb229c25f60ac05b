"""Host side of the LSH self-join (lshrs_amd.lsh_pairs_above, lshrs_join_*): the exports and where they are declared, the
workspace's size, the C entries' argument checks, what the Python layers decide before any GPU call, the plain-Python
reference on a case written by hand (the pairs, the row map, the triangular index), and the shared collision law.  No GPU."""

from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

from tests._join_reference import hand_segment, join_reference, pair_of, rowmap_reference

JOIN_EXPORTS = ("lshrs_join_workspace_bytes", "lshrs_join_rowmap_i64", "lshrs_join_emit_i64")


def _lib():
    from lshrs_amd import _native

    _native.build()
    return _native.load()


def _no_gpu(monkeypatch):
    from lshrs_amd import _native

    def no_gpu():
        raise AssertionError("the GPU was asked for")

    monkeypatch.setattr(_native, "require_gpu", no_gpu)
    monkeypatch.setattr(_native, "load", no_gpu)


def test_names_are_exported():
    import lshrs_amd
    from lshrs_amd import DeviceVectors, LSHRS, _exact, _join, _native

    assert callable(lshrs_amd.lsh_pairs_above) and "lsh_pairs_above" in lshrs_amd.__all__
    assert callable(_join.lsh_pairs) and "lsh_pairs" in _join.__all__ and "lsh_pairs_above" in _join.__all__
    assert callable(LSHRS.pairs_above) and callable(LSHRS.recall_pairs_above) and callable(DeviceVectors.lsh_pairs_above)
    assert callable(_exact._judge_pairs) and callable(_exact.collision_law)
    assert _native.UNITS[-1] == "join" and os.path.exists(os.path.join(_native.CSRC, "join.hip"))


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lshrs_[a-z0-9_]+)\s*\(", text)))


def test_the_three_entries_are_in_their_header_their_tuple_and_the_library():
    from lshrs_amd import _native

    lib = _lib()
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _native.LIBRARY], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (lshrs_\w+)", dynamic))
    assert _declared(os.path.join(_native.INCLUDE, "lshrs_join.h")) == sorted(JOIN_EXPORTS) == sorted(_native.EXPORTS_JOIN)
    assert '#include "lshrs_hip.h"' in open(os.path.join(_native.INCLUDE, "lshrs_join.h")).read()
    for name in JOIN_EXPORTS:
        assert name in exported and hasattr(lib, name), name
        assert name not in _native.EXPORTS and name not in _native.EXPORTS_KNN
    # the first two headers and their tuples are what they were
    assert _declared(os.path.join(_native.INCLUDE, "lshrs_hip.h")) == sorted(_native.EXPORTS)
    assert _declared(os.path.join(_native.INCLUDE, "lshrs_knn.h")) == sorted(_native.EXPORTS_KNN)
    assert len(_native.EXPORTS) == 75 == len(set(_native.EXPORTS)) and len(set(_native.EXPORTS_KNN)) == 6
    assert len(set(_native.EXPORTS_JOIN)) == 3
    assert exported == set(_native.EXPORTS) | set(_native.EXPORTS_KNN) | set(_native.EXPORTS_JOIN)
    assert lib.lshrs_abi_version() == 7 == _native.ABI_VERSION


def test_workspace_bytes():
    from lshrs_amd import _native

    size = _lib().lshrs_join_workspace_bytes
    # an int32 per (row, band), rounded up to 16 bytes, never nothing
    assert size(1000, 16) == 64000 and size(3, 33) == 400 and size(1, 1) == 16 and size(5, 1) == 32 and size(0, 7) == 16
    assert size(200000, 16) == 200000 * 16 * 4
    assert size(-1, 16) == _native.E_BADARG and size(10, 0) == _native.E_BADARG and size(10, -2) == _native.E_BADARG
    assert size((1 << 31) - 1, 1) > 0 and size(1 << 31, 1) == _native.E_TOOLARGE
    assert size(1 << 30, 1024) > 0 and size(1 << 30, 1025) == _native.E_TOOLARGE        # (2^40 cells)


def test_c_entries_check_their_arguments_on_the_host():
    """Status codes of lshrs_join_*, decided before anything touches a device (there is none here)."""
    from lshrs_amd import _native

    lib = _lib()
    buf = np.zeros(80, dtype=np.int64)
    p = (buf.ctypes.data + 15) // 16 * 16              # (16-byte aligned, with room behind it)
    bad, big = _native.E_BADARG, _native.E_TOOLARGE
    fn = lib.lshrs_join_rowmap_i64
    #        codes offsets n_codes band_bytes num_bands member_rows n_members n_rows max_bucket workspace err stream
    assert fn(p, p, -1, 2, 16, p, 10, 10, 64, p, p, None) == bad
    assert fn(p, p, 5, 0, 16, p, 10, 10, 64, p, p, None) == bad               # band_bytes outside 1..6
    assert fn(p, p, 5, 7, 16, p, 10, 10, 64, p, p, None) == bad
    assert fn(p, p, 5, 2, 0, p, 10, 10, 64, p, p, None) == bad                # num_bands < 1
    assert fn(p, p, 5, 2, 16, p, -1, 10, 64, p, p, None) == bad               # negative sizes
    assert fn(p, p, 5, 2, 16, p, 10, -1, 64, p, p, None) == bad
    assert fn(p, p, 5, 2, 16, p, 10, 10, 1, p, p, None) == bad                # max_bucket < 2
    assert fn(p, p, 5, 2, 16, p, 10, 10, 0, p, p, None) == bad
    assert fn(None, p, 5, 2, 16, p, 10, 10, 64, p, p, None) == bad            # null pointers
    assert fn(p, None, 5, 2, 16, p, 10, 10, 64, p, p, None) == bad
    assert fn(p, p, 5, 2, 16, None, 10, 10, 64, p, p, None) == bad
    assert fn(p, p, 5, 2, 16, p, 10, 10, 64, None, p, None) == bad
    assert fn(p, p, 5, 2, 16, p, 10, 10, 64, p, None, None) == bad
    assert fn(p + 4, p, 5, 2, 16, p, 10, 10, 64, p, p, None) == bad           # misaligned
    assert fn(p, p + 4, 5, 2, 16, p, 10, 10, 64, p, p, None) == bad
    assert fn(p, p, 5, 2, 16, p + 4, 10, 10, 64, p, p, None) == bad
    assert fn(p, p, 5, 2, 16, p, 10, 10, 64, p + 8, p, None) == bad
    assert fn(p, p, 5, 2, 16, p, 10, 10, 64, p, p + 2, None) == bad
    assert fn(p, p, 1 << 31, 2, 16, p, 10, 10, 64, p, p, None) == big         # more than 2^31 - 1 buckets
    assert fn(p, p, 5, 2, 16, p, 10, 1 << 31, 64, p, p, None) == big
    assert fn(p, p, 5, 2, 1025, p, 10, 1 << 30, 64, p, p, None) == big
    fn = lib.lshrs_join_emit_i64
    #        offsets prefix n_codes member_rows n_rows num_bands workspace raw_begin raw_count min_coll capacity a b hits total stream
    assert fn(p, p, -1, p, 10, 16, p, 0, 10, 1, 8, p, p, p, p, None) == bad
    assert fn(p, p, 5, p, -1, 16, p, 0, 10, 1, 8, p, p, p, p, None) == bad
    assert fn(p, p, 5, p, 10, 0, p, 0, 10, 1, 8, p, p, p, p, None) == bad                 # num_bands < 1
    assert fn(p, p, 5, p, 10, 16, p, -1, 10, 1, 8, p, p, p, p, None) == bad               # raw_begin < 0
    assert fn(p, p, 5, p, 10, 16, p, 0, -1, 1, 8, p, p, p, p, None) == bad                # raw_count < 0
    assert fn(p, p, 5, p, 10, 16, p, 0, 10, 0, 8, p, p, p, p, None) == bad                # min_collisions outside 1..num_bands
    assert fn(p, p, 5, p, 10, 16, p, 0, 10, 17, 8, p, p, p, p, None) == bad
    assert fn(p, p, 5, p, 10, 16, p, 0, 10, 1, -1, p, p, p, p, None) == bad               # capacity < 0
    assert fn(p, p, 5, p, 10, 16, p, 0, (1 << 31) + 1, 1, 8, p, p, p, p, None) == big     # raw_count > 2^31
    assert fn(p, p, 1 << 31, p, 10, 16, p, 0, 10, 1, 8, p, p, p, p, None) == big
    assert fn(None, p, 5, p, 10, 16, p, 0, 10, 1, 8, p, p, p, p, None) == bad             # null pointers
    assert fn(p, None, 5, p, 10, 16, p, 0, 10, 1, 8, p, p, p, p, None) == bad
    assert fn(p, p, 5, None, 10, 16, p, 0, 10, 1, 8, p, p, p, p, None) == bad
    assert fn(p, p, 5, p, 10, 16, None, 0, 10, 1, 8, p, p, p, p, None) == bad
    assert fn(p, p, 5, p, 10, 16, p, 0, 10, 1, 8, None, p, p, p, None) == bad             # slots, no arrays
    assert fn(p, p, 5, p, 10, 16, p, 0, 10, 1, 8, p, None, p, p, None) == bad
    assert fn(p, p, 5, p, 10, 16, p, 0, 10, 1, 8, p, p, None, p, None) == bad
    assert fn(p, p, 5, p, 10, 16, p, 0, 10, 1, 8, p, p, p, None, None) == bad             # no total
    assert fn(p, p, 5, p, 10, 16, p, 0, 10, 1, 8, p, p, p, p + 4, None) == bad            # misaligned
    assert fn(p, p, 5, p, 10, 16, p + 8, 0, 10, 1, 8, p, p, p, p, None) == bad
    assert fn(p, p, 5, p, 10, 16, p, 0, 10, 1, 8, p + 4, p, p, p, None) == bad
    assert fn(p, p, 5, p, 10, 16, p, 0, 10, 1, 8, p, p, p + 2, p, None) == bad
    # nothing to do: no launch, whatever the arrays are - but the rest is still checked
    assert fn(None, None, 5, None, 10, 16, None, 0, 0, 1, 0, None, None, None, p, None) == 0
    assert fn(None, None, 0, None, 10, 16, None, 0, 10, 1, 0, None, None, None, p, None) == 0
    assert fn(None, None, 5, None, 10, 16, None, 0, 0, 17, 0, None, None, None, p, None) == bad


@pytest.mark.parametrize("kwargs, match", (
    ({"threshold": float("nan")}, "threshold"), ({"threshold": [0.2, 0.3]}, "threshold"), ({"threshold": 1.5}, "threshold"),
    ({"threshold": None}, "threshold"), ({"max_pairs": -1}, "max_pairs"),
    ({"min_collisions": 0}, "min_collisions"), ({"min_collisions": 5}, "min_collisions"), ({"min_collisions": 1.5}, "min_collisions"),
    ({"min_collisions": True}, "min_collisions"), ({"min_collisions": None}, "min_collisions"),
    ({"max_bucket": 1}, "max_bucket"), ({"max_bucket": 0}, "max_bucket"), ({"max_bucket": 2.5}, "max_bucket"),
    ({"max_raw_pairs": -1}, "max_raw_pairs")))
def test_bad_arguments_raise_before_any_gpu_call(kwargs, match, monkeypatch):
    from lshrs_amd import LSHRS, InMemoryStorage, _join

    args = {"threshold": 0.5}
    args.update(kwargs)
    threshold = args.pop("threshold")
    _no_gpu(monkeypatch)
    with pytest.raises(ValueError, match=match):
        _join.lsh_pairs_above(None, threshold, None, None, None, 4, 1, **args)
    if "max_raw_pairs" not in args:
        index = LSHRS(dim=16, num_perm=16, num_bands=4, rows_per_band=4, storage=InMemoryStorage(), keep_vectors="float32")
        with pytest.raises(ValueError, match=match):
            index.pairs_above(threshold, **args)


def test_good_arguments_get_as_far_as_the_gpu(monkeypatch):
    from lshrs_amd import _join

    _no_gpu(monkeypatch)
    for args in ({}, {"min_collisions": 4}, {"min_collisions": np.int64(2), "max_bucket": 2}, {"max_bucket": np.int32(500)},
                 {"max_pairs": 0, "max_raw_pairs": 0}):
        with pytest.raises(AssertionError, match="the GPU was asked for"):
            _join.lsh_pairs_above(None, 0.5, None, None, None, 4, 1, **args)


def test_the_reference_on_a_case_written_by_hand():
    seg = hand_segment

    # band 0: {1, 2, 3} under key 7, {4} under key 9; band 1: {2, 3} under key 1 (3 through the second segment), {1, 4, 5, 6}
    # under key 2
    one = seg({0x007: [1, 2, 3], 0x009: [4], 0x101: [2], 0x102: [1, 4, 5, 6]})
    two = seg({0x101: [3, 2], 0x007: [3]})
    pairs, stats = join_reference([one, two])
    assert pairs == {(1, 2): 1, (1, 3): 1, (2, 3): 2, (1, 4): 1, (1, 5): 1, (1, 6): 1, (4, 5): 1, (4, 6): 1, (5, 6): 1}
    assert stats == {"buckets": 4, "skipped_buckets": 0, "raw_pairs": 3 + 0 + 1 + 6}
    assert join_reference([one, two], min_collisions=2)[0] == {(2, 3): 2}
    pairs, stats = join_reference([one, two], max_bucket=3)
    assert pairs == {(1, 2): 1, (1, 3): 1, (2, 3): 2} and stats["skipped_buckets"] == 1 and stats["raw_pairs"] == 4
    pairs, stats = join_reference([one, two], max_bucket=2)
    assert pairs == {(2, 3): 1} and stats["skipped_buckets"] == 2           # (the oversized bucket is no collision either)
    assert join_reference([], 1) == ({}, {"buckets": 0, "skipped_buckets": 0, "raw_pairs": 0})


def test_the_row_map_reference_on_the_case_written_by_hand():
    # the buckets of the case above as ONE segment (what a fold makes of them), sorted by code: g = 0 .. 3
    seg = hand_segment({0x007: [1, 2, 3], 0x009: [4], 0x101: [2, 3], 0x102: [1, 4, 5, 6]})
    none = [-1, -1]
    assert rowmap_reference(seg, 8, 2, 1).tolist() == [none, [0, 3], [0, 2], [0, 2], [-1, 3], [-1, 3], [-1, 3], none]
    got = rowmap_reference(seg, 8, 2, 1)
    assert got.dtype == np.int32 and got.shape == (8, 2)
    # buckets of more than max_bucket entries count in no role; a bucket of one entry never does
    assert rowmap_reference(seg, 8, 2, 1, max_bucket=3).tolist() == [none, [0, -1], [0, 2], [0, 2], none, none, none, none]
    assert rowmap_reference(seg, 8, 2, 1, max_bucket=2).tolist() == [none, none, [-1, 2], [-1, 2], none, none, none, none]
    # what a valid segment never holds defines no cell: rows outside [0, n_rows), bands outside [0, num_bands)
    assert rowmap_reference(seg, 4, 1, 1).tolist() == [[-1], [0], [0], [0]]
    odd = hand_segment({0x007: [1, -1, 3], 0x008: [3, 2]})
    assert rowmap_reference(odd, 4, 1, 1).tolist() == [[-1], [0], [1], [0]]          # (two buckets of one band: the first)


def _inverts(t):
    i, j = pair_of(t)
    return type(i) is int and type(j) is int and 0 <= i < j and j * (j - 1) // 2 + i == t


def test_pair_of_inverts_the_triangular_index():
    assert [pair_of(t) for t in range(7)] == [(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3), (0, 4)]
    assert all(_inverts(t) for t in range(5000))
    assert sorted(pair_of(t) for t in range(4950)) == [(i, j) for i in range(100) for j in range(i + 1, 100)]
    for centre in (1 << 24, 1 << 31, 1 << 32, 1 << 52):
        assert all(_inverts(t) for t in range(centre - 3, centre + 4)), centre
    for j in (2, 3, 4097, 65536, 92682, 92683, (1 << 26) + 1):
        first = j * (j - 1) // 2
        assert all(_inverts(t) for t in range(max(0, first - 3), first + 4)), j
        assert pair_of(first) == (0, j) and pair_of(first - 1) == (j - 2, j - 1) and pair_of(first + j - 1) == (j - 1, j)
    # (where a float32 and a 32-bit t stop being exact: what the GPU test's windows are placed around)
    assert pair_of(1 << 24)[1] == 5793 and pair_of(1 << 32)[1] == 92682
    with pytest.raises(ValueError):
        pair_of(-1)


def test_folding_segments_is_merge_csr_and_is_timed():
    from lshrs_amd import _join
    from lshrs_amd.packed_ops import _csr_host, merge_csr

    rng = np.random.default_rng(3)
    segs = []
    for _ in range(3):
        keys = rng.integers(0, 5, size=(40, 3, 1)).astype(np.uint8)
        segs.append(_csr_host(rng.choice(60, size=40, replace=False).astype(np.int64), keys))
    one, ms, folded = _join.fold_segments(segs)
    want = merge_csr(segs)
    assert np.array_equal(one.codes, want.codes) and np.array_equal(one.offsets, want.offsets) and ms >= 0.0 and folded == 3
    assert np.array_equal(one.members, want.members) and one.distinct
    assert join_reference([one])[0] == join_reference(segs)[0]
    assert _join.fold_segments(segs[:1]) == (segs[0], 0.0, 0) and _join.fold_segments([]) == (None, 0.0, 0)
    hollow = _csr_host(np.empty(0, np.int64), np.empty((0, 3, 1), np.uint8))
    assert _join.fold_segments([hollow, segs[0], hollow]) == (segs[0], 0.0, 0)          # (empty segments are not counted)
    assert _join.fold_segments([segs[0], hollow, segs[1]])[2] == 2


def test_the_shared_recall_law_is_above_recalls_expected():
    from lshrs_amd._exact import above_recall, collision_law

    rng = np.random.default_rng(5)
    scores = rng.uniform(-1.0, 1.0, size=50).astype(np.float32)
    scores[:3] = (1.0, -1.0, 1.0000001)
    ids = np.arange(50, dtype=np.int64)
    bounds = np.array([0, 20, 50], dtype=np.int64)
    for nb, r in ((16, 16), (4, 2), (128, 1)):
        got = above_recall(ids, scores, bounds, ids[:10], np.array([0, 4, 10]), nb, r)
        assert collision_law(scores, nb, r) == got["expected"]
        p = 1.0 - np.arccos(np.clip(scores.astype(np.float64), -1.0, 1.0)) / np.pi
        assert got["expected"] == float(np.mean(1.0 - (1.0 - p ** r) ** nb))
    assert np.isnan(collision_law(np.empty(0), 16, 16))
    assert np.isnan(above_recall(ids[:0], scores[:0], np.zeros(3, np.int64), ids[:0], np.zeros(3, np.int64), 4, 4)["expected"])
