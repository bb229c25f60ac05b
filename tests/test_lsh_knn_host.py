"""Host side of the LSH k-NN graph (lshrs_amd.lsh_knn, lshrs_graph_*): the names, the third library and what it exports, the C
entries' argument checks, what the Python layers decide before any GPU call, and the plain-Python reference on a segment
written out by hand.  No GPU."""

from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

from tests._join_reference import hand_segment
from tests._knn_join_reference import candidates_reference, desc_key, knn_join_reference, rank_list

GRAPH_EXPORTS = ("lshrs_graph_abi_version", "lshrs_graph_max_list", "lshrs_graph_wave_list", "lshrs_graph_degree_i64",
                 "lshrs_graph_fill_i64", "lshrs_graph_select_f32")


def _lib():
    from lshrs_amd import _native

    _native.build()
    return _native.load_graph()


def _no_gpu(monkeypatch):
    from lshrs_amd import _native

    def no_gpu():
        raise AssertionError("the GPU was asked for")

    for name in ("require_gpu", "load", "load_groups", "load_graph"):
        monkeypatch.setattr(_native, name, no_gpu)


def test_names_are_exported():
    import lshrs_amd
    from lshrs_amd import DeviceVectors, LSHRS, _knn_join, _native

    assert callable(lshrs_amd.lsh_knn) and "lsh_knn" in lshrs_amd.__all__
    for name in ("lsh_knn", "pair_adjacency", "select_neighbors"):
        assert callable(getattr(_knn_join, name)) and name in _knn_join.__all__
    assert callable(DeviceVectors.lsh_neighbors) and callable(LSHRS.neighbors) and callable(LSHRS.recall_neighbors)
    assert os.path.exists(_native.GRAPH_SOURCE) and "graph" not in _native.UNITS
    for doc in (lshrs_amd.lsh_knn.__doc__, LSHRS.neighbors.__doc__):
        doc = " ".join(doc.split())
        assert "restricted to its candidates" in doc.lower() and "bit for bit" in doc and "ascending id" in doc
    assert "OWN ID" in " ".join(LSHRS.recall_neighbors.__doc__.split())


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lshrs_[a-z0-9_]+)\s*\(", text)))


def _exported(path):
    dynamic = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (lshrs_\w+)", dynamic))


def test_the_entries_are_in_their_header_their_tuple_and_their_own_library():
    from lshrs_amd import _native

    lib = _lib()
    path = _native.GRAPH_LIBRARY
    assert os.path.basename(path) == "liblshrs_graph.so" and os.path.dirname(path) == _native.CSRC
    exported = _exported(path)
    header = os.path.join(_native.INCLUDE, "lshrs_graph.h")
    assert _declared(header) == sorted(GRAPH_EXPORTS) == sorted(_native.EXPORTS_GRAPH) == sorted(exported)
    assert len(set(_native.EXPORTS_GRAPH)) == 6
    others = _native.EXPORTS + _native.EXPORTS_KNN + _native.EXPORTS_JOIN + _native.EXPORTS_GROUPS
    for name in GRAPH_EXPORTS:
        assert hasattr(lib, name) and name not in others
    assert lib.lshrs_graph_abi_version() == 1 == _native.GRAPH_ABI_VERSION
    text = open(header).read()
    assert int(re.search(r"#define\s+LSHRS_GRAPH_ABI_VERSION\s+(\d+)", text).group(1)) == 1
    for name, want in (("ENDPOINT", 1), ("LOOP", 2), ("RANGE", 1), ("ENTRY", 2)):
        assert int(re.search(r"#define\s+LSHRS_GRAPH_ERR_" + name + r"\s+(\w+)", text).group(1), 0) == want \
            == getattr(_native, "GRAPH_ERR_" + name)
    # device code for gfx950 inside, and no need of the other two libraries
    assert b"gfx950" in open(path, "rb").read()
    needed = subprocess.run(["readelf", "-d", path], check=True, capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "liblshrs_" not in needed
    undefined = subprocess.run(["nm", "-D", "--undefined-only", path], check=True, capture_output=True, text=True).stdout
    assert not re.search(r"\blshrs_", undefined)
    # the first two libraries export what they exported
    first, second = _exported(_native.LIBRARY), _exported(_native.GROUPS_LIBRARY)
    assert first == set(_native.EXPORTS) | set(_native.EXPORTS_KNN) | set(_native.EXPORTS_JOIN)
    assert second == set(_native.EXPORTS_GROUPS) and len(second) == 4
    assert not (first | second) & exported


def test_the_list_bounds():
    lib = _lib()
    assert lib.lshrs_graph_max_list() >= 4096
    assert 1 <= lib.lshrs_graph_wave_list() <= lib.lshrs_graph_max_list()


def test_the_other_libraries_load_without_the_third(tmp_path, monkeypatch):
    from lshrs_amd import _native

    _lib()
    monkeypatch.setattr(_native, "_graph_lib", None)
    monkeypatch.setattr(_native, "GRAPH_LIBRARY", str(tmp_path / "nope.so"))
    assert _native.load().lshrs_abi_version() == _native.ABI_VERSION
    assert _native.load_groups().lshrs_groups_abi_version() == _native.GROUPS_ABI_VERSION
    with pytest.raises(_native.NativeLibraryError, match="has not been built") as exc:
        _native.load_graph()
    assert "nope.so" in str(exc.value)


def test_a_fresh_library_is_not_rebuilt():
    from lshrs_amd import _native

    _lib()
    deps = _native._sources_of(_native.GRAPH_SOURCE)
    assert {os.path.basename(p) for p in deps} == {"graph.hip", "lshrs_graph.h", "lshrs_hip.h", "lshrs_rows.h", "lshrs_common.h", "lshrs_lists.h"}
    assert os.path.getmtime(_native.GRAPH_LIBRARY) >= max(os.path.getmtime(p) for p in deps)
    before = os.path.getmtime(_native.GRAPH_LIBRARY)
    _native.build()                                             # fresh: nothing is compiled
    assert os.path.getmtime(_native.GRAPH_LIBRARY) == before and not os.path.exists(_native.GRAPH_LIBRARY + ".tmp")


def test_c_entries_check_their_arguments_on_the_host():
    """Status codes of lshrs_graph_*, decided before anything touches a device (there is none here)."""
    from lshrs_amd import _native

    lib = _lib()
    buf = np.zeros(16, dtype=np.int64)
    p = (buf.ctypes.data + 15) // 16 * 16
    bad, big, top = _native.E_BADARG, _native.E_TOOLARGE, (1 << 31) - 1
    degree, fill, select = lib.lshrs_graph_degree_i64, lib.lshrs_graph_fill_i64, lib.lshrs_graph_select_f32
    #             a  b  n_pairs n_rows degree err stream
    assert degree(p, p, -1, 5, p, p, None) == bad and degree(p, p, 3, -1, p, p, None) == bad
    assert degree(None, p, 3, 5, p, p, None) == bad and degree(p, None, 3, 5, p, p, None) == bad
    assert degree(p, p, 3, 5, None, p, None) == bad and degree(p, p, 3, 5, p, None, None) == bad
    assert degree(p + 4, p, 3, 5, p, p, None) == bad and degree(p, p + 4, 3, 5, p, p, None) == bad          # a, b: 8 bytes
    assert degree(p, p, 3, 5, p + 2, p, None) == bad and degree(p, p, 3, 5, p, p + 1, None) == bad          # degree, err: 4
    assert degree(p, p, top + 1, 5, p, p, None) == big and degree(p, p, 3, top + 1, p, p, None) == big
    assert degree(p, p, -1, top + 1, p, p, None) == bad
    assert degree(p, p, 0, 5, p, p, None) == 0 and degree(None, None, 0, 5, None, None, None) == 0
    assert degree(p, p, 3, 0, p, p, None) == 0 and degree(None, None, 3, 0, None, None, None) == 0
    #           a  b  n_pairs n_rows row_off cursor nbr stream
    assert fill(p, p, -1, 5, p, p, p, None) == bad and fill(p, p, 3, -1, p, p, p, None) == bad
    for k in range(5):
        args = [p, p, 3, 5, p, p, p, None]
        args[k if k < 2 else k + 2] = None
        assert fill(*args) == bad, k
    assert fill(p + 4, p, 3, 5, p, p, p, None) == bad and fill(p, p, 3, 5, p + 4, p, p, None) == bad
    assert fill(p, p, 3, 5, p, p + 2, p, None) == bad and fill(p, p, 3, 5, p, p, p + 4, None) == bad
    assert fill(p, p, top + 1, 5, p, p, p, None) == big and fill(p, p, 3, top + 1, p, p, p, None) == big
    assert fill(p, p, 0, 5, p, p, p, None) == 0 and fill(None, None, 0, 5, None, None, None, None) == 0
    assert fill(None, None, 3, 0, None, None, None, None) == 0

    #             nbr scores row_off n_rows total row_ids n_ids k out_ids out_scores out_count err stream
    def sel(**kw):
        args = dict(nbr=p, scores=p, row_off=p, n_rows=2, total=4, row_ids=p, n_ids=3, k=2, out_ids=p, out_scores=p, out_count=p,
                    err=p)
        args.update(kw)
        return select(*args.values(), None)

    assert sel(n_rows=-1) == bad and sel(total=-1) == bad and sel(k=0) == bad and sel(k=-3) == bad and sel(n_ids=-1) == bad
    for name in ("nbr", "scores", "row_off", "out_ids", "out_scores", "out_count", "err"):
        assert sel(**{name: None}) == bad, name
    for name in ("nbr", "row_off", "row_ids", "out_ids"):
        assert sel(**{name: p + 4}) == bad, name
    for name in ("scores", "out_scores", "out_count", "err"):
        assert sel(**{name: p + 2}) == bad, name
    assert sel(n_rows=top + 1) == big and sel(n_rows=top + 1, k=0) == bad
    assert sel(n_rows=0) == 0 and sel(n_rows=0, nbr=None, scores=None, row_off=None, out_ids=None, err=None) == 0
    assert not buf.any()


@pytest.mark.parametrize("kwargs, match", (
    ({"k": 0}, "k must be"), ({"k": -2}, "k must be"), ({"k": True}, "k must be"), ({"k": False}, "k must be"),
    ({"min_collisions": 0}, "min_collisions"), ({"min_collisions": 5}, "min_collisions"), ({"min_collisions": True}, "min_collisions"),
    ({"max_bucket": 1}, "max_bucket"), ({"max_bucket": 2.5}, "max_bucket"), ({"max_pairs": -1}, "max_pairs"),
    ({"max_raw_pairs": -1}, "max_raw_pairs")))
def test_bad_arguments_raise_before_any_gpu_call(kwargs, match, monkeypatch):
    from lshrs_amd import LSHRS, InMemoryStorage, lsh_knn

    args = {"k": 10}
    args.update(kwargs)
    k = args.pop("k")
    _no_gpu(monkeypatch)
    with pytest.raises(ValueError, match=match):
        lsh_knn(None, k, None, None, None, 4, 1, **args)
    index = LSHRS(dim=16, num_perm=16, num_bands=4, rows_per_band=4, storage=InMemoryStorage(), keep_vectors="float32")
    if "max_raw_pairs" not in args:
        with pytest.raises(ValueError, match=match):
            index.neighbors(k, **args)


def test_good_arguments_get_as_far_as_the_gpu(monkeypatch):
    from lshrs_amd import lsh_knn

    _no_gpu(monkeypatch)
    for k, args in ((1, {}), (np.int64(7), {"min_collisions": 4, "max_bucket": 2}), (10, {"max_pairs": 0, "max_raw_pairs": 0})):
        with pytest.raises(AssertionError, match="the GPU was asked for"):
            lsh_knn(None, k, None, None, None, 4, 1, **args)


def test_the_key_of_a_score():
    order = [np.inf, 1.0, np.float32(0.3), 0.0, -0.0, -1e-30, -1.0, -np.inf, np.nan]
    keys = [desc_key(s) for s in order]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert desc_key(np.nan) == desc_key(-np.nan) == 0xFFFFFFFF and desc_key(0.0) + 1 == desc_key(-0.0) == 0x80000000
    assert rank_list([(9, 0.5), (3, 0.5), (7, np.nan), (4, 0.75), (5, -0.0), (6, 0.0), (2, np.nan)], 6) == \
        [(4, 0.75), (3, 0.5), (9, 0.5), (6, 0.0), (5, -0.0), (2, pytest.approx(np.nan, nan_ok=True))]


def test_the_reference_on_a_segment_written_by_hand():
    # two bands of one key byte (code = band << 8 | key).  band 0: {10, 11, 12, 13} and {20, 21}; band 1: {10, 11}, {12, 20, 21}
    # and 30 alone.  40 has a row and is in no bucket.
    seg = hand_segment({0x001: [10, 11, 12, 13], 0x002: [20, 21], 0x101: [11, 10], 0x102: [12, 20, 21], 0x103: [30]})
    mates, stats = candidates_reference([seg])
    assert mates == {10: {11, 12, 13}, 11: {10, 12, 13}, 12: {10, 11, 13, 20, 21}, 13: {10, 11, 12}, 20: {12, 21}, 21: {12, 20}}
    assert stats["raw_pairs"] == 6 + 1 + 1 + 3 and stats["emitted"] == 9 and stats["buckets"] == 5
    live = [40, 30, 21, 20, 13, 12, 11, 10]

    def score(a, b):                    # oriented: asking from the lower id scores one notch higher
        table = {(10, 11): 0.5, (10, 12): 0.5, (10, 13): 0.25, (11, 12): 0.75, (11, 13): 0.75, (12, 13): -0.5, (12, 20): 0.5,
                 (12, 21): 0.5, (20, 21): 1.0}
        return table[(min(a, b), max(a, b))] + (0.0625 if a < b else 0.0)

    ids, nbrs, scores, counts, stats = knn_join_reference([seg], live, 2, score)
    nan = float("nan")
    assert ids.tolist() == [10, 11, 12, 13, 20, 21, 30, 40] and ids.dtype == np.int64
    assert nbrs.tolist() == [[11, 12], [12, 13], [11, 20], [11, 10], [21, 12], [20, 12], [-1, -1], [-1, -1]]
    assert counts.tolist() == [2, 2, 2, 2, 2, 2, 0, 0] and counts.dtype == np.int32 and nbrs.dtype == np.int64
    want = [[0.5625, 0.5625], [0.8125, 0.8125], [0.75, 0.5625], [0.75, 0.25], [1.0625, 0.5], [1.0, 0.5], [nan, nan], [nan, nan]]
    assert scores.dtype == np.float32 and np.array_equal(scores, np.array(want, dtype=np.float32), equal_nan=True)
    assert stats["candidates_max"] == 5 and stats["short_rows"] == 2
    # k beyond the lists: the width is min(k, n - 1), the lists are padded
    ids, nbrs, scores, counts, stats = knn_join_reference([seg], live, 100, score)
    assert nbrs.shape == (8, 7) and counts.tolist() == [3, 3, 5, 3, 2, 2, 0, 0] and stats["short_rows"] == 8
    assert nbrs[2].tolist() == [11, 20, 21, 10, 13, -1, -1] and np.isnan(scores[2, 5:]).all()
    # two collisions and more: only (10, 11) and (20, 21) meet in both bands; a bucket limit of 3 drops band 0's first bucket
    ids, nbrs, _, counts, stats = knn_join_reference([seg], live, 2, score, min_collisions=2)
    assert nbrs[:, 0].tolist() == [11, 10, -1, -1, 21, 20, -1, -1] and counts.tolist() == [1, 1, 0, 0, 1, 1, 0, 0]
    ids, nbrs, _, counts, stats = knn_join_reference([seg], live, 2, score, max_bucket=3)
    assert stats["skipped_buckets"] == 1 and nbrs.tolist()[:3] == [[11, -1], [10, -1], [20, 21]]
