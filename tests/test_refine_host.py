"""Host side of the graph refinement (lshrs_amd.refine_knn, lshrs_refine_*): the names, the fourth library and what it exports,
the C entries' argument checks, what the Python layers decide before any GPU call, and the plain-Python reference on graphs
worked out by hand.  No GPU."""

from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

from tests._refine_reference import (adjacency_of, bound_reference, csr_of, edges_reference, expand_reference,
                                     restricted_reference)

REFINE_EXPORTS = ("lshrs_refine_abi_version", "lshrs_refine_wave_set", "lshrs_refine_max_set", "lshrs_refine_edges_i64",
                  "lshrs_refine_expand_count_i64", "lshrs_refine_expand_write_i64")


def _lib():
    from lshrs_amd import _native

    _native.build()
    return _native.load_refine()


def _no_gpu(monkeypatch):
    from lshrs_amd import _native

    def no_gpu():
        raise AssertionError("the GPU was asked for")

    for name in ("require_gpu", "load", "load_groups", "load_graph", "load_refine"):
        monkeypatch.setattr(_native, name, no_gpu)


def test_names_are_exported():
    import lshrs_amd
    from lshrs_amd import DeviceVectors, LSHRS, _native, _refine
    from lshrs_amd.vectors import TensorRows

    for name in ("refine_knn", "graph_edges", "expand_candidates"):
        assert callable(getattr(lshrs_amd, name)) and name in lshrs_amd.__all__ and name in _refine.__all__
    assert callable(DeviceVectors.refine_neighbors) and callable(TensorRows.refine_neighbors)
    assert os.path.exists(_native.REFINE_SOURCE) and "refine" not in _native.UNITS
    doc = " ".join(lshrs_amd.refine_knn.__doc__.split())
    for phrase in ("RESTRICTED TO", "bit for bit", "never decreases", "fixed point", "within two steps", "ASCENDING ID"):
        assert phrase in doc, phrase
    import inspect

    assert inspect.signature(LSHRS.neighbors).parameters["refine_rounds"].default == 0
    assert inspect.signature(LSHRS.neighbors).parameters["max_degree"].default is None
    assert inspect.signature(LSHRS.recall_neighbors).parameters["refine_rounds"].default == 0


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lshrs_[a-z0-9_]+)\s*\(", text)))


def _exported(path):
    dynamic = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (lshrs_\w+)", dynamic))


def test_build_makes_the_fourth_library_with_its_header_s_entries_and_nothing_of_the_others():
    from lshrs_amd import _native

    lib = _lib()
    path = _native.REFINE_LIBRARY
    assert os.path.basename(path) == "liblshrs_refine.so" and os.path.dirname(path) == _native.CSRC and os.path.exists(path)
    exported = _exported(path)
    header = os.path.join(_native.INCLUDE, "lshrs_refine.h")
    assert _declared(header) == sorted(REFINE_EXPORTS) == sorted(_native.EXPORTS_REFINE) == sorted(exported)
    others = _native.EXPORTS + _native.EXPORTS_KNN + _native.EXPORTS_JOIN + _native.EXPORTS_GROUPS + _native.EXPORTS_GRAPH
    for name in REFINE_EXPORTS:
        assert hasattr(lib, name) and name not in others
    assert lib.lshrs_refine_abi_version() == 1 == _native.REFINE_ABI_VERSION
    text = open(header).read()
    assert int(re.search(r"#define\s+LSHRS_REFINE_ABI_VERSION\s+(\d+)", text).group(1)) == 1
    for name, want in (("OUTSIDE", 1), ("SELF", 2), ("RANGE", 1), ("ENTRY", 2)):
        assert int(re.search(r"#define\s+LSHRS_REFINE_ERR_" + name + r"\s+(\w+)", text).group(1), 0) == want \
            == getattr(_native, "REFINE_ERR_" + name)
    # device code for gfx950 inside, and no need of the other three libraries
    assert b"gfx950" in open(path, "rb").read()
    needed = subprocess.run(["readelf", "-d", path], check=True, capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "liblshrs_" not in needed
    undefined = subprocess.run(["nm", "-D", "--undefined-only", path], check=True, capture_output=True, text=True).stdout
    assert not re.search(r"\blshrs_", undefined)
    # the other three export what they exported
    assert _exported(_native.LIBRARY) == set(_native.EXPORTS) | set(_native.EXPORTS_KNN) | set(_native.EXPORTS_JOIN)
    assert _exported(_native.GROUPS_LIBRARY) == set(_native.EXPORTS_GROUPS)
    assert _exported(_native.GRAPH_LIBRARY) == set(_native.EXPORTS_GRAPH)
    # fresh: nothing is compiled again
    deps = _native._sources_of(_native.REFINE_SOURCE)
    assert {os.path.basename(p) for p in deps} == {"refine.hip", "lshrs_refine.h", "lshrs_hip.h", "lshrs_lists.h"}
    before = os.path.getmtime(path)
    _native.build()
    assert os.path.getmtime(path) == before and not os.path.exists(path + ".tmp")


def test_the_tiers_fit_two_workgroups_into_a_cu():
    lib = _lib()
    wave, most = lib.lshrs_refine_wave_set(), lib.lshrs_refine_max_set()
    assert 64 <= wave < most
    # a table of twice the limit, four bytes a slot: four waves' tables per workgroup, or one workgroup's; two of either
    # beside each other within the 160 KiB of a CU
    assert 2 * (4 * 2 * wave * 4) <= 160 * 1024 and 2 * (2 * most * 4 + 4096) <= 160 * 1024


def test_the_other_libraries_load_without_the_fourth(tmp_path, monkeypatch):
    from lshrs_amd import _native

    _lib()
    monkeypatch.setattr(_native, "_refine_lib", None)
    monkeypatch.setattr(_native, "REFINE_LIBRARY", str(tmp_path / "nope.so"))
    assert _native.load().lshrs_abi_version() == _native.ABI_VERSION
    assert _native.load_graph().lshrs_graph_abi_version() == _native.GRAPH_ABI_VERSION
    with pytest.raises(_native.NativeLibraryError, match="has not been built") as exc:
        _native.load_refine()
    assert "nope.so" in str(exc.value)


def test_c_entries_check_their_arguments_on_the_host():
    """Status codes of lshrs_refine_*, decided before anything touches a device (there is none here)."""
    from lshrs_amd import _native

    lib = _lib()
    buf = np.zeros(16, dtype=np.int64)
    p = (buf.ctypes.data + 15) // 16 * 16
    bad, big, top = _native.E_BADARG, _native.E_TOOLARGE, (1 << 31) - 1
    edges, count, write = lib.lshrs_refine_edges_i64, lib.lshrs_refine_expand_count_i64, lib.lshrs_refine_expand_write_i64
    #            graph n_rows k_in keep err stream
    assert edges(p, -1, 4, p, p, None) == bad and edges(p, 5, -1, p, p, None) == bad
    assert edges(None, 5, 4, p, p, None) == bad and edges(p, 5, 4, None, p, None) == bad and edges(p, 5, 4, p, None, None) == bad
    assert edges(p + 4, 5, 4, p, p, None) == bad and edges(p, 5, 4, p, p + 2, None) == bad
    assert edges(p, top + 1, 1, p, p, None) == big and edges(p, 1 << 30, 2, p, p, None) == big
    assert edges(p, 0, 4, p, p, None) == 0 and edges(None, 0, 4, None, None, None) == 0 and edges(None, 5, 0, None, None, None) == 0

    #             nbr row_off n_rows total max_degree cand_count err stream
    def cnt(**kw):
        args = dict(nbr=p, row_off=p, n_rows=2, total=4, max_degree=0, cand_count=p, err=p)
        args.update(kw)
        return count(*args.values(), None)

    assert cnt(n_rows=-1) == bad and cnt(total=-1) == bad and cnt(n_rows=top + 1) == big
    for name in ("nbr", "row_off", "cand_count", "err"):
        assert cnt(**{name: None}) == bad, name
    assert cnt(nbr=p + 4) == bad and cnt(row_off=p + 4) == bad and cnt(cand_count=p + 2) == bad and cnt(err=p + 1) == bad
    assert cnt(n_rows=0) == 0 and cnt(n_rows=0, nbr=None, row_off=None, cand_count=None, err=None) == 0

    #             nbr row_off n_rows total max_degree cand_off cand cand_total err stream
    def wr(**kw):
        args = dict(nbr=p, row_off=p, n_rows=2, total=4, max_degree=0, cand_off=p, cand=p, cand_total=4, err=p)
        args.update(kw)
        return write(*args.values(), None)

    assert wr(n_rows=-1) == bad and wr(total=-1) == bad and wr(cand_total=-1) == bad and wr(n_rows=top + 1) == big
    for name in ("nbr", "row_off", "cand_off", "cand", "err"):
        assert wr(**{name: None}) == bad, name
    for name in ("nbr", "row_off", "cand_off", "cand"):
        assert wr(**{name: p + 4}) == bad, name
    assert wr(err=p + 2) == bad
    assert wr(n_rows=0) == 0 and wr(n_rows=0, nbr=None, row_off=None, cand_off=None, cand=None, err=None) == 0
    assert not buf.any()


@pytest.mark.parametrize("kwargs, match", (
    ({"k": 0}, "k must be"), ({"k": -2}, "k must be"), ({"k": True}, "k must be"), ({"k": False}, "k must be"),
    ({"rounds": -1}, "rounds"), ({"rounds": True}, "rounds"), ({"rounds": 1.5}, "rounds"),
    ({"max_degree": 0}, "max_degree"), ({"max_degree": -3}, "max_degree"), ({"max_degree": True}, "max_degree"),
    ({"max_degree": 2.5}, "max_degree"), ({"max_entries": -1}, "max_entries"), ({"max_entries": False}, "max_entries")))
def test_bad_arguments_raise_before_any_gpu_call(kwargs, match, monkeypatch):
    from lshrs_amd import LSHRS, InMemoryStorage, expand_candidates, refine_knn

    args = {"k": 10}
    args.update(kwargs)
    k = args.pop("k")
    _no_gpu(monkeypatch)
    with pytest.raises(ValueError, match=match):
        refine_knn(None, None, k, **args)
    if "max_degree" in args:
        with pytest.raises(ValueError, match=match):
            expand_candidates(None, None, args["max_degree"])
    if "max_entries" not in args:
        index = LSHRS(dim=16, num_perm=16, num_bands=4, rows_per_band=4, storage=InMemoryStorage(), keep_vectors="float32")
        named = {"refine_rounds" if key == "rounds" else key: value for key, value in args.items()}
        with pytest.raises(ValueError, match=match):
            index.neighbors(k, **named)
        if "rounds" in args:
            with pytest.raises(ValueError, match=match):
                index.recall_neighbors(3, refine_rounds=args["rounds"])


def test_good_arguments_get_as_far_as_the_gpu(monkeypatch):
    from lshrs_amd import refine_knn

    _no_gpu(monkeypatch)
    for k, args in ((1, {}), (np.int64(7), {"rounds": 0, "max_degree": 1}), (10, {"rounds": np.int32(3), "max_entries": 0})):
        with pytest.raises(AssertionError, match="the GPU was asked for"):
            refine_knn(None, None, k, **args)


# ------------------------------------------------------------------------------------------
# the reference, on graphs worked out by hand
# ------------------------------------------------------------------------------------------
def test_a_path():
    # 0 -> 1 -> 2 -> 3 -> 4, one entry per row
    graph = np.array([[1], [2], [3], [4], [-1]])
    assert edges_reference(graph).reshape(-1).tolist() == [1, 1, 1, 1, 0]
    lists = adjacency_of(graph)
    assert lists == [[1], [0, 2], [1, 3], [2, 4], [3]]
    assert expand_reference(lists) == [{1, 2}, {0, 2, 3}, {0, 1, 3, 4}, {1, 2, 4}, {2, 3}]
    assert bound_reference(lists) == [1 + 2, 2 + 1 + 2, 2 + 2 + 2, 2 + 2 + 1, 1 + 2]
    nbr, off = csr_of(lists)
    assert nbr.tolist() == [1, 0, 2, 1, 3, 2, 4, 3] and off.tolist() == [0, 1, 3, 5, 7, 8]


def test_a_star():
    # the leaves 1 .. 5 all list the hub 0, which lists nobody
    graph = np.array([[-1]] + [[0]] * 5)
    assert edges_reference(graph).reshape(-1).tolist() == [0, 1, 1, 1, 1, 1]
    lists = adjacency_of(graph)
    assert lists == [[1, 2, 3, 4, 5]] + [[0]] * 5
    leaves = {1, 2, 3, 4, 5}
    assert expand_reference(lists) == [leaves] + [{0} | (leaves - {r}) for r in range(1, 6)]
    # a hub over the cap is nobody's midpoint, and still everybody's candidate; its own list is what it was
    assert expand_reference(lists, max_degree=4) == [leaves] + [{0}] * 5
    assert expand_reference(lists, max_degree=5) == expand_reference(lists)
    assert bound_reference(lists, max_degree=4) == [5 + 5] + [1] * 5 and bound_reference(lists) == [10] + [6] * 5


def test_a_mutual_pair_and_a_duplicated_entry():
    # 0 and 1 list each other (the lower row's entry survives); 2 lists 0 twice (the first occurrence counts) and 1 once
    graph = np.array([[1, -1, -1], [0, -1, -1], [0, 0, 1]])
    assert edges_reference(graph).tolist() == [[1, 0, 0], [0, 0, 0], [1, 0, 1]]
    assert adjacency_of(graph) == [[1, 2], [0, 2], [0, 1]]
    # what has no business in a table is kept out and nothing is read through it
    graph = np.array([[0, 7, -2], [2, -1, 0], [1, 1, -1]])
    assert edges_reference(graph).tolist() == [[0, 0, 0], [1, 0, 1], [0, 0, 0]]
    assert adjacency_of(graph) == [[1], [0, 2], [1]]
    # entries outside the rows are skipped by the expansion, as candidates and as midpoints
    assert expand_reference([[1, 9], [0, -1, 2], [1]]) == [{1, 2}, {0, 2}, {1, 0}]


def test_the_restriction_of_a_full_ranking():
    ids = np.array([10, 20, 30, 40])
    nbrs = np.array([[20, 30, 40], [10, 40, 30], [40, 10, 20], [30, 20, 10]])
    scores = np.array([[.9, .5, .1], [.9, .8, .2], [.7, .5, .2], [.7, .8, .1]], dtype=np.float32)
    got = restricted_reference(ids, nbrs, scores, {10: {30, 40}, 20: {10, 30, 40}, 30: set(), 40: {10}}, 2)
    assert got[0].tolist() == [[30, 40], [10, 40], [-1, -1], [10, -1]] and got[2].tolist() == [2, 2, 0, 1]
    assert np.array_equal(got[1], np.array([[.5, .1], [.9, .8], [np.nan] * 2, [.1, np.nan]], dtype=np.float32), equal_nan=True)
    assert restricted_reference(ids, nbrs, scores, [{20}] * 4, 9)[0].shape == (4, 3)
