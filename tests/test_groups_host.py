"""Host side of the near-duplicate groups (lshrs_amd.group_pairs, lshrs_cc_*): the names, the second library and what it
exports, the C entries' argument checks, what the Python layers decide before any GPU call, and the plain-Python reference
against SciPy's connected components.  No GPU."""

from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

from tests._groups_reference import group_lists, groups_reference, labels_reference, removable

GROUPS_EXPORTS = ("lshrs_groups_abi_version", "lshrs_cc_init_i32", "lshrs_cc_hook_i64", "lshrs_cc_flatten_i32")


def _lib():
    from lshrs_amd import _native

    _native.build()
    return _native.load_groups()


def _no_gpu(monkeypatch):
    from lshrs_amd import _native

    def no_gpu():
        raise AssertionError("the GPU was asked for")

    monkeypatch.setattr(_native, "require_gpu", no_gpu)
    monkeypatch.setattr(_native, "load", no_gpu)
    monkeypatch.setattr(_native, "load_groups", no_gpu)


def test_names_are_exported():
    import lshrs_amd
    from lshrs_amd import DeviceVectors, LSHRS, _groups, _native

    for name in ("group_pairs", "exact_groups_above", "lsh_groups_above"):
        assert callable(getattr(lshrs_amd, name)) and name in lshrs_amd.__all__ and name in _groups.__all__
    assert callable(_groups.connected_labels) and "connected_labels" in _groups.__all__
    assert callable(DeviceVectors.groups_above) and callable(DeviceVectors.lsh_groups_above)
    assert callable(LSHRS.groups_exact_above) and callable(LSHRS.groups_above) and callable(LSHRS.recall_groups_above)
    # the first library's units are what they were: the components are a library of their own
    assert _native.UNITS == ("sig_setup", "sig_f32", "sig16", "sig16r", "sig_replay", "sig_small", "sig_split", "storage",
                             "rerank", "query", "idmap", "scan", "pipeline", "join")
    assert os.path.exists(_native.GROUPS_SOURCE) and "groups" not in _native.UNITS
    for doc in (lshrs_amd.group_pairs.__doc__, lshrs_amd.exact_groups_above.__doc__, lshrs_amd.lsh_groups_above.__doc__,
                LSHRS.groups_above.__doc__, LSHRS.groups_exact_above.__doc__):
        doc = " ".join(doc.split())
        assert "connected component" in doc and "SINGLE LINKAGE" in doc and "smallest id" in doc


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lshrs_[a-z0-9_]+)\s*\(", text)))


def test_the_entries_are_in_their_header_their_tuple_and_their_own_library():
    from lshrs_amd import _native

    lib = _lib()
    path = _native.GROUPS_LIBRARY
    assert os.path.basename(path) == "liblshrs_groups.so" and os.path.dirname(path) == _native.CSRC
    dynamic = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (lshrs_\w+)", dynamic))
    header = os.path.join(_native.INCLUDE, "lshrs_groups.h")
    assert _declared(header) == sorted(GROUPS_EXPORTS) == sorted(_native.EXPORTS_GROUPS) == sorted(exported)
    assert len(set(_native.EXPORTS_GROUPS)) == 4
    for name in GROUPS_EXPORTS:
        assert hasattr(lib, name)
        assert name not in _native.EXPORTS + _native.EXPORTS_KNN + _native.EXPORTS_JOIN
    assert lib.lshrs_groups_abi_version() == 1 == _native.GROUPS_ABI_VERSION
    text = open(header).read()
    assert int(re.search(r"#define\s+LSHRS_GROUPS_ABI_VERSION\s+(\d+)", text).group(1)) == 1
    assert int(re.search(r"#define\s+LSHRS_CC_ERR_ENDPOINT\s+(\w+)", text).group(1), 0) == _native.CC_ERR_ENDPOINT == 1
    assert int(re.search(r"#define\s+LSHRS_CC_ERR_CAP\s+(\w+)", text).group(1), 0) == _native.CC_ERR_CAP == 2
    # device code for gfx950 inside, and no need of the first library
    assert b"gfx950" in open(path, "rb").read()
    needed = subprocess.run(["readelf", "-d", path], check=True, capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "liblshrs_hip" not in needed and "liblshrs_host" not in needed
    undefined = subprocess.run(["nm", "-D", "--undefined-only", path], check=True, capture_output=True, text=True).stdout
    assert not re.search(r"\blshrs_", undefined)
    # the first library exports what it exported
    first = subprocess.run(["nm", "-D", "--defined-only", _native.LIBRARY], check=True, capture_output=True, text=True).stdout
    assert set(re.findall(r"\bT (lshrs_\w+)", first)) == set(_native.EXPORTS) | set(_native.EXPORTS_KNN) | set(_native.EXPORTS_JOIN)
    assert not set(re.findall(r"\bT (lshrs_\w+)", first)) & exported


def test_the_first_library_loads_without_the_second(tmp_path, monkeypatch):
    from lshrs_amd import _native

    _lib()
    monkeypatch.setattr(_native, "_groups_lib", None)
    monkeypatch.setattr(_native, "GROUPS_LIBRARY", str(tmp_path / "nope.so"))
    assert _native.load().lshrs_abi_version() == _native.ABI_VERSION
    with pytest.raises(_native.NativeLibraryError, match="has not been built"):
        _native.load_groups()


def test_a_fresh_library_is_not_rebuilt_by_the_rule_of_the_first():
    from lshrs_amd import _native

    _lib()
    deps = _native._sources_of(_native.GROUPS_SOURCE)
    assert {os.path.basename(p) for p in deps} == {"groups.hip", "lshrs_groups.h", "lshrs_hip.h", "lshrs_lists.h"}
    assert os.path.getmtime(_native.GROUPS_LIBRARY) >= max(os.path.getmtime(p) for p in deps)
    before = os.path.getmtime(_native.GROUPS_LIBRARY)
    _native.build()                                             # fresh: nothing is compiled
    assert os.path.getmtime(_native.GROUPS_LIBRARY) == before and not os.path.exists(_native.GROUPS_LIBRARY + ".tmp")


def test_c_entries_check_their_arguments_on_the_host():
    """Status codes of lshrs_cc_*, decided before anything touches a device (there is none here)."""
    from lshrs_amd import _native

    lib = _lib()
    buf = np.zeros(16, dtype=np.int64)
    p = (buf.ctypes.data + 15) // 16 * 16
    bad, big, top = _native.E_BADARG, _native.E_TOOLARGE, (1 << 31) - 1
    init, hook, flatten = lib.lshrs_cc_init_i32, lib.lshrs_cc_hook_i64, lib.lshrs_cc_flatten_i32
    #           parent n stream
    assert init(p, -1, None) == bad
    assert init(None, 5, None) == bad and init(p + 2, 5, None) == bad
    assert init(p, top + 1, None) == big and init(None, top + 1, None) == big and init(p, 1 << 40, None) == big
    assert init(p, 0, None) == 0 and init(None, 0, None) == 0
    #           a b n_edges parent n err stream
    assert hook(p, p, -1, p, 5, p, None) == bad and hook(p, p, 3, p, -1, p, None) == bad
    assert hook(None, p, 3, p, 5, p, None) == bad and hook(p, None, 3, p, 5, p, None) == bad
    assert hook(p, p, 3, None, 5, p, None) == bad and hook(p, p, 3, p, 5, None, None) == bad
    assert hook(p + 4, p, 3, p, 5, p, None) == bad and hook(p, p + 4, 3, p, 5, p, None) == bad      # a, b: 8 bytes
    assert hook(p, p, 3, p + 2, 5, p, None) == bad and hook(p, p, 3, p, 5, p + 1, None) == bad      # parent, err: 4 bytes
    assert hook(p, p, 3, p, top + 1, p, None) == big and hook(p, p, -1, p, top + 1, p, None) == bad
    assert hook(p, p, 0, p, 5, p, None) == 0 and hook(None, None, 0, None, 5, None, None) == 0
    assert hook(p, p, 3, p, 0, p, None) == 0 and hook(None, None, 3, None, 0, None, None) == 0
    #              parent n err stream
    assert flatten(p, -1, p, None) == bad
    assert flatten(None, 5, p, None) == bad and flatten(p, 5, None, None) == bad
    assert flatten(p + 2, 5, p, None) == bad and flatten(p, 5, p + 2, None) == bad
    assert flatten(p, top + 1, p, None) == big
    assert flatten(p, 0, p, None) == 0 and flatten(None, 0, None, None) == 0
    assert not buf.any()


@pytest.mark.parametrize("a, b, match", (
    ([1, 2, 3], [4, 5], "equal length"),
    (np.zeros((2, 2), np.int64), np.zeros((2, 2), np.int64), "one-dimensional"),
    (np.int64(3), np.int64(4), "one-dimensional"),
    ([1.0, 2.0], [3.0, 4.0], "integer"),
    (np.array([1, 2]), np.array([True, False]), "integer"),
    (np.array(["a", "b"]), np.array([1, 2]), "integer")))
def test_bad_pair_lists_raise_before_any_gpu_call(a, b, match, monkeypatch):
    from lshrs_amd import _groups, group_pairs

    _no_gpu(monkeypatch)
    with pytest.raises(ValueError, match=match):
        group_pairs(a, b)
    with pytest.raises(ValueError, match=match):
        _groups.connected_labels(a, b, 10)


def test_bad_tensors_raise_before_any_gpu_call(monkeypatch):
    import torch

    from lshrs_amd import _groups, group_pairs

    _no_gpu(monkeypatch)
    ok = torch.arange(4)
    for a, b, match in ((ok, torch.arange(5), "equal length"), (ok.reshape(2, 2), ok.reshape(2, 2), "one-dimensional"),
                        (ok.float(), ok, "integer"), (ok, ok > 1, "integer")):
        with pytest.raises(ValueError, match=match):
            group_pairs(a, b)
    with pytest.raises(ValueError, match="n must be"):
        _groups.connected_labels(ok, ok, -1)
    # good ones get as far as the GPU: int32 tensors, lists, empty lists of no particular dtype
    for a, b in ((ok, ok), (ok.int(), ok.int()), ([1, 2], [2, 3]), ([], []), (np.array([1], np.uint8), np.array([2], np.int16))):
        with pytest.raises(AssertionError, match="the GPU was asked for"):
            group_pairs(a, b)


@pytest.mark.parametrize("kwargs, match", (
    ({"threshold": float("nan")}, "threshold"), ({"threshold": [0.2, 0.3]}, "threshold"), ({"threshold": 1.5}, "threshold"),
    ({"threshold": None}, "threshold"), ({"max_pairs": -1}, "max_pairs"),
    ({"min_collisions": 0}, "min_collisions"), ({"min_collisions": 5}, "min_collisions"), ({"min_collisions": True}, "min_collisions"),
    ({"max_bucket": 1}, "max_bucket"), ({"max_bucket": 2.5}, "max_bucket"), ({"max_raw_pairs": -1}, "max_raw_pairs")))
def test_bad_join_arguments_raise_before_any_gpu_call(kwargs, match, monkeypatch):
    """Through the existing checkers: what the two joins refuse, the group forms refuse."""
    from lshrs_amd import LSHRS, InMemoryStorage, exact_groups_above, lsh_groups_above

    args = {"threshold": 0.5}
    args.update(kwargs)
    threshold = args.pop("threshold")
    _no_gpu(monkeypatch)
    with pytest.raises(ValueError, match=match):
        lsh_groups_above(None, threshold, None, None, None, 4, 1, **args)
    index = LSHRS(dim=16, num_perm=16, num_bands=4, rows_per_band=4, storage=InMemoryStorage(), keep_vectors="float32")
    if "max_raw_pairs" not in args:
        with pytest.raises(ValueError, match=match):
            index.groups_above(threshold, **args)
    if not set(args) - {"max_pairs"}:
        with pytest.raises(ValueError, match=match):
            exact_groups_above(None, threshold, **args)


def test_good_join_arguments_get_as_far_as_the_gpu(monkeypatch):
    from lshrs_amd import exact_groups_above, lsh_groups_above

    _no_gpu(monkeypatch)
    with pytest.raises(AssertionError, match="the GPU was asked for"):
        exact_groups_above(None, 0.5, max_pairs=0)
    for args in ({}, {"min_collisions": 4, "max_bucket": 2}, {"max_pairs": 0, "max_raw_pairs": 0}):
        with pytest.raises(AssertionError, match="the GPU was asked for"):
            lsh_groups_above(None, 0.5, None, None, None, 4, 1, **args)


def test_the_reference_on_cases_written_by_hand():
    members, offsets = groups_reference([5, 9, 2, 7, 7], [9, 1, 2, 3, 3])
    assert members.tolist() == [1, 5, 9, 2, 3, 7] and offsets.tolist() == [0, 3, 4, 6]
    assert members.dtype == np.int64 and offsets.dtype == np.int64
    assert group_lists(members, offsets) == [[1, 5, 9], [2], [3, 7]] and removable(offsets) == 3
    members, offsets = groups_reference([], [])
    assert members.shape == (0,) and offsets.tolist() == [0] and removable(offsets) == 0
    # a chain a ~ b ~ c is one group; sparse ids up to 2^62
    big = 1 << 62
    assert group_lists(*groups_reference([big, 7], [7, 3])) == [[3, 7, big]]
    assert labels_reference([3, 0, -1, 4], [1, 0, 2, 9], 6).tolist() == [0, 1, 2, 1, 4, 5]
    assert labels_reference([], [], 3).dtype == np.int32


@pytest.mark.parametrize("n, degree, seed", ((50, 0.5, 1), (200, 1.0, 2), (2000, 0.8, 3), (2000, 1.2, 4), (3000, 3.0, 5)))
def test_the_reference_equals_scipy_connected_components(n, degree, seed):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    rng = np.random.default_rng(seed)
    e = int(n * degree / 2)
    ids = np.sort(rng.choice(1 << 50, size=n, replace=False)).astype(np.int64)
    a, b = rng.integers(0, n, size=e), rng.integers(0, n, size=e)
    graph = coo_matrix((np.ones(e, np.int8), (a, b)), shape=(n, n))
    count, labels = connected_components(graph, directed=False)
    touched = np.zeros(n, dtype=bool)
    touched[a] = touched[b] = True
    want = {}
    for v in np.flatnonzero(touched).tolist():
        want.setdefault(int(labels[v]), []).append(int(ids[v]))
    want = sorted(want.values())                       # (each list ascends: sorted by its first, smallest id)
    members, offsets = groups_reference(ids[a], ids[b])
    assert group_lists(members, offsets) == want
    assert members.shape[0] == int(touched.sum()) and removable(offsets) == int(touched.sum()) - len(want)
    # the dense labels: SciPy's partition, named by the smallest vertex
    mine = labels_reference(a, b, n)
    assert len(set(mine.tolist())) == count
    first = {}
    for v, lab in enumerate(labels.tolist()):
        first.setdefault(lab, v)
    assert mine.tolist() == [first[lab] for lab in labels.tolist()]
