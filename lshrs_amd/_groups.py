"""Near-duplicate GROUPS - ``group_pairs``, ``exact_groups_above``, ``lsh_groups_above`` - and what they are made of: the
connected components of a list of pairs, computed where the pairs are.

A GROUP is a connected component of the graph whose edges are the given pairs - for the two ``*_groups_above`` the graph
"score >= threshold" over the stored vectors.  That is SINGLE LINKAGE: two members of one group are joined by a chain of pairs
at or above the threshold, and may themselves score below it.  The first member of a group is its smallest id; keeping that
one of every group (and every id that is in no group) is a deduplication.

The components come from the three kernels of ``csrc/groups.hip`` (``include/lshrs_groups.h``, ``liblshrs_groups.so``) over
DENSE vertices: ``lshrs_cc_init_i32``, ``lshrs_cc_hook_i64`` - a lock-free union-find in which the larger root is always hung
under the smaller -, ``lshrs_cc_flatten_i32``.  The label of a vertex is the smallest vertex of its component, in whatever order
the lanes ran.  Around them, plumbing as ``_exact._judge_pairs`` has it: ``torch.unique`` makes arbitrary int64 ids dense
IN ID ORDER, so that the smallest vertex is the smallest id, and one stable ``torch.sort`` of the labels lays the groups out.

No CPU compute path: the host checks arguments, reads the error bits and three counts back, and keeps statistics.
"""

from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from . import _native
from ._exact import _finish, exact_pairs_above
from ._join import lsh_pairs_above
from .similarity import _on_device

__all__ = ["connected_labels", "group_pairs", "exact_groups_above", "lsh_groups_above"]

# edges of one hook launch: a longer list is hooked slice by slice into the same forest
_HOOK_SLICE = 1 << 31

ENDPOINT_MSG = "an endpoint of an edge lies outside [0, n)"


def _labels(torch, lib, a, b, n: int, dev):
    """The three kernels over contiguous int64 device tensors ``a`` / ``b`` (equal length) and ``n`` dense vertices: the int32
    labels, and the error bits read back behind them."""
    with torch.cuda.device(dev):
        labels = torch.empty((n,), dtype=torch.int32, device=dev)
        if n == 0:
            return labels, (_native.CC_ERR_ENDPOINT if int(a.shape[0]) else 0)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _native.check(lib.lshrs_cc_init_i32(labels.data_ptr(), n, stream), "lshrs_cc_init_i32")
        edges = int(a.shape[0])
        for begin in range(0, edges, _HOOK_SLICE):
            count = min(_HOOK_SLICE, edges - begin)
            _native.check(lib.lshrs_cc_hook_i64(a[begin:].data_ptr(), b[begin:].data_ptr(), count, labels.data_ptr(), n,
                                                err.data_ptr(), stream), "lshrs_cc_hook_i64")
        _native.check(lib.lshrs_cc_flatten_i32(labels.data_ptr(), n, err.data_ptr(), stream), "lshrs_cc_flatten_i32")
        return labels, int(err.item())


def _raise_for(bits: int) -> None:
    if bits & _native.CC_ERR_CAP:
        raise _native.NativeLibraryError("connected components: a lane passed the iteration cap of its loop "
                                         "(LSHRS_CC_ERR_CAP): the labels are not to be used")
    if bits & _native.CC_ERR_ENDPOINT:
        raise ValueError("connected components: " + ENDPOINT_MSG)


def _edge_args(ids_a, ids_b, what: str):
    """``ValueError`` unless the two are one-dimensional integer arrays (or tensors) of equal length; array-likes come back as
    int64 NumPy arrays, tensors as they are.  Pure host."""
    out = []
    for x in (ids_a, ids_b):
        if hasattr(x, "is_cuda") and hasattr(x, "dim"):              # a torch tensor, wherever it lives
            shape, integer = tuple(int(v) for v in x.shape), not (x.dtype.is_floating_point or x.dtype.is_complex
                                                                  or "bool" in str(x.dtype))
        else:
            x = np.asarray(x)
            shape, integer = tuple(x.shape), x.dtype.kind in "iu" or x.size == 0
        if len(shape) != 1:
            raise ValueError(f"{what}: the pairs are two one-dimensional arrays; received shape {shape}")
        if not integer:
            raise ValueError(f"{what}: the pairs are integer ids; received dtype {x.dtype}")
        out.append(x if hasattr(x, "is_cuda") else np.ascontiguousarray(x, dtype=np.int64))
    if int(out[0].shape[0]) != int(out[1].shape[0]):
        raise ValueError(f"{what}: the two arrays of a pair list have equal length; received {int(out[0].shape[0])} and "
                         f"{int(out[1].shape[0])}")
    return out


def _edges_on(torch, ids_a, ids_b):
    """The checked pair arrays as contiguous int64 tensors on one device: that of ``ids_a`` where it is there already."""
    on_gpu = isinstance(ids_a, torch.Tensor) and ids_a.is_cuda
    dev = ids_a.device if on_gpu else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        a, b = (_on_device(torch, t, np.int64).to(device=dev, dtype=torch.int64).contiguous() for t in (ids_a, ids_b))
    return a, b, dev


def connected_labels(a, b, n: int):
    """Device-level entry of the three kernels: the connected components of the undirected edges ``(a[e], b[e])`` over the
    dense vertices ``0 .. n - 1``.  ``a`` / ``b``: equal-length one-dimensional integer arrays, device tensors or array-likes
    (which are uploaded); repeated edges and ``a[e] == b[e]`` change nothing.  Returns the labels, int32 ``(n,)`` on the device:
    ``labels[x]`` is the smallest vertex of the component of ``x``.  An endpoint outside ``[0, n)`` raises ``ValueError``
    (the other edges were joined, the labels are dropped); a lane that passed its iteration cap - a logic error, never seen -
    raises ``NativeLibraryError``.  Lists of more than 2^31 edges are hooked in slices."""
    a, b = _edge_args(a, b, "connected_labels")
    n = int(n)
    if n < 0:
        raise ValueError(f"n must be >= 0; received {n}")
    torch = _native.require_gpu()
    lib = _native.load_groups()
    a, b, dev = _edges_on(torch, a, b)
    labels, bits = _labels(torch, lib, a, b, n, dev)
    _raise_for(bits)
    return labels


def _dense(torch, a, b):
    """Arbitrary int64 ids made dense in id order: ``(ids (v,) ascending, dense_a, dense_b)``."""
    p = int(a.shape[0])
    ids, inverse = torch.unique(torch.cat((a, b)), sorted=True, return_inverse=True)
    return ids, inverse[:p].contiguous(), inverse[p:].contiguous()


def _layout(torch, ids, labels):
    """The components laid out: ``(members, offsets, largest)`` - groups by ascending label (their smallest id), members
    ascending inside a group (the sort is stable and the dense order is the id order)."""
    by_label, order = torch.sort(labels, stable=True)
    _, count = torch.unique_consecutive(by_label, return_counts=True)
    offsets = torch.zeros(int(count.shape[0]) + 1, dtype=torch.int64, device=ids.device)
    offsets[1:] = torch.cumsum(count, 0)
    return ids[order].contiguous(), offsets, (int(count.max()) if int(count.shape[0]) else 0)


def group_pairs(ids_a, ids_b, *, return_tensors: bool = False, stats: Optional[Dict] = None):
    """The GROUPS of a list of pairs - the connected components of the graph whose edges are ``(ids_a[e], ids_b[e])``:
    ``(members (v,) int64, offsets (g + 1,) int64)``; group ``i`` is ``members[offsets[i]:offsets[i + 1]]``.  NumPy arrays, or
    device tensors with ``return_tensors``.

    ``ids_a`` / ``ids_b``: equal-length one-dimensional integer arrays - NumPy arrays, array-likes or tensors on any device -
    of arbitrary int64 ids, in any orientation; else ``ValueError`` before the GPU is touched.  Repeated pairs and pairs with
    ``a == b`` change nothing.  A group is a connected component, which is SINGLE LINKAGE: where the pairs are "score >=
    threshold", two members of one group are joined by a chain of such pairs and may score below the threshold against each
    other.  Groups come in ascending order of their smallest id, members ascend inside a group: the FIRST member of a group is
    its smallest id, and keeping that one per group is a deduplication.  Only ids that occur in a pair appear, so every group
    has at least two members unless all its pairs were ``a == b``.  No pairs give ``(empty, [0])``.

    The result does not depend on the order the lanes of the kernels ran in (``include/lshrs_groups.h``).
    ``stats``: a dict that receives ``pairs``, ``grouped`` (= v, the ids in some group), ``groups`` and ``largest`` (members
    of the largest group)."""
    ids_a, ids_b = _edge_args(ids_a, ids_b, "group_pairs")
    torch = _native.require_gpu()
    lib = _native.load_groups()
    a, b, dev = _edges_on(torch, ids_a, ids_b)
    with torch.cuda.device(dev):
        pairs = int(a.shape[0])
        out = {"pairs": pairs, "grouped": 0, "groups": 0, "largest": 0}
        members = torch.empty((0,), dtype=torch.int64, device=dev)
        offsets = torch.zeros(1, dtype=torch.int64, device=dev)
        if pairs:
            ids, da, db = _dense(torch, a, b)
            labels, bits = _labels(torch, lib, da, db, int(ids.shape[0]), dev)
            _raise_for(bits)
            members, offsets, largest = _layout(torch, ids, labels)
            out.update(grouped=int(members.shape[0]), groups=int(offsets.shape[0]) - 1, largest=largest)
    return _finish(stats, out, (members, offsets), return_tensors)


def _grouped(joined, jstats: Dict, return_tensors: bool, stats: Optional[Dict]):
    """The closing of both ``*_groups_above``: the join's device tensors grouped where they are, the two stats as one."""
    gstats: Dict = {}
    got = group_pairs(joined[0], joined[1], return_tensors=return_tensors, stats=gstats)
    if stats is not None:
        stats.clear()
        stats.update(jstats)
        stats.update(gstats)
    return got


def exact_groups_above(corpus, threshold, *, row_ids=None, max_pairs: int = 1 << 26, return_tensors: bool = False,
                       stats: Optional[Dict] = None):
    """The near-duplicate GROUPS among the rows of ``corpus`` at a cosine ``threshold``, exactly: the connected components of
    the graph whose edges are the pairs of :func:`lshrs_amd.exact_pairs_above` ``(corpus, threshold)`` - ``(members (v,)
    int64, offsets (g + 1,) int64)`` as :func:`group_pairs` returns them, under the ids of ``row_ids``.

    A group is a connected component of "score >= threshold", which is SINGLE LINKAGE: two members of one group are joined
    by a chain of pairs at or above the threshold and may score below it against each other.  The first member of a group is
    its smallest id; keeping that one per group is a deduplication.  A row that is in no pair is in no group.

    The join's pairs stay on the device and are grouped there.  ``corpus``, ``threshold``, ``row_ids``, ``max_pairs`` and the
    errors: those of ``exact_pairs_above``.  ``stats``: the join's (``rows``, ``emitted``, ``kept``, ...) and ``pairs``,
    ``grouped``, ``groups``, ``largest``."""
    jstats: Dict = {}
    joined = exact_pairs_above(corpus, threshold, row_ids=row_ids, max_pairs=max_pairs, return_tensors=True, stats=jstats)
    return _grouped(joined, jstats, return_tensors, stats)


def lsh_groups_above(corpus, threshold, codes, offsets, member_rows, num_bands: int, band_bytes: int, *, row_ids=None,
                     min_collisions: int = 1, max_bucket: Optional[int] = None, max_pairs: int = 1 << 26,
                     max_raw_pairs: int = 1 << 34, return_tensors: bool = False, stats: Optional[Dict] = None):
    """The near-duplicate GROUPS a banded index holds in its buckets at a cosine ``threshold``: the connected components of
    the graph whose edges are the pairs of :func:`lshrs_amd.lsh_pairs_above` with the same arguments - ``(members, offsets)``
    as :func:`group_pairs` returns them.

    A group is a connected component of "candidate pair with score >= threshold", which is SINGLE LINKAGE: two members of one
    group are joined by a chain of such pairs, and may neither collide nor score at the threshold against each other.  The
    first member of a group is its smallest id; keeping that one per group is a deduplication.  The pairs are a subset of
    ``exact_pairs_above``'s, so every group lies inside ONE group of :func:`exact_groups_above`.

    Arguments, keywords and errors: those of ``lsh_pairs_above``; the pairs stay on the device.  ``stats``: the join's and
    ``pairs``, ``grouped``, ``groups``, ``largest``."""
    jstats: Dict = {}
    joined = lsh_pairs_above(corpus, threshold, codes, offsets, member_rows, num_bands, band_bytes, row_ids=row_ids,
                             min_collisions=min_collisions, max_bucket=max_bucket, max_pairs=max_pairs,
                             max_raw_pairs=max_raw_pairs, return_tensors=True, stats=jstats)
    return _grouped(joined, jstats, return_tensors, stats)
