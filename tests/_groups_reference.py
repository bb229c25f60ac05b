"""Plain-Python reference of the near-duplicate groups (lshrs_amd.group_pairs): a union-find over (a, b) lists, returning
(members, offsets) in the order the package defines - groups by ascending smallest id, members ascending inside a group, only
ids that occur in a pair.  Every expected value of the group tests comes from here, never from the code under test; the file
itself is checked against scipy.sparse.csgraph.connected_components in tests/test_groups_host.py."""

from __future__ import annotations

import numpy as np


def groups_reference(ids_a, ids_b):
    """(members int64 (v,), offsets int64 (g + 1,)) of the pairs (ids_a[e], ids_b[e])."""
    a = [int(x) for x in np.asarray(ids_a).reshape(-1).tolist()]
    b = [int(x) for x in np.asarray(ids_b).reshape(-1).tolist()]
    assert len(a) == len(b)
    parent = {}

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for x, y in zip(a, b):
        parent.setdefault(x, x)
        parent.setdefault(y, y)
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    groups = {}
    for x in sorted(parent):
        groups.setdefault(find(x), []).append(x)
    members, offsets = [], [0]
    for root in sorted(groups):
        assert groups[root][0] == root
        members.extend(groups[root])
        offsets.append(len(members))
    return np.array(members, dtype=np.int64), np.array(offsets, dtype=np.int64)


def labels_reference(a, b, n):
    """int32 (n,): for every dense vertex the smallest vertex of its component under the edges (a[e], b[e]); edges with an
    endpoint outside [0, n) are left out."""
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    ok = (a >= 0) & (a < n) & (b >= 0) & (b < n)
    members, offsets = groups_reference(a[ok], b[ok])
    labels = np.arange(n, dtype=np.int32)
    for lo, hi in zip(offsets[:-1].tolist(), offsets[1:].tolist()):
        labels[members[lo:hi]] = members[lo]
    return labels


def group_lists(members, offsets):
    """[[id, ...], ...] of a (members, offsets) answer."""
    flat, at = np.asarray(members).tolist(), np.asarray(offsets).tolist()
    return [flat[lo:hi] for lo, hi in zip(at[:-1], at[1:])]


def removable(offsets) -> int:
    """The sum over the groups of size - 1: what a deduplication that keeps one id per group removes."""
    return int((np.diff(np.asarray(offsets)) - 1).sum())
