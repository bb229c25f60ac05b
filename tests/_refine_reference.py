"""The graph refinement in plain Python / NumPy, for the tests: which entries of a neighbour table are its undirected edges, the
sets ``C(r)`` of rows within two steps over an adjacency, and "``exact_knn`` with ``k = n - 1``, restricted to a set" - the
ranking a round of ``refine_knn`` must return, bit for bit."""

from __future__ import annotations

import numpy as np


def edges_reference(graph):
    """``keep`` (uint8, the table's shape) as include/lshrs_refine.h defines it: ``g = graph[r][c]`` is kept iff ``g >= 0``, no
    earlier column of row ``r`` holds ``g``, and not both ``g < r`` and row ``g`` lists ``r``.  Entries outside ``[-1,
    n_rows)`` and ``g == r`` are not kept and nothing is read through them."""
    graph = np.asarray(graph, dtype=np.int64)
    n_rows, k_in = graph.shape
    keep = np.zeros((n_rows, k_in), dtype=np.uint8)
    for r in range(n_rows):
        for c in range(k_in):
            g = int(graph[r, c])
            if g < 0 or g >= n_rows or g == r:
                continue
            if g in graph[r, :c].tolist():
                continue
            if g < r and r in graph[g].tolist():
                continue
            keep[r, c] = 1
    return keep


def adjacency_of(graph):
    """``[sorted A(r)]`` of the table read as an undirected graph: the lists ``pair_adjacency`` makes of the kept entries."""
    graph = np.asarray(graph, dtype=np.int64)
    keep = edges_reference(graph)
    lists = [set() for _ in range(graph.shape[0])]
    for r, c in zip(*np.nonzero(keep)):
        g = int(graph[r, c])
        lists[int(r)].add(g)
        lists[g].add(int(r))
    return [sorted(x) for x in lists]


def csr_of(lists):
    """``(nbr, row_off)`` int64 of lists laid end to end."""
    lens = np.array([len(x) for x in lists], dtype=np.int64)
    nbr = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists]) if len(lists) else np.zeros(0, np.int64)
    return nbr.astype(np.int64), np.r_[0, np.cumsum(lens)].astype(np.int64)


def bound_reference(lists, max_degree=None):
    """``U(r) = deg(r) + sum of deg(m) over the midpoints m of r``, per row: what decides a row's tier."""
    n = len(lists)
    out = []
    for r in range(n):
        mids = [m for m in lists[r] if 0 <= m < n and (max_degree is None or len(lists[m]) <= max_degree)]
        out.append(len(lists[r]) + sum(len(lists[m]) for m in mids))
    return out


def expand_reference(lists, max_degree=None):
    """``[C(r)]`` as sets over the adjacency ``lists`` (one list per row; entries outside ``[0, n)`` are skipped): ``A(r)`` and
    ``A(m)`` for every ``m`` in ``A(r)`` with ``len(A(m)) <= max_degree`` (None: every one), without ``r``."""
    n = len(lists)
    arrays = [np.asarray(x, dtype=np.int64).reshape(-1) for x in lists]
    arrays = [x[(x >= 0) & (x < n)] for x in arrays]
    out = []
    for r in range(n):
        parts = [arrays[r]] + [arrays[m] for m in arrays[r].tolist() if max_degree is None or len(lists[m]) <= max_degree]
        mine = set(np.unique(np.concatenate(parts)).tolist())
        mine.discard(r)
        out.append(mine)
    return out


def restricted_reference(full_ids, full_nbrs, full_scores, allowed, k):
    """``exact_knn(corpus, n - 1)`` - ``full_ids`` (n,), ``full_nbrs`` / ``full_scores`` (n, n - 1): every other id in the
    exact order - restricted per id to ``allowed[id]`` (a set of ids) and cut at ``k``: ``(neighbors (n, kk), scores (n, kk),
    counts (n,))`` in ``lsh_knn``'s form, ``kk = min(k, n - 1)``."""
    n = int(full_ids.shape[0])
    kk = max(0, min(int(k), n - 1))
    nbrs = np.full((n, kk), -1, dtype=np.int64)
    scores = np.full((n, kk), np.nan, dtype=np.float32)
    counts = np.zeros(n, dtype=np.int32)
    for i, a in enumerate(full_ids.tolist()):
        want = allowed.get(a, ()) if isinstance(allowed, dict) else allowed[i]
        at = [j for j, b in enumerate(full_nbrs[i].tolist()) if b in want][:kk]
        counts[i] = len(at)
        nbrs[i, :len(at)], scores[i, :len(at)] = full_nbrs[i, at], full_scores[i, at]
    return nbrs, scores, counts
