"""The LSH k-NN graph in plain Python, for the tests: the candidates of every id from ``_join_reference.join_reference``, a
score FUNCTION asked once per direction, and the order of the kernels' key - descending score, +0.0 ahead of -0.0, NaN last,
equal keys by ascending id."""

from __future__ import annotations

import numpy as np

from tests._join_reference import join_reference


def desc_key(score) -> int:
    """The orderable key of csrc/lshrs_rows.h of ONE float32 score: ascending key == descending score; integers only."""
    score = np.float32(score)
    if np.isnan(score):
        return 0xFFFFFFFF
    bits = int(score.view(np.uint32))
    return bits if bits & 0x80000000 else bits ^ 0x7FFFFFFF


def rank_list(entries, k):
    """``[(id, score), ...]`` in any order -> its best ``k`` in the kernels' order."""
    return sorted(entries, key=lambda e: (desc_key(e[1]), e[0]))[:k]


def candidates_reference(segments, min_collisions=1, max_bucket=None):
    """``({id: set of its candidates}, the join's stats)``: both directions of every pair of ``join_reference``."""
    pairs, stats = join_reference(segments, min_collisions=min_collisions, max_bucket=max_bucket)
    mates = {}
    for a, b in pairs:
        mates.setdefault(a, set()).add(b)
        mates.setdefault(b, set()).add(a)
    stats["emitted"] = len(pairs)
    return mates, stats


def knn_join_reference(segments, live_ids, k, score, min_collisions=1, max_bucket=None):
    """What ``lsh_knn`` returns, on the host: ``live_ids`` every id that has a row (any order), ``score(a, b)`` the float32
    score with id ``a`` asking and id ``b`` asked - called once per direction of every candidate pair.  Returns ``(ids (n,)
    int64 ascending, neighbors (n, kk) int64, scores (n, kk) float32, counts (n,) int32, stats)``; ``stats``: the join's and
    ``candidates_max``, ``short_rows``."""
    ids = np.sort(np.asarray(live_ids, dtype=np.int64))
    n = int(ids.shape[0])
    kk = max(0, min(int(k), n - 1))
    mates, stats = candidates_reference(segments, min_collisions, max_bucket)
    neighbors = np.full((n, kk), -1, dtype=np.int64)
    scores = np.full((n, kk), np.nan, dtype=np.float32)
    counts = np.zeros(n, dtype=np.int32)
    longest = short = 0
    for i, a in enumerate(ids.tolist()):
        mine = mates.get(a, ())
        longest, short = max(longest, len(mine)), short + (len(mine) < kk)
        best = rank_list([(b, np.float32(score(a, b))) for b in mine], kk)
        counts[i] = len(best)
        for j, (b, s) in enumerate(best):
            neighbors[i, j], scores[i, j] = b, s
    stats.update(candidates_max=longest, short_rows=short)
    return ids, neighbors, scores, counts, stats
