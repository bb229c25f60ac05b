"""The LSH self-join in plain Python, for the tests: a dict from bucket code to the union of its members across segments,
oversized buckets dropped, a counter of shared counted bands per pair."""

from __future__ import annotations

from collections import Counter
from itertools import combinations


def join_reference(segments, min_collisions=1, max_bucket=None):
    """``segments``: BucketCSR-likes (``codes``, ``offsets``, ``members``).  Returns ``({(a, b): collisions}, stats)`` for the
    pairs ``a < b`` of members that share a counted bucket (2 .. max_bucket members) in at least ``min_collisions`` bands - a
    code is one (band, key), so a pair meets at most once per band - and ``stats``: ``buckets``, ``skipped_buckets``,
    ``raw_pairs``."""
    buckets = {}
    for seg in segments:
        for g, code in enumerate(seg.codes.tolist()):
            buckets.setdefault(code, set()).update(seg.members[seg.offsets[g]:seg.offsets[g + 1]].tolist())
    shared, skipped, raw = Counter(), 0, 0
    for members in buckets.values():
        if max_bucket is not None and len(members) > max_bucket:
            skipped += 1
            continue
        raw += len(members) * (len(members) - 1) // 2
        shared.update(combinations(sorted(members), 2))
    pairs = {pair: n for pair, n in shared.items() if n >= min_collisions}
    return pairs, {"buckets": len(buckets), "skipped_buckets": skipped, "raw_pairs": raw}
