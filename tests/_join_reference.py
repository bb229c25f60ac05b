"""The LSH self-join in plain Python, for the tests: a dict from bucket code to the union of its members across segments,
oversized buckets dropped, a counter of shared counted bands per pair; the row map of one segment cell by cell; the
triangular index of a raw pair by integer arithmetic."""

from __future__ import annotations

import math
from collections import Counter
from itertools import combinations

import numpy as np


def hand_segment(buckets, bb=1):
    """``{code: [members]}`` as a segment (a ``BucketCSR``): the buckets by ascending code, the members as they are listed."""
    from lshrs_amd.packed_ops import BucketCSR

    codes = np.array(sorted(buckets), dtype=np.int64)
    lens = [len(buckets[c]) for c in codes.tolist()]
    members = np.array([m for c in codes.tolist() for m in buckets[c]], dtype=np.int64)
    return BucketCSR(bb, (codes >> 8 * bb).astype(np.int32), None, codes, np.r_[0, np.cumsum(lens)].astype(np.int64), members, 0)


def buckets_reference(segments):
    """``{code: set of members}``: every bucket of the segments, the union across them."""
    buckets = {}
    for seg in segments:
        for g, code in enumerate(seg.codes.tolist()):
            buckets.setdefault(code, set()).update(seg.members[seg.offsets[g]:seg.offsets[g + 1]].tolist())
    return buckets


def join_reference(segments, min_collisions=1, max_bucket=None):
    """``segments``: BucketCSR-likes (``codes``, ``offsets``, ``members``).  Returns ``({(a, b): collisions}, stats)`` for the
    pairs ``a < b`` of members that share a counted bucket (2 .. max_bucket members) in at least ``min_collisions`` bands - a
    code is one (band, key), so a pair meets at most once per band - and ``stats``: ``buckets``, ``skipped_buckets``,
    ``raw_pairs``."""
    buckets = buckets_reference(segments)
    shared, skipped, raw = Counter(), 0, 0
    for members in buckets.values():
        if max_bucket is not None and len(members) > max_bucket:
            skipped += 1
            continue
        raw += len(members) * (len(members) - 1) // 2
        shared.update(combinations(sorted(members), 2))
    pairs = {pair: n for pair, n in shared.items() if n >= min_collisions}
    return pairs, {"buckets": len(buckets), "skipped_buckets": skipped, "raw_pairs": raw}


def rowmap_reference(seg, n_rows, num_bands, band_bytes, max_bucket=None):
    """The row map of ONE segment whose members are rows: ``(n_rows, num_bands)`` int32, the cell ``[row, band]`` holding
    ``g`` where ``row`` is a member of bucket ``g`` of that band and the bucket has ``2 .. max_bucket`` entries (entries as
    the offsets count them), ``-1`` elsewhere.  What a valid segment never holds defines no cell: an entry whose row is
    outside ``[0, n_rows)``, a bucket whose band is outside ``[0, num_bands)``.  Where a row sits in two counted buckets of
    one band the cell keeps the FIRST of them (the kernel keeps whichever arrives first: the caller judges that cell)."""
    cells = np.full((int(n_rows), int(num_bands)), -1, dtype=np.int32)
    offsets, members = seg.offsets.tolist(), seg.members.tolist()
    for g, code in enumerate(seg.codes.tolist()):
        band, n = code >> (8 * band_bytes), offsets[g + 1] - offsets[g]
        if n < 2 or (max_bucket is not None and n > max_bucket) or not 0 <= band < num_bands:
            continue
        for row in members[offsets[g]:offsets[g + 1]]:
            if 0 <= row < n_rows and cells[row, band] == -1:
                cells[row, band] = g
    return cells


def pair_of(t):
    """The entries ``(i, j)``, ``i < j``, of raw pair ``t`` of a bucket: ``t == j (j - 1) // 2 + i``.  Integers only."""
    t = int(t)
    if t < 0:
        raise ValueError("a raw pair is not negative")
    j = (1 + math.isqrt(1 + 8 * t)) // 2            # the largest j with j (j - 1) / 2 <= t
    return t - j * (j - 1) // 2, j
