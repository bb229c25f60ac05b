"""The host side of a query, as plain functions: what ``LSHRS.query`` / ``query_many`` do between the signature pass and the
rerank that needs neither the index object nor a device - reading buckets through the reference's storage interface,
counting and ordering candidates (lshrs/core/main.py:1088-1111, :614), checking and applying the ``top_k`` / ``top_p`` cut
(:617-657) and stacking fetched vectors (:629-646).  Beside ``_query_device.py``, which does the same on the device."""

from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np


def ragged_positions(starts: np.ndarray, lens: np.ndarray) -> np.ndarray:
    """Concatenation of ``arange(starts[i], starts[i] + lens[i])`` over i."""
    total = int(lens.sum())
    return np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens) + np.repeat(starts, lens)


def split_rows(flat: list, lens: np.ndarray) -> List[list]:
    """A flat Python list cut into consecutive pieces of the given lengths."""
    ends = np.cumsum(lens).tolist()
    return [flat[lo:hi] for lo, hi in zip([0] + ends[:-1], ends)]


def bucket_pairs(store, keys: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Flat ``(query, band, member)`` arrays, query-major, from one ``get_bucket`` per (query, band) - the reference's storage
    interface (lshrs/storage/redis.py:282).  ``keys``: (q, bands, B) uint8."""
    qs, bs, ms = [], [], []
    for qi in range(keys.shape[0]):
        for band_id in range(keys.shape[1]):
            mem = store.get_bucket(band_id, keys[qi, band_id].tobytes())
            if mem:
                ms.append(np.fromiter((int(v) for v in mem), dtype=np.int64, count=len(mem)))
                qs.append(np.full(len(mem), qi, dtype=np.int64))
                bs.append(np.full(len(mem), band_id, dtype=np.int32))
    if not ms:
        return np.empty(0, np.int64), np.empty(0, np.int32), np.empty(0, np.int64)
    return np.concatenate(qs), np.concatenate(bs), np.concatenate(ms)


def order_candidates(q: np.ndarray, m: np.ndarray, nq: int, num_bands: int) -> Tuple[np.ndarray, np.ndarray]:
    """For every query: the stored ids that share at least one band bucket with it, ordered by (-collisions, id) -
    ``_candidate_counts`` + the sort of ``query`` (lshrs/core/main.py:1088-1111, :614) for a whole batch, as array
    work: from flat (query, member) pairs - one per (query, band, member) - one sort counts the collisions, one orders the
    candidates.  Returns ``(ids, bounds)``: query ``i``'s candidates are ``ids[bounds[i]:bounds[i + 1]]``.  No Python
    object per member."""
    if q.size == 0:
        return np.empty(0, np.int64), np.zeros(nq + 1, dtype=np.int64)
    qbits, cbits = max(1, int(nq - 1).bit_length()), int(num_bands).bit_length()
    mbits = 63 - qbits - cbits
    if int(m.min()) >= 0 and int(m.max()) < (1 << mbits):
        # one 64-bit key per pair: (query, member), then (query, bands - collisions, member): two plain sorts
        pair = np.sort((q << mbits) | m)
        first = np.r_[True, pair[1:] != pair[:-1]]
        starts = np.flatnonzero(first)
        counts = np.diff(np.r_[starts, pair.shape[0]])     # (one pair per (query, band, member): the lookup's contract)
        uniq = pair[starts]
        uq, um = uniq >> mbits, uniq & ((1 << mbits) - 1)
        ranked = np.sort((uq << (mbits + cbits)) | ((num_bands - counts) << mbits) | um)
        uq, um = ranked >> (mbits + cbits), ranked & ((1 << mbits) - 1)
    else:
        order = np.lexsort((m, q))                           # by query, then member
        q, m = q[order], m[order]
        first = np.r_[True, (q[1:] != q[:-1]) | (m[1:] != m[:-1])]
        starts = np.flatnonzero(first)
        counts = np.diff(np.r_[starts, q.shape[0]])
        uq, um = q[starts], m[starts]
        rank = np.lexsort((um, -counts, uq))                 # by query, then -collisions, then id
        uq, um = uq[rank], um[rank]
    return um, np.searchsorted(uq, np.arange(nq + 1)).astype(np.int64)


def check_cut(top_k: Optional[int], top_p: Optional[float]) -> None:
    """The reference's argument errors (lshrs/core/main.py:617-625, :653-656): ``top_p`` first, then ``top_k``."""
    if top_p is not None and not 0 < top_p <= 1:
        raise ValueError("top_p must be within the range (0, 1]")
    if top_k is not None and top_k <= 0:
        raise ValueError("top_k must be greater than zero when provided")


def keep_counts(lens, top_k: Optional[int], top_p: Optional[float]) -> np.ndarray:
    """How many of each list's ``lens`` ranked candidates the answer keeps: ``max(1, ceil(n * top_p))`` of a non-empty list
    (all of it without ``top_p``), at most ``top_k`` (lshrs/core/main.py:619-622, :652-657)."""
    lens = np.asarray(lens, dtype=np.int64)
    keep = lens if top_p is None else np.where(lens > 0, np.maximum(1, np.ceil(lens * top_p).astype(np.int64)), 0)
    return keep if top_k is None else np.minimum(keep, top_k)


def fetch_checked(fetch, dim: int, ids: list) -> np.ndarray:
    """``fetch(ids)`` as a ``(len(ids), dim)`` float32 array (lshrs/core/main.py:629-646)."""
    got = np.asarray(fetch(ids), dtype=np.float32)
    if got.ndim != 2 or got.shape[1] != dim:
        raise ValueError(f"Fetched vectors must have shape (n, {dim}); received {got.shape}")
    if got.shape[0] != len(ids):
        raise ValueError("vector_fetch_fn returned mismatched batch size "
                         f"(expected {len(ids)}, received {got.shape[0]})")
    return got


def fetch_table(fetch, dim: int, ids: np.ndarray, bounds: np.ndarray) -> np.ndarray:
    """The vectors of every candidate as one ``(len(ids), dim)`` float32 table - row j is the vector of ``ids[j]`` - fetched
    list by list (``ids[bounds[i]:bounds[i + 1]]``; empty lists skipped, at least one is not) as the reference does (main.py:629)."""
    return np.concatenate([fetch_checked(fetch, dim, ids[bounds[i]:bounds[i + 1]].tolist())
                           for i in np.flatnonzero(np.diff(bounds))], axis=0)
