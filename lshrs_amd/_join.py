"""The LSH self-join - ``lsh_pairs_above`` - and what it is made of: the near-duplicate pairs a banded index holds in its
buckets, reranked.  The approximate member of the family whose ground truth is ``exact_pairs_above``.

The pair ``{a, b}`` of distinct members is a CANDIDATE when a and b share a bucket in at least ``min_collisions`` bands;
buckets of more than ``max_bucket`` members count in no role.  The candidates come out of ONE bucket segment - ``codes``
ascending, ``offsets``, and for every entry of its member list the corpus row that holds the member's vector
(``member_rows``) - by two kernels of ``csrc/join.hip``:

row map   ``lshrs_join_rowmap_i64``: for every (row, band) the counted bucket the row is a member of.  A row in two different
          buckets of one band - an id indexed under two signatures and never deleted, which has one stored vector at most - is
          refused with ``ValueError`` before any pair is emitted.
emit      ``lshrs_join_emit_i64``: one lane per RAW pair (the ``len (len - 1) / 2`` pairs of every counted bucket, numbered
          through a prefix sum ``torch.cumsum`` makes), in launches of at most ``_EMIT_SLICE`` raw pairs.  The map tells in
          which bands a pair collides; it leaves only from the first of them: every candidate once, with its collision count,
          and the emitted count is the number of distinct candidate pairs.

What the emit lets through is judged by ``_exact._judge_pairs`` - the text ``exact_pairs_above`` judges its own first pass
with: for ``min_collisions = 1`` and no ``max_bucket`` the answer is ``exact_pairs_above``'s restricted to the candidate pairs,
scores bit for bit.

No CPU compute path: the host folds segments (array work, :func:`fold_segments`), reads one count per launch and keeps
statistics.
"""

from __future__ import annotations

import time
from typing import Dict, Optional

import numpy as np

from . import _native
from ._exact import _all_pairs, _check_max_pairs, _check_pairs_args, _finish, _judge_pairs, _rows_args
from .similarity import _on_device, corpus_suffix
from .vectors import NO_VECTOR_MSG

__all__ = ["lsh_pairs", "lsh_pairs_above", "fold_segments", "check_join_args"]

# slots of the first emit: pairs of 20 bytes; more candidates than that cost a second emit
_JOIN_FIRST_CAPACITY = 1 << 20
# raw pairs of one emit launch (what lshrs_join_emit_i64 takes at most): a larger join is several launches
_EMIT_SLICE = 1 << 31
_NO_MAX_BUCKET = (1 << 62)

TWO_SIGNATURES_MSG = ("an id sits in two different buckets of one band: it was indexed under two signatures and never deleted, "
                      "and has one stored vector at most - delete() it before it is indexed again")
OUT_OF_RANGE_MSG = "candidate index out of range of the corpus"


def check_join_args(threshold, min_collisions, max_bucket, max_pairs, num_bands: int, max_raw_pairs=0) -> float:
    """The threshold of a join as a float; ``ValueError`` for what ``lsh_pairs_above`` / ``LSHRS.pairs_above`` do not take:
    what :func:`_exact._check_pairs_args` refuses, a ``min_collisions`` that is no integer of ``1 .. num_bands``, a
    ``max_bucket`` that is neither None nor an integer ``>= 2``, a negative ``max_raw_pairs``.  Pure host."""
    t = _check_pairs_args(threshold, max_pairs)
    if isinstance(min_collisions, bool) or not isinstance(min_collisions, (int, np.integer)) or \
            not 1 <= int(min_collisions) <= int(num_bands):
        raise ValueError(f"min_collisions must be an integer in 1..{int(num_bands)}; received {min_collisions!r}")
    if max_bucket is not None and (isinstance(max_bucket, bool) or not isinstance(max_bucket, (int, np.integer))
                                   or int(max_bucket) < 2):
        raise ValueError(f"max_bucket must be None or an integer >= 2; received {max_bucket!r}")
    if int(max_raw_pairs) < 0:
        raise ValueError(f"max_raw_pairs must be >= 0; received {max_raw_pairs}")
    return t


def fold_segments(segments):
    """Several array segments (``packed_ops.BucketCSR`` with codes, one key width) as ONE: ``packed_ops.merge_csr`` - set
    semantics, an id once per bucket - or the segment itself where there is one (empty segments are nobody's).  Returns
    ``(segment or None, fold_ms, folded)``: host array work, timed; ``folded``: the segments merged, 0 where nothing was."""
    from .packed_ops import merge_csr

    segs = [s for s in segments if len(s)]
    if not segs:
        return None, 0.0, 0
    if len(segs) == 1:
        return segs[0], 0.0, 0
    t0 = time.perf_counter()
    one = merge_csr(segs)
    return one, (time.perf_counter() - t0) * 1e3, len(segs)


class _Plan:
    """A join between its two kernels: the row map, the raw pairs' prefix, the counts."""

    __slots__ = ("offsets", "prefix", "member_rows", "rowmap", "n_codes", "n_rows", "num_bands", "min_collisions", "raw_pairs",
                 "buckets", "skipped_buckets", "err", "launches")


def _plan(codes, offsets, member_rows, n_rows: int, num_bands: int, band_bytes: int, min_collisions: int, max_bucket) -> _Plan:
    """The first kernel and the plumbing around it: the ends of the offsets checked against ``member_rows`` (read back before
    the launch), the prefix sum of the counted buckets' pair counts, the row map, and what is read back behind it - the error
    bits, the raw pairs, the oversized buckets."""
    torch = _native.require_gpu()
    lib = _native.load()
    dev = offsets.device
    plan = _Plan()
    n_codes, n_members = int(codes.shape[0]), int(member_rows.shape[0])
    limit = _NO_MAX_BUCKET if max_bucket is None else int(max_bucket)
    with torch.cuda.device(dev):
        # (before anything is launched: the kernels bisect on the offsets and index member_rows through them)
        ends = torch.stack((offsets[0], offsets[-1])).cpu().tolist()
        if int(ends[0]) != 0 or int(ends[1]) != n_members:
            raise ValueError(f"offsets must run from 0 to the {n_members} entries of member_rows; received {ends[0]} .. {ends[1]}")
        lens = torch.diff(offsets)
        counted = (lens >= 2) & (lens <= limit)
        pairs = torch.where(counted, lens * (lens - 1) // 2, torch.zeros_like(lens))
        prefix = torch.zeros(n_codes + 1, dtype=torch.int64, device=dev)
        prefix[1:] = torch.cumsum(pairs, 0)
        nbytes = int(lib.lshrs_join_workspace_bytes(int(n_rows), int(num_bands)))
        if nbytes < 0:
            _native.check(nbytes, "lshrs_join_workspace_bytes")
        rowmap = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.check(lib.lshrs_join_rowmap_i64(codes.data_ptr(), offsets.data_ptr(), n_codes, int(band_bytes), int(num_bands),
                                                member_rows.data_ptr(), n_members, int(n_rows), limit, rowmap.data_ptr(),
                                                err.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                      "lshrs_join_rowmap_i64")
        # one copy back: the error bits, the raw pairs, the oversized buckets
        got = torch.stack((err[0].long(), prefix[-1], (lens > limit).sum())).cpu().tolist()
    plan.offsets, plan.prefix, plan.member_rows, plan.rowmap, plan.err = offsets, prefix, member_rows, rowmap, err
    plan.n_codes, plan.n_rows, plan.num_bands, plan.min_collisions = n_codes, int(n_rows), int(num_bands), int(min_collisions)
    plan.raw_pairs, plan.buckets, plan.skipped_buckets, plan.launches = int(got[1]), n_codes, int(got[2]), 0
    plan.err.fill_(0)
    bits = int(got[0])
    if bits & 256:
        raise IndexError(NO_VECTOR_MSG)
    if bits & 512:
        raise IndexError(OUT_OF_RANGE_MSG)
    if bits & 2:
        raise ValueError(f"a bucket's band lies outside the index's {int(num_bands)} bands")
    if bits & 1:
        raise ValueError("lsh join: " + TWO_SIGNATURES_MSG)
    return plan


def _emit(plan: _Plan, capacity: int):
    """The second kernel over all raw pairs, ``_EMIT_SLICE`` of them per launch, into arrays of ``capacity`` slots:
    ``(a, b, collisions, total, err)`` as ``scan_pairs`` returns its five (``err`` stays zero: the map was checked)."""
    torch = _native.require_gpu()
    lib = _native.load()
    dev = plan.offsets.device
    capacity = int(capacity)
    with torch.cuda.device(dev):
        a = torch.empty((capacity,), dtype=torch.int64, device=dev)
        b = torch.empty((capacity,), dtype=torch.int64, device=dev)
        hits = torch.empty((capacity,), dtype=torch.int32, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        outs = [t.data_ptr() if capacity else None for t in (a, b, hits)]
        for begin in range(0, plan.raw_pairs, _EMIT_SLICE):
            count = min(_EMIT_SLICE, plan.raw_pairs - begin)
            _native.check(lib.lshrs_join_emit_i64(plan.offsets.data_ptr(), plan.prefix.data_ptr(), plan.n_codes,
                                                  plan.member_rows.data_ptr(), plan.n_rows, plan.num_bands, plan.rowmap.data_ptr(),
                                                  begin, count, plan.min_collisions, capacity, *outs, total.data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream), "lshrs_join_emit_i64")
            plan.launches += 1
    return a, b, hits, total, plan.err


def _segment_args(torch, codes, offsets, member_rows, dev):
    """The segment as contiguous int64 tensors on ``dev``; ``ValueError`` where the shapes do not fit each other."""
    codes, offsets, member_rows = (_on_device(torch, t, np.int64).to(device=dev, dtype=torch.int64).contiguous()
                                   for t in (codes, offsets, member_rows))
    if codes.dim() != 1 or offsets.dim() != 1 or member_rows.dim() != 1 or int(offsets.shape[0]) != int(codes.shape[0]) + 1:
        raise ValueError("a segment is codes (g,), offsets (g + 1,) and member_rows (entries,)")
    return codes, offsets, member_rows


def lsh_pairs(codes, offsets, member_rows, n_rows: int, num_bands: int, band_bytes: int, *, min_collisions: int = 1,
              max_bucket: Optional[int] = None, capacity: int):
    """Device-level entry of the join's two kernels.  The segment: ``codes`` int64 ``(g,)`` ascending (``band << 8 band_bytes |
    key``), ``offsets`` int64 ``(g + 1,)``, ``member_rows`` int64 ``(offsets[-1],)`` - for every entry of the member list its
    row of a corpus of ``n_rows`` rows, every row at most once per bucket - all on one device.  Returns ``((a, b, collisions,
    total, err), raw_pairs)``: the first ``min(total, capacity)`` slots of ``a`` / ``b`` (int64 rows, ``a < b``) and
    ``collisions`` (int32) are the candidate pairs, each once, in no particular order; ``total`` (int64[1]) counts every one of
    them; ``raw_pairs``: the pairs the counted buckets hold, with repetitions.  Raises what :func:`lsh_pairs_above` raises
    for a member without a row and for a row in two buckets of one band."""
    if int(capacity) < 0:
        raise ValueError(f"capacity must be >= 0; received {capacity}")
    check_join_args(0.0, min_collisions, max_bucket, 0, num_bands)
    torch = _native.require_gpu()
    on_gpu = isinstance(offsets, torch.Tensor) and offsets.is_cuda
    dev = offsets.device if on_gpu else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        codes, offsets, member_rows = _segment_args(torch, codes, offsets, member_rows, dev)
        plan = _plan(codes, offsets, member_rows, n_rows, num_bands, band_bytes, min_collisions, max_bucket)
        return _emit(plan, capacity), plan.raw_pairs


def lsh_pairs_above(corpus, threshold, codes, offsets, member_rows, num_bands: int, band_bytes: int, *, row_ids=None,
                    min_collisions: int = 1, max_bucket: Optional[int] = None, max_pairs: int = 1 << 26,
                    max_raw_pairs: int = 1 << 34, return_tensors: bool = False, stats: Optional[Dict] = None):
    """Every candidate pair of a bucket segment at or above a cosine ``threshold``: ``(ids_a (p,) int64, ids_b (p,) int64,
    scores (p,) float32, collisions (p,) int32)`` with ``ids_a < ids_b``, scores descending, equal scores by ascending
    ``(ids_a, ids_b)``; NumPy arrays, or device tensors with ``return_tensors``.

    ``corpus``, ``row_ids``: as :func:`lshrs_amd.exact_pairs_above` takes them.  ``codes`` / ``offsets`` / ``member_rows``: ONE
    bucket segment as :func:`lsh_pairs` takes it, on the corpus's device (or array-likes, which are uploaded).  A pair is a
    candidate when its members share a bucket of ``2 .. max_bucket`` entries in at least ``min_collisions`` bands
    (``collisions``: in how many); it is in the answer when its RERANK score - oriented as ``exact_pairs_above`` defines it, the
    row of the lower id as the query - reaches ``float32(threshold)``.  For ``min_collisions = 1`` and no ``max_bucket`` the
    answer is ``exact_pairs_above``'s restricted to the candidate pairs, scores bit for bit.

    Capacity as in ``exact_pairs_above``: a first emit with ``2^20`` slots, a second with room for all, ``ValueError`` beyond
    ``max_pairs``.  More than ``max_raw_pairs`` raw pairs (a few huge buckets: their pairs grow with the square) raise
    ``ValueError`` before the emit is launched: set ``max_bucket``.
    ``stats``: a dict that receives ``buckets``, ``skipped_buckets`` (more than ``max_bucket`` entries), ``raw_pairs``,
    ``emitted`` (distinct candidate pairs), ``kept`` and ``launches`` (emit launches).

    A member without a row raises ``IndexError``; a row in two different buckets of one band raises ``ValueError`` (an id
    indexed under two signatures), both before any pair is emitted; a row of zero norm among the candidates raises
    ``ValueError("Cannot normalize zero vector")``."""
    max_pairs, max_raw_pairs = int(max_pairs), int(max_raw_pairs)
    _check_max_pairs(max_pairs)
    t = check_join_args(threshold, min_collisions, max_bucket, max_pairs, num_bands, max_raw_pairs)
    torch = _native.require_gpu()
    _native.load()
    corpus_suffix(corpus)
    dev = corpus.device
    with torch.cuda.device(dev):
        d_ids = _rows_args(torch, corpus, row_ids, "lsh_pairs_above")
        codes, offsets, member_rows = _segment_args(torch, codes, offsets, member_rows, dev)
        m = int(corpus.shape[0])
        out = {"buckets": int(codes.shape[0]), "skipped_buckets": 0, "raw_pairs": 0, "emitted": 0, "kept": 0, "launches": 0}
        ids_a = torch.empty((0,), dtype=torch.int64, device=dev)
        ids_b = torch.empty((0,), dtype=torch.int64, device=dev)
        scores = torch.empty((0,), dtype=torch.float32, device=dev)
        collisions = torch.empty((0,), dtype=torch.int32, device=dev)
        if int(member_rows.shape[0]):
            plan = _plan(codes, offsets, member_rows, m, num_bands, band_bytes, min_collisions, max_bucket)
            out["skipped_buckets"], out["raw_pairs"] = plan.skipped_buckets, plan.raw_pairs
            if plan.raw_pairs > max_raw_pairs:
                raise ValueError(f"lsh_pairs_above: the buckets hold {plan.raw_pairs} raw pairs, more than max_raw_pairs = "
                                 f"{max_raw_pairs}: set max_bucket to leave the largest buckets out")
            if plan.raw_pairs:
                last = []

                def launch(cap):
                    last[:] = [_emit(plan, cap)]
                    return last[0]

                pa, pb, emitted = _all_pairs(launch, min(_JOIN_FIRST_CAPACITY, max_pairs), max_pairs, "lsh_pairs_above", out)
                out["launches"] = plan.launches
                if emitted:
                    ids_a, ids_b, scores, index = _judge_pairs(torch, corpus, d_ids, pa[:emitted], pb[:emitted],
                                                               float(np.float32(t)))
                    collisions = last[0][2][:emitted][index].contiguous()
                    out["kept"] = int(ids_a.shape[0])
    return _finish(stats, out, (ids_a, ids_b, scores, collisions), return_tensors)
