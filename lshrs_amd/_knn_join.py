"""The LSH k-NN graph - ``lsh_knn`` - and what it is made of: for every stored row the ``k`` best of the rows it shares a
bucket with, reranked.  The approximate member of the family whose ground truth is ``exact_knn``.

The candidates of row ``i`` are the rows it forms a CANDIDATE PAIR with, exactly as the LSH self-join defines one
(``_join.py``): the two share a counted bucket in at least ``min_collisions`` bands.  The pairs come from the join's own two
kernels (``_join._plan`` / ``_join._emit``: every pair once, in no order); what this module adds stands behind them, in
``csrc/graph.hip`` (``include/lshrs_graph.h``, ``liblshrs_graph.so``):

adjacency  ``lshrs_graph_degree_i64``, ``torch.cumsum``, ``lshrs_graph_fill_i64``: the undirected pairs as one list per row.
           The order INSIDE a list is the order the lanes' atomics arrived in, and differs from run to run.
rerank     ``lshrs_cosine_ragged_*`` over the lists as they lie, consecutive rows as float32 queries: every pair is scored
           TWICE, once per direction, because the score is oriented (``exact_knn``: the asking row is the query) and the two
           directions may differ in the last bit.
select     ``lshrs_graph_select_f32``: per row the best ``k`` by (score descending, id ascending).  The id breaks every tie, so
           the answer is the same whatever order the adjacency left.

No CPU compute path: the host checks arguments, reads the counts the join reads and the error words back, and keeps
statistics.
"""

from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from . import _join, _native
from ._exact import (_PAIRS_QUERY_BYTES, _all_pairs, _check_max_pairs, _check_selection, _finish, _live_by_id, _rows_args,
                     _rows_as_f32)
from .similarity import _on_device, corpus_suffix, cosine_ragged_device

__all__ = ["lsh_knn", "pair_adjacency", "select_neighbors", "graph_max_list", "graph_wave_list"]

ENDPOINT_MSG = "an endpoint of a pair lies outside [0, n_rows)"
LOOP_MSG = "a pair joins a row with itself"


def graph_max_list() -> int:
    """The longest list ``lshrs_graph_select_f32`` selects from on the device."""
    return int(_native.load_graph().lshrs_graph_max_list())


def graph_wave_list() -> int:
    """The longest list ONE WAVE of ``lshrs_graph_select_f32`` sorts; longer ones take a workgroup."""
    return int(_native.load_graph().lshrs_graph_wave_list())


def _check_k(k) -> int:
    """``k`` as ``exact_knn`` checks it (``ValueError`` for ``k <= 0``), and no ``bool``.  Pure host."""
    if isinstance(k, bool):
        raise ValueError(f"k must be an integer > 0; received {k!r}")
    return _check_selection(k, "auto")


def pair_adjacency(a, b, n_rows: int):
    """Device-level entry of degree, prefix and fill: the undirected pairs ``(a[p], b[p])`` over the rows ``[0, n_rows)`` -
    contiguous int64 tensors of equal length on one device - as one list per row.  Returns ``(nbr (2 p,) int64, row_off
    (n_rows + 1,) int64, err int32[1])``: row ``r`` owns ``nbr[row_off[r]:row_off[r + 1]]``, the other ends of its pairs IN NO
    PARTICULAR ORDER (the order the lanes' atomic adds arrived in: it differs from run to run and nothing may depend on it).
    ``err``: bit 0 - an endpoint outside ``[0, n_rows)``, bit 1 - a pair with ``a == b``; such a pair is in no list and the
    tail of ``nbr`` behind ``row_off[-1]`` is then not written.  Nothing is read back here."""
    torch = _native.require_gpu()
    lib = _native.load_graph()
    dev = a.device
    n_pairs, n_rows = int(a.shape[0]), int(n_rows)
    if int(b.shape[0]) != n_pairs or a.dtype != torch.int64 or b.dtype != torch.int64:
        raise ValueError("a and b must be int64 tensors of equal length")
    a, b = a.contiguous(), b.contiguous()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        degree = torch.zeros((n_rows,), dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.check(lib.lshrs_graph_degree_i64(a.data_ptr(), b.data_ptr(), n_pairs, n_rows, degree.data_ptr(), err.data_ptr(),
                                                 stream), "lshrs_graph_degree_i64")
        row_off = torch.zeros((n_rows + 1,), dtype=torch.int64, device=dev)
        row_off[1:] = torch.cumsum(degree, 0, dtype=torch.int64)
        nbr = torch.empty((2 * n_pairs,), dtype=torch.int64, device=dev)
        degree.zero_()                              # (the counts are in row_off: the same words serve as the cursors)
        _native.check(lib.lshrs_graph_fill_i64(a.data_ptr(), b.data_ptr(), n_pairs, n_rows, row_off.data_ptr(),
                                               degree.data_ptr(), nbr.data_ptr(), stream), "lshrs_graph_fill_i64")
    return nbr, row_off, err


def _desc_key(torch, scores):
    """The orderable key of ``csrc/lshrs_rows.h`` as an int64 in ``[0, 2^32)``: ascending key == descending score, +0.0 ahead of
    -0.0, NaN last - the order ``lshrs_topk_desc_f32`` and ``lshrs_graph_select_f32`` sort by."""
    bits = scores.contiguous().view(torch.int32).long() & 0xFFFFFFFF
    key = torch.where(bits >= 0x80000000, bits, bits ^ 0x7FFFFFFF)
    return torch.where(torch.isnan(scores), torch.full_like(key, 0xFFFFFFFF), key)


def _ragged(torch, begin, lens):
    """For lists that begin at ``begin`` and hold ``lens`` entries (int64 tensors): ``(slot, at)`` - for every entry of all of
    them laid end to end, the list it belongs to and its position in the array the lists lie in."""
    dev = begin.device
    slot = torch.repeat_interleave(torch.arange(int(begin.shape[0]), dtype=torch.int64, device=dev), lens)
    first = torch.cumsum(lens, 0) - lens
    at = begin[slot] + (torch.arange(int(slot.shape[0]), dtype=torch.int64, device=dev) - first[slot])
    return slot, at


def _rank_long(torch, nbr, scores, row_off, row_ids, k: int, rows, out_ids, out_scores, out_count) -> None:
    """The lists of ``rows`` (int64, ascending: those the kernel left at -1) ranked with torch's stable sorts, the way
    ``_exact._judge_pairs`` orders its pairs: ascending id first, then ONE stable sort on {row, key of the score} - every list
    in the kernel's order.  All of them in one go: a list is a run of the sorted array."""
    dev = nbr.device
    begin = row_off[rows]
    lens = row_off[rows + 1] - begin
    slot, at = _ragged(torch, begin, lens)
    first = torch.cumsum(lens, 0) - lens                         # where every list begins among the gathered entries
    ids, sc = nbr[at], scores[at]
    if row_ids is not None:
        ids = row_ids[ids]
    _, order = torch.sort(ids, stable=True)
    slot, ids, sc = slot[order], ids[order], sc[order]
    _, order = torch.sort((slot << 32) | _desc_key(torch, sc), stable=True)
    ids, sc = ids[order], sc[order]
    take = first.unsqueeze(1) + torch.arange(k, dtype=torch.int64, device=dev).unsqueeze(0)       # (rows, k)
    have = torch.arange(k, dtype=torch.int64, device=dev).unsqueeze(0) < lens.unsqueeze(1)
    take = torch.where(have, take, torch.zeros_like(take))
    out_ids[rows] = torch.where(have, ids[take], torch.full_like(take, -1))
    out_scores[rows] = torch.where(have, sc[take], torch.full(take.shape, float("nan"), dtype=torch.float32, device=dev))
    out_count[rows] = torch.clamp(lens, max=k).to(torch.int32)


def select_neighbors(nbr, scores, row_off, row_ids, k: int, stats: Optional[Dict] = None):
    """Device-level entry of the select: row ``r`` owns the entries ``[row_off[r], row_off[r + 1])`` of ``nbr`` (int64) and
    ``scores`` (float32); the id of an entry is ``row_ids[nbr]`` (int64 tensor), or ``nbr`` itself where ``row_ids`` is None.
    Returns ``(ids (n_rows, k) int64, scores (n_rows, k) float32, count (n_rows,) int32)``: per row its best ``count = min(k,
    len)`` entries in the order of ``lshrs_topk_desc_f32`` - score descending, +0.0 ahead of -0.0, NaN last - EQUAL SCORES BY
    ASCENDING ID, then ``-1`` / ``NaN``.  The answer is the same for every order of the entries inside a list.

    Lists of more than :func:`graph_max_list` entries are left at ``count = -1`` by the kernel and ranked here with torch's
    stable sorts, in the same order; ``stats["long_lists"]`` counts them.  One word is read back: the kernel's error bits,
    which raise ``NativeLibraryError`` - a list outside ``nbr``, an entry outside ``row_ids`` - and beside it that count."""
    k = _check_k(k)
    torch = _native.require_gpu()
    lib = _native.load_graph()
    dev = row_off.device
    n_rows, total = int(row_off.shape[0]) - 1, int(nbr.shape[0])
    if n_rows < 0 or int(scores.shape[0]) < total:
        raise ValueError("row_off must have n_rows + 1 entries and scores one entry per entry of nbr")
    nbr, scores, row_off = nbr.contiguous(), scores.contiguous(), row_off.contiguous()
    if row_ids is not None:
        row_ids = row_ids.contiguous()
    with torch.cuda.device(dev):
        out_ids = torch.empty((n_rows, k), dtype=torch.int64, device=dev)
        out_scores = torch.empty((n_rows, k), dtype=torch.float32, device=dev)
        out_count = torch.empty((n_rows,), dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.check(lib.lshrs_graph_select_f32(nbr.data_ptr() if total else None, scores.data_ptr() if total else None,
                                                 row_off.data_ptr(), n_rows, total,
                                                 row_ids.data_ptr() if row_ids is not None else None,
                                                 int(row_ids.shape[0]) if row_ids is not None else 0, k, out_ids.data_ptr(),
                                                 out_scores.data_ptr(), out_count.data_ptr(), err.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream), "lshrs_graph_select_f32")
        got = torch.stack((err[0].long(), (out_count < 0).sum())).cpu().tolist() if n_rows else [0, 0]
        if int(got[0]) & _native.GRAPH_ERR_RANGE:
            raise _native.NativeLibraryError("lshrs_graph_select_f32: a row's list does not lie within nbr "
                                             "(LSHRS_GRAPH_ERR_RANGE)")
        if int(got[0]) & _native.GRAPH_ERR_ENTRY:
            raise _native.NativeLibraryError("lshrs_graph_select_f32: an entry of nbr lies outside row_ids "
                                             "(LSHRS_GRAPH_ERR_ENTRY)")
        if int(got[1]):
            rows = torch.nonzero(out_count < 0).reshape(-1)
            _rank_long(torch, nbr, scores, row_off, row_ids, k, rows, out_ids, out_scores, out_count)
        if stats is not None:
            stats["long_lists"] = int(got[1])
    return out_ids, out_scores, out_count


def _rerank_lists(torch, corpus, nbr, row_off, m: int):
    """The rerank's score of every directed entry of the adjacency, in place of the entry: row ``r`` - converted to float32 -
    as the query of its own list.  The asking rows go in chunks of consecutive positions whose float32 copy stays under
    ``_PAIRS_QUERY_BYTES``; the lists are used as they lie.  Returns ``(scores, err)``."""
    dev = corpus.device
    total, dim = int(nbr.shape[0]), int(corpus.shape[1])
    scores = torch.empty((max(1, total),), dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    count32 = torch.diff(row_off).to(torch.int32)
    step = max(1, _PAIRS_QUERY_BYTES // (4 * dim))
    for lo in range(0, m, step):
        hi = min(m, lo + step)
        queries = _rows_as_f32(torch, corpus, torch.arange(lo, hi, dtype=torch.int64, device=dev))
        cosine_ragged_device(corpus, queries, nbr, row_off[lo:hi].contiguous(), count32[lo:hi].contiguous(), total,
                             scores=scores, err=err)
    return scores, err


def _best_of_lists(torch, corpus, lists, off, d_ids, kk: int, live_rows, stats: Dict, adjacency_err=None, rerank=None):
    """The tail of ``lsh_knn`` and of a round of ``refine_knn``: the lists ``lists`` / ``off`` - one per row of ``corpus`` -
    reranked (:func:`_rerank_lists`), a zero norm refused, the best ``kk`` selected under the ids ``d_ids``
    (:func:`select_neighbors`, which leaves ``stats["long_lists"]``) and the live rows gathered: ``(neighbors, scores,
    counts)``.  ONE readback of its own, the rerank's error word; ``adjacency_err`` - the word of the ``pair_adjacency`` that
    made the lists, where nobody has read it yet - comes in the same transfer and is judged first.  ``rerank``: the caller's
    own name for :func:`_rerank_lists`, where it has one."""
    exact, err = (rerank or _rerank_lists)(torch, corpus, lists, off, int(corpus.shape[0]))
    bits = torch.stack((err[0], (err if adjacency_err is None else adjacency_err)[0])).cpu().tolist()
    if adjacency_err is not None and int(bits[1]):              # (the emit names rows of the map, a < b: never seen)
        raise _native.NativeLibraryError("lsh_knn: " + (ENDPOINT_MSG if int(bits[1]) & 1 else LOOP_MSG))
    if int(bits[0]) & 5:
        raise ValueError("Cannot normalize zero vector")
    s_ids, s_scores, s_count = select_neighbors(lists, exact, off, d_ids, kk, stats)
    return s_ids[live_rows].contiguous(), s_scores[live_rows].contiguous(), s_count[live_rows].contiguous()


def lsh_knn(corpus, k: int, codes, offsets, member_rows, num_bands: int, band_bytes: int, *, row_ids=None,
            min_collisions: int = 1, max_bucket: Optional[int] = None, max_pairs: int = 1 << 26,
            max_raw_pairs: int = 1 << 34, return_tensors: bool = False, stats: Optional[Dict] = None):
    """For every row of ``corpus`` the ``k`` best of its BUCKET MATES - the k-NN graph a banded LSH index holds in its buckets,
    the approximate counterpart of :func:`lshrs_amd.exact_knn`: ``(ids (n,) int64, neighbors (n, kk) int64, scores (n, kk)
    float32, counts (n,) int32)``; NumPy arrays, or device tensors with ``return_tensors``.

    ``corpus``, ``row_ids``: as ``exact_knn`` takes them.  ``codes`` / ``offsets`` / ``member_rows``: ONE bucket segment as
    :func:`lshrs_amd.lsh_pairs_above` takes it.  A pair ``{a, b}`` of distinct rows is a CANDIDATE exactly as that join defines
    it: the two share a bucket of ``2 .. max_bucket`` entries in at least ``min_collisions`` bands; the candidates of a row are
    the rows it forms a candidate pair with.

    ``n``: the live rows, in ascending order of their ids - a row that is in no counted bucket is included.  ``kk = max(0,
    min(k, n - 1))``, the width ``exact_knn`` returns.  ``counts[i] = min(kk, candidates of i)``; the first ``counts[i]``
    entries of row ``i`` are its candidates of largest score, equal scores by ascending id; the rest is ``-1`` / ``NaN``.
    ``scores[i, j]`` is the RERANK score with row ``ids[i]``, converted to float32, as the query and row ``neighbors[i, j]`` as
    the row (``lshrs_cosine_ragged_*``, the orientation ``exact_knn`` documents): every candidate pair is scored twice, once
    per direction, and the two scores may differ in the last bit.  The order is ``lshrs_topk_desc_f32``'s - +0.0 ahead of -0.0,
    NaN last - with ties broken by id, never by position: the order in which the pairs were emitted decides nothing.

    Hence, for ``min_collisions = 1`` and no ``max_bucket``, row ``i``'s list is ``exact_knn``'s ranking of row ``i``
    RESTRICTED TO ITS CANDIDATES, bit for bit; where every pair of live rows is a candidate, the first three arrays equal
    ``exact_knn(corpus, k)`` bit for bit.

    Capacity and refusals are the join's, with its messages, before any pair is emitted: a member without a row
    (``IndexError``), a row in two buckets of one band, more than ``max_raw_pairs`` raw pairs, more than ``max_pairs``
    candidate pairs (``ValueError``).  A candidate row of zero norm raises ``ValueError("Cannot normalize zero vector")``;
    ``k <= 0`` or a ``bool`` raises ``ValueError`` before anything touches the GPU.
    ``stats``: a dict that receives ``buckets``, ``skipped_buckets``, ``raw_pairs``, ``emitted`` (distinct candidate pairs),
    ``launches`` (emit launches), ``rows``, ``live``, ``candidates_max`` (the longest list), ``short_rows`` (live rows with
    fewer than ``kk`` candidates) and ``long_lists`` (lists beyond the kernel's, ranked by torch's sorts)."""
    k = _check_k(k)
    max_pairs, max_raw_pairs = int(max_pairs), int(max_raw_pairs)
    _check_max_pairs(max_pairs)
    _join.check_join_args(0.0, min_collisions, max_bucket, max_pairs, num_bands, max_raw_pairs)
    torch = _native.require_gpu()
    _native.load()
    _native.load_graph()
    corpus_suffix(corpus)
    dev = corpus.device
    with torch.cuda.device(dev):
        d_ids = _rows_args(torch, corpus, row_ids, "lsh_knn")
        codes, offsets, member_rows = _join._segment_args(torch, codes, offsets, member_rows, dev)
        m = int(corpus.shape[0])
        live_rows, live_ids = _live_by_id(torch, d_ids, m, dev)
        n = int(live_rows.shape[0])
        kk = max(0, min(k, n - 1))
        out = {"buckets": int(codes.shape[0]), "skipped_buckets": 0, "raw_pairs": 0, "emitted": 0, "launches": 0, "rows": m,
               "live": n, "candidates_max": 0, "short_rows": n if kk else 0, "long_lists": 0}
        neighbors = torch.full((n, kk), -1, dtype=torch.int64, device=dev)
        scores = torch.full((n, kk), float("nan"), dtype=torch.float32, device=dev)
        counts = torch.zeros((n,), dtype=torch.int32, device=dev)
        if int(member_rows.shape[0]):
            plan = _join._plan(codes, offsets, member_rows, m, num_bands, band_bytes, min_collisions, max_bucket)
            out["skipped_buckets"], out["raw_pairs"] = plan.skipped_buckets, plan.raw_pairs
            if plan.raw_pairs > max_raw_pairs:
                raise ValueError(f"lsh_knn: the buckets hold {plan.raw_pairs} raw pairs, more than max_raw_pairs = "
                                 f"{max_raw_pairs}: set max_bucket to leave the largest buckets out")
            emitted = 0
            if plan.raw_pairs:
                pa, pb, emitted = _all_pairs(lambda cap: _join._emit(plan, cap), min(_join._JOIN_FIRST_CAPACITY, max_pairs),
                                             max_pairs, "lsh_knn", out)
                out["launches"] = plan.launches
            if emitted and kk:
                nbr, row_off, err = pair_adjacency(pa[:emitted], pb[:emitted], m)
                sel: Dict = {}
                neighbors, scores, counts = _best_of_lists(torch, corpus, nbr, row_off, d_ids, kk, live_rows, sel, err)
                lens = torch.diff(row_off)[live_rows]
                got = torch.stack((lens.max(), (lens < kk).sum())).cpu().tolist() if n else [0, 0]
                out.update(candidates_max=int(got[0]), short_rows=int(got[1]), long_lists=sel["long_lists"])
    return _finish(stats, out, (live_ids, neighbors, scores, counts), return_tensors)
