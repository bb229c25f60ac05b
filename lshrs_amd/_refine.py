"""The refinement of a k-NN graph - ``refine_knn`` - and what it is made of: one local-join round (one round of NN-descent
without its flags and samples) lets every row also consider ITS NEIGHBOURS' NEIGHBOURS, in either direction of the graph's
entries.  It stands between the LSH graph (``lsh_knn``: cheap, as good as the buckets) and the exact one (``exact_knn``).

A round, over row positions:

edges      ``lshrs_refine_edges_i64``: the neighbour table as undirected pairs, each once (``csrc/refine.hip``,
           ``include/lshrs_refine.h``, ``liblshrs_refine.so``).
adjacency  ``_knn_join.pair_adjacency``: one list per row, ``A(r)``.
expand     ``lshrs_refine_expand_count_i64``, ``torch.cumsum``, ``lshrs_refine_expand_write_i64``: per row ``C(r)``, the rows at
           distance one or two - ``A(r)`` and ``A(m)`` for every midpoint ``m`` in ``A(r)`` - without ``r``, each once, IN NO
           PARTICULAR ORDER.
rerank     ``_knn_join._rerank_lists``: row ``r`` as the float32 query of its own list, the orientation of ``exact_knn``.
select     ``_knn_join.select_neighbors``: per row the best ``k`` by (score descending, id ascending) - independent of the
           order the expansion left.  (Both through ``_knn_join._best_of_lists``, the tail ``lsh_knn`` ends in.)

No CPU compute path: the host checks arguments, reads counts and error words back, and keeps statistics.
"""

from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from . import _native
from ._exact import _finish, _live_by_id, _rows_args
from ._knn_join import _best_of_lists, _check_k, _ragged, _rerank_lists, pair_adjacency
from .similarity import _on_device, corpus_suffix

__all__ = ["refine_knn", "graph_edges", "expand_candidates", "refine_wave_set", "refine_max_set"]

OUTSIDE_MSG = "an entry of the neighbour table lies outside [-1, n_rows)"
SELF_MSG = "a row lists itself as a neighbour"


def refine_wave_set() -> int:
    """The largest bound ``U(r)`` at which ONE WAVE of ``lshrs_refine_expand_*`` expands a row; beyond it a workgroup does."""
    return int(_native.load_refine().lshrs_refine_wave_set())


def refine_max_set() -> int:
    """The largest bound ``U(r)`` at which ``lshrs_refine_expand_*`` expands a row on the device."""
    return int(_native.load_refine().lshrs_refine_max_set())


def _check_count(value, name: str, least: int, none_ok: bool = False):
    """``value`` as an int of at least ``least`` (or None where that is allowed), and no ``bool``.  Pure host."""
    if value is None and none_ok:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) < least:
        raise ValueError(f"{name} must be an integer >= {least}" + (" or None" if none_ok else "") + f"; received {value!r}")
    return int(value)


def check_refine_args(rounds, max_degree, max_entries=0):
    """``(rounds, max_degree, max_entries)`` as ``refine_knn`` takes them: ``rounds >= 0``, ``max_degree`` None or ``>= 1``,
    ``max_entries >= 0``, none of them a ``bool`` - else ``ValueError``.  Pure host: it runs before anything touches the GPU."""
    return (_check_count(rounds, "rounds", 0), _check_count(max_degree, "max_degree", 1, none_ok=True),
            _check_count(max_entries, "max_entries", 0))


def graph_edges(graph):
    """Device-level entry of the edges: ``graph`` - a contiguous int64 ``(n_rows, k_in)`` device tensor of ROW POSITIONS, ``-1``
    for no entry - as undirected pairs.  Returns ``(keep (n_rows, k_in) uint8, err int32[1])``: ``keep[r, c]`` is 1 iff
    ``g = graph[r, c]`` is ``>= 0``, no earlier column of row ``r`` holds ``g``, and not both ``g < r`` and row ``g`` lists
    ``r`` - so that the kept ``(r, g)`` are every pair of the table once, ready for ``pair_adjacency``.  ``err``: bit 0 - an
    entry outside ``[-1, n_rows)``, bit 1 - a row that lists itself; such an entry is not kept.  Nothing is read back here."""
    torch = _native.require_gpu()
    lib = _native.load_refine()
    if graph.dtype != torch.int64 or graph.dim() != 2:
        raise ValueError("graph must be an int64 tensor of shape (n_rows, k_in)")
    graph = graph.contiguous()
    dev = graph.device
    n_rows, k_in = int(graph.shape[0]), int(graph.shape[1])
    with torch.cuda.device(dev):
        keep = torch.zeros((n_rows, k_in), dtype=torch.uint8, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.check(lib.lshrs_refine_edges_i64(graph.data_ptr(), n_rows, k_in, keep.data_ptr(), err.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream), "lshrs_refine_edges_i64")
    return keep, err


def _expand_with_torch(torch, nbr, row_off, rows, cap: Optional[int]):
    """``C(r)`` of ``rows`` (int64, ascending: those the kernel left at -1) with torch: their lists gathered, the lists of
    their midpoints gathered behind them, ``torch.unique`` on ``slot << 32 | candidate``.  Returns ``(lens, cands)``: per row
    of ``rows`` its number of candidates, and the candidates of all of them end to end (ascending inside a row)."""
    n_rows = int(row_off.shape[0]) - 1
    deg = torch.diff(row_off)
    slot, at = _ragged(torch, row_off[rows], deg[rows])
    mids = nbr[at]
    ok = (mids >= 0) & (mids < n_rows)
    slot, mids = slot[ok], mids[ok]
    through = deg[mids] <= cap if cap is not None else torch.ones_like(mids, dtype=torch.bool)
    slot2, at2 = _ragged(torch, row_off[mids[through]], deg[mids[through]])
    far = nbr[at2]
    own = torch.cat((slot, slot[through][slot2]))
    cand = torch.cat((mids, far))
    ok = (cand >= 0) & (cand < n_rows) & (cand != rows[own])
    keys = torch.unique((own[ok] << 32) | cand[ok])
    lens = torch.bincount(keys >> 32, minlength=int(rows.shape[0]))
    return lens, keys & 0xFFFFFFFF


def expand_candidates(nbr, row_off, max_degree: Optional[int] = None, stats: Optional[Dict] = None):
    """Device-level entry of count, prefix and write: over the adjacency ``nbr`` / ``row_off`` (contiguous int64 device tensors,
    what ``pair_adjacency`` returns) the rows within two steps of every row.  ``A(r)``: the list of ``r``; the MIDPOINTS of
    ``r``: every ``m`` in ``A(r)`` with at most ``max_degree`` entries of its own (None: every one); ``C(r)``: the union of
    ``A(r)`` and of ``A(m)`` over the midpoints, without ``r``, each row once.  A row over the cap stays a candidate of its
    neighbours - it only stops being a midpoint - so ``C(r)`` always holds ``A(r)``.

    Returns ``(cand (total,) int64, cand_off (n_rows + 1,) int64, err int32[1])``: row ``r`` owns ``cand[cand_off[r]:cand_off[r
    + 1]]``, ``C(r)`` IN NO PARTICULAR ORDER (the order the lanes won their slots of the hash set in: it differs from run to
    run and nothing may depend on it).  ``err``: bit 0 - a list outside ``nbr``, bit 1 - an entry outside ``[0, n_rows)``,
    which is skipped.  Rows whose bound ``U(r) = len(A(r)) + the lists of its midpoints`` exceeds :func:`refine_max_set` are
    left at ``-1`` by the count and expanded here with torch (gather, ``torch.unique``); ``stats["torch_rows"]`` counts them,
    ``stats["skipped_midpoints"]`` the rows over ``max_degree``.  Two numbers are read back between the launches: the total,
    and the count of such rows."""
    cap = _check_count(max_degree, "max_degree", 1, none_ok=True)
    torch = _native.require_gpu()
    lib = _native.load_refine()
    dev = row_off.device
    n_rows, total = int(row_off.shape[0]) - 1, int(nbr.shape[0])
    if n_rows < 0 or nbr.dtype != torch.int64 or row_off.dtype != torch.int64:
        raise ValueError("nbr and row_off must be int64 tensors, row_off of n_rows + 1 entries")
    nbr, row_off = nbr.contiguous(), row_off.contiguous()
    cap32 = min(cap, 0x7FFFFFFF) if cap is not None else 0
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        count = torch.zeros((n_rows,), dtype=torch.int32, device=dev)
        _native.check(lib.lshrs_refine_expand_count_i64(nbr.data_ptr() if total else None, row_off.data_ptr(), n_rows, total,
                                                        cap32, count.data_ptr(), err.data_ptr(), stream),
                      "lshrs_refine_expand_count_i64")
        beyond = count < 0
        over = (torch.diff(row_off) > cap).sum() if cap is not None else torch.zeros((), dtype=torch.int64, device=dev)
        got = torch.stack((beyond.sum(), over)).cpu().tolist() if n_rows else [0, 0]
        lens = count.long()
        rows = late = None
        if int(got[0]):
            rows = torch.nonzero(beyond).reshape(-1)
            lens[rows], late = _expand_with_torch(torch, nbr, row_off, rows, cap)
        cand_off = torch.zeros((n_rows + 1,), dtype=torch.int64, device=dev)
        cand_off[1:] = torch.cumsum(lens, 0)
        cand_total = int(cand_off[-1].item()) if n_rows else 0
        cand = torch.empty((cand_total,), dtype=torch.int64, device=dev)
        _native.check(lib.lshrs_refine_expand_write_i64(nbr.data_ptr() if total else None, row_off.data_ptr(), n_rows, total,
                                                        cap32, cand_off.data_ptr(), cand.data_ptr() if cand_total else None,
                                                        cand_total, err.data_ptr(), stream), "lshrs_refine_expand_write_i64")
        if rows is not None:
            cand[_ragged(torch, cand_off[rows], lens[rows])[1]] = late
    if stats is not None:
        stats["torch_rows"], stats["skipped_midpoints"] = int(got[0]), int(got[1])
    return cand, cand_off, err


def _ids_to_rows(torch, table, live_rows, live_ids, m: int):
    """A table of IDS (one row per live id in ascending order, ``-1`` for no entry) as the ``(m, width)`` table of ROW
    POSITIONS the kernels take (rows without an id: all ``-1``); ``ValueError`` for a name that is not a live id."""
    dev = table.device
    graph = torch.full((m, int(table.shape[1])), -1, dtype=torch.int64, device=dev)
    if int(table.numel()):
        named = table != -1
        at = torch.searchsorted(live_ids, table.clamp(min=0)).clamp(max=int(live_ids.shape[0]) - 1)
        if bool((named & (live_ids[at] != table)).any()):
            raise ValueError("refine_knn: neighbors names an id that has no row (never stored, or removed)")
        graph[live_rows] = torch.where(named, live_rows[at], torch.full_like(at, -1))
    return graph


def _own_lists(torch, graph):
    """The table itself as lists - what ``rounds = 0`` reranks: ``(cand, cand_off)`` of every entry that is the first of its
    row to name its row."""
    k_in = int(graph.shape[1])
    earlier = torch.tril(torch.ones((k_in, k_in), dtype=torch.bool, device=graph.device), -1)
    repeat = ((graph.unsqueeze(2) == graph.unsqueeze(1)) & earlier).any(dim=2)
    keep = (graph >= 0) & ~repeat
    cand_off = torch.zeros((int(graph.shape[0]) + 1,), dtype=torch.int64, device=graph.device)
    cand_off[1:] = torch.cumsum(keep.sum(dim=1), 0)
    return graph[keep].contiguous(), cand_off


def refine_knn(corpus, neighbors, k: int, *, row_ids=None, rounds: int = 1, max_degree: Optional[int] = None,
               max_entries: int = 1 << 28, return_tensors: bool = False, stats: Optional[Dict] = None):
    """A k-NN graph made better by its own entries: every row also considers its NEIGHBOURS' NEIGHBOURS - ``rounds`` local-join
    rounds over ``neighbors``: ``(ids (n,) int64, neighbors (n, kk) int64, scores (n, kk) float32, counts (n,) int32)`` in the
    form of :func:`lshrs_amd.lsh_knn`, ``kk = max(0, min(k, n - 1))``; NumPy arrays, or device tensors with ``return_tensors``.

    ``corpus``, ``row_ids``: as ``exact_knn`` takes them.  ``neighbors``: ``(n, k_in)`` int64 of IDS, ``-1`` for no entry, row
    ``i`` belonging to the ``i``-th live id in ascending order - what ``lsh_knn`` and ``exact_knn`` return, so that their
    output feeds in as it is; ``k`` need not equal ``k_in``.  A name that is not a live id, a row that lists itself and a first
    dimension other than ``n`` raise ``ValueError``.

    A round reads the table as an UNDIRECTED graph - ``a`` and ``b`` are adjacent when either lists the other; ``A(r)``: the
    rows adjacent to ``r`` - and gives row ``r`` the candidates ``C(r)``: ``A(r)`` and ``A(m)`` for every MIDPOINT ``m`` in
    ``A(r)``, without ``r``, each once.  ``max_degree`` (None: no cap; else ``>= 1``): a row with more than ``max_degree``
    adjacent rows is nobody's midpoint - it counts in no role as a connector, as ``max_bucket`` has it for large buckets -
    but stays a candidate of its neighbours.  The candidates are reranked with row ``r``, converted to float32, as the query
    (``lshrs_cosine_ragged_*``, the orientation ``exact_knn`` documents) and the best ``k`` kept in the order of
    ``lshrs_topk_desc_f32`` with EQUAL SCORES BY ASCENDING ID.  The next round's input is the previous round's output; the loop
    stops early when a round changes no neighbour id.  ``rounds = 0`` reranks the table's own entries and nothing else.

    By construction, after one round row ``i``'s list is ``exact_knn``'s ranking of row ``i`` RESTRICTED TO ``C(i)``, scores
    bit for bit - the kernel, the orientation and the tie by id are the same, and nothing depends on the order atomics arrive
    in.  Hence: every input neighbour stays a candidate, so the j-th score of a row never decreases from round to round;
    ``exact_knn``'s own graph is a fixed point; and where every pair of live rows is within two steps, the first three arrays
    equal ``exact_knn(corpus, k)`` bit for bit.

    More than ``max_entries`` directed candidate entries in a round raise ``ValueError`` before anything is reranked: set
    ``max_degree``.  ``k <= 0``, ``rounds < 0``, ``max_degree < 1``, ``max_entries < 0`` or a ``bool`` for any of them raise
    ``ValueError`` before anything touches the GPU; a candidate row of zero norm raises ``ValueError("Cannot normalize zero
    vector")``.
    ``stats``: a dict that receives ``rounds_run``; per round, as lists, ``edges`` (undirected pairs), ``entries`` (directed
    candidate entries), ``changed_rows`` (live rows whose ids differ from the round's input, compared over ``kk`` columns),
    ``candidates_max``, ``skipped_midpoints`` (rows over ``max_degree``), ``torch_rows`` (rows expanded by torch) and
    ``long_lists`` (lists ranked by torch's sorts); and ``rows``, ``live``, ``short_rows`` (live rows that end with fewer than
    ``kk`` candidates)."""
    k = _check_k(k)
    rounds, cap, max_entries = check_refine_args(rounds, max_degree, max_entries)
    torch = _native.require_gpu()
    _native.load()
    _native.load_graph()
    _native.load_refine()
    corpus_suffix(corpus)
    dev = corpus.device
    with torch.cuda.device(dev):
        d_ids = _rows_args(torch, corpus, row_ids, "refine_knn")
        m = int(corpus.shape[0])
        live_rows, live_ids = _live_by_id(torch, d_ids, m, dev)
        n = int(live_rows.shape[0])
        kk = max(0, min(k, n - 1))
        table = _on_device(torch, neighbors, np.int64).to(device=dev, dtype=torch.int64)
        if table.dim() != 2 or int(table.shape[0]) != n:
            raise ValueError(f"neighbors must have shape ({n}, k_in): one row per live id; received {tuple(table.shape)}")
        if bool((table == live_ids.unsqueeze(1)).any()):
            raise ValueError("refine_knn: " + SELF_MSG)
        per_round = ("edges", "entries", "changed_rows", "candidates_max", "skipped_midpoints", "torch_rows", "long_lists")
        out: Dict = {"rounds_run": 0, "rows": m, "live": n, "short_rows": n if kk else 0}
        out.update((name, []) for name in per_round)
        graph = _ids_to_rows(torch, table.contiguous(), live_rows, live_ids, m)
        neighbors_out = torch.full((n, kk), -1, dtype=torch.int64, device=dev)
        scores_out = torch.full((n, kk), float("nan"), dtype=torch.float32, device=dev)
        counts_out = torch.zeros((n,), dtype=torch.int32, device=dev)
        before = torch.full((n, kk), -1, dtype=torch.int64, device=dev)      # the input's ids over kk columns
        width = min(kk, int(table.shape[1]))
        before[:, :width] = table[:, :width]
        for step in range(max(rounds, 1) if kk else 0):
            did: Dict = {"edges": 0, "torch_rows": 0, "skipped_midpoints": 0, "long_lists": 0}
            if rounds == 0:
                cand, cand_off = _own_lists(torch, graph)
            else:
                keep, err0 = graph_edges(graph)
                at = torch.nonzero(keep)
                a, b = at[:, 0].contiguous(), graph[at[:, 0], at[:, 1]].contiguous()
                did["edges"] = int(a.shape[0])
                nbr, row_off, err1 = pair_adjacency(a, b, m)
                cand, cand_off, err2 = expand_candidates(nbr, row_off, cap, did)
                bits = torch.stack((err0[0], err1[0], err2[0])).cpu().tolist()
                if any(int(bit) for bit in bits):       # (the table was checked above, the pairs are the edges': never seen)
                    raise _native.NativeLibraryError(f"refine_knn: the round's kernels report {bits}: " +
                                                     (SELF_MSG if int(bits[0]) & _native.REFINE_ERR_SELF else OUTSIDE_MSG))
            entries = int(cand.shape[0])
            if entries > max_entries:
                raise ValueError(f"refine_knn: round {step + 1} holds {entries} candidate entries, more than max_entries = "
                                 f"{max_entries}: set max_degree to keep the rows with the most neighbours from connecting "
                                 f"theirs")
            lens = torch.diff(cand_off)[live_rows]
            if entries:
                neighbors_out, scores_out, counts_out = _best_of_lists(torch, corpus, cand, cand_off, d_ids, kk, live_rows, did,
                                                                       rerank=_rerank_lists)
            got = torch.stack((lens.max(), (lens < kk).sum(), (neighbors_out != before).any(dim=1).sum())).cpu().tolist()
            for name in per_round if rounds else ():
                out[name].append({"entries": entries, "candidates_max": int(got[0]), "changed_rows": int(got[2])}.get(
                    name, did.get(name)))
            out["short_rows"], out["rounds_run"] = int(got[1]), out["rounds_run"] + (1 if rounds else 0)
            if not int(got[2]) or rounds == 0:
                break
            before = neighbors_out
            graph = _ids_to_rows(torch, neighbors_out, live_rows, live_ids, m)
    return _finish(stats, out, (live_ids, neighbors_out, scores_out, counts_out), return_tensors)
