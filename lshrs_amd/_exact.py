"""Exact top-k cosine search over a device-resident row block - ``exact_top_k`` - and what it is made of.

The ground truth an approximate index is measured against (``LSHRS.recall``) and the answer when its buckets are thin
(``LSHRS.search_exact``, ``DeviceVectors.search``).  Two methods, the same answer:

"scan"    ``lshrs_scan_topk_*`` (``csrc/scan.hip``): every row against tiles of 64 queries on the matrix cores, keeping per
          query the ``window`` rows of the largest APPROXIMATE cosine; the window's rows are then rescored by the rerank's own
          kernel (``lshrs_cosine_ragged_*``), so a returned score is bit for bit the rerank's score of that (query, row), and
          ordered by ``lshrs_topk_desc_f32``.  A query is SETTLED (:func:`settled`) when the window saw every live row, or when
          ``a_window + epsilon <= s_k``: a row left out has an approximate score of at most ``a_window``, the last one in the
          window, hence a cosine of at most ``a_window + epsilon`` (``lshrs_scan_epsilon``: a proven bound on
          |approximate - cosine|), which is no more than ``s_k``, the k-th rescored score.  ``exact_top_k`` passes epsilon plus
          :func:`rerank_rounding`, so that the row's RERANK score, too, lies below ``s_k`` and both methods agree bit for bit.  Queries that are not settled - near-ties
          across the cut, a ``k`` too large for the window - take the other method.
"gather"  the rerank's kernels over the list of all live rows: ``lshrs_cosine_batch_*`` then ``lshrs_topk_desc_f32``, in chunks of
          queries whose score matrix stays under 128 MiB (under 1 GiB with everything else a chunk allocates).  Every row is read once per query.

``exact_above`` is the range search on the same first pass (``lshrs_scan_above_*``): every live row whose rerank score reaches a
threshold.  No window, no unsettled query: the first pass lets through whatever reaches ``threshold - (epsilon +
rerank_rounding)``, which no row of the answer can lie below, and the rerank's kernel decides the rest.

``exact_pairs_above`` is the self-join on that pass (``lshrs_scan_pairs_*``): every pair of live rows whose rerank score reaches
a threshold - the stored rows are their own queries, every unordered pair is multiplied once, and the rerank's kernel judges what
the pass lets through, the row of the lower id as the query (``_judge_pairs``: the text the LSH self-join of ``_join.py`` judges
its buckets' pairs with, too).

``exact_knn`` is the k-NN self-join on the top-k pass (``lshrs_scan_knn_*``): for every live row the ``k`` OTHER live rows
nearest to it - the stored rows are their own queries, a block at a time, no row enters its own window, and the settle rule and
the gather fallback are those of ``exact_top_k``.

Each layer is one text.  The two selections share ``_check_selection`` and ``_method_plan`` (arguments; scan or gather, window,
epsilon), ``_scan_selecting`` (the windows' buffers and the launch behind ``scan_windows`` and ``scan_knn``), ``_window_answer``
(from the windows to ids, scores and the settled queries: the tie rule and the settle rule live there and nowhere else),
``_live_by_id`` and ``_gather``.  The two emitting passes share ``_scan_emitting`` and ``_all_pairs``; the two joins
``_judge_pairs``; all of them ``_rows_args``, ``_scan_workspace`` and ``_finish``.

No CPU compute path: the host moves arrays, decides which queries are settled from three numbers per query, and keeps counts.
"""

from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from . import _native
from .similarity import (_CORPUS_ENTRY, _CORPUS_ENTRY_8BIT, _on_device, _raise_for_status, corpus_suffix, cosine_ragged_device,
                         cosine_scores_device, topk_desc_device)

__all__ = ["exact_top_k", "exact_above", "exact_pairs_above", "exact_knn", "scan_knn", "settled", "choose_window", "rerank_rounding", "scan_epsilon",
           "scan_max_window", "scan_windows", "scan_above", "scan_pairs", "above_bars", "above_recall", "collision_law"]

METHODS = ("auto", "scan", "gather")
# (query, live row) pairs of one chunk of the gather.  Per pair: 4 B of score, 8 B of candidate row, 1 B of status, and up to
# 16 B of the top-k kernel's workspace (a 64-bit item, the list padded to a power of two) - 128 MiB of scores, under 1 GiB in all
_GATHER_MAX_PAIRS = 1 << 25
_SCAN_MAX_DIM = 16384               # what lshrs_scan_topk_* and lshrs_cosine_* take
_SCAN_MAX_ROWS = (1 << 31) - 1
# slots of the range search's first launch: max(this, 64 per query) pairs of 16 bytes; more pairs than that cost a second launch
_ABOVE_FIRST_CAPACITY = 1 << 20
# ... and of the self-join's: pairs of 20 bytes
_PAIRS_FIRST_CAPACITY = 1 << 20
# float32 bytes of the lower-id rows one chunk of the self-join's rescoring gathers as queries
_PAIRS_QUERY_BYTES = 1 << 28


def scan_max_window() -> int:
    """The widest window ``lshrs_scan_topk_*`` keeps per query."""
    return int(_native.load().lshrs_scan_max_window())


def scan_epsilon(dtype, dim: int) -> float:
    """``lshrs_scan_epsilon``: the proven bound on |approximate score - cosine of the stored row| for rows of ``dtype``
    (a torch dtype or its name) and ``dim`` elements."""
    name = str(dtype).replace("torch.", "")
    suffix = _CORPUS_ENTRY.get(name, _CORPUS_ENTRY_8BIT.get(name))
    if suffix is None:
        raise ValueError(f"no scan over rows of {dtype}")
    eps = float(_native.load().lshrs_scan_epsilon(_native.SCAN_ELEMS.index(suffix), int(dim)))
    if eps < 0:
        raise ValueError(f"lshrs_scan_epsilon takes 1 <= dim <= 16384; received {dim}")
    return eps


def rerank_rounding(dim: int) -> float:
    """A bound on how far the rerank's float32 score of a (query, row) of ``dim`` elements can lie above the cosine.  With
    ``u = 2^-24``: each lane of ``cosine_kernel`` sums at most ``dim / 64 + 3`` fused multiply-adds and a tree of six additions
    joins the lanes - relative error at most ``(dim / 64 + 9) u`` of ``sum |q_i x_i| <= ||q|| ||x||`` for the dot product, half
    that for the row's norm, half of ``(dim / 256 + 10) u`` for the query's - then two square roots, a product and a division,
    one rounding each: ``(dim / 32 + 23) u`` to first order, charged as ``(dim / 16 + 32) u``.  The settle rule adds it to
    epsilon, so that a row left out scores strictly below the k-th kept one in the rerank's own arithmetic, not only in exact
    arithmetic."""
    return (int(dim) / 16.0 + 32.0) * 2.0 ** -24


def choose_window(k: int, max_window: int) -> int:
    """Rows the first pass keeps per query for a top-``k`` search: the next power of two at or above ``2 k``, at most
    ``max_window`` (``scan_max_window()``)."""
    if int(k) <= 0:
        raise ValueError("k must be > 0")
    return min(int(max_window), 1 << (2 * int(k) - 1).bit_length())


def settled(count, window: int, a_window, s_k, epsilon: float) -> np.ndarray:
    """Which queries the first pass settled.  Per query: ``count`` rows in its window (``out_count``), ``a_window`` the last
    approximate score of the window, ``s_k`` the k-th rescored score (``-inf`` where the window holds fewer than ``k`` rows).
    Settled: ``count < window`` - every live row was seen - or ``a_window + epsilon <= s_k`` (evaluated in float64)."""
    count = np.asarray(count, dtype=np.int64)
    a = np.asarray(a_window, dtype=np.float64)
    s = np.asarray(s_k, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (count < int(window)) | (a + float(epsilon) <= s)


def _check_selection(k, method) -> int:
    """``k`` as an int; ``ValueError`` for a ``method`` or a ``k`` that ``exact_top_k`` and ``exact_knn`` do not take.  Pure
    host: it runs before anything touches the GPU."""
    if method not in METHODS:
        raise ValueError("method must be 'auto', 'scan' or 'gather'")
    if int(k) <= 0:
        raise ValueError("k must be > 0")
    return int(k)


def _method_plan(k: int, method: str, dtype, dim: int):
    """How a selection of ``k`` (checked: :func:`_check_selection`) goes over rows of ``dtype`` and ``dim`` elements:
    ``(use_scan, window, eps)`` - whether the first pass runs, the window it keeps per query (0 without it: what ``stats``
    report as ``window``) and ``scan_epsilon``."""
    max_window = scan_max_window()
    use_scan = method == "scan" or (method == "auto" and 2 * k <= max_window)
    return use_scan, choose_window(k, max_window) if use_scan else 0, scan_epsilon(dtype, dim)


def _scan_workspace(torch, lib, sizer: str, dev, *shape):
    """The workspace of a first pass: ``sizer`` (``lshrs_scan_workspace_bytes`` or ``lshrs_scan_above_workspace_bytes``) of
    ``shape`` bytes on ``dev``; a negative size raises what ``_native.check`` makes of it."""
    nbytes = int(getattr(lib, sizer)(*shape))
    if nbytes < 0:
        _native.check(nbytes, sizer)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _scan_selecting(corpus, family: str, sizer: str, q: int, window: int, empty: bool, sizer_shape, head, row_ids):
    """The plumbing of the two selecting entries (``family``: "topk" or "knn"): the windows of ``q`` queries - rows,
    approximate scores, counts - and the error bits; unless ``empty``, the workspace (``sizer`` of ``sizer_shape``) and the
    launch, ``head`` being the entry's own arguments between ``row_ids`` and ``out_rows``.  Returns ``(rows, approx, count,
    err)``."""
    torch = _native.require_gpu()
    lib = _native.load()
    entry = f"lshrs_scan_{family}_" + corpus_suffix(corpus)
    dev = corpus.device
    rows = torch.empty((max(q, 0), window), dtype=torch.int64, device=dev)
    approx = torch.empty((max(q, 0), window), dtype=torch.float32, device=dev)
    count = torch.empty((max(q, 0),), dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    if empty:
        return rows, approx, count, err
    with torch.cuda.device(dev):
        ws = _scan_workspace(torch, lib, sizer, dev, *sizer_shape)
        _native.check(getattr(lib, entry)(corpus.data_ptr(), int(corpus.shape[0]), int(corpus.stride(0)), int(corpus.shape[1]),
                                          row_ids.data_ptr() if row_ids is not None else None, *head,
                                          rows.data_ptr(), approx.data_ptr(), count.data_ptr(), ws.data_ptr(), err.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream), entry)
    return rows, approx, count, err


def _scan_emitting(corpus, family: str, first_dtype, capacity: int, empty: bool, sizer_shape, head, row_ids):
    """The plumbing of the two emitting entries (``family``: "above" or "pairs"): three output arrays of ``capacity`` slots -
    the first of ``first_dtype`` - a cursor and the error bits; unless ``empty``, the workspace (``sizer_shape``: what
    ``lshrs_scan_<family>_workspace_bytes`` takes) and the launch, ``head`` being the entry's own arguments between ``row_ids``
    and ``capacity``.  No output pointer is passed for a ``capacity`` of 0.  Returns ``(first, second, approx, total, err)``."""
    torch = _native.require_gpu()
    lib = _native.load()
    entry = f"lshrs_scan_{family}_" + corpus_suffix(corpus)
    dev = corpus.device
    capacity = int(capacity)
    first = torch.empty((capacity,), dtype=first_dtype, device=dev)
    second = torch.empty((capacity,), dtype=torch.int64, device=dev)
    approx = torch.empty((capacity,), dtype=torch.float32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    if empty:
        return first, second, approx, total, err
    with torch.cuda.device(dev):
        ws = _scan_workspace(torch, lib, f"lshrs_scan_{family}_workspace_bytes", dev, *sizer_shape)
        outs = [t.data_ptr() if capacity else None for t in (first, second, approx)]
        _native.check(getattr(lib, entry)(corpus.data_ptr(), int(corpus.shape[0]), int(corpus.stride(0)), int(corpus.shape[1]),
                                          row_ids.data_ptr() if row_ids is not None else None, *head, capacity, *outs,
                                          total.data_ptr(), ws.data_ptr(), err.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream), entry)
    return first, second, approx, total, err


def _all_pairs(launch, first_capacity: int, max_pairs: int, caller: str, out: Dict):
    """The capacity protocol of ``exact_above`` and ``exact_pairs_above`` (``caller``: the name the messages carry):
    ``launch(capacity)`` - ``scan_above`` or ``scan_pairs`` with everything else bound - once with ``first_capacity`` slots
    and, when more pairs reached the bar, a second time with room for all.  One number crosses to the host per launch: how
    many pairs the pass found.  Returns ``(first, second, emitted)`` and records ``launches`` and ``emitted`` in ``out``."""
    first, second, _, total, err = launch(first_capacity)
    emitted = int(total.item())
    out["launches"] = 1
    if int(err.item()) & 5:
        raise ValueError("Cannot normalize zero vector")
    if emitted > max_pairs:
        raise ValueError(f"{caller}: {emitted} pairs reach the threshold's bar, more than max_pairs = {max_pairs}")
    if emitted > first_capacity:
        del first, second
        first, second, _, total, err = launch(emitted)
        out["launches"] = 2
        if int(total.item()) != emitted:            # (the same launches on the same data: the same count)
            raise RuntimeError(f"{caller}: the second pass counted other pairs than the first")
    out["emitted"] = emitted
    return first, second, emitted


def _descending(torch, scores):
    """An int64 in [0, 2^32) that DEscends with a float32 score (-0.0 with 0.0): a stable ascending sort on it orders by
    descending score and keeps the order of equal scores."""
    bits = (scores + 0.0).view(torch.int32)
    return 0x7FFFFFFF - torch.where(bits >= 0, bits, bits ^ 0x7FFFFFFF).long()


def scan_windows(corpus, queries, window: int, row_ids=None):
    """Device-level entry of the first pass: ``corpus`` (m, dim) as ``corpus_suffix`` accepts it, ``queries`` (q, dim) float32
    contiguous on the same device, ``row_ids`` optional int64 (m,) there.  Returns ``(rows (q, window) int64, approx (q, window)
    float32, count (q,) int32, err int32[1])`` as ``lshrs_scan_topk_*`` leaves them."""
    q, m, dim = int(queries.shape[0]), int(corpus.shape[0]), int(corpus.shape[1])
    return _scan_selecting(corpus, "topk", "lshrs_scan_workspace_bytes", q, window, q == 0, (q, m, dim, window),
                           (queries.data_ptr(), q, window), row_ids)


def _rescore(torch, corpus, queries, rows, count):
    """The rerank's score of every (query, window row): ``lshrs_cosine_ragged_*`` over the rows as they stand, ``-inf`` behind
    each query's ``count``."""
    dev = corpus.device
    q, w = int(rows.shape[0]), int(rows.shape[1])
    scores = torch.full((q, w), float("-inf"), dtype=torch.float32, device=dev)
    off = torch.arange(0, q * w, w, dtype=torch.int64, device=dev)
    return cosine_ragged_device(corpus, queries, rows, off, count, q * w, scores=scores)


def _window_answer(torch, corpus, queries, d_ids, rows, approx, count, err, kk: int, window: int, margin: float):
    """From the first pass's windows to the answer they hold: ``rows`` / ``approx`` / ``count`` / ``err`` as
    :func:`scan_windows` or :func:`scan_knn` leave them for the float32 ``queries`` (u, dim).  Returns ``(ids (u, kw), scores
    (u, kw), done)`` with ``kw = min(kk, window)``: the window's best by the rerank's score, equal scores by ascending id, and
    which queries that settles (:func:`settled` with ``margin``: epsilon plus :func:`rerank_rounding`).  Five things cross to
    the host: the error words of the pass and of the rescoring - a zero vector raises here - and per query ``count``, the
    window's last approximate score and the k-th rescored one."""
    # the window in ascending order of id (padding last): the tie rule of the top-k kernel then is ascending id
    wid = rows if d_ids is None else torch.where(rows >= 0, d_ids[rows.clamp(min=0)], rows)
    key = torch.where(rows >= 0, wid, torch.iinfo(torch.int64).max)
    by_id = torch.argsort(key, dim=1)
    rows_s, wid = torch.gather(rows, 1, by_id).contiguous(), torch.gather(wid, 1, by_id)
    exact, err2 = _rescore(torch, corpus, queries, rows_s, count)
    if int(err.item()) & 5 or int(err2.item()) & 5:
        raise ValueError("Cannot normalize zero vector")
    kw = min(kk, window)
    order, best = topk_desc_device(exact, kw)
    s_k = best[:, kw - 1] if kw == kk else torch.full((int(rows.shape[0]),), float("-inf"), device=corpus.device)
    done = settled(count.cpu().numpy(), window, approx[:, window - 1].cpu().numpy(), s_k.cpu().numpy(), margin)
    return torch.gather(wid, 1, order.long()), best, done


def _live_by_id(torch, d_ids, m: int, dev):
    """``(live_rows, live_ids)``, both contiguous: the rows of ``row_ids`` ``d_ids`` (None: all ``m``, under their index) that
    exist, in ascending order of their ids, and those ids."""
    if d_ids is None:
        live_rows = torch.arange(m, dtype=torch.int64, device=dev)
        return live_rows, live_rows
    live_rows = torch.nonzero(d_ids >= 0).reshape(-1)
    live_ids = d_ids[live_rows]
    by_id = torch.argsort(live_ids)
    return live_rows[by_id].contiguous(), live_ids[by_id].contiguous()


def _gather(torch, corpus, queries, live_rows, live_ids, kk: int):
    """Method "gather": ``(ids (q, kk), scores (q, kk))`` device tensors.  ``live_rows`` / ``live_ids``: the live rows in
    ascending order of their ids, so that the top-k kernel's tie rule (ascending position) is ascending id.  Queries go in chunks
    of ``_GATHER_MAX_PAIRS // live`` (at least one): what a chunk allocates - scores, the candidate matrix the batch entry wants,
    statuses, the top-k workspace - stays under 1 GiB while ``live <= 2^25``, and grows with ``live`` beyond."""
    q, live = int(queries.shape[0]), int(live_rows.shape[0])
    ids = torch.empty((q, kk), dtype=torch.int64, device=corpus.device)
    scores = torch.empty((q, kk), dtype=torch.float32, device=corpus.device)
    step = max(1, _GATHER_MAX_PAIRS // max(live, 1))
    for lo in range(0, q, step):
        hi = min(q, lo + step)
        cand = live_rows.unsqueeze(0).expand(hi - lo, live)
        got, status, qstatus = cosine_scores_device(corpus, queries[lo:hi], cand)
        _raise_for_status(status, qstatus)
        order, best = topk_desc_device(got, kk)
        ids[lo:hi] = live_ids[order.long()]
        scores[lo:hi] = best
    return ids, scores


def _search_args(queries, corpus, row_ids, caller: str):
    """The opening of ``exact_top_k`` and ``exact_above`` (``caller``: the name their messages carry): the corpus checked
    (``corpus_suffix``), the queries as a contiguous float32 ``(q, dim)`` tensor on its device, ``row_ids`` as an int64 ``(m,)``
    one there (or None), the shapes within the kernels' limits.  Returns ``(d_q, d_ids, q, m, dim)``."""
    torch = _native.require_gpu()
    _native.load()
    corpus_suffix(corpus)
    dev = corpus.device
    with torch.cuda.device(dev):
        d_q = _on_device(torch, queries, np.float32)
        if d_q.dim() != 2 or int(d_q.shape[1]) != int(corpus.shape[1]):
            raise ValueError(f"queries must have shape (q, {int(corpus.shape[1])}); received {tuple(d_q.shape)}")
        d_q = d_q.to(device=dev, dtype=torch.float32).contiguous()
        q, m, dim = int(d_q.shape[0]), int(corpus.shape[0]), int(corpus.shape[1])
        d_ids = _rows_args(torch, corpus, row_ids, caller)
    return d_q, d_ids, q, m, dim


def _rows_args(torch, corpus, row_ids, caller: str):
    """The rows' half of :func:`_search_args` (and all of it for ``exact_pairs_above``, which has no queries): the shape within
    the kernels' limits, ``row_ids`` as an int64 ``(m,)`` tensor on the corpus's device (or None)."""
    dev = corpus.device
    m, dim = int(corpus.shape[0]), int(corpus.shape[1])
    if dim > _SCAN_MAX_DIM or m > _SCAN_MAX_ROWS:
        # (beyond the scan and beyond the rerank's entries alike: what a rerank of such rows raises, before any launch)
        raise _native.NativeLibraryError(f"{caller}: shape outside kernel limits (LSHRS_E_TOOLARGE): {m} rows of {dim} "
                                         f"elements; at most {_SCAN_MAX_ROWS} rows of {_SCAN_MAX_DIM}")
    d_ids = None
    if row_ids is not None:
        d_ids = _on_device(torch, row_ids, np.int64).to(device=dev, dtype=torch.int64).contiguous()
        if d_ids.dim() != 1 or int(d_ids.shape[0]) != m:
            raise ValueError(f"row_ids must have shape ({m},); received {tuple(d_ids.shape)}")
    return d_ids


def _finish(stats: Optional[Dict], out: Dict, tensors, return_tensors: bool):
    """The closing of both: ``out`` handed over into the caller's ``stats``, the answer as it is or as NumPy arrays."""
    if stats is not None:
        stats.clear()
        stats.update(out)
    return tensors if return_tensors else tuple(t.cpu().numpy() for t in tensors)


def exact_top_k(queries, corpus, k: int, *, row_ids=None, method: str = "auto", return_tensors: bool = False,
                stats: Optional[Dict] = None):
    """The ``k`` rows of ``corpus`` nearest to every query by cosine, exactly: ``(ids (q, kk) int64, scores (q, kk) float32)``
    with ``kk = min(k, live rows)``, scores descending, equal scores by ascending id; NumPy arrays, or device tensors with
    ``return_tensors``.

    ``queries`` (q, dim): array-like or tensor, taken as float32.  ``corpus`` (m, dim): a device tensor of float32, bfloat16,
    float16, int8 or float8_e4m3fn with a unit inner stride (any row stride: it is searched in place).  ``row_ids``: optional
    int64 (m,); a row whose entry is negative does not exist for the search, the others are returned under their entry
    (default: every row, under its index).  A score is the rerank's score of that (query, row), bit for bit.

    ``method``: "scan" - one pass over the rows on the matrix cores keeps a window of candidates per query, the window is
    rescored, and only the queries it does not settle (:func:`settled`) go through "gather"; "gather" - every query scores
    every live row with the rerank's kernels; "auto" - "scan" while ``2 k`` fits the widest window, else "gather".  Rows of
    more than 16 384 elements, or 2^31 rows and more, are beyond the scan and the rerank's entries alike: the call raises the
    ``NativeLibraryError`` (``LSHRS_E_TOOLARGE``) a rerank of them raises.
    ``stats``: a dict that receives ``queries``, ``settled_first_pass``, ``gathered``, ``window`` and ``epsilon``.

    A query or a live row of zero norm raises ``ValueError("Cannot normalize zero vector")``, as the rerank does."""
    k = _check_selection(k, method)
    torch = _native.require_gpu()
    d_q, d_ids, q, m, dim = _search_args(queries, corpus, row_ids, "exact_top_k")
    dev = corpus.device
    with torch.cuda.device(dev):
        live = m if d_ids is None else int((d_ids >= 0).sum())
        kk = min(k, live)
        use_scan, window, eps = _method_plan(k, method, corpus.dtype, dim)
        out = {"queries": q, "settled_first_pass": 0, "gathered": 0, "window": window, "epsilon": eps}
        ids = torch.empty((q, kk), dtype=torch.int64, device=dev)
        scores = torch.empty((q, kk), dtype=torch.float32, device=dev)
        todo = None                                     # queries left to the gather: None = all of them
        if q and kk and use_scan:
            w_ids, w_scores, done = _window_answer(torch, corpus, d_q, d_ids, *scan_windows(corpus, d_q, window, d_ids), kk,
                                                   window, eps + rerank_rounding(dim))
            kw = int(w_ids.shape[1])
            ids[:, :kw], scores[:, :kw] = w_ids, w_scores
            out["settled_first_pass"] = int(done.sum())
            todo = torch.from_numpy(np.flatnonzero(~done)).to(dev)
        if q and kk and (todo is None or int(todo.numel())):
            live_rows, live_ids = _live_by_id(torch, d_ids, m, dev)
            sub = d_q if todo is None else d_q[todo].contiguous()
            g_ids, g_scores = _gather(torch, corpus, sub, live_rows, live_ids, kk)
            if todo is None:
                ids, scores = g_ids, g_scores
            else:
                ids[todo], scores[todo] = g_ids, g_scores
            out["gathered"] = int(sub.shape[0])
    return _finish(stats, out, (ids, scores), return_tensors)


# ------------------------------------------------------------------------------------------
# range search: every live row at or above a cosine threshold
# ------------------------------------------------------------------------------------------
def _check_max_pairs(max_pairs) -> None:
    if int(max_pairs) < 0:
        raise ValueError(f"max_pairs must be >= 0; received {max_pairs}")


def _check_above_args(q: int, threshold, max_pairs) -> np.ndarray:
    """The thresholds of ``q`` queries as float64 ``(q,)``; ``ValueError`` for what ``exact_above`` does not take.  Pure host."""
    _check_max_pairs(max_pairs)
    try:
        t = np.asarray(threshold, dtype=np.float64)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"threshold must be a number or an array of shape ({q},)") from exc
    if t.ndim == 0:
        t = np.full(q, float(t), dtype=np.float64)
    elif t.shape != (q,):
        raise ValueError(f"threshold must be a scalar or have shape ({q},); received {t.shape}")
    if not np.all(np.isfinite(t)) or np.any(t < -1.0) or np.any(t > 1.0):
        raise ValueError("threshold must be finite and within [-1, 1]")
    return t


def above_bars(thresholds, margin: float) -> np.ndarray:
    """The first pass's bars (float32) for float64 ``thresholds``: ``t - margin`` evaluated in float64 and rounded DOWN to
    float32, where ``t`` is the lower of the threshold and its float32 value (the answer is defined by the latter).  A row
    whose rerank score reaches ``float32(threshold)`` has a cosine of at least ``t - rerank_rounding`` and an approximate score
    of at least ``t - rerank_rounding - epsilon``: with ``margin`` their sum, it is at or above its bar."""
    t = np.asarray(thresholds, dtype=np.float64)
    with np.errstate(over="ignore"):
        t = np.minimum(t, t.astype(np.float32).astype(np.float64))
    want = t - float(margin)
    bars = want.astype(np.float32)
    high = bars.astype(np.float64) > want
    bars[high] = np.nextafter(bars[high], np.float32(-np.inf))
    return bars


def scan_above(corpus, queries, bars, capacity: int, row_ids=None):
    """Device-level entry of the range search's first pass (``lshrs_scan_above_*``): ``corpus`` / ``queries`` / ``row_ids`` as
    :func:`scan_windows` takes them, ``bars`` float32 ``(q,)`` on the device.  Returns ``(query (capacity,) int32, row
    (capacity,) int64, approx (capacity,) float32, total uint64-as-int64[1], err int32[1])``: the first ``min(total,
    capacity)`` slots are pairs, in no particular order; ``total`` counts every pair that reached its bar."""
    torch = _native.require_gpu()
    q, m, dim = int(queries.shape[0]), int(corpus.shape[0]), int(corpus.shape[1])
    return _scan_emitting(corpus, "above", torch.int32, capacity, q == 0, (q, m, dim),
                          (queries.data_ptr(), q, bars.data_ptr()), row_ids)


def exact_above(queries, corpus, threshold, *, row_ids=None, max_pairs: int = 1 << 26, return_tensors: bool = False,
                stats: Optional[Dict] = None):
    """Every row of ``corpus`` at or above a cosine ``threshold`` for every query, exactly: ``(ids (total,) int64, scores
    (total,) float32, bounds (q + 1,) int64)`` - query ``i`` owns ``[bounds[i], bounds[i + 1])``, scores descending, equal scores
    by ascending id (the triple ``LSHRS.query_many(return_arrays=True)`` returns); NumPy arrays, or device tensors with
    ``return_tensors``.

    ``queries``, ``corpus``, ``row_ids``: as :func:`exact_top_k` takes them.  ``threshold``: a number, or one per query
    (shape ``(q,)``); finite and within [-1, 1], else ``ValueError`` before anything touches the GPU.  The answer of a query
    is the set of live rows whose RERANK score of that (query, row) - the float32 ``lshrs_cosine_ragged_*`` produces, which is
    the score returned - satisfies ``score >= float32(threshold)``; no more, no fewer.

    One pass over the rows on the matrix cores (``lshrs_scan_above_*``) emits every pair whose approximate score reaches
    :func:`above_bars` ``(threshold, scan_epsilon + rerank_rounding)``; the pairs are grouped by query, rescored by the
    rerank's kernel, cut at the threshold and ordered, all on the device.  One number crosses to the host: how many pairs the
    pass found.  Beyond ``max(2^20, 64 q)`` of them the pass runs a second time with room for all; beyond ``max_pairs`` the
    call raises ``ValueError`` without allocating for them.
    ``stats``: a dict that receives ``queries``, ``emitted`` (pairs the first pass let through), ``kept``, ``launches`` (1 or
    2) and ``epsilon``.

    A query or a live row of zero norm raises ``ValueError("Cannot normalize zero vector")``; rows beyond the kernels raise
    the ``NativeLibraryError`` :func:`exact_top_k` raises."""
    shape = tuple(int(v) for v in getattr(queries, "shape", ())) or tuple(np.asarray(queries).shape)
    if len(shape) != 2:
        raise ValueError(f"queries must have shape (q, dim); received {shape}")
    max_pairs = int(max_pairs)
    thr64 = _check_above_args(shape[0], threshold, max_pairs)
    torch = _native.require_gpu()
    d_q, d_ids, q, m, dim = _search_args(queries, corpus, row_ids, "exact_above")
    dev = corpus.device
    with torch.cuda.device(dev):
        eps = scan_epsilon(corpus.dtype, dim)
        out = {"queries": q, "emitted": 0, "kept": 0, "launches": 0, "epsilon": eps}
        ids = torch.empty((0,), dtype=torch.int64, device=dev)
        scores = torch.empty((0,), dtype=torch.float32, device=dev)
        bounds = torch.zeros((q + 1,), dtype=torch.int64, device=dev)
        if q and m:
            bars = torch.from_numpy(above_bars(thr64, eps + rerank_rounding(dim))).to(dev)
            t32 = torch.from_numpy(thr64.astype(np.float32)).to(dev)
            capacity = min(max(_ABOVE_FIRST_CAPACITY, 64 * q), max_pairs)
            pq, prow, emitted = _all_pairs(lambda cap: scan_above(corpus, d_q, bars, cap, d_ids), capacity, max_pairs,
                                           "exact_above", out)
            if emitted:
                # by query (stable), then the rerank's own score of every pair: its lists are the queries' runs
                pq, by_q = torch.sort(pq[:emitted].long(), stable=True)
                prow = prow[:emitted][by_q].contiguous()
                count = torch.bincount(pq, minlength=q)
                off = (torch.cumsum(count, 0) - count).contiguous()
                exact, err2 = cosine_ragged_device(corpus, d_q, prow, off, count.to(torch.int32), emitted)
                if int(err2.item()) & 5:
                    raise ValueError("Cannot normalize zero vector")
                keep = exact >= t32[pq]                 # (a NaN is not kept)
                pq, exact = pq[keep], exact[keep]
                pid = prow[keep] if d_ids is None else d_ids[prow[keep]]
                # what is left is still grouped by query.  Ascending id first; then ONE stable sort on {query, an integer that
                # descends with the score (-0.0 with 0.0)} orders every query's run by descending score, ties by the id order
                _, order = torch.sort(pid, stable=True)
                pq, exact, pid = pq[order], exact[order], pid[order]
                _, order = torch.sort((pq << 32) | _descending(torch, exact), stable=True)
                pq, exact, pid = pq[order], exact[order], pid[order]
                ids, scores = pid.contiguous(), exact.contiguous()
                bounds[1:] = torch.cumsum(torch.bincount(pq, minlength=q), 0)
                out["kept"] = int(ids.shape[0])
    return _finish(stats, out, (ids, scores, bounds), return_tensors)


# ------------------------------------------------------------------------------------------
# self-join: every pair of live rows at or above a cosine threshold
# ------------------------------------------------------------------------------------------
def scan_pairs(corpus, bar: float, capacity: int, row_ids=None, qblock: int = 0):
    """Device-level entry of the self-join's first pass (``lshrs_scan_pairs_*``): ``corpus`` / ``row_ids`` as
    :func:`scan_windows` takes them, ``bar`` one float32 for every pair, ``qblock`` the rows taken as queries per launch (0: the
    library's plan; else a multiple of 64).  Returns ``(a (capacity,) int64, b (capacity,) int64, approx (capacity,) float32,
    total uint64-as-int64[1], err int32[1])``: the first ``min(total, capacity)`` slots are pairs of row POSITIONS, ``a < b``,
    in no particular order; ``total`` counts every pair that reached the bar."""
    torch = _native.require_gpu()
    m, dim = int(corpus.shape[0]), int(corpus.shape[1])
    return _scan_emitting(corpus, "pairs", torch.int64, capacity, m == 0, (m, dim, int(qblock)), (float(bar), int(qblock)),
                          row_ids)


def _pairs_block(lib, m: int, dim: int) -> int:
    """The rows ``lshrs_scan_pairs_*`` plans to take as queries per launch, read out of the workspace's size: the image of one
    block (16 KiB per tile of 64 rows and chunk of 64 elements), 256 bytes of norms per tile, and 16 bytes."""
    nbytes = int(lib.lshrs_scan_pairs_workspace_bytes(m, dim, 0))
    if nbytes < 0:
        _native.check(nbytes, "lshrs_scan_pairs_workspace_bytes")
    return (nbytes - 16) // (-(-dim // 64) * 16384 + 256) * 64


def _rows_as_f32(torch, corpus, rows):
    """The rows ``rows`` (int64, on the device) of ``corpus`` as a contiguous float32 tensor - each element converted exactly.
    (8-bit floats are gathered as bytes: indexing is not defined for them everywhere.)"""
    if corpus.dtype.is_floating_point and corpus.element_size() == 1:
        return corpus.view(torch.uint8)[rows].view(corpus.dtype).float().contiguous()
    return corpus[rows].float().contiguous()


def _check_pairs_args(threshold, max_pairs) -> float:
    """The threshold of ``exact_pairs_above`` as a float; ``ValueError`` for what it does not take: a negative ``max_pairs``
    first, as everywhere; then what is not ONE number; then all that :func:`_check_above_args` refuses.  Pure host."""
    _check_max_pairs(max_pairs)
    try:
        t = np.asarray(threshold, dtype=np.float64)
    except (TypeError, ValueError) as exc:
        raise ValueError("threshold must be a number") from exc
    if t.ndim != 0:
        raise ValueError(f"threshold must be one number for all pairs; received an array of shape {t.shape}")
    return float(_check_above_args(1, float(t), max_pairs)[0])


def _judge_pairs(torch, corpus, d_ids, pa, pb, t32: float):
    """What a self-join does with the pairs of row positions ``(pa, pb)`` its first pass let through - the exhaustive pass of
    ``exact_pairs_above``, the buckets of ``lsh_pairs_above``: oriented by id, rescored by the rerank's kernel, cut at
    ``t32`` (the threshold as a float32) and ordered.  Returns ``(ids_a, ids_b, scores, index)``: ``ids_a < ids_b``, scores
    descending, equal scores by ascending ``(ids_a, ids_b)``; ``index`` (int64): for every pair of the answer its position in
    ``pa`` / ``pb``, so that whatever else the caller holds per pair can follow."""
    dev = corpus.device
    n, dim = int(pa.shape[0]), int(corpus.shape[1])
    index = torch.arange(n, dtype=torch.int64, device=dev)
    # the orientation is by id: the row of the lower id asks, the row of the higher id is scored
    if d_ids is not None:
        ia, ib = d_ids[pa], d_ids[pb]
        swap = ia > ib
        pa, pb = torch.where(swap, pb, pa), torch.where(swap, pa, pb)
        ia, ib = torch.where(swap, ib, ia), torch.where(swap, ia, ib)
    else:
        ia, ib = pa, pb
    # by asking row (stable): its pairs are one ragged list; the distinct asking rows a chunk at a time as queries
    pa, by_a = torch.sort(pa, stable=True)
    pb, ia, ib, index = pb[by_a].contiguous(), ia[by_a], ib[by_a], index[by_a]
    urows, count = torch.unique_consecutive(pa, return_counts=True)
    off = (torch.cumsum(count, 0) - count).contiguous()
    count32 = count.to(torch.int32)
    exact = torch.empty((n,), dtype=torch.float32, device=dev)
    err2 = torch.zeros(1, dtype=torch.int32, device=dev)
    step = max(1, _PAIRS_QUERY_BYTES // (4 * dim))
    for lo in range(0, int(urows.shape[0]), step):
        hi = min(int(urows.shape[0]), lo + step)
        queries = _rows_as_f32(torch, corpus, urows[lo:hi])
        cosine_ragged_device(corpus, queries, pb, off[lo:hi].contiguous(), count32[lo:hi].contiguous(), n,
                             scores=exact, err=err2)
    if int(err2.item()) & 5:
        raise ValueError("Cannot normalize zero vector")
    keep = exact >= t32                     # (a NaN is not kept)
    ia, ib, exact, index = ia[keep], ib[keep], exact[keep], index[keep]
    # ascending (ids_a, ids_b) by two stable sorts, then ONE stable sort on an integer that descends with the score
    # (-0.0 with 0.0): descending score, ties in the id order
    _, order = torch.sort(ib, stable=True)
    ia, ib, exact, index = ia[order], ib[order], exact[order], index[order]
    _, order = torch.sort(ia, stable=True)
    ia, ib, exact, index = ia[order], ib[order], exact[order], index[order]
    _, order = torch.sort(_descending(torch, exact), stable=True)
    return ia[order].contiguous(), ib[order].contiguous(), exact[order].contiguous(), index[order].contiguous()


def exact_pairs_above(corpus, threshold, *, row_ids=None, max_pairs: int = 1 << 26, return_tensors: bool = False,
                      stats: Optional[Dict] = None):
    """Every pair of rows of ``corpus`` at or above a cosine ``threshold``, exactly - the near-duplicates among the stored
    vectors: ``(ids_a (p,) int64, ids_b (p,) int64, scores (p,) float32)`` with ``ids_a < ids_b`` in every pair, scores
    descending, equal scores by ascending ``(ids_a, ids_b)``; NumPy arrays, or device tensors with ``return_tensors``.

    ``corpus``, ``row_ids``: as :func:`exact_top_k` takes them (live entries of ``row_ids`` are taken to be distinct).
    ``threshold``: one number, finite and within [-1, 1], else ``ValueError`` before anything touches the GPU.  The pair
    ``{a, b}`` of live rows belongs to the answer exactly when its RERANK score reaches ``float32(threshold)``, and the score of
    a pair is DEFINED with the row of the lower id, converted to float32, as the query and the row of the higher id as the row
    (``lshrs_cosine_ragged_*``; it is the score returned): the rerank's score is not symmetric in its last bit, and the ids,
    unlike the rows' positions, are the caller's.  It is the answer :func:`exact_above` ``(corpus.float(), corpus, threshold)``
    gives, cut to ``query id < row id``.

    One pass over the rows on the matrix cores (``lshrs_scan_pairs_*``) with the rows themselves as the queries, a block of
    them at a time, multiplies every unordered pair once and emits what reaches :func:`above_bars` ``(threshold, scan_epsilon
    + rerank_rounding)`` - both bounds are about the true cosine, which is symmetric, so the bar holds for either orientation;
    the distinct lower-id rows of the emitted pairs are gathered as float32 queries, in chunks of bounded memory, the rerank's
    kernel scores the pairs, and the cut and the order are made on the device.  Capacity as in :func:`exact_above`: beyond
    ``2^20`` pairs the pass runs a second time with room for all; beyond ``max_pairs`` the call raises ``ValueError``.
    ``stats``: a dict that receives ``rows``, ``emitted``, ``kept``, ``launches`` (1 or 2), ``blocks`` (row blocks of a pass)
    and ``epsilon``.

    A live row of zero norm raises ``ValueError("Cannot normalize zero vector")``; rows beyond the kernels raise the
    ``NativeLibraryError`` :func:`exact_top_k` raises."""
    max_pairs = int(max_pairs)
    t = _check_pairs_args(threshold, max_pairs)
    torch = _native.require_gpu()
    lib = _native.load()
    corpus_suffix(corpus)
    dev = corpus.device
    with torch.cuda.device(dev):
        d_ids = _rows_args(torch, corpus, row_ids, "exact_pairs_above")
        m, dim = int(corpus.shape[0]), int(corpus.shape[1])
        eps = scan_epsilon(corpus.dtype, dim)
        out = {"rows": m, "emitted": 0, "kept": 0, "launches": 0, "blocks": 0, "epsilon": eps}
        ids_a = torch.empty((0,), dtype=torch.int64, device=dev)
        ids_b = torch.empty((0,), dtype=torch.int64, device=dev)
        scores = torch.empty((0,), dtype=torch.float32, device=dev)
        if m:
            bar = float(above_bars(np.array([t]), eps + rerank_rounding(dim))[0])
            t32 = float(np.float32(t))
            out["blocks"] = -(-m // _pairs_block(lib, m, dim))
            capacity = min(_PAIRS_FIRST_CAPACITY, max_pairs)
            pa, pb, emitted = _all_pairs(lambda cap: scan_pairs(corpus, bar, cap, d_ids), capacity, max_pairs,
                                         "exact_pairs_above", out)
            if emitted:
                ids_a, ids_b, scores, _ = _judge_pairs(torch, corpus, d_ids, pa[:emitted], pb[:emitted], t32)
                out["kept"] = int(ids_a.shape[0])
    return _finish(stats, out, (ids_a, ids_b, scores), return_tensors)


# ------------------------------------------------------------------------------------------
# k-NN self-join: the k nearest OTHER live rows of every live row
# ------------------------------------------------------------------------------------------
def scan_knn(corpus, q_begin: int, q_count: int, window: int, row_ids=None, qblock: int = 0):
    """Device-level entry of the k-NN self-join's first pass (``lshrs_scan_knn_*``): ``corpus`` / ``row_ids`` as
    :func:`scan_windows` takes them, the rows ``[q_begin, q_begin + q_count)`` of the corpus as the queries, ``qblock`` the rows
    taken as queries per launch (0: the library's plan; else a multiple of 64).  Returns ``(rows (q_count, window) int64, approx
    (q_count, window) float32, count (q_count,) int32, err int32[1])`` as :func:`scan_windows` does: per query row the
    ``window`` other live rows of the largest approximate score; count 0 for a dead query row."""
    q_begin, q, window, qblock = int(q_begin), int(q_count), int(window), int(qblock)
    m, dim = int(corpus.shape[0]), int(corpus.shape[1])
    # (never empty: the entry's argument checks answer for no query rows, too)
    return _scan_selecting(corpus, "knn", "lshrs_scan_knn_workspace_bytes", q, window, False, (q, m, dim, window, qblock),
                           (q_begin, q, window, qblock), row_ids)


def _knn_chunk(block: int, dim: int, window: int) -> int:
    """Query rows of one chunk of ``exact_knn``'s scan: whole blocks (at least one) whose float32 copy and windows - rows and
    two score arrays - stay under ``_PAIRS_QUERY_BYTES``."""
    return max(1, _PAIRS_QUERY_BYTES // (4 * int(dim) + 16 * int(window)) // int(block)) * int(block)


def _drop_self(torch, g_ids, own):
    """``g_ids`` (u, kk + 1) without each row's own id ``own`` (u,), or without its last entry where the own id is not in it -
    more than ``kk`` exact duplicates of lower id pushed it out: the mask ``(u, kk + 1)`` of what stays, ``kk`` a row."""
    is_self = g_ids == own.unsqueeze(1)
    last = int(g_ids.shape[1]) - 1
    drop = torch.where(is_self.any(dim=1), is_self.to(torch.int32).argmax(dim=1), torch.full_like(own, last))
    return torch.arange(last + 1, device=g_ids.device).unsqueeze(0) != drop.unsqueeze(1)


def exact_knn(corpus, k: int, *, row_ids=None, method: str = "auto", return_tensors: bool = False,
              stats: Optional[Dict] = None):
    """The ``k`` OTHER rows of ``corpus`` nearest to every row by cosine, exactly - the k-NN graph of the stored vectors:
    ``(ids (n,) int64, neighbors (n, kk) int64, scores (n, kk) float32)``; ``n``: the live rows, in ascending order of their
    ids; ``kk = min(k, n - 1)`` (0 when ``n <= 1``); per row scores descending, equal scores by ascending id; a row is never its
    own neighbour.  NumPy arrays, or device tensors with ``return_tensors``.

    ``corpus``, ``row_ids``: as :func:`exact_top_k` takes them (live entries of ``row_ids`` are taken to be distinct).
    ``scores[i, j]`` is the RERANK score with row ``ids[i]``, converted to float32, as the query and row ``neighbors[i, j]`` as
    the row - bit for bit what ``exact_top_k(corpus.float(), corpus, ...)`` returns for that pair.  The score is oriented, not
    symmetrised (see :func:`exact_pairs_above`): ``scores`` of (a, b) and of (b, a) may differ in the last bit.

    ``method``: "scan" - the query rows go in chunks of whole blocks whose windows and float32 copy stay bounded; per chunk one
    pass over all rows on the matrix cores (``lshrs_scan_knn_*``: the rows themselves are the queries, no float32 copy is made
    for the pass and one-term rows issue one MFMA per step) keeps a window of other rows per row, the window is rescored by the
    rerank's kernel and a row is settled as :func:`settled` says - ``count < window`` here meaning that every OTHER live row
    was seen; the rows it does not settle go through "gather".  "gather" - every row, as a float32 query, scores every live
    row with the rerank's kernels for ``kk + 1`` and the row itself is removed - or the last entry, where more than ``kk``
    duplicates of lower id pushed it out.  "auto" - "scan" while ``2 k`` fits the widest window, else "gather".
    ``stats``: a dict that receives ``rows``, ``live``, ``settled_first_pass``, ``gathered``, ``window``, ``epsilon`` and
    ``chunks``.

    ``k <= 0`` or a bad ``method`` raises ``ValueError`` before anything touches the GPU; a live row of zero norm raises
    ``ValueError("Cannot normalize zero vector")``; rows beyond the kernels raise the ``NativeLibraryError``
    :func:`exact_top_k` raises."""
    k = _check_selection(k, method)
    torch = _native.require_gpu()
    lib = _native.load()
    corpus_suffix(corpus)
    dev = corpus.device
    with torch.cuda.device(dev):
        d_ids = _rows_args(torch, corpus, row_ids, "exact_knn")
        m, dim = int(corpus.shape[0]), int(corpus.shape[1])
        # in ascending order of their ids: the order of the answer, and the gather's tie rule
        live_rows, live_ids = _live_by_id(torch, d_ids, m, dev)
        n = int(live_rows.shape[0])
        kk = max(0, min(k, n - 1))
        use_scan, window, eps = _method_plan(k, method, corpus.dtype, dim)
        out = {"rows": m, "live": n, "settled_first_pass": 0, "gathered": 0, "window": window, "epsilon": eps, "chunks": 0}
        neighbors = torch.empty((n, kk), dtype=torch.int64, device=dev)
        scores = torch.empty((n, kk), dtype=torch.float32, device=dev)
        if kk:
            block = _pairs_block(lib, m, dim)
            chunk = _knn_chunk(block, dim, window) if use_scan else max(1, _PAIRS_QUERY_BYTES // (4 * dim))
            # where the answer of the row at each position goes (-1: a dead row)
            slot = torch.full((m,), -1, dtype=torch.int64, device=dev)
            slot[live_rows] = torch.arange(n, dtype=torch.int64, device=dev)
            for lo in range(0, m, chunk):
                hi = min(m, lo + chunk)
                out["chunks"] += 1
                mine = torch.nonzero(slot[lo:hi] >= 0).reshape(-1)             # the chunk's live rows, by position
                if not int(mine.numel()):
                    continue
                pos = mine + lo
                queries = _rows_as_f32(torch, corpus, pos)
                todo = None                                 # rows of `mine` left to the gather: None = all of them
                if use_scan:
                    rows, approx, count, err = scan_knn(corpus, lo, hi - lo, window, d_ids)
                    w_ids, w_scores, done = _window_answer(torch, corpus, queries, d_ids, rows[mine], approx[mine],
                                                           count[mine].contiguous(), err, kk, window, eps + rerank_rounding(dim))
                    at, kw = slot[pos], int(w_ids.shape[1])
                    neighbors[at, :kw], scores[at, :kw] = w_ids, w_scores
                    out["settled_first_pass"] += int(done.sum())
                    todo = torch.from_numpy(np.flatnonzero(~done)).to(dev)
                if todo is None or int(todo.numel()):
                    sub = queries if todo is None else queries[todo].contiguous()
                    at = slot[pos] if todo is None else slot[pos[todo]]
                    g_ids, g_scores = _gather(torch, corpus, sub, live_rows, live_ids, kk + 1)
                    stay = _drop_self(torch, g_ids, live_ids[at])
                    neighbors[at] = g_ids[stay].view(-1, kk)
                    scores[at] = g_scores[stay].view(-1, kk)
                    out["gathered"] += int(sub.shape[0])
    return _finish(stats, out, (live_ids, neighbors, scores), return_tensors)


def collision_law(scores, num_bands: int, rows_per_band: int) -> float:
    """The mean over pairs of cosine ``scores`` of ``1 - (1 - p^r)^b`` with ``p = 1 - acos(s) / pi``: the chance that sign
    random projections put such a pair into one bucket of at least one of ``b = num_bands`` bands of ``r = rows_per_band``
    bits (NaN when there is no pair).  What ``above_recall`` and ``LSHRS.recall_pairs_above`` report as ``expected``."""
    scores = np.asarray(scores, dtype=np.float64)
    if not scores.shape[0]:
        return float("nan")
    p = 1.0 - np.arccos(np.clip(scores, -1.0, 1.0)) / np.pi
    return float(np.mean(1.0 - (1.0 - p ** int(rows_per_band)) ** int(num_bands)))


def above_recall(truth_ids, truth_scores, truth_bounds, cand_ids, cand_bounds, num_bands: int, rows_per_band: int) -> Dict:
    """The bookkeeping of ``LSHRS.recall_above``, on host arrays: the truth (ids, scores, bounds of :func:`exact_above`) against
    candidate lists (ids, bounds; every id at most once per query).  Returns ``recall`` (truth pairs that are candidates /
    truth pairs, pooled over the queries; 1.0 when there is no truth), ``per_query`` (float32, NaN where a query has no
    truth), ``truth_pairs``, ``candidates`` (mean list length), ``precision`` (share of the candidate pairs that are truth; 1.0
    when there is no candidate) and ``expected``: the mean over the truth pairs of ``1 - (1 - p^r)^b`` with ``p = 1 -
    acos(s) / pi``, the chance that sign random projections put a pair of cosine ``s`` into one bucket of at least one of
    ``b = num_bands`` bands of ``r = rows_per_band`` bits (NaN when there is no truth)."""
    truth_ids = np.asarray(truth_ids, dtype=np.int64)
    truth_scores = np.asarray(truth_scores, dtype=np.float64)
    truth_bounds = np.asarray(truth_bounds, dtype=np.int64)
    cand_ids = np.asarray(cand_ids, dtype=np.int64)
    cand_bounds = np.asarray(cand_bounds, dtype=np.int64)
    n = int(truth_bounds.shape[0]) - 1
    if int(cand_bounds.shape[0]) - 1 != n:
        raise ValueError("truth and candidates must cover the same queries")
    per = np.full(n, np.nan, dtype=np.float32)
    found = 0
    for i in range(n):
        mine = truth_ids[truth_bounds[i]:truth_bounds[i + 1]]
        if mine.shape[0]:
            hit = np.intersect1d(mine, cand_ids[cand_bounds[i]:cand_bounds[i + 1]]).shape[0]
            found += hit
            per[i] = hit / mine.shape[0]
    truth_pairs, cand_pairs = int(truth_ids.shape[0]), int(cand_ids.shape[0])
    expected = collision_law(truth_scores, num_bands, rows_per_band)
    return {"recall": found / truth_pairs if truth_pairs else 1.0, "per_query": per, "truth_pairs": truth_pairs,
            "candidates": cand_pairs / n if n else 0.0, "precision": found / cand_pairs if cand_pairs else 1.0,
            "expected": expected}
