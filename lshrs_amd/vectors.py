"""``DeviceVectors`` - the indexed vectors on the GPU, under the caller's own ids, for the rerank.

``LSHRS.set_corpus`` takes a tensor whose row ``i`` is the vector of id ``i``.  The reference's ids are whatever the caller's
database uses (``index(indices, vectors)``, lshrs/core/main.py:442; primary keys from the loaders): sparse, large, not
``0 .. m-1``.  This store keeps the vectors of such ids in one device-resident row block - float32, bfloat16, float16, int8
or float8_e4m3fn, the five element types the rerank reads (``similarity.corpus_entry``) - beside an id -> row hash table in
device memory (``csrc/idmap.hip``).  A query translates its candidates' ids to rows on the device
(``lshrs_idmap_lookup_ragged_i64``, one launch between the collide step and ``lshrs_cosine_ragged_*``) and reranks them
where they are: nothing is fetched, nothing crosses the link but the answer.

Rows are append-only: adding an id again appends its new vector and moves the id to it (the table keeps the LATEST row),
removing an id only takes it out of the table.  ``compact()`` drops the rows no id points at.  No CPU compute path: the
host only moves arrays and keeps the counts.
"""

from __future__ import annotations

import threading
from typing import Any, Dict

import numpy as np

from . import _native

__all__ = ["DeviceVectors", "VECTOR_DTYPES", "NO_VECTOR_MSG"]

# what a query raises (IndexError) when a candidate's id has no row here: never added, removed, or the store attached late
NO_VECTOR_MSG = "a candidate id has no stored vector in the attached DeviceVectors"

VECTOR_DTYPES = ("float32", "bfloat16", "float16", "int8", "float8_e4m3fn")
_ITEMSIZE = {"float32": 4, "bfloat16": 2, "float16": 2, "int8": 1, "float8_e4m3fn": 1}
_QUANTIZE = {"int8": "lshrs_quantize_rows_i8", "float8_e4m3fn": "lshrs_quantize_rows_f8e4m3"}
_MIN_SLOTS = 1024
_MIN_ROWS = 1024


def _pow2_at_least(n: int) -> int:
    return 1 << max(0, int(n) - 1).bit_length()


def check_ids(ids) -> np.ndarray:
    """Ids as a one-dimensional int64 host array; a negative one raises the reference's ``ValueError`` (main.py:398)."""
    arr = np.asarray(ids.detach().cpu().numpy() if hasattr(ids, "detach") else ids)
    if arr.ndim == 0:
        arr = arr.reshape(1)
    if arr.ndim != 1:
        raise ValueError(f"ids must be one-dimensional; received shape {arr.shape}")
    if arr.dtype.kind not in "iu" and arr.size:
        arr = np.array([int(i) for i in arr.tolist()], dtype=np.int64)
    arr = np.ascontiguousarray(arr, dtype=np.int64)
    if arr.size and int(arr.min()) < 0:
        raise ValueError("index must be non-negative")
    return arr


class RowSearches:
    """The nine searches over device-resident rows under ids - the route from whatever holds such rows to ``_exact`` /
    ``_join`` / ``_groups`` / ``_knn_join`` / ``_refine``.  The holder supplies ``dim``, ``_search_snapshot() -> (rows, row_ids)`` (``row_ids``: the id of every row,
    negative where it has none; None where the id is the row) and ``translate(ids) -> (rows of those ids, ...)``; it
    receives ``last_search_stats``: what the last search that returned did."""

    def _over_rows(self, fn, *queries, members=None, **kwargs):
        """``fn(*queries, rows, row_ids=..., stats=..., **kwargs)`` over ONE snapshot of the rows and their ids; ``queries``:
        those of the two routes that have them, ``(n, dim)``.  ``members`` (the LSH join's: ids of this holder) go in as
        ``member_rows``, translated after the snapshot.  The stats are stored once ``fn`` has returned: a call that raises
        leaves the previous ones."""
        for q in queries:
            shape = tuple(int(v) for v in getattr(q, "shape", ())) or tuple(np.asarray(q).shape)
            if len(shape) != 2 or shape[1] != self.dim:
                raise ValueError(f"Vectors must have shape (n, {self.dim}); received {shape}")
        rows, row_ids = self._search_snapshot()
        if members is not None:
            kwargs["member_rows"] = self.translate(members)[0]
        stats: Dict[str, Any] = {}
        got = fn(*queries, rows, row_ids=row_ids, stats=stats, **kwargs)
        self.last_search_stats = stats
        return got

    def search(self, queries, k: int = 10, *, method: str = "auto", return_tensors: bool = False):
        """The ``k`` stored vectors nearest to every query by cosine, exactly, under the caller's ids: ``(ids (q, kk) int64,
        scores (q, kk) float32)``, ``kk = min(k, len(self))`` - :func:`lshrs_amd.exact_top_k` over the row block where it is,
        superseded and erased rows left out.  What the call did (queries settled by the first pass, queries gathered, window,
        epsilon) is left in ``last_search_stats``."""
        from ._exact import exact_top_k

        return self._over_rows(exact_top_k, queries, k=k, method=method, return_tensors=return_tensors)

    def search_above(self, queries, threshold, *, max_pairs: int = 1 << 26, return_tensors: bool = False):
        """Every stored vector at or above a cosine ``threshold`` (a number, or one per query) for every query, exactly, under
        the caller's ids: ``(ids (total,) int64, scores (total,) float32, bounds (q + 1,) int64)`` -
        :func:`lshrs_amd.exact_above` over the row block where it is, superseded and erased rows left out.  What the call did
        (pairs the first pass let through, pairs kept, launches, epsilon) is left in ``last_search_stats``."""
        from ._exact import exact_above

        return self._over_rows(exact_above, queries, threshold=threshold, max_pairs=max_pairs, return_tensors=return_tensors)

    def pairs_above(self, threshold, *, max_pairs: int = 1 << 26, return_tensors: bool = False):
        """Every pair of stored vectors at or above a cosine ``threshold`` (one number), exactly, under the caller's ids:
        ``(ids_a (p,) int64, ids_b (p,) int64, scores (p,) float32)``, ``ids_a < ids_b``, scores descending -
        :func:`lshrs_amd.exact_pairs_above` over the row block where it is, superseded and erased rows left out.  What the call
        did (rows, pairs the first pass let through, pairs kept, launches, blocks, epsilon) is left in ``last_search_stats``."""
        from ._exact import exact_pairs_above

        return self._over_rows(exact_pairs_above, threshold=threshold, max_pairs=max_pairs, return_tensors=return_tensors)

    def lsh_pairs_above(self, threshold, codes, offsets, members, num_bands: int, band_bytes: int, *, return_tensors: bool = False,
                        **kwargs):
        """The candidate pairs of ONE bucket segment (``codes``, ``offsets``, ``members``: device int64 tensors, the members
        being ids of this store) at or above a cosine ``threshold``, under the caller's ids: ``(ids_a, ids_b, scores,
        collisions)`` - :func:`lshrs_amd.lsh_pairs_above` over the row block where it is, the members translated to its rows
        (``kwargs``: its ``min_collisions``, ``max_bucket``, ``max_pairs``, ``max_raw_pairs``).  A member without a stored
        vector raises ``IndexError``.  The rows and the table are two snapshots taken one after the other, without a lock across
        both.  What the call did is left in ``last_search_stats``."""
        from ._join import lsh_pairs_above

        return self._over_rows(lsh_pairs_above, threshold=threshold, codes=codes, offsets=offsets, members=members,
                               num_bands=num_bands, band_bytes=band_bytes, return_tensors=return_tensors, **kwargs)

    def groups_above(self, threshold, *, max_pairs: int = 1 << 26, return_tensors: bool = False):
        """The near-duplicate GROUPS among the stored vectors at a cosine ``threshold``, exactly, under the caller's ids:
        ``(members (v,) int64, offsets (g + 1,) int64)`` - the connected components of :meth:`pairs_above`'s pairs
        (:func:`lshrs_amd.exact_groups_above` over the row block where it is; single linkage: two members of one group may
        score below the threshold against each other).  Groups by ascending smallest id, members ascending: the first member
        of every group is the one to keep.  What the call did (the join's counts, pairs, ids grouped, groups, the largest
        group) is left in ``last_search_stats``."""
        from ._groups import exact_groups_above

        return self._over_rows(exact_groups_above, threshold=threshold, max_pairs=max_pairs, return_tensors=return_tensors)

    def lsh_groups_above(self, threshold, codes, offsets, members, num_bands: int, band_bytes: int, *, return_tensors: bool = False,
                         **kwargs):
        """The near-duplicate GROUPS ONE bucket segment holds at a cosine ``threshold``, under the caller's ids: ``(members,
        offsets)`` - the connected components of :meth:`lsh_pairs_above`'s pairs with the same arguments
        (:func:`lshrs_amd.lsh_groups_above` over the row block where it is; every group lies inside one group of
        :meth:`groups_above`).  What the call did is left in ``last_search_stats``."""
        from ._groups import lsh_groups_above

        return self._over_rows(lsh_groups_above, threshold=threshold, codes=codes, offsets=offsets, members=members,
                               num_bands=num_bands, band_bytes=band_bytes, return_tensors=return_tensors, **kwargs)

    def neighbors(self, k: int = 10, *, method: str = "auto", return_tensors: bool = False):
        """The ``k`` OTHER stored vectors nearest to every stored vector by cosine, exactly, under the caller's ids - the k-NN
        graph of the store: ``(ids (n,) int64 ascending, neighbors (n, kk) int64, scores (n, kk) float32)``, ``kk = min(k,
        len(self) - 1)`` - :func:`lshrs_amd.exact_knn` over the row block where it is, superseded and erased rows left out.
        What the call did (rows, live rows, rows settled by the first pass, rows gathered, window, epsilon, chunks) is left in
        ``last_search_stats``."""
        from ._exact import exact_knn

        return self._over_rows(exact_knn, k=k, method=method, return_tensors=return_tensors)

    def lsh_neighbors(self, k, codes, offsets, members, num_bands: int, band_bytes: int, *, return_tensors: bool = False,
                      **kwargs):
        """For every stored vector the ``k`` best of its bucket mates in ONE bucket segment (``codes``, ``offsets``,
        ``members``: device int64 tensors, the members being ids of this store), under the caller's ids: ``(ids (n,) int64
        ascending, neighbors (n, kk) int64, scores (n, kk) float32, counts (n,) int32)`` - :func:`lshrs_amd.lsh_knn` over the
        row block where it is, the members translated to its rows (``kwargs``: its ``min_collisions``, ``max_bucket``,
        ``max_pairs``, ``max_raw_pairs``); rows behind ``counts`` are ``-1`` / ``NaN``.  A member without a stored vector raises
        ``IndexError``.  The rows and the table are two snapshots taken one after the other, without a lock across both.  What
        the call did is left in ``last_search_stats``."""
        from ._knn_join import lsh_knn

        return self._over_rows(lsh_knn, k=k, codes=codes, offsets=offsets, members=members, num_bands=num_bands,
                               band_bytes=band_bytes, return_tensors=return_tensors, **kwargs)

    def refine_neighbors(self, neighbors, k: int = 10, *, rounds: int = 1, max_degree=None, return_tensors: bool = False):
        """A k-NN graph of the stored vectors made better by its own entries: ``neighbors`` - ``(n, k_in)`` int64 ids, ``-1``
        for no entry, one row per stored id in ascending order, what :meth:`lsh_neighbors` and :meth:`neighbors` return - after
        ``rounds`` local-join rounds in which every id also considers its neighbours' neighbours, under the caller's ids:
        ``(ids (n,) int64 ascending, neighbors (n, kk) int64, scores (n, kk) float32, counts (n,) int32)`` -
        :func:`lshrs_amd.refine_knn` over the row block where it is (``max_degree``: ids with more adjacent ids connect
        nobody).  A name without a stored vector raises ``ValueError``.  What the call did is left in ``last_search_stats``."""
        from ._refine import refine_knn

        return self._over_rows(refine_knn, neighbors=neighbors, k=k, rounds=rounds, max_degree=max_degree,
                               return_tensors=return_tensors)


class TensorRows(RowSearches):
    """:class:`RowSearches` over a plain ``(m, dim)`` device tensor whose row ``i`` is the vector of id ``i``."""

    def __init__(self, table) -> None:
        self._table, self.dim = table, int(table.shape[1])
        self.last_search_stats: Dict[str, Any] = {}

    def _search_snapshot(self):
        return self._table, None

    def translate(self, ids_dev, err=None):
        return ids_dev, None            # (the id is the row)


class DeviceVectors(RowSearches):
    """Vectors of ``dim`` elements of ``dtype`` in device memory, addressed by non-negative int64 ids.

    ``dtype``: "float32", "bfloat16", "float16" (torch's round-to-nearest cast of the float32 rows), "int8" or
    "float8_e4m3fn" (``lshrs_quantize_rows_*``: a scale per row, which a cosine does not see).  ``device``: a GPU index, a
    device string or a ``torch.device`` (default: the current GPU at the first ``add``).  ``capacity``: rows to make room for
    at the first allocation (``reserve``).  Nothing is allocated - and no GPU is needed - before the first ``add`` /
    ``reserve``.

    Thread safety: one lock around everything that swaps the row block or the table; a query takes ``snapshot()`` under it
    once and holds the tensors for the length of its call.  All device work runs on the current stream of the store's
    device; ``add`` returns when its rows and ids are in place.
    """

    def __init__(self, dim: int, dtype: str = "float32", device: Any = None, capacity: int = 0) -> None:
        if int(dim) <= 0:
            raise ValueError("Vector dimensionality must be greater than zero")
        name = str(dtype).replace("torch.", "")
        if name not in VECTOR_DTYPES:
            raise ValueError(f"dtype must be one of {', '.join(VECTOR_DTYPES)}; received {dtype!r}")
        if int(capacity) < 0:
            raise ValueError("capacity must not be negative")
        self.dim = int(dim)
        self.dtype = name
        self._device_arg = device
        self._capacity_hint = int(capacity)
        self._lock = threading.RLock()
        self._dev = None
        self._block = None          # (capacity, dim) tensor of `dtype`
        self._used = 0              # rows in use (live, superseded and erased ones)
        self._table = None          # (slots, 2) int64: {id, row} per slot, -1 = empty
        self._occupied = 0          # slots that hold an id (live or erased)
        self._live = 0              # ids that have a row
        self._row_ids = None        # row -> id of the rows in use (-1: no id points at the row), built by search(); None = stale
        self.last_search_stats: Dict[str, Any] = {}

    # ------------------------------------------------------------------ plumbing
    def _torch_dtype(self, torch):
        return getattr(torch, self.dtype)

    def _device(self, torch):
        if self._dev is None:
            arg = self._device_arg
            if arg is None:
                dev = torch.device("cuda", torch.cuda.current_device())
            else:
                dev = torch.device("cuda", arg) if isinstance(arg, int) else torch.device(arg)
                if dev.type != "cuda":
                    raise ValueError(f"DeviceVectors lives on a GPU; received device {arg!r}")
                if dev.index is None or dev.index >= torch.cuda.device_count():
                    dev = torch.device("cuda", torch.cuda.current_device())
            self._dev = dev
        return self._dev

    @property
    def device(self):
        """The store's ``torch.device`` (resolved at the first use of the GPU)."""
        return self._device(_native.require_gpu())

    def _bytes_view(self, torch, block):
        return block.view(torch.uint8)      # (rows, dim * itemsize): row moves do not depend on what torch can index

    def _new_table(self, torch, slots: int):
        nbytes = int(_native.load().lshrs_idmap_bytes(slots))
        if nbytes < 0:
            _native.check(nbytes, "lshrs_idmap_bytes")
        return torch.full((slots, 2), -1, dtype=torch.int64, device=self._dev)

    def _report(self, torch):
        return torch.zeros(4, dtype=torch.int32, device=self._dev)

    def _stream(self, torch):
        return torch.cuda.current_stream(self._dev).cuda_stream

    def _ensure_rows(self, torch, need: int) -> None:
        cap = 0 if self._block is None else int(self._block.shape[0])
        if need <= cap and self._block is not None:
            return
        new_cap = max(need, 2 * cap, self._capacity_hint, _MIN_ROWS)
        block = torch.empty((new_cap, self.dim), dtype=self._torch_dtype(torch), device=self._dev)
        if self._used:
            self._bytes_view(torch, block)[:self._used].copy_(self._bytes_view(torch, self._block)[:self._used])
        self._block, self._row_ids = block, None

    def _ensure_slots(self, torch, incoming: int) -> None:
        """Room for ``incoming`` more ids: occupied slots - live and erased - stay at or below half of ``slots``."""
        slots = 0 if self._table is None else int(self._table.shape[0])
        if self._table is not None and 2 * (self._occupied + incoming) <= slots:
            return
        new_slots = max(_MIN_SLOTS, 2 * slots, _pow2_at_least(2 * (self._live + incoming)))
        table = self._new_table(torch, new_slots)
        if self._table is not None and self._live:
            report = self._report(torch)
            _native.check(_native.load().lshrs_idmap_rehash(self._table.data_ptr(), slots, table.data_ptr(), new_slots,
                                                            report.data_ptr(), self._stream(torch)), "lshrs_idmap_rehash")
            got = report.cpu().tolist()
            if got[3] or got[1] != self._live:
                raise _native.NativeLibraryError(f"lshrs_idmap_rehash moved {got[1]} of {self._live} ids")
            self._occupied = got[0]
        else:
            self._occupied = 0
        self._table = table

    def _rows_on_device(self, torch, vectors):
        """``vectors`` as a device tensor: of the store's dtype (copied as it is) or float32 (converted by ``add``)."""
        want = self._torch_dtype(torch)
        if isinstance(vectors, torch.Tensor):
            x = vectors.detach()
            if x.dtype != want:
                x = x.float()
            return x if x.device == self._dev else x.to(self._dev)
        from .similarity import _upload

        return _upload(torch, np.asarray(vectors, dtype=np.float32), self._dev)

    # ------------------------------------------------------------------ writes
    def reserve(self, n: int) -> None:
        """Room for ``n`` rows and ``n`` ids without another allocation."""
        if int(n) < 0:
            raise ValueError("n must not be negative")
        torch = _native.require_gpu()
        _native.load()
        with self._lock, torch.cuda.device(self._device(torch)):
            self._ensure_rows(torch, max(int(n), 1))
            self._ensure_slots(torch, max(0, int(n) - self._occupied))

    def add(self, ids, vectors) -> None:
        """Append ``vectors`` ``(n, dim)`` - a NumPy array or a torch tensor on any device, taken where it is when it already
        lives on the store's device - behind the last row, in the store's dtype, then point ``ids`` at the new rows.  An id
        that is there already, or occurs several times in ``ids``, ends at its latest vector.  A negative id, a wrong shape
        and - for the 8-bit dtypes - a row that holds an inf or a NaN raise ``ValueError``; nothing of the call is added then."""
        shape = tuple(int(v) for v in getattr(vectors, "shape", ())) or tuple(np.asarray(vectors).shape)
        if len(shape) != 2 or shape[1] != self.dim:
            raise ValueError(f"Vectors must have shape (n, {self.dim}); received {shape}")
        id_arr = check_ids(ids)
        n = int(id_arr.shape[0])
        if shape[0] != n:
            raise ValueError(f"Number of vectors does not match number of indices (received {shape[0]} vectors for {n} indices)")
        torch = _native.require_gpu()
        lib = _native.load()
        if n == 0:
            return
        with self._lock, torch.cuda.device(self._device(torch)):
            x = self._rows_on_device(torch, vectors)
            self._ensure_rows(torch, self._used + n)
            self._ensure_slots(torch, n)
            tail = self._block[self._used:self._used + n]
            stream = self._stream(torch)
            if x.dtype == tail.dtype:
                self._bytes_view(torch, tail).copy_(self._bytes_view(torch, x if x.is_contiguous() else x.contiguous()))
            elif self.dtype in _QUANTIZE:
                if x.stride(1) != 1:
                    x = x.contiguous()
                status = torch.empty(n, dtype=torch.uint8, device=self._dev)
                entry = _QUANTIZE[self.dtype]
                pitch = int(x.stride(0)) if n > 1 else self.dim     # (ONE row is contiguous under any row stride: v[None] has 0)
                _native.check(getattr(lib, entry)(x.data_ptr(), n, pitch, self.dim, tail.data_ptr(), self.dim,
                                                  status.data_ptr(), stream), entry)
                bad = torch.nonzero(status).reshape(-1)
                if bad.numel():         # (the rows written stay behind `_used`: the next add overwrites them)
                    row = int(bad[0])
                    why = "holds an inf or a NaN" if int(status[row]) == 1 else "is too small to scale (Q / max|x| overflows float32)"
                    raise ValueError(f"DeviceVectors.add: row {row} {why}")
            else:
                tail.copy_(x)           # (float32 as it is; 16 bits: round to nearest)
            ids_dev = torch.from_numpy(id_arr).to(self._dev)
            report = self._report(torch)
            _native.check(lib.lshrs_idmap_insert_i64(self._table.data_ptr(), int(self._table.shape[0]), ids_dev.data_ptr(), n,
                                                     self._used, report.data_ptr(), stream), "lshrs_idmap_insert_i64")
            fresh, live, neg, full = report.cpu().tolist()      # (waits: rows and ids are in place when add returns)
            if neg or full:
                raise _native.NativeLibraryError("lshrs_idmap_insert_i64: " + ("negative id" if neg else "no free slot"))
            self._occupied += fresh
            self._live += live
            self._used += n
            self._row_ids = None

    def remove(self, ids) -> int:
        """Take ``ids`` out of the store (their rows stay until ``compact()``); returns how many were there."""
        id_arr = np.asarray(ids.detach().cpu().numpy() if hasattr(ids, "detach") else ids).reshape(-1).astype(np.int64)
        if id_arr.size == 0 or self._table is None:
            return 0
        torch = _native.require_gpu()
        lib = _native.load()
        with self._lock, torch.cuda.device(self._dev):
            ids_dev = torch.from_numpy(np.ascontiguousarray(id_arr)).to(self._dev)
            count = torch.zeros(1, dtype=torch.int32, device=self._dev)
            _native.check(lib.lshrs_idmap_erase_i64(self._table.data_ptr(), int(self._table.shape[0]), ids_dev.data_ptr(),
                                                    int(id_arr.size), count.data_ptr(), self._stream(torch)),
                          "lshrs_idmap_erase_i64")
            gone = int(count.item())
            self._live -= gone
            self._row_ids = None
            return gone

    def clear(self) -> None:
        """Forget every id and row (the device memory goes back to the allocator)."""
        with self._lock:
            self._block = self._table = self._row_ids = None
            self._used = self._occupied = self._live = 0

    def compact(self) -> None:
        """Drop the rows no id points at (superseded and erased ones): the live rows gathered in their order into a block of
        their own, the ids inserted into a fresh table."""
        if self._table is None:
            return
        torch = _native.require_gpu()
        with self._lock, torch.cuda.device(self._dev):
            ids, rows = self._live_pairs(torch)
            live = int(ids.shape[0])
            cap = max(live, _MIN_ROWS)
            block = torch.empty((cap, self.dim), dtype=self._torch_dtype(torch), device=self._dev)
            if live:
                self._bytes_view(torch, block)[:live].copy_(torch.index_select(self._bytes_view(torch, self._block), 0, rows))
            self._block, self._used, self._table, self._row_ids = block, 0, None, None
            self._occupied = self._live = 0
            self._ensure_slots(torch, live)
            if live:
                report = self._report(torch)
                _native.check(_native.load().lshrs_idmap_insert_i64(self._table.data_ptr(), int(self._table.shape[0]),
                                                                    ids.data_ptr(), live, 0, report.data_ptr(),
                                                                    self._stream(torch)), "lshrs_idmap_insert_i64")
                fresh, now_live, _, full = report.cpu().tolist()
                if full or now_live != live:
                    raise _native.NativeLibraryError(f"compact: {now_live} of {live} ids re-inserted")
                self._occupied, self._live, self._used = fresh, now_live, live

    def _live_pairs(self, torch):
        """(ids, rows) of the live entries as device tensors, in row order."""
        t = self._table
        mask = (t[:, 0] >= 0) & (t[:, 1] >= 0)
        ids, rows = t[mask, 0], t[mask, 1]
        order = torch.argsort(rows)
        return ids[order].contiguous(), rows[order].contiguous()

    # ------------------------------------------------------------------ reads
    def __len__(self) -> int:
        return self._live

    def __contains__(self, item) -> bool:
        try:
            key = int(item)
        except (TypeError, ValueError):
            return False
        if key < 0 or self._table is None:
            return False
        return bool(int(self.rows_of([key])[0]) >= 0)

    def rows_of(self, ids):
        """Device int64 tensor: the row of every id, -1 where the store has none (never added, removed, negative)."""
        torch = _native.require_gpu()
        self.snapshot()                     # (an empty store answers too)
        with torch.cuda.device(self._dev):
            if isinstance(ids, torch.Tensor):
                ids_dev = ids.detach().to(device=self._dev, dtype=torch.int64).reshape(-1).contiguous()
            else:
                ids_dev = torch.from_numpy(np.ascontiguousarray(np.asarray(ids).reshape(-1).astype(np.int64))).to(self._dev)
            return self.translate(ids_dev)[0]

    def translate(self, ids_dev, err=None):
        """Flat device lookup behind the query code: (rows, table kept alive) for a device int64 tensor of ids; ``err``
        (device int32[1], optional) gets bit 8 when an id has no row."""
        torch = _native.require_gpu()
        lib = _native.load()
        _, table, slots = self.snapshot()
        out = torch.empty(ids_dev.shape, dtype=torch.int64, device=ids_dev.device)
        n = int(ids_dev.numel())
        if n:
            with torch.cuda.device(self._dev):
                _native.check(lib.lshrs_idmap_lookup_i64(table.data_ptr(), slots, ids_dev.data_ptr(), n, out.data_ptr(),
                                                         err.data_ptr() if err is not None else None, self._stream(torch)),
                              "lshrs_idmap_lookup_i64")
        return out, table

    def snapshot(self):
        """``(rows, table, slots)`` under the lock: the ``(max(rows in use, 1), dim)`` view the rerank reads, the table tensor
        and its slot count.  The caller holds the tensors for the length of its call (a concurrent growth or ``compact()``
        swaps the store's own, not these).  An empty store hands out one row that no id points at."""
        torch = _native.require_gpu()
        _native.load()
        with self._lock:
            if self._block is None or self._table is None:
                with torch.cuda.device(self._device(torch)):
                    self._ensure_rows(torch, 1)
                    self._ensure_slots(torch, 0)
            return self._block[:max(self._used, 1)], self._table, int(self._table.shape[0])

    def _search_snapshot(self):
        """``(rows, row_ids)`` under the lock: the view :meth:`snapshot` hands out and, for each of its rows, the id that
        points at it (int64, -1 for a superseded or erased row).  Built from the table's live pairs at the first search after
        a write and kept until the next ``add`` / ``remove`` / ``compact`` / ``clear`` or swap of the block."""
        torch = _native.require_gpu()
        with self._lock:
            rows, _, _ = self.snapshot()
            if self._row_ids is None or int(self._row_ids.shape[0]) != int(rows.shape[0]):
                with torch.cuda.device(self._dev):
                    row_ids = torch.full((int(rows.shape[0]),), -1, dtype=torch.int64, device=self._dev)
                    if self._live:
                        ids, at = self._live_pairs(torch)
                        row_ids[at] = ids
                    self._row_ids = row_ids
            return rows, self._row_ids

    @property
    def rows(self):
        """The ``(rows in use, dim)`` view of the row block."""
        torch = _native.require_gpu()
        with self._lock:
            if self._block is None:
                with torch.cuda.device(self._device(torch)):
                    self._ensure_rows(torch, 1)
            return self._block[:self._used]

    @property
    def table(self):
        """The ``(slots, 2)`` int64 device tensor of ``{id, row}`` slots."""
        return self.snapshot()[1]

    def stats(self) -> Dict[str, int]:
        with self._lock:
            cap = 0 if self._block is None else int(self._block.shape[0])
            slots = 0 if self._table is None else int(self._table.shape[0])
            return {"live": self._live, "rows": self._used, "dead": self._used - self._live, "capacity": cap, "slots": slots,
                    "bytes": cap * self.dim * _ITEMSIZE[self.dtype] + 16 * slots}

    # ------------------------------------------------------------------ persistence
    def save(self, path) -> None:
        """One ``.npz``: ``ids``, the live rows' raw bytes, the dtype's name and ``dim`` - what a ``compact()`` would keep
        (the store itself is left as it is)."""
        if self._table is None or self._live == 0:
            ids_h = np.empty(0, np.int64)
            raw = np.empty((0, self.dim * _ITEMSIZE[self.dtype]), np.uint8)
        else:
            torch = _native.require_gpu()
            with self._lock, torch.cuda.device(self._dev):
                ids, rows = self._live_pairs(torch)
                raw = torch.index_select(self._bytes_view(torch, self._block), 0, rows).cpu().numpy()
                ids_h = ids.cpu().numpy()
        with open(path, "wb") as fh:
            np.savez(fh, ids=ids_h, rows=raw, dtype=np.array(self.dtype), dim=np.array(self.dim, dtype=np.int64))

    @classmethod
    def load(cls, path, device: Any = None) -> "DeviceVectors":
        """The store :meth:`save` wrote, on ``device``."""
        with np.load(path) as data:
            ids, raw, name, dim = data["ids"], data["rows"], str(data["dtype"]), int(data["dim"])
        store = cls(dim, name, device=device, capacity=int(ids.shape[0]))
        if ids.shape[0]:
            torch = _native.require_gpu()
            store.add(ids, torch.from_numpy(np.ascontiguousarray(raw)).view(getattr(torch, name)).reshape(-1, dim))
        return store
