"""``LSHRS`` — the caller side of the hot path, batched for the GPU.

Thin counterpart of the reference orchestrator (lshrs/core/main.py) for exactly the
methods that reach the accelerated path: constructor, ``ingest`` / ``index`` /
``create_signatures`` / ``flush`` (signature pass) and ``query`` / ``get_top_k`` /
``get_above_p`` (signature pass + cosine rerank), plus the storage pass-throughs and the on-disk /
pickle persistence of configuration + hyperplanes (same format as the reference).
Same keyword arguments, return types, error types and messages; storage (Redis) and the
loaders (PostgreSQL / Parquet) are the reference's own components and are not re-implemented.

What is different on purpose: ``index()`` hashes a whole loader batch in ONE kernel launch
instead of looping ``ingest()`` per vector (lshrs/core/main.py:514-515), while reproducing
what that loop lets a caller observe —
  * operations are enqueued vector-major, band-minor (main.py:1125-1128);
  * the buffer is flushed, whole, at the first vector boundary where it holds at least
    ``buffer_size`` operations (main.py:1131-1143), and once more at the end (main.py:518);
  * a bad row (negative id, zero vector) raises the same ``ValueError`` after every earlier row
    was enqueued (and possibly flushed), and the trailing flush is then not reached.
tests/golden/g5_orchestration.json holds the reference's own batches for these cases.
"""

from __future__ import annotations

import itertools
import json
import logging
import warnings
from pathlib import Path
from threading import Lock
from typing import Any, Callable, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _hostblas
from . import _query_host as qh
from ._gcpause import gc_paused as _gc_paused
from .bandrows import get_optimal_config
from .hasher import LSHHasher
from .packed_ops import bucket_csr as _bucket_csr
from .similarity import corpus_entry
from .similarity import rerank_padded_arrays as _rerank_padded
from .similarity import top_k_cosine
from .storage import BucketOperation, default_storage
from .vectors import NO_VECTOR_MSG, DeviceVectors, TensorRows

logger = logging.getLogger(__name__)

VectorFetchFn = Callable[[Sequence[int]], np.ndarray]
Loader = Callable[..., Iterator[Tuple[Sequence[int], np.ndarray]]]

__all__ = ["LSHRS", "lshrs"]

_FORMAT_VERSION = "0.1.1a4"  # on-disk format version string the reference writes (main.py:882)
_ZERO_MSG = "Cannot index zero vector - norm undefined. Check embeddings for corruption."
# what pairs_above / groups_above leave in last_search_stats for an index without buckets: the join's counts, all zero
_EMPTY_JOIN_STATS = {"buckets": 0, "skipped_buckets": 0, "raw_pairs": 0, "emitted": 0, "kept": 0, "launches": 0}


def _group_lists(members: np.ndarray, offsets: np.ndarray) -> List[List[int]]:
    """``(members, offsets)`` of a grouping as one list of ids per group."""
    with _gc_paused():
        flat, at = members.tolist(), offsets.tolist()
        return [flat[lo:hi] for lo, hi in zip(at[:-1], at[1:])]


def _device_tensor(obj):
    """`obj` if it is a torch tensor on a GPU (torch is only looked at when it is already imported), else None."""
    import sys

    torch = sys.modules.get("torch")
    if torch is not None and isinstance(obj, torch.Tensor) and obj.is_cuda:
        return obj
    return None


class ReferenceBlasMismatch(UserWarning):
    """An index hashed with ``reference_blas="host"`` is being loaded on a host whose BLAS sums differently at its shape."""


def _check_recorded_blas(reference_blas: str, recorded: Optional[str], rows_per_band: int, dim: int, strict: bool) -> None:
    """The reference's keys are ``sign(P_band @ v)`` AS THE HOST'S ``sgemv`` ROUNDS IT (lshrs/hash/lsh.py:200): an index
    built with ``reference_blas="host"`` on one OpenBLAS build and queried from the other hashes tied projections differently
    wherever the two builds sum differently - a scalar tail (``dim % 4 != 0``), one-row bands, fewer than 9 elements
    (``_hostblas.builds_differ``).  ``recorded`` is the build ``save_to_disk`` / pickle wrote down.  Says so (a
    :class:`ReferenceBlasMismatch` warning naming both builds; ``strict``: ``ValueError``); silent where the builds agree."""
    if reference_blas != "host" or not recorded or not _hostblas.builds_differ(rows_per_band, dim):
        return
    here = _hostblas.host_build_name()
    if here == recorded:
        return
    msg = (f"this index was hashed with reference_blas='host' on a {recorded!r} host; this host's NumPy runs "
           f"{here!r}" + ("" if here else " (a BLAS whose summation order is not recognised)") +
           f", which sums bands of {rows_per_band} rows over {dim} elements differently: keys of near-tie projections may "
           f"differ from the stored ones.  Load with reference_blas={recorded!r} to hash as the index was built.")
    if strict:
        raise ValueError(msg)
    warnings.warn(msg, ReferenceBlasMismatch, stacklevel=3)


class _DeferredStorage:
    """What an unpickled index holds until somebody touches the storage: the reference builds a ``RedisStorage`` inside
    ``__setstate__`` (lazy TCP, lshrs/core/main.py:1010-1044); here the client may not even be importable in the
    process that unpickles (a GPU worker that only hashes), so the storage is resolved on first use."""

    def __init__(self, redis_config: Dict[str, Any]) -> None:
        object.__setattr__(self, "_cfg", dict(redis_config))
        object.__setattr__(self, "_real", None)

    def _resolve(self):
        if self._real is None:
            rc = self._cfg
            object.__setattr__(self, "_real", default_storage(
                host=rc["host"], port=rc["port"], db=rc["db"], password=rc["password"],
                decode_responses=rc["decode_responses"], prefix=rc["prefix"], max_connections=rc["max_connections"]))
        return self._real

    def __getattr__(self, item):
        if item in ("_real", "_cfg") or (item.startswith("__") and item.endswith("__")):
            raise AttributeError(item)          # (copy / pickle probe an instance whose __init__ has not run: no recursion)
        if item in ("batch_add_csr", "batch_add_packed", "get_buckets_many") and self._real is None:
            raise AttributeError(item)          # (capability probes must not open a connection)
        return getattr(self._resolve(), item)


class LSHRS:
    """Redis-backed LSH index whose hashing and reranking run on MI355X.

    Keyword arguments are those of the reference constructor (lshrs/core/main.py:154-173).
    Extras: ``hasher`` (inject a ready hasher object; default builds ``LSHHasher``), ``device`` (GPU index for
    the default hasher) and ``packed_ingest``: how ``index()`` hands a batch's buckets to the storage.
    ``"auto"`` (default): batches of at least ``packed_auto_min_ops`` operations go as ONE bucket CSR grouped on the
    device (``storage.batch_add_csr`` / ``batch_add_packed``; the reference's ``RedisStorage`` - anything with its
    ``pipeline()`` + ``bucket_key()`` - is wrapped in ``RedisPackedWriter``: one ``SADD`` per bucket) where the storage
    can take that, smaller batches and other storages get the reference's ``(band, key, id)`` tuples through
    ``batch_add``; ``True``: the array path whenever the storage can take it; ``False``: always the reference's
    operation lists, flush boundaries included (what tests/golden/g5_orchestration.json pins).  Same bucket contents
    every way (lshrs/core/main.py:1113-1143, lshrs/storage/redis.py:348-416).
    ``reference_blas``: which BLAS build the band keys are the reference's keys on (``LSHHasher``; "host" = this process's
    NumPy).  A named build is stored by ``save_to_disk`` (key ``lshrs_amd`` of metadata.json, which the reference's loader
    does not read) and by pickle, so an index and everything that queries it hash alike on any machine.
    ``keep_vectors``: ``None`` (default: the index keeps no vectors, as the reference), the name of a dtype ("float32",
    "bfloat16", "float16", "int8", "float8_e4m3fn": the index creates a :class:`DeviceVectors` on the hasher's first
    device) or a ``DeviceVectors`` to use.  ``index`` / ``ingest`` / ``create_signatures`` then also put every vector whose
    buckets they hand to the storage into that store under its id (``idx.vectors``), ``delete`` / ``clear`` take them out,
    and - while no other corpus is attached - queries rerank against it on the device: ``vector_fetch_fn`` is never called
    for a rerank.  Vectors that live on the GPU are copied / converted where they are; a host array given to ``index()`` is
    uploaded a second time for the store (the streamed chunk's device buffer is released before the buckets are handed
    over).  The store's dtype travels with ``save_to_disk`` / pickle (a restored index has an empty
    store of the same kind); the vectors themselves through ``DeviceVectors.save`` / ``load``.
    """

    def __init__(
        self,
        *,
        dim: int,
        num_perm: int = 128,
        num_bands: Optional[int] = None,
        rows_per_band: Optional[int] = None,
        similarity_threshold: float = 0.5,
        buffer_size: int = 10_000,
        vector_fetch_fn: Optional[VectorFetchFn] = None,
        storage: Any = None,
        redis_host: str = "localhost",
        redis_port: int = 6379,
        redis_db: int = 0,
        redis_password: Optional[str] = None,
        redis_prefix: str = "lsh",
        redis_max_connections: int = 50,
        decode_responses: bool = False,
        seed: int = 42,
        hasher: Any = None,
        device: Any = None,
        packed_ingest: Union[bool, str] = "auto",
        devices: Optional[Sequence[int]] = None,
        reference_blas: str = "host",
        keep_vectors: Union[None, str, DeviceVectors] = None,
    ) -> None:
        if dim <= 0:
            raise ValueError("Vector dimensionality must be greater than zero")
        if num_perm <= 0:
            raise ValueError("num_perm must be greater than zero")
        if buffer_size <= 0:
            raise ValueError("buffer_size must be greater than zero")

        if num_bands is None or rows_per_band is None:
            num_bands, rows_per_band = get_optimal_config(num_perm, similarity_threshold)
        if num_bands is None or rows_per_band is None:  # pragma: no cover - defensive, as the reference
            raise RuntimeError(
                f"Auto-config failed: get_optimal_config({num_perm}, {similarity_threshold}) "
                f"-> ({num_bands}, {rows_per_band})")
        if num_bands * rows_per_band != num_perm:
            raise ValueError(
                f"num_bands * rows_per_band must equal num_perm (received {num_bands} * {rows_per_band} != {num_perm})")

        self._dim = dim
        self._buffer_size = buffer_size
        self._vector_fetch_fn = vector_fetch_fn
        if packed_ingest not in (True, False, "auto"):
            raise ValueError("packed_ingest must be True, False or 'auto'")
        self._packed_ingest = packed_ingest
        self.packed_auto_min_ops = 8_192     # "auto": below this many (band, key, id) operations the tuples are cheaper
        self._packed_writer = None
        self._hasher = hasher if hasher is not None else LSHHasher(
            num_bands=num_bands, rows_per_band=rows_per_band, dim=dim, seed=seed, device=device, devices=devices,
            reference_blas=reference_blas)
        self._storage = storage if storage is not None else default_storage(
            host=redis_host, port=redis_port, db=redis_db, password=redis_password,
            decode_responses=decode_responses, prefix=redis_prefix, max_connections=redis_max_connections)
        self._buffer: List[BucketOperation] = []
        self._buffer_lock = Lock()
        self._corpus = None                  # device-resident vectors for the rerank (set_corpus)
        if keep_vectors is None or isinstance(keep_vectors, DeviceVectors):
            self._vectors = keep_vectors
        elif isinstance(keep_vectors, str):
            self._vectors = DeviceVectors(dim, keep_vectors, device=getattr(self._hasher, "_device", None))
        else:
            raise ValueError("keep_vectors must be None, the name of a dtype or a DeviceVectors")
        if self._vectors is not None and self._vectors.dim != dim:
            raise ValueError(f"keep_vectors holds vectors of dimension {self._vectors.dim}; the index has {dim}")
        self.last_query_stats: Dict[str, Any] = {}
        self.last_search_stats: Dict[str, Any] = {}     # what the last search_exact did (lshrs_amd.exact_top_k's stats)
        from ._query_device import DeviceBuckets

        self._dev_buckets = DeviceBuckets()  # device mirror of the store's bucket arrays (query_many)
        self._one_query: Dict[int, Any] = {}    # per device: the pinned / device buffers of the single-query chain
        self._one_table = None          # the store's segments as a device table, beside the token of their snapshot (_bucket_table)
        self._one_join = None           # ... and as ONE folded segment on the device, for the self-join (_join_segment)
        self._config: Dict[str, Any] = {
            "dim": dim, "num_perm": num_perm, "num_bands": num_bands, "rows_per_band": rows_per_band,
            "similarity_threshold": similarity_threshold, "buffer_size": buffer_size, "seed": seed,
        }
        self._redis_config: Dict[str, Any] = {
            "host": redis_host, "port": redis_port, "db": redis_db, "password": redis_password,
            "prefix": redis_prefix, "decode_responses": decode_responses, "max_connections": redis_max_connections,
        }

    # ------------------------------------------------------------------ lifecycle
    def close(self) -> None:
        self.flush()
        self._storage.close()

    def __enter__(self) -> "LSHRS":
        return self

    def __exit__(self, exc_type, exc_value, traceback) -> None:
        self.close()

    # ------------------------------------------------------------------ ingestion
    def create_signatures(self, format: str = "postgres", **loader_kwargs: Any) -> None:
        """Stream ``(indices, vectors)`` batches from a loader and index each with one launch
        (reference: main.py:315-384).  ``format`` is "postgres"/"pg", "parquet"/"pq" (the reference's
        loaders, when that package is importable) or "batches" with ``batches=<iterable>``."""
        loader = self._resolve_loader(format)
        ingest = None
        try:
            for indices, vectors in loader(**loader_kwargs):
                if ingest is None and len(indices) and self._streams_buckets(len(indices) * self._config["num_bands"]):
                    # whole loader batches, dealt round-robin to one lane per device, their buckets handed to the storage in
                    # batch order (lshrs_amd/_ingest.py): the next batch is copied and hashed while this one's buckets are
                    # grouped and stored
                    self.flush()
                    ingest = self._open_ingest()
                    ingest.__enter__()
                if ingest is None:
                    self.index(indices, vectors)
                    continue
                if len(indices) == 0:
                    continue
                if vectors is None:
                    vectors = self._require_vector_fetch_fn()(indices)
                id_arr, arr = self._check_batch(indices, vectors)
                ingest.submit(id_arr, arr)
                if ingest.failed:
                    break
        except BaseException as exc:
            if ingest is not None:
                # what was handed over is stored as the reference's sequential loop would have stored it - unless the caller is
                # being interrupted: then nothing is waited for beyond the units in flight.  A bad row in a unit already handed
                # over comes first in row order and is what is raised - with the loader's own exception chained behind it.
                try:
                    ingest.close(wait=not isinstance(exc, (KeyboardInterrupt, SystemExit)))
                except BaseException as earlier:  # noqa: BLE001
                    if earlier is not exc:
                        raise earlier from exc
            raise
        if ingest is not None:
            ingest.close()

    def ingest(self, index: int, vector) -> None:
        """Hash one vector and buffer its bucket operations (reference: main.py:386-411)."""
        if index < 0:
            raise ValueError("index must be non-negative")
        arr = self._check_dim(vector)
        keys, flag = self._hash_one(arr)
        if flag & 1:
            raise ValueError(_ZERO_MSG)
        self._enqueue_packed(int(index), keys)
        self._keep(np.array([int(index)], dtype=np.int64), arr.reshape(1, -1))
        self._flush_buffer_if_needed()

    def index(self, indices: Sequence[int], vectors: Optional[np.ndarray] = None) -> None:
        """Index a batch: one signature-pass launch, then the reference's enqueue/flush sequence
        (reference: main.py:442-518)."""
        if len(indices) == 0:
            return
        if vectors is None:
            vectors = self._require_vector_fetch_fn()(indices)
        arr = self._check_rows(indices, vectors)
        n_ops = int(arr.shape[0]) * self._config["num_bands"]
        resident = _device_tensor(arr) is not None
        if self._streams_buckets(n_ops):
            # array path, pipelined (lshrs_amd/_ingest.py): copy + signature pass chunk by chunk, every chunk's
            # keys grouped into buckets on the device under the next chunk's copy, bucket arrays to the storage in row order.
            # Anything already buffered goes first so the storage sees operations in the original order.  Vectors that already
            # live on a GPU (round 6) are hashed where they are: only the bucket arrays cross the link.
            self.flush()
            id_arr, arr = self._id_array(indices), (arr if resident else np.ascontiguousarray(arr))
            with self._open_ingest(inline=True) as ingest:
                if resident or len(self._ingest_hashers()) == 1 or arr.shape[0] < 2 * self.lane_rows:
                    ingest.submit(id_arr, arr)
                else:                       # several devices: contiguous slices of whole chunks, dealt round-robin
                    for lo in range(0, arr.shape[0], self.lane_rows):
                        ingest.submit(id_arr[lo:lo + self.lane_rows], arr[lo:lo + self.lane_rows])
            return
        rows_given = arr                    # (what the vector store takes: a tensor on the GPU stays there)
        if resident:                        # (a store that does not take arrays gets the host form of the same rows)
            arr = np.asarray(arr.detach().cpu().numpy(), dtype=np.float32)
        sink = self._packed_sink(n_ops)
        packed = sink is not None
        id_arr = self._id_array(indices) if packed else None
        ids = id_arr if packed else [int(i) for i in indices]
        keys, flags = self._hasher.hash_batch_packed(arr, return_row_flags=True)

        # first row the per-vector loop of the reference would have choked on, and why
        stop, error = len(ids), None
        if id_arr is not None:
            negs = np.flatnonzero(id_arr < 0)
            neg = int(negs[0]) if negs.size else None
        else:
            neg = next((j for j, i in enumerate(ids) if i < 0), None)
        zero_rows = np.flatnonzero(flags & 1)
        zero = int(zero_rows[0]) if zero_rows.size else None
        if neg is not None and (zero is None or neg <= zero):
            stop, error = neg, ValueError("index must be non-negative")
        elif zero is not None:
            stop, error = zero, ValueError(_ZERO_MSG)

        if packed:
            # array path: same buckets, same members, no per-operation Python objects.
            # Anything already buffered goes first so the storage sees operations in the original order.
            self.flush()
            if hasattr(sink, "batch_add_csr"):
                # the whole batch (the rows in front of a bad one) as ONE bucket CSR, grouped on the device
                if stop:
                    sink.batch_add_csr(_bucket_csr(id_arr[:stop], keys[:stop]))
            else:
                per_call = max(1, -(-self._buffer_size // keys.shape[1]))  # vectors per storage call ~ buffer_size ops
                for lo in range(0, stop, per_call):
                    hi = min(stop, lo + per_call)
                    sink.batch_add_packed(id_arr[lo:hi], keys[lo:hi])
            self._keep(id_arr[:stop], rows_given[:stop])
            if error is not None:
                raise error
            return

        # The reference's operation tuples (main.py:1113-1143), a flush WINDOW at a time: the buffer is flushed, whole, at the
        # first vector boundary where it holds at least `buffer_size` operations - so the vectors up to that boundary are known
        # from the buffer's length at the window's start, and their operations are built in one pass each over the key bytes
        # (every band key as a `bytes` object), the ids (each `num_bands` times) and the band numbers - zipped, not looped -
        # and appended under ONE lock acquisition.  Same tuples, same order, same flush boundaries as the per-vector loop
        # (tests/golden/g5_orchestration.json); 58 k -> 400 k+ vectors/s of host work at 16 bands.
        nb, bb = int(keys.shape[1]), int(keys.shape[2])
        with _gc_paused():
            key_objs = np.ascontiguousarray(keys[:stop]).reshape(-1, bb).view(np.dtype((np.void, bb)))[:, 0].tolist()
            id_objs = list(itertools.chain.from_iterable(zip(*([ids[:stop]] * nb))))      # every id num_bands times, the SAME int objects
        band_objs = list(range(nb))
        j = 0
        while j < stop:
            with self._buffer_lock:
                held = len(self._buffer)
            take = min(stop - j, max(1, -(-(self._buffer_size - held) // nb)))
            lo, hi = j * nb, (j + take) * nb
            with _gc_paused():
                ops = list(zip(band_objs * take, key_objs[lo:hi], id_objs[lo:hi]))
            with self._buffer_lock:
                self._buffer.extend(ops)
                full = len(self._buffer) >= self._buffer_size
            if full:
                self.flush()
            j += take
        self._keep(ids[:stop], rows_given[:stop])
        if error is not None:
            raise error
        self.flush()

    def flush(self) -> None:
        """Send every buffered operation in one ``batch_add``; on failure put them back in front
        and re-raise (reference: main.py:413-440)."""
        with self._buffer_lock:
            if not self._buffer:
                return
            pending = self._buffer
            self._buffer = []
        try:
            self._storage.batch_add(pending)
        except Exception as exc:
            logger.error(f"Failed to flush buffer to Redis: {exc}")
            with self._buffer_lock:
                self._buffer[0:0] = pending
            raise

    # ------------------------------------------------------------------ queries
    def query(self, vector, *, top_k: Optional[int] = 10, top_p: Optional[float] = None
              ) -> Union[List[int], List[Tuple[int, float]]]:
        """Band-collision candidates, optionally reranked by cosine (reference: main.py:524-658)."""
        query_vector = self._check_dim(vector)
        answered = self._query_one_device(query_vector, top_k, top_p)
        if answered is not None:
            return answered
        keys, flag = self._hash_one(query_vector)
        if flag & 1:
            raise ValueError(_ZERO_MSG)
        if getattr(self._storage, "prefers_batched_lookup", False):
            # array-backed buckets: one vectorised lookup for all bands and two sorts instead of a Python loop per member
            candidate_indices = self._ordered_candidates_arrays(keys[None])[0].tolist()
        else:
            counts = self._candidate_counts_from_keys(keys)
            candidate_indices = [idx for idx, _ in sorted(counts.items(), key=lambda item: (-item[1], item[0]))]
        if not candidate_indices:
            return []

        if top_p is None:
            qh.check_cut(top_k, None)
            return candidate_indices[:top_k]

        qh.check_cut(None, top_p)
        corpus = self._rerank_corpus()
        if corpus is not None:
            # the indexed vectors are resident on the device (set_corpus / keep_vectors): gathered and scored there, nothing fetched
            from .similarity import rerank_batch

            cand = np.asarray([candidate_indices], dtype=np.int64)
            if isinstance(corpus, DeviceVectors):
                corpus, cand = self._stored_rows(corpus, cand)
            ranked = rerank_batch(query_vector[None], corpus, cand, k=len(candidate_indices))[0]
        else:
            arr = qh.fetch_checked(self._require_vector_fetch_fn(), self._dim, candidate_indices)
            ranked = top_k_cosine(query_vector, arr, k=len(candidate_indices))
        scored = [(candidate_indices[pos], score) for pos, score in ranked]
        qh.check_cut(top_k, top_p)                  # (the reference looks at `top_k` behind the rerank: main.py:653)
        return scored[:int(qh.keep_counts(len(scored), top_k, top_p))]

    def _query_one_device(self, query_vector: np.ndarray, top_k, top_p):
        """:meth:`query` as ONE chain of launches with one wait at its end (``_query_device.OneQuery``: signature kernel, bucket
        lookup, collision count and order, [rerank on the attached corpus], cut - the answer straight into pinned memory), where
        the store keeps its buckets as arrays and the hasher's one-launch kernel serves the shape; None: the caller takes the
        host-counted path (any other store or hasher, a rerank through ``vector_fetch_fn``, a list beyond the kernels' capacity).
        Errors in the reference's order: zero vector, then - only if there are candidates - the arguments."""
        from . import _query_device as qd

        h = self._hasher
        try:
            if not qd.OneQuery.applies(h):
                return None
        except Exception:      # noqa: BLE001 - a hasher of another kind
            return None
        bad_p = top_p is not None and not 0 < top_p <= 1
        rerank = top_p is not None and not bad_p
        corpus, idmap = self._rerank_corpus(), None
        if rerank and isinstance(corpus, DeviceVectors):
            # the index's own vectors, under their ids: one more launch in the chain translates the candidates to rows
            corpus, *idmap = corpus.snapshot()
        if rerank:
            try:
                corpus_entry(corpus, "ragged", self._dim)       # a device corpus the rerank reads as it is (f32 / 16 / 8 bits)
            except ValueError:
                return None
        dev = corpus.device if rerank else h._torch_device()
        try:
            table = self._bucket_table(dev, h.band_bytes)
            if table is None:
                return None
            one = self._one_query.get(dev.index)
            if one is None or one.shape != (h.num_bands, h.band_bytes, h.dim):
                one = self._one_query[dev.index] = qd.OneQuery(h, dev)
            k_arg = top_k if (top_k is not None and top_k > 0) else -1
            ucount, ids, scores, flag = one.run(h, query_vector, *table, k_arg, float(top_p) if rerank else -1.0, corpus,
                                                idmap=idmap)
            if flag & 1:
                raise ValueError(_ZERO_MSG)
            if ucount < 0:
                # more pairs than the chain's fixed capacity: the batch form, which sizes its arrays by what it finds (and takes
                # lists beyond the LDS network through global memory)
                ids, scores, _ = self._query_many_device(query_vector[None], top_k if (top_k is None or top_k > 0) else None,
                                                         top_p if rerank else None, self._rerank_corpus() if rerank else None)
                ucount = len(ids)
        except qd.TooLarge:
            return None
        if ucount == 0:
            return []
        qh.check_cut(top_k, top_p)
        if scores is None:
            return ids.tolist()
        return list(zip(ids.tolist(), scores.astype(np.float64).tolist()))

    def get_top_k(self, vector, topk: int = 10) -> List[int]:
        return list(self.query(vector, top_k=topk, top_p=None))  # type: ignore[arg-type]

    def get_above_p(self, vector, p: float = 0.95) -> List[Tuple[int, float]]:
        return list(self.query(vector, top_k=None, top_p=p))  # type: ignore[arg-type]

    def set_corpus(self, corpus) -> None:
        """Attach the indexed vectors as a device-resident ``(m, dim)`` float32, bfloat16, float16, int8 or float8_e4m3fn
        tensor whose row ``i`` is the vector of id ``i``: ``query`` / ``get_above_p`` / ``query_many`` then gather their
        candidates from it on the device instead of calling ``vector_fetch_fn`` (lshrs/core/main.py:629-646 fetches and stacks
        them on the host).  16- and 8-bit rows are converted to float32 exactly inside the rerank: the scores are those of
        ``corpus.float()`` (the reference's ``np.asarray(fetch(ids), dtype=np.float32)``), at half / a quarter of the memory
        and of the bytes gathered.  ``lshrs_amd.quantize_rows`` makes the 8-bit rows (a scale per row, which a cosine does
        not see).  Or a :class:`DeviceVectors`: the vectors under the ids they were added with, whatever those are - the
        candidates' ids are translated to its rows on the device.  ``None`` detaches (an index built with ``keep_vectors``
        then reranks against its own store again)."""
        if isinstance(corpus, DeviceVectors):
            if corpus.dim != self._dim:
                raise ValueError(f"corpus must hold vectors of dimension {self._dim}")
        elif corpus is not None and (getattr(corpus, "ndim", 0) != 2 or int(corpus.shape[1]) != self._dim):
            raise ValueError(f"corpus must have shape (m, {self._dim})")
        self._corpus = corpus

    @property
    def vectors(self) -> Optional[DeviceVectors]:
        """The store ``keep_vectors`` asked for (None without it)."""
        return self._vectors

    def _rerank_corpus(self):
        """What queries rerank against on the device: the attached corpus, else the index's own vectors, else None."""
        return self._corpus if self._corpus is not None else self._vectors

    def _keep(self, ids, rows) -> None:
        """``keep_vectors``: rows whose buckets went to the storage, into the store under their ids."""
        if self._vectors is not None and len(ids):
            self._vectors.add(ids, rows)

    @staticmethod
    def _stored_rows(store: DeviceVectors, cand: np.ndarray):
        """(row block, rows of the candidate ids ``cand`` as a device tensor) - padding (-1) stays -1; an id without a stored
        vector raises."""
        from . import _native

        torch = _native.require_gpu()
        rows, _, _ = store.snapshot()
        with torch.cuda.device(rows.device):
            ids_dev = torch.from_numpy(np.ascontiguousarray(cand, dtype=np.int64)).to(rows.device)
            cand_rows, _ = store.translate(ids_dev)
            if bool(((cand_rows < 0) & (ids_dev >= 0)).any()):
                raise IndexError(NO_VECTOR_MSG)
        return rows, cand_rows

    def query_many(self, vectors, *, top_k: Optional[int] = 10, top_p: Optional[float] = None, corpus=None,
                   return_arrays: bool = False, engine: str = "auto"):
        """Batched :meth:`query`: returns ``[query(v, top_k=top_k, top_p=top_p) for v in vectors]`` with ONE
        signature launch for all queries, the collision counting and candidate ordering of all of them on the device
        (``lshrs_amd/_query_device.py``: bucket lookup in the device-resident bucket arrays, sort / count / order per query
        inside a workgroup's LDS), ONE rerank over all candidate lists and ONE copy back (reference per
        query: main.py:524-658, ``_candidate_counts`` :1088-1111).

        ``vectors``: ``(n, dim)`` array-like as in the reference - or a torch tensor that already lives on a GPU (round 6: the
        queries then never cross the link; 10 000 x 768 are 30 MB = 0.7 of the 2.7 ms a reranked batch takes).
        ``corpus``: optional device-resident ``(m, dim)`` float32, bfloat16, float16, int8 or float8_e4m3fn tensor whose row
        ``i`` is the vector of id ``i`` (default: what :meth:`set_corpus` attached); with it the candidates are gathered on
        the device and ``vector_fetch_fn`` is not called (16- and 8-bit rows are converted to float32 exactly: the scores of
        ``corpus.float()``; another dtype raises ``ValueError``) - or a :class:`DeviceVectors` (see :meth:`set_corpus`).
        ``return_arrays``: ``(ids, scores, bounds)`` instead of lists - query ``i``'s answer is ``ids[bounds[i]:bounds[i + 1]]``
        (int64) with ``scores[...]`` (float32; ``None`` without ``top_p``): no Python object per result.
        ``engine``: "auto" (the device path wherever the hasher is the HIP one; a batch with a candidate list beyond the
        kernels' 16 384 entries is counted on the host), "device" (raise instead), "host" (NumPy counting between the two
        launches: round 5's path)."""
        arr = self._query_rows(vectors)
        qh.check_cut(top_k, top_p)
        if engine not in ("auto", "device", "host"):
            raise ValueError("engine must be 'auto', 'device' or 'host'")
        if corpus is None:
            corpus = self._rerank_corpus()
        elif isinstance(corpus, DeviceVectors) and corpus.dim != self._dim:
            raise ValueError(f"corpus must hold vectors of dimension {self._dim}")
        if int(arr.shape[0]) == 0:
            empty = (np.empty(0, np.int64), None if top_p is None else np.empty(0, np.float32), np.zeros(1, np.int64))
            return empty if return_arrays else []
        on_device = (engine != "host" and callable(getattr(self._hasher, "hash_device", None))
                     and getattr(self._hasher, "tie_break", "host") == "host")
        if engine == "device" and not on_device:
            raise RuntimeError("engine='device' needs the HIP hasher")
        got = None
        if on_device:
            from ._query_device import TooLarge

            try:
                got = self._query_many_device(arr, top_k, top_p, corpus)
            except TooLarge:
                if engine == "device":
                    raise
        if got is None:
            got = self._query_many_host(arr if isinstance(arr, np.ndarray) else arr.cpu().numpy(), top_k, top_p, corpus)
        ids, scores, bounds = got
        if return_arrays:
            return ids, scores, bounds
        keep = np.diff(bounds)
        with _gc_paused():
            if scores is None:
                return qh.split_rows(ids.tolist(), keep)
            return qh.split_rows(list(zip(ids.tolist(), scores.astype(np.float64).tolist())), keep)

    def _query_rows(self, vectors):
        """The queries of a batched query or an exact search as what it works with: a float32 device tensor where
        ``vectors`` lives on a GPU (it stays there: no copy over the link, no host array; itself where it is float32 already),
        else a float32 host array; ``(n, dim)`` or the ``ValueError`` every query raises."""
        resident = _device_tensor(vectors)
        arr = resident if resident is not None else np.asarray(vectors, dtype=np.float32)
        if len(arr.shape) != 2 or int(arr.shape[1]) != self._dim:
            raise ValueError(f"Vectors must have shape (n, {self._dim}); received {tuple(arr.shape)}")
        return arr if resident is None else resident.float()

    def _searched(self, caller: str):
        """What the exact searches and the joins go over, as ``vectors.RowSearches``: the ``DeviceVectors`` the index reranks
        from, else the attached corpus on its device (a host array is uploaded) under its rows' numbers.  Without a corpus
        or a store, raises in the name of ``caller``.  The caller copies its ``last_search_stats``."""
        corpus = self._rerank_corpus()
        if corpus is None:
            self._require_vector_fetch_fn()
            raise RuntimeError(f"{caller} needs the indexed vectors on the device: set_corpus(...) or keep_vectors=...")
        if isinstance(corpus, DeviceVectors):
            return corpus
        from . import _query_device as qd

        return TensorRows(qd.corpus_on(corpus, getattr(corpus, "device", None) if _device_tensor(corpus) is not None
                                       else self._hasher._torch_device(), self._dim))

    def search_exact(self, vectors, top_k: int = 10, *, return_arrays: bool = False):
        """The ``top_k`` indexed vectors nearest to every query by cosine, EXACTLY: every vector of the attached corpus
        (:meth:`set_corpus`), else of the index's own store (``keep_vectors``), is scored - no buckets involved
        (``lshrs_amd.exact_top_k``: one pass over the rows on the matrix cores, the survivors rescored by the rerank's kernel).
        The ground truth for :meth:`recall`, and the answer where the buckets of a query hold fewer than ``top_k`` members.
        ``vectors``: as in :meth:`query_many`.  Returns per query ``[(id, score), ...]``, scores descending and equal scores by
        ascending id - or ``(ids (n, kk) int64, scores (n, kk) float32)`` with ``return_arrays``; ``kk = min(top_k, vectors
        there)``.  Without a corpus or a store it raises what a rerank without a fetch function raises.  ``last_search_stats``
        tells what the call did.  A corpus that :meth:`set_corpus` was given as a HOST array is uploaded by every call, as every
        reranked query uploads it (and twice by :meth:`recall`, once for each of its halves): attach a device tensor."""
        arr = self._query_rows(vectors)
        qh.check_cut(top_k, None)
        if top_k is None:
            raise ValueError("search_exact needs a top_k")
        over = self._searched("search_exact")
        ids, scores = over.search(arr, top_k)
        self.last_search_stats = dict(over.last_search_stats)
        if return_arrays:
            return ids, scores
        with _gc_paused():
            return [list(zip(i, s)) for i, s in zip(ids.tolist(), scores.astype(np.float64).tolist())]

    def recall(self, vectors, *, top_k: int = 10, top_p: Optional[float] = None) -> Dict[str, Any]:
        """How much of the true top ``top_k`` the index returns for these queries: :meth:`query_many` ``(vectors, top_k=top_k,
        top_p=top_p)`` against :meth:`search_exact` ``(vectors, top_k)``.  Returns ``{"recall": mean over the queries of |LSH
        ids & exact ids| / len(exact ids), "per_query": that ratio per query (float32), "exact": the exact ids (n, kk),
        "returned": mean length of the LSH answers}``.  What ``num_bands x rows_per_band`` buys on a corpus, measured."""
        got_ids, _, bounds = self.query_many(vectors, top_k=top_k, top_p=top_p, return_arrays=True)
        exact, _ = self.search_exact(vectors, top_k, return_arrays=True)
        n = int(exact.shape[0])
        per = np.zeros(n, dtype=np.float32)
        for i in range(n):
            if exact.shape[1]:
                per[i] = np.intersect1d(got_ids[bounds[i]:bounds[i + 1]], exact[i]).shape[0] / exact.shape[1]
        return {"recall": float(per.mean()) if n else 0.0, "per_query": per, "exact": exact,
                "returned": float(np.diff(bounds).mean()) if n else 0.0}

    def search_exact_above(self, vectors, threshold, *, return_arrays: bool = False):
        """Every indexed vector at or above a cosine ``threshold`` (a number, or one per query) for every query, EXACTLY: the
        range-search counterpart of :meth:`search_exact`, over the same corpus (``lshrs_amd.exact_above``) and with the same
        errors where there is none.  Returns per query ``[(id, score), ...]``, scores descending and equal scores by ascending
        id - or ``(ids, scores, bounds)`` as :meth:`query_many` returns them with ``return_arrays``.  ``last_search_stats``
        tells what the call did."""
        arr = self._query_rows(vectors)
        over = self._searched("search_exact_above")
        ids, scores, bounds = over.search_above(arr, threshold)
        self.last_search_stats = dict(over.last_search_stats)
        if return_arrays:
            return ids, scores, bounds
        with _gc_paused():
            return qh.split_rows(list(zip(ids.tolist(), scores.astype(np.float64).tolist())), np.diff(bounds))

    def pairs_exact_above(self, threshold, *, return_arrays: bool = False):
        """Every pair of indexed vectors at or above a cosine ``threshold`` (one number), EXACTLY - the near-duplicates among
        what is indexed: the self-join beside :meth:`search_exact_above`, over the same corpus
        (``lshrs_amd.exact_pairs_above``) and with the same errors where there is none.  Returns ``[(id_a, id_b, score),
        ...]`` with ``id_a < id_b``, scores descending and equal scores by ascending ``(id_a, id_b)`` - or ``(ids_a, ids_b,
        scores)`` arrays with ``return_arrays``.  ``last_search_stats`` tells what the call did."""
        over = self._searched("pairs_exact_above")
        ids_a, ids_b, scores = over.pairs_above(threshold)
        self.last_search_stats = dict(over.last_search_stats)
        if return_arrays:
            return ids_a, ids_b, scores
        with _gc_paused():
            return list(zip(ids_a.tolist(), ids_b.tolist(), scores.astype(np.float64).tolist()))

    def neighbors_exact(self, top_k: int = 10, *, return_arrays: bool = False):
        """The ``top_k`` OTHER indexed vectors nearest to every indexed vector by cosine, EXACTLY - the k-NN graph of what is
        indexed: the self-join beside :meth:`search_exact`, over the same corpus (``lshrs_amd.exact_knn``) and with the same
        errors where there is none.  Returns ``[(id, [(neighbour, score), ...]), ...]`` in ascending order of id, scores
        descending and equal scores by ascending id - or ``(ids (n,), neighbors (n, kk), scores (n, kk))`` arrays with
        ``return_arrays``.  ``last_search_stats`` tells what the call did."""
        over = self._searched("neighbors_exact")
        ids, nbrs, scores = over.neighbors(top_k)
        self.last_search_stats = dict(over.last_search_stats)
        if return_arrays:
            return ids, nbrs, scores
        with _gc_paused():
            return [(i, list(zip(nb, sc))) for i, nb, sc in zip(ids.tolist(), nbrs.tolist(), scores.astype(np.float64).tolist())]

    def recall_above(self, vectors, threshold) -> Dict[str, Any]:
        """What the index finds of the pairs it is configured for, measured: the truth is :meth:`search_exact_above`
        ``(vectors, threshold)``, the candidates are :meth:`query_many` ``(vectors, top_k=None)`` - every id that shares a
        bucket with the query.  Returns ``recall`` (truth pairs among the candidates / truth pairs, pooled over the queries;
        1.0 when there are none), ``per_query`` (float32, NaN where a query has no truth), ``truth_pairs``, ``candidates``
        (mean list length), ``precision`` (share of the candidate pairs that are truth) and ``expected``: the mean over the
        truth pairs of ``1 - (1 - p^r)^b`` with ``p = 1 - acos(s) / pi``, the collision law of this hasher's sign random
        projections (``lshrs_amd._exact.above_recall``).  The measured counterpart of ``get_optimal_config``."""
        from ._exact import above_recall

        t_ids, t_scores, t_bounds = self.search_exact_above(vectors, threshold, return_arrays=True)
        cand_ids, _, cand_bounds = self.query_many(vectors, top_k=None, return_arrays=True)
        return above_recall(t_ids, t_scores, t_bounds, cand_ids, cand_bounds, self._config["num_bands"],
                            self._config["rows_per_band"])

    def pairs_above(self, threshold, *, min_collisions: int = 1, max_bucket: Optional[int] = None, max_pairs: int = 1 << 26,
                    return_arrays: bool = False):
        """The near-duplicate pairs the index holds IN ITS BUCKETS at or above a cosine ``threshold`` (one number): the LSH
        self-join, the approximate counterpart of :meth:`pairs_exact_above` (``lshrs_amd.lsh_pairs_above``).  Two ids are a
        candidate pair when they share a bucket in at least ``min_collisions`` bands (an integer of ``1 .. num_bands``);
        buckets of more than ``max_bucket`` members (None: no limit; else ``>= 2``) count in no role - neither as a source
        of pairs nor as a collision.  Every candidate pair is reranked once, the vector of the lower id as the query, and kept
        when its score reaches ``float32(threshold)``: for ``min_collisions = 1`` and no ``max_bucket`` the answer is
        :meth:`pairs_exact_above` restricted to the candidate pairs, scores bit for bit.  Returns ``[(id_a, id_b, score,
        collisions), ...]`` with ``id_a < id_b``, scores descending and equal scores by ascending ``(id_a, id_b)`` - or the four
        arrays with ``return_arrays``.  Nothing is hashed: the pairs come out of the bucket arrays as they stand.

        The store must keep every bucket as arrays (``packed_ingest``; no op-tuple buckets, keys of at most 6 bytes, not
        Redis), else ``RuntimeError``: there is no host fallback.  Several array segments are folded into one on the host
        (``packed_ops.merge_csr``: an id once per bucket) and the folded segment is kept on the device beside the store's
        snapshot token, so that a second call folds nothing; ``last_search_stats["fold_ms"]`` says what this call's fold cost.
        An id that sits in two different buckets of one band - indexed under two signatures and never deleted - raises
        ``ValueError`` before any pair is emitted; an id in the buckets without a vector raises ``IndexError``.  That refusal
        sees COUNTED buckets only (2 .. ``max_bucket`` members): an id under a second signature whose old buckets hold nobody
        else - its old partners were deleted - is NOT refused today.  It is joined out of whatever counted buckets it sits in
        and scored under its latest vector, so every pair returned is still a pair of :meth:`pairs_exact_above` with that
        score; it is refused as soon as, in some band, its old and its new bucket both count.  The vectors and
        the buckets are two snapshots taken one after the other, without a lock across both: an ``index()`` that lands between
        them can surface as that ``IndexError``.  Without a corpus or a store the call raises what :meth:`pairs_exact_above`
        raises; an empty index gives an empty answer.  ``last_search_stats`` receives ``buckets``, ``skipped_buckets``,
        ``raw_pairs`` (pairs the counted buckets hold, with repetitions), ``emitted`` (distinct candidate pairs), ``kept``,
        ``launches`` (emit launches), ``segments_folded`` and ``fold_ms``."""
        over, seg, fold, shape, kw = self._join_plan("pairs_above", threshold, min_collisions, max_bucket, max_pairs)
        if seg is None:                             # (no segment: an empty index)
            ids_a, ids_b, scores, collisions = (np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0, np.float32),
                                                np.empty(0, np.int32))
            self.last_search_stats = dict(_EMPTY_JOIN_STATS)
        else:
            ids_a, ids_b, scores, collisions = over.lsh_pairs_above(threshold, *seg, *shape, **kw)
            self.last_search_stats = dict(over.last_search_stats)
        self.last_search_stats.update(fold)
        if return_arrays:
            return ids_a, ids_b, scores, collisions
        with _gc_paused():
            return list(zip(ids_a.tolist(), ids_b.tolist(), scores.astype(np.float64).tolist(), collisions.tolist()))

    def _join_plan(self, caller: str, threshold, min_collisions, max_bucket, max_pairs):
        """What :meth:`pairs_above` and :meth:`groups_above` do before their join: the arguments checked on the host, the rows
        that are searched, the store's buckets as one segment.  Returns ``(rows, segment or None for an empty index, fold
        stats, (num_bands, band_bytes), keywords of the join)``."""
        from . import _join

        nb, bb = int(self._config["num_bands"]), int(self._hasher.band_bytes)
        _join.check_join_args(threshold, min_collisions, max_bucket, max_pairs, nb)
        kw = {"min_collisions": int(min_collisions), "max_bucket": max_bucket, "max_pairs": int(max_pairs)}
        fold: Dict[str, Any] = {}
        over = self._searched(caller)
        seg = self._join_segment(over._search_snapshot()[0].device, bb, fold)
        if fold.pop("empty"):
            seg = None
        return over, seg, fold, (nb, bb), kw

    def groups_exact_above(self, threshold, *, return_arrays: bool = False):
        """The near-duplicate GROUPS among what is indexed at a cosine ``threshold`` (one number), EXACTLY: the connected
        components of the pairs of :meth:`pairs_exact_above`, computed on the device (``lshrs_amd.exact_groups_above``), over
        the same corpus and with the same errors where there is none.  A group is a connected component of "score >=
        threshold" - SINGLE LINKAGE: two members of one group are joined by a chain of pairs at or above the threshold and may
        score below it against each other.  Returns ``[[id, ...], ...]``: groups by ascending smallest id, ids ascending
        inside a group, only ids that are in some pair - the first id of every group is the one to keep, and dropping the
        others is a deduplication - or ``(members (v,) int64, offsets (g + 1,) int64)`` with ``return_arrays``.
        ``last_search_stats`` tells what the call did (the join's counts, ``pairs``, ``grouped``, ``groups``, ``largest``)."""
        over = self._searched("groups_exact_above")
        members, offsets = over.groups_above(threshold)
        self.last_search_stats = dict(over.last_search_stats)
        return (members, offsets) if return_arrays else _group_lists(members, offsets)

    def groups_above(self, threshold, *, min_collisions: int = 1, max_bucket: Optional[int] = None, max_pairs: int = 1 << 26,
                     return_arrays: bool = False):
        """The near-duplicate GROUPS the index holds IN ITS BUCKETS at a cosine ``threshold``: the connected components of the
        pairs of :meth:`pairs_above` with the same arguments, computed on the device (``lshrs_amd.lsh_groups_above``) - the
        approximate counterpart of :meth:`groups_exact_above`.  A group is a connected component - SINGLE LINKAGE: two members
        of one group may neither share a bucket nor reach the threshold against each other.  The pairs are a subset of
        :meth:`pairs_exact_above`'s, so every group lies inside ONE group of :meth:`groups_exact_above`: the buckets split
        groups, they never merge them.  Returns ``[[id, ...], ...]`` as :meth:`groups_exact_above` does (the first id of a
        group is its smallest id, the one to keep), or ``(members, offsets)`` with ``return_arrays``; an empty index gives
        ``[]``.  The store, the errors and the two snapshots: as for
        :meth:`pairs_above`.  ``last_search_stats`` receives what :meth:`pairs_above` leaves there and ``pairs``, ``grouped``,
        ``groups``, ``largest``."""
        over, seg, fold, shape, kw = self._join_plan("groups_above", threshold, min_collisions, max_bucket, max_pairs)
        if seg is None:
            members, offsets = np.empty(0, np.int64), np.zeros(1, np.int64)
            self.last_search_stats = dict(_EMPTY_JOIN_STATS, pairs=0, grouped=0, groups=0, largest=0)
        else:
            members, offsets = over.lsh_groups_above(threshold, *seg, *shape, **kw)
            self.last_search_stats = dict(over.last_search_stats)
        self.last_search_stats.update(fold)
        return (members, offsets) if return_arrays else _group_lists(members, offsets)

    def recall_groups_above(self, threshold) -> Dict[str, Any]:
        """How much of the exact grouping the index recovers, measured as the duplicates a deduplication would remove: the
        truth is :meth:`groups_exact_above` ``(threshold)``, what the index finds is :meth:`groups_above` ``(threshold)``,
        whose groups refine the truth's.  Returns ``groups`` / ``truth_groups``, ``removable`` (the sum over the LSH groups
        of ``size - 1``: the ids that go when one per group is kept) / ``truth_removable`` (the same over the exact groups),
        ``recall = removable / truth_removable`` (at most 1; 1.0 when there is no truth) and ``largest`` /
        ``truth_largest``.  ``last_search_stats`` is that of the :meth:`groups_above` call."""
        t_members, t_offsets = self.groups_exact_above(threshold, return_arrays=True)
        members, offsets = self.groups_above(threshold, return_arrays=True)
        groups, truth_groups = int(offsets.shape[0]) - 1, int(t_offsets.shape[0]) - 1
        removable, truth_removable = int(members.shape[0]) - groups, int(t_members.shape[0]) - truth_groups
        return {"groups": groups, "truth_groups": truth_groups, "removable": removable, "truth_removable": truth_removable,
                "recall": removable / truth_removable if truth_removable else 1.0,
                "largest": int(np.diff(offsets).max()) if groups else 0,
                "truth_largest": int(np.diff(t_offsets).max()) if truth_groups else 0}

    def neighbors(self, top_k: int = 10, *, min_collisions: int = 1, max_bucket: Optional[int] = None, max_pairs: int = 1 << 26,
                  return_arrays: bool = False, refine_rounds: int = 0, max_degree: Optional[int] = None):
        """For every indexed vector the ``top_k`` best of the vectors it shares a bucket with - the k-NN graph the index holds
        IN ITS BUCKETS, the approximate counterpart of :meth:`neighbors_exact` (``lshrs_amd.lsh_knn``).  The candidates of an
        id are the ids it forms a candidate pair with as :meth:`pairs_above` defines one (a shared bucket in at least
        ``min_collisions`` bands; buckets of more than ``max_bucket`` members count in no role); they are reranked with the
        id's own vector as the query and ordered by descending score, equal scores by ascending id.  For ``min_collisions =
        1`` and no ``max_bucket`` an id's list is :meth:`neighbors_exact`'s ranking of that id restricted to its candidates,
        scores bit for bit; an id with fewer than ``top_k`` candidates has a shorter list, one with none an empty one.
        Returns ``[(id, [(neighbour, score), ...]), ...]`` in ascending order of id, the form of :meth:`neighbors_exact` - or,
        with ``return_arrays``, ``(ids (n,), neighbors (n, kk), scores (n, kk), counts (n,))`` with ``-1`` / ``NaN`` behind
        each row's ``counts``.  Nothing is hashed: the candidates come out of the bucket arrays as they stand.  An empty index
        gives an empty answer.

        The store, the errors, ``max_pairs`` (distinct candidate pairs) and the two snapshots: as for :meth:`pairs_above`.
        ``last_search_stats`` receives ``buckets``, ``skipped_buckets``, ``raw_pairs``, ``emitted``, ``launches``, ``rows``,
        ``live``, ``candidates_max``, ``short_rows`` (ids with fewer than ``kk`` candidates), ``long_lists``,
        ``segments_folded`` and ``fold_ms``.

        ``refine_rounds`` (default 0: the buckets' graph as it is): that many local-join rounds over the graph
        (``lshrs_amd.refine_knn``) - every id also considers its neighbours' neighbours, and its list becomes
        :meth:`neighbors_exact`'s ranking of it restricted to the ids within two steps, scores bit for bit; no score of a list
        ever decreases.  ``max_degree`` (None: no cap): an id with more adjacent ids connects nobody.  ``last_search_stats``
        then carries the refinement's own under ``"refine"``."""
        from ._knn_join import _check_k
        from ._refine import check_refine_args

        top_k = _check_k(top_k)
        refine_rounds, max_degree, _ = check_refine_args(refine_rounds, max_degree)
        over, seg, fold, shape, kw = self._join_plan("neighbors", 0.0, min_collisions, max_bucket, max_pairs)
        if seg is None:                             # (no bucket holds anybody: a segment without buckets - every list is empty)
            from . import _native

            torch = _native.require_gpu()
            dev = over._search_snapshot()[0].device
            seg = (torch.empty(0, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                   torch.empty(0, dtype=torch.int64, device=dev))
        ids, nbrs, scores, counts = over.lsh_neighbors(top_k, *seg, *shape, **kw)
        self.last_search_stats = dict(over.last_search_stats)
        self.last_search_stats.update(fold)
        if refine_rounds:
            found = ids
            ids, nbrs, scores, counts = over.refine_neighbors(nbrs, top_k, rounds=refine_rounds, max_degree=max_degree)
            if not np.array_equal(found, ids):
                raise RuntimeError("neighbors: the index changed between the buckets' graph and its refinement")
            self.last_search_stats["refine"] = dict(over.last_search_stats)
        if return_arrays:
            return ids, nbrs, scores, counts
        with _gc_paused():
            return [(i, list(zip(nb[:c], sc[:c]))) for i, nb, sc, c in
                    zip(ids.tolist(), nbrs.tolist(), scores.astype(np.float64).tolist(), counts.tolist())]

    def recall_neighbors(self, top_k: int = 10, refine_rounds: int = 0) -> Dict[str, Any]:
        """What the LSH k-NN graph finds of the true one, measured: the truth is :meth:`neighbors_exact` ``(top_k)``, what the
        index finds is :meth:`neighbors` ``(top_k)``.  Returns ``recall`` (the truth's (id, neighbour) entries that are in the
        found list of the same id / the truth's entries, pooled over the ids; 1.0 when there are none), ``per_row`` (float32,
        that share id by id in ascending order of id; NaN where an id has no truth), ``truth_entries``, ``found_entries``,
        ``short_rows`` (ids whose buckets hold fewer than ``kk`` candidates) and ``expected``: the mean over the truth's
        scores of the collision law :meth:`recall_above` reports (``lshrs_amd._exact.collision_law``; NaN when there is no
        truth).  An entry is found only under ITS OWN ID: where a truth neighbour ties bit for bit with the ``kk``-th and the
        found list holds the other id of the tie, the entry counts as missed.  ``last_search_stats`` is that of the
        :meth:`neighbors` call.  ``refine_rounds``: measure :meth:`neighbors` ``(top_k, refine_rounds=refine_rounds)``
        instead - ``short_rows`` is then the refinement's, ``expected`` stays the law of the buckets alone."""
        from ._exact import collision_law
        from ._refine import check_refine_args

        check_refine_args(refine_rounds, None)
        t_ids, t_nbrs, t_scores = self.neighbors_exact(top_k, return_arrays=True)
        ids, nbrs, _, counts = self.neighbors(top_k, return_arrays=True, refine_rounds=refine_rounds)
        if not np.array_equal(t_ids, ids):
            raise RuntimeError("recall_neighbors: the index changed between its two searches")
        n, kk = int(t_nbrs.shape[0]), int(t_nbrs.shape[1])
        hit = np.zeros(n, dtype=np.int64)
        if n and kk:
            # (id, neighbour) as one int64 per entry of the found lists - the row's rank above the neighbour's place among all
            # ids - and the truth's entries looked up among them
            rank = np.searchsorted(ids, nbrs.clip(min=0))
            own = np.arange(n, dtype=np.int64)[:, None]
            found = np.sort((own * n + rank)[nbrs >= 0])
            want = own * n + np.searchsorted(ids, t_nbrs)
            at = np.searchsorted(found, want).clip(max=max(0, found.shape[0] - 1))
            hit = ((found[at] == want) if found.shape[0] else np.zeros_like(want, dtype=bool)).sum(axis=1)
        truth_entries = n * kk
        per = (hit / kk).astype(np.float32) if kk else np.full(n, np.nan, dtype=np.float32)
        return {"recall": int(hit.sum()) / truth_entries if truth_entries else 1.0, "per_row": per,
                "truth_entries": truth_entries, "found_entries": int(counts.sum()),
                "short_rows": int(self.last_search_stats.get("refine", self.last_search_stats).get("short_rows", 0)),
                "expected": collision_law(t_scores.reshape(-1), self._config["num_bands"], self._config["rows_per_band"])}

    def _join_segment(self, dev, band_bytes: int, fold: Dict[str, Any]):
        """The store's bucket arrays as ONE segment on ``dev`` - ``(codes, offsets, members)`` int64 tensors, None for an empty
        index - folded where the store holds several (``_join.fold_segments``) and kept beside the token that came back with the
        segments, as :meth:`_bucket_table` keeps its table.  ``fold`` receives ``segments_folded``, ``fold_ms`` (both 0 where
        the kept segment served) and ``empty``.  A store that does not keep every bucket as arrays raises ``RuntimeError``."""
        from . import _join, _native

        torch = _native.require_gpu()
        st = self._resolved_storage()
        fold.update(segments_folded=0, fold_ms=0.0, empty=False)
        token_fn = getattr(st, "array_segments_token", None)
        kept = self._one_join
        if kept is not None and callable(token_fn) and kept[0] == (id(st), token_fn(), band_bytes, dev.index):
            fold["empty"] = kept[1] is None
            return kept[1]
        if callable(getattr(st, "array_segments_snapshot", None)):
            segs, token = st.array_segments_snapshot(band_bytes)
        else:
            segs, token = (st.array_segments(band_bytes) if callable(getattr(st, "array_segments", None)) else None), None
        if segs is None:
            raise RuntimeError("pairs_above joins on the store's bucket arrays: it needs a store that keeps every bucket as "
                               "arrays (packed_ingest into InMemoryStorage, band keys of at most 6 bytes; no op-tuple buckets)")
        one, fold_ms, folded = _join.fold_segments(segs)
        seg = None
        if one is not None and int(one.members.shape[0]):
            with torch.cuda.device(dev):
                seg = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)
                            for a in (one.codes, one.offsets, one.members))
        fold.update(segments_folded=folded, fold_ms=fold_ms, empty=seg is None)
        self._one_join = None if token is None else ((id(st), token, band_bytes, dev.index), seg, st)
        return seg

    def recall_pairs_above(self, threshold) -> Dict[str, Any]:
        """What the LSH self-join finds of the true near-duplicate pairs, measured: the truth is :meth:`pairs_exact_above`
        ``(threshold)``, what the index finds is :meth:`pairs_above` ``(threshold)`` - a subset of the truth, judged by the same
        kernel.  Returns ``recall`` (``kept / truth_pairs``; 1.0 when there is no truth), ``precision`` (``kept / emitted``:
        the share of the candidate pairs that reach the threshold; 1.0 when nothing was emitted), ``truth_pairs``,
        ``candidates`` (distinct candidate pairs), ``kept`` and ``expected``: the mean over the truth pairs of the collision
        law :meth:`recall_above` reports (``lshrs_amd._exact.collision_law``; NaN when there is no truth)."""
        from ._exact import collision_law

        _, _, t_scores = self.pairs_exact_above(threshold, return_arrays=True)
        ids_a, _, _, _ = self.pairs_above(threshold, return_arrays=True)
        truth_pairs, kept, emitted = int(t_scores.shape[0]), int(ids_a.shape[0]), int(self.last_search_stats["emitted"])
        return {"recall": kept / truth_pairs if truth_pairs else 1.0, "precision": kept / emitted if emitted else 1.0,
                "truth_pairs": truth_pairs, "candidates": emitted, "kept": kept,
                "expected": collision_law(t_scores, self._config["num_bands"], self._config["rows_per_band"])}

    def _query_many_device(self, arr, top_k, top_p, corpus):
        """``query_many`` with everything between the upload of the queries and the download of the answers on the device."""
        from . import _native
        from . import _query_device as qd

        torch = _native.require_gpu()
        nq = int(arr.shape[0])
        idmap = None
        if isinstance(corpus, DeviceVectors) and top_p is not None:
            corpus, *idmap = corpus.snapshot()
        if _device_tensor(corpus) is not None:
            dev = corpus.device
        elif isinstance(arr, torch.Tensor):
            dev = arr.device
        else:
            dev = self._hasher._torch_device()
        with torch.cuda.device(dev):
            x = qd.queries_on(arr, dev)
            flags = torch.empty(nq, dtype=torch.uint8, device=dev)
            keys_dev = self._hasher.hash_device(x, row_flags=flags)
            if bool((flags & 1).any()):
                raise ValueError(_ZERO_MSG)
            lists = self._device_lists(qd, keys_dev, dev)
            # (diagnostics of the last device-counted batch: bench.py's candidates/s; not part of the answer)
            self.last_query_stats = {"queries": nq, "pairs": lists.total, "longest_list": lists.max_pairs, "engine": "device",
                                     "segments": lists.segments}
            if top_p is None:
                return qd.rank_and_cut(lists, top_k, None)
            if lists.total == 0:
                return np.empty(0, np.int64), np.empty(0, np.float32), np.zeros(nq + 1, np.int64)
            if corpus is not None:
                return qd.rank_and_cut(lists, top_k, top_p, queries_dev=x, corpus=qd.corpus_on(corpus, dev, self._dim),
                                       idmap=idmap)
            # no resident corpus: the candidates' vectors come from the caller's fetch function, list by list as the reference
            # asks for them (main.py:629), and travel to the device as one table; candidate j reads row `rows[j]` of it
            ucount = lists.ucount.cpu().numpy()
            at = qh.ragged_positions(lists.pair_off.cpu().numpy()[:nq], ucount)      # where the lists sit in `cand_ids`
            table = qh.fetch_table(self._require_vector_fetch_fn(), self._dim, lists.cand_ids.cpu().numpy()[at],
                                   np.r_[0, np.cumsum(ucount)])
            rows = np.zeros(max(1, lists.total), dtype=np.int64)
            rows[at] = np.arange(at.shape[0], dtype=np.int64)
            return qd.rank_and_cut(lists, top_k, top_p, queries_dev=x, corpus=qd.upload(torch, table, dev),
                                   cand_rows=qd.upload(torch, rows, dev))

    def _device_lists(self, qd, keys_dev, dev):
        """Every query's candidates, counted and ordered on the device: from the device mirror of the store's bucket arrays
        where the store keeps arrays, else from one ``get_bucket`` per (query, band) (the reference's storage interface,
        lshrs/storage/redis.py:282) with the pairs handed over flat."""
        nq, nb, bb = (int(v) for v in keys_dev.shape)
        table = self._bucket_table(dev, bb)
        if table is not None:
            return qd.candidates_from_index(keys_dev, *table)
        q, bands, members = qh.bucket_pairs(self._resolved_storage(), keys_dev.cpu().numpy())
        return qd.candidates_from_pairs(members, bands, np.searchsorted(q, np.arange(nq + 1)).astype(np.int64), nb, dev)

    def _bucket_table(self, dev, band_bytes: int):
        """``DeviceBuckets.table`` of the store's bucket arrays on ``dev``, or None where the store does not keep every bucket
        of this key width as arrays (the caller reads it through ``get_bucket``).  Kept beside the token that came back WITH the
        segments (``array_segments_snapshot``: one acquisition of the store's lock): while the store does not change a call
        costs one token comparison, and an ``index()`` that lands behind the snapshot is seen by the next call.  A store that
        only has ``array_segments`` is asked every time."""
        st = self._resolved_storage()
        token_fn = getattr(st, "array_segments_token", None)
        kept = self._one_table
        if kept is not None and callable(token_fn) and kept[0] == (id(st), token_fn(), band_bytes, dev.index):
            return kept[1]
        if callable(getattr(st, "array_segments_snapshot", None)):
            segs, token = st.array_segments_snapshot(band_bytes)
        else:                                       # (a store of another kind: nothing to keep the answer beside)
            segs, token = (st.array_segments(band_bytes) if callable(getattr(st, "array_segments", None)) else None), None
        if segs is None:
            return None
        table = self._dev_buckets.table(segs, dev)
        # (with it what the descriptor points into - the segments, the mirror's device arrays - and the store, whose id is the key)
        self._one_table = None if token is None else ((id(st), token, band_bytes, dev.index), table, segs,
                                                        self._dev_buckets._table, st)
        return table

    def _query_many_host(self, arr: np.ndarray, top_k, top_p, corpus):
        """``query_many`` with the collision counting in NumPy between the signature launch and the rerank launch (round 5;
        what hashers without ``hash_device`` and batches beyond the device path's limits take).  Same arrays out."""
        nq = arr.shape[0]
        keys, flags = self._hasher.hash_batch_packed(arr, return_row_flags=True)
        if (flags & 1).any():
            raise ValueError(_ZERO_MSG)
        um, bounds = self._ordered_candidates_arrays(keys)
        lens = np.diff(bounds)
        if top_p is None:
            keep = qh.keep_counts(lens, top_k, None)
            return um[qh.ragged_positions(bounds[:-1], keep)], None, np.r_[0, np.cumsum(keep)].astype(np.int64)

        # rerank every non-empty candidate list in one launch: a (q, c_max) index matrix padded with -1
        # (out-of-range entries score NaN, which the device sort places last)
        c_max = int(lens.max()) if nq else 0
        if c_max == 0:
            return np.empty(0, np.int64), np.empty(0, np.float32), np.zeros(nq + 1, np.int64)
        rows = np.repeat(np.arange(nq, dtype=np.int64), lens)
        cols = np.arange(um.shape[0], dtype=np.int64) - np.repeat(bounds[:-1], lens)
        cand_ids = np.full((nq, c_max), -1, dtype=np.int64)
        cand_ids[rows, cols] = um
        if corpus is None:
            table = qh.fetch_table(self._require_vector_fetch_fn(), self._dim, um, bounds)
            cand = np.full((nq, c_max), -1, dtype=np.int64)
            cand[rows, cols] = np.arange(um.shape[0], dtype=np.int64)     # row of `table` = position in the flat list
        elif isinstance(corpus, DeviceVectors):
            table, cand = self._stored_rows(corpus, cand_ids)
        else:
            table, cand = corpus, cand_ids
        order, scores = _rerank_padded(arr, table, cand)                   # (q, c_max): positions, descending scores
        keep = qh.keep_counts(lens, top_k, top_p)
        krows = np.repeat(np.arange(nq, dtype=np.int64), keep)
        kcols = np.arange(int(keep.sum()), dtype=np.int64) - np.repeat(np.cumsum(keep) - keep, keep)
        return (cand_ids[krows, order[krows, kcols]], np.ascontiguousarray(scores[krows, kcols], dtype=np.float32),
                np.r_[0, np.cumsum(keep)].astype(np.int64))

    # ------------------------------------------------------------------ storage pass-throughs
    def delete(self, indices: Union[int, Sequence[int]]) -> None:
        """Remove ids from every bucket (reference: main.py:744-784)."""
        to_remove = [indices] if isinstance(indices, int) else [int(i) for i in indices]
        self._storage.remove_indices(to_remove)
        if self._vectors is not None:
            self._vectors.remove(to_remove)

    def clear(self) -> None:
        """Flush what is buffered, then drop every bucket (reference: main.py:786-796)."""
        self.flush()
        self._storage.clear()
        if self._vectors is not None:
            self._vectors.clear()

    def stats(self) -> Dict[str, Any]:
        """Static configuration summary (reference: main.py:798-840)."""
        return {
            "dimension": self._dim, "num_perm": self._config["num_perm"], "num_bands": self._config["num_bands"],
            "rows_per_band": self._config["rows_per_band"], "buffer_size": self._buffer_size,
            "similarity_threshold": self._config["similarity_threshold"], "redis_prefix": self._redis_config["prefix"],
        }

    # ------------------------------------------------------------------ persistence (same on-disk format)
    def save_to_disk(self, path) -> None:
        """``metadata.json`` (version, config, redis config with the password redacted) + ``projections.npz``
        (``arr_0 .. arr_{bands-1}``), the reference's format (main.py:846-895): an index saved by either
        implementation loads in the other.  Bucket contents live in the storage backend, not here."""
        self.flush()
        out = Path(path)
        out.mkdir(parents=True, exist_ok=True)
        redis_cfg = self._redis_config.copy()
        if "password" in redis_cfg:
            redis_cfg["password"] = "<REDACTED>"
        with open(out / "metadata.json", "w") as fh:
            meta = {"version": _FORMAT_VERSION, "config": self._config, "redis_config": redis_cfg}
            # (a key of our own: the reference's load_from_disk reads the three above only.)  Which BLAS the keys are the
            # reference's keys ON: the named build, or - for "host" - the build this host's NumPy was recognised as, so that a
            # loader on the other kind of host can tell (`_check_recorded_blas`)
            meta["lshrs_amd"] = self._blas_record()
            if self._vectors is not None:           # (the store's kind, not its vectors: DeviceVectors.save / load carry those)
                meta["lshrs_amd"]["keep_vectors"] = self._vectors.dtype
            json.dump(meta, fh, indent=2)
        np.savez_compressed(out / "projections.npz", *self._hasher.projections)

    @classmethod
    def load_from_disk(cls, path, *, redis_config: Optional[Dict[str, Any]] = None,
                       vector_fetch_fn: Optional[VectorFetchFn] = None, storage: Any = None,
                       reference_blas: Optional[str] = None, strict_blas: Optional[bool] = None) -> "LSHRS":
        """Rebuild from :meth:`save_to_disk` output (reference: main.py:898-983).  The stored hyperplanes
        replace the freshly drawn ones — assigning ``_hasher.projections`` re-uploads the device image.
        ``reference_blas``: override the stored choice (e.g. the build a ``"host"`` index was recorded on);
        ``strict_blas``: raise instead of warning when a ``"host"`` index is loaded on a host whose BLAS sums its shape
        differently (default: the class attribute ``LSHRS.strict_blas``)."""
        src = Path(path)
        if not src.exists():
            raise FileNotFoundError(f"Directory not found: {src}")
        with open(src / "metadata.json") as fh:
            meta = json.load(fh)
        cfg = meta["config"]
        redis_cfg = meta["redis_config"].copy()
        if redis_config:
            redis_cfg.update(redis_config)
        extra = meta.get("lshrs_amd", {})
        blas = extra.get("reference_blas", "host") if reference_blas is None else reference_blas
        blas = _hostblas.LEGACY_BUILD_NAMES.get(blas, blas)
        _check_recorded_blas(blas, extra.get("host_blas"), cfg["rows_per_band"], cfg["dim"],
                             cls.strict_blas if strict_blas is None else strict_blas)
        inst = cls(
            dim=cfg["dim"], num_perm=cfg["num_perm"], num_bands=cfg["num_bands"], rows_per_band=cfg["rows_per_band"],
            similarity_threshold=cfg["similarity_threshold"], buffer_size=cfg["buffer_size"],
            vector_fetch_fn=vector_fetch_fn, storage=storage, redis_host=redis_cfg["host"], redis_port=redis_cfg["port"],
            redis_db=redis_cfg["db"], redis_password=redis_cfg["password"], redis_prefix=redis_cfg["prefix"],
            decode_responses=redis_cfg["decode_responses"], seed=cfg["seed"], reference_blas=blas,
            keep_vectors=extra.get("keep_vectors"))
        with np.load(src / "projections.npz") as data:
            inst._hasher.projections = [data[f"arr_{i}"].astype(np.float32) for i in range(len(data.files))]
        return inst

    def __getstate__(self) -> Dict[str, Any]:
        """Config + hyperplanes; buffer is flushed, fetch function and storage are not carried
        (reference: main.py:989-1008)."""
        self.flush()
        state = {"config": self._config.copy(), "redis_config": self._redis_config.copy(),
                 "projections": [np.asarray(m, dtype=np.float32) for m in self._hasher.projections]}
        # extras the reference's __setstate__ ignores (it reads the three keys above): what this build needs to come
        # back on the same device with the same windows and ingest mode
        h = self._hasher
        state["lshrs_amd"] = {
            "host_blas": self._blas_record().get("host_blas"),
            "packed_ingest": self._packed_ingest,
            "keep_vectors": self._vectors.dtype if self._vectors is not None else None,
            "device": getattr(h, "_device", None) if isinstance(getattr(h, "_device", None), (int, str, type(None))) else str(h._device),
            "hasher_kwargs": {**{k: getattr(h, k) for k in ("tie_break", "precision", "tie_replay", "margin_guard",
                                                            "tie_threads", "audit_every", "audit_unflagged",
                                                            "reference_blas") if hasattr(h, k)},
                              **({"devices": list(h._devices)} if getattr(h, "_devices", None) else {})},
            "windows": {"tau_ulps": "bound" if getattr(h, "window_mode", {}).get("tau") == "bound" else getattr(h, "tau_ulps", 8.0),
                        "tau1_ulps": "bound" if getattr(h, "window_mode", {}).get("tau1") == "bound" else getattr(h, "tau1_ulps", 64.0)},
        }
        return state

    def __setstate__(self, state: Dict[str, Any]) -> None:
        cfg, rc = state["config"], state["redis_config"]
        extra = state.get("lshrs_amd", {})
        hasher = None
        if extra:
            hk = dict(extra.get("hasher_kwargs", {}))
            hk.pop("pipeline", None)               # (an option of earlier rounds: the interpreter-driven chunking is gone)
            if "reference_blas" in hk:
                hk["reference_blas"] = _hostblas.LEGACY_BUILD_NAMES.get(hk["reference_blas"], hk["reference_blas"])
            _check_recorded_blas(hk.get("reference_blas", "host"), extra.get("host_blas"), cfg["rows_per_band"], cfg["dim"],
                                 type(self).strict_blas)
            hk.update(extra.get("windows", {}))
            hasher = LSHHasher(num_bands=cfg["num_bands"], rows_per_band=cfg["rows_per_band"], dim=cfg["dim"],
                               seed=cfg["seed"], device=extra.get("device"), **hk)
        restored = self.__class__(
            dim=cfg["dim"], num_perm=cfg["num_perm"], num_bands=cfg["num_bands"], rows_per_band=cfg["rows_per_band"],
            similarity_threshold=cfg["similarity_threshold"], buffer_size=cfg["buffer_size"], vector_fetch_fn=None,
            redis_host=rc["host"], redis_port=rc["port"], redis_db=rc["db"], redis_password=rc["password"],
            redis_prefix=rc["prefix"], decode_responses=rc["decode_responses"], seed=cfg["seed"], hasher=hasher,
            packed_ingest=extra.get("packed_ingest", "auto"), storage=_DeferredStorage(rc),
            keep_vectors=extra.get("keep_vectors"))
        self.__dict__ = restored.__dict__
        self._hasher.projections = [np.asarray(m, dtype=np.float32) for m in state["projections"]]

    # ------------------------------------------------------------------ helpers
    strict_blas = False      # True: loading / unpickling a "host" index on a host of the other BLAS build raises (else: warns)

    def _blas_record(self) -> Dict[str, Any]:
        """What persistence writes about the BLAS the keys are the reference's keys on (`_check_recorded_blas` reads it)."""
        blas = getattr(self._hasher, "reference_blas", "host")
        rec: Dict[str, Any] = {"reference_blas": blas}
        if blas == "host":
            try:
                rec["host_blas"] = _hostblas.host_build_name()
            except Exception:           # pragma: no cover - a NumPy without OpenBLAS, the host library not built
                rec["host_blas"] = None
        return rec

    def _check_dim(self, vector) -> np.ndarray:
        """float32, flattened, right length (reference: main.py:1075-1080; the near-zero test of
        :1083 is evaluated by the kernel's row flag, see ``_ZERO_MSG`` call sites)."""
        resident = _device_tensor(vector)
        if resident is not None:       # ONE vector that lives on a GPU: the single-vector calls read theirs from (pinned) host memory
            vector = resident.detach().reshape(-1).cpu().numpy()
        arr = np.asarray(vector, dtype=np.float32).reshape(-1)
        if arr.shape[0] != self._dim:
            raise ValueError(f"Vector must have dimension {self._dim}; received {arr.shape[0]}")
        return arr

    def _hash_one(self, arr: np.ndarray):
        """(keys (bands, B), row flag) of one vector; concurrent callers share a launch where the hasher can coalesce."""
        one = getattr(self._hasher, "hash_one_packed", None)
        if one is not None:
            return one(arr)
        keys, flags = self._hasher.hash_batch_packed(arr.reshape(1, -1), return_row_flags=True)
        return keys[0], int(flags[0])

    def _candidate_counts_from_keys(self, band_keys: np.ndarray) -> Dict[int, int]:
        """Collision count per stored id over the query's band buckets (reference: main.py:1088-1111)."""
        counts: Dict[int, int] = {}
        for band_id in range(band_keys.shape[0]):
            for candidate in self._storage.get_bucket(band_id, band_keys[band_id].tobytes()):
                counts[candidate] = counts.get(candidate, 0) + 1
        return counts

    def _ordered_candidates_arrays(self, keys: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """``_query_host.order_candidates`` of these band keys' buckets (one vectorised lookup where the store has one)."""
        if hasattr(self._storage, "get_buckets_many"):
            q, m = self._storage.get_buckets_many(keys)
        else:
            q, _, m = qh.bucket_pairs(self._storage, keys)
        return qh.order_candidates(q, m, keys.shape[0], keys.shape[1])

    def _ordered_candidates_many(self, keys: np.ndarray) -> List[List[int]]:
        um, bounds = self._ordered_candidates_arrays(keys)
        return qh.split_rows(um.tolist(), np.diff(bounds))

    lane_rows = 262_144      # rows per unit when ONE index() call is cut up for several devices (two stream chunks)

    def _ingest_hashers(self) -> list:
        get = getattr(self._hasher, "device_hashers", None)
        return get() if callable(get) else [self._hasher]

    def _streams_buckets(self, n_ops: int) -> bool:
        """Does a batch of this many operations take the pipelined array path?  The storage must take bucket arrays
        (``batch_add_csr``, natively or through ``RedisPackedWriter``) and the hasher must be able to leave its keys on the
        device (``LSHHasher``; an injected hasher of another kind keeps the one-call path)."""
        sink = self._packed_sink(n_ops)
        return (sink is not None and hasattr(sink, "batch_add_csr")
                and callable(getattr(self._hasher, "device_hashers", None))
                and getattr(self._hasher, "tie_break", "host") == "host")

    def _open_ingest(self, inline: bool = False):
        from ._ingest import CsrIngest

        return CsrIngest(self._ingest_hashers(), self._packed_sink(1 << 62), lambda: ValueError(_ZERO_MSG),
                         lambda: ValueError("index must be non-negative"), inline=inline,
                         on_stored=self._keep if self._vectors is not None else None)

    def _check_rows(self, indices, vectors):
        """The rows of one batch - float32; a torch tensor that lives on a GPU stays where it is - with the reference's shape
        errors (main.py:504-511)."""
        resident = _device_tensor(vectors)
        arr = resident if resident is not None else np.asarray(vectors, dtype=np.float32)
        shape = tuple(int(v) for v in arr.shape)
        if len(shape) != 2 or shape[1] != self._dim:
            raise ValueError(f"Vectors must have shape (n, {self._dim}); received {shape}")
        if shape[0] != len(indices):
            raise ValueError(
                "Number of vectors does not match number of indices "
                f"(received {shape[0]} vectors for {len(indices)} indices)")
        return arr

    @staticmethod
    def _id_array(indices) -> np.ndarray:
        id_arr = np.asarray(indices)
        return id_arr.astype(np.int64) if id_arr.dtype.kind in "iuf" else np.array([int(i) for i in indices], dtype=np.int64)

    def _check_batch(self, indices, vectors):
        """(ids int64, rows float32 C-contiguous) of one batch; rows that live on a GPU stay where they are."""
        arr = self._check_rows(indices, vectors)
        return self._id_array(indices), (arr if _device_tensor(arr) is not None else np.ascontiguousarray(arr))

    def _resolved_storage(self):
        st = self._storage
        return st._resolve() if isinstance(st, _DeferredStorage) else st

    def _packed_sink(self, n_ops: int):
        """The object ``index()`` hands a batch's buckets to as arrays, or None for the reference's operation tuples
        (see ``packed_ingest`` in the class docstring)."""
        mode = self._packed_ingest
        if mode is False or (mode == "auto" and n_ops < self.packed_auto_min_ops):
            return None
        st = self._resolved_storage()            # (index() is about to write to it anyway)
        if hasattr(st, "batch_add_csr") or hasattr(st, "batch_add_packed"):
            return st
        if callable(getattr(st, "pipeline", None)) and callable(getattr(st, "bucket_key", None)):
            # the reference's RedisStorage (lshrs/storage/redis.py:187,508): same SADDs, one command per bucket
            if self._packed_writer is None or self._packed_writer.storage is not st:
                from .packed_ops import RedisPackedWriter

                self._packed_writer = RedisPackedWriter(st, flush_members=self._buffer_size)
            return self._packed_writer
        return None

    def _enqueue_packed(self, index: int, band_keys: np.ndarray) -> None:
        ops = [(b, band_keys[b].tobytes(), index) for b in range(band_keys.shape[0])]
        with self._buffer_lock:
            self._buffer.extend(ops)

    def _flush_buffer_if_needed(self) -> None:
        with self._buffer_lock:
            full = len(self._buffer) >= self._buffer_size
        if full:
            self.flush()

    def _require_vector_fetch_fn(self) -> VectorFetchFn:
        if self._vector_fetch_fn is None:
            raise RuntimeError("vector_fetch_fn must be supplied for operations requiring reranking")
        return self._vector_fetch_fn

    def _resolve_loader(self, format: str) -> Loader:
        """Loader lookup (reference: main.py:1159-1196).  The PostgreSQL / Parquet readers are the
        reference's own modules (I/O is out of scope here) and are imported from that package."""
        normalized = format.lower()
        if normalized in {"batches", "iter", "iterable"}:
            def _from_iterable(batches: Iterable[Tuple[Sequence[int], np.ndarray]]):
                yield from batches
            return _from_iterable
        if normalized in {"postgres", "pg"}:
            from lshrs.io.postgres import iter_postgres_vectors  # reference component
            return iter_postgres_vectors
        if normalized in {"parquet", "pq"}:
            from .parquet_fast import iter_parquet_vectors  # same contract as the reference's, array-based
            return iter_parquet_vectors
        raise ValueError(f"Unsupported signature creation format '{format}'")


lshrs = LSHRS  # lower-case alias kept by the reference (lshrs/core/main.py, last line)
