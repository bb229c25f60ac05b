"""ctypes binding of ``csrc/liblshrs_hip.so`` (the C ABI declared in ``include/lshrs_hip.h``, ``include/lshrs_knn.h`` and
``include/lshrs_join.h``), of ``csrc/liblshrs_groups.so`` (``include/lshrs_groups.h``: a library of its own, loaded by
:func:`load_groups` when the first grouping asks for it) and of ``csrc/liblshrs_graph.so`` (``include/lshrs_graph.h``: a third,
loaded by :func:`load_graph` when the first neighbour graph asks for it) and of ``csrc/liblshrs_refine.so``
(``include/lshrs_refine.h``: a fourth, loaded by :func:`load_refine` when the first refinement asks for it).

There is no CPU implementation behind this module: if the shared library has not
been built, or the ABI version does not match, loading raises — loudly — and so
does every compute entry point of the package.
"""

from __future__ import annotations

import ctypes
import os
import re
import subprocess
import threading
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(_HERE, "csrc")
# one translation unit per kernel family (what they share: csrc/lshrs_common.h); pipeline.hip: the native driver of the host-engine route
UNITS = ("sig_setup", "sig_f32", "sig16", "sig16r", "sig_replay", "sig_small", "sig_split", "storage", "rerank", "query", "idmap", "scan", "pipeline", "join")
SOURCES = tuple(os.path.join(CSRC, u + ".hip") for u in UNITS)
SOURCE = SOURCES[0]
# (LSHRS_HIP_LIBRARY: load another build of the same ABI instead - A/B measurements of compiler flags, tools/ab_build.py)
LIBRARY = os.environ.get("LSHRS_HIP_LIBRARY") or os.path.join(CSRC, "liblshrs_hip.so")
INCLUDE = os.path.join(REPO_ROOT, "include")
HIPCC_FLAGS = ("--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility-inlines-hidden")   # of every unit's compilation
ABI_VERSION = 7
QUERY_MAX_PAIRS = 16384   # LSHRS_QUERY_MAX_PAIRS
SIG_COUNTERS = 8          # LSHRS_SIG_COUNTERS of include/lshrs_hip.h
SIG_DEVICE_COUNTERS = SIG_COUNTERS + 6 * 4096      # LSHRS_SIG_DEVICE_COUNTERS: the device block (counters + stage-2 slots)
SMALL_MAX_ROWS = 256      # LSHRS_SMALL_MAX_ROWS
SORT_MAX_COLS = 1024      # kSortMaxCols of csrc/lshrs_common.h: padded key columns the column-wise stage 2 takes

BUILD_WRONG_KEYS = 0x1   # LSHRS_BUILD_WRONG_KEYS
BUILD_TUNED = 0x2        # LSHRS_BUILD_TUNED

SCAN_ELEMS = ("f32", "bf16", "f16", "i8", "f8e4m3")   # LSHRS_SCAN_F32 .. LSHRS_SCAN_F8E4M3, in that order

REPLAY_ROUTE_STAGE2, REPLAY_ROUTE_TIES, REPLAY_ROUTE_SMALL = 0, 1, 2     # LSHRS_REPLAY_ROUTE_* (lshrs_sig_replay_values_f32)

E_BADARG = -10001
E_TOOLARGE = -10002

# the second library: connected components (csrc/groups.hip, include/lshrs_groups.h) - one unit, no symbol of the first
GROUPS_SOURCE = os.path.join(CSRC, "groups.hip")
GROUPS_LIBRARY = os.path.join(CSRC, "liblshrs_groups.so")
GROUPS_ABI_VERSION = 1       # LSHRS_GROUPS_ABI_VERSION
CC_ERR_ENDPOINT = 0x1        # LSHRS_CC_ERR_ENDPOINT: an endpoint outside [0, n)
CC_ERR_CAP = 0x2             # LSHRS_CC_ERR_CAP: a lane passed an iteration cap

# the third library: neighbour lists out of pairs and their best k (csrc/graph.hip, include/lshrs_graph.h) - one unit, no symbol
# of the other two
GRAPH_SOURCE = os.path.join(CSRC, "graph.hip")
# (LSHRS_GRAPH_LIBRARY: load another build of the same ABI instead - the A/B of -DLSHRS_GRAPH_COMBINE, profiles/lsh_knn.json)
GRAPH_LIBRARY = os.environ.get("LSHRS_GRAPH_LIBRARY") or os.path.join(CSRC, "liblshrs_graph.so")
GRAPH_ABI_VERSION = 1        # LSHRS_GRAPH_ABI_VERSION
GRAPH_ERR_ENDPOINT = 0x1     # LSHRS_GRAPH_ERR_ENDPOINT (degree): an endpoint outside [0, n_rows)
GRAPH_ERR_LOOP = 0x2         # LSHRS_GRAPH_ERR_LOOP (degree): a pair with a == b
GRAPH_ERR_RANGE = 0x1        # LSHRS_GRAPH_ERR_RANGE (select): a list outside [0, total]
GRAPH_ERR_ENTRY = 0x2        # LSHRS_GRAPH_ERR_ENTRY (select): an entry outside [0, n_ids)

# the fourth library: the edges of a neighbour table and the rows within two steps (csrc/refine.hip, include/lshrs_refine.h) -
# one unit, no symbol of the other three
REFINE_SOURCE = os.path.join(CSRC, "refine.hip")
REFINE_LIBRARY = os.path.join(CSRC, "liblshrs_refine.so")
REFINE_ABI_VERSION = 1       # LSHRS_REFINE_ABI_VERSION
REFINE_ERR_OUTSIDE = 0x1     # LSHRS_REFINE_ERR_OUTSIDE (edges): an entry outside [-1, n_rows)
REFINE_ERR_SELF = 0x2        # LSHRS_REFINE_ERR_SELF (edges): a row that lists itself
REFINE_ERR_RANGE = 0x1       # LSHRS_REFINE_ERR_RANGE (count, write): a list outside its array, or too short
REFINE_ERR_ENTRY = 0x2       # LSHRS_REFINE_ERR_ENTRY (count, write): an entry outside [0, n_rows)

_lock = threading.Lock()
_lib: Optional[ctypes.CDLL] = None
_groups_lib: Optional[ctypes.CDLL] = None
_graph_lib: Optional[ctypes.CDLL] = None
_refine_lib: Optional[ctypes.CDLL] = None


class NativeLibraryError(RuntimeError):
    """The HIP extension is missing, stale or reported an error."""


def _sources_of(path: str, seen: Optional[set] = None) -> set:
    """A unit and the project's files it #includes, directly or through one of them: every quoted name that exists under
    csrc/ or include/ (headers and *.inc texts alike - no list to keep)."""
    seen = {path} if seen is None else seen
    with open(path, encoding="utf-8") as fh:
        names = re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', fh.read(), re.M)
    for name in names:
        for folder in (CSRC, INCLUDE):
            dep = os.path.join(folder, name)
            if os.path.exists(dep) and dep not in seen:
                seen.add(dep)
                _sources_of(dep, seen)
    return seen


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 into the in-tree shared library (and the host tie-break engine).
    One object per translation unit (kernels + C ABI, native pipeline driver), rebuilt only when stale."""
    from . import _hostblas

    _hostblas.build(force=force, verbose=verbose)
    with _lock:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        objdir = os.path.join(CSRC, "_obj")
        os.makedirs(objdir, exist_ok=True)
        objects, stale, relink = [], [], force or not os.path.exists(LIBRARY)
        for src in SOURCES:
            obj = os.path.join(objdir, os.path.basename(src) + ".o")
            objects.append(obj)
            if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(p) for p in _sources_of(src)):
                stale.append((src, obj))

        def compile_one(job):
            src, obj = job
            cmd = [hipcc, *HIPCC_FLAGS, "-I" + INCLUDE, "-I" + CSRC, "-c", src, "-o", obj + ".tmp"]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
            os.replace(obj + ".tmp", obj)

        if stale:       # (the units are independent: a few at a time - the two stage-1 kernels take ~7 s each, the rest 1-2 s)
            from concurrent.futures import ThreadPoolExecutor

            with ThreadPoolExecutor(max_workers=min(4, len(stale))) as pool:
                list(pool.map(compile_one, stale))
            relink = True
        if relink or os.path.getmtime(LIBRARY) < max(os.path.getmtime(o) for o in objects):
            cmd = [hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", *objects, "-o", LIBRARY + ".tmp"]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
            os.replace(LIBRARY + ".tmp", LIBRARY)
        # the side libraries, after the first and in their order: each one unit straight into a shared object, by the same
        # rule of staleness
        for side in SIDE_LIBRARIES:
            source, library = side.source(), side.library()
            if force or not os.path.exists(library) or \
                    os.path.getmtime(library) < max(os.path.getmtime(p) for p in _sources_of(source)):
                cmd = [hipcc, *HIPCC_FLAGS, "-I" + INCLUDE, "-I" + CSRC, "-shared", source, "-o", library + ".tmp"]
                if verbose:
                    print(" ".join(cmd))
                subprocess.run(cmd, check=True)
                os.replace(library + ".tmp", library)
        return LIBRARY


def _declare(lib: ctypes.CDLL) -> None:
    c = ctypes
    vp, i32, i64, f32 = c.c_void_p, c.c_int32, c.c_int64, c.c_float
    lib.lshrs_abi_version.argtypes = []
    lib.lshrs_abi_version.restype = c.c_int
    lib.lshrs_build_flags.argtypes = []
    lib.lshrs_build_flags.restype = c.c_uint32
    lib.lshrs_sig_workspace_bytes.argtypes = [i32, i32, i32]
    lib.lshrs_sig_workspace_bytes.restype = i64
    lib.lshrs_sig_padded_columns.argtypes = [i32, i32]
    lib.lshrs_sig_padded_columns.restype = i32
    lib.lshrs_sig_pack_projections.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.lshrs_sig_pack_projections.restype = c.c_int
    # (workspace, bands, rows, dim, coef_a, coef_b, coef_tie, stream)
    lib.lshrs_sig_set_window.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
    lib.lshrs_sig_set_window.restype = c.c_int
    # (X, n, ldx, workspace, bands, rows, dim, keys, tie_list, tie_cap, tie_count, tau, row_flags, opts, stream)
    lib.lshrs_sig_hash_batch_f32.argtypes = [vp, i64, i64, vp, i32, i32, i32, vp, vp, i32, vp, f32, vp, vp, vp]
    lib.lshrs_sig_hash_batch_f32.restype = c.c_int
    # (... row_flags, flag_list, flag_cap, flag_count, tau1, opts, stream)
    lib.lshrs_sig_hash_batch_split_f32.argtypes = [vp, i64, i64, vp, i32, i32, i32, vp, vp, i32, vp, f32, vp, vp, i32, vp,
                                                   f32, vp, vp]
    lib.lshrs_sig_hash_batch_split_f32.restype = c.c_int
    # (X, n, ldx, workspace, bands, rows, dim, keys, counters, tau, row_flags, flag_list, flag_y, flag_cap, tau1,
    #  blas_model, host_counts, audit, opts, stream)
    lib.lshrs_sig_hash_batch_split_replay_f32.argtypes = [vp, i64, i64, vp, i32, i32, i32, vp, vp, f32, vp, vp, vp, i32, f32,
                                                          i32, vp, vp, vp, vp]
    lib.lshrs_sig_hash_batch_split_replay_f32.restype = c.c_int
    # (X, n, ldx, workspace, bands, rows, dim, keys, tie_list, tie_cap, counters, tau, flag_list, flag_cap, blas_model,
    #  host_counts, stream)
    lib.lshrs_sig_resolve_ties_replay_f32.argtypes = [vp, i64, i64, vp, i32, i32, i32, vp, vp, i32, vp, f32, vp, i32, i32, vp,
                                                      vp]
    lib.lshrs_sig_resolve_ties_replay_f32.restype = c.c_int
    # (X, n, ldx, workspace, bands, rows, dim, keys, row_flags, counters, tau, blas_model, host_done, epoch, stream)
    lib.lshrs_sig_hash_small_replay_f32.argtypes = [vp, i64, i64, vp, i32, i32, i32, vp, vp, vp, f32, i32, vp, i32, vp]
    lib.lshrs_sig_hash_small_replay_f32.restype = c.c_int
    lib.lshrs_stream_synchronize.argtypes = [vp]
    lib.lshrs_stream_synchronize.restype = c.c_int
    lib.lshrs_wait_done.argtypes = [vp, i32, i64, vp]
    lib.lshrs_wait_done.restype = c.c_int
    lib.lshrs_sig_project_f32.argtypes = [vp, i64, i64, vp, i32, i32, i32, vp, i64, vp]
    lib.lshrs_sig_project_f32.restype = c.c_int
    # (X, n, ldx, workspace, bands, rows, dim, blas_model, route, keys, values, list, list_cap, sort, counters, stream)
    lib.lshrs_sig_replay_values_f32.argtypes = [vp, i64, i64, vp, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp]
    lib.lshrs_sig_replay_values_f32.restype = c.c_int
    lib.lshrs_gather_rows_f32.argtypes = [vp, i64, i32, vp, i64, vp, vp]
    lib.lshrs_gather_rows_f32.restype = c.c_int
    lib.lshrs_gather_tied_rows_f32.argtypes = [vp, i64, i32, vp, vp, i32, vp, vp]
    lib.lshrs_gather_tied_rows_f32.restype = c.c_int
    lib.lshrs_scatter_band_keys_u8.argtypes = [vp, i32, i32, vp, vp, vp, i64, vp]
    lib.lshrs_scatter_band_keys_u8.restype = c.c_int
    lib.lshrs_keys_to_hex_u8.argtypes = [vp, i64, vp, vp]
    lib.lshrs_keys_to_hex_u8.restype = c.c_int
    lib.lshrs_copy_to_host_u8.argtypes = [vp, vp, i64, vp]
    lib.lshrs_copy_to_host_u8.restype = c.c_int
    lib.lshrs_bucket_histogram_u8.argtypes = [vp, i64, i32, i32, vp, vp]
    lib.lshrs_bucket_histogram_u8.restype = c.c_int
    lib.lshrs_bucket_scatter_u8.argtypes = [vp, vp, i64, i32, i32, vp, vp, vp, vp]
    lib.lshrs_bucket_scatter_u8.restype = c.c_int
    lib.lshrs_cosine_batch_f32.argtypes = [vp, i64, i64, i32, vp, i32, vp, i32, vp, vp, vp, vp]
    lib.lshrs_cosine_batch_f32.restype = c.c_int
    lib.lshrs_l2_normalize_f32.argtypes = [vp, i64, i64, i32, vp, vp, vp]
    lib.lshrs_l2_normalize_f32.restype = c.c_int
    lib.lshrs_topk_workspace_bytes.argtypes = [i32, i32]
    lib.lshrs_topk_workspace_bytes.restype = i64
    lib.lshrs_topk_desc_f32.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
    lib.lshrs_topk_desc_f32.restype = c.c_int
    f64 = c.c_double
    # (keys, q, bands, band_bytes, segments, nseg, slot_start, slot_len, slot_off, pair_count, stream)
    lib.lshrs_query_lookup_u8.argtypes = [vp, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp]
    lib.lshrs_query_lookup_u8.restype = c.c_int
    # (counts, q, top_k, top_p, keep_out, offsets, totals, stream)
    lib.lshrs_query_scan_i32.argtypes = [vp, i32, i32, f64, vp, vp, vp, vp]
    lib.lshrs_query_scan_i32.restype = c.c_int
    # (segments, nseg, bands, slot_start, slot_len, slot_off, pair_off, q, max_pairs, cand_ids, cand_hits, ucount, stream)
    lib.lshrs_query_collide_index_i64.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
    lib.lshrs_query_collide_index_i64.restype = c.c_int
    # (members, bands, pair_off, q, max_pairs, num_bands, cand_ids, cand_hits, ucount, stream)
    lib.lshrs_query_collide_pairs_i64.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]
    lib.lshrs_query_collide_pairs_i64.restype = c.c_int
    lib.lshrs_query_big_workspace_bytes.argtypes = [i64]
    lib.lshrs_query_big_workspace_bytes.restype = i64
    # (segments, nseg, bands, slot_start, slot_off, pairs, workspace, cand_ids, cand_hits, ucount, stream)
    lib.lshrs_query_collide_big_i64.argtypes = [vp, i32, i32, vp, vp, i64, vp, vp, vp, vp, vp]
    lib.lshrs_query_collide_big_i64.restype = c.c_int
    # (keys, bands, band_bytes, segments, nseg, slot_start, slot_len, slot_off, max_pairs, top_k, top_p, rerank_follows, pair_off,
    #  cand_ids, ucount, keep, out_off, out_ids, done_host, epoch, copy_src, copy_dst, copy_n, stream)
    lib.lshrs_query_one_u8.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, i32, i32, f64, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, vp]
    lib.lshrs_query_one_u8.restype = c.c_int
    # (corpus, m, ldc, dim, queries, q, cand_rows, row_off, row_cnt, total, scores, err, stream)
    lib.lshrs_cosine_ragged_f32.argtypes = [vp, i64, i64, i32, vp, i32, vp, vp, vp, i64, vp, vp, vp]
    lib.lshrs_cosine_ragged_f32.restype = c.c_int
    # the same two forms on a corpus of 16- or 8-bit elements (ldc in elements): bf16 / f16 / int8 / e4m3fn converted exactly
    # to f32
    for dt in ("bf16", "f16", "i8", "f8e4m3"):
        batch, ragged = getattr(lib, "lshrs_cosine_batch_" + dt), getattr(lib, "lshrs_cosine_ragged_" + dt)
        batch.argtypes, batch.restype = lib.lshrs_cosine_batch_f32.argtypes, c.c_int
        ragged.argtypes, ragged.restype = lib.lshrs_cosine_ragged_f32.argtypes, c.c_int
    # (X, n, ldx, dim, out, ldo, status, stream): f32 rows to 8-bit codes, a scale of their own per row
    for dt in ("i8", "f8e4m3"):
        quant = getattr(lib, "lshrs_quantize_rows_" + dt)
        quant.argtypes, quant.restype = [vp, i64, i64, i32, vp, i64, vp, vp], c.c_int
    # (cand_ids, scores, pair_off, ucount, keep, out_off, q, max_candidates, out_ids, out_scores, done_host, epoch, stream)
    lib.lshrs_query_rank_f32.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp]
    lib.lshrs_query_rank_f32.restype = c.c_int
    # the id -> row table of a device-resident vector store (csrc/idmap.hip)
    lib.lshrs_idmap_bytes.argtypes = [i64]
    lib.lshrs_idmap_bytes.restype = i64
    lib.lshrs_idmap_home_slot.argtypes = [i64, i64]
    lib.lshrs_idmap_home_slot.restype = i64
    # (table, slots, ids, n, first_row, report, stream)
    lib.lshrs_idmap_insert_i64.argtypes = [vp, i64, vp, i64, i64, vp, vp]
    lib.lshrs_idmap_insert_i64.restype = c.c_int
    # (table, slots, ids, n, live_count, stream)
    lib.lshrs_idmap_erase_i64.argtypes = [vp, i64, vp, i64, vp, vp]
    lib.lshrs_idmap_erase_i64.restype = c.c_int
    # (table, slots, ids, n, rows, err, stream)
    lib.lshrs_idmap_lookup_i64.argtypes = [vp, i64, vp, i64, vp, vp, vp]
    lib.lshrs_idmap_lookup_i64.restype = c.c_int
    # (table, slots, cand_ids, pair_off, ucount, q, total, rows, err, stream)
    lib.lshrs_idmap_lookup_ragged_i64.argtypes = [vp, i64, vp, vp, vp, i32, i64, vp, vp, vp]
    lib.lshrs_idmap_lookup_ragged_i64.restype = c.c_int
    # (src, src_slots, dst, dst_slots, report, stream)
    lib.lshrs_idmap_rehash.argtypes = [vp, i64, vp, i64, vp, vp]
    lib.lshrs_idmap_rehash.restype = c.c_int
    # the exhaustive scan of a row block on the matrix cores (csrc/scan.hip)
    lib.lshrs_scan_workspace_bytes.argtypes = [i32, i64, i32, i32]
    lib.lshrs_scan_workspace_bytes.restype = i64
    lib.lshrs_scan_max_window.argtypes = []
    lib.lshrs_scan_max_window.restype = i32
    lib.lshrs_scan_epsilon.argtypes = [i32, i32]
    lib.lshrs_scan_epsilon.restype = f64
    # (corpus, m, ldc, dim, row_ids, queries, q, window, out_rows, out_approx, out_count, workspace, err, stream)
    for dt in SCAN_ELEMS:
        scan = getattr(lib, "lshrs_scan_topk_" + dt)
        scan.argtypes, scan.restype = [vp, i64, i64, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp], c.c_int
    lib.lshrs_scan_above_workspace_bytes.argtypes = [i32, i64, i32]
    lib.lshrs_scan_above_workspace_bytes.restype = i64
    # (corpus, m, ldc, dim, row_ids, queries, q, bars, capacity, out_query, out_row, out_approx, total, workspace, err, stream)
    for dt in SCAN_ELEMS:
        above = getattr(lib, "lshrs_scan_above_" + dt)
        above.argtypes, above.restype = [vp, i64, i64, i32, vp, vp, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp], c.c_int
    lib.lshrs_scan_pairs_workspace_bytes.argtypes = [i64, i32, i32]
    lib.lshrs_scan_pairs_workspace_bytes.restype = i64
    # (corpus, m, ldc, dim, row_ids, bar, qblock, capacity, out_a, out_b, out_approx, total, workspace, err, stream)
    for dt in SCAN_ELEMS:
        pairs = getattr(lib, "lshrs_scan_pairs_" + dt)
        pairs.argtypes, pairs.restype = [vp, i64, i64, i32, vp, f32, i32, i64, vp, vp, vp, vp, vp, vp, vp], c.c_int
    # the k-NN self-join (include/lshrs_knn.h): (q_count, m, dim, window, qblock)
    lib.lshrs_scan_knn_workspace_bytes.argtypes = [i32, i64, i32, i32, i32]
    lib.lshrs_scan_knn_workspace_bytes.restype = i64
    # (corpus, m, ldc, dim, row_ids, q_begin, q_count, window, qblock, out_rows, out_approx, out_count, workspace, err, stream)
    for dt in SCAN_ELEMS:
        knn = getattr(lib, "lshrs_scan_knn_" + dt)
        knn.argtypes, knn.restype = [vp, i64, i64, i32, vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp], c.c_int
    # the LSH self-join (include/lshrs_join.h): (n_rows, num_bands)
    lib.lshrs_join_workspace_bytes.argtypes = [i64, i32]
    lib.lshrs_join_workspace_bytes.restype = i64
    # (codes, offsets, n_codes, band_bytes, num_bands, member_rows, n_members, n_rows, max_bucket, workspace, err, stream)
    lib.lshrs_join_rowmap_i64.argtypes = [vp, vp, i64, i32, i32, vp, i64, i64, i64, vp, vp, vp]
    lib.lshrs_join_rowmap_i64.restype = c.c_int
    # (offsets, pair_prefix, n_codes, member_rows, n_rows, num_bands, workspace, raw_begin, raw_count, min_collisions, capacity,
    #  out_a, out_b, out_hits, total, stream)
    lib.lshrs_join_emit_i64.argtypes = [vp, vp, i64, vp, i64, i32, vp, i64, i64, i32, i64, vp, vp, vp, vp, vp]
    lib.lshrs_join_emit_i64.restype = c.c_int
    lib.lshrs_pipe_create.argtypes = [i32, i32, i32, i32, i32]
    lib.lshrs_pipe_create.restype = vp
    lib.lshrs_pipe_destroy.argtypes = [vp]
    lib.lshrs_pipe_destroy.restype = None
    lib.lshrs_pipe_hash_f32.argtypes = [vp, vp, i64, vp, vp, vp, f32, f32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.lshrs_pipe_hash_f32.restype = c.c_int


EXPORTS = (
    "lshrs_abi_version",
    "lshrs_build_flags",
    "lshrs_sig_workspace_bytes",
    "lshrs_sig_padded_columns",
    "lshrs_sig_pack_projections",
    "lshrs_sig_set_window",
    "lshrs_sig_hash_batch_f32",
    "lshrs_sig_hash_batch_split_f32",
    "lshrs_sig_hash_batch_split_replay_f32",
    "lshrs_sig_resolve_ties_replay_f32",
    "lshrs_sig_hash_small_replay_f32",
    "lshrs_stream_synchronize",
    "lshrs_wait_done",
    "lshrs_sig_project_f32",
    "lshrs_sig_replay_values_f32",
    "lshrs_gather_rows_f32",
    "lshrs_gather_tied_rows_f32",
    "lshrs_scatter_band_keys_u8",
    "lshrs_keys_to_hex_u8",
    "lshrs_copy_to_host_u8",
    "lshrs_bucket_histogram_u8",
    "lshrs_bucket_scatter_u8",
    "lshrs_cosine_batch_f32",
    "lshrs_l2_normalize_f32",
    "lshrs_topk_workspace_bytes",
    "lshrs_topk_desc_f32",
    "lshrs_query_lookup_u8",
    "lshrs_query_scan_i32",
    "lshrs_query_collide_index_i64",
    "lshrs_query_collide_pairs_i64",
    "lshrs_query_big_workspace_bytes",
    "lshrs_query_collide_big_i64",
    "lshrs_query_one_u8",
    "lshrs_cosine_ragged_f32",
    "lshrs_cosine_batch_bf16",
    "lshrs_cosine_batch_f16",
    "lshrs_cosine_ragged_bf16",
    "lshrs_cosine_ragged_f16",
    "lshrs_cosine_batch_i8",
    "lshrs_cosine_batch_f8e4m3",
    "lshrs_cosine_ragged_i8",
    "lshrs_cosine_ragged_f8e4m3",
    "lshrs_quantize_rows_i8",
    "lshrs_quantize_rows_f8e4m3",
    "lshrs_query_rank_f32",
    "lshrs_idmap_bytes",
    "lshrs_idmap_home_slot",
    "lshrs_idmap_insert_i64",
    "lshrs_idmap_erase_i64",
    "lshrs_idmap_lookup_i64",
    "lshrs_idmap_lookup_ragged_i64",
    "lshrs_idmap_rehash",
    "lshrs_scan_workspace_bytes",
    "lshrs_scan_max_window",
    "lshrs_scan_epsilon",
    "lshrs_scan_topk_f32",
    "lshrs_scan_topk_bf16",
    "lshrs_scan_topk_f16",
    "lshrs_scan_topk_i8",
    "lshrs_scan_topk_f8e4m3",
    "lshrs_scan_above_workspace_bytes",
    "lshrs_scan_above_f32",
    "lshrs_scan_above_bf16",
    "lshrs_scan_above_f16",
    "lshrs_scan_above_i8",
    "lshrs_scan_above_f8e4m3",
    "lshrs_scan_pairs_workspace_bytes",
    "lshrs_scan_pairs_f32",
    "lshrs_scan_pairs_bf16",
    "lshrs_scan_pairs_f16",
    "lshrs_scan_pairs_i8",
    "lshrs_scan_pairs_f8e4m3",
    "lshrs_pipe_create",
    "lshrs_pipe_destroy",
    "lshrs_pipe_hash_f32",
)
# ... and what include/lshrs_knn.h declares beside them (additive to ABI 7)
EXPORTS_KNN = (
    "lshrs_scan_knn_workspace_bytes",
    "lshrs_scan_knn_f32",
    "lshrs_scan_knn_bf16",
    "lshrs_scan_knn_f16",
    "lshrs_scan_knn_i8",
    "lshrs_scan_knn_f8e4m3",
)
# ... and include/lshrs_join.h (additive to ABI 7 as well)
EXPORTS_JOIN = (
    "lshrs_join_workspace_bytes",
    "lshrs_join_rowmap_i64",
    "lshrs_join_emit_i64",
)


def load() -> ctypes.CDLL:
    """Load the library (once).  Raises NativeLibraryError when it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIBRARY):
            raise NativeLibraryError(
                f"{LIBRARY} is missing: the HIP extension has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'`). "
                "lshrs_amd has no CPU fallback."
            )
        # torch ships its own libamdhip64 (same SONAME); importing it first makes our
        # NEEDED entry resolve to the runtime torch allocates with.
        import torch  # noqa: F401

        try:
            lib = ctypes.CDLL(LIBRARY)
        except OSError as exc:  # pragma: no cover - environment specific
            raise NativeLibraryError(f"cannot load {LIBRARY}: {exc}") from exc
        for name in EXPORTS + EXPORTS_KNN + EXPORTS_JOIN:
            if not hasattr(lib, name):
                raise NativeLibraryError(f"{LIBRARY} does not export {name}; rebuild it")
        _declare(lib)
        got = lib.lshrs_abi_version()
        if got != ABI_VERSION:
            raise NativeLibraryError(f"{LIBRARY} has ABI version {got}, expected {ABI_VERSION}; rebuild it")
        flags = int(lib.lshrs_build_flags())
        if flags & BUILD_WRONG_KEYS and os.environ.get("LSHRS_ALLOW_AB") != "1":
            # an A/B build that drops work the keys need (tools/ab_build.py -DLSHRS_AB_...): indistinguishable from the
            # product by ABI number, so it says what it is and is refused here
            raise NativeLibraryError(
                f"{LIBRARY} is a measurement build whose keys are wrong by design (lshrs_build_flags() = {flags:#x}); "
                "set LSHRS_ALLOW_AB=1 to load it for an A/B run, or unset LSHRS_HIP_LIBRARY")
        _lib = lib
        return lib


class _SideLibrary:
    """One of the libraries beside the first - one unit, no symbol of another: what it is built from, what it exports and how
    it is loaded.  Its source, its path, its ABI number and the loaded library are the module's own ``<NAME>_SOURCE``,
    ``<NAME>_LIBRARY``, ``<NAME>_ABI_VERSION`` and ``_<name>_lib``, read when they are used."""

    def __init__(self, name: str, abi: str, entries: dict):
        self.name, self.abi, self.entries = name, abi, entries      # entries: export -> (argtypes, restype), all of them

    def source(self) -> str:
        return globals()[self.name.upper() + "_SOURCE"]

    def library(self) -> str:
        return globals()[self.name.upper() + "_LIBRARY"]

    def load(self) -> ctypes.CDLL:
        """Load the library (once).  Raises NativeLibraryError when it is not there."""
        slot = "_" + self.name + "_lib"
        if globals()[slot] is not None:
            return globals()[slot]
        with _lock:
            if globals()[slot] is not None:
                return globals()[slot]
            path, version = self.library(), globals()[self.name.upper() + "_ABI_VERSION"]
            if not os.path.exists(path):
                raise NativeLibraryError(
                    f"{path} is missing: the HIP extension has not been built "
                    "(run `python -c 'import __graft_entry__ as g; g.build()'`). "
                    "lshrs_amd has no CPU fallback."
                )
            import torch  # noqa: F401  (its libamdhip64 first, as in load())

            try:
                lib = ctypes.CDLL(path)
            except OSError as exc:  # pragma: no cover - environment specific
                raise NativeLibraryError(f"cannot load {path}: {exc}") from exc
            for name in self.entries:
                if not hasattr(lib, name):
                    raise NativeLibraryError(f"{path} does not export {name}; rebuild it")
            for name, (argtypes, restype) in self.entries.items():
                getattr(lib, name).argtypes, getattr(lib, name).restype = argtypes, restype
            got = getattr(lib, self.abi)()
            if got != version:
                raise NativeLibraryError(f"{path} has ABI version {got}, expected {version}; rebuild it")
            globals()[slot] = lib
            return lib


_vp, _i32, _i64, _int = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int
# what include/lshrs_groups.h declares: the exports of liblshrs_groups.so, all of them
_GROUPS = _SideLibrary("groups", "lshrs_groups_abi_version", {
    "lshrs_groups_abi_version": ([], _int),
    "lshrs_cc_init_i32": ([_vp, _i64, _vp], _int),                               # (parent, n, stream)
    "lshrs_cc_hook_i64": ([_vp, _vp, _i64, _vp, _i64, _vp, _vp], _int),          # (a, b, n_edges, parent, n, err, stream)
    "lshrs_cc_flatten_i32": ([_vp, _i64, _vp, _vp], _int),                       # (parent, n, err, stream)
})
# what include/lshrs_graph.h declares: the exports of liblshrs_graph.so, all of them
_GRAPH = _SideLibrary("graph", "lshrs_graph_abi_version", {
    "lshrs_graph_abi_version": ([], _int),
    "lshrs_graph_max_list": ([], _i32),
    "lshrs_graph_wave_list": ([], _i32),
    "lshrs_graph_degree_i64": ([_vp, _vp, _i64, _i64, _vp, _vp, _vp], _int),     # (a, b, n_pairs, n_rows, degree, err, stream)
    # (a, b, n_pairs, n_rows, row_off, cursor, nbr, stream)
    "lshrs_graph_fill_i64": ([_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp], _int),
    # (nbr, scores, row_off, n_rows, total, row_ids, n_ids, k, out_ids, out_scores, out_count, err, stream)
    "lshrs_graph_select_f32": ([_vp, _vp, _vp, _i64, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp], _int),
})
# what include/lshrs_refine.h declares: the exports of liblshrs_refine.so, all of them
_REFINE = _SideLibrary("refine", "lshrs_refine_abi_version", {
    "lshrs_refine_abi_version": ([], _int),
    "lshrs_refine_wave_set": ([], _i32),
    "lshrs_refine_max_set": ([], _i32),
    "lshrs_refine_edges_i64": ([_vp, _i64, _i32, _vp, _vp, _vp], _int),          # (graph, n_rows, k_in, keep, err, stream)
    # (nbr, row_off, n_rows, total, max_degree, cand_count, err, stream)
    "lshrs_refine_expand_count_i64": ([_vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp], _int),
    # (nbr, row_off, n_rows, total, max_degree, cand_off, cand, cand_total, err, stream)
    "lshrs_refine_expand_write_i64": ([_vp, _vp, _i64, _i64, _i32, _vp, _vp, _i64, _vp, _vp], _int),
})
SIDE_LIBRARIES = (_GROUPS, _GRAPH, _REFINE)                # in the order build() makes them
EXPORTS_GROUPS, EXPORTS_GRAPH, EXPORTS_REFINE = tuple(_GROUPS.entries), tuple(_GRAPH.entries), tuple(_REFINE.entries)


def load_groups() -> ctypes.CDLL:
    """Load the library of the connected components (once).  Raises NativeLibraryError when it is not there; :func:`load`
    neither loads it nor needs it."""
    return _GROUPS.load()


def load_graph() -> ctypes.CDLL:
    """Load the library of the neighbour lists (once).  Raises NativeLibraryError when it is not there; :func:`load` and
    :func:`load_groups` neither load it nor need it."""
    return _GRAPH.load()


def load_refine() -> ctypes.CDLL:
    """Load the library of the graph refinement (once).  Raises NativeLibraryError when it is not there; :func:`load`,
    :func:`load_groups` and :func:`load_graph` neither load it nor need it."""
    return _REFINE.load()


class SigOpts(ctypes.Structure):
    """``lshrs_sig_opts`` of include/lshrs_hip.h: optional per-call measurement hooks (events, clock probe)."""

    _fields_ = [("struct_bytes", ctypes.c_uint32), ("done_epoch", ctypes.c_int32),
                ("ev_stage1_start", ctypes.c_void_p), ("ev_stage1_stop", ctypes.c_void_p),
                ("ev_stage2_start", ctypes.c_void_p), ("ev_stage2_stop", ctypes.c_void_p),
                ("clock_probe", ctypes.c_void_p), ("sort", ctypes.c_void_p), ("done_host", ctypes.c_void_p)]

    def __init__(self, events=None, clock_probe=None, sort=None):
        super().__init__()
        self._sort_ref = None
        self.struct_bytes = ctypes.sizeof(SigOpts)
        if events is not None:
            (self.ev_stage1_start, self.ev_stage1_stop, self.ev_stage2_start, self.ev_stage2_stop) = events
        if clock_probe is not None:
            self.clock_probe = clock_probe
        self.set_sort(sort)

    def set_sort(self, sort) -> None:
        """Attach (or detach) the scratch of the column-sorted stage 2; the SigSort object must outlive the call it is passed to."""
        self._sort_ref = sort
        self.sort = ctypes.addressof(sort) if sort is not None else None


class SigSort(ctypes.Structure):
    """``lshrs_sig_sort`` of include/lshrs_hip.h: scratch for the column-sorted stage 2."""

    _fields_ = [("struct_bytes", ctypes.c_uint32), ("cap", ctypes.c_int32), ("list", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("hist", ctypes.c_void_p), ("thr", ctypes.c_void_p), ("mode", ctypes.c_int32), ("parity", ctypes.c_int32)]

    def __init__(self, list_ptr: int, y_ptr: int, hist_ptr: int, cap: int, thr_ptr=None, mode: int = 1):
        super().__init__()
        self.struct_bytes = ctypes.sizeof(SigSort)
        self.list, self.y, self.hist, self.cap = list_ptr, y_ptr, hist_ptr, int(cap)
        self.thr, self.mode, self.parity = thr_ptr, int(mode), 0


class SigAudit(ctypes.Structure):
    """``lshrs_sig_audit`` of include/lshrs_hip.h: where a launch leaves its sample of the projections stage 1 decided on
    its own, for stage 2 to verify against the replayed host-BLAS value."""

    _fields_ = [("struct_bytes", ctypes.c_uint32), ("seed", ctypes.c_uint32), ("list", ctypes.c_void_p),
                ("vals", ctypes.c_void_p), ("slots", ctypes.c_int32), ("target", ctypes.c_int32)]

    def __init__(self, list_ptr: int, vals_ptr: int, slots: int, target: int, seed: int = 0):
        super().__init__()
        self.struct_bytes = ctypes.sizeof(SigAudit)
        self.list, self.vals, self.slots, self.target, self.seed = list_ptr, vals_ptr, int(slots), int(target), int(seed) & 0xFFFFFFFF


def check(code: int, what: str) -> None:
    """Turn a C-ABI status into an exception."""
    if code == 0:
        return
    if code == E_BADARG:
        raise NativeLibraryError(f"{what}: bad argument (LSHRS_E_BADARG)")
    if code == E_TOOLARGE:
        raise NativeLibraryError(f"{what}: shape outside kernel limits (LSHRS_E_TOOLARGE)")
    raise NativeLibraryError(f"{what}: HIP error {-code}")


_torch_ok = None


def require_gpu():
    """Return the torch module after checking a GPU is usable; raise loudly otherwise."""
    global _torch_ok
    if _torch_ok is not None:          # (checked once per process: this sits on the per-call path of the hasher)
        return _torch_ok
    import torch

    if not torch.cuda.is_available():
        raise NativeLibraryError(
            "no MI355X/ROCm device is visible to PyTorch; lshrs_amd computes only on the GPU "
            "(there is no CPU fallback)."
        )
    _torch_ok = torch
    return torch
