"""Wall-clock check of the near-duplicate groups, NOT part of `-m gpu` (a slow or shared box must not turn parity red):
group_pairs on device tensors against the route it replaces - the same pairs copied to the host, made dense by np.unique,
scipy.sparse.csgraph.connected_components, and the same (members, offsets) assembled in NumPy.  Both give equal arrays.

  pairs    the pairs of exact_pairs_above(0.75) over the planted corpus of tests/test_perf_exact_pairs.py (200 000 x 768 bf16
           rows, about 110 000 pairs);
  random   2^24 random edges over 2^23 vertices.

A host clock around each whole call, which ends in a device synchronise; the device route is called once to warm up and then
REPEATS times (the least and the median are recorded, the least is compared), the host route twice.  The parts of the device
route on their own: torch.unique (_groups._dense), the three kernels (_groups._labels) and the sort that lays the groups out
(_groups._layout).  And on the first workload LSHRS.groups_above against LSHRS.pairs_above, both with return_arrays, over the
index of tests/test_perf_lsh_join.py (16 bands x 16 rows).

Measured on an MI355X (profiles/groups.json).  random: 11.3 ms on the device (median of five 13.6) against 4 379 ms on the
host, 388x; of the device route torch.unique takes 3.8 ms, the three kernels with the read-back of the error bits 7.4 ms, the
layout 0.5 ms; 8.23 M ids grouped, one group of 8.22 M and 6 180 small ones.  pairs: 110 000 pairs, 22 000 ids in 2 000 groups
of 11 - 0.44 ms against 6.9 ms, 15.7x; torch.unique 0.20 ms, kernels 0.10 ms, layout 0.14 ms: at this size the device route
is launch and synchronisation latency, and torch.unique is the largest part of it.  LSHRS.groups_above 6.75 ms against
LSHRS.pairs_above 6.47 ms (1.04x): 101 279 pairs kept, 21 979 ids in 2 000 groups, 0.999 of the exact grouping's removable ids.
Floor: on the 2^24-edge workload host / device >= three quarters of the measured ratio, the margin the other perf tests keep
against a shared box.  The small workload's ratio is recorded, not asserted.
LSHRS_PROFILE_OUT=<path>: the figures as JSON (profiles/groups.json is one such run)."""

from __future__ import annotations

import json
import os
import time

import numpy as np
import pytest

from tests.test_perf_exact_pairs import _corpus

# host / device of the whole call on the 2^24-edge workload, measured on an MI355X (profiles/groups.json): 4 379 / 11.29 ms
MEASURED_RATIO = 387.9
REPEATS = 5
BANDS, ROWS = 16, 16


def _host_route(a, b):
    """What a caller did before: the pairs to the host, dense numbers, SciPy's components, the groups in the package's order."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    a, b = a.cpu().numpy(), b.cpu().numpy()
    if a.shape[0] == 0:
        return np.empty(0, np.int64), np.zeros(1, np.int64)
    ids, inverse = np.unique(np.concatenate((a, b)), return_inverse=True)
    v, p = ids.shape[0], a.shape[0]
    graph = coo_matrix((np.ones(p, np.int8), (inverse[:p], inverse[p:])), shape=(v, v))
    _, labels = connected_components(graph, directed=False)
    _, first = np.unique(labels, return_index=True)         # the smallest dense vertex of every component
    smallest = first[labels]
    order = np.argsort(smallest, kind="stable")
    sizes = np.bincount(smallest, minlength=v)
    offsets = np.zeros(first.shape[0] + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(sizes[sizes > 0])
    return ids[order], offsets


def _clocked(torch, fn, repeats):
    """fn() `repeats` times, a host clock around each call and a synchronise at both ends: (times in ms, the last result)."""
    times, out = [], None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times, out


def _measure(torch, a, b):
    from lshrs_amd import _groups, _native, group_pairs

    lib = _native.load_groups()
    group_pairs(a, b, return_tensors=True)                                      # warm-up
    dev_ms, got = _clocked(torch, lambda: group_pairs(a, b, return_tensors=True), REPEATS)
    host_ms, want = _clocked(torch, lambda: _host_route(a, b), 2)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    # the parts of the device route
    _groups._dense(torch, a, b)
    unique_ms, (ids, da, db) = _clocked(torch, lambda: _groups._dense(torch, a, b), REPEATS)
    v = int(ids.shape[0])
    _groups._labels(torch, lib, da, db, v, a.device)
    kernels_ms, (labels, bits) = _clocked(torch, lambda: _groups._labels(torch, lib, da, db, v, a.device), REPEATS)
    assert bits == 0
    _groups._layout(torch, ids, labels)
    layout_ms, _ = _clocked(torch, lambda: _groups._layout(torch, ids, labels), REPEATS)
    sizes = np.diff(want[1])
    return {"pairs": int(a.shape[0]), "grouped": v, "groups": int(sizes.shape[0]), "largest": int(sizes.max()) if sizes.size else 0,
            "device_ms": min(dev_ms), "device_median_ms": float(np.median(dev_ms)), "host_ms": min(host_ms),
            "ratio": min(host_ms) / min(dev_ms), "unique_ms": min(unique_ms), "kernels_ms": min(kernels_ms),
            "layout_ms": min(layout_ms)}


@pytest.mark.perf
def test_perf_groups_on_the_device_beat_the_host_route():
    import torch

    from lshrs_amd import LSHRS, InMemoryStorage, _native, exact_pairs_above

    assert torch.cuda.is_available(), "perf tests need a visible MI355X"
    _native.load_groups()                                   # (missing: the test fails here, before it builds its corpus)
    m, dim, t = 200_000, 768, 0.75
    record = {"shape": {"rows": m, "dim": dim, "threshold": t, "random_edges": 1 << 24, "random_vertices": 1 << 23,
                        "num_bands": BANDS, "rows_per_band": ROWS, "repeats": REPEATS}}
    corpus = _corpus(torch, m, dim, torch.bfloat16)
    pa, pb, _ = exact_pairs_above(corpus, t, return_tensors=True)
    assert pa.shape[0] >= m // 100 * 10
    record["pairs"] = _measure(torch, pa, pb)
    # the whole calls of the index on that workload: the groups out of the buckets against the pairs out of the buckets
    rows32 = corpus.float()
    index = LSHRS(dim=dim, num_perm=BANDS * ROWS, num_bands=BANDS, rows_per_band=ROWS,
                  storage=InMemoryStorage(record_batches=False), packed_ingest=True)
    for lo in range(0, m, m // 4):
        index.index(np.arange(lo, lo + m // 4, dtype=np.int64), rows32[lo:lo + m // 4])
    index.set_corpus(corpus)
    index.pairs_above(t, return_arrays=True)                # (the first call folds the four segments: its cost, once)
    index.groups_above(t, return_arrays=True)
    pairs_ms, found = _clocked(torch, lambda: index.pairs_above(t, return_arrays=True), REPEATS)
    groups_ms, got = _clocked(torch, lambda: index.groups_above(t, return_arrays=True), REPEATS)
    stats = dict(index.last_search_stats)
    want = _host_route(torch.from_numpy(found[0]), torch.from_numpy(found[1]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    record["index"] = {"pairs_above_ms": min(pairs_ms), "groups_above_ms": min(groups_ms),
                       "groups_over_pairs": min(groups_ms) / min(pairs_ms), "kept": stats["kept"], "groups": stats["groups"],
                       "grouped": stats["grouped"], "largest": stats["largest"], "recall": index.recall_groups_above(t)["recall"]}
    del corpus, rows32, index, pa, pb
    torch.cuda.empty_cache()
    gen = torch.Generator("cuda").manual_seed(11)
    a = torch.randint(0, 1 << 23, (1 << 24,), device="cuda", generator=gen)
    b = torch.randint(0, 1 << 23, (1 << 24,), device="cuda", generator=gen)
    record["random"] = _measure(torch, a, b)
    record["random"]["floor"] = None if MEASURED_RATIO is None else 0.75 * MEASURED_RATIO
    print(json.dumps(record))
    out = os.environ.get("LSHRS_PROFILE_OUT")
    if out:
        with open(out, "w") as fh:
            json.dump(record, fh, indent=1)
            fh.write("\n")
    assert MEASURED_RATIO is not None, "no measured ratio recorded: the floor cannot be set"
    assert record["random"]["ratio"] >= 0.75 * MEASURED_RATIO, record
