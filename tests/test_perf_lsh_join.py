"""Wall-clock check of the LSH self-join, NOT part of `-m gpu` (a slow or shared box must not turn parity red): the planted
corpus of tests/test_perf_exact_pairs.py (200 000 x 768 rows, about ten partners above a cosine of 0.75 for 1 % of them), indexed
with 16 bands x 16 rows (2-byte band keys) in four index() calls, the rows attached as a bf16 and then as an f32 tensor.  Timed,
each once after a warm-up of the same call, events around the whole call:

  join     LSHRS.pairs_above(0.75, return_arrays=True) - the buckets' candidate pairs, each reranked once;
  detour   what there was before it: every stored row back through query_many(rows, top_k=None, top_p=1.0, return_arrays=True)
           in chunks of 10 000 rows - hashed again, collided per query, every pair reranked twice - cut to score >= t and
           asking id < id;
  exact    LSHRS.pairs_exact_above(0.75): the exhaustive self-join, the truth.

and the join's three parts on their own: the row map with its plumbing (_join._plan), the emit (_join._emit) and the rerank of
what was emitted (_exact._judge_pairs).  The answer that was timed must equal the detour's pairs and scores, and the exact
join's pairs restricted to them, bit for bit.

Measured on an MI355X (profiles/lsh_pairs.json): bf16 rows 6.45 ms against 29.9 ms for the detour, 4.64x, and 104.8 ms for the
exact join, 16.2x; f32 rows 6.91 against 28.5 ms, 4.13x, and 240.6 ms, 34.8x.  Row map 0.29 ms, one emit 1.08 ms (it runs twice:
5.3 M candidates pass the first launch's 2^20 slots), rerank and order 3.6 / 3.9 ms: the emit costs less than the rerank of what
it emits.  5.59 M raw pairs, 5.30 M candidates, 101 279 kept of 110 000: recall 0.921 (expected 0.922).  The fold of the four
segments on the host: 555 ms, once, in the warm-up call.  The join took 6.5 .. 6.9 ms in each of four runs; the detour's
single timed call took 28.0 .. 29.9 ms in six of the eight timings and 44.3 and 53.8 ms in two (single ratios from 4.1 to 7.8): the
recorded run is one of the plain ones.  (That run was made while MEASURED_RATIO still held the first run's ratios, 6.719 and
4.323 - the first of them from an outlier of the detour - so its own floor check failed for bf16, 4.64 against 5.04; the
constants were then set to this run's ratios: the profile's "note" says the same.)
Floor: join <= detour / FLOOR per dtype, FLOOR = three quarters of the measured ratio, the margin the other perf tests keep
against a shared box.  The ratio against the exact join is recorded, not asserted: it depends on the configuration's recall.
LSHRS_PROFILE_OUT=<path>: the figures as JSON (profiles/lsh_pairs.json is one such run)."""

from __future__ import annotations

import json
import os

import numpy as np
import pytest

from tests.test_perf_exact_pairs import _corpus, _timed

# whole-call ratio detour / pairs_above measured on an MI355X (profiles/lsh_pairs.json)
MEASURED_RATIO = {"bfloat16": 4.639, "float32": 4.132}   # 29.9 / 6.45 ms and 28.5 / 6.91 ms
CHUNK = 10_000
BANDS, ROWS = 16, 16


@pytest.mark.perf
def test_perf_lsh_join_beats_the_query_detour():
    import torch

    from lshrs_amd import LSHRS, InMemoryStorage, _join
    from lshrs_amd._exact import _judge_pairs, collision_law

    assert torch.cuda.is_available(), "perf tests need a visible MI355X"

    m, dim, t = 200_000, 768, 0.75
    record = {"shape": {"rows": m, "dim": dim, "threshold": t, "num_bands": BANDS, "rows_per_band": ROWS, "band_bytes": 2,
                        "index_calls": 4, "detour_query_chunk": CHUNK}}
    for name in ("bfloat16", "float32"):
        corpus = _corpus(torch, m, dim, getattr(torch, name))
        rows32 = corpus.float()
        index = LSHRS(dim=dim, num_perm=BANDS * ROWS, num_bands=BANDS, rows_per_band=ROWS,
                      storage=InMemoryStorage(record_batches=False), packed_ingest=True)
        for lo in range(0, m, m // 4):
            index.index(np.arange(lo, lo + m // 4, dtype=np.int64), rows32[lo:lo + m // 4])
        index.set_corpus(corpus)
        index.pairs_above(t, return_arrays=True)                # (the first call folds the four segments: its cost, once)
        first = dict(index.last_search_stats)

        def join():
            return index.pairs_above(t, return_arrays=True)

        def detour():
            found = []
            for lo in range(0, m, CHUNK):
                ids, scores, bounds = index.query_many(rows32[lo:lo + CHUNK], top_k=None, top_p=1.0, return_arrays=True)
                asking = np.repeat(np.arange(lo, lo + bounds.shape[0] - 1, dtype=np.int64), np.diff(bounds))
                keep = (scores >= np.float32(t)) & (asking < ids)
                found.append((asking[keep], ids[keep], scores[keep]))
            return tuple(np.concatenate(part) for part in zip(*found))

        def exact():
            return index.pairs_exact_above(t, return_arrays=True)

        join_ms, (ja, jb, js, jc) = _timed(torch, join)
        stats = dict(index.last_search_stats)
        detour_ms, (da, db, ds) = _timed(torch, detour)
        exact_ms, (ea, eb, es) = _timed(torch, exact)
        # the join's parts
        seg = index._join_segment(corpus.device, 2, {})
        plan_ms, plan = _timed(torch, lambda: _join._plan(*seg, m, BANDS, 2, 1, None))
        emit_ms, (pa, pb, _, total, _) = _timed(torch, lambda: _join._emit(plan, stats["emitted"]))
        assert int(total.item()) == stats["emitted"]
        rerank_ms, _ = _timed(torch, lambda: _judge_pairs(torch, corpus, None, pa, pb, float(np.float32(t))))
        # the answer that was timed: the detour's pairs ...
        order = np.lexsort((db, da, -ds.astype(np.float64)))
        assert np.array_equal(ja, da[order]) and np.array_equal(jb, db[order])
        assert np.array_equal(js.view(np.uint32), ds[order].view(np.uint32))
        # ... and the exact join's pairs restricted to them, bit for bit
        found = set(zip(da.tolist(), db.tolist()))
        keep = np.array([p in found for p in zip(ea.tolist(), eb.tolist())], dtype=bool)
        assert np.array_equal(ja, ea[keep]) and np.array_equal(jb, eb[keep])
        assert np.array_equal(js.view(np.uint32), es[keep].view(np.uint32))
        assert jc.min() >= 1 and len(ja) == stats["kept"] and len(ea) >= m // 100 * 10
        record[name] = {
            "join_total_ms": join_ms, "detour_total_ms": detour_ms, "exact_total_ms": exact_ms,
            "ratio": detour_ms / join_ms, "ratio_to_exact": exact_ms / join_ms,
            "rowmap_ms": plan_ms, "emit_ms": emit_ms, "rerank_ms": rerank_ms, "emit_costs_more_than_rerank": emit_ms > rerank_ms,
            "fold_ms": first["fold_ms"], "segments_folded": first["segments_folded"],
            "buckets": stats["buckets"], "raw_pairs": stats["raw_pairs"], "emitted": stats["emitted"], "kept": stats["kept"],
            "launches": stats["launches"], "truth_pairs": int(len(ea)), "recall": len(ja) / len(ea),
            "expected_recall": collision_law(es, BANDS, ROWS),
        }
        del corpus, rows32, index, seg, plan
        torch.cuda.empty_cache()
    print(json.dumps(record))
    out = os.environ.get("LSHRS_PROFILE_OUT")
    if out:
        with open(out, "w") as fh:
            json.dump(record, fh, indent=1)
            fh.write("\n")
    for name in ("bfloat16", "float32"):
        assert record[name]["ratio"] >= 0.75 * MEASURED_RATIO[name], record
