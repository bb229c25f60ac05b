"""Wall-clock check of the exact search, NOT part of `-m gpu` (a slow or shared box must not turn parity red): 256 queries
against 200 000 x 768 bf16 rows, top 10 - the whole scan method (first pass, rescoring, ordering, settle) against the SCORING
LAUNCH ALONE of the gather method, lshrs_cosine_batch_bf16 over all rows: the kernels the package had before the scan, so the
comparison never is against the code under test.  Interleaved in one process, median of 9.  `pytest -m perf`.

Floor: scan total <= gather scoring / 8.  A query tile of at least 32 reads every row at least 32 times less often than the
gather does; a factor of four is left for selection, rescoring, ordering and the matrix work.
LSHRS_PROFILE_OUT=<path>: the figures as JSON (profiles/exact_search.json is one such run)."""

from __future__ import annotations

import json
import os

import numpy as np
import pytest


@pytest.mark.perf
def test_perf_scan_beats_the_gather_scoring_launch():
    import torch

    assert torch.cuda.is_available(), "perf tests need a visible MI355X"
    from lshrs_amd import exact_top_k
    from lshrs_amd._exact import scan_windows
    from lshrs_amd.similarity import cosine_scores_device

    m, dim, q, k = 200_000, 768, 256, 10
    gen = torch.Generator("cuda").manual_seed(3)
    corpus = torch.randn(m, dim, device="cuda", generator=gen).to(torch.bfloat16)
    queries = torch.randn(q, dim, device="cuda", generator=gen)
    all_rows = torch.arange(m, dtype=torch.int64, device="cuda").unsqueeze(0).expand(q, m).contiguous()
    stats = {}

    def run(kind):
        if kind == "scan":
            return exact_top_k(queries, corpus, k, method="scan", return_tensors=True, stats=stats)
        if kind == "first_pass":
            return scan_windows(corpus, queries, 32)
        return cosine_scores_device(corpus, queries, all_rows)

    kinds = ("scan", "gather_scoring", "first_pass")
    for _ in range(3):
        for kind in kinds:
            run(kind)
    torch.cuda.synchronize()
    times = {kind: [] for kind in kinds}
    for rnd in range(9):
        for kind in (kinds if rnd % 2 == 0 else kinds[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(kind)
            b.record()
            torch.cuda.synchronize()
            times[kind].append(a.elapsed_time(b))
    scan, gather, first = (sorted(times[kind])[4] for kind in kinds)
    ids, scores = exact_top_k(queries, corpus, k, method="scan", stats=stats)
    g_ids, g_scores = exact_top_k(queries[:16], corpus, k, method="gather")
    assert np.array_equal(ids[:16], g_ids) and np.array_equal(scores[:16], g_scores)
    tiles = (q + 63) // 64
    record = {
        "shape": {"rows": m, "dim": dim, "dtype": "bfloat16", "queries": q, "k": k, "window": stats["window"]},
        "scan_total_ms": scan, "scan_first_pass_ms": first, "gather_scoring_ms": gather, "ratio": gather / scan,
        "first_pass_bytes_per_s": tiles * m * dim * 2 / (first * 1e-3),
        "first_pass_share_of_8TBps": tiles * m * dim * 2 / (first * 1e-3) / 8e12,
        "first_pass_bf16_flops_per_s": 2 * 2.0 * m * dim * tiles * 64 / (first * 1e-3),
        "gather_candidates_per_s": q * m / (gather * 1e-3),
        "settled_share": stats["settled_first_pass"] / q, "epsilon": stats["epsilon"],
    }
    print(json.dumps(record))
    out = os.environ.get("LSHRS_PROFILE_OUT")
    if out:
        with open(out, "w") as fh:
            json.dump(record, fh, indent=1)
            fh.write("\n")
    assert scan <= gather / 8, record
