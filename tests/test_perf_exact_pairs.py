"""Wall-clock check of the self-join, NOT part of `-m gpu` (a slow or shared box must not turn parity red): 200 000 x 768 rows,
about ten planted partners above a cosine of 0.75 for 1 % of them - the whole of exact_pairs_above against the same answer
obtained the way it was before the self-join existed: exact_above(rows.float(), rows, t) in chunks of 8 192 queries, cut to
(query id < row id).  Each route is timed once after a warm-up of the same call (a run takes tenths of a second: thousands of
times a launch's overhead), events around the whole call; the two first passes (lshrs_scan_pairs_* over all blocks,
lshrs_scan_above_* over all chunks) are timed the same way.  bf16 rows, then f32.  `pytest -m perf`.

What instruction counts predict for the first pass: half the (a, b) products (the triangle), and for bf16 one MFMA per step
instead of two (the queries' mid term is zero): about 4x on bf16 and about 2x on f32.
Measured on an MI355X (profiles/exact_pairs.json): bf16 whole call 106.3 ms against 210.5 ms, 1.98x, first pass 103.2 against
171.0 ms, 1.66x (298 TFLOP/s of bf16 MFMA executed); f32 240.6 against 338.7 ms, 1.41x, first pass 239.0 against 306.4 ms, 1.28x.
bf16 is UNDER 2x, less than the triangle alone should give.  The reason: the range scan's pass is not bound by its MFMAs - the
detour executes 719 TFLOP/s of them, the self-join with half as many per step 298 - so dropping the zero term's MFMA buys little:
what remains per chunk (the rows' loads, their fragments and norms on the vector ALU, the B chunk through LDS between two
barriers) takes as long as before.  And the kernel runs one workgroup per CU to stay free of scratch, which leaves a CU nothing
to do at those barriers: a build with two per CU (a few spilled dwords) measured 75.2 ms for the bf16 first pass, 2.26x, and
165.2 ms for f32, 1.86x.  Twenty-five launches of decreasing size, each ending in a part-filled tail, take their share too.
Floor: pairs <= detour / FLOOR per dtype, FLOOR = three quarters of the ratio of the whole calls measured on an MI355X
(profiles/exact_pairs.json), the margin tests/test_perf_exact_above.py keeps.
LSHRS_PROFILE_OUT=<path>: the figures as JSON (profiles/exact_pairs.json is one such run)."""

from __future__ import annotations

import json
import os

import numpy as np
import pytest

# whole-call ratio detour / exact_pairs_above measured on an MI355X (profiles/exact_pairs.json)
MEASURED_RATIO = {"bfloat16": 1.980, "float32": 1.408}   # 210.5 / 106.3 ms and 338.7 / 240.6 ms
CHUNK = 8192


def _corpus(torch, m, dim, dtype):
    gen = torch.Generator("cuda").manual_seed(7)
    x = torch.randn(m, dim, device="cuda", generator=gen)
    src = torch.randperm(m, device="cuda", generator=gen)[:m // 100]
    rest = torch.randperm(m, device="cuda", generator=gen)
    rest = rest[~torch.isin(rest, src)][:src.shape[0] * 10].reshape(-1, 10)
    scale = 0.5 + 1.5 * torch.rand(src.shape[0], 10, 1, device="cuda", generator=gen)
    x[rest.reshape(-1)] = (x[src][:, None, :] * scale
                           + 0.25 * torch.randn(src.shape[0], 10, dim, device="cuda", generator=gen)).reshape(-1, dim)
    return x.to(dtype)


def _timed(torch, fn):
    fn()                                                    # warm-up: allocator, code objects, clocks
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


@pytest.mark.perf
def test_perf_self_join_beats_the_range_search_detour():
    import torch

    assert torch.cuda.is_available(), "perf tests need a visible MI355X"
    from lshrs_amd import exact_above, exact_pairs_above
    from lshrs_amd._exact import above_bars, rerank_rounding, scan_above, scan_epsilon, scan_pairs

    m, dim, t = 200_000, 768, 0.75
    record = {"shape": {"rows": m, "dim": dim, "threshold": t, "detour_query_chunk": CHUNK}}
    for name in ("bfloat16", "float32"):
        corpus = _corpus(torch, m, dim, getattr(torch, name))
        bar = above_bars(np.array([t]), scan_epsilon(corpus.dtype, dim) + rerank_rounding(dim))
        stats = {}

        def pairs():
            return exact_pairs_above(corpus, t, return_tensors=True, stats=stats)

        def detour():
            queries = corpus.float()
            found = []
            for lo in range(0, m, CHUNK):
                ids, scores, bounds = exact_above(queries[lo:lo + CHUNK], corpus, t, return_tensors=True)
                asking = torch.repeat_interleave(torch.arange(lo, lo + bounds.shape[0] - 1, device="cuda"), bounds.diff())
                keep = asking < ids
                found.append((asking[keep], ids[keep], scores[keep]))
            return tuple(torch.cat(part) for part in zip(*found))

        def pairs_first_pass():
            return scan_pairs(corpus, float(bar[0]), 1 << 20)

        def detour_first_pass():
            queries = corpus.float()
            for lo in range(0, m, CHUNK):
                n = min(CHUNK, m - lo)
                scan_above(corpus, queries[lo:lo + n], torch.full((n,), float(bar[0]), device="cuda"), 1 << 20)

        pairs_ms, (pa, pb, ps) = _timed(torch, pairs)
        detour_ms, (da, db, ds) = _timed(torch, detour)
        pairs_first_ms, _ = _timed(torch, pairs_first_pass)
        detour_first_ms, _ = _timed(torch, detour_first_pass)
        # the answer that was timed: the detour's pairs, ordered as documented
        da, db, ds = da.cpu().numpy(), db.cpu().numpy(), ds.cpu().numpy()
        order = np.lexsort((db, da, -ds.astype(np.float64)))
        assert np.array_equal(pa.cpu().numpy(), da[order]) and np.array_equal(pb.cpu().numpy(), db[order])
        assert np.array_equal(ps.cpu().numpy().view(np.uint32), ds[order].view(np.uint32))
        assert ps.shape[0] >= m // 100 * 10
        terms = 1 if name == "bfloat16" else 3              # MFMAs per (step, tile, column block) of the self-join's pass
        record[name] = {
            "pairs_total_ms": pairs_ms, "detour_total_ms": detour_ms, "ratio": detour_ms / pairs_ms,
            "pairs_first_pass_ms": pairs_first_ms, "detour_first_pass_ms": detour_first_ms,
            "first_pass_ratio": detour_first_ms / pairs_first_ms,
            # bf16 multiply-adds the matrix cores execute for the triangle, as 2 flops each
            "pairs_first_pass_mfma_flops_per_s": terms * 2.0 * (m * (m - 1) / 2) * dim / (pairs_first_ms * 1e-3),
            # ... and the useful ones: one dot product per unordered pair
            "pairs_first_pass_pair_flops_per_s": 2.0 * (m * (m - 1) / 2) * dim / (pairs_first_ms * 1e-3),
            "emitted": stats["emitted"], "kept": stats["kept"], "launches": stats["launches"], "blocks": stats["blocks"],
            "floor": None if MEASURED_RATIO[name] is None else 0.75 * MEASURED_RATIO[name],
        }
        del corpus
        torch.cuda.empty_cache()
    print(json.dumps(record))
    out = os.environ.get("LSHRS_PROFILE_OUT")
    if out:
        with open(out, "w") as fh:
            json.dump(record, fh, indent=1)
            fh.write("\n")
    for name in ("bfloat16", "float32"):
        assert MEASURED_RATIO[name] is not None, "no measured ratio recorded: the floor cannot be set"
        assert record[name]["ratio"] >= 0.75 * MEASURED_RATIO[name], record
