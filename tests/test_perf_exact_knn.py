"""Wall-clock check of the k-NN self-join, NOT part of `-m gpu` (a slow or shared box must not turn parity red): 200 000 x 768
rows, k = 10 - the whole of exact_knn against the same answer obtained the way it was before exact_knn existed:
exact_top_k(rows.float()[chunk], rows, 11) in chunks of 8 192 queries, the row itself dropped (or else the last entry).  Each
route is timed once after a warm-up of the same call (a run takes tenths of a second: thousands of times a launch's overhead),
events around the whole call; the two first passes (lshrs_scan_knn_* over all chunks, lshrs_scan_topk_* over all chunks of the
float32 copy) are timed the same way.  bf16 rows, then f32.  `pytest -m perf`.

What instruction counts predict for the first pass: for bf16 one MFMA per step instead of two (the queries' mid term is zero),
up to 2x; for f32 the same three MFMAs, 1x.  No triangle here: every block scans all rows.  On top, the detour's float32 copy
of the rows (614 MB) and the image built from it come off.
Measured on an MI355X (profiles/exact_knn.json): bf16 whole call 205.1 ms against 211.2 ms, 1.03x, first pass 201.0 against
196.2 ms, 0.98x (306 TFLOP/s of bf16 MFMA executed); f32 368.3 against 369.3 ms, 1.00x, first pass 362.8 against 353.0 ms, 0.97x.
Parity, not 2x, and the first pass a few percent BEHIND.  The reason: the pass is not bound by its MFMAs (the detour executes
twice as many in the same time), so dropping the zero term's MFMA buys nothing - what remains per chunk (the rows' loads, their
fragments and norms on the vector ALU, the B chunk through LDS between two barriers) takes as long as before - and the SELF
instantiations spill a few dwords more than the others (20 against 12 bytes a lane for aligned bf16 rows).  The whole call gains
what it no longer does: the float32 copy and the image from it.  The kernel runs two workgroups per CU: a build with one per CU
(no scratch) measured 295.6 ms for the bf16 whole call, 0.72x, and 513.6 ms for f32, 0.72x (`variant_one_workgroup_per_cu`).
Floor: knn <= detour / FLOOR per dtype, FLOOR = three quarters of the ratio of the whole calls measured on an MI355X
(profiles/exact_knn.json), the margin tests/test_perf_exact_pairs.py keeps.
LSHRS_PROFILE_OUT=<path>: the figures as JSON (profiles/exact_knn.json is one such run)."""

from __future__ import annotations

import json
import os

import pytest

# whole-call ratio detour / exact_knn measured on an MI355X (profiles/exact_knn.json)
MEASURED_RATIO = {"bfloat16": 1.030, "float32": 1.003}      # 211.2 / 205.1 ms and 369.3 / 368.3 ms
CHUNK = 8192
K = 10


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
def test_perf_knn_self_join_beats_the_top_k_detour():
    import torch

    assert torch.cuda.is_available(), "perf tests need a visible MI355X"
    from lshrs_amd import _native, exact_knn, exact_top_k
    from lshrs_amd._exact import _knn_chunk, _pairs_block, choose_window, scan_knn, scan_max_window, scan_windows

    m, dim = 200_000, 768
    record = {"shape": {"rows": m, "dim": dim, "k": K, "detour_query_chunk": CHUNK}}
    for name in ("bfloat16", "float32"):
        corpus = _corpus(torch, m, dim, getattr(torch, name))
        window = choose_window(K, scan_max_window())
        chunk = _knn_chunk(_pairs_block(_native.load(), m, dim), dim, window)
        stats = {}

        def knn():
            return exact_knn(corpus, K, return_tensors=True, stats=stats)

        def detour():
            queries = corpus.float()
            found = []
            for lo in range(0, m, CHUNK):
                ids, scores = exact_top_k(queries[lo:lo + CHUNK], corpus, K + 1, return_tensors=True)
                own = torch.arange(lo, lo + ids.shape[0], device="cuda").unsqueeze(1)
                is_self = ids == own
                drop = torch.where(is_self.any(dim=1), is_self.int().argmax(dim=1), torch.full_like(own[:, 0], K))
                stay = torch.arange(K + 1, device="cuda").unsqueeze(0) != drop.unsqueeze(1)
                found.append((ids[stay].view(-1, K), scores[stay].view(-1, K)))
            return tuple(torch.cat(part) for part in zip(*found))

        def knn_first_pass():
            for lo in range(0, m, chunk):
                scan_knn(corpus, lo, min(chunk, m - lo), window)

        def detour_first_pass():
            queries = corpus.float()
            for lo in range(0, m, CHUNK):
                scan_windows(corpus, queries[lo:lo + CHUNK], choose_window(K + 1, scan_max_window()))

        knn_ms, (ids, nbrs, scores) = _timed(torch, knn)
        detour_ms, (d_n, d_s) = _timed(torch, detour)
        knn_first_ms, _ = _timed(torch, knn_first_pass)
        detour_first_ms, _ = _timed(torch, detour_first_pass)
        # the answer that was timed
        assert torch.equal(ids, torch.arange(m, device="cuda")) and torch.equal(nbrs, d_n)
        assert torch.equal(scores.view(torch.int32), d_s.view(torch.int32))
        terms = 1 if name == "bfloat16" else 3              # MFMAs per (step, tile, column block) of the self-join's pass
        record[name] = {
            "knn_total_ms": knn_ms, "detour_total_ms": detour_ms, "ratio": detour_ms / knn_ms,
            "knn_first_pass_ms": knn_first_ms, "detour_first_pass_ms": detour_first_ms,
            "first_pass_ratio": detour_first_ms / knn_first_ms,
            # bf16 multiply-adds the matrix cores execute for the full square, as 2 flops each
            "knn_first_pass_mfma_flops_per_s": terms * 2.0 * m * m * dim / (knn_first_ms * 1e-3),
            "window": stats["window"], "chunks": stats["chunks"], "settled_first_pass": stats["settled_first_pass"],
            "gathered": stats["gathered"],
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
