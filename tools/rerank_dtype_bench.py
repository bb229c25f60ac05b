"""The cosine rerank on a device corpus stored in float32, bfloat16, float16, int8 and float8_e4m3fn - BASELINE config 3's
rerank: a 1M x 768 corpus, 10 000 queries x 1 000 candidates (the candidate table of tools/rerank_repro.py).  The 16-bit
corpora are the f32 rows rounded, the 8-bit ones the f32 rows through quantize_rows (a scale per row).

Per corpus dtype, in one process:
  kernel   lshrs_cosine_ragged_{f32,bf16,f16,i8,f8e4m3} timed by HIP events, the dtypes interleaved launch by launch (drift
           between them cancels), median of --launches each; candidates/s and the bytes a candidate needs (row + 8-B index +
           4-B score: element bytes * dim + 12) as a fraction of 8 TB/s; the largest score difference against the f32 kernel
           on the original rows (for 8 bits: the quantization's effect) and against the f32 kernel on corpus.float() (the
           kernel's own error)
  quantize quantize_rows' time on the 1M x 768 rows (median of 5) and the drift it brings, 1 - cos(row, quantized row)
  api      LSHRS.query_many(top_k=None, top_p=0.5, return_arrays=True) of the 10 000 queries against the corpus indexed under
           id = row, with that corpus attached (set_corpus): queries/s from host arrays and from queries already on the GPU
           (best of --reps, dtypes in rotating order)

Prints one JSON line (and writes it to --out).  Needs the MI355X: there is no CPU fallback.

    python tools/rerank_dtype_bench.py [--kernel-only] [--out FILE]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

M, DIM, Q, C = 1_000_000, 768, 10_000, 1_000
PEAK = 8.0e12
DTYPES = ("float32", "bfloat16", "float16", "int8", "float8_e4m3fn")
EIGHT = ("int8", "float8_e4m3fn")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=11)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true", help="skip the query_many part (a profiler run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("rerank_dtype_bench: no GPU visible - this tool measures the MI355X and has no CPU fallback")
    from lshrs_amd import _native
    from lshrs_amd.similarity import corpus_entry, quantize_rows

    lib = _native.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    gen = torch.Generator(dev).manual_seed(20240101)
    f32 = torch.empty((M, DIM), dtype=torch.float32, device=dev)
    for lo in range(0, M, 250_000):
        f32[lo:lo + 250_000] = torch.randn(250_000, DIM, device=dev, generator=gen)
    corpora = {"float32": f32, "bfloat16": f32.to(torch.bfloat16), "float16": f32.to(torch.float16)}
    quantize = {}
    for kind in EIGHT:
        dt = getattr(torch, kind)
        corpora[kind] = quantize_rows(f32, dt)                     # (also the warm-up of the timed calls below)
        ts = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            again = quantize_rows(f32, dt)
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
            assert torch.equal(again.view(torch.uint8), corpora[kind].view(torch.uint8))
        del again
        # 1 - cos(row, quantized row), in float64
        drift = []
        for lo in range(0, M, 125_000):
            x = f32[lo:lo + 125_000].double()
            y = corpora[kind][lo:lo + 125_000].double()
            drift.append(1 - (x * y).sum(1) / (x.norm(dim=1) * y.norm(dim=1)))
        drift = torch.cat(drift)
        quantize[kind] = {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                          "drift_1_minus_cos_mean": float(drift.mean()), "drift_1_minus_cos_max": float(drift.max())}
        del drift
    rng7, rng8 = np.random.default_rng(7), np.random.default_rng(8)
    qrows = rng7.choice(M, Q, replace=False)
    noise = (0.1 * rng7.standard_normal((Q, DIM))).astype(np.float32)
    queries = f32[torch.from_numpy(qrows).to(dev)] + torch.from_numpy(noise).to(dev)
    rows = torch.from_numpy(rng8.integers(0, M, (Q, C), dtype=np.int64)).to(dev).reshape(-1)
    row_off = torch.arange(Q, dtype=torch.int64, device=dev) * C
    row_cnt = torch.full((Q,), C, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    scores = {k: torch.empty(Q * C, dtype=torch.float32, device=dev) for k in DTYPES}
    stream = torch.cuda.current_stream(dev).cuda_stream

    def launch(kind, corpus=None, out=None):
        corpus = corpora[kind] if corpus is None else corpus
        entry = corpus_entry(corpus, "ragged", DIM)
        _native.check(getattr(lib, entry)(corpus.data_ptr(), M, corpus.stride(0), DIM, queries.data_ptr(), Q, rows.data_ptr(),
                                          row_off.data_ptr(), row_cnt.data_ptr(), Q * C,
                                          (scores[kind] if out is None else out).data_ptr(), err.data_ptr(), stream), entry)

    for _ in range(4):
        for kind in DTYPES:
            launch(kind)
    ms = {k: [] for k in DTYPES}
    for rnd in range(args.launches):
        order = DTYPES[rnd % len(DTYPES):] + DTYPES[:rnd % len(DTYPES)]
        for kind in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch(kind)
            b.record()
            torch.cuda.synchronize()
            ms[kind].append(a.elapsed_time(b))
    assert int(err.item()) == 0, "a candidate outside the corpus or of zero norm"
    kernel = {}
    for kind in DTYPES:
        med = float(np.median(ms[kind]))
        per_cand = corpora[kind].element_size() * DIM + 8 + 4
        kernel[kind] = {"median_ms": round(med, 4), "min_ms": round(min(ms[kind]), 4), "max_ms": round(max(ms[kind]), 4),
                        "launches": len(ms[kind]), "candidates_per_s": Q * C / (med * 1e-3),
                        "bytes_per_candidate": per_cand, "fraction_of_8TBps": Q * C * per_cand / (med * 1e-3) / PEAK}
        # the narrower scores against the f32 kernel's on the same lists (bf16 / f16 rows are the f32 rows rounded, the 8-bit
        # ones quantized) and against the f32 kernel on the upcast corpus (the kernel's own error)
        kernel[kind]["max_abs_diff_vs_f32"] = float((scores[kind] - scores["float32"]).abs().max())
        if kind != "float32":
            upcast, ref = corpora[kind].float(), torch.empty(Q * C, dtype=torch.float32, device=dev)
            launch("float32", upcast, ref)
            torch.cuda.synchronize()
            kernel[kind]["max_abs_diff_vs_upcast"] = float((scores[kind] - ref).abs().max())
            del upcast, ref
    assert int(err.item()) == 0
    for kind in DTYPES[1:]:
        kernel[kind]["speedup_vs_f32"] = kernel["float32"]["median_ms"] / kernel[kind]["median_ms"]
    for kind in EIGHT:
        kernel[kind]["speedup_vs_bf16"] = kernel["bfloat16"]["median_ms"] / kernel[kind]["median_ms"]
    out = {"tool": "rerank_dtype_bench", "device": torch.cuda.get_device_name(dev), "corpus_rows": M, "dim": DIM, "queries": Q,
           "candidates_per_query": C, "kernel": kernel, "quantize_rows_1M_x_768": quantize}

    if not args.kernel_only:
        from lshrs_amd import LSHRS, InMemoryStorage

        host = f32.cpu().numpy()
        idx = LSHRS(dim=DIM, num_perm=256, storage=InMemoryStorage(), packed_ingest=True)
        t0 = time.perf_counter()
        idx.index(np.arange(M, dtype=np.int64), host)
        index_s = time.perf_counter() - t0
        q_host = queries.cpu().numpy()
        idx.query_many(q_host[:200], top_k=10)                # (the store's bucket arrays go to the device once)
        api = {k: {} for k in DTYPES}
        for rnd in range(args.reps):
            for kind in DTYPES[rnd % len(DTYPES):] + DTYPES[:rnd % len(DTYPES)]:
                idx.set_corpus(corpora[kind])
                for form, qs in (("host_arrays", q_host), ("queries_on_gpu", queries)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ids, sc, bounds = idx.query_many(qs, top_k=None, top_p=0.5, return_arrays=True)
                    dt = time.perf_counter() - t0
                    api[kind][form] = max(api[kind].get(form, 0.0), Q / dt)
                    api[kind]["pairs_per_query"] = float(idx.last_query_stats["pairs"]) / Q
                    api[kind]["kept"] = int(bounds[-1])
        for kind in DTYPES:
            api[kind] = {k: (round(v, 1) if isinstance(v, float) else v) for k, v in api[kind].items()}
        out["query_many_top_p_0.5_arrays_queries_per_s"] = api
        out["index_seconds"] = round(index_s, 2)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
