"""What the id -> row translation of a ``DeviceVectors`` costs (csrc/idmap.hip), against the plain device-corpus path.

  kernel   BASELINE config 3's rerank - 1M x 768 corpus, 10 000 queries x 1 000 candidates - for bfloat16 and int8 rows:
           A = lshrs_cosine_ragged_* on row numbers (the yardstick), B = lshrs_idmap_lookup_ragged_i64 over random 40-bit
           ids + the same launch on its output, L = the lookup alone.  HIP events, A / B / L interleaved launch by launch in
           one process, median of --launches each.
  api      one index (500 000 x 768 under ids 0 .. n-1, so that the plain tensor is usable too), the same queries:
           query_many(top_k=None, top_p=0.5, return_arrays=True) of 10 000 queries and get_above_p(p=0.5) per call, with the
           plain bfloat16 tensor attached and with the DeviceVectors of the same rows (interleaved, medians).
  index    LSHRS.index() of 500 000 x 768 with keep_vectors off / "bfloat16" / "int8", the rows given from host memory and as
           a CUDA tensor (best of --reps; a host array is uploaded a second time for the store).

Prints one JSON line (and writes it to --out, default profiles/vector_store.json).  Needs the MI355X: no CPU fallback.

    python tools/vector_store_bench.py [--kernel-only] [--out FILE]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

M, DIM, Q, C = 1_000_000, 768, 10_000, 1_000
N_INDEX = 500_000
KINDS = ("bfloat16", "int8")


def rerank_through_the_map(torch, launches: int):
    """{kind: {"A_ms", "B_ms", "L_ms", "B_over_A"}} - shared with tests/test_perf_vector_store.py."""
    from lshrs_amd import DeviceVectors, _native
    from lshrs_amd.similarity import corpus_entry

    lib = _native.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(dev).manual_seed(20240101)
    rng = np.random.default_rng(11)
    ids = np.unique(rng.integers(0, 1 << 40, size=M + M // 4, dtype=np.int64))
    ids = rng.permutation(ids)[:M]                                   # row i holds id ids[i]
    stores = {k: DeviceVectors(DIM, k, capacity=M) for k in KINDS}
    qrows = rng.choice(M, Q, replace=False)
    queries = torch.empty((Q, DIM), dtype=torch.float32, device=dev)
    for lo in range(0, M, 125_000):
        x = torch.randn(125_000, DIM, device=dev, generator=gen)
        for k in KINDS:
            stores[k].add(ids[lo:lo + 125_000], x)
        inside = np.flatnonzero((qrows >= lo) & (qrows < lo + 125_000))
        queries[torch.from_numpy(inside).to(dev)] = x[torch.from_numpy(qrows[inside] - lo).to(dev)]
    queries += 0.1 * torch.randn(Q, DIM, device=dev, generator=gen)
    rows_h = rng.integers(0, M, (Q, C), dtype=np.int64)
    rows = torch.from_numpy(rows_h).to(dev).reshape(-1)
    cand_ids = torch.from_numpy(ids[rows_h]).to(dev).reshape(-1)
    del rows_h
    off = torch.arange(Q, dtype=torch.int64, device=dev) * C
    cnt = torch.full((Q,), C, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    translated = torch.empty(Q * C, dtype=torch.int64, device=dev)
    scores = {v: torch.empty(Q * C, dtype=torch.float32, device=dev) for v in ("A", "B")}
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {}
    for kind in KINDS:
        corpus, table, slots = stores[kind].snapshot()
        entry = getattr(lib, corpus_entry(corpus, "ragged", DIM))

        def cosine(cand, dst):
            _native.check(entry(corpus.data_ptr(), M, corpus.stride(0), DIM, queries.data_ptr(), Q, cand.data_ptr(), off.data_ptr(),
                                cnt.data_ptr(), Q * C, dst.data_ptr(), err.data_ptr(), stream), "cosine")

        def lookup():
            _native.check(lib.lshrs_idmap_lookup_ragged_i64(table.data_ptr(), slots, cand_ids.data_ptr(), off.data_ptr(),
                                                            cnt.data_ptr(), Q, Q * C, translated.data_ptr(), err.data_ptr(), stream),
                          "lookup")

        forms = {"A": lambda: cosine(rows, scores["A"]), "B": lambda: (lookup(), cosine(translated, scores["B"])), "L": lookup}
        for _ in range(3):
            for f in forms.values():
                f()
        ms = {v: [] for v in forms}
        names = tuple(forms)
        for rnd in range(launches):
            for v in names[rnd % 3:] + names[:rnd % 3]:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                forms[v]()
                b.record()
                torch.cuda.synchronize()
                ms[v].append(a.elapsed_time(b))
        assert int(err.item()) == 0 and torch.equal(translated, rows) and torch.equal(scores["A"], scores["B"])
        med = {v: float(np.median(t)) for v, t in ms.items()}
        out[kind] = {"A_ms": round(med["A"], 4), "B_ms": round(med["B"], 4), "L_ms": round(med["L"], 4),
                     "B_over_A": round(med["B"] / med["A"], 4), "launches": launches,
                     "A_min_max_ms": [round(min(ms["A"]), 4), round(max(ms["A"]), 4)],
                     "B_min_max_ms": [round(min(ms["B"]), 4), round(max(ms["B"]), 4)],
                     "A_candidates_per_s": Q * C / (med["A"] * 1e-3), "B_candidates_per_s": Q * C / (med["B"] * 1e-3),
                     "table_slots": slots, "table_bytes": 16 * slots}
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=11)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vector_store.json"))
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("vector_store_bench: no GPU visible - this tool measures the MI355X and has no CPU fallback")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    out = {"tool": "vector_store_bench", "device": torch.cuda.get_device_name(dev), "corpus_rows": M, "dim": DIM, "queries": Q,
           "candidates_per_query": C, "rerank_through_the_map": rerank_through_the_map(torch, args.launches)}
    torch.cuda.empty_cache()

    if not args.kernel_only:
        from lshrs_amd import LSHRS, InMemoryStorage

        gen = torch.Generator(dev).manual_seed(5)
        x_dev = torch.randn(N_INDEX, DIM, device=dev, generator=gen)
        x_host = x_dev.cpu().numpy()
        ids = np.arange(N_INDEX, dtype=np.int64)
        index_s: dict = {}
        kept = None
        for rep in range(args.reps):
            for keep in (None, "bfloat16", "int8"):
                for form, rows in (("host", x_host), ("cuda", x_dev)):
                    idx = LSHRS(dim=DIM, num_perm=256, storage=InMemoryStorage(), packed_ingest=True, keep_vectors=keep)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    idx.index(ids, rows)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    key = f"keep_vectors={keep}"
                    index_s.setdefault(key, {})[form] = min(index_s.get(key, {}).get(form, 1e9), dt)
                    if keep == "bfloat16" and form == "cuda":
                        kept = idx
        out["index_500k_x_768_seconds_best"] = {k: {f: round(v, 4) for f, v in d.items()} for k, d in index_s.items()}
        out["index_500k_x_768_rows_per_s"] = {k: {f: round(N_INDEX / v, 1) for f, v in d.items()} for k, d in index_s.items()}

        plain = x_dev.to(torch.bfloat16)
        assert torch.equal(plain.view(torch.int16), kept.vectors.rows.view(torch.int16))
        rng = np.random.default_rng(3)
        q_host = (x_host[rng.choice(N_INDEX, Q, replace=False)] + 0.1 * rng.standard_normal((Q, DIM))).astype(np.float32)
        kept.query_many(q_host[:200], top_k=10)
        many = {"plain_tensor": [], "device_vectors": []}
        for rnd in range(2 * args.reps + 3):
            for name in (("plain_tensor", "device_vectors") if rnd % 2 else ("device_vectors", "plain_tensor")):
                kept.set_corpus(plain if name == "plain_tensor" else None)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = kept.query_many(q_host, top_k=None, top_p=0.5, return_arrays=True)
                many[name].append(time.perf_counter() - t0)
                if name == "plain_tensor":
                    want = got
                elif rnd:
                    assert all(np.array_equal(a, b) for a, b in zip(got, want))
        out["query_many_top_p_0.5_arrays_ms"] = {k: round(1e3 * float(np.median(v[1:])), 3) for k, v in many.items()}
        out["query_many_pairs_per_query"] = float(kept.last_query_stats["pairs"]) / Q
        one = {"plain_tensor": [], "device_vectors": []}
        for i in range(400):
            for name in (("plain_tensor", "device_vectors") if i % 2 else ("device_vectors", "plain_tensor")):
                kept.set_corpus(plain if name == "plain_tensor" else None)
                t0 = time.perf_counter()
                kept.get_above_p(q_host[i], p=0.5)
                one[name].append(time.perf_counter() - t0)
        out["get_above_p_0.5_us_per_call"] = {k: round(1e6 * float(np.median(v[40:])), 2) for k, v in one.items()}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
