"""Wall-clock check of the rerank through a DeviceVectors' id -> row table, NOT part of `-m gpu` (a slow or shared box must
not turn parity red): BASELINE config 3's rerank - 1M x 768 corpus, 10 000 queries x 1 000 candidates - with
A = lshrs_cosine_ragged_* on row numbers (the existing entry: the yardstick) and B = lshrs_idmap_lookup_ragged_i64 over random
40-bit ids + the same launch on its output, interleaved in one process.  `pytest -m perf`.

bfloat16: B <= 1.25 x A - the estimate from bytes (one 64-B table sector + 16 B per candidate beside the 1 548 B of row:
+5-10 %) plus the up-to-7 % box-to-box spread profiles/README.md records.  Measured: 1.067 (profiles/vector_store.json).
int8: profiles/vector_store.json records A / B = 1.3536 / 1.5266 ms = 0.887; the floor is 0.75 x that = 0.665 - the margin
test_perf_half_corpus.py and test_perf_eight_bit_corpus.py leave under their own measurements."""

from __future__ import annotations

import numpy as np
import pytest

BF16_CEILING_B_OVER_A = 1.25
INT8_FLOOR_A_OVER_B = 0.665          # 0.75 x 0.887 (profiles/vector_store.json: int8 A 1.3536 ms, B 1.5266 ms)


@pytest.mark.perf
def test_perf_rerank_through_the_map_against_the_plain_path():
    import torch

    assert torch.cuda.is_available(), "perf tests need a visible MI355X"
    from lshrs_amd import DeviceVectors, _native
    from lshrs_amd.similarity import corpus_entry

    lib = _native.load()
    m, dim, q, c = 1_000_000, 768, 10_000, 1_000
    rng = np.random.default_rng(11)
    ids = np.unique(rng.integers(0, 1 << 40, size=m + m // 4, dtype=np.int64))
    ids = rng.permutation(ids)[:m]                                   # row i holds id ids[i]
    gen = torch.Generator("cuda").manual_seed(3)
    stores = {k: DeviceVectors(dim, k, capacity=m) for k in ("bfloat16", "int8")}
    for lo in range(0, m, 125_000):
        x = torch.randn(125_000, dim, device="cuda", generator=gen)
        for store in stores.values():
            store.add(ids[lo:lo + 125_000], x)
    del x
    queries = torch.randn(q, dim, device="cuda", generator=gen)
    rows_h = rng.integers(0, m, (q, c), dtype=np.int64)
    rows = torch.from_numpy(rows_h).cuda().reshape(-1)
    cand_ids = torch.from_numpy(ids[rows_h]).cuda().reshape(-1)
    off = torch.arange(q, dtype=torch.int64, device="cuda") * c
    cnt = torch.full((q,), c, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    translated = torch.empty(q * c, dtype=torch.int64, device="cuda")
    scores = {v: torch.empty(q * c, dtype=torch.float32, device="cuda") for v in "AB"}
    stream = torch.cuda.current_stream().cuda_stream
    ratio = {}
    for kind, store in stores.items():
        corpus, table, slots = store.snapshot()
        entry = getattr(lib, corpus_entry(corpus, "ragged", dim))

        def cosine(cand, dst):
            _native.check(entry(corpus.data_ptr(), m, corpus.stride(0), dim, queries.data_ptr(), q, cand.data_ptr(), off.data_ptr(),
                                cnt.data_ptr(), q * c, dst.data_ptr(), err.data_ptr(), stream), "cosine")

        def form_a():
            cosine(rows, scores["A"])

        def form_b():
            _native.check(lib.lshrs_idmap_lookup_ragged_i64(table.data_ptr(), slots, cand_ids.data_ptr(), off.data_ptr(),
                                                            cnt.data_ptr(), q, q * c, translated.data_ptr(), err.data_ptr(), stream),
                          "lookup")
            cosine(translated, scores["B"])

        for _ in range(3):
            form_a()
            form_b()
        times = {"A": [], "B": []}
        for rnd in range(9):
            for name, fn in ((("A", form_a), ("B", form_b)) if rnd % 2 else (("B", form_b), ("A", form_a))):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                times[name].append(a.elapsed_time(b))
        assert int(err.item()) == 0 and torch.equal(translated, rows) and torch.equal(scores["A"], scores["B"])
        med = {k: sorted(v)[4] for k, v in times.items()}
        ratio[kind] = med["B"] / med["A"]
        print(f"{kind}: plain {med['A']:.3f} ms ({q * c / med['A'] / 1e6:.2f} G cand/s), through the map {med['B']:.3f} ms "
              f"({q * c / med['B'] / 1e6:.2f} G cand/s): B / A = {ratio[kind]:.3f}")
    assert ratio["bfloat16"] <= BF16_CEILING_B_OVER_A, ratio
    assert 1.0 / ratio["int8"] >= INT8_FLOOR_A_OVER_B, ratio
