"""Wall-clock check of the rerank on an 8-bit corpus, NOT part of `-m gpu` (a slow or shared box must not turn parity red):
BASELINE config 3's rerank - 1M x 768 corpus, 10 000 queries x 1 000 candidates through lshrs_cosine_ragged_* - with the
int8, e4m3fn and bf16 launches interleaved in one process on the same candidate lists.  `pytest -m perf`.

Floors: 0.75 x the median ratio over bf16 that profiles/eight_bit_corpus_rerank.json records (int8 1.83x, e4m3fn 1.86x),
never below 1.0 - the margin test_perf_half_corpus.py leaves under its own measurement."""

from __future__ import annotations

import numpy as np
import pytest

FLOOR_VS_BF16 = {"int8": 1.37, "float8_e4m3fn": 1.39}


@pytest.mark.perf
def test_perf_8bit_rerank_reads_half_the_bytes_of_bf16_in_less_time():
    import torch

    assert torch.cuda.is_available(), "perf tests need a visible MI355X"
    from lshrs_amd import _native, quantize_rows

    lib = _native.load()
    m, dim, q, c = 1_000_000, 768, 10_000, 1_000
    gen = torch.Generator("cuda").manual_seed(3)
    f32 = torch.randn(m, dim, device="cuda", generator=gen)
    corpora = {"bf16": f32.to(torch.bfloat16), "int8": quantize_rows(f32, torch.int8),
               "float8_e4m3fn": quantize_rows(f32, torch.float8_e4m3fn)}
    rng7, rng8 = np.random.default_rng(7), np.random.default_rng(8)        # the candidate table of tools/rerank_repro.py
    qrows = torch.from_numpy(rng7.choice(m, q, replace=False)).cuda()
    queries = f32[qrows] + torch.from_numpy((0.1 * rng7.standard_normal((q, dim))).astype(np.float32)).cuda()
    del f32
    rows = torch.from_numpy(rng8.integers(0, m, (q, c), dtype=np.int64)).cuda().reshape(-1)
    row_off = torch.arange(q, dtype=torch.int64, device="cuda") * c
    row_cnt = torch.full((q,), c, dtype=torch.int32, device="cuda")
    scores = {k: torch.empty(q * c, dtype=torch.float32, device="cuda") for k in corpora}
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    fn = {"bf16": lib.lshrs_cosine_ragged_bf16, "int8": lib.lshrs_cosine_ragged_i8,
          "float8_e4m3fn": lib.lshrs_cosine_ragged_f8e4m3}
    kinds = tuple(corpora)

    def launch(kind):
        _native.check(fn[kind](corpora[kind].data_ptr(), m, dim, dim, queries.data_ptr(), q, rows.data_ptr(), row_off.data_ptr(),
                               row_cnt.data_ptr(), q * c, scores[kind].data_ptr(), err.data_ptr(), stream), kind)

    for _ in range(3):
        for kind in kinds:
            launch(kind)
    times = {k: [] for k in kinds}
    for rnd in range(9):
        for kind in kinds[rnd % 3:] + kinds[:rnd % 3]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch(kind)
            b.record()
            torch.cuda.synchronize()
            times[kind].append(a.elapsed_time(b))
    assert int(err.item()) == 0
    med = {k: sorted(v)[4] for k, v in times.items()}
    print("ragged rerank, config 3: " + ", ".join(f"{k} {t:.3f} ms ({q * c / t / 1e6:.2f} G cand/s)" for k, t in med.items()))
    for kind, floor in FLOOR_VS_BF16.items():
        # (the same lists: the 8-bit rows are the quantized rows, bf16 the rounded ones - scores close, not equal)
        assert float((scores[kind] - scores["bf16"]).abs().max()) < 0.05, kind
        print(f"{kind}: {med['bf16'] / med[kind]:.2f}x bf16 (floor {floor})")
        assert med["bf16"] / med[kind] >= max(1.0, floor), kind
