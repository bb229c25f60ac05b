"""Wall-clock check of the rerank on a bf16 corpus, NOT part of `-m gpu` (a slow or shared box must not turn parity red):
BASELINE config 3's rerank - 1M x 768 corpus, 10 000 queries x 1 000 candidates through lshrs_cosine_ragged_* - with the
bf16 and the f32 launches interleaved in one process on the same candidate lists.  `pytest -m perf`."""

from __future__ import annotations

import numpy as np
import pytest


@pytest.mark.perf
def test_perf_bf16_rerank_reads_half_the_bytes_in_less_time():
    import torch

    assert torch.cuda.is_available(), "perf tests need a visible MI355X"
    from lshrs_amd import _native

    lib = _native.load()
    m, dim, q, c = 1_000_000, 768, 10_000, 1_000
    gen = torch.Generator("cuda").manual_seed(3)
    f32 = torch.randn(m, dim, device="cuda", generator=gen)
    bf16 = f32.to(torch.bfloat16)
    rng7, rng8 = np.random.default_rng(7), np.random.default_rng(8)        # the candidate table of tools/rerank_repro.py
    qrows = torch.from_numpy(rng7.choice(m, q, replace=False)).cuda()
    queries = f32[qrows] + torch.from_numpy((0.1 * rng7.standard_normal((q, dim))).astype(np.float32)).cuda()
    rows = torch.from_numpy(rng8.integers(0, m, (q, c), dtype=np.int64)).cuda().reshape(-1)
    row_off = torch.arange(q, dtype=torch.int64, device="cuda") * c
    row_cnt = torch.full((q,), c, dtype=torch.int32, device="cuda")
    scores = {k: torch.empty(q * c, dtype=torch.float32, device="cuda") for k in ("f32", "bf16")}
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    fn = {"f32": (lib.lshrs_cosine_ragged_f32, f32), "bf16": (lib.lshrs_cosine_ragged_bf16, bf16)}

    def launch(kind):
        f, corpus = fn[kind]
        _native.check(f(corpus.data_ptr(), m, dim, dim, queries.data_ptr(), q, rows.data_ptr(), row_off.data_ptr(),
                        row_cnt.data_ptr(), q * c, scores[kind].data_ptr(), err.data_ptr(), stream), kind)

    for _ in range(3):
        launch("f32")
        launch("bf16")
    times = {"f32": [], "bf16": []}
    for rnd in range(9):
        for kind in (("f32", "bf16") if rnd % 2 == 0 else ("bf16", "f32")):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch(kind)
            b.record()
            torch.cuda.synchronize()
            times[kind].append(a.elapsed_time(b))
    assert int(err.item()) == 0
    t32, t16 = sorted(times["f32"])[4], sorted(times["bf16"])[4]
    print(f"ragged rerank, config 3: f32 {t32:.3f} ms ({q * c / t32 / 1e6:.2f} G cand/s), "
          f"bf16 {t16:.3f} ms ({q * c / t16 / 1e6:.2f} G cand/s), {t32 / t16:.2f}x")
    assert float((scores["f32"] - scores["bf16"]).abs().max()) < 0.02                  # (the same lists: bf16-rounded rows)
    assert t32 / t16 >= 1.5
