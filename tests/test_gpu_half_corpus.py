"""The rerank on a device corpus stored in bfloat16 or float16 (lshrs_cosine_{batch,ragged}_{bf16,f16}, cosine_kernel's 16-bit
instantiations): every element converted to f32 exactly, the scores those of the upcast corpus.  Against the f32 kernel on
``corpus.float()``, the float64 cosine, and the reference's flow restated literally (oracle.query_literal) with a fetch
function that upcasts - the reference reranks ``np.asarray(fetch(ids), dtype=np.float32)`` (lshrs/core/main.py:636)."""

from __future__ import annotations

import math

import numpy as np
import pytest

from tests._ranking import judge_ranking

pytestmark = pytest.mark.gpu
HALF = ("bfloat16", "float16")


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _clustered(rng, n, dim, clusters, spread):
    centers = rng.standard_normal((clusters, dim)).astype(np.float32)
    return (np.repeat(centers, n // clusters, axis=0) + spread * rng.standard_normal((n, dim))).astype(np.float32)


def _corpora(torch, dim, m, seed, width=None, col=0):
    """(f32 host rows, {dtype: device corpus}): rows of widely varying norms, two of them zero; `width` > dim: the corpus is
    the column slice [col, col + dim) of a wider tensor (row stride `width` elements)."""
    rng = np.random.default_rng(seed)
    rows = (rng.standard_normal((m, dim)) * rng.uniform(0.01, 100, size=(m, 1))).astype(np.float32)
    rows[3] = 0
    rows[m - 1] = 0
    out = {}
    for name in HALF:
        dt = getattr(torch, name)
        if width is None:
            out[name] = torch.from_numpy(rows).cuda().to(dt)
        else:
            big = torch.zeros((m, width), dtype=dt, device="cuda")
            big[:, col:col + dim] = torch.from_numpy(rows).cuda().to(dt)
            out[name] = big[:, col:col + dim]
            assert out[name].stride(0) == width and out[name].stride(1) == 1
    return rows, out


@pytest.mark.parametrize("dim,c,width,col", [(4, 7, None, 0), (30, 65, None, 0), (100, 1000, None, 0), (768, 1000, None, 0),
                                             (1536, 333, None, 0), (2050, 64, None, 0), (50, 300, None, 0),
                                             (64, 300, 72, 0),        # ldc > dim, aligned
                                             (64, 300, 70, 0),        # ldc not a multiple of 8
                                             (64, 300, 72, 1)])       # base 2 bytes past a 16-B boundary
def test_half_kernel_equals_f32_kernel_on_the_upcast(dim, c, width, col):
    torch = _torch()
    from oracle.build import cosine_f64

    from lshrs_amd.similarity import cosine_scores_device

    m = c + 40
    _, corpora = _corpora(torch, dim, m, dim * 7 + c, width, col)
    rng = np.random.default_rng(dim + c)
    q = 3
    queries = torch.from_numpy(rng.standard_normal((q, dim)).astype(np.float32)).cuda()
    queries[2] = 0                                                           # a zero query
    idx = torch.from_numpy(rng.integers(0, m, size=(q, c))).cuda()
    idx[0, 0], idx[0, 1] = 3, m - 1                                          # zero rows
    idx[1, 0] = -1
    idx[1, c - 1] = m                                                        # outside the corpus
    for name, corpus in corpora.items():
        up = corpus.float()
        s16, st16, qs16 = cosine_scores_device(corpus, queries, idx)
        s32, st32, qs32 = cosine_scores_device(up, queries, idx)
        assert torch.equal(st16, st32) and torch.equal(qs16, qs32), name
        assert st16[0, 0] == 1 and st16[0, 1] == 1 and st16[1, 0] == 2 and st16[1, c - 1] == 2 and qs16.tolist() == [0, 0, 1]
        ok = (st16 == 0) & (qs16 == 0)[:, None]
        assert torch.equal(torch.isnan(s16), ~ok), name                      # NaN exactly where a status is set
        assert float((s16[ok] - s32[ok]).abs().max()) <= 2e-6, name
        up_h, q_h, i_h = up.cpu().numpy(), queries.cpu().numpy(), idx.cpu().numpy()
        for qi in range(2):
            valid = ok[qi].cpu().numpy()
            want = cosine_f64(q_h[qi], up_h[i_h[qi][valid]])
            assert np.abs(s16[qi].cpu().numpy()[valid] - want).max() <= 2e-6, (name, qi)


@pytest.mark.parametrize("dim", [64, 50])
def test_f16_subnormals_and_large_bf16_rows_are_exact(dim):
    """f16 rows made only of subnormals (multiples of 2^-24) score their true cosine - a flush to zero would report a zero
    norm; bf16 rows near the top of the f32 range give what the f32 kernel gives on the upcast."""
    torch = _torch()
    from lshrs_amd.similarity import cosine_scores_device

    rng = np.random.default_rng(dim)
    q = rng.standard_normal((1, dim)).astype(np.float32)
    sub = rng.integers(1, 1024, size=(4, dim)) * rng.choice([-1, 1], size=(4, dim))
    sub_f16 = torch.from_numpy((sub * 2.0 ** -24).astype(np.float16)).cuda()
    assert bool((sub_f16.abs() < 2.0 ** -14).all())                           # all subnormal in f16
    s, st, _ = cosine_scores_device(sub_f16, torch.from_numpy(q).cuda(), None, c=4)
    assert st.tolist() == [[0, 0, 0, 0]]
    exact = sub.astype(np.float64)
    want = exact @ q[0].astype(np.float64) / (np.linalg.norm(exact, axis=1) * np.linalg.norm(q[0].astype(np.float64)))
    assert np.abs(s[0].cpu().numpy() - want).max() <= 2e-6

    big = np.stack([rng.standard_normal(dim) * 2.0 ** 56,                  # squares near 2^112: the norm still fits f32
                    np.full(dim, 2.0 ** 100),                              # squares beyond f32: ||c|| = inf in both kernels
                    rng.standard_normal(dim) * 3e38]).astype(np.float32)
    big_bf16 = torch.from_numpy(big).cuda().to(torch.bfloat16)
    qd = torch.from_numpy(q).cuda()
    s16, st16, _ = cosine_scores_device(big_bf16, qd, None, c=3)
    s32, st32, _ = cosine_scores_device(big_bf16.float(), qd, None, c=3)
    assert torch.equal(st16, st32)
    a, b = s16.cpu().numpy()[0], s32.cpu().numpy()[0]
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))
    fin = np.isfinite(a)
    assert fin[0] and np.abs(a[fin] - b[fin]).max() <= 2e-6


@pytest.mark.parametrize("dim,num_perm,nb,r,n,clusters,spread", [
    (64, 64, 16, 4, 1500, 150, 0.35),
    (768, 256, 16, 16, 2000, 200, 0.3),
    (96, 512, 16, 32, 1500, 150, 0.25),
    (50, 40, 8, 5, 1000, 50, 0.3),
])
def test_query_many_on_a_half_corpus_equals_the_reference_flow(dim, num_perm, nb, r, n, clusters, spread):
    torch = _torch()
    from lshrs_amd import LSHRS, InMemoryStorage
    from oracle import lshrs_oracle as O

    rng = np.random.default_rng(dim * 7 + nb)
    data = _clustered(rng, n, dim, clusters, spread)
    store = InMemoryStorage()
    idx = LSHRS(dim=dim, num_perm=num_perm, num_bands=nb, rows_per_band=r, storage=store, packed_ingest=True, seed=42)
    third = n // 3
    idx.index(np.arange(third), data[:third])
    idx.index(np.arange(third, 2 * third), data[third:2 * third])
    idx.index(np.arange(2 * third, n), data[2 * third:])
    idx.index(np.arange(100), data[:100])
    nq = 300
    queries = (data[rng.choice(n, nq, replace=False)] + 0.05 * rng.standard_normal((nq, dim))).astype(np.float32)
    queries[::50] = rng.standard_normal((len(queries[::50]), dim)).astype(np.float32)
    P = idx._hasher.projections
    lit_all = [O.query_literal(store, P, dim, v, top_k=None) for v in queries]
    sample = np.r_[0:12, 290:300] if r > 4 else np.r_[0:6, 295:300]
    for name in HALF:
        corpus = torch.from_numpy(data).cuda().to(getattr(torch, name))
        upcast = corpus.float().cpu().numpy()
        fetch = lambda ids: upcast[np.asarray(ids)]  # noqa: E731
        for top_p in (0.5, 1.0, 0.01):
            for top_k in (None, 3, 5):
                want = [O.query_literal(store, P, dim, queries[i], top_k=top_k, top_p=top_p, fetch=fetch) for i in sample]
                listed = idx.query_many(queries, top_k=top_k, top_p=top_p, corpus=corpus, engine="device")
                hosted = idx.query_many(queries[sample], top_k=top_k, top_p=top_p, corpus=corpus, engine="host")
                for j, i in enumerate(sample):
                    judged = dict(query=queries[i], candidates=lit_all[i], fetch=fetch)
                    judge_ranking(listed[i], want[j], **judged)
                    judge_ranking(hosted[j], want[j], **judged)
                for i in range(nq):
                    n_cand = len(lit_all[i])
                    lim = 0 if n_cand == 0 else max(1, math.ceil(n_cand * top_p))
                    assert len(listed[i]) == (min(lim, top_k) if top_k is not None else lim), (name, i)
                ids, scores, bounds = idx.query_many(queries, top_k=top_k, top_p=top_p, corpus=corpus, return_arrays=True)
                assert scores.dtype == np.float32 and len(ids) == len(scores) == bounds[-1]
                assert [list(zip(ids[bounds[i]:bounds[i + 1]].tolist(), scores[bounds[i]:bounds[i + 1]].astype(np.float64).tolist()))
                        for i in range(nq)] == listed, (name, top_k, top_p)


def _one_query_index(torch):
    from lshrs_amd import LSHRS, InMemoryStorage

    rng = np.random.default_rng(21)
    dim, n = 768, 3000
    data = _clustered(rng, n, dim, 150, 0.3)
    store = InMemoryStorage()
    idx = LSHRS(dim=dim, num_perm=256, storage=store, packed_ingest=True)
    idx.index(np.arange(1500), data[:1500])
    idx.index(np.arange(1500, n), data[1500:])
    queries = (data[rng.choice(n, 60, replace=False)] + 0.05 * rng.standard_normal((60, dim))).astype(np.float32)
    return idx, store, data, queries


def test_one_query_reranks_a_bf16_corpus_in_its_chain(monkeypatch):
    """`get_above_p` / `query` on a corpus attached in bf16 stay ONE chain (OneQuery): the host-counted path is made to fail."""
    torch = _torch()
    import lshrs_amd.core as core
    import lshrs_amd.similarity as similarity
    from oracle import lshrs_oracle as O

    idx, store, data, queries = _one_query_index(torch)
    corpus = torch.from_numpy(data).cuda().to(torch.bfloat16)
    upcast = corpus.float().cpu().numpy()
    fetch = lambda ids: upcast[np.asarray(ids)]  # noqa: E731

    def boom(*a, **k):
        raise AssertionError("the host-counted rerank was taken")

    monkeypatch.setattr(similarity, "rerank_batch", boom)
    monkeypatch.setattr(core, "top_k_cosine", boom)
    idx.set_corpus(corpus)
    P = idx._hasher.projections
    for v in queries:
        judged = dict(query=v, candidates=O.query_literal(store, P, 768, v, top_k=None), fetch=fetch)
        judge_ranking(idx.get_above_p(v, p=0.5), O.query_literal(store, P, 768, v, top_k=None, top_p=0.5, fetch=fetch), **judged)
        judge_ranking(idx.query(v, top_k=3, top_p=1.0), O.query_literal(store, P, 768, v, top_k=3, top_p=1.0, fetch=fetch), **judged)
    assert idx._one_query, "the single-query chain was not taken"


def test_errors_on_a_half_corpus_are_the_references():
    torch = _torch()
    from lshrs_amd import LSHRS, InMemoryStorage

    rng = np.random.default_rng(2)
    data = _clustered(rng, 600, 32, 30, 0.2)
    idx = LSHRS(dim=32, num_perm=16, storage=InMemoryStorage(), packed_ingest=True)
    idx.index(np.arange(600), data)
    q = data[400:408] + 0.01
    first = idx.query_many(q[:1], top_k=1)[0][0]
    for name in HALF:
        corpus = torch.from_numpy(data).cuda().to(getattr(torch, name))
        with pytest.raises(IndexError, match="out of range"):
            idx.query_many(q, top_k=None, top_p=1.0, corpus=corpus[:300])
        with pytest.raises(IndexError, match="out of range"):
            idx.query_many(q, top_k=None, top_p=1.0, corpus=corpus[:300], engine="host")
        dead = corpus.clone()
        dead[first] = 0
        with pytest.raises(ValueError, match="Cannot normalize zero vector"):
            idx.query_many(q[:1], top_k=None, top_p=1.0, corpus=dead)
        with pytest.raises(ValueError, match="Cannot normalize zero vector"):
            idx.query_many(q[:1], top_k=None, top_p=1.0, corpus=dead, engine="host")
    with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
        idx.query_many(q, top_k=None, top_p=0.5, corpus=torch.from_numpy(data).cuda().double())


def test_full_size_config3_on_a_bf16_corpus():
    """BASELINE config 3 with the corpus in bf16: 1M x 768 on the device, 10k queries x 1k candidates."""
    torch = _torch()
    from lshrs_amd import rerank_batch
    from lshrs_amd.similarity import cosine_scores_device

    gen = torch.Generator("cuda").manual_seed(7)
    corpus = torch.empty((1_000_000, 768), dtype=torch.bfloat16, device="cuda")
    for lo in range(0, 1_000_000, 250_000):
        corpus[lo:lo + 250_000] = torch.randn(250_000, 768, device="cuda", generator=gen)
    qrows = torch.randperm(1_000_000, device="cuda", generator=gen)[:10_000]
    queries = corpus[qrows].float() + 0.1 * torch.randn(10_000, 768, device="cuda", generator=gen)
    cidx = torch.randint(0, 1_000_000, (10_000, 1000), device="cuda", generator=gen)
    cidx[:, 17] = qrows
    order, scores = rerank_batch(queries, corpus, cidx, k=1000, return_tensors=True)
    assert order.shape == (10_000, 1000) and scores.shape == (10_000, 1000)
    assert bool((scores[:, :-1] >= scores[:, 1:]).all()), "not sorted"
    assert bool((order[:, 0] == 17).all()), "planted near-duplicate not ranked first"
    assert bool((scores[:, 0] > 0.99).all())
    assert bool((torch.sort(order.long(), dim=1).values == torch.arange(1000, device="cuda")).all()), "not a permutation"
    for qi in (0, 1234, 9999):
        s32, _, _ = cosine_scores_device(corpus[cidx[qi]].float(), queries[qi:qi + 1], None, c=1000)
        assert float((scores[qi] - s32[0][order[qi].long()]).abs().max()) <= 2e-6, qi
