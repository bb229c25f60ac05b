"""The rerank on a device corpus stored in int8 or OCP fp8 e4m3fn (lshrs_cosine_{batch,ragged}_{i8,f8e4m3}, cosine_kernel's
8-bit instantiations) and the quantizer that writes such a corpus (quantize_rows, lshrs_quantize_rows_*).  Every element is
converted to f32 exactly, so the scores are those of ``corpus.float()``: against the f32 kernel on the upcast, the float64
cosine, and the reference's flow restated literally (oracle.query_literal) with a fetch function that upcasts - the
reference reranks ``np.asarray(fetch(ids), dtype=np.float32)`` (lshrs/core/main.py:636)."""

from __future__ import annotations

import math

import numpy as np
import pytest

from tests._ranking import judge_ranking

pytestmark = pytest.mark.gpu
EIGHT = ("int8", "float8_e4m3fn")


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _clustered(rng, n, dim, clusters, spread):
    centers = rng.standard_normal((clusters, dim)).astype(np.float32)
    return (np.repeat(centers, n // clusters, axis=0) + spread * rng.standard_normal((n, dim))).astype(np.float32)


def _e4m3_values():
    """The 256 OCP e4m3fn codes decoded in float64 from the format's definition (bias 7, 3 mantissa bits, exponent 0
    subnormal, S.1111.111 NaN, no infinity)."""
    out = np.empty(256)
    for code in range(256):
        e, m = (code >> 3) & 15, code & 7
        v = math.nan if (e == 15 and m == 7) else (m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
        out[code] = -v if code & 0x80 else v
    return out


def _as_dtype(torch, codes_u8, name):
    """uint8 device tensor -> the same bytes as `name` (a view: no conversion)."""
    return codes_u8.view(torch.int8) if name == "int8" else codes_u8.view(torch.float8_e4m3fn)


def _random_codes(rng, name, shape):
    """Random codes over the whole range of the format (int8 -128 included; e4m3 without its two NaN codes)."""
    codes = rng.integers(0, 256, size=shape).astype(np.uint8)
    if name == "float8_e4m3fn":
        codes[(codes & 0x7F) == 0x7F] ^= 1            # NaN -> 448 / -448
    return codes


def _corpus(torch, name, codes, width=None, col=0):
    """(m, dim) codes -> device corpus of `name`; `width` > dim: the column slice [col, col + dim) of a wider tensor (row
    stride `width` bytes; col = 1 puts the base one byte past a 16-B boundary)."""
    m, dim = codes.shape
    if width is None:
        return _as_dtype(torch, torch.from_numpy(codes).cuda(), name)
    big = torch.zeros((m, width), dtype=torch.uint8, device="cuda")
    big[:, col:col + dim] = torch.from_numpy(codes).cuda()
    out = _as_dtype(torch, big, name)[:, col:col + dim]
    assert out.stride(0) == width and out.stride(1) == 1 and out.data_ptr() % 16 == col % 16
    return out


def _ragged(torch, lib, corpus, queries, idx):
    """The ragged entry of `corpus`'s dtype over the rows of `idx` as one list per query: (scores (q, c), err)."""
    from lshrs_amd import _native
    from lshrs_amd.similarity import corpus_entry

    q, c = (int(v) for v in idx.shape)
    entry = corpus_entry(corpus, "ragged")
    rows = idx.contiguous().reshape(-1)
    row_off = torch.arange(q, dtype=torch.int64, device="cuda") * c
    row_cnt = torch.full((q,), c, dtype=torch.int32, device="cuda")
    scores = torch.empty(q * c, dtype=torch.float32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    _native.check(getattr(lib, entry)(corpus.data_ptr(), int(corpus.shape[0]), int(corpus.stride(0)), int(corpus.shape[1]),
                                      queries.data_ptr(), q, rows.data_ptr(), row_off.data_ptr(), row_cnt.data_ptr(), q * c,
                                      scores.data_ptr(), err.data_ptr(), torch.cuda.current_stream().cuda_stream), entry)
    return scores.reshape(q, c), int(err.item())


def test_the_e4m3_table_is_the_format_and_torch_reads_it_so():
    """The float64 table the tests below use, against torch's own CPU decode of the 256 codes."""
    torch = _torch()
    want = _e4m3_values()
    got = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == 2
    assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
    assert want[0x7E] == 448 and want[0x01] == 2.0 ** -9 and want[0x08] == 2.0 ** -6


@pytest.mark.parametrize("name", EIGHT)
@pytest.mark.parametrize("dim,c,width,col", [(4, 7, None, 0), (15, 65, None, 0), (16, 300, None, 0), (17, 300, None, 0),
                                             (100, 1000, None, 0), (768, 1000, None, 0), (1536, 333, None, 0),
                                             (2050, 64, None, 0),
                                             (64, 300, 80, 0),        # ldc > dim, aligned
                                             (64, 300, 70, 0),        # ldc not a multiple of 16
                                             (64, 300, 80, 1)])       # base 1 byte past a 16-B boundary
def test_8bit_kernel_equals_f32_kernel_on_the_upcast(name, dim, c, width, col):
    torch = _torch()
    from oracle.build import cosine_f64

    from lshrs_amd import _native
    from lshrs_amd.similarity import cosine_scores_device

    lib = _native.load()
    m = c + 40
    rng = np.random.default_rng(dim * 7 + c + len(name))
    codes = _random_codes(rng, name, (m, dim))
    codes[3] = 0                                                             # zero rows
    codes[m - 1] = 0x80 if name == "float8_e4m3fn" else 0                    # (-0.0 everywhere: zero too)
    corpus = _corpus(torch, name, codes, width, col)
    q = 3
    queries = torch.from_numpy(rng.standard_normal((q, dim)).astype(np.float32)).cuda()
    queries[2] = 0                                                           # a zero query
    idx = torch.from_numpy(rng.integers(0, m, size=(q, c))).cuda()
    idx[0, 0], idx[0, 1] = 3, m - 1
    idx[1, 0] = -1
    idx[1, c - 1] = m                                                        # outside the corpus
    up = corpus.float()
    s8, st8, qs8 = cosine_scores_device(corpus, queries, idx)
    s32, st32, qs32 = cosine_scores_device(up, queries, idx)
    assert torch.equal(st8, st32) and torch.equal(qs8, qs32)
    assert st8[0, 0] == 1 and st8[0, 1] == 1 and st8[1, 0] == 2 and st8[1, c - 1] == 2 and qs8.tolist() == [0, 0, 1]
    ok = (st8 == 0) & (qs8 == 0)[:, None]
    assert torch.equal(torch.isnan(s8), ~ok)                                 # NaN exactly where a status is set
    assert float((s8[ok] - s32[ok]).abs().max()) <= 2e-6
    up_h, q_h, i_h = up.cpu().numpy(), queries.cpu().numpy(), idx.cpu().numpy()
    for qi in range(2):
        valid = ok[qi].cpu().numpy()
        want = cosine_f64(q_h[qi], up_h[i_h[qi][valid]])
        assert np.abs(s8[qi].cpu().numpy()[valid] - want).max() <= 2e-6, qi
    # the ragged form: the same lists as one list per query - the batch form's scores, the f32 ragged entry's err bits
    r8, err8 = _ragged(torch, lib, corpus, queries, idx)
    r32, err32 = _ragged(torch, lib, up, queries, idx)
    assert err8 == err32 == 7                                                # zero row, outside, zero query with candidates
    assert torch.equal(torch.isnan(r8), torch.isnan(s8)) and torch.equal(r8[ok], s8[ok])
    assert torch.equal(torch.isnan(r32), torch.isnan(r8)) and float((r8[ok] - r32[ok]).abs().max()) <= 2e-6


@pytest.mark.parametrize("name", EIGHT)
@pytest.mark.parametrize("dim", [16, 17])
def test_every_code_converts_exactly(name, dim):
    """All 256 codes, each in a row of its own beside a code for 1.0 within the same four elements: where a row's non-zeros
    share one group of four, the 8-bit kernel and the f32 kernel on the upcast add the same products in the same order (dim
    16: the 16-B path, every byte of the load; dim 17: the one-element path), so their scores agree BIT FOR BIT exactly
    when every code converts to its value.  The upcast is torch's CPU decode (itself checked against the format above)."""
    torch = _torch()
    from lshrs_amd.similarity import cosine_scores_device

    one = 0x38 if name == "float8_e4m3fn" else 1                             # (e4m3 0x38 = 1.0)
    codes = np.zeros((256, dim), dtype=np.uint8)
    for code in range(256):
        g, p = code % 4, (code // 4) % 4                                     # group (= dword of the load), byte within it
        codes[code, 4 * g + p] = code
        codes[code, 4 * g + (p + 1) % 4] = one
    corpus = _as_dtype(torch, torch.from_numpy(codes).cuda(), name)
    up = _as_dtype(torch, torch.from_numpy(codes), name).float().cuda()      # (decoded on the host)
    rng = np.random.default_rng(dim)
    queries = torch.from_numpy(rng.standard_normal((4, dim)).astype(np.float32)).cuda()
    idx = torch.arange(256, device="cuda").repeat(4, 1)
    s8, st8, _ = cosine_scores_device(corpus, queries, idx)
    s32, st32, _ = cosine_scores_device(up, queries, idx)
    assert torch.equal(st8, st32) and int(st8.max()) == 0
    a, b = s8.cpu().numpy(), s32.cpu().numpy()
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))
    nan_rows = [0x7F, 0xFF] if name == "float8_e4m3fn" else []
    assert sorted(set(np.nonzero(np.isnan(a))[1].tolist())) == nan_rows      # an e4m3 NaN scores NaN with status 0


def test_special_rows_score_their_true_cosine():
    """int8 rows holding -128 (a hand-made corpus may, quantize_rows never does); e4m3 rows of subnormals only (multiples of
    2^-9: a flush to zero would report a zero norm), rows at +-448, and a row holding a NaN code."""
    torch = _torch()
    from lshrs_amd.similarity import cosine_scores_device

    for dim in (64, 50):                                                     # the 16-B path and the one-element path
        rng = np.random.default_rng(dim)
        qh = rng.standard_normal((1, dim)).astype(np.float32)
        qd = torch.from_numpy(qh).cuda()
        q64 = qh[0].astype(np.float64)

        i8 = np.stack([np.full(dim, -128), np.where(np.arange(dim) % 2, -128, 127), rng.integers(-128, 128, dim),
                       np.r_[-128, np.zeros(dim - 1)]]).astype(np.int8)
        i8[2, dim // 2] = -128
        assert (i8 == -128).any(axis=1).all()
        s, st, _ = cosine_scores_device(torch.from_numpy(i8).cuda(), qd, None, c=4)
        assert st.tolist() == [[0, 0, 0, 0]]
        x = i8.astype(np.float64)
        want = x @ q64 / (np.linalg.norm(x, axis=1) * np.linalg.norm(q64))
        assert np.abs(s[0].cpu().numpy() - want).max() <= 2e-6

        table = _e4m3_values()
        sub = (rng.integers(1, 8, size=(3, dim)) | (rng.integers(0, 2, size=(3, dim)) << 7)).astype(np.uint8)   # e = 0
        top = np.where(rng.integers(0, 2, size=(2, dim)) == 1, 0x7E, 0xFE).astype(np.uint8)                   # +-448
        top[1, ::3] = 0x38                                                                                      # (and 1.0)
        f8 = np.concatenate([sub, top])
        vals = table[f8]
        assert (np.abs(vals[:3]) < 2.0 ** -6).all() and (np.abs(vals[3]) == 448).all()
        corpus = torch.from_numpy(f8).cuda().view(torch.float8_e4m3fn)
        s, st, _ = cosine_scores_device(corpus, qd, None, c=5)
        assert st.tolist() == [[0, 0, 0, 0, 0]]
        want = vals @ q64 / (np.linalg.norm(vals, axis=1) * np.linalg.norm(q64))
        assert np.abs(s[0].cpu().numpy() - want).max() <= 2e-6
        s32, st32, _ = cosine_scores_device(corpus.float(), qd, None, c=5)
        assert torch.equal(st, st32) and float((s - s32).abs().max()) <= 2e-6

        nan_row = f8[3:4].copy()
        nan_row[0, dim // 2] = 0x7F
        s, st, _ = cosine_scores_device(torch.from_numpy(nan_row).cuda().view(torch.float8_e4m3fn), qd, None, c=1)
        s32, st32, _ = cosine_scores_device(torch.from_numpy(nan_row).view(torch.float8_e4m3fn).float().cuda(), qd, None, c=1)
        assert st.tolist() == st32.tolist() == [[0]] and math.isnan(float(s[0, 0])) and math.isnan(float(s32[0, 0]))


def _quantize_reference(x: np.ndarray, name: str) -> np.ndarray:
    """quantize_rows restated in NumPy, step by step in float32: absmax, Q / absmax, multiply, round to nearest-even (int8:
    clamp to [-127, 127]; e4m3fn: torch's CPU cast, which rounds to nearest-even).  Zero rows stay zero."""
    import torch

    x = np.asarray(x, dtype=np.float32)
    q = np.float32(127.0 if name == "int8" else 448.0)
    absmax = np.abs(x).max(axis=1)
    out = np.zeros(x.shape, dtype=np.uint8)
    for r in np.nonzero(absmax != 0)[0]:
        s = q / absmax[r]
        assert s.dtype == np.float32
        y = x[r] * s
        assert y.dtype == np.float32
        if name == "int8":
            out[r] = np.clip(np.rint(y), -127, 127).astype(np.int8).view(np.uint8)
        else:
            out[r] = torch.from_numpy(y).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return out


def _quantize_inputs(dim):
    rng = np.random.default_rng(dim)
    rows = [rng.standard_normal((40, dim)) * rng.uniform(1e-3, 1e3, size=(40, 1)),     # Gaussian rows of many scales
            rng.uniform(-1, 1, (4, dim)) ** 7 * 10]                                   # mostly tiny, a few large elements
    ties_i8 = np.resize(np.array([0.5, 1.5, 2.5, -0.5, -2.5, 126.5, -126.5, 3.5, 64.5, -0.25]), dim)
    ties_i8[0] = 127                                                                  # absmax 127: s = 1, x * s = x
    ties_f8 = np.resize(np.array([1.0625, 1.1875, -1.0625, 2.0 ** -10, 3 * 2.0 ** -10, 15 * 2.0 ** -10, 432.0, -432.0,
                                  0.0078125 * 1.5, 24.0 + 1.0, 13.0]), dim)
    ties_f8[0] = -448                                                                 # absmax 448: s = 1
    one = np.zeros((2, dim))
    one[0, dim // 3] = -3.7                                                           # one non-zero element
    one[1, dim - 1] = 1e-30
    rows += [ties_i8[None], ties_f8[None], np.zeros((2, dim)), one]
    return np.concatenate(rows).astype(np.float32)


@pytest.mark.parametrize("name", EIGHT)
@pytest.mark.parametrize("dim", [100, 768, 17])
def test_quantize_rows_is_its_numpy_restatement_bit_for_bit(name, dim):
    torch = _torch()
    from lshrs_amd import quantize_rows

    x = _quantize_inputs(dim)
    dt = getattr(torch, name)
    got = quantize_rows(torch.from_numpy(x).cuda(), dt)
    assert got.dtype == dt and tuple(got.shape) == x.shape and got.is_cuda
    got_u8 = got.view(torch.uint8).cpu().numpy()
    want = _quantize_reference(x, name)
    assert np.array_equal(got_u8, want), np.argwhere(got_u8 != want)[:5]
    if name == "int8":
        assert (got_u8 != 0x80).all()                                         # -128 never written
        assert (np.abs(got.cpu().numpy().astype(np.int32)).max(axis=1)[:-4] == 127).all()
    else:
        assert ((got_u8 & 0x7F) != 0x7F).all()                                # never NaN
    assert (got_u8[-4:-2] == 0).all()                                         # the zero rows stay zero

    # strided input: a column slice of a wider tensor (row stride > dim) and a transposed one (inner stride != 1)
    wide = torch.zeros((x.shape[0], dim + 9), dtype=torch.float32, device="cuda")
    wide[:, 5:5 + dim] = torch.from_numpy(x).cuda()
    assert np.array_equal(quantize_rows(wide[:, 5:5 + dim], dt).view(torch.uint8).cpu().numpy(), want)
    tr = torch.from_numpy(np.ascontiguousarray(x.T)).cuda().t()
    assert tr.stride(1) != 1
    assert np.array_equal(quantize_rows(tr, dt).view(torch.uint8).cpu().numpy(), want)


@pytest.mark.parametrize("name", EIGHT)
def test_quantize_rows_refuses_what_it_cannot_scale(name):
    torch = _torch()
    from lshrs_amd import quantize_rows

    dt = getattr(torch, name)
    x = np.ones((5, 32), dtype=np.float32)
    for bad in (np.inf, -np.inf, np.nan):
        y = x.copy()
        y[3, 7] = bad
        with pytest.raises(ValueError, match="row 3"):
            quantize_rows(torch.from_numpy(y).cuda(), dt)
    with pytest.raises(TypeError):
        quantize_rows(torch.from_numpy(x).cuda().double(), dt)
    with pytest.raises(TypeError):
        quantize_rows(torch.from_numpy(x).cuda(), torch.float8_e5m2)
    assert quantize_rows(torch.empty((0, 32), device="cuda"), dt).shape == (0, 32)


@pytest.mark.parametrize("dim,num_perm,nb,r,n,clusters,spread", [
    (64, 64, 16, 4, 1500, 150, 0.35),
    (768, 256, 16, 16, 2000, 200, 0.3),
    (50, 40, 8, 5, 1000, 50, 0.3),
])
def test_query_many_on_an_8bit_corpus_equals_the_reference_flow(dim, num_perm, nb, r, n, clusters, spread):
    torch = _torch()
    from lshrs_amd import LSHRS, InMemoryStorage, quantize_rows
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
    for name in EIGHT:
        corpus = quantize_rows(torch.from_numpy(data).cuda(), getattr(torch, name))
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


@pytest.mark.parametrize("name", EIGHT)
def test_one_query_reranks_an_8bit_corpus_in_its_chain(monkeypatch, name):
    """`get_above_p` / `query` on a corpus attached in 8 bits stay ONE chain (OneQuery): the host-counted path is made to
    fail."""
    torch = _torch()
    import lshrs_amd.core as core
    import lshrs_amd.similarity as similarity
    from lshrs_amd import LSHRS, InMemoryStorage, quantize_rows
    from oracle import lshrs_oracle as O

    rng = np.random.default_rng(21)
    dim, n = 768, 3000
    data = _clustered(rng, n, dim, 150, 0.3)
    store = InMemoryStorage()
    idx = LSHRS(dim=dim, num_perm=256, storage=store, packed_ingest=True)
    idx.index(np.arange(1500), data[:1500])
    idx.index(np.arange(1500, n), data[1500:])
    queries = (data[rng.choice(n, 60, replace=False)] + 0.05 * rng.standard_normal((60, dim))).astype(np.float32)
    corpus = quantize_rows(torch.from_numpy(data).cuda(), getattr(torch, name))
    upcast = corpus.float().cpu().numpy()
    fetch = lambda ids: upcast[np.asarray(ids)]  # noqa: E731

    def boom(*a, **k):
        raise AssertionError("the host-counted rerank was taken")

    monkeypatch.setattr(similarity, "rerank_batch", boom)
    monkeypatch.setattr(core, "top_k_cosine", boom)
    idx.set_corpus(corpus)
    P = idx._hasher.projections
    for v in queries:
        judged = dict(query=v, candidates=O.query_literal(store, P, dim, v, top_k=None), fetch=fetch)
        judge_ranking(idx.get_above_p(v, p=0.5), O.query_literal(store, P, dim, v, top_k=None, top_p=0.5, fetch=fetch), **judged)
        judge_ranking(idx.query(v, top_k=3, top_p=1.0), O.query_literal(store, P, dim, v, top_k=3, top_p=1.0, fetch=fetch), **judged)
    assert idx._one_query, "the single-query chain was not taken"


def test_errors_on_an_8bit_corpus_are_the_references():
    torch = _torch()
    from lshrs_amd import LSHRS, InMemoryStorage, quantize_rows

    rng = np.random.default_rng(2)
    data = _clustered(rng, 600, 32, 30, 0.2)
    idx = LSHRS(dim=32, num_perm=16, storage=InMemoryStorage(), packed_ingest=True)
    idx.index(np.arange(600), data)
    q = data[400:408] + 0.01
    first = idx.query_many(q[:1], top_k=1)[0][0]
    for name in EIGHT:
        corpus = quantize_rows(torch.from_numpy(data).cuda(), getattr(torch, name))
        with pytest.raises(IndexError, match="out of range"):
            idx.query_many(q, top_k=None, top_p=1.0, corpus=corpus[:300])
        with pytest.raises(IndexError, match="out of range"):
            idx.query_many(q, top_k=None, top_p=1.0, corpus=corpus[:300], engine="host")
        dead = corpus.clone()
        dead.view(torch.uint8)[first] = 0
        with pytest.raises(ValueError, match="Cannot normalize zero vector"):
            idx.query_many(q[:1], top_k=None, top_p=1.0, corpus=dead)
        with pytest.raises(ValueError, match="Cannot normalize zero vector"):
            idx.query_many(q[:1], top_k=None, top_p=1.0, corpus=dead, engine="host")
    raw = torch.from_numpy(data).cuda().to(torch.bfloat16).view(torch.uint8)[:, :32]      # (any 600 x 32 bytes)
    for other in (torch.float8_e5m2, torch.float8_e4m3fnuz, torch.uint8):
        with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
            idx.query_many(q, top_k=None, top_p=0.5, corpus=raw.contiguous().view(other))


@pytest.mark.parametrize("name", EIGHT)
def test_full_size_config3_on_an_8bit_corpus(name):
    """BASELINE config 3 with the corpus quantized: 1M x 768 on the device, 10k queries x 1k candidates."""
    torch = _torch()
    from lshrs_amd import quantize_rows, rerank_batch
    from lshrs_amd.similarity import cosine_scores_device

    dt = getattr(torch, name)
    rows = lambda i: corpus.view(torch.uint8)[i].view(dt).float()  # noqa: E731 - (gathered as bytes, then upcast)
    gen = torch.Generator("cuda").manual_seed(7)
    corpus = torch.empty((1_000_000, 768), dtype=dt, device="cuda")
    for lo in range(0, 1_000_000, 250_000):
        part = quantize_rows(torch.randn(250_000, 768, device="cuda", generator=gen), dt)
        corpus.view(torch.uint8)[lo:lo + 250_000] = part.view(torch.uint8)
    qrows = torch.randperm(1_000_000, device="cuda", generator=gen)[:10_000]
    near = rows(qrows)
    queries = near + 0.1 * near.abs().mean() * torch.randn(10_000, 768, device="cuda", generator=gen)
    cidx = torch.randint(0, 1_000_000, (10_000, 1000), device="cuda", generator=gen)
    cidx[:, 17] = qrows
    order, scores = rerank_batch(queries, corpus, cidx, k=1000, return_tensors=True)
    assert order.shape == (10_000, 1000) and scores.shape == (10_000, 1000)
    assert bool((scores[:, :-1] >= scores[:, 1:]).all()), "not sorted"
    assert bool((order[:, 0] == 17).all()), "planted near-duplicate not ranked first"
    assert bool((scores[:, 0] > 0.99).all())
    assert bool((torch.sort(order.long(), dim=1).values == torch.arange(1000, device="cuda")).all()), "not a permutation"
    for qi in (0, 1234, 9999):
        s32, _, _ = cosine_scores_device(rows(cidx[qi]), queries[qi:qi + 1], None, c=1000)
        assert float((scores[qi] - s32[0][order[qi].long()]).abs().max()) <= 2e-6, qi
