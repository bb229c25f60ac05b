"""Pin the CPU oracle to the reference-generated goldens (tests/golden, made by make_golden.py
from the real upstream modules).  CPU only.

Where NumPy's BLAS rounds like the one that made the goldens (its fingerprint is stored beside
them, g2_blas_fingerprint.json) every row must match; on a foreign CPU the BLAS summation order
may differ, so rows whose smallest |projection| is inside float32 rounding noise are exempt there
(their margin is stored with the fixture).
"""

from __future__ import annotations

import hashlib
import json
import os

import numpy as np
import pytest

from oracle import lshrs_oracle as O

SHAPES = [
    (42, 16, 4, 128, 101), (42, 16, 16, 768, 102), (7, 16, 32, 1536, 103), (123, 3, 5, 4, 104),
    (42, 4, 12, 32, 105), (5, 2, 24, 100, 106), (9, 5, 8, 30, 107),
]


def blas_fingerprint() -> dict:
    """sha256 of what this process's NumPy returns for ``plane @ x`` - the reference's call - at every (rows, dim) of SHAPES,
    on seeded vectors and on vectors built to cancel against a row (where the summation order shows)."""
    out = {}
    for _, _, r, dim, _ in SHAPES:
        rng = np.random.default_rng(20240601 + 7 * r + dim)
        plane = rng.standard_normal((r, dim)).astype(np.float32)
        h = hashlib.sha256()
        for i in range(64):
            x = rng.standard_normal(dim)
            if i % 2:
                p = plane[i % r].astype(np.float64)
                x = x - (x @ p) / (p @ p) * p
            h.update((plane @ np.ascontiguousarray(x, dtype=np.float32)).tobytes())
        out[f"r{r}_d{dim}"] = h.hexdigest()
    return out


def same_blas_as_goldens(golden_dir) -> bool:
    """Does this host's BLAS round like the one that made the goldens?  (Then every g2 row must match.)"""
    with open(os.path.join(golden_dir, "g2_blas_fingerprint.json")) as fh:
        return json.load(fh)["plane_at_x_sha256"] == blas_fingerprint()


def test_g1_projection_stream(golden_dir):
    for rec in json.load(open(os.path.join(golden_dir, "g1_projections.json"))):
        planes = O.make_projections(rec["num_bands"], rec["rows_per_band"], rec["dim"], rec["seed"])
        stacked = np.concatenate(planes, axis=0)
        assert stacked.dtype == np.float32 and all(p.flags.c_contiguous for p in planes)
        assert stacked.reshape(-1)[:8].tobytes().hex() == rec["first8_hex"]
        assert hashlib.sha256(stacked.tobytes()).hexdigest() == rec["sha256"]
        # stream continuity: num_bands draws == one (num_perm, dim) draw
        one = np.random.default_rng(rec["seed"]).standard_normal(stacked.shape).astype(np.float32)
        assert np.array_equal(one, stacked)


@pytest.mark.parametrize("seed,nb,r,dim,dseed", SHAPES)
def test_g2_signatures(golden_dir, seed, nb, r, dim, dseed):
    g = np.load(os.path.join(golden_dir, "g2_signatures.npz"))
    tag = f"s{seed}_b{nb}_r{r}_d{dim}_x{dseed}"
    want, margin = g[tag + "_keys"], g[tag + "_minabs"]
    planes = O.make_projections(nb, r, dim, seed)
    x = np.random.default_rng(dseed).standard_normal((256, dim)).astype(np.float32)
    got = O.hash_batch_literal_packed(planes, x)
    assert got.shape == want.shape == (256, nb, (r + 7) // 8)
    rows = np.ones(256, bool) if same_blas_as_goldens(golden_dir) else margin >= 1e-3
    assert np.array_equal(got[rows], want[rows])
    # single-vector and batch forms agree; tail bits of the last byte are zero
    for i in (0, 100, 255):
        assert O.hash_vector_literal(planes, x[i], dim) == tuple(bytes(got[i, b]) for b in range(nb))
    if r % 8:
        assert not (got[:, :, -1] >> (r % 8)).any()
    # margins are what they claim: f64 projections
    assert np.allclose(np.abs(O.exact_projection_f64(planes, x)).min(axis=1), margin, rtol=1e-9, atol=1e-12)


def test_g3_special_values(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "g3_specials.json")))
    planes = [np.array(p, dtype=np.float32) for p in g["projections"]]
    for case in g["cases"]:
        x = np.frombuffer(bytes.fromhex(case["x_hex"]), dtype=np.float32)
        with np.errstate(all="ignore"):
            got = [k.hex() for k in O.hash_vector_literal(planes, x, 4)]
        assert got == case["keys_hex"], case["name"]


def test_g4_cosine(golden_dir):
    g = np.load(os.path.join(golden_dir, "g4_cosine.npz"))
    j = json.load(open(os.path.join(golden_dir, "g4_cosine.json")))
    rng = np.random.default_rng(201)
    q = rng.standard_normal(768).astype(np.float32)
    cands = rng.standard_normal((64, 768)).astype(np.float32)
    cands[5] = q * 3.0
    cands[9] = -q
    cands[11] = cands[12]
    s = O.cosine_similarity(q, cands)
    assert s.dtype == np.float32
    assert np.allclose(s, g["scores_q201_c64"], atol=1e-6, rtol=0)
    for k, want in j["topk"].items():
        got = O.top_k_cosine(q, cands, k=int(k))
        assert len(got) == len(want) == min(int(k), 64)
        assert np.allclose([v for _, v in got], [v for _, v in want], atol=1e-6)
        # positions agree except inside the deliberate tie pair (11, 12)
        gi, wi = [i for i, _ in got], [i for i, _ in want]
        assert all(a == b or {a, b} == {11, 12} for a, b in zip(gi, wi))
    q3 = np.array([1.0, 0.0, 0.0], dtype=np.float32)
    c4 = [np.array(v, dtype=np.float32) for v in ([1, 0, 0], [0, 1, 0], [-1, 0, 0], [1, 1, 0])]
    assert np.allclose(O.cosine_similarity(q3, c4), j["ref_test_cosine"], atol=1e-7)
    assert np.allclose(O.cosine_similarity(q3, c4), [1.0, 0.0, -1.0, 0.70710677], atol=1e-6)
    c5 = [np.array(v, dtype=np.float32) for v in ([1, .1, 0], [0, 1, 0], [1, 0, 0], [-1, 0, 0], [.9, .2, 0])]
    top3 = O.top_k_cosine(q3, c5, k=3)
    assert [i for i, _ in top3] == [2, 0, 4] == [i for i, _ in j["ref_test_topk3"]]
    assert len(O.top_k_cosine(q3, c5, k=10)) == j["ref_test_topk10_len"] == 5
    with pytest.raises(ValueError):
        O.top_k_cosine(q3, c5, k=0)
    with pytest.raises(ValueError):
        O.l2_norm(np.zeros(4, dtype=np.float32))
    with pytest.raises(ValueError):
        O.cosine_similarity(q3, [])  # np.stack([]) — observed reference behaviour
    u = O.l2_norm(np.array([3.0, 4.0, 0.0]))
    assert u.dtype == np.float32 and np.allclose(u, [0.6, 0.8, 0.0])
    # batched form
    rng = np.random.default_rng(202)
    corpus = rng.standard_normal((500, 32)).astype(np.float32)
    queries = rng.standard_normal((6, 32)).astype(np.float32)
    cidx = rng.integers(0, 500, size=(6, 40))
    got = O.rerank_batch(queries, corpus, cidx, k=40)
    for i in range(6):
        assert np.allclose(O.cosine_similarity(queries[i], corpus[cidx[i]]), g["batch_scores_202"][i], atol=1e-6)
        assert np.allclose([v for _, v in got[i]], [v for _, v in j["batch_topk_202"][i]], atol=1e-6)


def test_g6_autoconfig_matches_reference(golden_dir):
    from lshrs_amd.bandrows import get_optimal_config

    table = json.load(open(os.path.join(golden_dir, "g6_autoconfig.json")))
    for key, want in table.items():
        n, t = key.split(":")
        assert list(get_optimal_config(int(n), float(t))) == want, key
    assert get_optimal_config(64, 0.5) == (16, 4)       # BASELINE config 1
    assert get_optimal_config(256, 0.5) == (16, 16)     # configs 2-4
    assert get_optimal_config(512, 0.5) == (16, 32)     # config 5
    assert get_optimal_config(4096, 0.9) == (64, 64)    # reference tests/test_lshrs.py
    assert get_optimal_config(97, 0.5) == (1, 97)       # prime: most-square fallback


def test_prepare_vector_and_zero_rows():
    with pytest.raises(ValueError, match="dimension"):
        O.prepare_vector(np.ones(5), 4)
    with pytest.raises(ValueError, match="zero vector"):
        O.prepare_vector(np.full(4, 1e-9), 4)
    assert O.prepare_vector([1, 0, 0, 0], 4).dtype == np.float32
    x = np.zeros((5, 4), dtype=np.float32)
    x[1, 2] = 2e-8
    x[2] = 1e-8
    x[3, 0] = np.nan
    x[4] = -9e-9
    assert O.is_zero_vector_rows(x).tolist() == [True, False, True, False, True]


def test_chain_model_agrees_with_blas_up_to_rounding():
    """The BLAS-free fmaf-chain model and the NumPy literal path are two roundings of the same
    dot products: identical signs except where |y| is inside float32 noise."""
    from oracle.build import chain_hash_packed, chain_project

    planes = O.make_projections(16, 16, 768, 42)
    x = np.random.default_rng(7).standard_normal((512, 768)).astype(np.float32)
    y = chain_project(planes, x)
    y64 = O.exact_projection_f64(planes, x)
    assert np.abs(y - y64).max() < 1e-3
    a, b = chain_hash_packed(planes, x), O.hash_batch_literal_packed(planes, x)
    diff_rows = (a != b).any(axis=(1, 2))
    assert (np.abs(y64).min(axis=1)[diff_rows] < 1e-3).all()
    assert diff_rows.sum() <= 2


def g8_inputs():
    rng8 = np.random.default_rng(801)
    centers = rng8.standard_normal((300, 768)).astype(np.float32)
    data = (np.repeat(centers, 10, axis=0) + 0.3 * rng8.standard_normal((3000, 768))).astype(np.float32)
    qrows = rng8.choice(3000, 100, replace=False)
    queries = (data[qrows] + 0.05 * rng8.standard_normal((100, 768))).astype(np.float32)
    return data, qrows, queries


def test_g8_queries_at_768d(golden_dir):
    """The oracle's restatement of index() + query() against what the reference itself answered for 100 queries on
    3 000 clustered 768-d vectors (tests/golden/make_golden.py, G8) - the pin of SURVEY §8f-2's path."""
    import hashlib

    from lshrs_amd import InMemoryStorage

    g8 = json.load(open(os.path.join(golden_dir, "g8_queries_768.json")))
    data, qrows, queries = g8_inputs()
    assert [int(v) for v in qrows] == g8["query_rows"]
    P = O.make_projections(g8["num_bands"], g8["rows_per_band"], 768, 42)
    store = InMemoryStorage()
    O.index_literal(store, list(range(3000)), data, P, 768, 10_000)
    h = hashlib.sha256()
    for batch in store.batches:
        for b, k, i in batch:
            h.update(bytes([b]) + k + int(i).to_bytes(4, "little"))
    if h.hexdigest() != g8["ops_sha256"]:
        pytest.skip("this CPU's BLAS rounds a near-zero projection of the g8 data differently from the build container's")
    fetch = lambda ids: data[np.asarray(ids)]  # noqa: E731
    for qi, q in enumerate(queries):
        assert O.query_literal(store, P, 768, q, top_k=10) == g8["top_k_10"][qi]
        assert O.query_literal(store, P, 768, q, top_k=None) == g8["top_k_all"][qi]
        got = O.query_literal(store, P, 768, q, top_k=None, top_p=0.5, fetch=fetch)
        assert [i for i, _ in got] == [i for i, _ in g8["above_p_half"][qi]]
        assert np.abs(np.array([s for _, s in got]) - np.array([s for _, s in g8["above_p_half"][qi]])).max() <= 1e-6
        got = O.query_literal(store, P, 768, q, top_k=3, top_p=1.0, fetch=fetch)
        assert [i for i, _ in got] == [i for i, _ in g8["topk3_topp1"][qi]]
