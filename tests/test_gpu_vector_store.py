"""``DeviceVectors`` - the indexed vectors on the GPU under the caller's own ids (csrc/idmap.hip: the id -> row table) - and
what ``LSHRS`` does with it: ``set_corpus`` / ``query_many(corpus=)`` take one, ``keep_vectors=`` makes the index fill one.
The table against a Python dict; the queries against the plain device-corpus path (bit for bit: same kernel, same rows)
and against the reference's flow restated literally (oracle.query_literal) with a fetch function that returns each id's
latest stored row, upcast."""

from __future__ import annotations

import numpy as np
import pytest

from tests._ranking import judge_ranking

pytestmark = pytest.mark.gpu
DTYPES = ("float32", "bfloat16", "float16", "int8", "float8_e4m3fn")


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _clustered(rng, n, dim, clusters, spread):
    centers = rng.standard_normal((clusters, dim)).astype(np.float32)
    return (np.repeat(centers, n // clusters, axis=0) + spread * rng.standard_normal((n, dim))).astype(np.float32)


def _stored_form(torch, name, x):
    """float32 rows (host array or device tensor) as a device tensor of dtype `name`, made WITHOUT the store: torch's cast
    for 16 bits, quantize_rows for 8."""
    from lshrs_amd import quantize_rows

    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    if name == "float32":
        return xd.clone()
    if name in ("int8", "float8_e4m3fn"):
        return quantize_rows(xd, getattr(torch, name))
    return xd.to(getattr(torch, name))


def _raw(torch, t):
    """The bytes of a (n, dim) tensor as a host uint8 array (n, dim * itemsize)."""
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _random_ids(rng, n, bits=40):
    ids = np.unique(rng.integers(0, 1 << bits, size=n + n // 4 + 16, dtype=np.int64))
    assert ids.shape[0] >= n
    return np.sort(rng.choice(ids, n, replace=False))


# ------------------------------------------------------------------------------------------ the map against a dict
@pytest.mark.parametrize("reserve", [0, 700])
@pytest.mark.parametrize("name", DTYPES)
def test_the_map_against_a_dict(name, reserve):
    torch = _torch()
    from lshrs_amd import DeviceVectors

    rng = np.random.default_rng(DTYPES.index(name) * 2 + (reserve > 0))
    dim = 32
    pool = np.concatenate([_random_ids(rng, 4000, 40), (1 << 58) + _random_ids(rng, 3000, 40)])
    never = np.concatenate([_random_ids(rng, 300, 39) + (1 << 41), np.array([0, 1, (1 << 62) + 5])])
    never = np.setdiff1d(never, pool)
    store = DeviceVectors(dim, name)
    if reserve:
        store.reserve(reserve)
        assert store.stats()["capacity"] >= reserve and store.stats()["slots"] >= 2 * reserve
    model: dict = {}                       # id -> latest row
    expect = np.empty((0, dim * store.rows.element_size()), dtype=np.uint8)      # expected bytes of every row in use
    removed: set = set()
    slots_seen, caps_seen = [store.stats()["slots"]], [store.stats()["capacity"]]

    def check():
        assert len(store) == len(model)
        st = store.stats()
        assert st["live"] == len(model) and st["rows"] == expect.shape[0] and st["dead"] == st["rows"] - st["live"]
        present = np.array(list(model), dtype=np.int64)
        probe = np.concatenate([rng.choice(present, min(len(present), 400), replace=False) if len(present) else present,
                                np.array(sorted(removed), dtype=np.int64)[:200], never])
        rng.shuffle(probe)
        rows = store.rows_of(probe).cpu().numpy()
        want = np.array([model.get(int(i), -1) for i in probe], dtype=np.int64)
        assert np.array_equal(rows, want)
        hit = rows >= 0
        if hit.any():
            got = store.rows.view(torch.uint8)[torch.from_numpy(rows[hit]).cuda()].cpu().numpy()
            assert np.array_equal(got, expect[rows[hit]])
        for i in probe[:3]:
            assert (int(i) in store) == (int(i) in model)
        if st["slots"] != slots_seen[-1]:
            slots_seen.append(st["slots"])
        if st["capacity"] != caps_seen[-1]:
            caps_seen.append(st["capacity"])

    check()
    for step in range(26):
        kind = "add" if step < 3 or step % 5 not in (3, 4) else ("remove" if step % 5 == 3 else "compact")
        if kind == "add":
            k = int(rng.integers(1, 1500))
            hi = min(pool.shape[0], 600 * (step + 1))                     # the pool opens up: new ids AND re-adds
            ids = rng.choice(pool[:hi], k, replace=True)                  # repeats inside the call
            x = rng.standard_normal((k, dim)).astype(np.float32)
            base = expect.shape[0]
            given = torch.from_numpy(x).cuda() if step % 2 else x         # a device tensor or a host array
            store.add(ids if step % 3 else ids.tolist(), given)
            expect = np.concatenate([expect, _raw(torch, _stored_form(torch, name, x))])
            for j, i in enumerate(ids.tolist()):
                model[i] = base + j
                removed.discard(i)
        elif kind == "remove":
            present = np.array(list(model), dtype=np.int64)
            gone = rng.choice(present, len(present) // 4, replace=False)
            listed = np.concatenate([gone, gone[:5], never[:5]])           # twice listed, never there
            assert store.remove(listed) == len(gone)
            for i in gone.tolist():
                del model[i]
                removed.add(i)
        else:
            order = sorted(model.items(), key=lambda kv: kv[1])
            expect = expect[[r for _, r in order]] if order else expect[:0]
            model = {i: j for j, (i, _) in enumerate(order)}
            store.compact()
            assert store.stats()["dead"] == 0
        check()
    grew = [b for a, b in zip(slots_seen, slots_seen[1:]) if b > a]
    assert len(grew) >= 3, slots_seen                                       # three doublings of the table ...
    assert len([b for a, b in zip(caps_seen, caps_seen[1:]) if b > a]) >= 3, caps_seen      # ... and of the row block
    store.clear()
    assert len(store) == 0 and store.stats()["slots"] == 0
    assert bool((store.rows_of(pool[:50]) == -1).all())


def test_a_bad_row_adds_nothing():
    _torch()
    from lshrs_amd import DeviceVectors

    store = DeviceVectors(16, "int8")
    x = np.ones((6, 16), dtype=np.float32)
    store.add([10, 11], x[:2])
    x[3, 2] = np.inf
    with pytest.raises(ValueError, match="row 3"):
        store.add([20, 21, 22, 23, 24, 25], x)
    with pytest.raises(ValueError, match="non-negative"):
        store.add([30, -1], x[:2])
    assert len(store) == 2 and store.stats()["rows"] == 2
    assert store.rows_of([10, 11, 20, 23, 30]).cpu().tolist() == [0, 1, -1, -1, -1]


def test_a_table_with_no_free_slot_answers_and_returns():
    """The bounded-probe condition through the raw ABI: 8 slots, 9 distinct ids."""
    torch = _torch()
    from lshrs_amd import _native

    lib = _native.load()
    stream = torch.cuda.current_stream().cuda_stream
    ids = torch.tensor([3, 1 << 40, 17, 5, (1 << 58) + 1, 8, 64, 2, 99], dtype=torch.int64, device="cuda")

    def lookup(table, what):
        rows = torch.full((what.numel(),), -7, dtype=torch.int64, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert lib.lshrs_idmap_lookup_i64(table.data_ptr(), 8, what.data_ptr(), what.numel(), rows.data_ptr(), err.data_ptr(),
                                          stream) == 0
        return rows.cpu().tolist(), int(err.item())

    # eight, then the ninth: which one finds no slot is decided
    table = torch.full((8, 2), -1, dtype=torch.int64, device="cuda")
    report = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert lib.lshrs_idmap_insert_i64(table.data_ptr(), 8, ids.data_ptr(), 8, 100, report.data_ptr(), stream) == 0
    assert report.cpu().tolist() == [8, 8, 0, 0]
    report.zero_()
    assert lib.lshrs_idmap_insert_i64(table.data_ptr(), 8, ids[8:].data_ptr(), 1, 108, report.data_ptr(), stream) == 0
    assert report.cpu().tolist() == [0, 0, 0, 1]                     # the "full" flag, nothing taken
    rows, err = lookup(table, ids)
    assert rows == [100, 101, 102, 103, 104, 105, 106, 107, -1] and err == 256
    rows, err = lookup(table, ids[:8])
    assert err == 0
    absent = torch.tensor([1000, 7, (1 << 61) + 3, -5], dtype=torch.int64, device="cuda")
    assert lookup(table, absent) == ([-1, -1, -1, -1], 256)           # a full table, ids that are not in it: it answers
    # erase in a full table, then the id again: its slot is still its own
    live = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.lshrs_idmap_erase_i64(table.data_ptr(), 8, ids[2:4].data_ptr(), 2, live.data_ptr(), stream) == 0
    assert int(live.item()) == 2 and lookup(table, ids[:4])[0] == [100, 101, -1, -1]
    report.zero_()
    assert lib.lshrs_idmap_insert_i64(table.data_ptr(), 8, ids[2:3].data_ptr(), 1, 200, report.data_ptr(), stream) == 0
    assert report.cpu().tolist() == [0, 1, 0, 0] and lookup(table, ids[:4])[0] == [100, 101, 200, -1]
    # all nine in ONE call: eight of them get in, whichever they are, and the call says so
    table2 = torch.full((8, 2), -1, dtype=torch.int64, device="cuda")
    report.zero_()
    assert lib.lshrs_idmap_insert_i64(table2.data_ptr(), 8, ids.data_ptr(), 9, 0, report.data_ptr(), stream) == 0
    assert report.cpu().tolist() == [8, 8, 0, 1]
    rows, err = lookup(table2, ids)
    assert sorted(r for r in rows if r >= 0) == sorted(set(range(9)) - {rows.index(-1)}) and rows.count(-1) == 1 and err == 256
    # a negative id is reported and skipped
    table3 = torch.full((8, 2), -1, dtype=torch.int64, device="cuda")
    report.zero_()
    neg = torch.tensor([4, -1, 6], dtype=torch.int64, device="cuda")
    assert lib.lshrs_idmap_insert_i64(table3.data_ptr(), 8, neg.data_ptr(), 3, 0, report.data_ptr(), stream) == 0
    assert report.cpu().tolist() == [2, 2, 1, 0] and lookup(table3, neg)[0] == [0, -1, 2]
    # rehash into a larger table: the live entries, their rows
    table4 = torch.full((32, 2), -1, dtype=torch.int64, device="cuda")
    report.zero_()
    assert lib.lshrs_idmap_rehash(table.data_ptr(), 8, table4.data_ptr(), 32, report.data_ptr(), stream) == 0
    assert report.cpu().tolist() == [7, 7, 0, 0]
    rows = torch.empty(9, dtype=torch.int64, device="cuda")
    assert lib.lshrs_idmap_lookup_i64(table4.data_ptr(), 32, ids.data_ptr(), 9, rows.data_ptr(), None, stream) == 0
    assert rows.cpu().tolist() == [100, 101, 200, -1, 104, 105, 106, 107, -1]


# ------------------------------------------------------------------------------------------ queries: the plain path
def _plain_index(n, dim, num_perm, rng, **kw):
    from lshrs_amd import LSHRS, InMemoryStorage

    data = _clustered(rng, n, dim, n // 10, 0.3)
    idx = LSHRS(dim=dim, num_perm=num_perm, storage=InMemoryStorage(), packed_ingest=True, seed=42, **kw)
    return idx, data


@pytest.mark.parametrize("name", DTYPES)
def test_exactly_the_plain_path_when_ids_are_rows(name):
    torch = _torch()
    from lshrs_amd import DeviceVectors

    rng = np.random.default_rng(31)
    n, dim = 2000, 64
    idx, data = _plain_index(n, dim, 64, rng)
    idx.index(np.arange(n // 2), data[:n // 2])
    idx.index(np.arange(n // 2, n), data[n // 2:])
    queries = (data[rng.choice(n, 200, replace=False)] + 0.05 * rng.standard_normal((200, dim))).astype(np.float32)
    plain = _stored_form(torch, name, data)
    store = DeviceVectors(dim, name)
    store.add(np.arange(n), data)
    assert np.array_equal(_raw(torch, store.rows), _raw(torch, plain))
    for engine in ("device", "host"):
        for top_k in (None, 3):
            for top_p in (0.5, 1.0, 0.01):
                a = idx.query_many(queries, top_k=top_k, top_p=top_p, corpus=plain, return_arrays=True, engine=engine)
                b = idx.query_many(queries, top_k=top_k, top_p=top_p, corpus=store, return_arrays=True, engine=engine)
                assert len(a[0]) > 0
                for x, y in zip(a, b):
                    assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (engine, top_k, top_p)
    idx.set_corpus(store)
    a = idx.query_many(queries, top_k=None, top_p=0.5, corpus=plain, return_arrays=True)
    b = idx.query_many(queries, top_k=None, top_p=0.5, return_arrays=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", DTYPES)
def test_exactly_the_plain_path_under_renamed_ids(name):
    """new_id = sorted_random_40bit[i]: an increasing renaming keeps the (-collisions, id) order, so the answers are those
    of the un-renamed index on the plain corpus - renamed ids, the same scores and bounds bit for bit."""
    torch = _torch()
    from lshrs_amd import LSHRS, InMemoryStorage

    rng = np.random.default_rng(32)
    n, dim = 3000, 64
    idx, data = _plain_index(n, dim, 64, rng)
    idx.index(np.arange(n), data)
    new_id = _random_ids(rng, n, 40)
    kept = LSHRS(dim=dim, num_perm=64, storage=InMemoryStorage(), packed_ingest=True, seed=42, keep_vectors=name)
    batches = np.array_split(np.arange(n), 6)
    for b in rng.permutation(6):                                    # shuffled batches: row != rank of the id
        kept.index(new_id[batches[b]], data[batches[b]])
    assert len(kept.vectors) == n
    rows = kept.vectors.rows_of(new_id).cpu().numpy()
    assert not np.array_equal(rows, np.arange(n)) and np.array_equal(np.sort(rows), np.arange(n))
    queries = (data[rng.choice(n, 200, replace=False)] + 0.05 * rng.standard_normal((200, dim))).astype(np.float32)
    plain = _stored_form(torch, name, data)
    for engine in ("device", "host"):
        for top_k, top_p in ((None, 0.5), (3, 1.0), (None, 0.01)):
            ids, scores, bounds = idx.query_many(queries, top_k=top_k, top_p=top_p, corpus=plain, return_arrays=True, engine=engine)
            rids, rscores, rbounds = kept.query_many(queries, top_k=top_k, top_p=top_p, return_arrays=True, engine=engine)
            assert len(ids) > 0 and np.array_equal(new_id[ids], rids)
            assert np.array_equal(scores.view(np.uint32), rscores.view(np.uint32)) and np.array_equal(bounds, rbounds)


# ------------------------------------------------------------------------------------------ queries: the reference's flow
class _Latest:
    """Host model of what the store must hold: id -> latest vector, and the fetch function of the reference's flow (each
    id's latest row in the store's dtype, upcast to float32)."""

    def __init__(self, torch, name, dim):
        self.torch, self.name, self.dim, self.vec = torch, name, dim, {}

    def put(self, ids, x):
        up = _stored_form(self.torch, self.name, x).float().cpu().numpy()
        for i, row in zip(np.asarray(ids).tolist(), up):
            self.vec[int(i)] = row

    def drop(self, ids):
        for i in np.asarray(ids).tolist():
            self.vec.pop(int(i), None)

    def fetch(self, ids):
        return np.stack([self.vec[int(i)] for i in ids]) if len(ids) else np.empty((0, self.dim), np.float32)


@pytest.mark.parametrize("dim,num_perm,nb,r,n,clusters,spread,names", [
    (64, 64, 16, 4, 1500, 150, 0.35, ("float32", "int8")),
    (768, 256, 16, 16, 2000, 200, 0.3, ("bfloat16", "float8_e4m3fn")),
    (50, 40, 8, 5, 1000, 50, 0.3, ("float16", "int8")),
])
def test_the_reference_flow_is_the_judge(dim, num_perm, nb, r, n, clusters, spread, names):
    torch = _torch()
    from lshrs_amd import LSHRS, InMemoryStorage
    from oracle import lshrs_oracle as O

    for name in names:
        rng = np.random.default_rng(dim * 7 + nb)
        data = _clustered(rng, n, dim, clusters, spread)
        ids = _random_ids(rng, n, 40)
        ids[::7] += 1 << 57                                        # sparse, some of them large
        store = InMemoryStorage()
        idx = LSHRS(dim=dim, num_perm=num_perm, num_bands=nb, rows_per_band=r, storage=store, packed_ingest=True, seed=42,
                    keep_vectors=name)
        latest = _Latest(torch, name, dim)
        third = n // 3
        for lo, hi in ((0, third), (third, 2 * third), (2 * third, n)):
            idx.index(ids[lo:hi], data[lo:hi])
            latest.put(ids[lo:hi], data[lo:hi])
        # some ids indexed twice, with other vectors (their neighbours', perturbed): the stale buckets keep the id, the
        # rerank sees the later vector
        again = rng.choice(n, 120, replace=False)
        moved = (data[(again + 1) % n] + 0.02 * rng.standard_normal((120, dim))).astype(np.float32)
        idx.index(ids[again], torch.from_numpy(moved).cuda())
        latest.put(ids[again], moved)
        gone = ids[rng.choice(n, 60, replace=False)]
        idx.delete(gone.tolist())
        latest.drop(gone)
        assert len(idx.vectors) == len(latest.vec) == n - 60
        nq = 48
        queries = (data[rng.choice(n, nq, replace=False)] + 0.05 * rng.standard_normal((nq, dim))).astype(np.float32)
        queries[::16] = rng.standard_normal((len(queries[::16]), dim)).astype(np.float32)
        P = idx._hasher.projections
        cands = [O.query_literal(store, P, dim, v, top_k=None) for v in queries]
        for top_k, top_p in ((None, 0.5), (3, 1.0), (5, 0.01)):
            want = [O.query_literal(store, P, dim, v, top_k=top_k, top_p=top_p, fetch=latest.fetch) for v in queries]
            assert sum(len(w) for w in want) > nq // 2
            listed = idx.query_many(queries, top_k=top_k, top_p=top_p, engine="device")
            hosted = idx.query_many(queries, top_k=top_k, top_p=top_p, engine="host")
            a_ids, a_scores, a_bounds = idx.query_many(queries, top_k=top_k, top_p=top_p, return_arrays=True)
            for i in range(nq):                                  # every query
                judged = dict(query=queries[i], candidates=cands[i], fetch=latest.fetch)
                judge_ranking(listed[i], want[i], **judged)
                judge_ranking(hosted[i], want[i], **judged)
                arr = list(zip(a_ids[a_bounds[i]:a_bounds[i + 1]].tolist(), a_scores[a_bounds[i]:a_bounds[i + 1]].astype(np.float64).tolist()))
                assert arr == listed[i]
        for v, c in zip(queries, cands):
            judged = dict(query=v, candidates=c, fetch=latest.fetch)
            judge_ranking(idx.get_above_p(v, p=0.5), O.query_literal(store, P, dim, v, top_k=None, top_p=0.5, fetch=latest.fetch), **judged)
            judge_ranking(idx.query(v, top_k=3, top_p=1.0), O.query_literal(store, P, dim, v, top_k=3, top_p=1.0, fetch=latest.fetch), **judged)


@pytest.mark.parametrize("name", ("bfloat16", "int8"))
def test_one_query_stays_one_chain(monkeypatch, name):
    """`get_above_p` / `query` on a keep_vectors index - no vector_fetch_fn, no set_corpus - answer through OneQuery: the
    host-counted rerank is made to fail."""
    torch = _torch()
    import lshrs_amd.core as core
    import lshrs_amd.similarity as similarity
    from lshrs_amd import LSHRS, InMemoryStorage
    from oracle import lshrs_oracle as O

    rng = np.random.default_rng(21)
    dim, n = 768, 3000
    data = _clustered(rng, n, dim, 150, 0.3)
    ids = _random_ids(rng, n, 40)
    store = InMemoryStorage()
    idx = LSHRS(dim=dim, num_perm=256, storage=store, packed_ingest=True, keep_vectors=name)
    idx.index(ids[:1500], data[:1500])
    idx.index(ids[1500:], data[1500:])
    latest = _Latest(torch, name, dim)
    latest.put(ids, data)
    queries = (data[rng.choice(n, 60, replace=False)] + 0.05 * rng.standard_normal((60, dim))).astype(np.float32)

    def boom(*a, **k):
        raise AssertionError("the host-counted rerank was taken")

    monkeypatch.setattr(similarity, "rerank_batch", boom)
    monkeypatch.setattr(core, "top_k_cosine", boom)
    P = idx._hasher.projections
    for v in queries:
        judged = dict(query=v, candidates=O.query_literal(store, P, dim, v, top_k=None), fetch=latest.fetch)
        judge_ranking(idx.get_above_p(v, p=0.5), O.query_literal(store, P, dim, v, top_k=None, top_p=0.5, fetch=latest.fetch), **judged)
        judge_ranking(idx.query(v, top_k=3, top_p=1.0), O.query_literal(store, P, dim, v, top_k=3, top_p=1.0, fetch=latest.fetch), **judged)
    assert idx._one_query, "the single-query chain was not taken"


# ------------------------------------------------------------------------------------------ ingest
def _store_state(torch, vectors, ids):
    rows = vectors.rows_of(ids).cpu().numpy()
    hit = rows >= 0
    raw = vectors.rows.view(torch.uint8)[torch.from_numpy(rows[hit]).cuda()].cpu().numpy()
    return hit, raw


def test_ingest_contract():
    """A zero vector in the middle of a batch: the call raises as without a store, and the store holds exactly the ids in
    front of the bad row - on the operation-tuple path, the pipelined array path and two create_signatures lanes."""
    torch = _torch()
    from lshrs_amd import LSHRS, InMemoryStorage

    rng = np.random.default_rng(5)
    dim = 64
    kw = dict(dim=dim, num_perm=64, num_bands=16, rows_per_band=4, seed=42)

    def expect_front(idx, ids, data, bad):
        assert len(idx.vectors) == bad
        hit, raw = _store_state(torch, idx.vectors, ids)
        assert hit[:bad].all() and not hit[bad:].any()
        assert np.array_equal(raw, _raw(torch, _stored_form(torch, "bfloat16", data[:bad])))
        # ... which are the ids the storage holds
        held = set()
        for seg in idx._storage.array_segments(idx._hasher.band_bytes) or []:
            held.update(np.asarray(seg.members).tolist())
        if held:
            assert held == set(ids[:bad].tolist())

    # below packed_auto_min_ops: the reference's operation tuples
    n, bad = 200, 120
    ids, data = _random_ids(rng, n), rng.standard_normal((n, dim)).astype(np.float32)
    data[bad] = 0.0
    small = LSHRS(storage=InMemoryStorage(), keep_vectors="bfloat16", **kw)
    assert n * 16 < small.packed_auto_min_ops
    with pytest.raises(ValueError, match="zero vector"):
        small.index(ids.tolist(), data)
    assert len(small.vectors) == bad and bool((small.vectors.rows_of(ids[:bad]) >= 0).all())
    assert bool((small.vectors.rows_of(ids[bad:]) == -1).all())
    # a negative id in front of the zero vector ends the batch there
    neg = LSHRS(storage=InMemoryStorage(), keep_vectors="bfloat16", **kw)
    bad_ids = ids.copy()
    bad_ids[50] = -4
    with pytest.raises(ValueError, match="non-negative"):
        neg.index(bad_ids.tolist(), data)
    assert len(neg.vectors) == 50

    # the pipelined array path
    n, bad = 6000, 3500
    ids, data = _random_ids(rng, n), rng.standard_normal((n, dim)).astype(np.float32)
    data[bad] = 0.0
    piped = LSHRS(storage=InMemoryStorage(), packed_ingest=True, keep_vectors="bfloat16", **kw)
    assert piped._streams_buckets(n * 16)
    with pytest.raises(ValueError, match="zero vector"):
        piped.index(ids, data)
    expect_front(piped, ids, data, bad)
    # ... the same rows given as a CUDA tensor leave the same store
    resident = LSHRS(storage=InMemoryStorage(), packed_ingest=True, keep_vectors="bfloat16", **kw)
    with pytest.raises(ValueError, match="zero vector"):
        resident.index(ids, torch.from_numpy(data).cuda())
    expect_front(resident, ids, data, bad)
    assert np.array_equal(_raw(torch, resident.vectors.rows), _raw(torch, piped.vectors.rows))
    assert np.array_equal(resident.vectors.rows_of(ids).cpu().numpy(), piped.vectors.rows_of(ids).cpu().numpy())

    # create_signatures, two lanes: units in order, the unit with the bad row ends the stream
    lanes = LSHRS(storage=InMemoryStorage(), packed_ingest=True, keep_vectors="bfloat16", devices=[0, 0], **kw)
    cuts = [0, 1500, 3000, 4500, 6000]                              # the bad row (3500) sits in the third of four batches
    batches = [(ids[a:b], data[a:b]) for a, b in zip(cuts, cuts[1:])]
    with pytest.raises(ValueError, match="zero vector"):
        lanes.create_signatures(format="batches", batches=iter(batches))
    expect_front(lanes, ids, data, bad)
    assert np.array_equal(lanes.vectors.rows_of(ids).cpu().numpy(), piped.vectors.rows_of(ids).cpu().numpy())

    # an id indexed twice ends at its later vector, whichever path took it
    twice = LSHRS(storage=InMemoryStorage(), packed_ingest=True, keep_vectors="float32", **kw)
    good = rng.standard_normal((4000, dim)).astype(np.float32)
    gids = _random_ids(rng, 2000)
    twice.index(np.concatenate([gids, gids]), good)                 # in one call
    assert len(twice.vectors) == 2000 and twice.vectors.stats()["rows"] == 4000
    got = twice.vectors.rows[twice.vectors.rows_of(gids)].cpu().numpy()
    assert np.array_equal(got, good[2000:])

    # ingest() one by one == index() of the same rows
    m = 40
    one = LSHRS(storage=InMemoryStorage(), keep_vectors="int8", **kw)
    for i in range(m):
        one.ingest(int(gids[i]), good[i])
    one.flush()
    both = LSHRS(storage=InMemoryStorage(), keep_vectors="int8", **kw)
    both.index(gids[:m].tolist(), good[:m])
    assert len(one.vectors) == len(both.vectors) == m
    assert np.array_equal(_raw(torch, one.vectors.rows), _raw(torch, both.vectors.rows))
    assert np.array_equal(one.vectors.rows_of(gids[:m]).cpu().numpy(), np.arange(m))
    with pytest.raises(ValueError, match="zero vector"):
        one.ingest(12345, np.zeros(dim, dtype=np.float32))
    with pytest.raises(ValueError, match="non-negative"):
        one.ingest(-1, good[0])
    assert len(one.vectors) == m
    # delete() and clear() reach the store
    one.delete([int(gids[0]), int(gids[1])])
    assert len(one.vectors) == m - 2 and int(gids[0]) not in one.vectors and int(gids[2]) in one.vectors
    one.clear()
    assert len(one.vectors) == 0


# ------------------------------------------------------------------------------------------ errors
def test_a_candidate_without_a_stored_vector():
    torch = _torch()
    from lshrs_amd import DeviceVectors, LSHRS, InMemoryStorage
    from oracle import lshrs_oracle as O

    rng = np.random.default_rng(2)
    dim, n = 32, 600
    data = _clustered(rng, n, dim, 30, 0.2)
    ids = _random_ids(rng, n)
    idx = LSHRS(dim=dim, num_perm=16, storage=InMemoryStorage(), packed_ingest=True)
    idx.index(ids, data)
    q = (data[400:408] + 0.01).astype(np.float32)
    # never stored: a store attached late, holding a part of the ids
    part = DeviceVectors(dim, "bfloat16")
    part.add(ids[:300], data[:300])
    empty = DeviceVectors(dim, "int8")
    for corpus in (part, empty):
        for engine in ("device", "host"):
            with pytest.raises(IndexError, match="no stored vector"):
                idx.query_many(q, top_k=None, top_p=0.5, corpus=corpus, engine=engine)
        idx.set_corpus(corpus)
        with pytest.raises(IndexError, match="no stored vector"):
            idx.get_above_p(q[0], p=0.5)
        idx.set_corpus(None)
    # removed from the store but not from the buckets
    kept = LSHRS(dim=dim, num_perm=16, storage=InMemoryStorage(), packed_ingest=True, keep_vectors="float16")
    kept.index(ids, data)
    assert kept.query_many(q, top_k=None, top_p=0.5, engine="device") == kept.query_many(q, top_k=None, top_p=0.5, engine="host")
    first = kept.get_above_p(q[0], p=1.0)[0][0]
    assert kept.vectors.remove([first]) == 1
    for engine in ("device", "host"):
        with pytest.raises(IndexError, match="no stored vector"):
            kept.query_many(q[:1], top_k=None, top_p=1.0, engine=engine)
    with pytest.raises(IndexError, match="no stored vector"):
        kept.get_above_p(q[0], p=1.0)
    # a zero vector among the stored ones: the reference's error, as on a plain corpus
    kept.vectors.add([first], np.zeros((1, dim), dtype=np.float32))
    with pytest.raises(ValueError, match="Cannot normalize zero vector"):
        kept.get_above_p(q[0], p=1.0)
    with pytest.raises(ValueError, match="Cannot normalize zero vector"):
        kept.query_many(q[:1], top_k=None, top_p=1.0)
    # a tensor of a dtype the rerank does not read keeps its message
    with pytest.raises(ValueError, match="corpus must be a float32, bfloat16 or float16"):
        idx.query_many(q, top_k=None, top_p=0.5, corpus=torch.zeros((n, dim), dtype=torch.float64, device="cuda"))

    # ids beyond the item layout (2^61 with 16 bands): counted on the host, reranked from the store
    big = LSHRS(dim=dim, num_perm=64, num_bands=16, rows_per_band=4, storage=InMemoryStorage(), packed_ingest=True,
                keep_vectors="float32")
    big_ids = (1 << 61) + ids
    big.index(big_ids, data)
    with pytest.raises(Exception):
        big.query_many(q, top_k=None, top_p=0.5, engine="device")
    got = big.query_many(q, top_k=None, top_p=0.5, engine="auto")
    P = big._hasher.projections
    fetch = lambda want: data[np.searchsorted(big_ids, np.asarray(want))]  # noqa: E731
    assert sum(len(g) for g in got) > 0
    for i, v in enumerate(q):
        judged = dict(query=v, candidates=O.query_literal(big._storage, P, dim, v, top_k=None), fetch=fetch)
        judge_ranking(got[i], O.query_literal(big._storage, P, dim, v, top_k=None, top_p=0.5, fetch=fetch), **judged)
        judge_ranking(big.get_above_p(v, p=0.5), O.query_literal(big._storage, P, dim, v, top_k=None, top_p=0.5, fetch=fetch), **judged)


# ------------------------------------------------------------------------------------------ persistence
@pytest.mark.parametrize("name", DTYPES)
def test_save_and_load(tmp_path, name):
    torch = _torch()
    from lshrs_amd import DeviceVectors

    rng = np.random.default_rng(9)
    dim, n = 48, 3000
    ids = _random_ids(rng, n)
    x = rng.standard_normal((n + 500, dim)).astype(np.float32)
    store = DeviceVectors(dim, name)
    store.add(ids, x[:n])
    store.add(ids[:500], x[n:])                                     # superseded rows
    store.remove(ids[1000:1200])                                    # erased ones
    assert store.stats()["dead"] == 700
    path = tmp_path / "vectors.npz"
    store.save(path)
    assert store.stats()["dead"] == 700                             # (the store itself is left as it is)
    back = DeviceVectors.load(path)
    assert back.dtype == name and back.dim == dim and len(back) == len(store) == n - 200
    assert back.stats()["dead"] == 0 and back.stats()["rows"] == n - 200
    rows_a, rows_b = store.rows_of(ids).cpu().numpy(), back.rows_of(ids).cpu().numpy()
    assert np.array_equal(rows_a >= 0, rows_b >= 0) and not (rows_b[1000:1200] >= 0).any()
    live = rows_a >= 0
    bytes_a = store.rows.view(torch.uint8)[torch.from_numpy(rows_a[live]).cuda()].cpu().numpy()
    bytes_b = back.rows.view(torch.uint8)[torch.from_numpy(rows_b[live]).cuda()].cpu().numpy()
    assert np.array_equal(bytes_a, bytes_b)
    store.compact()
    assert np.array_equal(store.rows_of(ids).cpu().numpy(), rows_b) and np.array_equal(_raw(torch, store.rows), _raw(torch, back.rows))
    empty = DeviceVectors(dim, name)
    empty.save(tmp_path / "empty.npz")
    assert len(DeviceVectors.load(tmp_path / "empty.npz")) == 0


# ------------------------------------------------------------------------------------------ full size
def test_full_size_rerank_through_the_map():
    """1 M x 768 bfloat16 under random 40-bit ids, 10 000 queries x 1 000 candidates through the ragged lookup + rerank: the
    planted near-duplicate ranks first for every query, and the answer is the plain path's on the translated rows."""
    torch = _torch()
    from lshrs_amd import DeviceVectors
    from lshrs_amd import _query_device as qd

    m, dim, nq, c = 1_000_000, 768, 10_000, 1_000
    rng = np.random.default_rng(77)
    ids = _random_ids(rng, m, 40)
    rng.shuffle(ids)                                                 # row i holds id ids[i]
    store = DeviceVectors(dim, "bfloat16", capacity=m)
    gen = torch.Generator("cuda").manual_seed(3)
    for lo in range(0, m, 125_000):
        store.add(ids[lo:lo + 125_000], torch.randn(125_000, dim, device="cuda", generator=gen))
    assert len(store) == m and store.stats()["rows"] == m
    rows, table, slots = store.snapshot()
    cand_rows_h = rng.integers(0, m, size=(nq, c), dtype=np.int64)
    planted_at = rng.integers(0, c, size=nq)
    planted_row = cand_rows_h[np.arange(nq), planted_at]
    # (a row drawn twice in one list would tie with the planted one: make the planted row unique in its list)
    dup = (cand_rows_h == planted_row[:, None]).sum(axis=1) > 1
    assert dup.sum() < nq // 50
    for i in np.flatnonzero(dup):
        others = cand_rows_h[i] == planted_row[i]
        others[planted_at[i]] = False
        cand_rows_h[i, others] = (planted_row[i] + 1 + np.arange(others.sum())) % m
    cand_ids = torch.from_numpy(ids[cand_rows_h].reshape(-1)).cuda()
    cand_rows = torch.from_numpy(cand_rows_h.reshape(-1)).cuda()
    queries = rows[torch.from_numpy(planted_row).cuda()].float() + 0.05 * torch.randn(nq, dim, device="cuda", generator=gen)
    pair_off = torch.arange(0, (nq + 1) * c, c, dtype=torch.int64, device="cuda")
    ucount = torch.full((nq,), c, dtype=torch.int32, device="cuda")
    lists = qd._Lists(nq, nq * c, c, pair_off, cand_ids, None, ucount, rows.device)
    assert np.array_equal(store.rows_of(cand_ids[:100_000]).cpu().numpy(), cand_rows_h.reshape(-1)[:100_000])
    got = qd.rank_and_cut(lists, 5, 1.0, queries_dev=queries, corpus=rows, idmap=(table, slots))
    want = qd.rank_and_cut(lists, 5, 1.0, queries_dev=queries, corpus=rows, cand_rows=cand_rows)
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    top_ids, top_scores, bounds = got
    assert np.array_equal(bounds, np.arange(nq + 1) * 5)
    assert np.array_equal(top_ids[::5], ids[planted_row])
    assert top_scores[::5].min() > 0.9 and top_scores[1::5].max() < 0.5
