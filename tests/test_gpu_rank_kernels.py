"""`query_rank_kernel` and `query_one_kernel` (csrc/query.hip) on their own, through the C ABI - `lshrs_query_rank_f32`,
`lshrs_query_one_u8` and, for the capacity they share, `lshrs_query_collide_*` - against NumPy / dict models written from
include/lshrs_hip.h: exact score ties, NaN, infinities and signed zeros, list lengths at the seams of the three sort variants,
`ucount = -1` rows inside a batch, compacted outputs with a guard behind them, who publishes `done`, and capacities that are
not powers of two (`max_pairs`: what the caller's buffers hold - a longer list writes nothing)."""

from __future__ import annotations

import math

import numpy as np
import pytest

from tests._plumbing_reference import rank_model as _rank_model, special_scores as _special_scores
from tests._ranking import literal_lists

pytestmark = pytest.mark.gpu

FILL_ID = -7_777_777
FILL_SCORE = 777.0
ROOM = 16384               # LSHRS_QUERY_MAX_PAIRS: the most any of these entries writes, whatever capacity it is handed
GUARD = 1024
U_VALUES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 16383, 16384]
CAPACITIES = [512, 600, 1000, 16384]


def _gpu():
    import torch

    from lshrs_amd import _native

    dev = torch.device("cuda", 0)
    return torch, _native, _native.load(), dev


def _ptr(t):
    return t.data_ptr() if t is not None else None


# ------------------------------------------------------------------------------------------------------------------
# the models
# ------------------------------------------------------------------------------------------------------------------

def _keep_model(n, top_k, top_p):
    """lshrs_query_scan_i32's cut: 0 for no candidates; top_p < 0: min(n, top_k) (top_k < 0: n); else
    min(max(1, ceil((double)n * top_p)), top_k)."""
    if n <= 0:
        return 0
    k = n if top_p < 0 else min(n, max(1, math.ceil(n * top_p)))
    return k if top_k < 0 else min(k, top_k)


def _same_f32(got, want):
    """Bit for bit, NaN compared as NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn])


def _rank_batch(rng):
    """About 60 lists: every U value three times, keep from {0, 1, U - 1, U} spread over them (three of the four for every
    length; the full network, U = 16384, at U, 1 and U - 1), two `ucount = -1` rows in the middle; lists 3 entries apart in the flat arrays (so that a wrong base shows), outputs compact."""
    rows = []
    for shift in (0, 2, 3):
        for i, u in enumerate(U_VALUES):
            k = [0, 1, u - 1, u][(i + shift) % 4]
            rows.append((u, u, min(max(k, 0), u)))                      # (span in the flat arrays, ucount, keep)
    rows[30:30] = [(700, -1, 0), (300, -1, 0)]
    spans = np.array([r[0] + 3 for r in rows], dtype=np.int64)
    pair_off = np.r_[0, np.cumsum(spans)].astype(np.int64)
    ucount = np.array([r[1] for r in rows], dtype=np.int32)
    keep = np.array([r[2] for r in rows], dtype=np.int32)
    out_off = np.r_[0, np.cumsum(keep)].astype(np.int64)
    total = int(pair_off[-1])
    cand = rng.permutation(4 * total)[:total].astype(np.int64) + (1 << 40)
    scores = np.full(total, np.nan, dtype=np.float32)
    for qi, (span, u, _) in enumerate(rows):
        b = int(pair_off[qi])
        scores[b:b + span] = _special_scores(rng, span)
    assert {int(k) for k in keep} >= {0, 1, 16382, 16383, 16384} and len(rows) == 62
    return pair_off, ucount, keep, out_off, cand, scores


def _call_rank(torch, lib, dev, pair_off, ucount, keep, out_off, cand, scores, max_candidates, *, done=None, epoch=0,
               pinned_out=False):
    """One launch; returns (out_ids, out_scores) as host arrays WITH their guard (the caller synchronises when pinned)."""
    kept = int(out_off[-1])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_off, d_u, d_keep, d_out, d_cand = up(pair_off), up(ucount), up(keep), up(out_off), up(cand)
    d_scores = up(scores) if scores is not None else None
    if pinned_out:
        o_ids = torch.full((kept + GUARD,), FILL_ID, dtype=torch.int64).pin_memory()
        o_sc = torch.full((kept + GUARD,), FILL_SCORE, dtype=torch.float32).pin_memory()
    else:
        o_ids = torch.full((kept + GUARD,), FILL_ID, dtype=torch.int64, device=dev)
        o_sc = torch.full((kept + GUARD,), FILL_SCORE, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.lshrs_query_rank_f32(_ptr(d_cand), _ptr(d_scores), _ptr(d_off), _ptr(d_u), _ptr(d_keep), _ptr(d_out), len(ucount),
                                  int(max_candidates), _ptr(o_ids), _ptr(o_sc), _ptr(done), int(epoch), stream)
    assert rc == 0, rc
    if done is not None:
        assert lib.lshrs_wait_done(_ptr(done), int(epoch), 2_000_000, stream) == 0
        assert int(done.numpy()[0]) == epoch                           # (read BEFORE any other synchronisation: the word says so)
        got = o_ids.numpy().copy(), o_sc.numpy().copy()
        torch.cuda.synchronize(dev)
    else:
        torch.cuda.synchronize(dev)
        got = o_ids.cpu().numpy(), o_sc.cpu().numpy()
    assert np.array_equal(d_cand.cpu().numpy(), cand)                   # the inputs are read only
    return got


def _rank_expected(pair_off, ucount, keep, out_off, cand, scores, max_candidates):
    kept = int(out_off[-1])
    ids = np.full(kept + GUARD, FILL_ID, dtype=np.int64)
    sc = np.full(kept + GUARD, FILL_SCORE, dtype=np.float32)
    for qi in range(len(ucount)):
        b, ob, u, k = int(pair_off[qi]), int(out_off[qi]), int(ucount[qi]), int(keep[qi])
        if k <= 0:
            continue
        if scores is None:
            ids[ob:ob + k] = cand[b:b + k]
        elif u <= max_candidates:
            order = np.asarray(_rank_model(scores[b:b + u])[:k], dtype=np.int64)
            ids[ob:ob + k] = cand[b + order]
            sc[ob:ob + k] = scores[b + order]
    return ids, sc


# ------------------------------------------------------------------------------------------------------------------
# lshrs_query_rank_f32
# ------------------------------------------------------------------------------------------------------------------

def test_rank_orders_ties_nans_infinities_and_zeros_at_every_seam():
    torch, _native, lib, dev = _gpu()
    rng = np.random.default_rng(2024)
    pair_off, ucount, keep, out_off, cand, scores = _rank_batch(rng)
    got_ids, got_sc = _call_rank(torch, lib, dev, pair_off, ucount, keep, out_off, cand, scores, 16384)
    want_ids, want_sc = _rank_expected(pair_off, ucount, keep, out_off, cand, scores, 16384)
    kept = int(out_off[-1])
    for qi in range(len(ucount)):                                      # (list by list first: a failure names the list)
        ob, k = int(out_off[qi]), int(keep[qi])
        assert np.array_equal(got_ids[ob:ob + k], want_ids[ob:ob + k]), (qi, int(ucount[qi]), k)
        assert _same_f32(got_sc[ob:ob + k], want_sc[ob:ob + k]), (qi, int(ucount[qi]), k)
    assert np.array_equal(got_ids, want_ids) and _same_f32(got_sc, want_sc)
    assert np.all(got_ids[kept:] == FILL_ID) and np.all(got_sc[kept:] == FILL_SCORE)       # the guard behind the last entry
    # the model itself, on the four things the header names
    assert _rank_model(np.array([1.0, 2.0, 1.0, 2.0], np.float32)) == [1, 3, 0, 2]
    assert _rank_model(np.array([np.nan, -np.inf, np.nan, np.inf], np.float32)) == [3, 1, 0, 2]
    assert _rank_model(np.array([-0.0, 0.0], np.float32)) == [1, 0]

    # scores == NULL: the order the lists have, any length - also beyond a max_candidates that plays no part then
    got_ids, got_sc = _call_rank(torch, lib, dev, pair_off, ucount, keep, out_off, cand, None, 512)
    want_ids, _ = _rank_expected(pair_off, ucount, keep, out_off, cand, None, 512)
    assert np.array_equal(got_ids, want_ids)
    assert np.all(got_sc == FILL_SCORE)                                 # out_scores unused


@pytest.mark.parametrize("u,k", [(1025, 1024), (513, 513), (3, 1)])
def test_rank_of_one_query_publishes_behind_its_pinned_outputs(u, k):
    """q = 1 with done_host: outputs and offsets' consumers in pinned host memory; after lshrs_wait_done the outputs are
    complete and *done_host == epoch."""
    torch, _native, lib, dev = _gpu()
    rng = np.random.default_rng(u)
    pair_off = np.array([0, u], np.int64)
    ucount, keep, out_off = np.array([u], np.int32), np.array([k], np.int32), np.array([0, k], np.int64)
    cand = rng.permutation(10 * u)[:u].astype(np.int64)
    scores = _special_scores(rng, u)
    done = torch.zeros(1, dtype=torch.int32).pin_memory()
    got_ids, got_sc = _call_rank(torch, lib, dev, pair_off, ucount, keep, out_off, cand, scores, 16384, done=done, epoch=41 + u,
                                 pinned_out=True)
    want_ids, want_sc = _rank_expected(pair_off, ucount, keep, out_off, cand, scores, 16384)
    assert np.array_equal(got_ids, want_ids) and _same_f32(got_sc, want_sc)
    # done_host with q != 1 is refused before anything is launched
    p = _ptr(done)
    assert lib.lshrs_query_rank_f32(p, None, p, p, p, p, 2, 16, p, None, p, 1, None) == _native.E_BADARG


def test_positive_zero_ranks_ahead_of_negative_zero_in_both_entries():
    """The header of lshrs_query_rank_f32 and of lshrs_topk_desc_f32 (they share the key): the two zeros are not a tie."""
    torch, _native, lib, dev = _gpu()
    scores = np.array([-0.0, 0.0], dtype=np.float32)
    cand = np.array([50, 60], dtype=np.int64)
    ids, sc = _call_rank(torch, lib, dev, np.array([0, 2], np.int64), np.array([2], np.int32), np.array([2], np.int32),
                         np.array([0, 2], np.int64), cand, scores, 16)
    assert ids[:2].tolist() == [60, 50] and _same_f32(sc[:2], np.array([0.0, -0.0], np.float32))
    d_scores = torch.from_numpy(scores).to(dev)
    order = torch.full((2,), -1, dtype=torch.int32, device=dev)
    srt = torch.full((2,), FILL_SCORE, dtype=torch.float32, device=dev)
    rc = lib.lshrs_topk_desc_f32(d_scores.data_ptr(), 1, 2, 2, order.data_ptr(), srt.data_ptr(), None,
                                 torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize(dev)
    assert order.cpu().numpy().tolist() == [1, 0] and _same_f32(srt.cpu().numpy(), np.array([0.0, -0.0], np.float32))


@pytest.mark.parametrize("cap", CAPACITIES)
def test_rank_leaves_lists_beyond_max_candidates_exactly_to_the_caller(cap):
    """max_candidates is the number itself, not the power of two the network is sized for: lists of cap - 1 and cap are
    ranked, lists of cap + 1 and of the next power of two are not touched."""
    torch, _native, lib, dev = _gpu()
    rng = np.random.default_rng(cap)
    lengths = [cap - 1, cap, cap + 1, 1 << cap.bit_length()]
    pair_off = np.r_[0, np.cumsum(lengths)].astype(np.int64)
    ucount = np.array(lengths, np.int32)
    keep = ucount.copy()
    out_off = pair_off.copy()
    total = int(pair_off[-1])
    cand = rng.permutation(4 * total)[:total].astype(np.int64)
    scores = np.concatenate([_special_scores(rng, n) for n in lengths])
    got_ids, got_sc = _call_rank(torch, lib, dev, pair_off, ucount, keep, out_off, cand, scores, cap)
    want_ids, want_sc = _rank_expected(pair_off, ucount, keep, out_off, cand, scores, cap)
    for qi, n in enumerate(lengths):
        ob = int(out_off[qi])
        if n > cap:
            assert np.all(got_ids[ob:ob + n] == FILL_ID) and np.all(got_sc[ob:ob + n] == FILL_SCORE), (qi, n)
        else:
            assert np.array_equal(got_ids[ob:ob + n], want_ids[ob:ob + n]) and _same_f32(got_sc[ob:ob + n], want_sc[ob:ob + n]), (qi, n)
    assert np.array_equal(got_ids, want_ids) and _same_f32(got_sc, want_sc)


# ------------------------------------------------------------------------------------------------------------------
# segments whose pair lists have a chosen length
# ------------------------------------------------------------------------------------------------------------------

def _segments_with_lists(rng, lengths, nb):
    """Two BucketCSR segments (one-byte keys) and keys (len(lengths), nb, 1): query j - key j in every band - selects buckets
    holding exactly lengths[j] members with multiplicity.  Ids sit in 1 .. nb bands of their list; for lists of 200 pairs and
    more, five ids are in BOTH segments (twice in a bucket: two pairs, one collision).  Keys >= 200: rows no query selects."""
    from lshrs_amd.packed_ops import _csr_host

    assert len(lengths) < 200
    rows = [[], []]                                                     # per segment: (id slot, key row)
    plan = []
    for j, want in enumerate(lengths):
        left = want
        dup = []
        if want >= 200:
            dup = rng.integers(1, nb + 1, size=5).tolist()
            left -= 2 * sum(dup)
        singles = []
        while left > 0:
            m = min(left, int(rng.integers(1, nb + 1)))
            singles.append(m)
            left -= m
        plan.append((j, dup, singles))
    n_ids = sum(len(d) + len(s) for _, d, s in plan) + 50
    ids = (rng.permutation(8 * n_ids)[:n_ids].astype(np.int64) + 1) * 1_000_003
    nxt = 0
    for j, dup, singles in plan:
        for m, both in [(m, True) for m in dup] + [(m, False) for m in singles]:
            key = rng.integers(200, 256, size=nb).astype(np.uint8)
            key[rng.choice(nb, size=m, replace=False)] = j
            for g in ((0, 1) if both else (int(rng.integers(0, 2)),)):
                rows[g].append((ids[nxt], key))
            nxt += 1
    for _ in range(50):
        rows[int(rng.integers(0, 2))].append((ids[nxt], rng.integers(200, 256, size=nb).astype(np.uint8)))
        nxt += 1
    segs = []
    for g in range(2):
        seg = _csr_host(np.array([r[0] for r in rows[g]], dtype=np.int64), np.stack([r[1] for r in rows[g]])[:, :, None])
        seg.distinct = True
        segs.append(seg)
    keys = np.repeat(np.arange(len(lengths), dtype=np.uint8)[:, None, None], nb, axis=1)
    return segs, keys


def _pairs_of(segs, keys, nb, bb):
    """The (member, band) pairs of every query, with multiplicity, flat, and their offsets: what the lookup's slots name."""
    ms, bs, off = [], [], [0]
    for qi in range(keys.shape[0]):
        n = 0
        for b in range(nb):
            code = (b << (8 * bb)) | int.from_bytes(keys[qi, b].tobytes(), "little")
            for seg in segs:
                g = int(np.searchsorted(seg.codes, code))
                if g < len(seg) and int(seg.codes[g]) == code:
                    mem = seg.members[seg.offsets[g]:seg.offsets[g + 1]]
                    ms.append(mem)
                    bs.append(np.full(len(mem), b, np.int32))
                    n += len(mem)
        off.append(off[-1] + n)
    return (np.concatenate(ms) if ms else np.empty(0, np.int64), np.concatenate(bs) if bs else np.empty(0, np.int32),
            np.asarray(off, np.int64))


# ------------------------------------------------------------------------------------------------------------------
# lshrs_query_one_u8
# ------------------------------------------------------------------------------------------------------------------

def _call_one(torch, lib, dev, desc, nseg, key_row, nb, bb, *, max_pairs, top_k=-1, top_p=-1.0, rerank_follows=0, epoch=1,
              done_before=0, copy_src=None):
    """One launch with every output pre-filled; everything it may have written, as host arrays."""
    nslots = max(1, nb * nseg)
    s_start = torch.zeros(nslots, dtype=torch.int64, device=dev)
    s_len = torch.zeros(nslots, dtype=torch.int32, device=dev)
    s_off = torch.zeros(nslots, dtype=torch.int32, device=dev)
    keys_d = torch.from_numpy(np.ascontiguousarray(key_row)).to(dev)
    pair_off = torch.full((2,), -5, dtype=torch.int64, device=dev)
    cand = torch.full((ROOM + GUARD,), FILL_ID, dtype=torch.int64, device=dev)
    out_ids = torch.full((ROOM + GUARD,), FILL_ID, dtype=torch.int64, device=dev)
    ucount = torch.full((1,), -9, dtype=torch.int32, device=dev)
    keep = torch.full((1,), -9, dtype=torch.int32, device=dev)
    out_off = torch.full((3,), -5, dtype=torch.int64, device=dev)
    done = torch.full((1,), done_before, dtype=torch.int32).pin_memory()
    src = dst = None
    copy_n = 0
    if copy_src is not None:
        copy_n = len(copy_src)
        src = torch.from_numpy(copy_src).pin_memory()
        dst = torch.full((copy_n + 8,), FILL_SCORE, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.lshrs_query_one_u8(_ptr(keys_d), nb, bb, _ptr(desc), nseg, _ptr(s_start), _ptr(s_len), _ptr(s_off), int(max_pairs),
                                int(top_k), float(top_p), int(rerank_follows), _ptr(pair_off), _ptr(cand), _ptr(ucount),
                                _ptr(keep), _ptr(out_off), _ptr(out_ids), _ptr(done), int(epoch), _ptr(src), _ptr(dst), copy_n,
                                stream)
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    res = dict(pair_off=pair_off.cpu().numpy().tolist(), cand=cand.cpu().numpy(), out_ids=out_ids.cpu().numpy(),
               ucount=int(ucount.cpu()[0]), keep=int(keep.cpu()[0]), out_off=out_off.cpu().numpy().tolist(),
               done=int(done.numpy()[0]), copied=dst.cpu().numpy() if dst is not None else None)
    res["device"] = (cand, pair_off, ucount, keep)                      # (for a rank launch behind this one)
    return res


def _check_one(res, want_ids, pairs, *, max_pairs, top_k, top_p, rerank_follows, epoch, done_before):
    """The header's account of what lshrs_query_one_u8 leaves, for a list within the capacity."""
    u = len(want_ids)
    k = _keep_model(u, top_k, top_p)
    what = (pairs, u, k, top_k, top_p, rerank_follows)
    assert res["ucount"] == u, what
    assert res["keep"] == k, what
    assert res["pair_off"] == [0, pairs], what
    assert res["out_off"] == [0, k, u], what
    assert res["cand"][:u].tolist() == want_ids, what
    assert np.all(res["cand"][max_pairs:] == FILL_ID), what
    if rerank_follows and k > 0:                                        # the rank launch behind it writes out_ids and publishes
        assert np.all(res["out_ids"] == FILL_ID), what
        assert res["done"] == done_before, what
    else:                                                               # this launch does (also when nothing is kept)
        assert res["out_ids"][:k].tolist() == want_ids[:k], what
        assert np.all(res["out_ids"][k:] == FILL_ID), what
        assert res["done"] == epoch, what
    return k


def test_one_query_lookup_collide_cut_and_who_publishes():
    torch, _native, lib, dev = _gpu()
    from lshrs_amd import _query_device as qd
    from lshrs_amd.packed_ops import _csr_host

    rng = np.random.default_rng(77)
    nb, bb, key_space = 16, 2, 40
    segs = []
    for _ in range(3):                                                  # ids overlap between segments: an id twice in a bucket
        ids = rng.choice(600, size=400, replace=False).astype(np.int64)
        vals = rng.integers(0, key_space, size=(400, nb))
        seg = _csr_host(ids, np.stack([(vals >> (8 * j)) & 0xFF for j in range(bb)], axis=-1).astype(np.uint8))
        seg.distinct = True
        segs.append(seg)
    mirror = qd.DeviceBuckets()
    desc, nseg, _ = mirror.table(segs, dev)
    assert nseg == 3
    vals = rng.integers(0, key_space + 3, size=(6, nb))                 # (+3: some bands select no bucket)
    vals[5] = key_space + 1                                             # no candidates at all
    keys = np.stack([(vals >> (8 * j)) & 0xFF for j in range(bb)], axis=-1).astype(np.uint8)
    want = [[i for i, _ in w] for w in literal_lists(segs, keys, nb, bb)]
    pairs = np.diff(_pairs_of(segs, keys, nb, bb)[2]).tolist()
    assert want[5] == [] and pairs[5] == 0 and all(len(w) > 20 for w in want[:5])
    assert any(p > len(w) for p, w in zip(pairs, want))                 # ids in several bands / twice in a bucket
    cuts = [(-1, -1.0), (7, -1.0), (10 ** 6, -1.0), (-1, 0.3), (-1, 1.0), (-1, 1e-9), (5, 0.5), (1000, 0.5), (1, 0.01)]
    assert {_keep_model(len(want[0]), k, p) for k, p in cuts} >= {1, 5, 7, len(want[0]), math.ceil(len(want[0]) * 0.3)}
    epoch = 100
    for qi in range(6):
        for top_k, top_p in cuts:
            for follows in (0, 1):
                epoch += 1
                kw = dict(max_pairs=ROOM, top_k=top_k, top_p=top_p, rerank_follows=follows, epoch=epoch, done_before=epoch - 1)
                res = _call_one(torch, lib, dev, desc, nseg, keys[qi], nb, bb, **kw)
                _check_one(res, want[qi], pairs[qi], **kw)
    # the query vector copied for the rerank launch: copy_n floats, exactly, nothing behind them
    src = _special_scores(rng, 771)
    res = _call_one(torch, lib, dev, desc, nseg, keys[0], nb, bb, max_pairs=ROOM, top_p=0.5, rerank_follows=1, copy_src=src)
    assert _same_f32(res["copied"][:771], src) and np.all(res["copied"][771:] == FILL_SCORE)
    # an empty index: nseg = 0, no segment table - no candidates, published by this launch whatever follows
    for follows in (0, 1):
        kw = dict(max_pairs=ROOM, top_k=3, top_p=0.5, rerank_follows=follows, epoch=9, done_before=4)
        _check_one(_call_one(torch, lib, dev, None, 0, keys[0], nb, bb, **kw), [], 0, **kw)
    # the chain of one reranked query: this launch leaves the list, the rank launch behind it (q = 1, done_host) cuts,
    # writes and publishes - from the device arrays this one left
    res = _call_one(torch, lib, dev, desc, nseg, keys[1], nb, bb, max_pairs=ROOM, top_k=-1, top_p=0.5, rerank_follows=1, epoch=7)
    u = len(want[1])
    k = _keep_model(u, -1, 0.5)
    assert res["keep"] == k and res["done"] == 0
    cand_d, off_d, u_d, keep_d = res["device"]
    scores = _special_scores(rng, u)
    sc_d = torch.from_numpy(scores).to(dev)
    zero_off = torch.zeros(2, dtype=torch.int64, device=dev)
    o_ids = torch.full((k + GUARD,), FILL_ID, dtype=torch.int64).pin_memory()
    o_sc = torch.full((k + GUARD,), FILL_SCORE, dtype=torch.float32).pin_memory()
    done = torch.zeros(1, dtype=torch.int32).pin_memory()
    torch.cuda.synchronize(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    assert lib.lshrs_query_rank_f32(cand_d.data_ptr(), sc_d.data_ptr(), off_d.data_ptr(), u_d.data_ptr(), keep_d.data_ptr(),
                                    zero_off.data_ptr(), 1, ROOM, o_ids.data_ptr(), o_sc.data_ptr(), done.data_ptr(), 8, stream) == 0
    assert lib.lshrs_wait_done(done.data_ptr(), 8, 2_000_000, stream) == 0
    assert int(done.numpy()[0]) == 8
    order = _rank_model(scores)[:k]
    assert o_ids.numpy()[:k].tolist() == [want[1][p] for p in order] and _same_f32(o_sc.numpy()[:k], scores[order])
    assert np.all(o_ids.numpy()[k:] == FILL_ID)
    torch.cuda.synchronize(dev)


def _capacity_case(cap):
    rng = np.random.default_rng(cap + 1)
    nb = 16
    lengths = [cap - 1, cap, cap + 1, 1 << cap.bit_length()]
    segs, keys = _segments_with_lists(rng, lengths, nb)
    members, bands, pair_off = _pairs_of(segs, keys, nb, 1)
    assert np.diff(pair_off).tolist() == lengths
    want = literal_lists(segs, keys, nb, 1)
    assert all(0 < len(w) < n for w, n in zip(want, lengths))           # collisions: fewer candidates than pairs
    return nb, lengths, segs, keys, members, bands, pair_off, want


@pytest.mark.parametrize("cap", CAPACITIES)
def test_one_query_keeps_to_max_pairs_exactly(cap):
    """max_pairs is what cand_ids holds: a pair list of max_pairs + 1 - or of the next power of two - leaves ucount = -1,
    keep = 0 and nothing written, although the LDS network (sized to a power of two) would take it.  cand_ids and out_ids
    have room for LSHRS_QUERY_MAX_PAIRS entries and a guard whatever `cap` is: nothing this test does leaves its own memory.
    (Before max_pairs was handed to the kernel beside the LDS size, the max_pairs + 1 cases at 600 and 1000 ran: ucount came
    back as the candidate count and up to 1 024 ids were written into a buffer declared to hold 600.)"""
    torch, _native, lib, dev = _gpu()
    from lshrs_amd import _query_device as qd

    nb, lengths, segs, keys, _, _, _, want = _capacity_case(cap)
    mirror = qd.DeviceBuckets()
    desc, nseg, _ = mirror.table(segs, dev)
    assert nseg == 2
    for j, n in enumerate(lengths):
        for follows in (0, 1):
            kw = dict(max_pairs=cap, top_k=-1, top_p=-1.0 if not follows else 1.0, rerank_follows=follows, epoch=20 + j,
                      done_before=3)
            res = _call_one(torch, lib, dev, desc, nseg, keys[j], nb, 1, **kw)
            if n <= cap:
                _check_one(res, [i for i, _ in want[j]], n, **kw)
                continue
            assert res["ucount"] == -1, (cap, n, res["ucount"])
            assert res["keep"] == 0 and res["out_off"] == [0, 0, -1] and res["pair_off"] == [0, 0], (cap, n)
            assert np.all(res["cand"][cap:] == FILL_ID) and np.all(res["out_ids"][cap:] == FILL_ID), (cap, n)
            assert np.all(res["cand"] == FILL_ID) and np.all(res["out_ids"] == FILL_ID), (cap, n)      # "untouched"
            assert res["done"] == 20 + j, (cap, n)                      # nothing kept: this launch publishes, whatever follows


@pytest.mark.parametrize("cap", CAPACITIES)
def test_collide_keeps_to_max_pairs_exactly(cap):
    """lshrs_query_collide_index_i64 / _pairs_i64: "ucount[qi] = -1: the list is longer than max_pairs - exactly that number -
    nothing written", in one batch of four lists around `cap`; the others are counted as a dict counts them."""
    torch, _native, lib, dev = _gpu()
    from lshrs_amd import _query_device as qd

    nb, lengths, segs, keys, members, bands, pair_off, want = _capacity_case(cap)
    total = int(pair_off[-1])
    stream = torch.cuda.current_stream(dev).cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

    def check(cand, hits, ucount, what):
        cand, hits, ucount = cand.cpu().numpy(), hits.cpu().numpy(), ucount.cpu().numpy()
        for j, n in enumerate(lengths):
            b = int(pair_off[j])
            if n > cap:
                assert ucount[j] == -1, (what, cap, n, int(ucount[j]))
                assert np.all(cand[b:b + n] == FILL_ID) and np.all(hits[b:b + n] == -3), (what, cap, n)
            else:
                u = len(want[j])
                assert ucount[j] == u, (what, cap, n)
                assert list(zip(cand[b:b + u].tolist(), hits[b:b + u].tolist())) == want[j], (what, cap, n)
                assert np.all(cand[b + u:b + n] == FILL_ID), (what, cap, n)
        assert np.all(cand[total:] == FILL_ID) and np.all(hits[total:] == -3), what

    def outputs():
        return (torch.full((total + GUARD,), FILL_ID, dtype=torch.int64, device=dev),
                torch.full((total + GUARD,), -3, dtype=torch.int32, device=dev), torch.full((4,), -9, dtype=torch.int32, device=dev))

    # pairs handed in flat
    cand, hits, ucount = outputs()
    m_d, b_d, off_d = up(members), up(bands), up(pair_off)
    torch.cuda.synchronize(dev)
    assert lib.lshrs_query_collide_pairs_i64(m_d.data_ptr(), b_d.data_ptr(), off_d.data_ptr(), 4, cap, nb, cand.data_ptr(),
                                             hits.data_ptr(), ucount.data_ptr(), stream) == 0
    torch.cuda.synchronize(dev)
    check(cand, hits, ucount, "pairs")
    # members read from the segments through the lookup's slots
    mirror = qd.DeviceBuckets()
    desc, nseg, _ = mirror.table(segs, dev)
    nslots = nb * nseg
    s_start = torch.zeros(4 * nslots, dtype=torch.int64, device=dev)
    s_len = torch.zeros(4 * nslots, dtype=torch.int32, device=dev)
    s_off = torch.zeros(4 * nslots, dtype=torch.int32, device=dev)
    count = torch.zeros(4, dtype=torch.int32, device=dev)
    keys_d = up(keys)
    cand, hits, ucount = outputs()
    torch.cuda.synchronize(dev)
    assert lib.lshrs_query_lookup_u8(keys_d.data_ptr(), 4, nb, 1, desc.data_ptr(), nseg, s_start.data_ptr(), s_len.data_ptr(),
                                     s_off.data_ptr(), count.data_ptr(), stream) == 0
    torch.cuda.synchronize(dev)
    assert count.cpu().numpy().tolist() == lengths
    assert lib.lshrs_query_collide_index_i64(desc.data_ptr(), nseg, nb, s_start.data_ptr(), s_len.data_ptr(), s_off.data_ptr(),
                                             off_d.data_ptr(), 4, cap, cand.data_ptr(), hits.data_ptr(), ucount.data_ptr(),
                                             stream) == 0
    torch.cuda.synchronize(dev)
    check(cand, hits, ucount, "index")
