"""An independent reference for the exhaustive scan (csrc/scan.hip): a plain helper module - imported by the tests, collected
by nobody.

`lshrs_scan_above_*` with a bar of -inf emits the approximate score of EVERY (query, live row), through a kernel that has no
selection, no slices' winners and no merge; the pass that computes the scores is one text (csrc/scan_pass.inc) compiled into
both kernels, and the header promises "same arithmetic".  So the answer of `lshrs_scan_topk_*` is fully determined by those
scores and the item order - descending score, then ascending row - and can be asked for bit for bit, whatever the data:

`all_pairs_approx`  the scores, as a dense (q, m) float32 matrix (NaN where nothing was emitted);
`expected_windows`  the windows those scores determine;
`plan`              the slice count the library plans for a shape, read out of the workspace size.
"""

from __future__ import annotations

import numpy as np

QTILE = 64              # queries per workgroup of the scan
KCHUNK = 64             # k per staged chunk of the query image
CHUNK_BYTES = 16384     # one chunk of one query tile, both terms
MERGE_ITEMS = 8192      # slices * window one merge workgroup sorts in LDS

NEG_INF_BITS = 0xFF800000


def _stored_form(torch, name, x):
    """float32 rows (a host array or a device tensor) as a device tensor of dtype `name`: torch's cast for 16 bits,
    quantize_rows for 8."""
    from lshrs_amd import quantize_rows

    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    if name == "float32":
        return xd.clone()
    if name in ("int8", "float8_e4m3fn"):
        return quantize_rows(xd, getattr(torch, name))
    return xd.to(getattr(torch, name))


def all_pairs_approx(stored, Q_dev, row_ids=None, complete=True):
    """The approximate score of every (query, live row) of `stored` (m, dim; any stored form and layout) for the float32
    device queries `Q_dev` (q, dim): `(A, emitted)`, A a (q, m) float32 NumPy matrix, NaN where no pair was emitted.

    Asserted here: `total` is the number of pairs written, every (query, row) appears exactly once, no dead row appears; and
    with `complete` - the caller's word that the data is finite and nothing has zero norm - that the error word is 0 and
    `total` is q x (live rows).  Every lane of every tile hits: this is also the heaviest use of the range scan's
    reserve-and-write path."""
    import torch

    from lshrs_amd._exact import scan_above

    q, m = int(Q_dev.shape[0]), int(stored.shape[0])
    dev = stored.device
    bars = torch.full((q,), float("-inf"), dtype=torch.float32, device=dev)
    capacity = q * m
    pq, prow, papprox, total, err = scan_above(stored, Q_dev, bars, capacity, row_ids)
    torch.cuda.synchronize(dev)
    emitted = int(total.item())
    assert 0 <= emitted <= capacity, f"total {emitted} of at most {capacity} pairs"
    pq, prow, papprox = pq[:emitted].long(), prow[:emitted], papprox[:emitted]
    assert bool(((pq >= 0) & (pq < q)).all()) and bool(((prow >= 0) & (prow < m)).all()), "a pair outside (q, m)"
    flat = pq * m + prow
    seen = torch.bincount(flat, minlength=q * m)
    assert int(seen.max().item()) <= 1, "a (query, row) was emitted twice"
    assert int(seen.sum().item()) == emitted                  # (total == pairs written: every slot below it holds a pair)
    live = torch.ones(m, dtype=torch.bool, device=dev) if row_ids is None else row_ids >= 0
    assert bool(live[prow].all()), "a dead row was emitted"
    if complete:
        assert int(err.item()) == 0, f"error word {int(err.item())} on finite data of non-zero norm"
        assert emitted == q * int(live.sum().item()), f"{emitted} pairs of {q} x {int(live.sum().item())}"
    A = torch.full((q * m,), float("nan"), dtype=torch.float32, device=dev)
    A[flat] = papprox
    if complete:
        assert not bool(torch.isnan(A.view(q, m)[:, live]).any()), "a NaN score on finite data"
    return A.view(q, m).cpu().numpy(), emitted


def scan_keys(bits):
    """`scan_key` of float32 bit patterns (uint32 array): sign-magnitude to ascending-orderable, so that +0.0 (0x80000000)
    sorts above -0.0 (0x7fffffff).  Not a float compare."""
    u = np.asarray(bits, dtype=np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def expected_windows(A, live_mask, window):
    """The windows the scores `A` (q, m) float32 determine: per query the live, non-NaN rows in the kernel's item order -
    descending `scan_key` of the score's bits, then ascending row - cut at `window`.  Returns `(rows (q, window) int64,
    approx_bits (q, window) uint32, count (q,) int32)`, padded with row -1 and the bits of -inf; count = min(window, number of
    such rows).  The windows of a narrower `window` are the first columns of these (and count its minimum with them)."""
    A = np.ascontiguousarray(A, dtype=np.float32)
    q, m = A.shape
    window = int(window)
    live = np.ones(m, dtype=bool) if live_mask is None else np.asarray(live_mask, dtype=bool)
    bits = A.view(np.uint32)
    valid = live[None, :] & ~np.isnan(A)
    # an item as the kernel builds it: {key, ~row}; 0 = no item (every real key is above 0)
    item = (scan_keys(bits).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(m, dtype=np.uint64))[None, :]
    item = np.where(valid, item, np.uint64(0))
    down = ~item                                             # ascending `down` = descending item
    w = min(window, m)
    if m > w:
        part = np.argpartition(down, w - 1, axis=1)[:, :w]
        order = np.take_along_axis(part, np.argsort(np.take_along_axis(down, part, axis=1), axis=1), axis=1)
    else:
        order = np.argsort(down, axis=1)
    count = np.minimum(valid.sum(axis=1), window).astype(np.int32)
    rows = np.full((q, window), -1, dtype=np.int64)
    out_bits = np.full((q, window), NEG_INF_BITS, dtype=np.uint32)
    rows[:, :w] = order
    out_bits[:, :w] = np.take_along_axis(bits, order, axis=1)
    pad = np.arange(window)[None, :] >= count[:, None]
    rows[pad] = -1
    out_bits[pad] = NEG_INF_BITS
    return rows, out_bits, count


def narrower(expected, window):
    """`expected_windows(A, live, W)` for a W at or below the window `expected` was made with: its first columns."""
    rows, bits, count = expected
    assert window <= rows.shape[1]
    return rows[:, :window], bits[:, :window], np.minimum(count, window).astype(np.int32)


def plan(lib, q, m, dim, window):
    """The slices `lshrs_scan_topk_*` cuts (q, m, dim, window) into, out of `lshrs_scan_workspace_bytes`: the workspace is the
    query image (16 KiB per query tile and 64-chunk of dim), the query norms (256 B per tile), slices x window 8-byte items per
    query, and 16 bytes."""
    nbytes = int(lib.lshrs_scan_workspace_bytes(q, m, dim, window))
    assert nbytes > 0, nbytes
    qtiles, nchunks = -(-q // QTILE), -(-dim // KCHUNK)
    parts = nbytes - 16 - qtiles * nchunks * CHUNK_BYTES - qtiles * QTILE * 4
    assert parts > 0 and parts % (q * window * 8) == 0, (nbytes, parts)
    return parts // (q * window * 8)


def merge_items(slices, window):
    """`(n, npad)`: the items one merge workgroup takes for a query, and the power of two its network is padded to."""
    n = slices * window
    npad = 2
    while npad < n:
        npad <<= 1
    return n, npad


def selection_cap(window):
    """The per-query buffer of the scan's selection: the power of two at or above 2 x window, at least 64."""
    cap = 64
    while cap < 2 * window:
        cap <<= 1
    return cap
