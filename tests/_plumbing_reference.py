"""Plain NumPy / Python statements of the plumbing entry points of include/lshrs_hip.h - the tie-break's gathers and key
patch, the key hex text, the bucket histogram and scatter, l2_norm and the order of lshrs_topk_desc_f32 - and the guarded
device buffers the GPU tests (tests/test_gpu_plumbing_kernels.py) hand to them.  Nothing here touches a device unless it is
given `torch`; tests/test_plumbing_reference_host.py checks every statement against an independent one."""

from __future__ import annotations

import math

import numpy as np

GUARD_BYTES = 64
GUARD_FILL = 0xA5
FILL_I32 = int(np.array([GUARD_FILL] * 4, dtype=np.uint8).view(np.int32)[0])     # an int32 / float32 of untouched memory


# ------------------------------------------------------------------------------------------------------------------
# guarded device buffers
# ------------------------------------------------------------------------------------------------------------------

def guarded(torch, nbytes_or_shape, dtype=None, offset=0, device=None):
    """A device tensor of `dtype` (default uint8) and the given shape (an int: that many elements) that is a view into a
    larger uint8 buffer filled with 0xA5: GUARD_BYTES + offset bytes in front of it, GUARD_BYTES behind it.  The buffer
    starts at an allocation boundary (a multiple of 64 at least), so the view starts at `offset` modulo 64: an odd offset
    puts a base at an odd address where the ABI allows any.  The view itself is filled with 0xA5 too: whatever a kernel
    leaves alone still reads FILL_I32."""
    dtype = torch.uint8 if dtype is None else dtype
    shape = (int(nbytes_or_shape),) if isinstance(nbytes_or_shape, (int, np.integer)) else tuple(int(s) for s in nbytes_or_shape)
    item = torch.empty(0, dtype=dtype).element_size()
    assert offset >= 0 and offset % item == 0, "the view must be aligned to its own element"
    nbytes = item * math.prod(shape)
    device = torch.device("cuda", 0) if device is None else device
    buf = torch.full((GUARD_BYTES + offset + nbytes + GUARD_BYTES,), GUARD_FILL, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 64 == 0
    view = buf[GUARD_BYTES + offset:GUARD_BYTES + offset + nbytes].view(dtype).view(shape)
    assert view.data_ptr() == buf.data_ptr() + GUARD_BYTES + offset
    view.guard_buffer = buf                      # (what guards_intact reads; the view keeps the buffer alive)
    return view


def guards_intact(view):
    """Both guards of a tensor `guarded` made: every byte of its buffer in front of it and behind it is still 0xA5."""
    buf = view.guard_buffer
    assert buf.element_size() == 1 and buf.dim() == 1
    front = view.data_ptr() - buf.data_ptr()
    nbytes = view.numel() * view.element_size()
    assert front >= GUARD_BYTES and buf.numel() == front + nbytes + GUARD_BYTES
    host = buf.cpu().numpy()
    return bool(np.all(host[:front] == GUARD_FILL) and np.all(host[front + nbytes:] == GUARD_FILL))


def fill_guarded(torch, view, array):
    """Copy a host array into a guarded view of the same dtype and shape (the guards stay what they were)."""
    src = torch.from_numpy(np.ascontiguousarray(array))
    assert src.dtype == view.dtype and tuple(src.shape) == tuple(view.shape), (src.dtype, view.dtype, src.shape, view.shape)
    view.copy_(src)
    return view


def bits(a):
    """float32 values as their int32 bit patterns: NaN payloads, infinities and the sign of zero count in a comparison."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------------
# the order of lshrs_topk_desc_f32 (and of lshrs_query_rank_f32: they share the key)
# ------------------------------------------------------------------------------------------------------------------

def rank_model(scores):
    """Positions of `scores` in the header's order: descending score; ties by ascending position; NaN last, by position;
    +0.0 ahead of -0.0 wherever they stand."""
    def key(p):
        v = float(scores[p])
        if v != v:
            return (1, 0.0, 0, p)
        return (0, -v, int(np.signbit(scores[p])) if v == 0.0 else 0, p)

    return sorted(range(len(scores)), key=key)


def special_scores(rng, n):
    """Quarter steps in [-1.5, 1.5] - thirteen values, so runs of exact ties at every length - and, where they fit: a -0.0 AHEAD
    of a +0.0, three NaNs (one with the sign bit and a payload), +inf and -inf."""
    s = (rng.integers(-6, 7, size=n) / 4.0).astype(np.float32)
    neg_nan = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]
    specials = [np.float32(-0.0), np.float32(0.0), np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), neg_nan,
                np.float32(np.nan)][:n]
    pos = np.sort(rng.choice(n, size=len(specials), replace=False)) if n else np.empty(0, np.int64)
    rest = rng.permutation(pos[2:])
    for p, v in zip(np.r_[pos[:2], rest].astype(np.int64), specials):
        s[p] = v
    return s


# ------------------------------------------------------------------------------------------------------------------
# the tie-break's plumbing and the key text
# ------------------------------------------------------------------------------------------------------------------

def gather_reference(x, dim, rows):
    """lshrs_gather_rows_f32: dst[t] = X[rows[t]][:dim]."""
    return np.ascontiguousarray(np.asarray(x)[np.asarray(rows, dtype=np.int64), :dim])


def tied_rows_reference(x, dim, tie_list, tie_count, tie_cap):
    """lshrs_gather_tied_rows_f32: (row of entry e, for e < min(tie_count, tie_cap); the rows of dst those entries fill).
    Entry e is (tie_list[2e], tie_list[2e + 1]) = (row * 65536 + w, mask): the row is all that matters here."""
    live = max(0, min(int(tie_count), int(tie_cap)))
    rows = np.asarray(tie_list, dtype=np.int64).reshape(-1, 2)[:live, 0] >> 16
    return rows, gather_reference(x, dim, rows)


def scatter_keys_reference(keys, rows, bands, patch):
    """lshrs_scatter_band_keys_u8: keys[rows[t]][bands[t]][:] = patch[t][:] on a copy of keys (n, num_bands, band_bytes)."""
    out = np.array(keys, dtype=np.uint8, copy=True)
    out[np.asarray(rows, dtype=np.int64), np.asarray(bands, dtype=np.int64), :] = np.asarray(patch, dtype=np.uint8)
    return out


_HEX_DIGITS = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)


def hex_reference(keys):
    """lshrs_keys_to_hex_u8: hex[2i], hex[2i + 1] = the lower-case hex digits of byte i, high nibble first."""
    flat = np.asarray(keys, dtype=np.uint8).reshape(-1)
    out = np.empty(2 * flat.size, dtype=np.uint8)
    out[0::2] = _HEX_DIGITS[flat >> 4]
    out[1::2] = _HEX_DIGITS[flat & 15]
    return out


# ------------------------------------------------------------------------------------------------------------------
# buckets
# ------------------------------------------------------------------------------------------------------------------

def bucket_bins(keys):
    """bin of every (row, band) of keys (n, num_bands, band_bytes): band << (8 * band_bytes) | the key read little-endian."""
    keys = np.asarray(keys, dtype=np.uint8)
    n, nb, bb = keys.shape
    value = np.zeros((n, nb), dtype=np.int64)
    for j in range(bb):
        value |= keys[:, :, j].astype(np.int64) << (8 * j)
    return (np.arange(nb, dtype=np.int64)[None, :] << (8 * bb)) | value


def bucket_reference(keys, ids):
    """lshrs_bucket_histogram_u8 / lshrs_bucket_scatter_u8: (counts int32[num_bands << (8 * band_bytes)], {bin: sorted ids})
    - the ids with multiplicity (an id two rows carry stands twice in every bin both rows fall into); empty bins have no
    entry in the dict."""
    keys = np.asarray(keys, dtype=np.uint8)
    n, nb, bb = keys.shape
    ids = np.asarray(ids, dtype=np.int64)
    assert ids.shape == (n,)
    bins = bucket_bins(keys).reshape(-1)
    per_pair = np.repeat(ids, nb)
    counts = np.zeros(nb << (8 * bb), dtype=np.int32)
    np.add.at(counts, bins, 1)
    order = np.lexsort((per_pair, bins))
    sorted_bins, sorted_ids = bins[order], per_pair[order]
    cuts = np.flatnonzero(np.diff(sorted_bins)) + 1
    members = {int(chunk_bins[0]): chunk_ids.tolist()
               for chunk_bins, chunk_ids in zip(np.split(sorted_bins, cuts), np.split(sorted_ids, cuts)) if len(chunk_bins)}
    return counts, members


# ------------------------------------------------------------------------------------------------------------------
# l2_norm
# ------------------------------------------------------------------------------------------------------------------

def l2_reference(x):
    """x / ||x|| row by row in float64 (a zero row: NaN, no claim is made about it)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / np.sqrt(np.sum(x * x, axis=-1, keepdims=True))


def l2_tolerance(dim):
    """Bound on |out - reference| / |reference| for lshrs_l2_normalize_f32, from the kernel's own arithmetic (u = 2^-24, the
    relative error of one float32 rounding; one unit in the last place is at most 2 u of the value):

      - the sum of squares is a sum of NON-NEGATIVE terms, so no term's error is magnified by cancellation: every term passes
        through at most ceil(dim / 256) fused multiply-adds in its lane (one rounding each), six butterfly additions across the
        wave and three additions of the four waves' parts.  Its relative error is at most (ceil(dim / 256) + 9) u;
      - the square root halves a relative error and adds at most one unit in the last place: (ceil(dim / 256) + 9) / 2 u + 2 u;
      - the division adds at most one more: + 2 u.

    Together ((ceil(dim / 256) + 9) / 2 + 4) * 2^-24 of |reference|: 9 u up to 256-d, 9.5 u at 257-d, 10.5 u at 1000-d.
    (First order in u; the terms dropped are below 100 u^2 = 6e-6 u.  The float64 reference's own error, about dim * 2^-53,
    is of that size too.)"""
    steps = -(-int(dim) // 256) + 9
    return (steps / 2.0 + 4.0) * 2.0 ** -24
