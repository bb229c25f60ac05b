"""The plumbing kernels of csrc/storage.hip - the tie-break's two gathers and its key patch, the key hex text, the bucket
histogram and scatter - and of csrc/rerank.hip - l2_norm and the LDS bitonic network behind lshrs_topk_desc_f32 - called
directly at their C ABI and compared with the plain statements of tests/_plumbing_reference.py: every output between two
guards of 0xA5 bytes that are checked when the test ends, floats compared as bits, sizes at every edge of the launch
geometry (the 256-lane stride of the row kernels, 16 bytes per lane and 4096 per workgroup of the hex kernel, the 2048
workgroups of the tied-row gather, every power of two of the network)."""

from __future__ import annotations

import numpy as np
import pytest

from tests import _plumbing_reference as R

pytestmark = pytest.mark.gpu


def _gpu():
    import torch

    from lshrs_amd import _native

    dev = torch.device("cuda", 0)
    return torch, _native.load(), dev


def _up(torch, dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _stream(torch, dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _salted_matrix(rng, n, dim, pad):
    """(n, dim + pad) float32: Gaussian data salted with NaN, +-Inf, -0.0 and a subnormal in rows 0 .. 4 and n - 1; the `pad`
    columns behind `dim` hold bit patterns (8388608.0 + position) that stand nowhere in the data."""
    x = rng.standard_normal((n, dim + pad)).astype(np.float32)
    salt = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(-0.0),
            np.array([0x00000123], np.uint32).view(np.float32)[0], np.array([0xFFC00001], np.uint32).view(np.float32)[0]]
    for i, (row, v) in enumerate(zip([0, 1, 2, 3, 4, n - 1], salt)):
        x[row, (7 * i) % dim] = v
    x[:, dim:] = (8388608.0 + np.arange(n * pad, dtype=np.float32)).reshape(n, pad)
    return x


# ------------------------------------------------------------------------------------------------------------------
# 1. lshrs_gather_rows_f32
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 5, 255, 256, 257, 700])
def test_gather_rows_copies_exactly_the_rows_asked_for(dim):
    torch, lib, dev = _gpu()
    rng = np.random.default_rng(dim)
    n, pad = 41, 3
    x = _salted_matrix(rng, n, dim, pad)
    d_x = _up(torch, dev, x)
    pad_bits = R.bits(x[:, dim:]).reshape(-1)
    for m in (1, 3, 300):
        rows = {1: [40], 3: [40, 0, 40]}.get(m)
        if rows is None:
            rows = rng.integers(0, n, size=m)
            rows[[0, 7, 150, 299]] = [40, 0, 0, 40]                         # repeats, the first row and the last
            rows[20:24] = [1, 2, 3, 4]                                      # (the other salted rows)
        rows = np.asarray(rows, dtype=np.int64)
        d_rows = _up(torch, dev, rows)
        dst = R.guarded(torch, (m, dim), torch.float32, device=dev)
        assert lib.lshrs_gather_rows_f32(d_x.data_ptr(), dim + pad, dim, d_rows.data_ptr(), m, dst.data_ptr(),
                                         _stream(torch, dev)) == 0
        torch.cuda.synchronize(dev)
        got = R.bits(dst.cpu().numpy())
        assert np.array_equal(got, R.bits(R.gather_reference(x, dim, rows))), (dim, m)
        assert not np.isin(got, pad_bits).any(), (dim, m)                   # nothing from columns dim .. ldx
        assert R.guards_intact(dst), (dim, m)
        assert np.array_equal(d_rows.cpu().numpy(), rows)
    assert np.array_equal(R.bits(d_x.cpu().numpy()), R.bits(x))            # the source is read only


# ------------------------------------------------------------------------------------------------------------------
# 2. lshrs_gather_tied_rows_f32
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [5, 300])
@pytest.mark.parametrize("cap", [1, 7, 2048, 2049, 5000])
def test_gather_tied_rows_stops_at_the_count_read_on_the_device(cap, dim):
    """Entries (row << 16 | w, mask) with w from {0, 1, 65535} and any 32-bit mask: only the row matters.  EVERY entry of the
    list names a valid row, also those behind the count - what must not happen then is a row of dst written, not a fault."""
    torch, lib, dev = _gpu()
    rng = np.random.default_rng(1000 * dim + cap)
    n, pad = 41, 3
    x = _salted_matrix(rng, n, dim, pad)
    d_x = _up(torch, dev, x)
    rows = rng.integers(0, n, size=cap).astype(np.int64)
    rows[0], rows[-1] = n - 1, 0
    w = rng.choice(np.array([0, 1, 65535], dtype=np.int64), size=cap)
    mask = rng.integers(0, 1 << 32, size=cap, dtype=np.int64)
    mask[0] |= 1 << 31
    mask[-1] = 0xFFFFFFFF
    tie_list = np.stack([(rows << 16) | w, mask], axis=1).reshape(-1)
    d_list = _up(torch, dev, tie_list)
    for count in sorted({0, 1, cap - 1, cap, cap + 5}):
        d_count = _up(torch, dev, np.array([count], np.int32))
        dst = R.guarded(torch, (cap, dim), torch.float32, device=dev)
        assert lib.lshrs_gather_tied_rows_f32(d_x.data_ptr(), dim + pad, dim, d_list.data_ptr(), d_count.data_ptr(), cap,
                                              dst.data_ptr(), _stream(torch, dev)) == 0
        torch.cuda.synchronize(dev)
        got = R.bits(dst.cpu().numpy())
        live_rows, want = R.tied_rows_reference(x, dim, tie_list, count, cap)
        live = len(live_rows)
        assert live == min(count, cap) and np.array_equal(live_rows, rows[:live])
        assert np.array_equal(got[:live], R.bits(want)), (cap, count, dim)
        assert np.all(got[live:] == R.FILL_I32), (cap, count, dim)          # rows at or past the count: as they were filled
        assert R.guards_intact(dst), (cap, count, dim)
        assert int(d_count.cpu()[0]) == count
    assert np.array_equal(d_list.cpu().numpy(), tie_list)


# ------------------------------------------------------------------------------------------------------------------
# 3. lshrs_scatter_band_keys_u8
# ------------------------------------------------------------------------------------------------------------------

_PATCH_TOTALS = (1, 255, 256, 257)


def _patch_counts(nb, bb, n=50):
    """Every m with m * bb in {1, 255, 256, 257} that n * nb distinct (row, band) pairs allow - and, since 257 is prime, the
    multiples of bb on either side of the 256-thread workgroup edge as well."""
    ms = {t // bb for t in _PATCH_TOTALS if t % bb == 0}
    ms |= {255 // bb, 256 // bb, 256 // bb + 1, -(-257 // bb)}
    return sorted(m for m in ms if 1 <= m <= n * nb)


# (6, 1) is not one of the layouts a hasher of this project produces side by side with the others: it is here because it is
# the smallest one-byte layout of 50 rows with 257 distinct (row, band) pairs - m * bb = 255, 256 and 257 all exist for it.
@pytest.mark.parametrize("nb,bb", [(1, 1), (16, 2), (7, 3), (3, 5), (6, 1)])
def test_scatter_band_keys_patches_its_bands_and_nothing_else(nb, bb):
    torch, lib, dev = _gpu()
    rng = np.random.default_rng(100 * nb + bb)
    n = 50
    before = ((np.arange(n * nb * bb, dtype=np.int64) * 7 + 3) & 0xFF).astype(np.uint8).reshape(n, nb, bb)
    counts = _patch_counts(nb, bb)
    assert counts and (nb * n < 257 or any(m * bb <= 256 for m in counts) and any(m * bb > 256 for m in counts))
    if (nb, bb) == (6, 1):
        assert {255, 256, 257} <= set(counts)
    for m in counts:
        pairs = rng.permutation(n * nb)[:m]                                 # distinct (row, band) pairs
        rows, bands = (pairs // nb).astype(np.int64), (pairs % nb).astype(np.int32)
        patch = (before[rows, bands, :].astype(np.int64) + rng.integers(1, 256, size=(m, bb))).astype(np.uint8)
        assert np.all(patch != before[rows, bands, :])                      # every patched byte changes
        keys = R.fill_guarded(torch, R.guarded(torch, (n, nb, bb), offset=1, device=dev), before)
        assert keys.data_ptr() % 2 == 1
        d_rows, d_bands = _up(torch, dev, rows), _up(torch, dev, bands)
        d_patch = R.fill_guarded(torch, R.guarded(torch, (m, bb), offset=3, device=dev), patch)
        assert lib.lshrs_scatter_band_keys_u8(keys.data_ptr(), nb, bb, d_rows.data_ptr(), d_bands.data_ptr(),
                                              d_patch.data_ptr(), m, _stream(torch, dev)) == 0
        torch.cuda.synchronize(dev)
        want = R.scatter_keys_reference(before, rows, bands, patch)
        assert int((want != before).sum()) == m * bb
        assert np.array_equal(keys.cpu().numpy(), want), (nb, bb, m)
        assert R.guards_intact(keys), (nb, bb, m)
        assert np.array_equal(d_patch.cpu().numpy(), patch) and R.guards_intact(d_patch)


# ------------------------------------------------------------------------------------------------------------------
# 4. lshrs_keys_to_hex_u8
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nbytes", [1, 15, 16, 17, 4095, 4096, 4097, 8193])
def test_keys_to_hex_is_bytes_hex_to_the_last_character(nbytes):
    torch, lib, dev = _gpu()
    data = ((np.arange(nbytes, dtype=np.int64) + 0xAF) & 0xFF).astype(np.uint8)     # cycles through all 256 values; the first byte is two letters
    assert nbytes < 256 or len(set(data.tolist())) == 256
    keys = R.fill_guarded(torch, R.guarded(torch, nbytes, offset=1, device=dev), data)
    assert keys.data_ptr() % 2 == 1
    out = R.guarded(torch, 2 * nbytes, device=dev)
    assert lib.lshrs_keys_to_hex_u8(keys.data_ptr(), nbytes, out.data_ptr(), _stream(torch, dev)) == 0
    torch.cuda.synchronize(dev)
    got = out.cpu().numpy().tobytes()
    assert got == data.tobytes().hex().encode()
    assert got == R.hex_reference(data).tobytes()
    assert R.guards_intact(out)                                             # nothing behind hex[2 * nbytes]
    assert np.array_equal(keys.cpu().numpy(), data) and R.guards_intact(keys)


# ------------------------------------------------------------------------------------------------------------------
# 5. lshrs_bucket_histogram_u8 and lshrs_bucket_scatter_u8
# ------------------------------------------------------------------------------------------------------------------

def _bucket_key_sets(rng, n, nb, bb):
    sets = {"random": rng.integers(0, 256, size=(n, nb, bb), dtype=np.uint8)}
    one = np.empty((n, nb, bb), dtype=np.uint8)
    one[:] = np.array([0x5A, 0xC3], dtype=np.uint8)[:bb]                   # one bin per band receives all n
    sets["one-bin"] = one
    if bb == 2:
        alt = np.empty((n, nb, 2), dtype=np.uint8)
        alt[0::2] = np.array([0xFF, 0x00], dtype=np.uint8)                  # key 0x00ff: its low byte comes first
        alt[1::2] = np.array([0x00, 0xFF], dtype=np.uint8)                  # key 0xff00
        sets["byte-order"] = alt
    return sets


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
@pytest.mark.parametrize("nb", [1, 16, 33])
@pytest.mark.parametrize("bb", [1, 2])
def test_bucket_histogram_and_scatter_fill_every_bin(bb, nb, n):
    torch, lib, dev = _gpu()
    rng = np.random.default_rng(10000 * bb + 100 * nb + n)
    nbins = nb << (8 * bb)
    ids = rng.integers(0, 1 << 40, size=n, dtype=np.int64)
    ids[1::2] = (1 << 62) - 1 - rng.integers(0, 1000, size=len(ids[1::2]))  # near 2^62
    if n > 1:
        ids[-1] = ids[0]                                                    # one id on two rows
    d_ids = _up(torch, dev, ids)
    stream = _stream(torch, dev)
    for name, keys in _bucket_key_sets(rng, n, nb, bb).items():
        what = (name, bb, nb, n)
        want_counts, want_members = R.bucket_reference(keys, ids)
        if name == "one-bin":
            assert len(want_members) == nb and all(len(v) == n for v in want_members.values())
        if name == "byte-order":                                            # by construction, not through the reference
            for b in range(nb):
                assert want_counts[(b << 16) | 0x00FF] == (n + 1) // 2 and want_counts[(b << 16) | 0xFF00] == n // 2
        d_keys = R.fill_guarded(torch, R.guarded(torch, (n, nb, bb), offset=1, device=dev), keys)
        counts = R.guarded(torch, nbins, torch.int32, device=dev).zero_()
        assert lib.lshrs_bucket_histogram_u8(d_keys.data_ptr(), n, nb, bb, counts.data_ptr(), stream) == 0
        torch.cuda.synchronize(dev)
        got_counts = counts.cpu().numpy()
        assert np.array_equal(got_counts, want_counts), what               # all bins
        offsets = np.r_[0, np.cumsum(got_counts.astype(np.int64))[:-1]].astype(np.int64)
        d_offsets = _up(torch, dev, offsets)
        cursors = R.guarded(torch, nbins, torch.int32, device=dev).zero_()
        members = R.guarded(torch, n * nb, torch.int64, device=dev)
        assert lib.lshrs_bucket_scatter_u8(d_keys.data_ptr(), d_ids.data_ptr(), n, nb, bb, d_offsets.data_ptr(),
                                           cursors.data_ptr(), members.data_ptr(), stream) == 0
        torch.cuda.synchronize(dev)
        got_members = members.cpu().numpy()
        # every bin's slice, sorted: the slices are contiguous and in bin order, so sorting by (bin of the slot, id) sorts
        # each slice in place; the reference laid out the same way
        slot_bin = np.repeat(np.arange(nbins, dtype=np.int64), want_counts)
        assert len(slot_bin) == n * nb
        got_sorted = got_members[np.lexsort((got_members, slot_bin))]
        want_flat = np.fromiter((i for b in sorted(want_members) for i in want_members[b]), dtype=np.int64, count=n * nb)
        assert np.array_equal(got_sorted, want_flat), what
        for b in list(want_members)[:50]:                                   # and a few bins as the header words it
            lo = int(offsets[b])
            assert sorted(got_members[lo:lo + int(got_counts[b])].tolist()) == want_members[b], (what, b)
        assert np.array_equal(cursors.cpu().numpy(), want_counts), what    # cursors end equal to counts
        assert np.array_equal(counts.cpu().numpy(), want_counts), what     # (the scatter leaves counts alone)
        assert R.guards_intact(members) and R.guards_intact(counts) and R.guards_intact(cursors), what
        assert np.array_equal(d_keys.cpu().numpy(), keys) and R.guards_intact(d_keys), what


# ------------------------------------------------------------------------------------------------------------------
# 6. lshrs_l2_normalize_f32
# ------------------------------------------------------------------------------------------------------------------

L2_DIMS = [1, 3, 255, 256, 257, 1000]


def _l2_run(torch, lib, dev, x, dim, with_status=True):
    """One launch on x (n, ldx) -> (out (n, dim) as a host array, status or None); the guards of both checked."""
    n, ldx = x.shape
    d_x = _up(torch, dev, x)
    out = R.guarded(torch, (n, dim), torch.float32, device=dev)
    status = R.guarded(torch, n, device=dev) if with_status else None
    assert lib.lshrs_l2_normalize_f32(d_x.data_ptr(), n, ldx, dim, out.data_ptr(),
                                      status.data_ptr() if with_status else None, _stream(torch, dev)) == 0
    torch.cuda.synchronize(dev)
    assert R.guards_intact(out)
    assert status is None or R.guards_intact(status)
    assert np.array_equal(R.bits(d_x.cpu().numpy()), R.bits(x))
    return out.cpu().numpy(), (status.cpu().numpy() if with_status else None)


@pytest.mark.parametrize("dim", L2_DIMS)
def test_l2_normalize_is_within_its_derived_bound_of_float64(dim):
    """Largest |out - reference| / |reference| measured on an MI355X, in units of 2^-24, against l2_tolerance(dim):
    1-d 0 (9), 3-d 1.30 (9), 255-d 2.05 (9), 256-d 1.79 (9), 257-d 1.43 (9.5), 1000-d 1.69 (10.5)."""
    torch, lib, dev = _gpu()
    rng = np.random.default_rng(dim)
    n, pad = 9, 5
    x = np.full((n, dim + pad), 1e30, dtype=np.float32)                     # (the columns behind dim: a sum that took one in is off by far)
    scale = (10.0 ** rng.uniform(-2.0, 2.0, size=n)).astype(np.float32)     # every row its own factor from [0.01, 100]
    x[:, :dim] = rng.standard_normal((n, dim)).astype(np.float32) * scale[:, None]
    x[[2, 7], :dim] = 0.0
    x[7, 0] = -0.0
    out, status = _l2_run(torch, lib, dev, x, dim)
    zero = np.zeros(n, dtype=bool)
    zero[[2, 7]] = True
    assert np.array_equal(status, zero.astype(np.uint8))
    ref = R.l2_reference(x[:, :dim])
    live = ~zero
    assert np.all(np.isfinite(ref[live])) and np.all(ref[live] != 0.0)
    err = np.abs(out[live].astype(np.float64) - ref[live]) / np.abs(ref[live])
    tol = R.l2_tolerance(dim)
    print(f"l2_normalize dim={dim}: largest relative error {err.max() * 2 ** 24:.3f} * 2^-24, bound {tol * 2 ** 24:.1f} * 2^-24")
    assert err.max() <= tol, (dim, float(err.max()), tol)
    # status = NULL is accepted, and changes nothing
    again, none = _l2_run(torch, lib, dev, x, dim, with_status=False)
    assert none is None and np.array_equal(R.bits(again[live]), R.bits(out[live]))


@pytest.mark.parametrize("dim", L2_DIMS)
def test_l2_normalize_is_exactly_scale_invariant(dim):
    """Rows with every |x| in [2^-12, 2^4], and the same rows times 2^40 and times 2^-40: squares, sums, root and quotient
    all stay normal numbers (2^-104 <= x^2, sums below 2^98), so every operation of the scaled runs is the unscaled one with
    another exponent and the outputs agree bit for bit.  The only check here at norms far from 1."""
    torch, lib, dev = _gpu()
    rng = np.random.default_rng(77 + dim)
    n, pad = 9, 5
    x = np.full((n, dim + pad), 3.0, dtype=np.float32)
    x[:, :dim] = (np.exp2(rng.uniform(-12.0, 4.0, size=(n, dim))) * rng.choice([-1.0, 1.0], size=(n, dim))).astype(np.float32)
    assert np.all(np.abs(x[:, :dim]) >= 2.0 ** -12) and np.all(np.abs(x[:, :dim]) <= 2.0 ** 4)
    base, status = _l2_run(torch, lib, dev, x, dim)
    assert not status.any()
    ref = R.l2_reference(x[:, :dim])
    assert (np.abs(base.astype(np.float64) - ref) <= R.l2_tolerance(dim) * np.abs(ref)).all()
    for e in (40, -40):
        scaled = np.ldexp(x, e).astype(np.float32)
        assert np.array_equal(np.ldexp(scaled.astype(np.float64), -e), x.astype(np.float64))       # exact
        out, status = _l2_run(torch, lib, dev, scaled, dim)
        assert not status.any()
        assert np.array_equal(R.bits(out), R.bits(base)), (dim, e)


# ------------------------------------------------------------------------------------------------------------------
# 7. lshrs_topk_desc_f32
# ------------------------------------------------------------------------------------------------------------------

TOPK_C = sorted({1, 2, 3} | {c for p in range(2, 15) for c in ((1 << p) - 1, 1 << p, (1 << p) + 1) if c <= 16384})


def _topk_rows(rng, c, q):
    """Rows of different kinds: special_scores (exact ties, both zeros, both NaNs, both infinities), all entries equal, a
    strictly ascending ramp (the network has to turn it round)."""
    rows = [R.special_scores(rng, c), np.full(c, 0.25, dtype=np.float32), np.arange(c, dtype=np.float32) - np.float32(c // 2)]
    assert np.all(np.diff(rows[2]) > 0)
    return np.stack(rows[:q]) if q == 3 else np.stack([rows[0], rows[2]])


def _topk_check(torch, lib, dev, scores, models, k, workspace=None):
    q, c = scores.shape
    d_scores = _up(torch, dev, scores)
    order = R.guarded(torch, (q, k), torch.int32, device=dev)
    srt = R.guarded(torch, (q, k), torch.float32, device=dev)
    rc = lib.lshrs_topk_desc_f32(d_scores.data_ptr(), q, c, k, order.data_ptr(), srt.data_ptr(),
                                 workspace.data_ptr() if workspace is not None else None, _stream(torch, dev))
    assert rc == 0, (rc, c, k)
    torch.cuda.synchronize(dev)
    got_order, got_sorted = order.cpu().numpy(), srt.cpu().numpy()
    for qi in range(q):
        want = np.asarray(models[qi][:k], dtype=np.int32)
        assert np.array_equal(got_order[qi], want), (c, k, qi)
        assert np.array_equal(R.bits(got_sorted[qi]), R.bits(scores[qi][want])), (c, k, qi)
    assert R.guards_intact(order) and R.guards_intact(srt), (c, k)         # k < c: nothing past q * k in either output
    assert workspace is None or R.guards_intact(workspace), (c, k)
    assert np.array_equal(R.bits(d_scores.cpu().numpy()), R.bits(scores))


@pytest.mark.parametrize("c", TOPK_C)
def test_topk_lds_network_obeys_the_rank_model_at_every_size(c):
    torch, lib, dev = _gpu()
    rng = np.random.default_rng(c)
    scores = _topk_rows(rng, c, 3)
    models = [R.rank_model(row) for row in scores]
    assert models[1] == list(range(c)) and models[2] == list(range(c - 1, -1, -1))
    for k in sorted({1, c // 2, c} - {0}):
        _topk_check(torch, lib, dev, scores, models, k)                     # workspace = NULL throughout


def test_topk_global_network_obeys_the_same_model():
    """c = 16385: the first length the LDS network does not take - the same kind of rows through the network in global
    memory, its workspace between guards."""
    torch, lib, dev = _gpu()
    rng = np.random.default_rng(16385)
    c, q = 16385, 2
    scores = _topk_rows(rng, c, q)
    models = [R.rank_model(row) for row in scores]
    nbytes = lib.lshrs_topk_workspace_bytes(q, c)
    assert nbytes == q * 32768 * 8
    for k in (1, c):
        workspace = R.guarded(torch, nbytes, device=dev)
        assert workspace.data_ptr() % 8 == 0
        _topk_check(torch, lib, dev, scores, models, k, workspace=workspace)
