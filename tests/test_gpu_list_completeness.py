"""GPU tests that the lists the signature kernels leave for the exact decision are COMPLETE: every projection inside its window
is in stage 1's flag list (split pass: sig16_kernel, sig16r_kernel) or in the tie list (f32 pass: sig_kernel), nothing outside
it is, nothing twice.  A dropped entry costs a key bit only where the fast sign also happens to be wrong - once in many
millions of random projections - so no comparison of keys notices a kernel that loses entries; the lists are read here and
judged by the CPU models (tests/_list_reference.py: how the inputs get their power, and the float64 judge).

What lies between "value computed" and "entry in the list": the wave-uniform screen (a maximum per column block, built per
layout - padded blocks, the fine geometry, the narrow slot, compact blocks, the resident image - by lshrs_sig_pack_projections
and again by lshrs_sig_set_window; with a caller's window, the norms' maxima instead), the exact test and its `hits` mask,
the column ids through the tables, the LDS stage and what happens when it is full, the flush, the bucket segments.
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import _list_reference as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _hasher(c, nb, r, dim, form):
    from lshrs_amd import LSHHasher

    kw = {"reference_blas": L.REFERENCE_BLAS}                 # (the device replay whatever this host's BLAS is)
    if form == "tau1":                                        # a caller's window the hasher keeps: no guard, no audit to replace it
        kw.update(tau1_ulps=L.TAU1_UNITS, margin_guard=0.0, audit_unflagged=0)
    h = LSHHasher(num_bands=nb, rows_per_band=r, dim=dim, seed=L.HASHER_SEED, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(h.projections, L.gaussian_planes(nb, r, dim)))
    h.projections = [p.copy() for p in c.planes]              # (as test_split_window_margin_with_assigned_hyperplanes assigns them)
    assert h._replay_model() == c.model
    return h


def _expected_keys_check(h, c, keys0, dim):
    """The keys of the batch are the reference's (oracle/lshrs_oracle.py's literal loop).  On a host whose own BLAS is not the
    build the hasher is pinned to, the two may round a projection within a few units of zero to different sides: there the
    bits of projections below 16 units of 2^-24 ||x|| ||p|| are left out (summation orders differ by sqrt(dim)/4 units or so)."""
    from oracle.lshrs_oracle import hash_batch_literal_packed

    want = hash_batch_literal_packed(c.planes, c.x)
    if h._host_blas_agrees():
        assert np.array_equal(keys0, want)
        return
    nb, r = h.num_bands, h.rows_per_band
    P = np.concatenate(c.planes).astype(np.float64)
    with np.errstate(all="ignore"):
        x64 = c.x.astype(np.float64)
        near = ~(np.abs(x64 @ P.T) > 16 * L.U * np.sqrt((x64 * x64).sum(1))[:, None] * c.pnorm)
    near[np.isnan(c.x).any(axis=1)] = False                   # (a NaN row: every bit 0 on any host)
    bits = lambda k: np.unpackbits(k, axis=2, bitorder="little")[:, :, :r].reshape(k.shape[0], nb * r)
    assert near.mean() < 0.02
    assert np.array_equal(bits(keys0)[~near], bits(want)[~near])


def _run_split(torch, nb, r, dim, layout, form, copies=1, buckets=False):
    c = L.split_case(nb, r, dim, layout, form)
    g = L.sig16_layout(nb, r, dim)
    must_not = c.must_not if g["resident"] else c.must_not16
    n0, ncols = c.must.shape
    n = n0 * copies
    h = _hasher(c, nb, r, dim, form)
    h.stage2_sorted = "buckets" if buckets else False
    assert h._stage2_mode() == (1 if buckets else None)
    assert h._resident_shape() == g["resident"]
    if not h._split_applies(n, replay=True):
        # 192 key columns below 384-d: the hasher's plan keeps them on the f32 kernel (it is faster there); the library's split pass
        # takes them, and it is the only shape on which the narrow slot sits behind TWO column blocks of the main geometry
        assert (nb, r, dim) == (24, 8, 300) and g["narrow"] and g["cb"] == 2
        h._split_shape_ok = (h._projection_version, True)
        assert h._split_applies(n, replay=True)
    # room for everything the judge does not rule out (+ the NaN row's padding columns), so that no pass is repeated for room
    h._flag_cap_hint = copies * (int((~must_not).sum()) + 1024) + 4096
    xd = torch.from_numpy(np.tile(c.x, (copies, 1))).cuda()
    keys = h.hash_device(xd)
    st = dict(h.last_stats)
    assert st["route"] == "split+replay" and st["tie_break_engine"] == "device-replay", st
    if form == "proven":
        assert st["window"] == "proven", st
        (coef, _info), = h._window_coef_cache.values()        # what the hasher handed to lshrs_sig_set_window
        assert np.array_equal(coef, c.coef)
    else:
        assert st["window"] == "measured" and st["tau1_ulps"] == L.TAU1_UNITS and h.window_mode["tau1"] == "measured", st

    padcols = g["padcols"]
    keyidx = np.full(1 << L.ENTRY_COL_BITS, -1, dtype=np.int64)
    keyidx[c.key_cols] = np.arange(ncols)
    if buckets:
        # a pass may be repeated ONCE for segment room (a column outgrew its segment); the list is the repeated pass's
        assert st["relaunches"] <= 1 and (st["relaunches"] == 0 or h._bucket_cap_hint > 0), st
        entries, vals, seg_col, counts, per = L.bucket_lists(h, padcols)
        assert (counts <= per).all()
        rows, cols = L.entry_rows_cols(entries)
        assert np.array_equal(cols, seg_col)                  # every entry sits in its own column's segment
        sample = (entries & L.AUDIT_BIT) != 0
        assert (keyidx[cols] >= 0).all()                      # (no segment for a padding column)
        if form == "proven":
            assert st["audited_unflagged"] > 0 and int(sample.sum()) >= st["audited_unflagged"]
        else:
            assert not sample.any()
    else:
        assert st["relaunches"] == 0, st
        entries, vals = L.stage1_list(L.only_scratch(h), int(st["flagged"]))
        rows, cols = L.entry_rows_cols(entries)
        sample = np.zeros(entries.size, dtype=bool)
        assert (entries >= 0).all() and (entries & L.AUDIT_BIT == 0).all() and (rows < n).all()
        assert np.unique(entries).size == entries.size        # nothing twice, the padding columns included
        # a padding column: only the NaN row's, only in the padded layouts (0 * NaN; stage 2 skips them)
        pad = keyidx[cols] < 0
        assert (cols < max(256, padcols)).all()
        if g["compact"] or g["resident"]:
            assert not pad.any()
        nan_row = int(np.flatnonzero(np.isnan(c.x).any(axis=1))[0])
        assert ((rows[pad] % n0) == nan_row).all() and np.isnan(vals[pad]).all()
        entries, vals, rows, cols, sample = entries[~pad], vals[~pad], rows[~pad], cols[~pad], sample[~pad]
        assert int(st["flagged"]) == entries.size + int(pad.sum())
    assert (rows >= 0).all() and (rows < n).all()
    # nothing twice - and a sample is never also a flag (entries without the mark are compared)
    plain = entries & ~np.int64(L.AUDIT_BIT)
    assert np.unique(plain).size == plain.size
    flag = ~sample
    assert int(st["flagged"]) >= int(flag.sum()) and (buckets is False or int(st["flagged"]) == int(flag.sum()))
    got = np.zeros((copies, n0, ncols), dtype=bool)
    got[rows[flag] // n0, rows[flag] % n0, keyidx[cols[flag]]] = True
    missing = np.argwhere(c.must[None] & ~got)
    extra = np.argwhere(must_not[None] & got)
    print(f"{nb} x {r} x {dim} {layout} {form} x{copies}{' buckets' if buckets else ''}: {int(flag.sum())} flagged, must "
          f"{int(c.must.sum())}, undecided {int((~c.must & ~must_not).sum())}, missing {len(missing)}, extra {len(extra)}, "
          f"relaunches {st['relaunches']}")
    assert len(missing) == 0, (missing[:8], [(float(c.y1[i, j]), float(c.W[i, j])) for _, i, j in missing[:8]])
    assert len(extra) == 0, (extra[:8], [(float(c.y1[i, j]), float(c.W_up[i, j])) for _, i, j in extra[:8]])
    # the value beside every entry: the accumulator model's, bit for bit; NaN for a row flagged wholesale
    r0, k0 = rows % n0, keyidx[cols]
    whole = c.wholesale[r0]
    assert np.isnan(vals[whole]).all() and not sample[whole].any()
    assert np.array_equal(vals[~whole].view(np.uint32), c.y1[r0[~whole], k0[~whole]].view(np.uint32))
    # the keys: every copy the same, and the reference's
    kh = keys.cpu().numpy().reshape(copies, n0, nb, h.band_bytes)
    assert (kh == kh[:1]).all()
    _expected_keys_check(h, c, kh[0], dim)
    return c, g, st


@pytest.mark.parametrize("nb,r,dim,layout,form", L.split_params(L.SIG16_SHAPES))
def test_sig16_kernel_flags_every_projection_inside_its_window(torch_mod, nb, r, dim, layout, form):
    """sig16_kernel<COMPACT, PARTIAL, 4> (128-row workgroups) on every layout of its tables - padded blocks (one, two), compact
    blocks (one, two, a partial tile), the narrow slot (128 and 192 key columns) -, proven window and a caller's 300 units, plain list.
    must: |y1| <= (1 - eps) W, with y1 the accumulator model's value and W the window in float64.  must not: |y1| > (1 + eps) W_up,
    where W_up counts the squares of the row's last 32 elements once more in both norms: the kernel splits the clamped prefetch
    behind the last k-tile like a tile for the first two thirds of its slices, which (read in sig16.hip: `split_step` slices 0 ..
    15 in the last stage) adds the last k-tile's elements once more for the first of a wave's two 16-row tiles and two of every
    eight of them for the second - never more than W_up, which is therefore the most a window can be.
    The cases whose first 128 rows want more than kS1ListCap = 4096 entries of one column block run the append's overflow branch."""
    c, g, st = _run_split(torch_mod, nb, r, dim, layout, form)
    bpb = g["compact"][0] if g["compact"] else 0
    wants = int(L.workgroup_wants(c, 128, bpb, nb, r).max())
    assert (wants > L.S1_LIST_CAP[4]) == ((nb, r, dim) in L.S1_OVERFLOW_SHAPES), wants


@pytest.mark.parametrize("nb,r,dim,layout,form", L.split_params(L.SIG16_W8_SHAPES))
def test_sig16_kernel_256_row_workgroups_flag_every_projection_inside_its_window(torch_mod, nb, r, dim, layout, form):
    """sig16_kernel<., ., 8>: more than 11 k-tiles and more than 128 groups of 256 rows - the rows 66 times over, every copy
    judged against the one model (padded and compact blocks, an odd and an even number of k-tiles)."""
    g = L.sig16_layout(nb, r, dim)
    n = L.split_case(nb, r, dim, layout, form).x.shape[0] * L.W8_COPIES
    ncb = g["compact"][1] if g["compact"] else g["cb"]
    assert g["ktiles"] > 11 and -(-n // 256) * ncb > 128      # sig16_half_rows (sig_split.hip) restated: neither rule gives 128 rows
    _run_split(torch_mod, nb, r, dim, layout, form, copies=L.W8_COPIES)


@pytest.mark.parametrize("nb,r,dim,layout,form", L.split_params(L.SIG16R_SHAPES))
def test_sig16r_kernel_flags_every_projection_inside_its_window(torch_mod, nb, r, dim, layout, form):
    """sig16r_kernel<NCT, KT> for 4 .. 16 column tiles and 2, 4, 8 k-tiles (one and two row tiles per wave, a partial k-tile):
    its window is the proven one (W_up = W), its per-wave list stage holds 64 entries and is outgrown by every wave that holds
    a row flagged wholesale."""
    _run_split(torch_mod, nb, r, dim, layout, form)


@pytest.mark.parametrize("nb,r,dim,layout,form", L.split_params(L.BUCKET_SHAPES))
def test_bucket_segments_hold_every_projection_inside_its_window(torch_mod, nb, r, dim, layout, form):
    """stage2_sorted="buckets" (what "auto" gives long rows): the same verdicts on the segments stage 1 fills per key column -
    the staged entries' flush, the overflow branch straight to the segments, the audit-marked samples beside them."""
    _run_split(torch_mod, nb, r, dim, layout, form, buckets=True)


@pytest.mark.parametrize("nb,r,dim,layout,form", L.f32_params())
def test_sig_kernel_lists_every_projection_inside_the_tie_window(torch_mod, nb, r, dim, layout, form):
    """lshrs_sig_hash_batch_f32 with a tie list: every |y| < W is in it (y: the fmaf chain, to which lshrs_sig_project_f32 is
    pinned bit for bit; W = tau ||x|| ||p_j|| with tau = 256 x 2^-24, or ||x|| coef_tie[j] with LSHRS_WINDOW_PROVEN), nothing
    outside it is.  NT = 8, 4, 2, 1 of the main geometry (its screen: `wtmax` / `norm_max` per column block), the fine geometry
    (`wtmax_fine` / the fine image's `norm_max` per 32-column tile) at 512 rows of 768 elements, and rows of 301 elements at
    an odd 4-byte address."""
    torch = torch_mod
    from lshrs_amd import LSHHasher, _native
    from oracle.build import chain_hash_packed

    c = L.f32_case(nb, r, dim, layout, form)
    n, ncols = c.must.shape
    # the geometry this batch takes: sig_prefer_fine's formula restated, so that a change of plan cannot quietly move the case
    g = L.sig16_layout(nb, r, dim)
    layers = float(((n + 127) // 128 * g["cb"] + 255) // 256)
    fine = g["nt"] > 1 and 30.0 + 2.3e-5 * n * g["tiles32"] * g["ktiles"] < layers * (4.4 * g["ktiles"] + 10.0)
    assert fine == (dim in (301, 768)) and fine == L.prefers_fine(nb, r, dim, n)
    h = LSHHasher(num_bands=nb, rows_per_band=r, dim=dim, seed=L.HASHER_SEED, reference_blas=L.REFERENCE_BLAS, precision="f32")
    h.projections = [p.copy() for p in c.planes]
    lib = _native.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    ws = h._workspace(dev)
    h._ensure_window(dev, ws, c.model)
    (coef, _info), = h._window_coef_cache.values()
    assert np.array_equal(coef, c.coef)
    if dim % 4:                                               # rows at an odd 4-byte address
        buf = torch.zeros(n * dim + 1, dtype=torch.float32, device=dev)
        xd = buf[1:].view(n, dim)
        xd.copy_(torch.from_numpy(c.x.copy()))
        assert xd.data_ptr() % 8 == 4
    else:
        xd = torch.from_numpy(c.x.copy()).to(dev)
    cap = 4096
    ties = torch.zeros((cap, 2), dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    keys = torch.empty((n, nb, h.band_bytes), dtype=torch.uint8, device=dev)
    tau = 0.0 if form == "proven" else L.TAU_UNITS * L.U      # (0: LSHRS_WINDOW_PROVEN)
    _native.check(lib.lshrs_sig_hash_batch_f32(xd.data_ptr(), n, xd.stride(0), ws.data_ptr(), nb, r, dim, keys.data_ptr(),
                                               ties.data_ptr(), cap, count.data_ptr(), tau, None, None,
                                               torch.cuda.current_stream(dev).cuda_stream), "lshrs_sig_hash_batch_f32")
    torch.cuda.current_stream(dev).synchronize()
    k = int(count.item())
    assert 0 < k <= cap
    t = ties.cpu().numpy()
    assert not t[k:].any()                                    # tie_count IS the number of entries written
    rows, words, masks = t[:k, 0] >> 16, t[:k, 0] & 0xFFFF, t[:k, 1]
    assert (rows >= 0).all() and (rows < n).all() and (words < -(-g["padcols"] // 32)).all()
    assert (masks > 0).all() and (masks < (1 << 32)).all()
    assert np.unique(t[:k, 0]).size == k                      # no word twice for a row
    iskey = np.zeros(32 * (int(words.max()) + 1 + g["padcols"] // 32), dtype=bool)
    iskey[c.key_cols] = True
    keyidx = np.cumsum(iskey) - 1
    got = np.zeros((n, ncols), dtype=bool)
    for b in range(32):
        hit = (masks >> b) & 1 == 1
        col = 32 * words[hit] + b
        assert iskey[col].all(), (b, col[~iskey[col]][:4])    # no mask bit on a padding column
        got[rows[hit], keyidx[col]] = True
    missing, extra = np.argwhere(c.must & ~got), np.argwhere(c.must_not & got)
    print(f"{nb} x {r} x {dim} {layout} {form}: {k} entries, {int(got.sum())} projections, must {int(c.must.sum())}, undecided "
          f"{int((~c.must & ~c.must_not).sum())}, missing {len(missing)}, extra {len(extra)}, {'fine' if fine else 'main'} geometry")
    assert len(missing) == 0, (missing[:8], [(float(c.y[i, j]), float(c.W[i, j])) for i, j in missing[:8]])
    assert len(extra) == 0, (extra[:8], [(float(c.y[i, j]), float(c.W[i, j])) for i, j in extra[:8]])
    assert np.array_equal(keys.cpu().numpy(), chain_hash_packed(c.planes, c.x))
