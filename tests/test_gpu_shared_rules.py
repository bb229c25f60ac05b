"""GPU tests of the stage-1 rules the signature kernels share (csrc/lshrs_common.h) that a comparison of keys alone does not
notice: the range guard of the row window (`window_hi`) and the value that travels with a list entry (`ykeep`).  A wrong
guard costs a key bit only where a near-tie of such a row falls outside the window; a wrong `ykeep` only moves a statistic.
Both are contracts of the list stage 1 leaves for stage 2, so the list itself is read here."""

from __future__ import annotations

import numpy as np
import pytest

from tests._list_reference import S1_LIST, S1_VALUES, AUDIT_ENTRIES, AUDIT_VALUES

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@gpu
@pytest.mark.parametrize("nb,r,dim", [(16, 4, 128),       # sig16r_kernel (resident image)
                                      (16, 16, 288)])     # sig16_kernel, one plain list (stage2_sorted off)
def test_rows_outside_the_guarded_range_are_flagged_wholesale_and_carry_no_stage1_value(torch_mod, nb, r, dim):
    """A row whose largest |x| lies outside [2^-32, 2^32]: EVERY key column of it is in stage 1's list (stage 2 decides the
    whole row) and its entries carry NaN instead of a stage-1 value; every other entry carries a finite one.  Keys and row
    flags are those of the exact-f32 pass with the same tie replay, bit for bit."""
    torch = torch_mod
    from lshrs_amd import LSHHasher

    kw = {"reference_blas": "openblas-haswell"}          # (the device replay whatever this host's BLAS is)
    h = LSHHasher(num_bands=nb, rows_per_band=r, dim=dim, seed=7, **kw)
    h.stage2_sorted = False
    f32 = LSHHasher(num_bands=nb, rows_per_band=r, dim=dim, seed=7, precision="f32", **kw)
    n, big, small = 3_000, 8, 9
    x = np.random.default_rng(11).standard_normal((n, dim)).astype(np.float32)
    x[big] *= np.float32(2.0 ** 40)
    x[small] *= np.float32(2.0 ** -40)
    xd = torch.from_numpy(x).cuda()
    flags = torch.zeros(n, dtype=torch.uint8, device="cuda")
    got = h.hash_device(xd, row_flags=flags)
    st = dict(h.last_stats)
    assert st["route"] == "split+replay" and st["tie_break_engine"] == "device-replay" and st["relaunches"] == 0, st
    fl32 = torch.zeros(n, dtype=torch.uint8, device="cuda")
    assert torch.equal(got, f32.hash_device(xd, row_flags=fl32)) and torch.equal(flags, fl32)

    (scratch,) = h._replay_scratch.values()                # (one stream: one list)
    k = int(st["flagged"])
    items = scratch[S1_LIST][:k].cpu().numpy()
    y1 = scratch[S1_VALUES][:k].cpu().numpy()
    rows, cols = items >> 21, items & ((1 << 21) - 1)
    key_cols = {b * 8 * h.band_bytes + j for b in range(nb) for j in range(r)}
    for row in (big, small):
        mine = rows == row
        assert key_cols <= set(cols[mine].tolist()), (row, int(mine.sum()))
        assert np.isnan(y1[mine]).all(), row
    rest = (rows != big) & (rows != small)
    print(f"{nb} x {r} x {dim}: {k} entries, {int(rest.sum())} of them from rows inside the range")
    assert rest.any() and np.isfinite(y1[rest]).all()


@gpu
@pytest.mark.parametrize("nb,r,dim,exact", [(16, 4, 128, True),       # sig16r_kernel
                                            (16, 16, 288, False)])    # sig16_kernel
def test_the_window_of_a_sampled_projection_is_the_proven_one_widened_by_a_thousandth(torch_mod, nb, r, dim, exact):
    """The audit sample carries the window stage 1 compared each sampled projection with: it must be
    1.001 (||x_hi|| coef_a[j] + ||x_mid|| coef_b[j]) with x_hi = bf16(x), x_mid = bf16(x - x_hi), the norms taken in float64
    here.  Tolerance 1e-4 of the ratio: stage 1 sums the squares in f32 (at most dim 2^-24 = 1.7e-5 relative at 288 elements,
    halved by the root) and rounds a root, three products and a sum (2^-24 each) - and a factor of 1.0 would be 1e-3 away.
    sig16r_kernel's windows are that value.  sig16_kernel splits the clamped prefetch behind the last k-tile like a tile (two
    thirds of it) and so adds squares of the row's last 32 elements a second time: its windows come out 1.002 .. 1.10 times
    the proven one here and are held from below only - never narrower."""
    torch = torch_mod
    from lshrs_amd import LSHHasher

    h = LSHHasher(num_bands=nb, rows_per_band=r, dim=dim, seed=7, reference_blas="openblas-haswell")
    h.stage2_sorted = False
    x = torch.from_numpy(np.random.default_rng(12).standard_normal((3_000, dim)).astype(np.float32)).cuda()
    h.hash_device(x)
    (scratch,) = h._replay_scratch.values()
    scratch[AUDIT_ENTRIES].fill_(-1)                                  # (slots no unit of the next launch writes stay empty)
    h.hash_device(x)
    st = dict(h.last_stats)
    assert st["route"] == "split+replay" and st["window"] == "proven" and st["audited_unflagged"] > 0, st
    items = scratch[AUDIT_ENTRIES].cpu().numpy()
    vals = scratch[AUDIT_VALUES].cpu().numpy().reshape(-1, 2)[:items.size]
    live = items >= 0
    assert int(live.sum()) >= st["audited_unflagged"]
    rows, cols = items[live] >> 21, items[live] & ((1 << 21) - 1)
    band, j = cols // (8 * h.band_bytes), cols % (8 * h.band_bytes)
    assert (j < r).all()
    (coef, _info), = h._window_coef_cache.values()
    ca, cb = coef[0].astype(np.float64)[band * r + j], coef[1].astype(np.float64)[band * r + j]
    xs = x.cpu()[torch.from_numpy(rows)]
    hi = xs.to(torch.bfloat16).to(torch.float32)
    mid = (xs - hi).to(torch.bfloat16).to(torch.float32)
    nh, nm = hi.double().norm(dim=1).numpy(), mid.double().norm(dim=1).numpy()
    ratio = vals[live, 1].astype(np.float64) / (nh * ca + nm * cb)
    print(f"{nb} x {r} x {dim}: {int(live.sum())} sampled windows, ratio {ratio.min():.6f} .. {ratio.max():.6f}")
    assert ratio.min() > 1.001 - 1e-4
    assert not exact or ratio.max() < 1.001 + 1e-4
