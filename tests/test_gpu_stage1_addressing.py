"""Stage 1's LDS-DMA goes through two buffer descriptors per workgroup (sig16.hip: the fragment image of the column block, and
exactly the bytes of x the workgroup may touch) with the lane offsets as 32-bit values and the stage / k-tile advance as a
scalar.  What that addressing can get wrong shows as wrong keys: a last workgroup with ONE valid row (its descriptor covers one
row, every other lane is clamped onto it) on both workgroup shapes, rows that are a strided view (the row stride is not the
vector length, the base is not the allocation's), a row slice that starts at an odd row, compact column blocks and a partial
last k-tile.  Every case compares the keys of ALL rows with the reference-literal loop on the same array - never with another
device path - and none reaches outside its tensor."""

from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAST_ROW_ALONE = 129 * 256 + 1     # 33 025 rows: more than 128 workgroups of 256 rows (so that long vectors take that shape), the last one with one row


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


_cases: dict = {}


def _case(torch, nb, r, dim, n):
    """-> (hasher, parent tensor of (n + 3, dim + 64), the reference's keys of its view [3:, 32:32 + dim]); made once per shape.
    The parent is poisoned around the view: NaN behind every row's end and in the rows in front, Inf in the columns in front."""
    key = (nb, r, dim, n)
    if key not in _cases:
        from lshrs_amd import LSHHasher
        from oracle.lshrs_oracle import hash_batch_literal_packed

        h = LSHHasher(num_bands=nb, rows_per_band=r, dim=dim, seed=31)
        big = torch.randn(n + 3, dim + 64, device="cuda", generator=torch.Generator("cuda").manual_seed(dim + n))
        big[:, dim + 32:] = float("nan")
        big[:, :32] = float("inf")
        big[:3] = float("nan")
        want = hash_batch_literal_packed(h.projections, big[3:, 32:32 + dim].cpu().numpy())
        want.setflags(write=False)
        _cases[key] = (h, big, want)
    return _cases[key]


def _check(h, x, want):
    got = h.hash_device(x)
    if h._replay_model():            # (the host BLAS's summation order is one the replay knows: the split pass with its own stage 2)
        assert h.last_stats["route"] == "split+replay", h.last_stats
    bad = np.flatnonzero((got.cpu().numpy() != want).any(axis=(1, 2)))
    assert bad.size == 0, (bad[:8], bad.size, h.last_stats)


@pytest.mark.parametrize("nb,r,dim", [(16, 16, 384), (16, 16, 768), (20, 10, 768), (16, 16, 429)])
def test_last_workgroup_of_256_rows_with_one_valid_row(torch_mod, nb, r, dim):
    """33 025 rows: 129 full workgroups of 256 rows and one with a single row - twelve k-tiles (the shortest vectors that take
    this shape), 768-d, compact column blocks (20 x 10) and a partial last k-tile (429-d)."""
    h, big, want = _case(torch_mod, nb, r, dim, LAST_ROW_ALONE)
    _check(h, big[3:, 32:32 + dim].contiguous(), want)


@pytest.mark.parametrize("n", [257, 385])
def test_last_workgroup_of_128_rows_with_one_valid_row(torch_mod, n):
    """16 x 16 x 288 (nine k-tiles: 128-row workgroups): two and three full workgroups and one with a single row."""
    h, big, want = _case(torch_mod, 16, 16, 288, n)
    _check(h, big[3:, 32:32 + 288].contiguous(), want)


@pytest.mark.parametrize("nb,r,dim,n", [(16, 16, 384, LAST_ROW_ALONE), (16, 16, 288, 385)])
def test_rows_of_a_column_slice(torch_mod, nb, r, dim, n):
    """A column slice [:, 32:32 + dim] of an (n, dim + 64) tensor: the row stride is dim + 64 and the first row starts 128 bytes
    into the parent's; the x descriptor ends with the last row's last element, in front of the NaNs behind it."""
    torch = torch_mod
    h, big, want = _case(torch, nb, r, dim, n)
    view = big[3:].contiguous()[:, 32:32 + dim]
    assert view.stride(0) == dim + 64 and view.data_ptr() % 16 == 0
    _check(h, view, want)


@pytest.mark.parametrize("nb,r,dim,n", [(16, 16, 384, LAST_ROW_ALONE), (16, 16, 288, 385)])
def test_rows_from_an_odd_row_of_a_larger_tensor(torch_mod, nb, r, dim, n):
    """A row slice [3:] (and the column slice on top): the base is neither the allocation's nor a multiple of the workgroup's rows."""
    torch = torch_mod
    h, big, want = _case(torch, nb, r, dim, n)
    view = big[3:, 32:32 + dim]
    assert view.data_ptr() != big.data_ptr() and view.data_ptr() % 16 == 0
    _check(h, view, want)
    rows = big[:, 32:32 + dim].contiguous()[3:]          # the row slice alone: stride = dim
    assert rows.stride(0) == dim and rows.data_ptr() % 16 == 0
    _check(h, rows, want)
