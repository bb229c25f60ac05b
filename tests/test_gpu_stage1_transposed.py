"""Stage 1 keeps its accumulators as P X^T (sig16.hip): a lane ends with 64 columns of ONE row, the fragment image is packed in
the order that makes them consecutive bits of the row's sign string (lshrs_common.h: t16_colmap), the coefficients and padded
column ids are gathered through the same map, and the words go straight to the key stores.  What that can get wrong shows as
wrong keys: a column in the wrong bit, a padding column or a block's tail with a bit set, a key row that is not whole words, a
compact block's sign words in the wrong place, a zero row that is not all zeros.  Every case compares the keys of ALL rows with
the reference-literal loop on the same array - never with another device path."""

from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = 4099                       # 17 row groups of 256: the 128-row workgroups (two per CU), the last one with three rows
LONG = 129 * 256 + 1               # more than 128 workgroups of 256 rows per column block: that shape, the last one with one row
LONG_TWO_BLOCKS = 65 * 256 + 1     # the same for hashers of two column blocks


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _rows(nb, r, dim, n, seed):
    """Gaussian rows with what the sign words treat on their own: an all-zero row, a row with a NaN, a row of +-0 and tiny
    elements, a row scaled out of the guarded range, and a row that IS a hyperplane (one projection far from zero, its
    neighbours not)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[5] = 0.0
    x[n // 2, dim // 3] = np.nan
    x[n // 2 + 1] = np.where(rng.random(dim) < 0.5, np.float32(-0.0), np.float32(1e-30))
    x[n // 2 + 2] *= np.float32(2.0 ** 40)
    x[n - 1] = 0.0
    x[n - 1, 0] = 1.0
    return x


def _check(torch, nb, r, dim, n, seed):
    from lshrs_amd import LSHHasher
    from oracle.lshrs_oracle import hash_batch_literal_packed

    h = LSHHasher(num_bands=nb, rows_per_band=r, dim=dim, seed=seed)
    x = _rows(nb, r, dim, n, seed)
    want = hash_batch_literal_packed(h.projections, x)
    got = h.hash_device(torch.from_numpy(x).cuda())
    if h._replay_model():            # (the host BLAS's summation order is one the replay knows: the split pass with its own stage 2)
        assert h.last_stats["route"] == "split+replay", h.last_stats
    bad = np.flatnonzero((got.cpu().numpy() != want).any(axis=(1, 2)))
    assert bad.size == 0, (bad[:8], bad.size, h.last_stats)


@pytest.mark.parametrize("nb,r,dim", [(25, 8, 768),      # key rows of 25 bytes: byte stores, the block's tail behind column 200
                                      (128, 4, 768),     # two compact blocks of 64 bands: the sign words through the byte table
                                      (30, 12, 416),     # two padded blocks, four padding columns in every band, 13 k-tiles
                                      (16, 16, 300)])    # a partial last k-tile
def test_keys_of_the_128_row_workgroups(torch_mod, nb, r, dim):
    _check(torch_mod, nb, r, dim, SMALL, seed=41)


@pytest.mark.parametrize("nb,r,dim,n", [(25, 8, 768, LONG), (30, 12, 416, LONG_TWO_BLOCKS), (128, 4, 384, LONG_TWO_BLOCKS)])
def test_keys_of_the_256_row_workgroups(torch_mod, nb, r, dim, n):
    _check(torch_mod, nb, r, dim, n, seed=43)
