"""GPU tests of the REPLAYED VALUE.  The keys are the reference's only because the device replays the host BLAS's summation order
for every projection whose sign is in doubt - in sig_fix8_kernel<true, GENERAL, SLAB, SAMEP>, sig_fixany_kernel and
sig_small_kernel<KT, GENERAL>, each of which writes that order out by hand - and every other test judges them through key bits:
a last-place error flips the sign of a cancelled projection only some of the time.  Here the value itself comes out
(lshrs_sig_replay_values_f32: the product's kernels through the product's own choice of kernel) and is compared, entry by entry
and bit for bit, with lshrs_tb_model_row_dot - the side pinned to NumPy (tests/_replay_reference.py: rows, lists, judge).

Every parameter list restates the dispatch rule it is meant to hit, so that a change of plan cannot quietly move a case to
another kernel."""
from __future__ import annotations

import numpy as np
import pytest

from tests import _replay_reference as R

pytestmark = pytest.mark.gpu

STAGE2, TIES, SMALL = 0, 1, 2
TOTALS = {}                              # route -> [entries compared by value, NaN by construction] (printed by every case)


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _workspace(torch, c, model):
    """The hyperplane workspace as test_gpu_list_completeness.py gets it: a hasher pinned to a named build, the planes assigned."""
    from lshrs_amd import LSHHasher

    h = LSHHasher(num_bands=c.nb, rows_per_band=c.r, dim=c.dim, seed=7, reference_blas=R.build_of(model, c.r, c.dim))
    h.projections = [p.copy() for p in c.planes]
    assert h._replay_model() == model
    dev = torch.device("cuda", torch.cuda.current_device())
    return h, dev, h._workspace(dev)


def _rows_on_device(torch, dev, x, ldx=None, odd=False):
    """x as (19, ldx) on the device with 1024 floats of slack behind it; odd: the view starts at an odd 4-byte address."""
    n, dim = x.shape
    ldx = dim if ldx is None else ldx
    buf = torch.zeros(n * ldx + 1 + R.GUARD_FLOATS, dtype=torch.float32, device=dev)
    view = buf[1 if odd else 0:][:n * ldx].view(n, ldx)
    view[:, :dim].copy_(torch.from_numpy(x.copy()))
    assert view.data_ptr() % 16 == (4 if odd else 0)
    return view


def _run_list(torch, route, c, model, entries, *, odd=False, expect=0, sort_cap=None, counts=None, ws_model=None):
    """One call on a plain list (sort_cap None) or on column segments (ws_model: the workspace's hasher is pinned to another model
    than the call names - for a refusal, where no build names the refused model); -> (rc, values, guard, keys, counters, keys0, want)"""
    from lshrs_amd import _native

    lib = _native.load()
    h, dev, ws = _workspace(torch, c, model if ws_model is None else ws_model)
    want = R.expected_values(c.planes, c.x, entries, model, c.r)
    keys0 = R.complement_keys(c, entries, want)
    xd = _rows_on_device(torch, dev, c.x, odd=odd)
    m = entries.size
    values = torch.full((m + R.GUARD_FLOATS,), float(R.SENTINEL), dtype=torch.float32, device=dev)
    keys = torch.zeros(R.N_ROWS * c.row_bytes + 16, dtype=torch.uint8, device=dev)        # (the patch is a 32-bit atomic around the byte)
    keys[:R.N_ROWS * c.row_bytes].copy_(torch.from_numpy(keys0.reshape(-1)))
    counters = torch.zeros(_native.SIG_DEVICE_COUNTERS, dtype=torch.int32, device=dev)
    lst = torch.from_numpy(np.where(entries < 0, 0, entries)).to(dev)                     # (an empty slot of a segment is never read)
    sort, keep = None, None
    if sort_cap is None:
        counters[1] = m
        args = (lst.data_ptr(), m, None)
    else:
        hist = torch.zeros(2 * R.SORT_MAX_COLS, dtype=torch.int32, device=dev)
        hist[:c.padcols].copy_(torch.from_numpy(counts))
        y = torch.zeros(m, dtype=torch.float32, device=dev)
        thr = torch.zeros(m, dtype=torch.float32, device=dev)
        sort = _native.SigSort(lst.data_ptr(), y.data_ptr(), hist.data_ptr(), m, thr_ptr=thr.data_ptr())
        keep = (hist, y, thr)
        import ctypes

        args = (None, 0, ctypes.addressof(sort))
    stream = torch.cuda.current_stream(dev)
    rc = lib.lshrs_sig_replay_values_f32(xd.data_ptr(), R.N_ROWS, xd.stride(0), ws.data_ptr(), c.nb, c.r, c.dim, model, route,
                                         keys.data_ptr(), values.data_ptr(), *args, counters.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert rc == expect, (rc, expect)
    out = values.cpu().numpy()
    del keep
    return (out[:m], out[m:], keys.cpu().numpy()[:R.N_ROWS * c.row_bytes].reshape(R.N_ROWS, c.row_bytes),
            counters.cpu().numpy()[:8], keys0, want)


def _judge_list(c, model, entries, res, label, route, written=None, flips_exact=True):
    got, guard, keys, counters, keys0, want = res
    sent = R.bits(np.array([R.SENTINEL]))[0]
    compared, nan = R.judge(c, entries, want, got, model, label, written=written)
    assert (R.bits(guard) == sent).all(), f"{label}: the guard behind the values was written"
    listed = written
    assert np.array_equal(keys, R.expected_key_bits(c, entries, want, keys0, listed=listed)), f"{label}: key bits"
    rows, cols = R.entry_rows_cols(entries)
    live = (cols < c.padcols) if written is None else ((cols < c.padcols) & written)
    if flips_exact:                                          # every listed bit started as the complement: each is patched once
        assert int(counters[3]) == int(live.sum()), (counters, int(live.sum()))
    tot = TOTALS.setdefault(route, [0, 0])
    tot[0] += compared
    tot[1] += nan
    print(f"{label}: model {model}, {entries.size} entries, {compared} compared by value, {nan} NaN by construction; "
          f"route total {tot[0]} / {tot[1]}")
    return compared


def _nothing_written(res):
    got, guard, keys, counters, keys0, _want = res
    sent = R.bits(np.array([R.SENTINEL]))[0]
    assert (R.bits(got) == sent).all() and (R.bits(guard) == sent).all() and np.array_equal(keys, keys0) and not counters[[0, 2, 3, 4, 5, 6, 7]].any()


# ------------------------------------------------------------------------------------------------------------------
# stage 2 of the split pass, plain list
# ------------------------------------------------------------------------------------------------------------------
STAGE2_KERNELS = {                       # lshrs_replay_stage2's choice, restated per shape: (kernel, slab, GENERAL), slabs of k-tiles
    (16, 128): ("fix8", 4, False), (16, 160): ("fix8", 6, False), (16, 768): ("fix8", 6, False), (16, 416): ("fix8", 6, False),
    (4, 200): ("fix8", 6, True), (10, 300): ("fix8", 6, True), (13, 640): ("fix8", 6, True), (7, 102): ("fix8", 4, True),
    (6, 101): ("fix8", 4, True), (3, 103): ("fix8", 4, True), (5, 100): ("fix8", 4, True),
    (4, 8192): ("fix8", 6, True), (16, 4160): ("fix8", 6, True), (5, 4108): None,
    (1, 64): ("fixany", 0, False), (1, 100): ("fixany", 0, False), (1, 96): ("fixany", 0, False), (1, 33): ("fixany", 0, False),
    (1, 768): ("fixany", 0, False), (1, 1000): ("fixany", 0, False),
}
STAGE2_PARAMS = [(r, dim, build, model) for r, dim in R.STAGE2_SHAPES for build, model in R.models_of(r, dim)]


@pytest.mark.parametrize("r,dim,build,model", STAGE2_PARAMS)
def test_stage2_replays_the_hosts_value_on_a_plain_list(torch_mod, r, dim, build, model):
    """lshrs_replay_stage2 on a caller's list: the short slab (four k-tiles), one slab of 6, four slabs, a partial last slab, a
    partial k-tile, the left-over row kinds with 8 m + 4 elements and tails of 1 / 2 / 3, two blocks of 4096 and a block boundary
    inside a slab, sdot on both builds.  (5, 4108) - 8 m + 4 beyond one block - is not the split pass's: LSHRS_E_BADARG."""
    from lshrs_amd import _native

    nb = R.stage2_bands(r)
    c = R.case(nb, r, dim)
    kernel = STAGE2_KERNELS[(r, dim)]
    entries = R.plain_list(c)
    refusal = R.stage2_refusal(nb, r, dim, model)
    if kernel is None:
        assert refusal == _native.E_BADARG and (dim & ~3) % 8 != 0 and (dim & ~3) > 4096
        _nothing_written(_run_list(torch_mod, STAGE2, c, model, entries, expect=_native.E_BADARG))
        return
    assert refusal == 0 and R.stage2_kernel(r, dim) == kernel
    kt = R.ktiles(dim)
    assert (kernel[0] == "fixany") == (r == 1) and (r == 1 or (kernel[1] == 4) == (kt <= R.FIX_SLAB_SHORT))
    assert r == 1 or kernel[2] == ((r & 3) != 0 or kt > R.BLAS_BLOCK_TILES or dim % 32 != 0)
    if (r, dim) == (16, 416):
        assert kt % 6 == 1                                   # a last slab of one k-tile
    if (r, dim) == (16, 4160):
        assert kt == 130 and 128 % 6 == 2                    # the block boundary falls inside a slab
    res = _run_list(torch_mod, STAGE2, c, model, entries)
    _judge_list(c, model, entries, res, f"stage 2 {nb} x {r} x {dim} ({build})", "stage2")
    assert int(res[3][1]) == entries.size and int(res[3][7]) == 0


# ------------------------------------------------------------------------------------------------------------------
# stage 2, column segments (SAMEP)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,r,dim", R.BUCKET_SHAPES)
@pytest.mark.parametrize("short", [0, 1])
def test_stage2_replays_the_hosts_value_on_column_segments(torch_mod, nb, r, dim, short):
    """sig_fix8_kernel<true, GENERAL, 6, true>: eight entries share one hyperplane slab in LDS.  Segments filled here, col_cap the
    longest column; once more with col_cap one short of it: the entries beyond a segment's end are not taken (they have no
    place in the segments, so no value), counter [7] says so, the rest are exact."""
    from lshrs_amd import _native

    c = R.case(nb, r, dim)
    (_b, model), = R.models_of(r, dim)[:1]
    assert model == 1 and dim % 4 == 0
    _seg, counts, _cap, longest = R.bucket_segments(c)
    entries, counts, col_cap, longest = R.bucket_segments(c, col_cap=longest - short)
    # split_buckets (sig_split.hip) restated: long rows, at most 1024 padded key columns, bands of two rows and more, room
    assert R.ktiles(dim) > R.FIX_SLAB_SHORT and c.padcols <= R.SORT_MAX_COLS and r != 1 and entries.size // c.padcols == col_cap >= 64
    assert R.stage2_kernel(r, dim, buckets=True) == ("fix8-samep", 6, (r & 3) != 0 or dim % 32 != 0)
    assert int((counts > col_cap).sum()) == (int((counts == longest).sum()) if short else 0) and (not short or (counts > col_cap).any())
    rows, cols = R.entry_rows_cols(entries)
    taken = (entries >= 0) & ((entries & R.AUDIT_BIT) == 0)                               # slots that hold a plain entry
    assert int((entries >= 0).sum()) == int(np.minimum(counts, col_cap).sum())
    res = _run_list(torch_mod, STAGE2, c, model, entries, sort_cap=col_cap, counts=counts)
    _judge_list(c, model, entries, res, f"segments {nb} x {r} x {dim} col_cap {col_cap} (longest {longest})", "stage2-segments",
                written=taken, flips_exact=False)
    counters = res[3]
    assert (int(counters[7]) != 0) == bool(short), counters
    assert int(counters[4]) == 1 and int(counters[3]) >= 1                                # one audit entry, compared only


# ------------------------------------------------------------------------------------------------------------------
# behind the f32 kernel
# ------------------------------------------------------------------------------------------------------------------
TIES_TAIL_PARAMS = [(r, dim, build, model) for r, dim in R.TIES_TAIL_SHAPES for build, model in R.models_of(r, dim)]
TIES_BLOCK_PARAMS = [(r, dim, build, model) for r, dim in R.TIES_BLOCK_SHAPES for build, model in R.models_of(r, dim)]


@pytest.mark.parametrize("r,dim,build,model", TIES_TAIL_PARAMS)
def test_tie_replay_at_an_odd_address_replays_the_hosts_value(torch_mod, r, dim, build, model):
    """sig_fixany_kernel behind the f32 kernel: rows at an odd 4-byte address (never `fast`), the left-over kinds, tails 1 / 2 / 3."""
    c = R.case(R.stage2_bands(r), r, dim)
    assert R.ties_plan(r, dim, model, aligned16=False) == (0, True)
    entries = R.plain_list(c)
    res = _run_list(torch_mod, TIES, c, model, entries, odd=True)
    _judge_list(c, model, entries, res, f"ties odd address {c.nb} x {r} x {dim} ({build})", "ties")


@pytest.mark.parametrize("r,dim", [(10, 300), (13, 640), (5, 100), (16, 128), (16, 768)])
def test_tie_replay_on_aligned_rows_takes_the_lds_dma_form(torch_mod, r, dim):
    """`fast`: whole groups of four in 16-byte aligned rows - sig_fix8_kernel<true, GENERAL, 6, false> whatever the length (slabs of
    six even for rows of four k-tiles and fewer: a pairing the stage-2 route never makes)."""
    c = R.case(R.stage2_bands(r), r, dim)
    assert dim % 4 == 0 and R.ties_plan(r, dim, 1, aligned16=True) == (0, False)
    entries = R.plain_list(c)
    res = _run_list(torch_mod, TIES, c, 1, entries)
    _judge_list(c, 1, entries, res, f"ties aligned {c.nb} x {r} x {dim}", "ties")


@pytest.mark.parametrize("r,dim,build,model", TIES_BLOCK_PARAMS)
def test_tie_replay_of_a_short_last_block_replays_the_hosts_value(torch_mod, r, dim, build, model):
    """8 m + 4 elements beyond 4096: the last, short block takes ITS first four first - the plain-load form's, aligned or not."""
    c = R.case(4, r, dim)
    body = dim & ~3
    assert body % 8 != 0 and body > 4096 and R.ties_plan(r, dim, model, aligned16=True) == (0, True)
    entries = R.plain_list(c)
    res = _run_list(torch_mod, TIES, c, model, entries, odd=bool(dim % 4))
    _judge_list(c, model, entries, res, f"ties short last block 4 x {r} x {dim} ({build})", "ties")


@pytest.mark.parametrize("r", R.TIES_MODEL3_ROWS)
def test_tie_replay_of_the_small_matrix_kernels_replays_the_hosts_value(torch_mod, r):
    """Model 3 (the SkylakeX build's small-matrix kernels): every dim in 1 .. 8, bands whose rows sit in blocks of 16 / 8 / 4 / 2 / 1."""
    from lshrs_amd import _hostblas

    for dim in R.SMALL_DIMS:
        assert _hostblas.named_model("openblas-skylakex", r, dim) == 3 and R.ties_plan(r, dim, 3, True) == (0, True)
        c = R.case(3, r, dim)
        entries = R.plain_list(c)
        res = _run_list(torch_mod, TIES, c, 3, entries, odd=bool(dim % 2))
        _judge_list(c, 3, entries, res, f"ties model 3: 3 x {r} x {dim}", "ties")


@pytest.mark.parametrize("r", R.TIES_MODEL2_ROWS)
def test_tie_replay_below_nine_elements_on_the_haswell_build(torch_mod, r):
    """The Haswell / Zen build runs its usual kernels down to one element: model 2 where there is a scalar tail, model 1 at 4 and 8
    (at 8 elements in aligned rows: the LDS-DMA form with a single partial k-tile)."""
    from lshrs_amd import _hostblas, _native

    for dim in R.SMALL_DIMS:
        model = _hostblas.named_model("openblas-haswell", r, dim)
        assert model == (1 if dim % 4 == 0 else 2)
        odd = dim == 4
        code, plain = R.ties_plan(r, dim, model, aligned16=not odd)
        assert code == 0 and plain == (dim != 8)
        c = R.case(3, r, dim)
        entries = R.plain_list(c)
        res = _run_list(torch_mod, TIES, c, model, entries, odd=odd)
        _judge_list(c, model, entries, res, f"ties haswell: 3 x {r} x {dim}", "ties")
        if dim % 4:                                          # the SkylakeX order is not modelled there: refused, nothing launched
            assert R.ties_plan(r, dim, 1, True) == (_native.E_TOOLARGE, None)
            _nothing_written(_run_list(torch_mod, TIES, c, 1, entries, expect=_native.E_TOOLARGE, ws_model=2))
        else:                                                # whole groups of four are model 1's: model 2 is refused on aligned rows
            assert R.ties_plan(r, dim, 2, True) == ((_native.E_TOOLARGE, None) if dim == 8 else (0, True))
            if dim == 8:
                _nothing_written(_run_list(torch_mod, TIES, c, 2, entries, expect=_native.E_TOOLARGE, ws_model=1))


# ------------------------------------------------------------------------------------------------------------------
# a handful of rows: every projection
# ------------------------------------------------------------------------------------------------------------------
SMALL_KERNELS = {(16, 768): (24, False), (4, 128): (24, False), (16, 1536): (48, False), (8, 3072): (128, False), (8, 4096): (128, False),
                 (10, 300): (24, True), (7, 12): (24, True), (13, 640): (24, True), (10, 1504): (48, True), (6, 4088): (128, True)}


@pytest.mark.parametrize("r,dim", R.SMALL_SHAPES + R.SMALL_SHAPES_MORE)
def test_small_kernel_replays_the_hosts_value_for_every_projection(torch_mod, r, dim):
    """sig_small_kernel<KT, GENERAL>: KT = 24 / 48 / 128 by the k-tiles, GENERAL by blas_general - every column of every row, the
    padding columns included; the keys are written whole."""
    torch = torch_mod
    from lshrs_amd import _native

    nb = R.stage2_bands(r)
    c = R.case(nb, r, dim)
    kt = R.ktiles(dim)
    assert R.small_kernel(r, dim) == SMALL_KERNELS[(r, dim)] == ((24 if kt <= 24 else 48 if kt <= 48 else 128), R.blas_general(r, dim))
    h, dev, ws = _workspace(torch, c, 1)
    h.hash_batch_packed(c.x[:3])
    if h.last_stats.get("path") != "small-replay":
        pytest.skip(f"the hasher does not take {nb} x {r} x {dim} through the small kernel: {h.last_stats}")
    lib = _native.load()
    cols = np.arange(c.padcols)
    entries = R.flag_entries(np.repeat(np.arange(R.N_ROWS), cols.size), np.tile(cols, R.N_ROWS))
    want = R.expected_values(c.planes, c.x, entries, 1, r)
    ldx = 32 * kt
    xd = _rows_on_device(torch, dev, c.x, ldx=ldx)
    m = entries.size
    values = torch.full((m + R.GUARD_FLOATS,), float(R.SENTINEL), dtype=torch.float32, device=dev)
    keys = torch.full((R.N_ROWS * c.row_bytes + 16,), 0xA5, dtype=torch.uint8, device=dev)
    counters = torch.zeros(_native.SIG_DEVICE_COUNTERS, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    rc = lib.lshrs_sig_replay_values_f32(xd.data_ptr(), R.N_ROWS, ldx, ws.data_ptr(), nb, r, dim, 1, SMALL, keys.data_ptr(),
                                         values.data_ptr(), None, 0, None, counters.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert rc == 0, rc
    out = values.cpu().numpy()
    sent = R.bits(np.array([R.SENTINEL]))[0]
    compared, nan = R.judge(c, entries, want, out[:m], 1, f"small {nb} x {r} x {dim}")
    assert (R.bits(out[m:]) == sent).all()
    kb = keys.cpu().numpy()
    assert (kb[R.N_ROWS * c.row_bytes:] == 0xA5).all()
    with np.errstate(invalid="ignore"):
        bits = (want > 0).astype(np.uint8).reshape(R.N_ROWS, c.padcols)
    assert np.array_equal(kb[:R.N_ROWS * c.row_bytes].reshape(R.N_ROWS, c.row_bytes), np.packbits(bits, axis=1, bitorder="little"))
    tot = TOTALS.setdefault("small", [0, 0])
    tot[0] += compared
    tot[1] += nan
    print(f"small {nb} x {r} x {dim}: KT {SMALL_KERNELS[(r, dim)]}, {compared} compared by value, {nan} NaN by construction; "
          f"route total {tot[0]} / {tot[1]}")
