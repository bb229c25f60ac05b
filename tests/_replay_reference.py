"""What tests/test_gpu_replay_values.py judges the device replay by: the value `lshrs_tb_model_row_dot` (csrc/host_tiebreak.cpp, the
side pinned to NumPy bit for bit: tests/test_reference_blas.py, tests/test_blas_order.py) gives for every list entry, the batch and
the lists every case uses, and the judge.  NumPy and the host library only - no GPU here; tests/test_replay_reference_host.py
checks this module on the CPU.

The device lets the replayed value out through lshrs_sig_replay_values_f32 (include/lshrs_hip.h): `yb`, whose sign patches the
key.  A replay that is off by a last-place rounding flips the sign of a cancelled projection only some of the time; the value
shows it on every entry of every row.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

ENTRY_COL_BITS = 21                      # kEntryColBits of csrc/lshrs_common.h: entry = (row << 21) | padded key column
AUDIT_BIT = 1 << 62
BUILDS = ("openblas-skylakex", "openblas-haswell")
SENTINEL = np.float32(-7.25e33)          # what `values` holds where nothing may be written (no replay gives it: |y| << 1e33 or non-finite)
GUARD_FLOATS = 1024
SORT_MAX_COLS = 1024

# the batch: 19 rows, so that 19 * columns ends inside a group of eight
N_ROWS = 19
ROW_SMALL, ROW_LARGE, ROW_EXPONENTS = 6, 7, 8
ROWS_CANCELLED = (9, 10, 11, 12)
ROW_POSITIVE, ROW_SUBNORMAL, ROW_ZERO, ROW_NAN, ROW_INF = 13, 14, 15, 16, 17
ROW_LAST = 18                            # Gaussian again: the batch does not end on a special row
NONFINITE_ROWS = (ROW_NAN, ROW_INF)

# ---- the parameter lists of the GPU tests (the (r, dim) of the issue; nb is chosen so that the route takes the shape) ----------
STAGE2_SHAPES = [(16, 128), (16, 160), (16, 768), (16, 416), (4, 200), (10, 300), (13, 640), (7, 102), (6, 101), (3, 103), (5, 100),
                 (4, 8192), (16, 4096 + 64), (5, 4108), (1, 64), (1, 100), (1, 96), (1, 33), (1, 768), (1, 1000)]
BUCKET_SHAPES = [(16, 16, 768), (20, 10, 768), (16, 10, 300)]                       # (nb, r, dim)
TIES_TAIL_SHAPES = [(10, 300), (13, 640), (7, 102), (6, 101), (3, 103), (5, 100)]   # on a view at an odd 4-byte address
TIES_BLOCK_SHAPES = [(4, 4100), (3, 8196), (6, 4101), (7, 8199)]                    # short last block
TIES_MODEL3_ROWS = (2, 3, 4, 5, 7, 9, 16, 17, 20, 33)                               # x every dim in 1..8
TIES_MODEL2_ROWS = (2, 5, 6, 7)                                                     # x every dim in 1..8
SMALL_DIMS = tuple(range(1, 9))
SMALL_SHAPES = [(16, 768), (4, 128), (16, 1536), (8, 3072), (8, 4096), (10, 300), (7, 12), (13, 640)]
SMALL_SHAPES_MORE = [(10, 1504), (6, 4088)]      # GENERAL at KT = 48 and 128 as well (the list above has GENERAL at KT = 24 only)


def stage2_bands(r):
    """Bands for the stage-2 route: 256 padded key columns, the fewest with which the split pass takes every shape."""
    return 256 // (8 * ((r + 7) // 8))


def models_of(r, dim):
    """[(build, model)] for both named builds, a duplicate model skipped."""
    from lshrs_amd import _hostblas

    out = []
    for build in BUILDS:
        m = _hostblas.named_model(build, r, dim)
        if m and m not in [mm for _b, mm in out]:
            out.append((build, m))
    return out


def build_of(model, r, dim):
    """A named build that gives this model at this shape (what LSHHasher(reference_blas=...) is told)."""
    from lshrs_amd import _hostblas

    for build in BUILDS:
        if _hostblas.named_model(build, r, dim) == model:
            return build
    raise AssertionError((model, r, dim))


# ---- dispatch rules, restated (csrc/lshrs_common.h, sig_replay.hip, sig_small.hip) ---------------------------------------------
K_TILE, FIX_SLAB, FIX_SLAB_SHORT, BLAS_BLOCK_TILES = 32, 6, 4, 128


def ktiles(dim):
    return -(-dim // K_TILE)


def blas_general(r, dim):
    return (r & 3) != 0 or ktiles(dim) > BLAS_BLOCK_TILES or dim % K_TILE != 0


def stage2_kernel(r, dim, buckets=False):
    """Which kernel lshrs_replay_stage2 launches: (name, slab, GENERAL)."""
    if r == 1:
        return ("fixany", 0, False)
    if ktiles(dim) <= FIX_SLAB_SHORT:
        return ("fix8", FIX_SLAB_SHORT, blas_general(r, dim))
    return ("fix8-samep" if buckets else "fix8", FIX_SLAB, blas_general(r, dim))


def stage2_refusal(nb, r, dim, model):
    """The code lshrs_sig_hash_batch_split_replay_f32 answers this shape with (0: it takes it) - its header's contract."""
    from lshrs_amd import _native

    tail_ok = dim % 4 != 0 and dim >= 9 and r >= 2 and model in (1, 2)
    one_row_ok = r == 1 and model in (1, 2)
    if not tail_ok and not one_row_ok and (model != 1 or dim % 4 != 0):
        return _native.E_BADARG
    body = dim & ~3
    resident = nb * r <= 256 and 8 <= dim <= 256
    if (dim < 32 and not resident) or (body % 8 != 0 and body > 4096):
        return _native.E_BADARG
    if nb * 8 * ((r + 7) // 8) < 128 and not resident:
        return _native.E_TOOLARGE
    return 0


def ties_plan(r, dim, model, aligned16):
    """lshrs_sig_resolve_ties_replay_f32's choice: (code, plain-load form?) with fast / short_last_block restated."""
    from lshrs_amd import _native

    if model not in (1, 2, 3) or (model == 3 and (dim > 8 or r < 2)):
        return _native.E_BADARG, None
    fast = dim % 4 == 0 and dim >= 8 and aligned16 and r >= 2 and model != 3
    body = dim & ~3
    if r != 1 and dim < 9 and dim % 4 != 0 and model == 1:
        return _native.E_TOOLARGE, None
    short_last_block = body % 8 != 0 and body > 4096
    if fast and not short_last_block and model != 1:
        return _native.E_TOOLARGE, None
    return 0, (not fast) or short_last_block


def small_kernel(r, dim):
    """(KT, GENERAL) of sig_small_kernel for this shape."""
    kt = ktiles(dim)
    return (24 if kt <= 24 else 48 if kt <= 48 else 128), blas_general(r, dim)


def row_kind(j, r):
    """blas_row_kind: 0 the 8-lane fma kernel (and padding), 1 the 4x2 kernel, 2 the 4x1 kernel."""
    r4 = r & ~3
    if j < r4 or j >= r:
        return 0
    return 2 if (r & 3) == 1 or j - r4 == 2 else 1


# ---- the case builder ------------------------------------------------------------------------------------------------------------
def _cancel(rng, p, dim):
    """A Gaussian row made orthogonal to hyperplane p in float64: what is left of the projection is the summation order's."""
    p = p.astype(np.float64)
    x = rng.standard_normal(dim)
    pp = float(p @ p)
    return x - (x @ p) / pp * p if pp > 0 else x


@functools.lru_cache(maxsize=None)
def case(nb, r, dim, seed=20261020):
    """Hyperplanes and the fixed batch for one shape.  Hyperplanes: Gaussian, band nb // 2 on an int8 grid (/ 64).  Rows: Gaussian;
    scaled by 2^-9 and by 300; per-element exponents over 2^+-10; four rows cancelled in float64 against a band's first row, its
    last row and its last-but-one row (the left-over kinds; the fourth against the last row of the last band); a row with all
    products positive (against band 0's last row); 1e-42 subnormals; zero; a NaN; a +Inf."""
    rng = np.random.default_rng([seed, nb, r, dim])
    grid_band = nb // 2
    planes = [(rng.integers(-127, 128, (r, dim)) / 64.0).astype(np.float32) if b == grid_band else
              rng.standard_normal((r, dim)).astype(np.float32) for b in range(nb)]
    x = rng.standard_normal((N_ROWS, dim))
    x[ROW_SMALL] *= 2.0 ** -9
    x[ROW_LARGE] *= 300.0
    x[ROW_EXPONENTS] *= 2.0 ** rng.integers(-10, 11, dim)
    b0 = 1 % nb
    targets = [(b0, 0), (b0, r - 1), (b0, max(r - 2, 0)), (nb - 1, r - 1)]
    for row, (b, j) in zip(ROWS_CANCELLED, targets):
        x[row] = _cancel(rng, planes[b][j], dim)
    p = planes[0][r - 1].astype(np.float64)
    x[ROW_POSITIVE] = np.abs(x[ROW_POSITIVE]) * np.where(p < 0, -1.0, 1.0)
    x = x.astype(np.float32)
    x[ROW_SUBNORMAL] = (rng.integers(1, 200, dim) * np.float64(1e-42)).astype(np.float32) * np.where(rng.random(dim) < 0.5, -1, 1)
    x[ROW_ZERO] = 0.0
    x[ROW_NAN, (dim - 1) // 2] = np.nan
    x[ROW_INF, min(5, dim - 1)] = np.inf
    tiny = np.abs(x[ROW_SUBNORMAL])
    assert (tiny > 0).all() and (tiny < np.finfo(np.float32).tiny).all()
    assert (planes[0][r - 1].astype(np.float64) * x[ROW_POSITIVE] >= 0).all()
    bb = (r + 7) // 8
    return SimpleNamespace(nb=nb, r=r, dim=dim, planes=planes, x=x, bb=bb, row_bytes=nb * bb, padcols=nb * bb * 8, cancelled=targets,
                           grid_band=grid_band)


def flag_entries(rows, cols):
    return (np.asarray(rows, dtype=np.int64) << ENTRY_COL_BITS) | np.asarray(cols, dtype=np.int64)


def entry_rows_cols(entries):
    e = np.asarray(entries, dtype=np.int64) & ~np.int64(AUDIT_BIT)
    return e >> ENTRY_COL_BITS, e & ((1 << ENTRY_COL_BITS) - 1)


def key_columns(c):
    return np.array([b * 8 * c.bb + j for b in range(c.nb) for j in range(c.r)], dtype=np.int64)


def padding_columns(c, band):
    return np.array([band * 8 * c.bb + j for j in range(c.r, 8 * c.bb)], dtype=np.int64)


def dead_columns(c):
    """Three columns >= padcols: entries that are not live - nothing may be written for them."""
    return np.array([c.padcols, c.padcols + 5, (1 << ENTRY_COL_BITS) - 1], dtype=np.int64)


def plain_list(c, seed=5):
    """Every (row, key column) pair of the batch and the padding columns of the last band, in a seeded shuffle, with three
    entries whose column is >= padcols among them.  -> int64 entries."""
    rng = np.random.default_rng([seed, c.nb, c.r, c.dim])
    cols = np.concatenate([key_columns(c), padding_columns(c, c.nb - 1)])
    if (N_ROWS * cols.size + 3) % 8 == 0:                    # (the list must end inside a group of eight: one padding column fewer)
        cols = cols[:-1]
    rows = np.repeat(np.arange(N_ROWS), cols.size)
    cols = np.tile(cols, N_ROWS)
    dead = dead_columns(c)
    rows = np.concatenate([rows, rng.integers(0, N_ROWS, dead.size)])
    cols = np.concatenate([cols, dead])
    order = rng.permutation(rows.size)
    return flag_entries(rows[order], cols[order])


BUCKET_ROUNDS = 4        # a column's 19 rows this many times over (a segment shorter than 64 entries is not one the split pass fills)


def bucket_segments(c, col_cap=None, seed=6):
    """The column segments as stage 1 would leave them: column k holds its 19 rows BUCKET_ROUNDS times over, each round in its own
    order, and k % 8 entries more - so that the columns end at every place inside a group of eight; the padding columns of the
    last band have segments too; column 3 carries one audit entry (bit 62: compared, never patched, no value).  Every entry of
    a segment carries that segment's column - the format's precondition (the eight lanes of a group fetch ONE hyperplane slab
    between them, each by its own entry's column): entries with a column >= padcols belong to the plain lists only.
    col_cap: the segments' stride (default: the longest column).
    -> (list int64 [padcols * col_cap] (-1 where empty), counts int32 [padcols] = entries WANTED, col_cap, longest)"""
    rng = np.random.default_rng([seed, c.nb, c.r, c.dim])
    live = np.zeros(c.padcols, dtype=bool)
    live[key_columns(c)] = True
    live[padding_columns(c, c.nb - 1)] = True
    segs = []
    for k in range(c.padcols):
        if not live[k]:
            segs.append(np.zeros(0, dtype=np.int64))
            continue
        rows = np.concatenate([rng.permutation(N_ROWS) for _ in range(BUCKET_ROUNDS)] + [rng.permutation(N_ROWS)[:k % 8]])
        seg = flag_entries(rows, np.full(rows.size, k))
        if k == 3:
            seg[11] |= AUDIT_BIT
        segs.append(seg)
    counts = np.array([s.size for s in segs], dtype=np.int32)
    longest = int(counts.max())
    col_cap = longest if col_cap is None else int(col_cap)
    out = np.full(c.padcols * col_cap, -1, dtype=np.int64)
    for k, seg in enumerate(segs):
        m = min(seg.size, col_cap)
        out[k * col_cap:k * col_cap + m] = seg[:m]
    return out, counts, col_cap, longest


def expected_values(planes, x, entries, model, r):
    """float32 per entry: lshrs_tb_model_row_dot(planes[band][j], x[row], dim, model, j, r).  A padded key column (bit >= r of its
    band) expects zero - its hyperplane is a zero row of the workspace; where the row holds a NaN or an Inf that zero times x is a
    NaN on the kernels that multiply it out and 0 on those that do not (no key bit depends on it: neither is > 0), so the value
    given here is NaN and the judge takes either (`padded_nonfinite`).  Entries whose column lies beyond the last band: NaN."""
    from lshrs_amd import _hostblas

    lib = _hostblas.load()
    rows, cols = entry_rows_cols(entries)
    nb, dim = len(planes), planes[0].shape[1]
    bc = 8 * ((r + 7) // 8)
    planes = [np.ascontiguousarray(p, dtype=np.float32) for p in planes]
    x = np.ascontiguousarray(x, dtype=np.float32)
    finite = np.isfinite(x).all(axis=1)
    out = np.full(rows.size, np.nan, dtype=np.float32)
    cache = {}
    for i, (row, col) in enumerate(zip(rows.tolist(), cols.tolist())):
        b, j = divmod(col, bc)
        if b >= nb:
            continue
        if j >= r:
            out[i] = 0.0 if finite[row] else np.nan
            continue
        v = cache.get((row, col))
        if v is None:
            v = lib.lshrs_tb_model_row_dot(planes[b][j].ctypes.data, x[row].ctypes.data, dim, model, j, r)
            cache[(row, col)] = v
        out[i] = v
    return out


def bits(a):
    """uint32 patterns with -0.0 mapped to +0.0: the sign of a zero carries no key bit."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return u


def ulp_distance(a, b):
    def lin(u):
        u = u.astype(np.int64)
        return np.where(u & 0x80000000, -(u & 0x7FFFFFFF), u)
    return np.abs(lin(bits(a)) - lin(bits(b)))


def check_reference(c, entries, want, model):
    """What the case builder asserts of the reference ALONE (CPU): the NaN entries are entries of the NaN row and of the Inf row
    and of no other; every entry of the NaN row is NaN; no entry of the Inf row is finite (one +Inf among finite products gives
    +-Inf - compared bit for bit like any other value - and a NaN only where it meets a zero hyperplane element or an Inf of the other
    sign: at dim = 1 it cannot be NaN, so "every entry of the Inf row is NaN" is not a statement that holds).  -> live mask"""
    rows, cols = entry_rows_cols(entries)
    live = cols < c.padcols
    nan = np.isnan(want)
    assert not nan[live & ~np.isin(rows, NONFINITE_ROWS)].any()
    assert nan[live & (rows == ROW_NAN)].all()
    assert not np.isfinite(want[live & (rows == ROW_INF)]).any()
    zero_row = live & (rows == ROW_ZERO)
    assert (bits(want[zero_row]) == 0).all()
    return live


def judge(c, entries, want, got_values, model, label, written=None):
    """values of live entries equal the reference as uint32 (after -0.0 -> +0.0); NaN exactly where the reference is NaN (a padded
    column of a NaN / Inf row: NaN or zero); everything else still the sentinel.  `written`: live entries the kernel was allowed to
    leave out (None: none) - e.g. those beyond a clamped segment; they must be sentinels.  -> (compared, nan_by_construction)"""
    rows, cols = entry_rows_cols(entries)
    live = check_reference(c, entries, want, model)
    if written is not None:
        live = live & written
    got = np.ascontiguousarray(got_values, dtype=np.float32)
    assert got.shape == want.shape
    sent = bits(np.array([SENTINEL]))[0]
    untouched = bits(got[~live]) == sent
    assert untouched.all(), f"{label}: {int((~untouched).sum())} values written for entries that are not live"
    bc = 8 * c.bb
    padded_nonfinite = live & ((cols % bc) >= c.r) & np.isin(rows, NONFINITE_ROWS)
    nan_w, nan_g = np.isnan(want), np.isnan(got)
    strict = live & ~padded_nonfinite
    bad = strict & ((nan_w != nan_g) | (~nan_w & (bits(want) != bits(got))))
    loose_ok = nan_g | (bits(got) == 0)
    bad |= padded_nonfinite & ~loose_ok
    if bad.any():
        idx = np.flatnonzero(bad)
        print(f"{label}: {idx.size} of {int(live.sum())} live entries differ (model {model}); first eight:")
        for i in idx[:8]:
            j = int(cols[i] % bc)
            print(f"  entry {i}: row {int(rows[i])} column {int(cols[i])} (band {int(cols[i] // bc)} bit {j}, kind {row_kind(j, c.r)}) "
                  f"want {bits(want[i:i + 1])[0]:#010x} got {bits(got[i:i + 1])[0]:#010x} "
                  f"ulps {int(ulp_distance(want[i:i + 1], got[i:i + 1])[0]) if not (nan_w[i] or nan_g[i]) else 'nan'}")
    assert not bad.any(), f"{label}: {int(bad.sum())} replayed values differ from lshrs_tb_model_row_dot"
    nan_set = live & nan_g
    assert np.isin(rows[nan_set], NONFINITE_ROWS).all()
    compared = int((strict & ~nan_w).sum())
    return compared, int((live & (nan_w | padded_nonfinite)).sum())


def expected_key_bits(c, entries, values_ref, keys0, listed=None):
    """The keys after the patch: every LISTED live bit is value > 0, every other bit as keys0 had it.  keys0: (19, row_bytes) u8."""
    rows, cols = entry_rows_cols(entries)
    live = cols < c.padcols
    if listed is not None:
        live = live & listed
    bitsarr = np.unpackbits(keys0, axis=1, bitorder="little")
    with np.errstate(invalid="ignore"):
        bitsarr[rows[live], cols[live]] = (values_ref[live] > 0).astype(np.uint8)
    return np.packbits(bitsarr, axis=1, bitorder="little")


def complement_keys(c, entries, values_ref):
    """keys that start as the complement of the expected bits (every listed bit has to be patched), 0xA5 elsewhere"""
    rows, cols = entry_rows_cols(entries)
    live = cols < c.padcols
    start = np.unpackbits(np.full((N_ROWS, c.row_bytes), 0xA5, dtype=np.uint8), axis=1, bitorder="little")
    with np.errstate(invalid="ignore"):
        start[rows[live], cols[live]] = 1 - (values_ref[live] > 0).astype(np.uint8)
    return np.packbits(start, axis=1, bitorder="little")
