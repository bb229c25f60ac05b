"""Models and inputs for the COMPLETENESS of the lists the signature kernels leave for the exact decision (pure NumPy).

The signature pass gives the reference's keys because every projection whose fast value could have the wrong sign is handed
to the exact decision: stage 1's flag list in the split pass (every `NOT(|y1| > window(row, column))`), the tie list in the
f32 pass (every `|y| < tau ||x|| ||p||`).  An entry that is dropped costs a key bit only where the fast sign also happens
to be wrong - once in many millions of random projections - so the lists themselves are judged here, from the values the
CPU models give (oracle.build.split_stage1_model, chain_project) and the windows restated in float64.

Inputs with power:
  * `uneven_scales` - every key column times a power of two (the bf16 split and both value models are unchanged; only the
    norms and the window coefficients move), so that a maximum per column block that is taken over the wrong block, the
    wrong columns or read from the wrong slot is too small by a factor of 16 or 64, not by the few percent that separate
    the norms of Gaussian hyperplanes;
  * `build_batch` - rows whose projection on one chosen hyperplane sits at a chosen FRACTION of that row's and column's own
    window (inside: 0.05 .. 0.9, outside: 1.15 .. 2.5), rows flagged wholesale, a zero row, a NaN row, and a group of rows
    planted on every eighth key column that makes one workgroup want more entries than its LDS stage holds.

Also here: the names of the scratch slots of `LSHHasher` the tests read stage 1's lists from.
"""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -24
ENTRY_COL_BITS = 21                       # lshrs_common.h: flag_entry = (row << 21) | padded key column
ENTRY_COL_MASK = (1 << ENTRY_COL_BITS) - 1
AUDIT_BIT = 1 << 62                       # kAuditBit: a bucket entry that is a SAMPLE of what stage 1 did not flag
S1_LIST_CAP = {4: 4096, 8: 8192}          # kS1ListCap of sig16_kernel<., ., W>: entries a workgroup stages in LDS
SORT_MAX_COLS = 1024

# ---- slots of a value of LSHHasher._replay_scratch (one per device and stream; _replay_paths.py builds it) ----------------
S1_LIST = 0            # int64 [cap]: stage 1's plain list
S1_VALUES = 5          # float32 [cap]: the stage-1 value of every list entry
AUDIT_ENTRIES = 6      # int64: the audit sample of a launch, one entry per slot (-1: none)
AUDIT_VALUES = 7       # float32: (stage-1 value, window) per slot
# ---- slots of a value of LSHHasher._sort_res (the bucket form) --------------------------------------------------------------
SORT_STRUCT = 0        # _native.SigSort: .cap = entries of all segments together
SORT_TENSORS = 3       # (segments int64, their values, 2 x SORT_MAX_COLS column counters, the audit entries' windows)
SORT_LAUNCHES = 4      # [launches so far]: launch k counts in counter set k & 1


def only_scratch(h):
    """The scratch of a hasher that has launched on ONE stream."""
    (scratch,) = h._replay_scratch.values()
    return scratch


def stream_scratch(h, torch, device):
    return h._replay_scratch[(device.index, torch.cuda.current_stream(device).cuda_stream)]


def stage1_list(scratch, count):
    """(entries int64, stage-1 values float32) of the first `count` entries of the plain list."""
    return scratch[S1_LIST][:count].cpu().numpy(), scratch[S1_VALUES][:count].cpu().numpy()


def entry_rows_cols(entries):
    e = np.asarray(entries, dtype=np.int64) & ~np.int64(AUDIT_BIT)
    return e >> ENTRY_COL_BITS, e & ENTRY_COL_MASK


def bucket_lists(h, padcols):
    """The bucket form's list of the last launch: (entries, values, column of the segment each was found in, per-column
    counts as stage 1 wanted them, segment capacity).  Entries past a segment's capacity were not stored."""
    (res,) = h._sort_res.values()
    lst, y, hist, _thr = res[SORT_TENSORS]
    per = int(res[SORT_STRUCT].cap) // padcols
    used = ((res[SORT_LAUNCHES][0] - 1) & 1) * SORT_MAX_COLS
    counts = hist[used:used + padcols].cpu().numpy().astype(np.int64)
    lst, y = lst.cpu().numpy(), y.cpu().numpy()
    keep = np.concatenate([c * per + np.arange(min(int(k), per)) for c, k in enumerate(counts)] or [np.zeros(0)]).astype(np.int64)
    return lst[keep], y[keep], keep // per, counts, per


# ------------------------------------------------------------------------------------------------- hyperplanes
def key_columns(nb, r):
    """Padded column id of every key column, band-major (the order of `window_coefficients` and of the CPU models)."""
    bb8 = 8 * ((r + 7) // 8)
    return np.arange(nb).repeat(r) * bb8 + np.tile(np.arange(r), nb)


def layouts(nb, r):
    return ("A", "B") if nb * r > 256 else ("first", "middle", "last")


def uneven_scales(ncols, layout, block=256):
    """(power-of-two scale per key column, the large columns).  Blocks are runs of `block` key columns (256; compact column
    blocks hold whole bands: 250 key columns of bands of 10 rows).
    One block: every column x 1, ONE column x 64 - the first, a middle or the last key column.
    Two blocks, layout A: block 0 x 1 with one column x 64; block 1 as a whole x 1/16, its large column included (x 4: still
    64 times its neighbours) - so block 1's maximum is 1/16 of block 0's; layout B: the roles swapped.  The large column
    sits at a different position in each block and layout.  A maximum read from the other block is 16 times too small in
    one of the two layouts; one that misses the large column is 64 times too small."""
    s = np.ones(ncols)
    nblk = -(-ncols // block)
    if nblk == 1:
        large = [{"first": 0, "middle": ncols // 2 + 3, "last": ncols - 1}[layout]]
        s[large] = 64.0
        return s, large
    assert nblk == 2 and layout in ("A", "B")
    small = 1 if layout == "A" else 0
    large = []
    for k in range(nblk):
        lo, hi = block * k, min(ncols, block * k + block)
        pos = lo + (37 + 71 * k + (113 if layout == "B" else 0)) % (hi - lo)
        if k == small:
            s[lo:hi] = 1.0 / 16.0
        s[pos] *= 64.0
        large.append(pos)
    return s, large


def scaled_planes(planes, layout, block=256):
    """The hasher's hyperplanes with `uneven_scales` applied: (list of per-band float32 matrices, large key columns)."""
    nb, r = len(planes), planes[0].shape[0]
    s, large = uneven_scales(nb * r, layout, block)
    out = [(np.asarray(p, dtype=np.float32) * s[b * r:(b + 1) * r, None].astype(np.float32)) for b, p in enumerate(planes)]
    return out, large


# ------------------------------------------------------------------------------------------------- windows (float64)
def bf16_rne(v):
    u = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def band_eps(dim):
    """Relative half-width of the band around a window the judge leaves undecided: the kernels form the window in f32 - a sum
    of `dim` squares (at most dim 2^-24 relative, halved by the root), a root, products and a sum (a few 2^-24 more)."""
    return (dim + 8) * U


def split_windows(x, form, coef=None, pnorm=None, tau1_units=None):
    """Stage 1's window of every (row, key column), from x as cast: -> (W, W_up, wholesale rows, zero rows).
    form "proven": W = 1.001 (||x_hi|| coef_a[j] + ||x_mid|| coef_b[j]); "tau1": W = 1.001 tau1 2^-24 ||x_hi|| ||p_j||.
    W_up: the same with the squares of the row's last 32 elements counted once more in both norms (sig16_kernel).
    wholesale: a non-finite window or a largest |x| outside [2^-32, 2^32] - every key column goes to the exact decision."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        xh = bf16_rne(x)
        xm = bf16_rne(x - xh)
        h2, m2 = (xh.astype(np.float64) ** 2).sum(1), (xm.astype(np.float64) ** 2).sum(1)
        h2u = h2 + (xh[:, -32:].astype(np.float64) ** 2).sum(1)
        m2u = m2 + (xm[:, -32:].astype(np.float64) ** 2).sum(1)
        amax = np.nanmax(np.abs(x.astype(np.float64)), axis=1)
        if form == "proven":
            ca, cb = np.asarray(coef[0], dtype=np.float64), np.asarray(coef[1], dtype=np.float64)
            W = 1.001 * (np.sqrt(h2)[:, None] * ca + np.sqrt(m2)[:, None] * cb)
            Wu = 1.001 * (np.sqrt(h2u)[:, None] * ca + np.sqrt(m2u)[:, None] * cb)
        else:
            t = 1.001 * float(tau1_units) * U * np.asarray(pnorm, dtype=np.float64)
            W, Wu = np.sqrt(h2)[:, None] * t, np.sqrt(h2u)[:, None] * t
        zero = amax == 0.0
        wholesale = ~np.isfinite(h2) | ~np.isfinite(m2) | ((amax != 0.0) & ~((amax >= 2.0 ** -32) & (amax <= 2.0 ** 32)))
    return W, Wu, wholesale, zero


def tie_windows(x, form, coef_tie=None, pnorm=None, tau=None):
    """The f32 pass's tie window: "proven": ||x|| coef_tie[j]; "tau": tau ||x|| ||p_j||."""
    with np.errstate(all="ignore"):
        xn = np.sqrt((np.asarray(x, dtype=np.float64) ** 2).sum(1))
        c = np.asarray(coef_tie, dtype=np.float64) if form == "proven" else float(tau) * np.asarray(pnorm, dtype=np.float64)
        return xn[:, None] * c


def judge(y, W, W_up, eps, wholesale=None, zero=None):
    """-> (must, must_not) boolean (rows, key columns); what is in neither is the undecided band.
    must = |y| <= (1 - eps) W, must_not = |y| > (1 + eps) W_up.  A window of zero (a zero row) flags nothing: the kernels'
    tests are strict where the window is 0.  A NaN value outside a wholesale row never satisfies a kernel's test."""
    with np.errstate(all="ignore"):
        a = np.abs(np.asarray(y, dtype=np.float64))
        must = (a <= (1.0 - eps) * W) & (W > 0)
        must_not = (a > (1.0 + eps) * W_up) | (W_up == 0) | np.isnan(a) | np.isnan(W_up)
        must &= ~must_not
    if wholesale is not None:
        must[wholesale], must_not[wholesale] = True, False
    if zero is not None:
        must[zero], must_not[zero] = False, True
    return must, must_not


# ------------------------------------------------------------------------------------------------- rows
LEAD_VISITS = 16       # planted rows per large column that are spread over the batch (+ 48 rows in three whole tiles)


def build_batch(P, window_of, value_of, large, seed, n_planted=512, group=40, n_scaled=11, bf16_tiles=True):
    """Rows for one case.  P: (key columns, dim) float64, the hyperplanes as the kernels hold them; window_of(x float32) ->
    (rows, key columns) float64, the window the planted fractions refer to.
    Layout of the batch: `group` consecutive rows planted INSIDE the window on every 8th key column, one true zero row, one
    row with a NaN, `n_scaled` rows scaled by 2^40 or 2^-40 (flagged wholesale by the split pass), then `n_planted` rows with
    ONE planted column each - all key columns in turn, the large columns `LEAD_VISITS` times each and in three whole 16-row tiles more (two in three inside) -,
    the fraction drawn from [0.05, 0.9] (inside, every other row) or [1.15, 2.5] (outside), with both signs.
    The correction runs along p in float64 (`planted_edge` of tests/test_gpu_signature.py) and is cast to float32.  The
    fraction is one of the value the KERNEL holds - value_of(x float32) -> (rows, key columns) float32, the CPU model of
    it -, which strays from the exact projection by a few percent of a window at 768-d and by more on short rows: the
    correction is repeated on the model's value, for the rows that need it, until every planted projection sits at 0.02 ..
    0.97 of its window (inside) or at 1.12 and more (outside: sig16_kernel's widened window reaches 1.10 at 300-d).
    -> (x float32, planted (rows, key columns) bool, inside (rows,) bool: the row's planted fraction is below 1,
        value_of(x))."""
    rng = np.random.default_rng(seed)
    ncols, dim = P.shape
    pn2 = (P * P).sum(1)

    def fractions(k, inside, high=None):
        f = np.where(inside, rng.uniform(0.05, 0.9, k), rng.uniform(1.15, 2.5, k))
        if high is not None:
            f = np.where(high, rng.uniform(0.7, 0.9, k), f)
        return f * np.where(rng.random(k) < 0.5, -1.0, 1.0)

    # the planted rows
    x0 = rng.standard_normal((n_planted, dim))
    stride = next(s for s in range(max(2, ncols // 3) | 1, ncols + 8, 2) if np.gcd(s, ncols) == 1) if ncols > 1 else 1
    cols = np.array([(5 + i * stride) % ncols for i in range(n_planted)], dtype=np.int64)
    inside = np.arange(n_planted) % 2 == 0
    # ... of which `LEAD_VISITS` per large column, spread over the batch so that no two of one column share a 16-row tile (a
    # wave's screen is one ballot per 16 rows x 32 columns: what one lane sends to the exact test, its neighbours ride along):
    # in turn inside, inside at 0.7 .. 0.9 of the window - the upper part of the range, where a screen that lost the LARGER
    # of its two maxima still shows: the x_mid term keeps 40 .. 60 % of a proven window - and outside
    n_lead = LEAD_VISITS * len(large)
    lead_at = 64 + (n_planted - 74) // n_lead * np.arange(n_lead)
    # ... and three whole 16-row tiles (rows 64 .. 111 of the batch) whose rows are rounded to bf16 values once they are planted,
    # so that what the corrections below add (a few 1e-5 ||x||) is all there is of x_mid: x_mid is
    # then next to nothing and the proven window is its x_hi term alone.  Elsewhere the x_mid term's maximum - the large column's
    # too - keeps the screen of every Gaussian row of a tile 25 times above an ordinary column's window, the tile's words all go
    # to the exact test and a lost maximum of the x_hi term (`wamax`) never shows.
    first = group + 2 + n_scaled
    tile_at = np.arange(64, 112 if bf16_tiles else 64) - first      # (the f32 pass has no x_mid term: no such tiles)
    lead_at = np.concatenate([tile_at, lead_at])
    n_lead = lead_at.size
    assert (tile_at >= 0).all() and np.unique(lead_at).size == n_lead and lead_at.max() < n_planted
    high = np.zeros(n_planted, dtype=bool)
    rest = np.setdiff1d(np.arange(n_planted), lead_at)
    cols[rest] = (5 + np.arange(rest.size) * stride) % ncols      # (all key columns in turn over the rows that are left)
    cols[lead_at] = np.asarray(large)[np.arange(n_lead) % len(large)]
    kind = (np.arange(n_lead) // len(large)) % 3
    inside[lead_at] = kind != 2
    high[lead_at] = kind == 1
    idx = np.arange(n_planted)
    W0 = window_of(x0.astype(np.float32))
    target = fractions(n_planted, inside, high) * W0[idx, cols]
    p = P[cols]
    xp = x0 + ((target - (x0 * p).sum(1)) / pn2[cols])[:, None] * p
    xp[tile_at] = bf16_rne(xp[tile_at].astype(np.float32)).astype(np.float64)
    # the group: every 8th key column of each of its rows, all inside
    sel = np.arange(0, ncols, 8)
    g0 = rng.standard_normal((group, dim))
    if group:
        Wg = window_of(g0.astype(np.float32))[:, sel]
        tg = fractions(group * sel.size, np.ones(group * sel.size, dtype=bool)).reshape(group, sel.size) * Wg
        Ps = P[sel]
        g0 = g0 + np.linalg.solve(Ps @ Ps.T, (tg - g0 @ Ps.T).T).T @ Ps
    # rows that are not planted
    zero = np.zeros((1, dim))
    nan = rng.standard_normal((1, dim))
    nan[0, min(3, dim - 1)] = np.nan
    scaled = rng.standard_normal((n_scaled, dim)) * np.where(np.arange(n_scaled) % 3 == 2, 2.0 ** -40, 2.0 ** 40)[:, None]
    x = np.concatenate([g0, zero, nan, scaled, xp]).astype(np.float32)
    n = x.shape[0]
    planted = np.zeros((n, ncols), dtype=bool)
    planted[:group, sel] = True
    assert first == n - n_planted
    planted[first + idx, cols] = True
    want_in = np.zeros((n, 1), dtype=bool)
    want_in[:group] = True
    want_in[first:, 0] = inside
    frac = np.zeros((n, ncols))             # the signed fraction of its window every planted projection is to sit at
    frac[first + idx, cols] = target / W0[idx, cols]
    if group:
        frac[:group, sel] = tg / Wg
    for _round in range(8):
        y = value_of(x)
        with np.errstate(all="ignore"):
            Wx = window_of(x)               # (the window moves with the row: ||x_mid|| feels a correction of 1e-4 ||x||)
            fr = np.abs(y.astype(np.float64)) / Wx
        ok = ~planted | np.where(want_in, (fr >= 0.02) & (fr <= 0.97), fr >= 1.12)
        bad = np.flatnonzero(~ok.all(axis=1))
        if bad.size == 0:
            break
        x64 = x.astype(np.float64)
        for i in bad:                       # (only the rows that miss: every cast draws the split's residual afresh)
            Ps = P[planted[i]]
            x64[i] -= np.linalg.solve(Ps @ Ps.T, y[i, planted[i]].astype(np.float64) - (frac[i] * Wx[i])[planted[i]]) @ Ps
        x = x64.astype(np.float32)
    else:
        raise AssertionError("the planted fractions did not settle")
    row_inside = np.zeros(n, dtype=bool)
    row_inside[:group] = True
    row_inside[first:] = inside
    return x, planted, row_inside, y


# ------------------------------------------------------------------------------------------------- cases
TAU1_UNITS = 300.0                # the caller's stage-1 window of the "tau1" form
TAU_UNITS = 256.0                 # the caller's tie window of the f32 pass
HASHER_SEED = 7
REFERENCE_BLAS = "openblas-haswell"

SIG16_SHAPES = [(16, 16, 768), (16, 16, 300),            # padded, one block: whole tiles / a partial last tile
                (32, 16, 384), (32, 16, 429),            # padded, two blocks
                # compact blocks: one / two / a partial tile.  (Two compact blocks need THREE padded ones - sig_compact: ncb < cb -,
                # so 40 x 10 x 416 and not 30 x 12 x 416, whose 480 padded columns are two blocks either way: the padded layout.)
                (20, 10, 768), (40, 10, 416), (20, 10, 429),
                (16, 8, 768), (24, 8, 300)]              # the narrow slot: 128 and 192 key columns
SIG16_W8_SHAPES = [(16, 16, 416), (20, 10, 768)]         # 256-row workgroups: 13 and 24 k-tiles, batches of > 128 row groups
SIG16R_SHAPES = [(16, 4, 128), (16, 16, 128), (5, 12, 64), (12, 16, 44), (16, 8, 256)]
BUCKET_SHAPES = [(16, 16, 768), (20, 10, 768), (32, 16, 384)]
W8_COPIES = 66
# the shapes whose first 128 rows want more than kS1ListCap = 4096 entries of one column block (tests/test_list_reference.py
# computes it): the 40 rows planted on every 8th column + 13 rows flagged wholesale, on blocks of 250 key columns and more
S1_OVERFLOW_SHAPES = {(16, 16, 300), (16, 16, 768), (32, 16, 384), (32, 16, 429), (40, 10, 416)}
F32_SHAPES = [(16, 16, 64), (8, 16, 64), (4, 16, 64), (2, 16, 64),       # NT = 8, 4, 2, 1 of the main geometry
              (16, 16, 768), (32, 16, 768),                              # the fine geometry at 512 rows
              (16, 16, 301)]                                             # rows at an odd 4-byte address, a scalar tail


def split_params(shapes):
    return [(nb, r, dim, lay, form) for nb, r, dim in shapes for lay in layouts(nb, r) for form in ("proven", "tau1")]


def f32_params():
    return [(nb, r, dim, lay, form) for nb, r, dim in F32_SHAPES for lay in layouts(nb, r) for form in ("proven", "tau")]


def gaussian_planes(nb, r, dim, seed=HASHER_SEED):
    """The hyperplanes LSHHasher(seed=...) draws (lshrs/hash/lsh.py:93-94): one generator, a float64 draw per band."""
    gen = np.random.default_rng(seed)
    return [gen.standard_normal((r, dim)).astype(np.float32) for _ in range(nb)]


def _coefficients(planes, r, dim):
    from lshrs_amd import _hostblas
    from lshrs_amd.windows import window_coefficients

    model = _hostblas.named_model(REFERENCE_BLAS, r, dim)
    assert model in (1, 2), (r, dim, model)
    ca, cb, ct, _info = window_coefficients(np.concatenate(planes, axis=0), int(model), r)
    return np.stack([ca, cb, ct]), model


def stage1_model(planes, x, workers=8):
    """oracle.build.split_stage1_model over row slices on a few threads (the C model releases the interpreter; the same bits)."""
    from concurrent.futures import ThreadPoolExecutor

    from oracle.build import load_mfma, split_stage1_model

    load_mfma()
    cuts = np.linspace(0, x.shape[0], workers + 1).astype(int)
    with ThreadPoolExecutor(workers) as pool:
        parts = list(pool.map(lambda i: split_stage1_model(planes, x[cuts[i]:cuts[i + 1]]), range(workers)))
    return np.concatenate(parts, axis=0)


class Case:
    """One case's inputs and verdicts (computed once, shared by the tests that run it; nothing here is changed afterwards)."""


@functools.lru_cache(maxsize=None)
def split_case(nb, r, dim, layout, form):
    """Split pass: hyperplanes, rows, stage 1's value of every projection (the accumulator model) and the verdicts for
    sig16r_kernel (`must_not`: W_up = W) and sig16_kernel (`must_not16`: W_up counts the last 32 elements once more)."""
    c = Case()
    compact = sig16_layout(nb, r, dim)["compact"]
    c.planes, c.large = scaled_planes(gaussian_planes(nb, r, dim), layout, compact[0] * r if compact else 256)
    c.coef, c.model = _coefficients(c.planes, r, dim)
    P = np.concatenate(c.planes, axis=0).astype(np.float64)
    c.pnorm = np.sqrt((P * P).sum(1))
    kw = dict(form=form, coef=c.coef, pnorm=c.pnorm, tau1_units=TAU1_UNITS)
    seed = 1000 * dim + 10 * nb + r + (500 if form == "tau1" else 0) + sum(map(ord, layout))
    c.x, c.planted, c.row_inside, c.y1 = build_batch(P, lambda x: split_windows(x, **kw)[0], lambda x: stage1_model(c.planes, x),
                                                     c.large, seed)
    c.W, c.W_up, c.wholesale, c.zero = split_windows(c.x, **kw)
    eps = band_eps(dim)
    c.must, c.must_not = judge(c.y1, c.W, c.W, eps, c.wholesale, c.zero)
    _, c.must_not16 = judge(c.y1, c.W, c.W_up, eps, c.wholesale, c.zero)
    c.key_cols = key_columns(nb, r)
    for a in (c.x, c.y1, c.must, c.must_not, c.must_not16, c.planted):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def f32_case(nb, r, dim, layout, form):
    """f32 pass: 512 rows (509 planted, a zero row, a NaN row, one scaled by 2^40), the chain's value of every projection and
    the verdicts of the strict test |y| < W."""
    from oracle.build import chain_project

    c = Case()
    c.planes, c.large = scaled_planes(gaussian_planes(nb, r, dim), layout)
    c.coef, c.model = _coefficients(c.planes, r, dim)
    P = np.concatenate(c.planes, axis=0).astype(np.float64)
    c.pnorm = np.sqrt((P * P).sum(1))
    kw = dict(form=form, coef_tie=c.coef[2], pnorm=c.pnorm, tau=TAU_UNITS * U)
    seed = 2000 * dim + 10 * nb + r + (500 if form == "tau" else 0) + sum(map(ord, layout))
    c.x, c.planted, c.row_inside, c.y = build_batch(P, lambda x: tie_windows(x, **kw), lambda x: chain_project(c.planes, x), c.large,
                                                    seed, n_planted=509, group=0, n_scaled=1, bf16_tiles=False)
    c.W = tie_windows(c.x, **kw)
    c.must, c.must_not = judge(c.y, c.W, c.W, band_eps(dim))
    c.key_cols = key_columns(nb, r)
    for a in (c.x, c.y, c.must, c.must_not, c.planted):
        a.setflags(write=False)
    return c


def workgroup_wants(c, wg_rows, compact_bpb=0, nb=0, r=0):
    """Entries every (row tile, 256-column block) workgroup of sig16_kernel must stage at the least: the `must` pairs of its
    rows and columns.  Padded layout: blocks of 256 padded columns; compact: `compact_bpb` whole bands per block."""
    n = c.must.shape[0]
    if compact_bpb:
        blk = (np.arange(nb).repeat(r)) // compact_bpb
    else:
        blk = c.key_cols // 256
    tiles = -(-n // wg_rows)
    out = np.zeros((tiles, int(blk.max()) + 1), dtype=np.int64)
    for t in range(tiles):
        rows = c.must[t * wg_rows:(t + 1) * wg_rows]
        for b in range(out.shape[1]):
            out[t, b] = int(rows[:, blk == b].sum())
    return out


def sig16_layout(nb, r, dim):
    """Which layout sig16_kernel runs a shape on - lshrs_common.h's sig_geom / sig_compact / sig_resident restated:
    -> dict(padcols, blocks of the padded geometry, compact (bands per block, blocks) or None, narrow, resident)."""
    bb = (r + 7) // 8
    padcols = nb * bb * 8
    tiles32 = -(-padcols // 32)
    nt = 8 if tiles32 >= 8 else (4 if tiles32 > 2 else (2 if tiles32 > 1 else 1))
    cb = -(-tiles32 // nt)
    compact = None
    if nt == 8 and r <= 128:
        bpb = 256 // r
        ncb = -(-nb // bpb)
        if ncb < cb:
            compact = (bpb, ncb)
    real = nb * r
    resident = False
    if real <= 256 and 8 <= dim <= 256:
        nct = ((real + 15) // 16 + 3) // 4 * 4
        kt = 2 if dim <= 64 else (4 if dim <= 128 else 8)
        resident = nct * kt <= 64
    return dict(padcols=padcols, tiles32=tiles32, nt=nt, cb=cb, ktiles=-(-dim // 32), compact=compact,
                narrow=nt < 8 and padcols >= 128, resident=resident)


def prefers_fine(nb, r, dim, m):
    """sig_prefer_fine of lshrs_common.h restated: does a partial round of m rows take the fine geometry?"""
    g = sig16_layout(nb, r, dim)
    if g["nt"] <= 1:
        return False
    layers = float(((m + 127) // 128 * g["cb"] + 255) // 256)
    t_main = layers * (4.4 * g["ktiles"] + 10.0)
    t_fine = 30.0 + 2.3e-5 * float(m) * g["tiles32"] * g["ktiles"]
    return t_fine < t_main
