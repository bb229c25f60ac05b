"""The arithmetic of the exhaustive scan (csrc/scan_pass.inc, the norms and the division of csrc/scan.hip) at the ends of the
ranges lshrs_scan_epsilon is stated for, on the GPU.

The reference is the float64 cosine of the rows AS STORED (upcast by torch), the scores are those of EVERY (query, row)
(tests/_scan_reference.all_pairs_approx - not only the members of a window), and the one tolerance is the project's own:
|a - cos| <= lshrs_scan_epsilon(elem, dim).  Every case prints max |a - cos| / epsilon; DESIGN.md (K6) records what an MI355X
printed.  Where two layouts of the same rows are scanned - vector loads of whole chunks (ALIGNED) and element-wise loads - their
scores must be the same bits: the register image is the same."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import _scan_reference as R

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "bfloat16", "float16", "int8", "float8_e4m3fn")
# below one MFMA step (1 .. 7), round a step (8, 16), round half a chunk (32), at and just past whole 64-chunks (64, 128, 192)
LADDER = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192)
M, Q = 600, 70
_RAW = {4: "int32", 2: "int16", 1: "uint8"}


def _torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _layouts(torch, stored):
    """The same rows twice: `aligned` - 16-byte base, a row stride that is a multiple of 16 elements (ALIGNED = true) - and
    `odd` - an odd row stride, the base one element into its allocation (the element path; as
    tests/test_gpu_exact_above.py::test_unaligned_rows builds it).  Everything between the rows is 0x7f bytes - huge values
    or NaNs in every type: a read at k >= dim would show."""
    m, dim = int(stored.shape[0]), int(stored.shape[1])
    raw_t = getattr(torch, _RAW[stored.element_size()])
    raw = stored.contiguous().view(raw_t)
    junk = int.from_bytes(b"\x7f" * stored.element_size(), "little")
    wide = torch.full((m, (dim + 15) // 16 * 16 + 16), junk, dtype=raw_t, device="cuda")
    wide[:, :dim] = raw
    aligned = wide.view(stored.dtype)[:, :dim]
    ld = dim + (3 if dim % 2 == 0 else 4)
    flat = torch.full((m * ld + 1,), junk, dtype=raw_t, device="cuda")
    torch.as_strided(flat, (m, dim), (ld, 1), 1).copy_(raw)
    odd = torch.as_strided(flat.view(stored.dtype), (m, dim), (ld, 1), 1)
    assert aligned.data_ptr() % 16 == 0 and aligned.stride(0) % 16 == 0
    assert odd.stride(0) % 2 == 1 and odd.data_ptr() == flat.data_ptr() + stored.element_size() and odd.data_ptr() % 16 != 0
    assert torch.equal(aligned.contiguous().view(raw_t), raw)
    assert torch.equal(odd.contiguous().view(raw_t), raw)
    return aligned, odd


def _cos64(stored, Qs):
    x = stored.float().cpu().numpy().astype(np.float64)
    q = Qs.astype(np.float64)
    return (q @ x.T) / (np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(x, axis=1)[None, :])


def _check(torch, stored, Qs, label, both_layouts=False):
    """|A - cos64| <= epsilon for every pair of A (no NaN, error word 0: asserted by all_pairs_approx); returns the ratio."""
    from lshrs_amd._exact import scan_epsilon

    dim = int(stored.shape[1])
    eps = scan_epsilon(stored.dtype, dim)
    assert 0 < eps <= 2.0 ** -7
    Qd = torch.from_numpy(np.ascontiguousarray(Qs, dtype=np.float32)).cuda()
    if both_layouts:
        aligned, odd = _layouts(torch, stored)
        A, _ = R.all_pairs_approx(aligned, Qd)
        B, _ = R.all_pairs_approx(odd, Qd)
        differ = int((A.view(np.uint32) != B.view(np.uint32)).sum())
        assert differ == 0, f"{label}: {differ} scores of the vector-load and the element-load layouts are not the same bits"
    else:
        A, _ = R.all_pairs_approx(stored, Qd)
    assert not np.isnan(A).any()
    cos = _cos64(stored, Qs)
    assert np.isfinite(cos).all()
    worst = float(np.abs(A.astype(np.float64) - cos).max())
    print(f"scan range end: {label}: max |a - cos| / epsilon = {worst / eps:.4f} (max |a - cos| {worst:.3e}, epsilon {eps:.3e})")
    assert worst <= eps, f"{label}: max |a - cos| {worst:.3e} beyond epsilon {eps:.3e}"
    return worst / eps


def _gaussian(seed, m, dim, q):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((m, dim)).astype(np.float32), rng.standard_normal((q, dim)).astype(np.float32)


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("dim", LADDER)
def test_dim_ladder_on_both_load_paths(dim, name):
    torch = _torch()
    X, Qs = _gaussian(3000 + dim, M, dim, Q)
    _check(torch, R._stored_form(torch, name, X), Qs, f"dim {dim} {name}", both_layouts=True)


@functools.lru_cache(maxsize=None)
def _long_rows(positive):
    X, Qs = _gaussian(16_384 + positive, M, 16_384, 5)
    if positive:
        X, Qs = np.abs(X), np.abs(Qs)
    X.setflags(write=False)
    Qs.setflags(write=False)
    return X, Qs


@pytest.mark.parametrize("positive", (False, True), ids=("gaussian", "positive"))
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("dim", (16_383, 16_384))
def test_largest_dim(dim, name, positive):
    """The far end of the stated range, where epsilon (5.3e-3 / 7.6e-3) is close to the 2^-7 at which it stops being useful.
    All-positive data: sum |q_i x_i| = q . x, the accumulation bound's worst case."""
    torch = _torch()
    X, Qs = _long_rows(positive)
    stored = R._stored_form(torch, name, np.array(X[:, :dim]))
    _check(torch, stored, np.array(Qs[:, :dim]), f"dim {dim} {name} {'positive' if positive else 'gaussian'}")


def _scaled(seed, dim, low, high):
    """Row i times 2^e_i, e_i uniform in [low, high]; query j times 2^+20 or 2^-20."""
    rng = np.random.default_rng(seed)
    X, Qs = _gaussian(seed + 1, M, dim, Q)
    X = np.ldexp(X, rng.integers(low, high + 1, size=(M, 1))).astype(np.float32)
    Qs = np.ldexp(Qs, rng.choice((-20, 20), size=(Q, 1))).astype(np.float32)
    return X, Qs


@pytest.mark.parametrize("dim", (100, 772))
@pytest.mark.parametrize("case", ("float32", "bfloat16", "float16", "float32-one-large-element"))
def test_rows_and_queries_far_from_unit_scale(case, dim):
    torch = _torch()
    name = case.split("-")[0]
    if name == "float16":
        X, Qs = _scaled(50 + dim, dim, -10, 4)
        X[::3] = _gaussian(60 + dim, M, dim, 1)[0][::3]                 # every third row: unit scale ...
        X[::3, 1::2] *= np.float32(2.0 ** -16)                          # ... with every other element an f16 subnormal
    else:
        # (one element 2^20 times the others: the rows' own scale stops at 2^20, so that ||x||^2 stays inside f32)
        X, Qs = _scaled(50 + dim, dim, -40, 20 if case.endswith("one-large-element") else 40)
        if case.endswith("one-large-element"):
            at = np.random.default_rng(70 + dim).integers(0, dim, size=M)
            X[np.arange(M), at] *= np.float32(2.0 ** 20)
    stored = R._stored_form(torch, name, X)
    if name == "float16":
        a = stored[::3].float().abs()
        sub, normal = (a > 0) & (a < 2.0 ** -14), a >= 2.0 ** -14
        assert bool(sub.any(dim=1).all()) and bool(normal.any(dim=1).all()), "rows that mix f16 subnormals with normals"
    assert bool(torch.isfinite(stored.float()).all()) and bool((stored.float().abs().amax(dim=1) > 0).all())
    _check(torch, stored, Qs, f"scale {case} dim {dim}", both_layouts=True)


@pytest.mark.parametrize("dim", (100, 772))
def test_worst_case_split(dim):
    """f32 rows and queries, all positive, the low 16 mantissa bits all ones: the largest truncation residual the split can
    leave, on both operands and all of one sign."""
    torch = _torch()
    X, Qs = _gaussian(900 + dim, M, dim, Q)
    X = (np.abs(X).view(np.uint32) | np.uint32(0xFFFF)).view(np.float32)
    Qs = (np.abs(Qs).view(np.uint32) | np.uint32(0xFFFF)).view(np.float32)
    assert np.isfinite(X).all() and np.isfinite(Qs).all()
    _check(torch, R._stored_form(torch, "float32", X), Qs, f"worst-case split float32 dim {dim}", both_layouts=True)


@pytest.mark.parametrize("dim", (16, 17, 100))
@pytest.mark.parametrize("name", ("int8", "float8_e4m3fn"))
def test_every_code(name, dim):
    """Rows built from raw bytes, over every code of the type: int8 with -128, e4m3fn with -0 (0x80) and the subnormals
    (0x01 .. 0x07, 0x81 .. 0x87) - codes quantize_rows never emits.  The two NaN codes of e4m3fn are no finite data."""
    torch = _torch()
    rng = np.random.default_rng(40 + dim)
    codes = np.arange(256, dtype=np.uint8)
    if name == "float8_e4m3fn":
        codes = codes[(codes & 0x7F) != 0x7F]
        assert codes.shape[0] == 254
    raw = codes[rng.integers(0, codes.shape[0], size=(M, dim))]
    assert np.unique(raw).shape[0] == codes.shape[0], "not every code was drawn"
    stored = torch.from_numpy(raw).cuda().view(getattr(torch, name))
    assert bool((stored.float().abs().amax(dim=1) > 0).all())
    if name == "int8":
        assert int(stored.min().item()) == -128
    _, Qs = _gaussian(41 + dim, 1, dim, Q)
    _check(torch, stored, Qs, f"every code {name} dim {dim}", both_layouts=True)
