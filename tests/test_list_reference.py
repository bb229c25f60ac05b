"""CPU tests of tests/_list_reference.py: the inputs of tests/test_gpu_list_completeness.py are inside the conditions that
give those tests their power - checked here, without a GPU, for every parametrised case."""
from __future__ import annotations

import numpy as np
import pytest

from tests import _list_reference as L

SPLIT = sorted(set(L.split_params(L.SIG16_SHAPES + L.SIG16_W8_SHAPES + L.SIG16R_SHAPES + L.BUCKET_SHAPES)))


def _conditions(c, must_not, dim):
    must = int(c.must.sum())
    und = int((~c.must & ~must_not).sum())
    planted_must = int((c.must & c.planted).sum())
    assert und * 100 <= must, (und, must)                       # the undecided band: at most 1 % of the must set
    assert planted_must >= 150, planted_must
    # the planted fractions keep clear of the band: every planted projection of a row inside the guarded range has a verdict
    assert not (c.planted & ~c.must & ~must_not).any()
    # ... and the verdict is the one it was planted for (a fraction below 1: must; above: must not)
    assert (c.must[c.planted] == np.broadcast_to(c.row_inside[:, None], c.planted.shape)[c.planted]).all()
    return must, und, planted_must


@pytest.mark.parametrize("nb,r,dim,layout,form", SPLIT)
def test_split_pass_inputs_have_power(nb, r, dim, layout, form):
    c = L.split_case(nb, r, dim, layout, form)
    g = L.sig16_layout(nb, r, dim)
    must, und, planted = _conditions(c, c.must_not if g["resident"] else c.must_not16, dim)
    n = c.x.shape[0]
    assert int(c.zero.sum()) == 1 and int(np.isnan(c.x).any(axis=1).sum()) == 1 and int(c.wholesale.sum()) == 12
    assert not c.must[c.zero].any() and c.must[c.wholesale].all()
    assert np.unique(c.x, axis=0).shape[0] == n                 # distinct rows
    # every large column is planted inside its window at least 8 times, and every key column is planted
    for col in c.large:
        assert int((c.planted[:, col] & c.must[:, col]).sum()) >= 8, col
    assert c.planted[40:].any(axis=0).sum() >= min(c.planted.shape[1], 400)
    # the windows really are uneven: the large column's coefficient is 16 x (two blocks) or more above every other block's largest
    pn = c.pnorm
    assert pn[c.large].max() > 30 * np.median(pn)
    print(f"{nb} x {r} x {dim} {layout} {form}: must {must}, undecided {und}, planted must {planted}")


def test_one_workgroup_outgrows_its_lds_stage():
    """At least one case makes a 128-row workgroup of sig16_kernel want more than kS1ListCap = 4096 entries (the group of 40
    rows planted on every 8th column + the rows flagged wholesale): the overflow branches of the append run."""
    over = set()
    for nb, r, dim, layout, form in L.split_params(L.SIG16_SHAPES):
        c = L.split_case(nb, r, dim, layout, form)
        g = L.sig16_layout(nb, r, dim)
        bpb = g["compact"][0] if g["compact"] else 0
        wants = int(L.workgroup_wants(c, 128, bpb, nb, r).max())
        assert (wants > L.S1_LIST_CAP[4]) == ((nb, r, dim) in L.S1_OVERFLOW_SHAPES), (nb, r, dim, layout, form, wants)
        if wants > L.S1_LIST_CAP[4]:
            over.add((nb, r, dim))
    assert over == L.S1_OVERFLOW_SHAPES and set(L.BUCKET_SHAPES) & over       # (the bucket form's overflow branch runs too)


@pytest.mark.parametrize("nb,r,dim,layout,form", L.f32_params())
def test_f32_pass_inputs_have_power(nb, r, dim, layout, form):
    c = L.f32_case(nb, r, dim, layout, form)
    assert c.x.shape[0] == 512
    _conditions(c, c.must_not, dim)
    for col in c.large:
        assert int((c.planted[:, col] & c.must[:, col]).sum()) >= 8, col


def test_layouts_restate_the_library():
    """The shapes reach the layout they are listed under (sig_geom / sig_compact / sig_resident restated)."""
    lay = {s: L.sig16_layout(*s) for s in L.SIG16_SHAPES + L.SIG16_W8_SHAPES + L.SIG16R_SHAPES}
    for s in [(16, 16, 768), (16, 16, 300), (16, 16, 416)]:
        assert lay[s]["cb"] == 1 and not lay[s]["compact"] and not lay[s]["narrow"] and not lay[s]["resident"], s
    for s in [(32, 16, 384), (32, 16, 429)]:
        assert lay[s]["cb"] == 2 and not lay[s]["compact"], s
    assert lay[(20, 10, 768)]["compact"] == (25, 1) and lay[(20, 10, 429)]["compact"] == (25, 1)
    assert lay[(40, 10, 416)]["compact"] == (25, 2) and lay[(40, 10, 416)]["cb"] == 3
    assert lay[(16, 8, 768)]["narrow"] and lay[(16, 8, 768)]["padcols"] == 128
    assert lay[(24, 8, 300)]["narrow"] and lay[(24, 8, 300)]["padcols"] == 192 and lay[(24, 8, 300)]["cb"] == 2
    assert all(lay[s]["resident"] for s in L.SIG16R_SHAPES)
    assert not any(lay[s]["resident"] for s in L.SIG16_SHAPES + L.SIG16_W8_SHAPES)
    # 256-row workgroups: more than 11 k-tiles (and the test tiles the rows to more than 128 row groups)
    assert all(lay[s]["ktiles"] > 11 for s in L.SIG16_W8_SHAPES)
    # the f32 pass: NT = 8, 4, 2, 1 in the main geometry at 64-d; the fine geometry at 512 rows of 301 and 768 elements
    assert [L.sig16_layout(*s)["nt"] for s in L.F32_SHAPES[:4]] == [8, 4, 2, 1]
    assert [L.prefers_fine(*s, 512) for s in L.F32_SHAPES] == [False, False, False, False, True, True, True]


def test_uneven_scales_are_powers_of_two_and_mirrored():
    for ncols in (60, 128, 192, 200, 256):
        for layout in ("first", "middle", "last"):
            s, large = L.uneven_scales(ncols, layout)
            assert len(large) == 1 and s[large[0]] == 64 and (np.delete(s, large) == 1).all()
    for ncols in (400, 512):
        a, la = L.uneven_scales(ncols, "A")
        b, lb = L.uneven_scales(ncols, "B")
        assert np.all(np.log2(a) == np.round(np.log2(a))) and np.all(np.log2(b) == np.round(np.log2(b)))
        assert a[:256].max() == 64 and a[256:].max() == 4 and b[:256].max() == 4 and b[256:].max() == 64
        assert la[0] % 256 != la[1] % 256 and set(la) != set(lb)


def test_the_judge_on_a_hand_made_table():
    y = np.array([[0.5, 1.0, 1.5, np.nan, 0.0]])
    W = np.ones((1, 5))
    must, must_not = L.judge(y, W, 1.2 * W, 0.01)
    assert must.tolist() == [[True, False, False, False, True]] and must_not.tolist() == [[False, False, True, True, False]]
    must, must_not = L.judge(y, W, W, 0.01, wholesale=np.array([True]))
    assert must.all() and not must_not.any()
    must, must_not = L.judge(np.zeros((1, 2)), np.zeros((1, 2)), np.zeros((1, 2)), 0.01, zero=np.array([True]))
    assert not must.any() and must_not.all()
