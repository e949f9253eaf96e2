"""tests/outline_reference.py, the selection outline's specification, pinned on hand-made planes: the disc of every width around
a single pixel, pixels on the image's edges and corners, full and empty planes, inner against outer of the complement, a band
domain, a NaN, the threshold's tie, and the colour step by step."""
import numpy as np
import pytest

import outline_reference as OL

f32 = np.float32


def _plane(h, w, at=()):
    c = np.zeros((h, w), f32)
    for x, y in at:
        c[y, x] = 1.0
    return c


def _disc(h, w, cx, cy, r):
    """the disc by brute force over the pixels, in integers"""
    return np.array([[(x - cx) ** 2 + (y - cy) ** 2 <= r * r for x in range(w)] for y in range(h)])


@pytest.mark.parametrize("width", [1, 2, 3, 16])
def test_a_single_pixel_gives_the_disc_minus_its_centre(width):
    n = 2 * width + 5
    c = n // 2
    m = OL.outline_mask(_plane(n, n, [(c, c)]), 0.5, width, OL.OUTER)
    want = _disc(n, n, c, c, width)
    want[c, c] = False
    assert np.array_equal(m, want)
    assert m.sum() == {1: 4, 2: 12, 3: 28, 16: 796}[width]
    # the row extents are the half-widths floor(sqrt(r^2 - dy^2))
    for dy in range(-width, width + 1):
        hw = max(h for h in range(width + 1) if h * h + dy * dy <= width * width)
        xs = np.flatnonzero(want[c + dy] | (dy == 0) * (np.arange(n) == c))
        assert xs.min() == c - hw and xs.max() == c + hw
    # the single pixel has no inner outline wider than itself: it is inside and next to pixels that are not
    inner = OL.outline_mask(_plane(n, n, [(c, c)]), 0.5, width, OL.INNER)
    assert inner.sum() == 1 and inner[c, c]


@pytest.mark.parametrize("at", [(0, 0), (8, 0), (0, 5), (8, 6), (4, 0), (4, 6), (0, 3), (8, 3)])
def test_a_pixel_on_an_edge_or_corner_is_clipped_to_the_image(at):
    h, w = 7, 9
    for width in (1, 2, 3):
        m = OL.outline_mask(_plane(h, w, [at]), 0.5, width, OL.OUTER)
        want = _disc(h, w, at[0], at[1], width)
        want[at[1], at[0]] = False
        assert np.array_equal(m, want), (at, width)


def test_full_and_empty_planes_have_no_outline():
    full, empty = np.ones((9, 70), f32), np.zeros((9, 70), f32)
    for width in (1, 16):
        for side in (OL.OUTER, OL.INNER):
            assert not OL.outline_mask(full, 0.5, width, side).any()       # the image's border is not an edge: nothing outside the domain counts
            assert not OL.outline_mask(empty, 0.5, width, side).any()


def test_inner_is_the_outer_outline_of_the_complement_within_the_domain():
    rng = np.random.default_rng(5)
    cover = (rng.random((40, 150)) < 0.02).astype(f32)
    cover[10:25, 30:90] = 1.0
    dom = OL.band_domain(150, 40, (32, 128))
    for domain in (None, dom):
        d = np.ones(cover.shape, bool) if domain is None else domain
        comp = np.where(d & (cover < 0.5), f32(1.0), f32(0.0))
        for width in (1, 2, 5):
            inner = OL.outline_mask(cover, 0.5, width, OL.INNER, domain)
            assert np.array_equal(inner, OL.outline_mask(comp, 0.5, width, OL.OUTER, domain)) and inner.any()
            outer = OL.outline_mask(cover, 0.5, width, OL.OUTER, domain)
            assert not (inner & outer).any() and not (outer & (cover >= 0.5)).any() and (inner <= (cover >= 0.5)).all()


def test_a_band_domain_is_neither_neighbour_nor_written():
    h, w = 11, 160
    band = (64, 128)
    dom = OL.band_domain(w, h, band)
    assert dom[:, 64:128].all() and not dom[:, :64].any() and not dom[:, 128:].any()
    assert OL.band_domain(333, 3, (320, 333))[:, 320:].all()                  # the last bin column is clipped to the image
    # an inside pixel just outside the band draws nothing inside it; one just inside draws nothing outside it
    c = _plane(h, w, [(63, 5), (130, 5)])
    assert not OL.outline_mask(c, 0.5, 3, OL.OUTER, dom).any()
    c = _plane(h, w, [(64, 5)])
    m = OL.outline_mask(c, 0.5, 3, OL.OUTER, dom)
    want = _disc(h, w, 64, 5, 3) & dom
    want[5, 64] = False
    assert np.array_equal(m, want) and not m[:, :64].any()
    # inner: the band's border is not an edge (what lies beyond it is not "not inside")
    full = np.ones((h, w), f32)
    assert not OL.outline_mask(full, 0.5, 3, OL.INNER, dom).any()
    full[5, 63] = 0.0                                                          # a hole outside the domain changes nothing
    assert not OL.outline_mask(full, 0.5, 3, OL.INNER, dom).any()
    full[5, 64] = 0.0
    assert OL.outline_mask(full, 0.5, 3, OL.INNER, dom).sum() == 17            # the half disc of radius 3 without its centre


def test_a_nan_is_not_inside_and_the_tie_is():
    c = np.zeros((5, 5), f32)
    c[2, 2] = np.nan
    assert not OL.outline_mask(c, 0.5, 1, OL.OUTER).any()
    full = np.ones((5, 5), f32)
    full[2, 2] = np.nan
    assert OL.outline_mask(full, 0.5, 1, OL.INNER).sum() == 4                   # the NaN is a hole: its four neighbours are the inner edge
    t = f32(0.3)
    c = np.zeros((5, 5), f32)
    c[2, 2] = t
    c[0, 0] = np.nextafter(t, f32(0))
    m = OL.outline_mask(c, t, 1, OL.OUTER)
    assert m.sum() == 4 and m[2, 1] and not m[0, 1]                             # cover == threshold is inside, one ulp below is not


def test_apply_is_four_roundings_in_written_order():
    ov = np.array([[[0.3, 0.7, 0.1, 0.9], [0.2, 0.4, 0.6, 0.8]]], f32)
    mask = np.array([[True, False]])
    rgb, alpha = (0.125, 7.0, -3.0), f32(0.4)
    out = OL.apply(ov, mask, rgb, alpha)
    assert out.dtype == f32 and np.array_equal(out[0, 1].view(np.uint32), ov[0, 1].view(np.uint32))
    k = f32(1.0) - alpha
    from fractions import Fraction as F
    for ch in range(4):
        add = alpha if ch == 3 else f32(rgb[ch]) * alpha                        # rounded to f32 before the fma
        exact = F(float(ov[0, 0, ch])) * F(float(k)) + F(float(add))            # the fma: one rounding of the exact value
        lo, hi = np.nextafter(out[0, 0, ch], f32(-np.inf)), np.nextafter(out[0, 0, ch], f32(np.inf))
        assert abs(F(float(out[0, 0, ch])) - exact) <= min(abs(F(float(lo)) - exact), abs(F(float(hi)) - exact)), ch
    # alpha 1 replaces the pixel, alpha 0 leaves it (k = 1, + 0)
    one = OL.apply(ov, mask, rgb, 1.0)
    assert np.array_equal(one[0, 0], np.array([0.125, 7.0, -3.0, 1.0], f32))
    assert np.array_equal(OL.apply(ov, mask, rgb, 0.0), ov)
    assert not ov.flags.writeable or np.array_equal(ov[0, 0], np.array([0.3, 0.7, 0.1, 0.9], f32))   # the input is not changed
