"""The selection outline's specification in numpy ("Selection overlay"): which pixels are edge pixels, and
what an edge pixel becomes.  The mask is integer arithmetic on one f32 compare, the colour four roundings per channel in written
order, so a device image is compared with apply(ov, outline_mask(cover, ...), ...) bit for bit.

domain: bool [H, W], the pixels the pass defines (None: the whole image); band_domain builds a band context's.
inside(p) = cover[p] >= threshold for p in the domain (f32; a NaN is not inside); pixels outside the domain are neither inside
nor outside, are ignored by the neighbourhood and are never edge pixels.
side 0 (outer): edge(p) = !inside(p) and some q of the domain with inside(q) has (qx - px)^2 + (qy - py)^2 <= width^2;
side 1 (inner): the same with inside and !inside exchanged."""
import numpy as np

from depth_reference import BIN_PX, _fma

_f32 = np.float32
OUTER, INNER = 0, 1


def band_domain(W, H, band):
    """the pixels of a band context's bin columns that lie inside the image; band = (x0, x1) in pixels, whole bins"""
    dom = np.zeros((H, W), bool)
    dom[:, (band[0] // BIN_PX) * BIN_PX:min(-(-band[1] // BIN_PX) * BIN_PX, W)] = True
    return dom


def disc_offsets(width):
    r = int(width)
    return [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r]


def _dilate(src, width):
    """pixels with a set pixel of `src` within the disc (every offset shifted in turn: the definition, nothing cleverer)"""
    H, W = src.shape
    out = np.zeros_like(src)
    for dx, dy in disc_offsets(width):
        if abs(dy) >= H or abs(dx) >= W:           # the offset leaves the image from every pixel
            continue
        # out[y, x] |= src[y + dy, x + dx]
        ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
        xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
        out[yd, xd] |= src[ys, xs]
    return out


def outline_mask(cover, threshold, width, side, domain=None):
    cover = np.asarray(cover)
    assert cover.dtype == np.float32 and cover.ndim == 2 and side in (OUTER, INNER) and 1 <= int(width)
    dom = np.ones(cover.shape, bool) if domain is None else np.asarray(domain, bool)
    with np.errstate(invalid="ignore"):
        inside = dom & (cover >= _f32(threshold))
    outside = dom & ~inside
    source, target = (inside, outside) if side == OUTER else (outside, inside)
    return target & _dilate(source, width)


def apply(ov, mask, rgb, alpha):
    """k = 1.0f - alpha; out.c = fma(ov.c, k, rgb_c * alpha); out.a = fma(ov.a, k, alpha) where mask; ov elsewhere.  Every step in
    f32; the fma as tests/depth_reference.py states it (the exact product of two f32 in f64, the sum rounded once to f32)."""
    ov = np.asarray(ov)
    assert ov.dtype == np.float32 and ov.shape == mask.shape + (4,)
    alpha = _f32(alpha)
    k = _f32(_f32(1.0) - alpha)
    add = np.array([_f32(_f32(c) * alpha) for c in rgb] + [alpha], _f32)
    out = ov.copy()
    out[mask] = _fma(ov[mask], k, add[None, :])
    return out
