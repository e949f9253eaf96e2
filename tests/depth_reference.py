"""What the depth planes must BE: a numpy statement of DESIGN.md section 4 ("Depth planes and pick"), fed by the ORACLE
(oracle.project -> rec, bbox, raw[:, 10]; oracle.sort -> the order), never by device read-backs.

    For a pixel, its fragments are the splats in depth order whose pixel box holds it and whose coverage test passes:
    vx, vy relative to the centre of the first pixel of the pixel's 32 x 32 bin, with the compositor's fused multiply-adds
    (f32; an fma is the f64 product-sum rounded once to f32), q = fma(vy, vy, vx * vx), kept iff q <= 4, weight
    B = exp2(la - q log2(e)).  z of a splat is raw[:, 10] (w of the centre's clip position).  From T = 1, D = 0:
        w = T * B;  D += w * z;  T -= w;  the first fragment with 1 - T >= hit_alpha is the pixel's hit
    (the sums in f64).  mean = D, hit = z of the hit (+inf: none), index = its splat (0xffffffff: none), alpha = 1 - T.

Knife edges -- pixels where a rounding of the device's f32 walk may legitimately decide otherwise -- are returned as a
mask and left out of comparisons: a fragment with |q - 4| <= 1e-4 whose weight T * B could still be seen (above 1e-6:
behind a saturated pixel an edge fragment changes nothing, and the dense centre of a large scene has thousands of
fragments per pixel), or accumulated alpha within 1e-4 of hit_alpha after some fragment."""
import numpy as np

BIN_PX = 32
NONE = 0xFFFFFFFF
EDGE = 1e-4
SEEN = 1e-6
LOG2E = 1.4426950408889634
_f32, _f64 = np.float32, np.float64


def _fma(a, b, c):
    return (np.asarray(a, _f64) * np.asarray(b, _f64) + np.asarray(c, _f64)).astype(_f32)


def coverage_q(rc, xs, ys):
    """q of the record rc[8] at the pixels ys x xs (int arrays), shape [len(ys), len(xs)], in the compositor's f32 arithmetic"""
    rc = np.asarray(rc, _f32)
    bx0, by0 = (xs // BIN_PX) * BIN_PX, (ys // BIN_PX) * BIN_PX
    cxr = (rc[0] - (bx0.astype(_f32) + _f32(0.5)))[None, :]
    cyr = (rc[1] - (by0.astype(_f32) + _f32(0.5)))[:, None]
    pxl, pyl = (xs - bx0).astype(_f32)[None, :], (ys - by0).astype(_f32)[:, None]
    ncu = -_fma(rc[3], cyr, rc[2] * cxr)
    ncw = -_fma(rc[5], cyr, rc[4] * cxr)
    vx = _fma(rc[2], pxl, _fma(rc[3], pyl, ncu))
    vy = _fma(rc[4], pxl, _fma(rc[5], pyl, ncw))
    return _fma(vy, vy, vx * vx)


def depth_planes_reference(rec, bbox, z, order, W, H, window=None, hit_alpha=0.5):
    """The planes of the window (x0, y0, w, h) (default: the image) as a dict: mean f64, hit f32, index u32, alpha f64,
    mask bool (knife edges), all [h, w]."""
    x0, y0, w, h = window or (0, 0, W, H)
    rec = np.asarray(rec, _f32).reshape(-1, 8)
    bb = np.asarray(bbox, np.int64).reshape(-1, 4)
    z = np.asarray(z, _f32).reshape(-1)
    T = np.ones((h, w), _f64)
    D = np.zeros((h, w), _f64)
    hit = np.full((h, w), np.inf, _f32)
    index = np.full((h, w), NONE, np.uint32)
    mask = np.zeros((h, w), bool)
    order = np.asarray(order, np.int64).reshape(-1)
    inside = (bb[:, 0] <= bb[:, 2]) & (bb[:, 1] <= bb[:, 3]) & (bb[:, 2] >= x0) & (bb[:, 0] < x0 + w) & (bb[:, 3] >= y0) & (bb[:, 1] < y0 + h)
    for i in order[inside[order]]:
        xa, xb = max(bb[i, 0], x0), min(bb[i, 2], x0 + w - 1, W - 1)
        ya, yb = max(bb[i, 1], y0), min(bb[i, 3], y0 + h - 1, H - 1)
        if xa > xb or ya > yb:
            continue
        q = coverage_q(rec[i], np.arange(xa, xb + 1), np.arange(ya, yb + 1))
        sl = (slice(ya - y0, yb - y0 + 1), slice(xa - x0, xb - x0 + 1))
        keep = q <= _f32(4.0)
        edge = np.abs(q.astype(_f64) - 4.0) <= EDGE
        if not (keep.any() or edge.any()):
            continue
        B = np.exp2(_f64(rec[i, 6]) - q.astype(_f64) * LOG2E)
        mask[sl] |= edge & (T[sl] * B > SEEN)
        B = np.where(keep, B, 0.0)
        wgt = T[sl] * B
        D[sl] += wgt * _f64(z[i])
        T[sl] -= wgt
        alpha = 1.0 - T[sl]
        mask[sl] |= keep & (np.abs(alpha - hit_alpha) <= EDGE)
        new = keep & (index[sl] == NONE) & (alpha >= hit_alpha)
        index[sl] = np.where(new, np.uint32(i), index[sl])
        hit[sl] = np.where(new, z[i], hit[sl])
    return {"mean": D, "hit": hit, "index": index, "alpha": 1.0 - T, "mask": mask}
