"""Splat selection, the specification in numpy ("Selection"): which splats a screen region picks -- from the
ORACLE's projection (oracle.project: rec, bbox) or from an index plane, never from anything the selection kernels wrote --, which a
world box picks, the ops on bool arrays, and the packing into words."""
import numpy as np

NONE = 0xFFFFFFFF
OPS = ("replace", "add", "subtract", "intersect")


def pack(picked):
    """bool[n] -> uint32[ceil(n / 32)]: splat i is bit i & 31 of word i >> 5; the bits at and above n are 0."""
    b = np.asarray(picked, dtype=bool).reshape(-1)
    words = np.zeros(-(-b.size // 32), dtype=np.uint32)
    i = np.nonzero(b)[0]
    np.bitwise_or.at(words, i >> 5, (np.uint32(1) << (i & 31).astype(np.uint32)).astype(np.uint32))
    return words


def unpack(words, n):
    w = np.asarray(words, dtype=np.uint32)
    i = np.arange(n)
    return ((w[i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(bool)


def apply_op(S, P, op):
    S, P = np.asarray(S, dtype=bool), np.asarray(P, dtype=bool)
    return {"replace": P.copy(), "add": S | P, "subtract": S & ~P, "intersect": S & P}[op]


def listed(bbox, band=None):
    """The splats a frame lists: a non-empty pixel box; on a band context (band = its pixel columns [px0, px1), whole bins) a box
    that touches the band."""
    vis = (bbox[:, 0] <= bbox[:, 2]) & (bbox[:, 1] <= bbox[:, 3])
    if band is not None:
        vis &= (bbox[:, 2] >= band[0]) & (bbox[:, 0] < band[1])
    return vis


def in_region(X, Y, rect, mask=None):
    """Which of the pixels (X[k], Y[k]) -- float or int arrays; anything outside the rectangle, NaN included, is out -- lie in the
    region: rect = (x0, y0, x1, y1), mask [y1 - y0, stride >= x1 - x0] with non-zero = inside, row 0 = y0."""
    x0, y0, x1, y1 = rect
    with np.errstate(invalid="ignore"):
        ok = (X >= x0) & (X < x1) & (Y >= y0) & (Y < y1)
    if mask is not None:
        m = np.asarray(mask)
        assert m.ndim == 2 and m.shape[0] >= y1 - y0 and m.shape[1] >= x1 - x0
        k = np.nonzero(ok)[0]
        ok[k] = m[(Y[k] - y0).astype(np.int64), (X[k] - x0).astype(np.int64)] != 0
    return ok


def centre_pick(rec, bbox, rect, mask=None, band=None):
    """GSR_SELECT_CENTRE: listed, and the centre pixel (floor(cx), floor(cy)) in the region."""
    X, Y = np.floor(rec[:, 0].astype(np.float64)), np.floor(rec[:, 1].astype(np.float64))
    return listed(bbox, band) & in_region(X, Y, rect, mask)


def hit_pick(index, n, rect, mask=None):
    """GSR_SELECT_HIT: the values of the index plane [H, W] at the region's pixels."""
    x0, y0, x1, y1 = rect
    ys, xs = np.mgrid[y0:y1, x0:x1]
    ok = in_region(xs.reshape(-1), ys.reshape(-1), rect, mask)
    vals = index[y0:y1, x0:x1].reshape(-1)[ok]
    vals = vals[vals != NONE]
    out = np.zeros(n, dtype=bool)
    out[vals] = True
    return out


def box_pick(positions, box):
    """gsr_select_box: limitBox's comparisons, f64 on the f32 positions."""
    p = np.asarray(positions, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    b = [float(v) for v in box]
    return (p[:, 0] >= b[0]) & (p[:, 0] <= b[1]) & (p[:, 1] >= b[2]) & (p[:, 1] <= b[3]) & (p[:, 2] >= b[4]) & (p[:, 2] <= b[5])


def disc(cx, cy, radius, stride_pad=0):
    """(rect, mask) of the pixels whose centre lies within `radius` of (cx, cy); the mask's rows are stride_pad bytes longer than
    the rectangle is wide, and the padding is non-zero so that a reader with the wrong stride is found out."""
    x0, y0, x1, y1 = int(np.floor(cx - radius)), int(np.floor(cy - radius)), int(np.ceil(cx + radius)), int(np.ceil(cy + radius))
    ys, xs = np.mgrid[y0:y1, x0:x1]
    inside = (xs + 0.5 - cx) ** 2 + (ys + 0.5 - cy) ** 2 <= radius * radius
    mask = np.full((y1 - y0, x1 - x0 + stride_pad), 255, dtype=np.uint8)
    mask[:, :x1 - x0] = inside * 255
    return (x0, y0, x1, y1), mask
