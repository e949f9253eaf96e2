"""Splat data, the specification in numpy f64 (include/gsplat_hip.h, "splat data"): the value of an attribute of every splat, the
histogram's edges, and what gsr_attr_stats, gsr_attr_histogram and gsr_select_attr return.  The scene arrives as the harness reads
it back (HIPRenderer.read_scene: data u32[8n], positions f32[3n], scales f32[3n]), the contribution accumulators as read_contrib
returns them, the selection and the hidden set as their words.  Nothing here looks at the device code."""
import numpy as np

ATTRS = {"x": 0, "y": 1, "z": 2, "distance": 3, "red": 4, "green": 5, "blue": 6, "opacity": 7, "scale_x": 8, "scale_y": 9, "scale_z": 10,
         "scale_min": 11, "scale_max": 12, "contrib_weight": 13, "contrib_peak": 14, "contrib_pixels": 15}
SCOPE_SELECTED, SCOPE_VISIBLE = 1, 2


def unpack(words, n):
    """bool[n] of a set's words (None: the empty set); bits at and above n do not count"""
    if words is None:
        return np.zeros(n, dtype=bool)
    w = np.asarray(words, dtype=np.uint32)
    i = np.arange(n)
    out = np.zeros(n, dtype=bool)
    ok = (i >> 5) < w.size
    out[ok] = ((w[i[ok] >> 5] >> (i[ok] & 31).astype(np.uint32)) & 1) != 0
    return out


def pack(bits):
    b = np.asarray(bits, dtype=bool)
    w = np.zeros(-(-b.size // 32), dtype=np.uint32)
    i = np.nonzero(b)[0]
    np.bitwise_or.at(w, i >> 5, (np.uint32(1) << (i & 31).astype(np.uint32)))
    return w


def attr_value(attr, data=None, positions=None, scales=None, origin=None, contrib=None):
    """float64[n]: the value of attribute `attr` (a name of ATTRS or its code) of every splat, in the header's order of operations"""
    a = ATTRS[attr] if isinstance(attr, str) else int(attr)
    if a <= 3:
        p = np.asarray(positions, dtype=np.float32).reshape(-1, 3).astype(np.float64)
        if a < 3:
            return p[:, a].copy()
        o = np.asarray(origin, dtype=np.float64).reshape(3)
        dx, dy, dz = p[:, 0] - o[0], p[:, 1] - o[1], p[:, 2] - o[2]
        with np.errstate(invalid="ignore", over="ignore"):
            return np.sqrt((dx * dx + dy * dy) + dz * dz)   # (IEEE: numpy's f64 sqrt is correctly rounded)
    if a <= 7:
        rgba = np.asarray(data, dtype=np.uint32).reshape(-1, 8)[:, 7]
        return ((rgba >> np.uint32(8 * (a - 4))) & np.uint32(0xff)).astype(np.float64)
    if a <= 12:
        s = np.asarray(scales, dtype=np.float32).reshape(-1, 3).astype(np.float64)
        if a <= 10:
            return s[:, a - 8].copy()
        nan = np.isnan(s).any(axis=1)
        with np.errstate(invalid="ignore"):
            v = s.min(axis=1) if a == 11 else s.max(axis=1)
        v[nan] = np.nan
        return v
    weight, peak, pixels = contrib
    if a == 13:
        return np.asarray(weight, dtype=np.uint64).astype(np.float64) * (1.0 / 16777216.0)
    if a == 14:
        return np.asarray(peak, dtype=np.float32).astype(np.float64)
    if a == 15:
        return np.asarray(pixels, dtype=np.uint32).astype(np.float64)
    raise ValueError("unknown attribute %r" % (attr,))


def edges(lo, hi, bins):
    """float64[bins + 1]: w = (hi - lo) / bins; edge(k) = k == bins ? hi : min(lo + k * w, hi)"""
    lo, hi = np.float64(lo), np.float64(hi)
    w = (hi - lo) / np.float64(bins)
    e = np.minimum(lo + np.arange(bins + 1, dtype=np.float64) * w, hi)
    e[bins] = hi
    return e


def in_scope(n, scope=0, sel_words=None, hid_words=None):
    m = np.ones(n, dtype=bool)
    if scope & SCOPE_SELECTED:
        m &= unpack(sel_words, n)
    if scope & SCOPE_VISIBLE:
        m &= ~unpack(hid_words, n)
    return m


def stats(v, scope_mask=None):
    """(count, nan, min, max) of the values in scope"""
    v = np.asarray(v, dtype=np.float64)
    if scope_mask is not None:
        v = v[scope_mask]
    nan = np.isnan(v)
    good = v[~nan]
    return int(v.size), int(nan.sum()), (float(good.min()) if good.size else np.inf), (float(good.max()) if good.size else -np.inf)


def histogram(v, lo, hi, bins, scope_mask=None):
    """(counts uint32[bins], (below, above, nan)): a value lo <= v < hi is in the largest bin b < bins with edge(b) <= v"""
    v = np.asarray(v, dtype=np.float64)
    if scope_mask is not None:
        v = v[scope_mask]
    e = edges(lo, hi, bins)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        below, above = v < e[0], v >= e[bins]
    inside = v[~nan & ~below & ~above]
    # the largest b with e[b] <= v among the first `bins` edges (searchsorted on a nondecreasing array: the insertion point behind equals)
    b = np.searchsorted(e[:bins], inside, side="right") - 1
    counts = np.bincount(b, minlength=bins).astype(np.uint32)
    return counts, (int(below.sum()), int(above.sum()), int(nan.sum()))


def select(v, lo, hi):
    """bool[n]: lo <= v < hi; a NaN is never picked"""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (v >= lo) & (v < hi)


def fold(sel, picked, op):
    """the selection after `op` (0 replace, 1 add, 2 subtract, 3 intersect) with the picked set"""
    sel, picked = np.asarray(sel, dtype=bool), np.asarray(picked, dtype=bool)
    return (picked, sel | picked, sel & ~picked, sel & picked)[op]
