"""The depth plane of a depth ring (gsr_delivery_open_depth), restated in numpy from DESIGN.md section 4 ("Frame delivery with
depth") and from nothing else: which pixels of the hit plane are delivered, and the 16-bit quantiser, all in binary32."""
import numpy as np

STEPS = (1, 2)


def plane_size(W, H, step):
    """(Wd, Hd): ceil(W / step) columns, ceil(H / step) rows"""
    return (W + step - 1) // step, (H + step - 1) // step


def subsample(hit, step):
    """sample (i, j) of the delivered plane is pixel (step * i, step * j) of the hit plane: a point sample"""
    assert step in STEPS
    return np.ascontiguousarray(np.asarray(hit)[::step, ::step])


def quantise_u16(z, near):
    """u = 65535 unless z > 0; otherwise q = min(near / z, 1) and u = rint(q * 65535), every step a binary32 operation
    (correctly rounded division and product, round half to even)"""
    z = np.asarray(z, dtype=np.float32)
    near = np.float32(near)
    assert np.isfinite(near) and near > 0
    pos = z > 0                                               # False for 0, negatives and NaN
    with np.errstate(divide="ignore", over="ignore", invalid="ignore", under="ignore"):
        q = np.divide(near, np.where(pos, z, np.float32(1)), dtype=np.float32)
        q = np.minimum(q, np.float32(1))
        u = np.rint(q * np.float32(65535)).astype(np.uint16)
    return np.where(pos, u, np.uint16(65535)).astype(np.uint16)


def dequantise_u16(u, near):
    """what a client recovers: z ~ near * 65535 / u (u = 0: no hit)"""
    u = np.asarray(u).astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.where(u > 0, float(np.float32(near)) * 65535.0 / u, np.inf)
