"""The definition of the delivery ring's 4:2:0 Y'CbCr frames ("Frame delivery in Y'CbCr") in plain numpy,
from an [H, W, 4] uint8 image: what gsr_read_pixels_rgba8 returns for the frame, premultiplied.  Everything is integer
arithmetic, so the device's payload must equal this byte for byte."""
import numpy as np

# BT.709 in 1/256: (y0, Y row, Cb row, Cr row, chroma clamp)
LIMITED = (16, (47, 157, 16), (-26, -86, 112), (112, -102, -10), (16, 240))
FULL = (0, (54, 183, 19), (-29, -99, 128), (128, -116, -12), (0, 255))


def layout(W, H, fmt):
    """{bytes, trailer, planes: [(offset, stride, rows)]} of a W x H frame; the trailer lies at the payload rounded up to 4."""
    Wc, Hc = (W + 1) // 2, (H + 1) // 2
    if fmt == "rgba8":
        planes, size = [(0, W * 4, H)], W * H * 4
    elif fmt == "nv12":
        planes, size = [(0, W, H), (W * H, 2 * Wc, Hc)], W * H + 2 * Wc * Hc
    elif fmt == "i420":
        planes, size = [(0, W, H), (W * H, Wc, Hc), (W * H + Wc * Hc, Wc, Hc)], W * H + 2 * Wc * Hc
    else:
        raise ValueError(fmt)
    return {"bytes": size, "trailer": (size + 3) // 4 * 4, "planes": planes}


def over_background(rgba, background=(0, 0, 0)):
    """[H, W, 3] int64: the premultiplied pixel laid over the background, min(255, c + ((255 - a) * bg + 127) // 255)"""
    px = rgba.astype(np.int64)
    t = 255 - px[..., 3:4]
    return np.minimum(255, px[..., :3] + (t * np.asarray(background, dtype=np.int64) + 127) // 255)


def planes(rgba, full_range=False, background=(0, 0, 0)):
    """(Y [H, W], Cb [Hc, Wc], Cr [Hc, Wc]) uint8"""
    y0, cy, cb, cr, (lo, hi) = FULL if full_range else LIMITED
    rgb = over_background(rgba, background)
    H, W = rgb.shape[:2]
    Y = y0 + ((rgb @ np.asarray(cy, dtype=np.int64) + 128) >> 8)
    # 2 x 2 sums with the coordinates clamped to the image: odd sizes replicate the last column / row
    ys = np.minimum(np.arange(2 * ((H + 1) // 2)), H - 1)
    xs = np.minimum(np.arange(2 * ((W + 1) // 2)), W - 1)
    p = rgb[ys][:, xs]
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    Cb = np.clip(128 + ((s @ np.asarray(cb, dtype=np.int64) + 512) >> 10), lo, hi)     # (>> on int64: arithmetic, i.e. floor)
    Cr = np.clip(128 + ((s @ np.asarray(cr, dtype=np.int64) + 512) >> 10), lo, hi)
    return Y.astype(np.uint8), Cb.astype(np.uint8), Cr.astype(np.uint8)


def payload(rgba, fmt, full_range=False, background=(0, 0, 0)):
    """the slot's payload bytes (1-D uint8) in `fmt` ("nv12" / "i420")"""
    Y, Cb, Cr = planes(rgba, full_range, background)
    if fmt == "nv12":
        return np.concatenate([Y.ravel(), np.stack([Cb, Cr], axis=-1).ravel()])
    if fmt == "i420":
        return np.concatenate([Y.ravel(), Cb.ravel(), Cr.ravel()])
    raise ValueError(fmt)


def to_rgb_float(Y, Cb, Cr, full_range=False):
    """the float BT.709 inverse ([H, W, 3] in 0..255, chroma upsampled by replication): what a decoder shows"""
    H, W = Y.shape
    up = lambda c: np.repeat(np.repeat(c.astype(np.float64), 2, axis=0), 2, axis=1)[:H, :W]
    if full_range:
        y, pb, pr = Y / 255.0, (up(Cb) - 128) / 255.0, (up(Cr) - 128) / 255.0
    else:
        y, pb, pr = (Y - 16.0) / 219.0, (up(Cb) - 128) / 224.0, (up(Cr) - 128) / 224.0
    kr, kb = 0.2126, 0.0722
    r = y + 2 * (1 - kr) * pr
    b = y + 2 * (1 - kb) * pb
    g = (y - kr * r - kb * b) / (1 - kr - kb)
    return np.stack([r, g, b], axis=-1) * 255.0
