"""The compositor's staging mask -- which 8 x 8 quadrants of a 32 x 32 bin an entry is walked in -- as a numpy statement of
k_blend.hip's staging block, f32, operation for operation (the device code is compiled without contraction: every product
and sum below is one rounding, as there), and the truth it must never undercut: a (splat, quadrant) pair is COVERED when
some pixel centre of the quadrant passes the walk's own test, tests/depth_reference.py's coverage_q <= 4.

    records are rec[8] = (cx, cy, ux, uy, wx, wy, log2 opacity, colour word); vPosition = (u . d, w . d), d = pixel - centre

    two_axes:   the separating axes u and w plus the bounding circle -- the rule of k_blend2 (two waves per tile)
    four_axes:  the same plus the diagonals (u + w) / sqrt 2 and (u - w) / sqrt 2 -- the rule of k_blend / k_blend_unfused

The masks are conservative culls: a quadrant left out must hold no covered pixel, a quadrant left in costs only time."""
import numpy as np

from depth_reference import BIN_PX, coverage_q

_f32 = np.float32
HALF = _f32(3.5)         # a quadrant's pixel centres lie within 3.5 px of its centre in x and in y
CU = _f32(2.0005)        # |vPosition.x|, |vPosition.y| <= 2 plus the rounding slack of the sums
CP = _f32(2.8295)        # |vPosition.x +- vPosition.y| <= 2 sqrt 2 plus twice that slack and one more addition (k_blend.hip)
CIRCLE = _f32(4.002)


def _columns_rows(rec, bin_x0, bin_y0):
    """vPosition at the centres of the bin's 16 quadrants, [n, row, column], and the distances of the circle test"""
    rec = np.asarray(rec, _f32).reshape(-1, 8)
    cx, cy, ux, uy, wx, wy = (rec[:, j] for j in range(6))
    qx = (np.arange(4) * 8 + 4 + int(bin_x0)).astype(_f32)      # (float)(binX0 + 8 k + 4): exact
    qy = (np.arange(4) * 8 + 4 + int(bin_y0)).astype(_f32)
    dcx = qx[None, :] - cx[:, None]
    dcy = qy[None, :] - cy[:, None]
    ucol, wcol = ux[:, None] * dcx, wx[:, None] * dcx
    ur, wr = uy[:, None] * dcy, wy[:, None] * dcy
    vxc = ucol[:, None, :] + ur[:, :, None]
    vyc = wcol[:, None, :] + wr[:, :, None]
    ddx = np.maximum(np.abs(dcx) - HALF, _f32(0.0))
    ddy = np.maximum(np.abs(dcy) - HALF, _f32(0.0))
    dist2 = (ddx * ddx)[:, None, :] + (ddy * ddy)[:, :, None]
    return rec, vxc, vyc, dist2


def two_axes(rec, bin_x0, bin_y0):
    """bool[n, 4 rows, 4 columns]: the quadrants of the bin at (bin_x0, bin_y0) flagged by the u, w and circle tests"""
    rec, vxc, vyc, dist2 = _columns_rows(rec, bin_x0, bin_y0)
    ux, uy, wx, wy = (rec[:, j] for j in range(2, 6))
    eu = HALF * (np.abs(ux) + np.abs(uy)) + CU
    ew = HALF * (np.abs(wx) + np.abs(wy)) + CU
    minlen2 = np.minimum(ux * ux + uy * uy, wx * wx + wy * wy)
    return (np.abs(vxc) <= eu[:, None, None]) & (np.abs(vyc) <= ew[:, None, None]) & (dist2 * minlen2[:, None, None] <= CIRCLE)


def four_axes(rec, bin_x0, bin_y0, cp=CP):
    """bool[n, 4 rows, 4 columns]: the shipped rule of the one-wave-per-tile kernels (cp: the diagonal constant, for the
    tests of its slack)"""
    rec, vxc, vyc, _ = _columns_rows(rec, bin_x0, bin_y0)
    ux, uy, wx, wy = (rec[:, j] for j in range(2, 6))
    ep = HALF * (np.abs(ux + wx) + np.abs(uy + wy)) + _f32(cp)
    em = HALF * (np.abs(ux - wx) + np.abs(uy - wy)) + _f32(cp)
    diagonals = (np.abs(vxc + vyc) <= ep[:, None, None]) & (np.abs(vxc - vyc) <= em[:, None, None])
    return two_axes(rec, bin_x0, bin_y0) & diagonals


def covered(rec, bin_x0, bin_y0):
    """bool[n, 4 rows, 4 columns]: brute force -- some pixel centre of the quadrant has coverage_q <= 4"""
    rec = np.asarray(rec, _f32).reshape(-1, 8)
    xs, ys = np.arange(BIN_PX) + int(bin_x0), np.arange(BIN_PX) + int(bin_y0)
    out = np.zeros((len(rec), 4, 4), bool)
    for i, rc in enumerate(rec):
        keep = coverage_q(rc, xs, ys) <= _f32(4.0)
        out[i] = keep.reshape(4, 8, 4, 8).any(axis=(1, 3))
    return out


def bins_of(W, H):
    """the origins of the frame's bins"""
    return [(x, y) for y in range(0, H, BIN_PX) for x in range(0, W, BIN_PX)]
