"""Rotating SH coefficients ("Rotating SH coefficients"): the specification in numpy.

  * the basis B_1 .. B_15, the direction factors of eval_sh_rgb as vertex.glsl.ts:72-98 writes them (basis);
  * the band matrices of a rotation in f64, by sample-and-solve over 24 Fibonacci-sphere directions (matrices);
  * the rotation of the coefficients in f32 in the stated order, stored as halves rounded to nearest even (apply);
  * the condition under which a frame is baked, and the quaternion it is baked with (bake);
  * how far the colour of the coefficient form may lie from the colour of the frame form (colour_bound), and how far a rotation
    and its inverse may leave a band from where it was (round_trip_bound).

Pure numpy.  Shared by tests/test_sh_rotate_reference.py, tests/test_sh_rotate_abi.py (no GPU) and tests/test_gpu_sh_rotate.py."""
import numpy as np

import sh_follow_reference as sf

F = np.float32
BANDS = ((1, 3), (4, 5), (9, 7))     # (first coefficient, width) of bands 1, 2, 3
SAMPLES = 24
NAN_HALF = 0x7e00


# ---- the basis ----
def basis(d):
    """[..., 3] unit directions -> [..., 15]: B_1 .. B_15 in f64"""
    d = np.asarray(d, dtype=np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    C1, C2, C3 = sf.C1, sf.C2, sf.C3
    return np.stack([-C1 * y, -C1 * z, C1 * x,
                     C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy),
                     C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                     C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)], axis=-1)


def fibonacci(count=SAMPLES):
    """[count, 3]: phi = acos(1 - 2(i + 0.5) / count), theta = pi (1 + sqrt 5)(i + 0.5)"""
    i = np.arange(count, dtype=np.float64) + 0.5
    phi, theta = np.arccos(1.0 - 2.0 * i / count), np.pi * (1.0 + np.sqrt(5.0)) * i
    return np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], axis=1)


def unit(q):
    """q / |q| in f64, |q| = sqrt(((xx + yy) + zz) + ww); None for a q that is not finite or has no length"""
    q = np.asarray(q, dtype=np.float64).reshape(4)
    if not np.isfinite(q).all():
        return None
    with np.errstate(over="ignore"):
        length = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    if not (length > 0.0 and np.isfinite(length)):
        return None
    return q / length


# ---- the matrices, f64 ----
def matrices(q):
    """(D_1 [3, 3], D_2 [5, 5], D_3 [7, 7]) of the rotation R(q / |q|): c' = D_l c makes sum c'_k B_k(R d) = sum c_k B_k(d).
    Each solves Y_l(S)^T D_l = Y_l(R^T S)^T in the least-squares sense over the 24 directions S; x = y = z = 0: the exact identity."""
    u = unit(q)
    assert u is not None, "q must be finite and not zero"
    if u[0] == 0.0 and u[1] == 0.0 and u[2] == 0.0:
        return tuple(np.eye(w) for _, w in BANDS)
    R = sf.rotation_matrix(u)
    S = fibonacci()
    Y, Z = basis(S), basis(S @ R)        # (a row of S @ R is (R^T d)^T)
    return tuple(np.linalg.lstsq(Y[:, j0 - 1:j0 - 1 + w], Z[:, j0 - 1:j0 - 1 + w], rcond=None)[0] for j0, w in BANDS)


def conjugate(q):
    x, y, z, w = (float(v) for v in q)
    return (-x, -y, -z, w)


def multiply(a, b):
    """the quaternion of R(a) R(b), (x, y, z, w)"""
    x1, y1, z1, w1 = (float(v) for v in a)
    x2, y2, z2, w2 = (float(v) for v in b)
    return (w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2,
            w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2)


# ---- the halves of a texture ----
def halves(tex):
    """u32[8 * rows] -> u16[rows, 16]: half 2j in the low 16 bits of word j"""
    w = np.asarray(tex, dtype=np.uint32).reshape(-1, 8)
    return np.stack([w & 0xffff, w >> 16], axis=2).reshape(-1, 16).astype(np.uint16)


def words(h):
    """u16[rows, 16] -> u32[8 * rows]"""
    h = np.asarray(h, dtype=np.uint16).reshape(-1, 8, 2).astype(np.uint32)
    return np.ascontiguousarray((h[:, :, 0] | (h[:, :, 1] << 16)).reshape(-1))


# ---- the rotation of the coefficients, f32 ----
def apply_halves(h, M32):
    """u16[rows, 16] -> u16[rows, 16]: per band and k in band order s = M[k][j0] * c[j0]; s = s + M[k][j] * c[j], j ascending, every
    product and sum rounded to f32; stored as a half rounded to nearest even, any NaN as 0x7e00; half 0 keeps its bits."""
    h = np.asarray(h, dtype=np.uint16).reshape(-1, 16)
    c = h.view(np.float16).astype(F)
    out = h.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for (j0, w), M in zip(BANDS, M32):
            M = np.asarray(M)
            assert M.dtype == F and M.shape == (w, w)
            for k in range(w):
                s = M[k, 0] * c[:, j0]
                for j in range(1, w):
                    s = s + M[k, j] * c[:, j0 + j]
                assert s.dtype == F
                bits = s.astype(np.float16).view(np.uint16)
                out[:, j0 + k] = np.where(np.isnan(s), np.uint16(NAN_HALF), bits)
    return out


def m32(D):
    """the f64 matrices rounded once to f32"""
    return tuple(np.asarray(d, dtype=np.float64).astype(F) for d in D)


def apply(tex, band, selected, M32):
    """the three textures after gsr_scene_rotate_sh: the rows of the splats i > band[0] (of those whose entry of the bool mask
    `selected` over the splats is set; None: every SH row) rotated, every other row as it was"""
    first = int(band[0]) + 1
    out = []
    for t in tex:
        h = halves(t)
        rows = np.ones(h.shape[0], dtype=bool) if selected is None else np.asarray(selected, dtype=bool)[first:first + h.shape[0]]
        h[rows] = apply_halves(h[rows], M32)
        out.append(words(h))
    return out


def rows_in_scope(n, band, selected):
    first = int(band[0]) + 1
    return n - first if selected is None else int(np.asarray(selected, dtype=bool)[first:n].sum())


# ---- baking a frame ----
BAKE_TOLERANCE = 2.0 ** -20


def bake(linv):
    """the quaternion (x, y, z, w) float64[4] gsr_scene_bake_sh_frame rotates the coefficients by, or None where it refuses:
    s2 = (sum L_ij^2) / 3; max |(L L^T)_ij / s2 - delta_ij| <= 2^-20 and det > 0; Q = L / sqrt(s2); Shepperd's branches on R = Q^T.
    The identity frame: (0, 0, 0, 1)."""
    L = np.asarray(linv, dtype=np.float64).reshape(3, 3)
    if np.array_equal(L, sf.IDENTITY):
        return np.array([0.0, 0.0, 0.0, 1.0])
    s2 = 0.0
    for v in L.reshape(-1):
        s2 += v * v
    s2 = s2 / 3.0
    if not (np.isfinite(s2) and s2 > 0.0):
        return None
    worst = 0.0
    for i in range(3):
        for j in range(3):
            g = (L[i, 0] * L[j, 0] + L[i, 1] * L[j, 1]) + L[i, 2] * L[j, 2]
            e = abs(g / s2 - (1.0 if i == j else 0.0))
            if not e <= worst:
                worst = e
    det = (L[0, 0] * (L[1, 1] * L[2, 2] - L[1, 2] * L[2, 1]) - L[0, 1] * (L[1, 0] * L[2, 2] - L[1, 2] * L[2, 0])) + \
        L[0, 2] * (L[1, 0] * L[2, 1] - L[1, 1] * L[2, 0])
    if not (worst <= BAKE_TOLERANCE and det > 0.0):
        return None
    R = (L / np.sqrt(s2)).T
    tr = (R[0, 0] + R[1, 1]) + R[2, 2]
    if tr > 0.0:
        s = np.sqrt(tr + 1.0) * 2.0
        w, x, y, z = 0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = np.sqrt(((1.0 + R[0, 0]) - R[1, 1]) - R[2, 2]) * 2.0
        w, x, y, z = (R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s
    elif R[1, 1] > R[2, 2]:
        s = np.sqrt(((1.0 + R[1, 1]) - R[0, 0]) - R[2, 2]) * 2.0
        w, x, y, z = (R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s
    else:
        s = np.sqrt(((1.0 + R[2, 2]) - R[0, 0]) - R[1, 1]) * 2.0
        w, x, y, z = (R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s
    return np.array([x, y, z, w], dtype=np.float64)


# ---- bounds ----
def round_trip_bound(c, w):
    """how far (2-norm) a band of width w may lie from c after apply(q) and apply(q^-1).  Each store rounds a value x to within
    2^-11 |x| (nearest even, normal halves) or 2^-25 (half the subnormal quantum), so a band moves by at most 2^-11 ||x|| +
    sqrt(w) 2^-25 per store and there are two stores: 2 * 2^-11 ||c|| + 2 sqrt(w) 2^-25.  The factor 1 + 2^-9 pays for the rest,
    each of it below 2^-10 of the first term: the f32 sums ((w + 1) 2^-24 ||c|| per rotation), the f32 rounding of the two
    matrices (their product is the identity to 2 sqrt(w) 2^-24) and the second store rounding a band that is 2^-11 longer."""
    c = np.asarray(c, dtype=np.float64)
    return 2.0 * 2.0 ** -11 * (1.0 + 2.0 ** -9) * np.linalg.norm(c, axis=-1) + 2.0 * np.sqrt(w) * 2.0 ** -25


def colour_bound(tex, band, q, positions, view):
    """[n, 3] f64: how far the colour of the coefficient form (coefficients `tex` rotated by q on the device, evaluated for the
    direction d = normalize(p - camera)) may lie from the colour of the frame form (the coefficients `tex` evaluated through the
    frame R(q)^T), per splat and channel; 0 for splats without SH.  Evaluated in f64 from the exact rotated coefficients
    x = D(q) c.  In exact arithmetic the two colours are equal (the defining property), so the bound is the sum of what is rounded:
      * the stored coefficient: |c'_k - x_k| <= 2^-11 |x_k| (1 + 2^-10) + 2^-25 (the store, nearest even; the subnormal quantum)
        + 2^-21 ||x_band|| (the f32 matrix and the f32 sums: (w + 1) 2^-24 sum_j |M_kj| |c_j| <= 8 * 2^-24 ||c_band||); it enters
        the colour through |B_k(d)|;
      * the two f32 evaluations, each below 2^-16 sum_k |coefficient_k| (the DC coefficient included: the sums round against it): the direction is within 2^-20 of the exact one (the
        frame's entries rounded to f32, five operations through it, the normalisation), a B_k of degree l <= 3 and maximum <= 0.75
        moves by at most 2 l 0.75 2^-20 under it, the at most 8 operations of a factor whose intermediate values stay below 3 * 2.9
        add 70 * 2^-24, and the 16 sums another 16 * 0.75 * 2^-24;
      * 2^-22 for the two final additions of 0.5.  The clamps to [0, 1] move nothing apart."""
    n = np.asarray(positions).size // 3
    first = int(band[0]) + 1
    p = np.asarray(positions, dtype=F).reshape(-1, 3).astype(np.float64)
    v = np.asarray(view, dtype=F).reshape(-1).astype(np.float64)
    cp = np.array([-(v[k * 4] * v[12] + v[k * 4 + 1] * v[13] + v[k * 4 + 2] * v[14]) for k in range(3)])
    d = p[first:] - cp
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    B = np.abs(basis(d))
    D = matrices(q)
    out = np.zeros((n, 3))
    for ch in range(3):
        c = sf.half_coefficients(tex[ch])[:n - first]
        per = np.zeros((n - first, 15))
        x_all = np.zeros((n - first, 15))
        for (j0, w), Dl in zip(BANDS, D):
            x = c[:, j0:j0 + w] @ Dl.T
            x_all[:, j0 - 1:j0 - 1 + w] = x
            per[:, j0 - 1:j0 - 1 + w] = 2.0 ** -11 * (1.0 + 2.0 ** -10) * np.abs(x) + 2.0 ** -25 + \
                2.0 ** -21 * np.linalg.norm(x, axis=1, keepdims=True)
        out[first:, ch] = (B * per).sum(axis=1) + 2.0 ** -16 * (2.0 * np.abs(c[:, 0]) + np.abs(c[:, 1:]).sum(axis=1) + np.abs(x_all).sum(axis=1)) + 2.0 ** -22
    return out
