"""SH colour that follows the scene through rotate / scale / limitBox ("SH frame"): the specification in numpy.

  * the frame's bookkeeping in f64 (frame_rotate, frame_scale: the statements gsr_scene_rotate / _scale and Scene.js execute);
  * the direction the projection evaluates SH for, in binary32 and in the written order (directions_f32);
  * the colour, through the oracle's eval_sh_rgb -- the oracle is only GIVEN the transformed direction;
  * the compaction of the three textures and the recount of bandsIndices under a limitBox (compact_sh, recount_bands).

Pure numpy apart from `colours`, which calls the CPU oracle.  Shared by tests/test_sh_follow_reference.py (no GPU) and
tests/test_gpu_sh_follow.py."""
import numpy as np

IDENTITY = np.eye(3, dtype=np.float64)
F = np.float32


# ---- the frame, f64 ----
def rotation_matrix(q):
    """R(q), q = (x, y, z, w), row-major 3x3: what k_scene_rotate and Scene.rotate build."""
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w],
                     [2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w],
                     [2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y]], dtype=np.float64)


def frame_rotate(L, q):
    """Linv <- Linv . R(q)^T, every entry (a*b + c*d) + e*f in f64."""
    R = rotation_matrix(q)
    out = np.empty((3, 3), dtype=np.float64)
    for i in range(3):
        for j in range(3):
            out[i, j] = (L[i, 0] * R[j, 0] + L[i, 1] * R[j, 1]) + L[i, 2] * R[j, 2]
    return out


def frame_scale(L, s):
    """Linv <- Linv . diag(1/sx, 1/sy, 1/sz): column j times the f64 reciprocal of s[j]."""
    out = np.empty((3, 3), dtype=np.float64)
    for i in range(3):
        for j in range(3):
            out[i, j] = L[i, j] * (1.0 / float(s[j]))
    return out


def frame_after(transforms, L=IDENTITY):
    """the frame after (("rotate" | "scale" | "translate" | "limit_box", values), ...) with follow on"""
    for name, v in transforms:
        if name == "rotate":
            L = frame_rotate(L, v)
        elif name == "scale":
            L = frame_scale(L, v)
    return L


# ---- the direction, binary32 ----
def camera_position_f32(view):
    """inverse(view)[3].xyz of the rigid column-major view matrix, as k_project_key computes it"""
    v = np.asarray(view, dtype=F).reshape(-1)
    cp = np.empty(3, dtype=F)
    for q in range(3):
        t = F(v[q * 4 + 0] * v[12])
        t = F(t + F(v[q * 4 + 1] * v[13]))
        t = F(t + F(v[q * 4 + 2] * v[14]))
        cp[q] = -t
    return cp


def directions_f32(positions, view, frame=None):
    """[n, 3] f32: normalize(p - camera), through the frame first when it is not the identity (m = (float)Linv):
         e_k = (m[k][0]*dvx + m[k][1]*dvy) + m[k][2]*dvz;  dl = sqrtf((e_0*e_0 + e_1*e_1) + e_2*e_2);  dir = e / dl"""
    p = np.asarray(positions, dtype=F).reshape(-1, 3)
    cp = camera_position_f32(view)
    d = [p[:, k] - cp[k] for k in range(3)]
    if frame is not None and not np.array_equal(np.asarray(frame, dtype=np.float64).reshape(3, 3), IDENTITY):
        m = np.asarray(frame, dtype=np.float64).reshape(3, 3).astype(F)
        d = [(m[k, 0] * d[0] + m[k, 1] * d[1]) + m[k, 2] * d[2] for k in range(3)]
    with np.errstate(invalid="ignore", divide="ignore"):
        dl = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        out = np.stack([d[0] / dl, d[1] / dl, d[2] / dl], axis=1)
    assert out.dtype == F
    return out


def degrees(n, band):
    """per splat: 0 = no SH, else the degree 1..3 (vertex.glsl.ts:180-204)"""
    i = np.arange(n)
    return np.where(i > band[0], np.where(i > band[1], np.where(i > band[2], 3, 2), 1), 0)


def colours(oracle, sh, band, positions, view, frame=None, only=None):
    """[n, 3] f32: the specification's colour of every SH splat (of those in the mask `only`); the others stay 0"""
    n = np.asarray(positions).size // 3
    d = directions_f32(positions, view, frame)
    deg = degrees(n, band)
    out = np.zeros((n, 3), dtype=F)
    first = int(band[0]) + 1
    for i in np.nonzero((deg > 0) & (True if only is None else only))[0]:
        out[i] = oracle.eval_sh_rgb(sh, i - first, deg[i], d[i])
    return out


# ---- the same polynomial in f64 (the yardstick of the f32 specification's own error) ----
C0, C1 = 0.28209479177387814, 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277, -0.5900435899266435)


def half_coefficients(tex):
    """u32[8 * count] -> f64[count, 16]: word j holds coefficients 2j (low half) and 2j + 1"""
    w = np.asarray(tex, dtype=np.uint32).reshape(-1, 8)
    h = np.stack([w & 0xffff, w >> 16], axis=2).reshape(-1, 16).astype(np.uint16)
    return h.view(np.float16).astype(np.float64)


def colours_f64(sh, band, positions, view):
    """eval_sh_rgb (vertex.glsl.ts:57-104) in f64 for the direction normalize(p - camera) in f64: [n, 3], 0 for splats without SH"""
    p = np.asarray(positions, dtype=F).reshape(-1, 3).astype(np.float64)
    v = np.asarray(view, dtype=F).reshape(-1).astype(np.float64)
    cp = np.array([-(v[q * 4] * v[12] + v[q * 4 + 1] * v[13] + v[q * 4 + 2] * v[14]) for q in range(3)])
    d = p - cp
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    n = p.shape[0]
    deg = degrees(n, band)
    first = int(band[0]) + 1
    x, y, z = d[first:, 0], d[first:, 1], d[first:, 2]
    dg = deg[first:]
    out = np.zeros((n, 3))
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    for ch in range(3):
        k = half_coefficients(sh[ch])[:n - first].T
        r = C0 * k[0] - (C1 * y * k[1] + C1 * z * k[2] - C1 * x * k[3])
        s2 = (C2[0] * xy * k[4] + C2[1] * yz * k[5] + C2[2] * (2 * zz - xx - yy) * k[6] + C2[3] * xz * k[7] + C2[4] * (xx - yy) * k[8])
        s3 = (C3[0] * y * (3 * xx - yy) * k[9] + C3[1] * xy * z * k[10] + C3[2] * y * (4 * zz - xx - yy) * k[11] +
              C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * k[12] + C3[4] * x * (4 * zz - xx - yy) * k[13] + C3[5] * z * (xx - yy) * k[14] +
              C3[6] * x * (xx - 3 * yy) * k[15])
        r = r + np.where(dg > 1, s2, 0.0) + np.where(dg > 2, s3, 0.0)
        out[first:, ch] = np.clip(r + 0.5, 0.0, 1.0)
    return out


# ---- limitBox ----
def keep_mask(positions, box):
    """Scene.limitBox's test (Scene.ts:307-366) on f32 positions against the f64 box (xMin, xMax, yMin, yMax, zMin, zMax)"""
    p = np.asarray(positions, dtype=F).reshape(-1, 3).astype(np.float64)
    b = [float(v) for v in box]
    return (p[:, 0] >= b[0]) & (p[:, 0] <= b[1]) & (p[:, 1] >= b[2]) & (p[:, 1] <= b[3]) & (p[:, 2] >= b[4]) & (p[:, 2] <= b[5])


def recount_bands(band, keep):
    """band'[k] = (number of kept splats with index <= band[k]) - 1, through the exclusive prefix at band[k] + 1 clamped to [0, n]"""
    keep = np.asarray(keep, dtype=bool)
    prefix = np.concatenate([[0], np.cumsum(keep)])
    return np.array([int(prefix[min(max(int(b) + 1, 0), keep.size)]) - 1 for b in band], dtype=np.int32)


def compact_sh(sh, band, keep):
    """(textures of 8 * sh_count' words, band', sh_count'): the 8-word groups of the kept SH splats (i > band[0]), in order;
    sh_count' = kept - (band'[0] + 1); sh_count' == 0 is the cleared state: empty textures, band (-1, -1, -1)"""
    keep = np.asarray(keep, dtype=bool)
    first = int(band[0]) + 1
    rows_kept = keep[first:]
    nb = recount_bands(band, keep)
    count = int(keep.sum()) - (int(nb[0]) + 1)
    assert count == int(rows_kept.sum())
    if count == 0:
        return [np.zeros(0, dtype=np.uint32) for _ in range(3)], np.array([-1, -1, -1], dtype=np.int32), 0
    out = [np.ascontiguousarray(np.asarray(t, dtype=np.uint32)[:8 * rows_kept.size].reshape(-1, 8)[rows_kept].reshape(-1)) for t in sh]
    return out, nb, count
