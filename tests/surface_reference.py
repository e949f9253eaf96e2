"""Point-to-plane registration, the specification in numpy f64 (include/gsplat_hip.h, "point-to-plane registration"): the rows of 29
doubles along the target's stored f32 normals, their fixed tree, the 6 x 6 Cholesky solve with its Cayley step and the registration
loop -- every operation in the header's written order, so that the device and the host library are compared with it bit for bit.
The match, the transformed point, compose and delta are register_reference's, unchanged.  Also corner_scenario(), the box corner
of the registration tests, and families(), the shapes of tests/test_gpu_surface.py.

Vector work is element-wise numpy (one rounding per operation, never a dot product or a sum); the solve is Python floats."""
import math

import numpy as np

import normal_reference as nref
import register_reference as rr

NONE = rr.NONE
ROW = 29
GROUP = rr.GROUP
CONVERGED, MAX_ITERATIONS, TOO_FEW, DEGENERATE = 0, 1, 2, 3
MIN_PAIRS = 6
PIVOT = 2.0 ** -40


def _normals(normals):
    return np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)


# ---- the rows ----
def rows(source, target, normals, idx, M=None, d2=None):
    """float64[n, 29]: (J_a * J_b for a <= b, J_a * r, r * r, d2) with J = (T x n, n) and r = n . (T - Q) for a matched splat whose
    match has a normal (n_x no NaN); 29 times +0.0 for every other"""
    src, tgt, nrm = rr._positions(source), rr._positions(target), _normals(normals)
    t, _ = rr.transform(src, M)
    idx = np.asarray(idx)
    out = np.zeros((src.shape[0], ROW), np.float64)
    i = np.nonzero(idx != NONE)[0]
    i = i[~np.isnan(nrm[idx[i], 0])]
    j = idx[i]
    T, Q, n = t[i], tgt[j].astype(np.float64), nrm[j].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = T - Q
        r = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
        J = [T[:, 1] * n[:, 2] - T[:, 2] * n[:, 1], T[:, 2] * n[:, 0] - T[:, 0] * n[:, 2], T[:, 0] * n[:, 1] - T[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]]
        at = 0
        for a in range(6):
            for b in range(a, 6):
                out[i, at] = J[a] * J[b]
                at += 1
        for a in range(6):
            out[i, 21 + a] = J[a] * r
        out[i, 27] = r * r
    out[i, 28] = np.asarray(d2, np.float64)[i]
    return out


def tree(x, width=ROW):
    """float64[width]: register_reference.tree's fixed tree at another row width -- groups of 256 consecutive rows, the last padded
    with +0.0; within a group for s = 128, 64, .., 1: x[l] = x[l] + x[l + s] for l < s; the group results the same way"""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, width)
    if not x.shape[0]:
        return np.zeros(width, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        while True:
            g = (x.shape[0] + GROUP - 1) // GROUP
            y = np.zeros((g * GROUP, width), np.float64)
            y[:x.shape[0]] = x
            y = y.reshape(g, GROUP, width)
            s = GROUP // 2
            while s:
                y[:, :s] = y[:, :s] + y[:, s:2 * s]
                s //= 2
            x = y[:, 0].copy()
            if g == 1:
                return x[0]


def sums(source, target, normals, idx, d2, M=None):
    """(pairs, surface_pairs, float64[29])"""
    idx = np.asarray(idx)
    matched = idx != NONE
    has = ~np.isnan(_normals(normals)[idx[matched], 0])
    return int(matched.sum()), int(has.sum()), tree(rows(source, target, normals, idx, M, d2))


def step_rms(count, value):
    return math.sqrt(float(value) * (1.0 / float(count))) if count else math.inf


# ---- the solve: Cholesky on the 6 x 6 normal equations and the Cayley step, Python floats in the header's order ----
def surface_solve(surface_pairs, sum29):
    """(D float64[12], rms or None, degenerate): degenerate = j + 1 when pivot j is not above the floor (D the identity, no rms);
    ValueError for what gsr_surface_solve refuses"""
    s = [float(v) for v in np.asarray(sum29, np.float64).reshape(ROW)]
    if surface_pairs < MIN_PAIRS or not all(math.isfinite(v) for v in s):
        raise ValueError("surface_pairs < 6 or a non-finite sum")
    inv = 1.0 / float(surface_pairs)
    A = [[0.0] * 6 for _ in range(6)]
    at = 0
    for a in range(6):
        for b in range(a, 6):
            A[a][b] = A[b][a] = s[at]
            at += 1
    g = [-s[21 + a] for a in range(6)]
    floor = max(A[a][a] for a in range(6)) * PIVOT
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        v = A[j][j]
        for k in range(j):
            v = v - L[j][k] * L[j][k]
        if not v > floor:
            return rr.IDENTITY.copy(), None, j + 1
        L[j][j] = math.sqrt(v)
        for i in range(j + 1, 6):
            v = A[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        v = g[i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v / L[i][i]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * x[k]
        x[i] = v / L[i][i]
    w, qx, qy, qz = 1.0, 0.5 * x[0], 0.5 * x[1], 0.5 * x[2]
    ln = math.sqrt(((w * w + qx * qx) + qy * qy) + qz * qz)
    w, x_, y_, z_ = w / ln, qx / ln, qy / ln, qz / ln
    R = [[1.0 - 2.0 * (y_ * y_ + z_ * z_), 2.0 * (x_ * y_ - z_ * w), 2.0 * (x_ * z_ + y_ * w)],
         [2.0 * (x_ * y_ + z_ * w), 1.0 - 2.0 * (x_ * x_ + z_ * z_), 2.0 * (y_ * z_ - x_ * w)],
         [2.0 * (x_ * z_ - y_ * w), 2.0 * (y_ * z_ + x_ * w), 1.0 - 2.0 * (x_ * x_ + y_ * y_)]]
    D = np.zeros(12, np.float64)
    for k in range(3):
        D[4 * k:4 * k + 3] = R[k]
        D[4 * k + 3] = x[3 + k]
    return D, math.sqrt(s[27] * inv), 0


# ---- the loop ----
def register_surface(source, target, normals, radius, M0=None, max_iterations=32, tolerance=2.0 ** -40, scope_mask=None, target_mask=None):
    """(M float64[12], info): info = status, iterations, pairs, surface_pairs, rms, surface_rms, delta and step_pairs,
    step_surface_pairs, step_rms, step_surface_rms (lists, one entry per step); step_sums keeps (surface_pairs, sum29) of every step"""
    assert 1 <= max_iterations <= rr.MAX_STEPS and tolerance >= 0.0
    M = rr._matrix(M0).reshape(12).copy()
    info = {"status": MAX_ITERATIONS, "iterations": 0, "pairs": 0, "surface_pairs": 0, "rms": math.inf, "surface_rms": math.inf, "delta": math.inf,
            "step_pairs": [], "step_surface_pairs": [], "step_rms": [], "step_surface_rms": [], "step_sums": []}
    for t in range(max_iterations):
        idx, d2, _ = rr.match(source, target, radius, M, scope_mask, target_mask)
        pairs, surface_pairs, s29 = sums(source, target, normals, idx, d2, M)
        info["iterations"], info["pairs"], info["surface_pairs"] = t + 1, pairs, surface_pairs
        info["rms"], info["surface_rms"] = step_rms(pairs, s29[28]), step_rms(surface_pairs, s29[27])
        info["step_pairs"].append(pairs)
        info["step_surface_pairs"].append(surface_pairs)
        info["step_rms"].append(info["rms"])
        info["step_surface_rms"].append(info["surface_rms"])
        info["step_sums"].append((surface_pairs, s29))
        if surface_pairs < MIN_PAIRS:
            info["status"] = TOO_FEW
            break
        D, _, degenerate = surface_solve(surface_pairs, s29)
        if degenerate:
            info["status"] = DEGENERATE
            info["degenerate"] = degenerate
            break
        info["delta"] = rr.delta(D)
        M = rr.rigid_compose(D, M)
        if info["delta"] <= tolerance:
            info["status"] = CONVERGED
            break
    return M, info


# ---- the scenario of the registration tests: three unit faces of a box corner ----
RADIUS = 0.25
TARGET_PER_FACE, SOURCE_PER_FACE = 400, 300
# the stored rotation (r0, r1, r2, r3) whose third axis, the one of the shortest scale, is the face's normal EXACTLY: with
# Quaternion(r1, r2, r3, -r0) the third row of the rotation matrix is (1, 0, 0), (0, 1, 0), (0, 0, 1) in every bit
FACE_ROTATION = np.array([[0.5, 0.5, 0.5, 0.5], [-0.5, 0.5, 0.5, 0.5], [1.0, 0.0, 0.0, 0.0]], np.float32)
FACE_SCALES = np.array([0.05, 0.05, 0.001], np.float32)
_CORNER = None


def corner_motion():
    return rr.motion(0.06, (0.3, 0.9, 0.2), (0.04, -0.03, 0.05))


def _face(points2, face):
    """the n x 2 samples of [0, 1)^2 on face 0 (x = 0), 1 (y = 0) or 2 (z = 0)"""
    return np.insert(points2, face, 0.0, axis=1)


def corner_scenario():
    """dict: target f32[1200, 3], target_rotations f32[1200, 4], target_scales f32[1200, 3], target_face int[1200], and the same for
    the 900 source rows, which are OTHER samples of the same three faces moved by the inverse of corner_motion(); M_true float64[12].
    400 target and 300 source samples per face, face after face.  Computed once."""
    global _CORNER
    if _CORNER is None:
        rng = np.random.default_rng(11)
        tgt = np.concatenate([_face(rng.uniform(0.0, 1.0, (TARGET_PER_FACE, 2)), f) for f in range(3)]).astype(np.float32)
        other = np.concatenate([_face(rng.uniform(0.0, 1.0, (SOURCE_PER_FACE, 2)), f) for f in range(3)])
        R, t = corner_motion()
        src = ((other - t) @ R).astype(np.float32)                  # R^T (p - t), row by row
        tf, sf = np.repeat(np.arange(3), TARGET_PER_FACE), np.repeat(np.arange(3), SOURCE_PER_FACE)
        out = {"target": tgt, "target_face": tf, "target_rotations": FACE_ROTATION[tf].copy(), "target_scales": np.tile(FACE_SCALES, (tgt.shape[0], 1)),
               "source": src, "source_face": sf, "source_rotations": FACE_ROTATION[sf].copy(), "source_scales": np.tile(FACE_SCALES, (src.shape[0], 1)),
               "M_true": np.concatenate([R, t[:, None]], axis=1).reshape(12)}
        out["target_normals"] = nref.own_normals(tgt, out["target_rotations"], out["target_scales"])[0]
        assert np.array_equal(out["target_normals"], np.eye(3, dtype=np.float32)[tf])
        for a in out.values():
            a.setflags(write=False)
        _CORNER = out
    return _CORNER


def corner_faces(faces):
    """(target, rotations, scales, normals) of the corner's target restricted to the given faces"""
    c = corner_scenario()
    keep = np.isin(c["target_face"], faces)
    return c["target"][keep], c["target_rotations"][keep], c["target_scales"][keep], c["target_normals"][keep]


# ---- the input families of tests/test_gpu_surface.py ----
_FAMILIES = None


def families():
    """[(name, source, target, radius, M, rotations f32[m, 4], scales f32[m, 3], normals f32[m, 3])]: register_reference.families()
    with, per target, seeded rotations and scales whose own_normals are seeded unit f32 normals -- every seventh row a zero
    quaternion, which is no rotation: three NaNs -- and one family whose target has no normal at all.  Computed once."""
    global _FAMILIES
    if _FAMILIES is None:
        rng = np.random.default_rng(29)
        out = []
        for name, src, tgt, radius, M in rr.families():
            m = tgt.shape[0]
            rot = rng.normal(0.0, 1.0, (m, 4)).astype(np.float32)
            rot[::7] = 0.0
            scl = rng.uniform(0.01, 0.1, (m, 3)).astype(np.float32)
            out.append((name, src, tgt, radius, M, rot, scl))
        name, src, tgt, radius, M, rot, scl = out[4]                   # 255 x 300
        out.append(("no normal at all", src, tgt, radius, M, np.zeros_like(rot), scl))
        _FAMILIES = [f + (nref.own_normals(f[2], f[5], f[6])[0],) for f in out]
        assert np.isnan(_FAMILIES[-1][7]).all() and all(np.isnan(f[7][::7]).all() for f in _FAMILIES)
    return _FAMILIES
