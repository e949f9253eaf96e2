"""Normals, the specification in numpy f64 (include/gsplat_hip.h, "normals"): per splat in scope a unit normal, the surface
variation and the length of the list it came from -- by the PCA of the k nearest neighbours within `radius` (knn_reference.lists),
or from the splat's own shortest axis -- the info block and the closed-range picker.  +, -, *, / and sqrt of numpy f64 arrays are
the correctly rounded IEEE operations, applied element by element, so the array code below IS the header's sequence of operations
for every row at once; one() states the KNN source once more for a single neighbourhood as a scalar loop over
merge_reference.jacobi, and tests/test_normal_reference.py holds the two against each other bit for bit.  Positions arrive as the
harness reads them back (f32[3n]); scope masks are bool[n] (None: every splat).  Nothing here looks at the device code."""
import math

import numpy as np

import knn_reference as kr
import merge_reference as mr
import neighbour_reference as nr

SOURCES = {"knn": 0, "own": 1}
STATS = {"dot": 0, "abs_dot": 1, "variation": 2}
MIN_K, MAX_K = 2, kr.MAX_K
DEFAULT_BUDGET, MAX_BUDGET = kr.DEFAULT_BUDGET, kr.MAX_BUDGET
NAN32 = np.uint32(0x7fc00000)
NAN64 = np.uint64(0x7ff8000000000000)
ENTRIES = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def _positions(positions):
    return np.asarray(positions, dtype=np.float32).reshape(-1, 3).astype(np.float64)


def _scope(scope_mask, n):
    return np.ones(n, dtype=bool) if scope_mask is None else np.asarray(scope_mask, dtype=bool).reshape(n)


# ---- one neighbourhood, scalar: the header's steps 1 to 8 on python floats ----
def one(points):
    """(u[3] before the orientation, variation, tot, lam, V) of the points q_0 .. q_m (q_0 the splat itself), each three python floats"""
    M = float(len(points))
    mu = []
    for c in range(3):
        s = float(points[0][c])
        for q in points[1:]:
            s = s + float(q[c])
        mu.append(s / M)
    C = []
    for x, y in ENTRIES:
        s = 0.0
        for q in points:
            s = s + (float(q[x]) - mu[x]) * (float(q[y]) - mu[y])
        C.append(s / M)
    lam, V = mr.jacobi(C)
    l = [v if v > 0 else 0.0 for v in lam]
    tot = (l[0] + l[1]) + l[2]
    c = 0
    if l[1] < l[c]:
        c = 1
    if l[2] < l[c]:
        c = 2
    return [V[0][c], V[1][c], V[2][c]], (l[c] / tot if tot > 0 else float("nan")), tot, lam, V


def orient_one(u, p, toward=None):
    """the orientation of one normal (python floats)"""
    s = 0.0
    if toward is not None:
        s = (u[0] * (float(toward[0]) - p[0]) + u[1] * (float(toward[1]) - p[1])) + u[2] * (float(toward[2]) - p[2])
    if toward is not None and s < 0:
        flip = True
    elif toward is not None and s > 0:
        flip = False
    else:
        flip = u[0] < 0 if u[0] != 0 else u[1] < 0 if u[1] != 0 else u[2] < 0
    return [-v for v in u] if flip else list(u)


# ---- every row at once ----
def jacobi(C):
    """(lam float64[m, 3], V float64[m, 3, 3]) of m symmetric matrices given by their six entries (float64[m, 6]): merge_reference.jacobi
    on every row, the same operations in the same order"""
    C = np.asarray(C, dtype=np.float64).reshape(-1, 6)
    m = C.shape[0]
    A = np.empty((m, 3, 3), np.float64)
    for e, (x, y) in enumerate(ENTRIES):
        A[:, x, y] = C[:, e]
        A[:, y, x] = C[:, e]
    V = np.zeros((m, 3, 3), np.float64)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0
    with np.errstate(over="ignore"):
        for _ in range(6):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                w = np.nonzero(A[:, p, q] != 0.0)[0]
                if not w.size:
                    continue
                apq, app, aqq, arp, arq = A[w, p, q], A[w, p, p], A[w, q, q], A[w, r, p], A[w, r, q]
                th = (aqq - app) / (2.0 * apq)
                t = 1.0 / (np.abs(th) + np.sqrt(th * th + 1.0))
                t = np.where(th < 0, -t, t)
                cs = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * cs
                A[w, p, p] = app - t * apq
                A[w, q, q] = aqq + t * apq
                A[w, p, q] = A[w, q, p] = 0.0
                A[w, r, p] = A[w, p, r] = cs * arp - sn * arq
                A[w, r, q] = A[w, q, r] = sn * arp + cs * arq
                for k in range(3):
                    vkp, vkq = V[w, k, p], V[w, k, q]
                    V[w, k, p] = cs * vkp - sn * vkq
                    V[w, k, q] = sn * vkp + cs * vkq
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1), V


def _smallest(l):
    """(c* int[m], tot float64[m]) of the clamped eigenvalues l float64[m, 3]: the smallest c with l_c minimal"""
    tot = (l[:, 0] + l[:, 1]) + l[:, 2]
    c = np.zeros(l.shape[0], np.int64)
    rows = np.arange(l.shape[0])
    c[l[:, 1] < l[rows, c]] = 1
    c[l[:, 2] < l[rows, c]] = 2
    return c, tot


def _orient(u, p, toward):
    """the orientation of the rows u float64[m, 3] at the positions p"""
    with np.errstate(invalid="ignore", over="ignore"):
        first = np.where(u[:, 0] != 0, u[:, 0] < 0, np.where(u[:, 1] != 0, u[:, 1] < 0, u[:, 2] < 0))
        if toward is None:
            flip = first
        else:
            t = np.asarray(toward, dtype=np.float64).reshape(3)
            s = (u[:, 0] * (t[0] - p[:, 0]) + u[:, 1] * (t[1] - p[:, 1])) + u[:, 2] * (t[2] - p[:, 2])
            flip = np.where(s < 0, True, np.where(s > 0, False, first))
    return np.where(flip[:, None], -u, u)


def _store(n, rows, u, variation):
    """(normals float32[n, 3], variation float64[n]): the valid rows' values, quiet NaNs everywhere else"""
    normals = np.full((n, 3), NAN32, np.uint32).view(np.float32)
    var = np.full(n, NAN64, np.uint64).view(np.float64)
    normals[rows] = u.astype(np.float32)
    var[rows] = variation
    return normals, var


def knn_normals(positions, radius, k, scope_mask=None, toward=None, lists=None):
    """(normals float32[n, 3], variation float64[n], found uint32[n]) of the KNN source.  lists: (found, idx, d2) of
    knn_reference.lists for the same positions, radius, k and scope, when the caller holds them already."""
    p = _positions(positions)
    n = p.shape[0]
    found, idx, _ = kr.lists(positions, radius, k, scope_mask) if lists is None else lists
    found = np.asarray(found, dtype=np.uint32)
    idx = np.asarray(idx).reshape(n, -1)
    rows = np.nonzero(found >= 2)[0]
    f = found[rows].astype(np.int64)
    M = (f + 1).astype(np.float64)
    total = p[rows].copy()
    for t in range(k):
        live = f > t
        total[live] = total[live] + p[idx[rows[live], t]]
    mu = total / M[:, None]
    acc = np.zeros((rows.size, 6), np.float64)
    d = p[rows] - mu
    for e, (x, y) in enumerate(ENTRIES):
        acc[:, e] = acc[:, e] + d[:, x] * d[:, y]
    for t in range(k):
        live = f > t
        d = p[idx[rows[live], t]] - mu[live]
        for e, (x, y) in enumerate(ENTRIES):
            acc[live, e] = acc[live, e] + d[:, x] * d[:, y]
    lam, V = jacobi(acc / M[:, None])
    l = np.where(lam > 0, lam, 0.0)
    c, tot = _smallest(l)
    ok = tot > 0
    r = np.arange(rows.size)
    u = _orient(V[r, :, c], p[rows], toward)
    with np.errstate(invalid="ignore", divide="ignore"):
        variation = l[r, c] / tot
    normals, var = _store(n, rows[ok], u[ok], variation[ok])
    return normals, var, found.copy()


def own_normals(positions, rotations, scales, scope_mask=None, toward=None):
    """(normals float32[n, 3], variation float64[n], found uint32[n]) of the OWN source"""
    p = _positions(positions)
    n = p.shape[0]
    rot = np.asarray(rotations, dtype=np.float32).reshape(n, 4)
    scl = np.asarray(scales, dtype=np.float32).reshape(n, 3)
    s = _scope(scope_mask, n)
    fin = s & np.isfinite(p).all(axis=1) & np.isfinite(rot).all(axis=1) & np.isfinite(scl).all(axis=1)
    rows = np.nonzero(fin)[0]
    r64, s64 = rot[rows].astype(np.float64), scl[rows].astype(np.float64)
    qx, qy, qz, qw = r64[:, 1], r64[:, 2], r64[:, 3], -r64[:, 0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        b = (1 - 2 * qy * qy - 2 * qz * qz, 2 * qx * qy - 2 * qz * qw, 2 * qx * qz + 2 * qy * qw,
             2 * qx * qy + 2 * qz * qw, 1 - 2 * qx * qx - 2 * qz * qz, 2 * qy * qz - 2 * qx * qw,
             2 * qx * qz - 2 * qy * qw, 2 * qy * qz + 2 * qx * qw, 1 - 2 * qx * qx - 2 * qy * qy)
        b = np.stack(b, axis=1).reshape(-1, 3, 3)
        l = np.abs(s64) * np.abs(s64)
        c, tot = _smallest(l)
        i = np.arange(rows.size)
        a = b[i, c, :]
        nrm = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
        ok = (tot > 0) & (nrm > 0) & np.isfinite(nrm) & (rot[rows] != 0).any(axis=1)   # (a zero quaternion is no rotation)
        u = _orient(a / nrm[:, None], p[rows], toward)
        variation = l[i, c] / tot
    normals, var = _store(n, rows[ok], u[ok], variation[ok])
    return normals, var, np.zeros(n, np.uint32)


def info(positions, variation, scope_mask=None):
    """the exact fields of gsr_normal_info (pair_bound and budget are the index's)"""
    v = np.asarray(variation, dtype=np.float64)
    s = _scope(scope_mask, v.size)
    ok = v[~np.isnan(v)]
    return {"in_scope": int(s.sum()), "nonfinite": nr.nonfinite(positions, scope_mask), "valid": int(ok.size),
            "variation_min": float(ok.min()) if ok.size else float("inf"), "variation_max": float(ok.max()) if ok.size else float("-inf")}


def values(normals, variation, stat, axis=None):
    """float64[n]: the picker's value, from the STORED float32 normal widened to f64"""
    if stat == "variation":
        return np.asarray(variation, dtype=np.float64).copy()
    nm = np.asarray(normals, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    a = np.asarray(axis, dtype=np.float64).reshape(3)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (nm[:, 0] * a[0] + nm[:, 1] * a[1]) + nm[:, 2] * a[2]
    if stat == "abs_dot":
        return np.abs(v)
    if stat != "dot":
        raise ValueError(stat)
    return v


def select(normals, variation, stat, lo, hi, axis=None):
    """bool[n]: lo <= value <= hi, both ends closed; a NaN (a row without a normal) is never picked"""
    v = values(normals, variation, stat, axis)
    with np.errstate(invalid="ignore"):
        return (v >= lo) & (v <= hi)


# ---- shapes ----
def plane_lattice():
    """a 5 x 5 lattice of spacing 0.25 in the plane z = 0: (positions f32[25, 3], radius, k)"""
    g = np.arange(5, dtype=np.float64) * 0.25
    p = np.array([[x, y, 0.0] for y in g for x in g], dtype=np.float32)
    return p, 0.3, 8


def sphere(count=2048):
    """Fibonacci points on the unit sphere: (positions f32[count, 3], radius, k)"""
    i = np.arange(count, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / count
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    rho = np.sqrt(1.0 - z * z)
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1).astype(np.float32), 0.25, 12


_FAMILIES = None


def families():
    """[(name, positions f32[n, 3], radius, k)]: knn_reference.families() with k >= 2, the plane lattice and the sphere; built once and
    left unchanged"""
    global _FAMILIES
    if _FAMILIES is None:
        out = [f for f in kr.families() if f[3] >= MIN_K]
        clusters = [f for f in out if f[0] == "clusters and floaters, k 8"][0]
        out.append(("clusters and floaters, k 2", clusters[1], clusters[2], 2))
        for name, (p, radius, k) in (("plane lattice", plane_lattice()), ("sphere", sphere())):
            p.setflags(write=False)
            out.append(("%s, k %d" % (name, k), p, radius, k))
        _FAMILIES = out
    return _FAMILIES
