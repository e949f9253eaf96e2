"""The specification of "Planes" (include/gsplat_hip.h, "planes") in numpy f64 with Python integers for the
generator: candidates, hypotheses, scores, the best hypothesis, the picker and the alignment.  Every expression is written in
the header's order; numpy multiplies, adds, divides and takes square roots one correctly rounded operation at a time, so the
device's results are compared with these bit for bit.  families() holds the smallest shapes that can go wrong."""
import numpy as np

MASK64 = (1 << 64) - 1
MAX_HYPOTHESES = 4096
CHUNK = 512                      # PLANE_CHUNK (gsplat.js_amd/csrc/gsr_internal.h): candidates a score workgroup stages at a time
MAX_CHUNK_GROUPS = 2048          # PLANE_MAX_CHUNK_GROUPS: beyond CHUNK * this many candidates a workgroup walks a second chunk
DEFAULT_BUDGET, MAX_BUDGET = 1 << 34, 1 << 38


def mix(z):
    """the splitmix64 finaliser on uint64, wrapping"""
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def mulhi64(a, b):
    return (a * b) >> 64


def rank(seed, h, j, m):
    return mulhi64(mix((seed + 3 * h + j) & MASK64), m)


def _xyz(p):
    return np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)


def candidates(p, mask=None):
    """(cand, in_scope, nonfinite): the splats in scope (mask bool[n]; None: every splat) with three finite floats, ascending"""
    p = _xyz(p)
    scope = np.ones(p.shape[0], bool) if mask is None else np.asarray(mask, bool)
    fin = np.isfinite(p).all(axis=1)
    cand = np.nonzero(scope & fin)[0].astype(np.uint32)
    return cand, int(scope.sum()), int(scope.sum()) - int(cand.size)


def hypotheses(p, cand, count, seed):
    """(planes f64[count, 4], triples uint32[count, 3], degenerate bool[count]); a degenerate hypothesis's plane is zeros"""
    p = _xyz(p).astype(np.float64)
    m = int(cand.size)
    planes = np.zeros((count, 4), np.float64)
    if m == 0:
        return planes, np.zeros((count, 3), np.uint32), np.ones(count, bool)
    r = np.array([[rank(seed, h, j, m) for j in range(3)] for h in range(count)], dtype=np.int64).reshape(count, 3)
    tri = cand[r]
    A, B, C = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = B - A, C - A
        Nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        Ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        Nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        l2 = (Nx * Nx + Ny * Ny) + Nz * Nz
        deg = (r[:, 0] == r[:, 1]) | (r[:, 0] == r[:, 2]) | (r[:, 1] == r[:, 2]) | ~np.isfinite(l2) | (l2 == 0)
        ln = np.sqrt(l2)
        nx, ny, nz = Nx / ln, Ny / ln, Nz / ln
        neg = (nx < 0) | ((nx == 0) & ((ny < 0) | ((ny == 0) & (nz < 0))))
        nx, ny, nz = np.where(neg, -nx, nx), np.where(neg, -ny, ny), np.where(neg, -nz, nz)
        d = -((nx * A[:, 0] + ny * A[:, 1]) + nz * A[:, 2])
    ok = ~deg
    planes[ok] = np.stack([nx, ny, nz, d], axis=1)[ok]
    return planes, tri.astype(np.uint32), deg


def distance(p, plane):
    """s = ((a*(double)x + b*(double)y) + c*(double)z) + d of every row of p"""
    p = _xyz(p).astype(np.float64)
    a, b, c, d = (np.float64(v) for v in plane)
    with np.errstate(all="ignore"):
        return ((a * p[:, 0] + b * p[:, 1]) + c * p[:, 2]) + d


def scores(p, cand, planes, threshold, degenerate=None):
    """uint32[K]: the candidates within threshold of each plane, used as given; a degenerate hypothesis scores 0"""
    q = _xyz(p).astype(np.float64)[cand]
    planes = np.asarray(planes, np.float64).reshape(-1, 4)
    out = np.zeros(planes.shape[0], np.uint32)
    if not cand.size:
        return out
    x, y, z = q[:, 0][None, :], q[:, 1][None, :], q[:, 2][None, :]
    step = max(1, (1 << 22) // int(cand.size))
    with np.errstate(all="ignore"):
        for h0 in range(0, planes.shape[0], step):
            pl = planes[h0:h0 + step]
            s = ((pl[:, 0:1] * x + pl[:, 1:2] * y) + pl[:, 2:3] * z) + pl[:, 3:4]
            out[h0:h0 + step] = (np.abs(s) <= np.float64(threshold)).sum(axis=1)
    if degenerate is not None:
        out[degenerate] = 0
    return out


def fit(p, threshold, count, seed=0, mask=None):
    """(info, scores): gsr_fit_plane's info as the Python host's dict (plane: float64[4]) and all `count` scores"""
    cand, in_scope, nonfinite = candidates(p, mask)
    info = {"in_scope": in_scope, "nonfinite": nonfinite, "hypotheses": 0, "degenerate": 0, "found": 0, "best": 0, "triple": (0, 0, 0), "inliers": 0,
            "tests": count * int(cand.size), "budget": DEFAULT_BUDGET, "plane": np.zeros(4, np.float64)}
    if not in_scope:                                                   # an empty scene or an empty scope: zeros
        return info, np.zeros(count, np.uint32)
    planes, tri, deg = hypotheses(p, cand, count, seed)
    sc = scores(p, cand, planes, threshold, deg)
    info["hypotheses"], info["degenerate"] = count, int(deg.sum())
    if not deg.all():
        key = [(int(sc[h]) << 32) | ((~h) & 0xffffffff) for h in range(count) if not deg[h]]
        best = (~max(key)) & 0xffffffff
        info.update(found=1, best=best, triple=tuple(int(v) for v in tri[best]), inliers=int(sc[best]), plane=planes[best].copy())
    return info, sc


def select(p, plane, lo, hi):
    """bool[n]: lo <= s && s <= hi over all splats; a NaN distance is never picked"""
    s = distance(p, plane)
    with np.errstate(all="ignore"):
        return (np.float64(lo) <= s) & (s <= np.float64(hi))


def _unit(v):
    v = np.asarray(v, np.float64)
    ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return v[:3] / ln, ln


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.float64)


def alignment(plane, axis=(0, 1, 0)):
    """(q_xyzw, t) of gsr_plane_alignment"""
    plane = np.asarray(plane, np.float64)
    n, ln = _unit(plane[:3])
    a, _ = _unit(axis)
    d = plane[3] / ln
    c = (n[0] * a[0] + n[1] * a[1]) + n[2] * a[2]
    if c > -1.0 + 2.0 ** -20:
        v, w = _cross(n, a), 1.0 + c
    else:
        k = 0
        if abs(n[1]) < abs(n[k]):
            k = 1
        if abs(n[2]) < abs(n[k]):
            k = 2
        e = np.zeros(3, np.float64)
        e[k] = 1.0
        v, w = _cross(n, e), np.float64(0.0)
    ln = np.sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + w * w)
    return np.array([v[0] / ln, v[1] / ln, v[2] / ln, w / ln], np.float64), d * a


def quat_matrix(q):
    """the 3x3 matrix of (x, y, z, w), as Scene.rotate builds it"""
    x, y, z, w = (np.float64(v) for v in q)
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w],
                     [2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w],
                     [2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y]], np.float64)


# ---- the shapes ----
FLOOR_N, FLOOR_THRESHOLD, FLOOR_HYPOTHESES = 8192, 0.01, 256


def floor_scene():
    """(p float32[8192, 3], n_true, floor bool[8192]): in [-4, 4]^3 a tilted floor with 60 % of the splats and sigma 0.004, a
    smaller wall, and uniform clutter"""
    rng = np.random.default_rng(20)
    n = FLOOR_N
    nf, nw = (n * 6) // 10, n // 5
    n_true = np.array([0.12, 0.98, -0.16], np.float64)
    n_true /= np.linalg.norm(n_true)
    u = np.cross(n_true, [1.0, 0.0, 0.0]); u /= np.linalg.norm(u)
    v = np.cross(n_true, u)
    centre = np.array([0.2, -1.1, 0.3])
    ab = rng.uniform(-2.4, 2.4, (nf, 2))
    floor = centre + ab[:, :1] * u + ab[:, 1:] * v + rng.normal(0.0, 0.004, (nf, 1)) * n_true
    wn = np.cross(n_true, [0.0, 0.0, 1.0]); wn /= np.linalg.norm(wn)     # a wall, at right angles to the floor
    wu = np.cross(wn, n_true)
    cd = np.stack([rng.uniform(-2.0, 2.0, nw), rng.uniform(0.0, 2.0, nw)], axis=1)
    wall = centre + 2.0 * wn + cd[:, :1] * wu + cd[:, 1:] * n_true + rng.normal(0.0, 0.004, (nw, 1)) * wn
    clutter = rng.uniform(-4.0, 4.0, (n - nf - nw, 3))
    p = np.clip(np.concatenate([floor, wall, clutter]), -4.0, 4.0).astype(np.float32)
    is_floor = np.arange(n) < nf
    order = rng.permutation(n)
    return p[order], n_true, is_floor[order]


def _cloud(rng, n):
    """n splats: two thirds on the plane z = 0.25 x - 0.5 y + 0.125 with a little noise, the rest anywhere in [-2, 2]^3"""
    xy = rng.uniform(-2.0, 2.0, (n, 2))
    z = 0.25 * xy[:, 0] - 0.5 * xy[:, 1] + 0.125 + rng.normal(0.0, 0.003, n)
    p = np.concatenate([xy, z[:, None]], axis=1)
    off = np.arange(n) % 3 == 2
    p[off] = rng.uniform(-2.0, 2.0, (int(off.sum()), 3))
    return p.astype(np.float32)


def _lattice(zs, side=8, step=0.25):
    g = (np.arange(side) - side // 2) * step
    x, y, z = np.meshgrid(g, g, np.asarray(zs, np.float32).astype(np.float64), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float32)


def families():
    """[(name, positions float32[n, 3], threshold, hypotheses, seed)]"""
    rng = np.random.default_rng(7)
    out = []
    add = lambda name, p, t=0.01, h=64, seed=0: out.append((name, np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3), float(t), int(h), int(seed)))
    add("n = 1", [[0.5, -0.25, 2.0]], h=8)
    add("n = 2", [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], h=8)
    add("n = 3", [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5]], t=0.0, h=65, seed=3)
    add("all coincident", np.tile(np.array([[0.5, 0.5, 0.5]], np.float32), (70, 1)), h=63)
    line = np.arange(100, dtype=np.float64)[:, None] * np.array([[0.25, -0.5, 0.125]])
    add("all colinear", line, h=64)
    for m in (63, 64, 65, 255, 256, 257):
        add("n = %d" % m, _cloud(rng, m), h=64, seed=m)
    for m in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        add("n = %d (chunk)" % m, _cloud(rng, m), h=65, seed=m)
    for h in (1, 63, 64, 65, 256, 257, 4096):
        add("H = %d" % h, _cloud(rng, 300), h=h, seed=1000 + h)
    add("two parallel lattice planes", _lattice([0.0, 1.0]), t=0.125, h=64, seed=5)
    t = np.float32(0.25)
    beyond = np.nextafter(t, np.float32(1.0))
    add("lattice at exactly +-threshold and one ulp beyond", _lattice([0.0, t, -t, beyond, -beyond], side=4), t=0.25, h=256, seed=9)
    add("coordinates near 1e30", _cloud(rng, 200).astype(np.float64) * 1e30, t=1e28, h=64, seed=11)
    add("coordinates near 1e-30", _cloud(rng, 200).astype(np.float64) * 1e-30, t=1e-32, h=64, seed=12)
    bad = _cloud(rng, 301)
    bad[5, 0] = np.nan; bad[64, 1] = np.inf; bad[65, 2] = -np.inf; bad[130] = np.nan; bad[300, 0] = np.inf
    add("non-finite rows", bad, h=64, seed=13)
    add("a second chunk per workgroup", _cloud(rng, CHUNK * MAX_CHUNK_GROUPS + CHUNK + 1), h=8, seed=14)
    add("floor, wall and clutter", floor_scene()[0], t=FLOOR_THRESHOLD, h=FLOOR_HYPOTHESES, seed=0)
    return out
