"""Matching and registration, the specification in numpy f64 (include/gsplat_hip.h, "matching and registration"): the transformed
point, the blocked O(n * m) match with its total order (d2, index), the rows and their fixed tree, Horn's closed form with an
8-sweep Jacobi, compose / decompose and the registration loop -- every operation in the header's written order, so that the device
and the host library are compared with it bit for bit.  Also what the implementation counts (pair_bound, through the index's
own key and bucket), the picker, the scenarios of the registration tests and families(), the shapes of tests/test_gpu_match.py.

Vector work is element-wise numpy (one rounding per operation, never a dot product or a sum); the solve is Python floats."""
import math

import numpy as np

import neighbour_reference as nr

NONE = 0xffffffff
DEFAULT_BUDGET = nr.DEFAULT_BUDGET
MAX_BUDGET = nr.MAX_BUDGET
CONVERGED, MAX_ITERATIONS, TOO_FEW = 0, 1, 2
MAX_STEPS = 256
GROUP = 256
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0], np.float64)


def _positions(positions):
    return np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)


def _scope(scope_mask, n):
    return np.ones(n, dtype=bool) if scope_mask is None else np.asarray(scope_mask, dtype=bool).reshape(n)


def _matrix(M):
    return (IDENTITY if M is None else np.ascontiguousarray(M, dtype=np.float64).reshape(12)).reshape(3, 4)


# ---- the transformed point ----
def transform(positions, M=None):
    """(T float64[n, 3], ok bool[n]): T_k = ((M[k][0]*x + M[k][1]*y) + M[k][2]*z) + M[k][3] on the stored floats as doubles; ok: the
    position and all three T_k are finite"""
    p = _positions(positions).astype(np.float64)
    m = _matrix(M)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.stack([((m[k, 0] * p[:, 0] + m[k, 1] * p[:, 1]) + m[k, 2] * p[:, 2]) + m[k, 3] for k in range(3)], axis=1)
    return t, np.isfinite(p).all(axis=1) & np.isfinite(t).all(axis=1)


# ---- the match ----
def match(source, target, radius, M=None, scope_mask=None, target_mask=None, block=512):
    """(idx uint32[n], d2 float64[n], info): for every source splat in scope the indexed target splat smallest in (d2, index) among
    those with d2 <= radius * radius; (NONE, +inf) without one, (NONE, NaN) outside the scope.  info: the integers of
    gsr_match_info and d2_min / d2_max; pair_bound is pair_bound()'s."""
    src, tgt = _positions(source), _positions(target)
    n, m = src.shape[0], tgt.shape[0]
    s, s2 = _scope(scope_mask, n), _scope(target_mask, m)
    t, ok = transform(src, M)
    indexed = s2 & np.isfinite(tgt).all(axis=1)
    q = tgt[indexed].astype(np.float64)
    qi = np.nonzero(indexed)[0]
    r2 = np.float64(radius) * np.float64(radius)
    idx = np.full(n, NONE, np.uint32)
    d2 = np.where(s, np.inf, np.nan).astype(np.float64)
    query = np.nonzero(s & ok)[0]
    if q.shape[0]:
        for a in range(0, query.size, block):
            i = query[a:a + block]
            ex = t[i, None, 0] - q[None, :, 0]
            ey = t[i, None, 1] - q[None, :, 1]
            ez = t[i, None, 2] - q[None, :, 2]
            with np.errstate(over="ignore", invalid="ignore"):
                d = (ex * ex + ey * ey) + ez * ez
            d = np.where(d <= r2, d, np.inf)
            j = np.argmin(d, axis=1)               # the first of the smallest: ties go to the smaller target index
            best = d[np.arange(i.size), j]
            has = np.isfinite(best)
            idx[i[has]] = qi[j[has]]
            d2[i[has]] = best[has]
    matched = idx != NONE
    info = {"in_scope": int(s.sum()), "nonfinite": int((s & ~ok).sum()), "target_indexed": int(indexed.sum()), "matched": int(matched.sum()),
            "pair_bound": pair_bound(src, tgt, radius, M, scope_mask, target_mask), "budget": DEFAULT_BUDGET,
            "d2_min": float(d2[matched].min()) if matched.any() else math.inf, "d2_max": float(d2[matched].max()) if matched.any() else -math.inf}
    return idx, d2, info


def select(d2, lo, hi, scope_mask=None):
    """the picker's set: in scope, lo <= v && (v < hi || hi == +inf) with v = sqrt(d2) (hi None: +inf)"""
    d2 = np.asarray(d2, np.float64)
    hi = np.inf if hi is None else hi
    with np.errstate(invalid="ignore"):
        v = np.sqrt(d2)
        return _scope(scope_mask, d2.size) & (lo <= v) & ((v < hi) | (hi == np.inf))


# ---- what the implementation counts: the queries' walk over the hashed index ----
def _bucket(k, mask):
    k = k.astype(np.uint64)
    with np.errstate(over="ignore"):
        k = k ^ (k >> np.uint64(33)); k = k * np.uint64(0xff51afd7ed558ccd)
        k = k ^ (k >> np.uint64(33)); k = k * np.uint64(0xc4ceb9fe1a85ec53)
        k = k ^ (k >> np.uint64(33))
    return (k & np.uint64(0xffffffff)) & np.uint64(mask)


def pair_bound(source, target, radius, M=None, scope_mask=None, target_mask=None):
    """The sum over the queries of the populations of the 27 buckets their walk visits: cells outside the clamp are skipped, a
    bucket two cells share is counted twice.  The buckets are the smallest power of two >= max(256, 2 * target count)."""
    src, tgt = _positions(source), _positions(target)
    n, m = src.shape[0], tgt.shape[0]
    s, s2 = _scope(scope_mask, n), _scope(target_mask, m)
    buckets = 256
    while buckets < 2 * m:
        buckets *= 2
    c, ok = nr.cells(tgt, radius)
    pop = np.bincount(_bucket(nr._key(c[s2 & ok]), buckets - 1).astype(np.int64), minlength=buckets) if m else np.zeros(buckets, np.int64)
    t, tok = transform(src, M)
    inv_h = np.float64(1.0) / (np.float64(radius) * nr.SLACK)
    tq = t[s & tok]
    if not tq.shape[0]:
        return 0
    with np.errstate(over="ignore"):
        qc = np.clip(np.floor(tq * inv_h), -nr.CELL_HALF, nr.CELL_HALF - 1).astype(np.int64)
    total = 0
    for z in (-1, 0, 1):
        for y in (-1, 0, 1):
            for x in (-1, 0, 1):
                around = qc + np.array([x, y, z], dtype=np.int64)
                inside = ((around >= -nr.CELL_HALF) & (around < nr.CELL_HALF)).all(axis=1)
                around = np.clip(around, -nr.CELL_HALF, nr.CELL_HALF - 1)
                total += int((pop[_bucket(nr._key(around), buckets - 1).astype(np.int64)] * inside).sum())
    return total


# ---- the sums ----
def rows(source, target, idx, d2, M=None):
    """float64[n, 16]: (T, Q, T_a * Q_b for ab = 00, 01, .., 22, d2) for a matched splat, sixteen +0.0 for every other"""
    src, tgt = _positions(source), _positions(target)
    t, _ = transform(src, M)
    out = np.zeros((src.shape[0], 16), np.float64)
    i = np.nonzero(np.asarray(idx) != NONE)[0]
    q = tgt[np.asarray(idx)[i]].astype(np.float64)
    out[i, 0:3] = t[i]
    out[i, 3:6] = q
    for a in range(3):
        for b in range(3):
            out[i, 6 + 3 * a + b] = t[i, a] * q[:, b]
    out[i, 15] = np.asarray(d2)[i]
    return out


def tree(x):
    """float64[16]: the rows summed by the fixed tree -- groups of 256 consecutive rows, the last padded with +0.0; within a group
    for s = 128, 64, .., 1: x[l] = x[l] + x[l + s] for l < s; the group results the same way until one row is left"""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 16)
    if not x.shape[0]:
        return np.zeros(16, np.float64)
    while True:
        g = (x.shape[0] + GROUP - 1) // GROUP
        y = np.zeros((g * GROUP, 16), np.float64)
        y[:x.shape[0]] = x
        y = y.reshape(g, GROUP, 16)
        s = GROUP // 2
        while s:
            y[:, :s] = y[:, :s] + y[:, s:2 * s]
            s //= 2
        x = y[:, 0].copy()
        if g == 1:
            return x[0]


def sums(source, target, idx, d2, M=None):
    """(pairs, float64[16])"""
    return int((np.asarray(idx) != NONE).sum()), tree(rows(source, target, idx, d2, M))


def step_rms(pairs, sum16):
    return math.sqrt(float(sum16[15]) * (1.0 / float(pairs))) if pairs else math.inf


# ---- the rigid solve: Horn's closed form, Python floats in the header's order ----
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
SWEEPS = 8


def rigid_solve(pairs, sum16):
    """(D float64[12], rms); ValueError for what gsr_rigid_solve refuses"""
    s = [float(v) for v in np.asarray(sum16, np.float64).reshape(16)]
    if pairs < 3 or not all(math.isfinite(v) for v in s):
        raise ValueError("pairs < 3 or a non-finite sum")
    inv = 1.0 / float(pairs)
    mT = [s[a] * inv for a in range(3)]
    mQ = [s[3 + a] * inv for a in range(3)]
    S = [[s[6 + 3 * a + b] * inv - mT[a] * mQ[b] for b in range(3)] for a in range(3)]
    A = [[0.0] * 4 for _ in range(4)]
    A[0][0] = (S[0][0] + S[1][1]) + S[2][2]
    A[0][1] = S[1][2] - S[2][1]
    A[0][2] = S[2][0] - S[0][2]
    A[0][3] = S[0][1] - S[1][0]
    A[1][1] = (S[0][0] - S[1][1]) - S[2][2]
    A[1][2] = S[0][1] + S[1][0]
    A[1][3] = S[2][0] + S[0][2]
    A[2][2] = (S[1][1] - S[0][0]) - S[2][2]
    A[2][3] = S[1][2] + S[2][1]
    A[3][3] = (S[2][2] - S[0][0]) - S[1][1]
    for p in range(4):
        for q in range(p):
            A[p][q] = A[q][p]
    V = [[1.0 if p == q else 0.0 for q in range(4)] for p in range(4)]
    for _ in range(SWEEPS):
        for p, q in PAIRS:
            apq = A[p][q]
            if apq == 0.0:
                continue
            app, aqq = A[p][p], A[q][q]
            th = (aqq - app) / (2.0 * apq)
            t = 1.0 / (math.fabs(th) + math.sqrt(th * th + 1.0))
            if th < 0.0:
                t = -t
            cs = 1.0 / math.sqrt(t * t + 1.0)
            sn = t * cs
            A[p][p] = app - t * apq
            A[q][q] = aqq + t * apq
            A[p][q] = A[q][p] = 0.0
            for r in range(4):
                if r == p or r == q:
                    continue
                arp, arq = A[r][p], A[r][q]
                A[r][p] = A[p][r] = cs * arp - sn * arq
                A[r][q] = A[q][r] = sn * arp + cs * arq
            for k in range(4):
                vkp, vkq = V[k][p], V[k][q]
                V[k][p] = cs * vkp - sn * vkq
                V[k][q] = sn * vkp + cs * vkq
    best = 0
    for k in range(1, 4):
        if A[k][k] > A[best][best]:
            best = k
    w, x, y, z = V[0][best], V[1][best], V[2][best], V[3][best]
    ln = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / ln, x / ln, y / ln, z / ln
    first = w if w != 0.0 else x if x != 0.0 else y if y != 0.0 else z
    if first < 0.0:
        w, x, y, z = -w, -x, -y, -z
    R = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
         [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
         [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]]
    D = np.zeros(12, np.float64)
    for k in range(3):
        D[4 * k:4 * k + 3] = R[k]
        D[4 * k + 3] = mQ[k] - ((R[k][0] * mT[0] + R[k][1] * mT[1]) + R[k][2] * mT[2])
    return D, math.sqrt(s[15] * inv)


def rigid_compose(D, M):
    """D o M: apply M, then D"""
    D = [float(v) for v in np.asarray(D, np.float64).reshape(12)]
    M = [float(v) for v in np.asarray(M, np.float64).reshape(12)]
    out = np.zeros(12, np.float64)
    for k in range(3):
        for c in range(4):
            v = (D[4 * k] * M[c] + D[4 * k + 1] * M[4 + c]) + D[4 * k + 2] * M[8 + c]
            if c == 3:
                v = v + D[4 * k + 3]
            out[4 * k + c] = v
    return out


def rigid_decompose(M):
    """(q_xyzw float64[4], t float64[3]): Shepperd's four branches in the header's order"""
    M = [float(v) for v in np.asarray(M, np.float64).reshape(12)]
    R00, R01, R02, R10, R11, R12, R20, R21, R22 = M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10]
    tr = (R00 + R11) + R22
    if tr > 0.0:
        s = math.sqrt(tr + 1.0) * 2.0
        w, x, y, z = 0.25 * s, (R21 - R12) / s, (R02 - R20) / s, (R10 - R01) / s
    elif R00 > R11 and R00 > R22:
        s = math.sqrt(((1.0 + R00) - R11) - R22) * 2.0
        w, x, y, z = (R21 - R12) / s, 0.25 * s, (R01 + R10) / s, (R02 + R20) / s
    elif R11 > R22:
        s = math.sqrt(((1.0 + R11) - R00) - R22) * 2.0
        w, x, y, z = (R02 - R20) / s, (R01 + R10) / s, 0.25 * s, (R12 + R21) / s
    else:
        s = math.sqrt(((1.0 + R22) - R00) - R11) * 2.0
        w, x, y, z = (R10 - R01) / s, (R02 + R20) / s, (R12 + R21) / s, 0.25 * s
    return np.array([x, y, z, w], np.float64), np.array([M[3], M[7], M[11]], np.float64)


def delta(D):
    return float(np.abs(np.asarray(D, np.float64).reshape(12) - IDENTITY).max())


# ---- the loop ----
def register(source, target, radius, M0=None, max_iterations=32, tolerance=2.0 ** -40, scope_mask=None, target_mask=None):
    """(M float64[12], info): info = status, iterations, pairs, rms, delta, step_pairs, step_rms (lists, one entry per step)"""
    assert 1 <= max_iterations <= MAX_STEPS and tolerance >= 0.0
    M = _matrix(M0).reshape(12).copy()
    info = {"status": MAX_ITERATIONS, "iterations": 0, "pairs": 0, "rms": math.inf, "delta": math.inf, "step_pairs": [], "step_rms": []}
    for t in range(max_iterations):
        idx, d2, _ = match(source, target, radius, M, scope_mask, target_mask)
        pairs, s16 = sums(source, target, idx, d2, M)
        info["iterations"], info["pairs"], info["rms"] = t + 1, pairs, step_rms(pairs, s16)
        info["step_pairs"].append(pairs)
        info["step_rms"].append(info["rms"])
        if pairs < 3:
            info["status"] = TOO_FEW
            break
        D, _ = rigid_solve(pairs, s16)
        info["delta"] = delta(D)
        M = rigid_compose(D, M)
        if info["delta"] <= tolerance:
            info["status"] = CONVERGED
            break
    return M, info


# ---- the scenarios of the registration tests ----
def motion(angle=0.12, axis=(0.3, 0.9, 0.2), t=(0.05, -0.03, 0.04)):
    """(R float64[3, 3], t float64[3]) of a rotation by `angle` about `axis` and a translation"""
    a = np.asarray(axis, np.float64)
    a = a / np.sqrt((a * a).sum())
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K), np.asarray(t, np.float64)


RADIUS = 0.25
PARTNERS, FAR = 900, 60
_SCENARIOS = {}


def scenario(floaters=False, seed=7):
    """(source f32[n, 3], target f32[1500, 3], partner int64[900]): the target is 1500 seeded normal points scaled by (1, 0.3, 0.6);
    source rows 0 .. 899 are the targets partner[i] moved by the INVERSE of motion() and stored as f32; 60 more source rows lie
    50 units away, where nothing matches; floaters: 60 further rows scattered inside the cloud, with no partner.  Computed once."""
    key = (bool(floaters), seed)
    if key not in _SCENARIOS:
        rng = np.random.default_rng(seed)
        tgt = (rng.normal(0.0, 1.0, (1500, 3)) * np.array([1.0, 0.3, 0.6])).astype(np.float32)
        partner = rng.permutation(1500)[:PARTNERS]
        R, t = motion()
        src = (tgt[partner].astype(np.float64) - t) @ R          # R^T (q - t), row by row
        far = rng.normal(0.0, 1.0, (FAR, 3)) + np.array([50.0, 0.0, 0.0])
        parts = [src, far]
        if floaters:
            parts.append(rng.uniform(-1.0, 1.0, (60, 3)) * np.array([1.0, 0.3, 0.6]))
        src = np.concatenate(parts).astype(np.float32)
        d = tgt.astype(np.float64)
        gap = np.sqrt(((d[:, None, :] - d[None, :, :]) ** 2).sum(axis=2) + np.eye(1500) * 1e9).min()
        assert gap > 2.0 ** -16, gap                              # the target's smallest spacing: a match within 2^-17 is THE partner
        assert np.abs(tgt).max() < 4.0 and np.abs(src[:PARTNERS]).max() < 4.0
        for a in (src, tgt, partner):
            a.setflags(write=False)
        _SCENARIOS[key] = (src, tgt, partner)
    return _SCENARIOS[key]


# ---- the input families of tests/test_gpu_match.py ----
def families():
    """[(name, source f32[n, 3], target f32[m, 3], radius, M float64[12] or None)]: the smallest shapes that can still go wrong"""
    rng = np.random.default_rng(23)
    R, t = motion(0.05, (0.2, -0.5, 0.8), (0.02, 0.01, -0.03))
    small = np.concatenate([R, t[:, None]], axis=1).reshape(12)
    out = [("1 x 1", np.array([[0.1, 0.2, 0.3]], np.float32), np.array([[0.1, 0.2, 0.35]], np.float32), 0.1, None)]
    tgt300 = rng.normal(0.0, 0.5, (300, 3)).astype(np.float32)
    for n in (63, 64, 65, 255, 256, 257):              # wave, workgroup and tree-group edges
        out.append(("%d x 300" % n, rng.normal(0.0, 0.5, (n, 3)).astype(np.float32), tgt300, 0.3, small))
    tgt512 = rng.normal(0.0, 1.0, (512, 3)).astype(np.float32)
    for n in (65536, 65537):                           # the tree's third level and its padding; every fifth source out of reach
        src = tgt512[np.arange(n) % 512].astype(np.float64) + rng.normal(0.0, 0.01, (n, 3))
        src[::5] += 100.0
        out.append(("%d x 512" % n, src.astype(np.float32), tgt512, 0.0625, small))
    a, b = [1.5, -0.25, 0.75], [-0.5, 0.5, 0.25]
    out.append(("coincident targets", np.array([a, b, [1.5, -0.25, 0.76], [0.0, 0.0, 0.0]], np.float32), np.array([b, a, b, a, a, b], np.float32), 0.05, None))
    lat = nr.lattice(0.25, side=6)                     # exact multiples of the radius, through negative coordinates
    shifted = np.concatenate([lat + np.float32([0.25, 0.0, 0.0]), lat + np.float32([0.0, 0.125, 0.0]), lat + np.float32([0.0, 0.0, -0.5])])
    out.append(("lattice, radius = spacing", shifted, lat, 0.25, None))
    # queries exactly on cell faces: the cell side is h = 0.25 * (1 + 2^-10); the stored source is k * h - 1 and M adds the 1 back
    h = 0.25 * (1.0 + 2.0 ** -10)
    k = np.arange(-4, 5, dtype=np.float64)
    faces = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) * h
    assert np.array_equal((faces - 1.0).astype(np.float32).astype(np.float64) + 1.0, faces)
    plus_one = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0])
    out.append(("queries on cell faces", (faces - 1.0).astype(np.float32), (faces + rng.uniform(-0.2, 0.2, faces.shape)).astype(np.float32), 0.25, plus_one))
    far = nr.lattice(0.25, side=5, origin=(2.0 ** 19, -(2.0 ** 19), 2.0 ** 19))
    out.append(("2^19 radii out", np.concatenate([far + np.float32([0.25, 0.0, 0.0]), far + np.float32([0.0, 0.5, 0.0]), far[:7]]), far, 0.25, None))
    beyond = nr.lattice(0.25, side=4, origin=(2.0 ** 21, 0.0, -(2.0 ** 22)))
    out.append(("beyond the clamp", np.concatenate([beyond + np.float32([0.0, 0.25, 0.0]), beyond + np.float32([0.5, 0.0, 0.0]), beyond[:5]]), beyond, 0.25, None))
    out.append(("non-finite rows", nr.with_nonfinite(rng.normal(0.0, 0.5, (200, 3))), nr.with_nonfinite(rng.normal(0.0, 0.5, (150, 3))[::-1]), 0.3, small))
    big = rng.normal(0.0, 0.5, (130, 3)).astype(np.float32)
    big[::4, 0] = np.float32(3e38) * np.sign(big[::4, 0])           # M[0][0] * x overflows for these rows: no query
    big[1::4, 0] = 0.0                                              # and stays small for these
    out.append(("M overflows for some rows", big, rng.normal(0.0, 0.5, (120, 3)).astype(np.float32), 0.3,
                np.array([1e300, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0])))
    return out
