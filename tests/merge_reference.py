"""The specification of merging cells (include/gsplat_hip.h, "merging cells") in Python f64: scalar loops per cell, math.sqrt, every
sum over the members in ascending index order.  A Python float is an IEEE f64 and +, -, *, / and math.sqrt are correctly rounded, so
the steps below ARE the header's.  The packed covariance words are not restated: they come from the oracle, by
SceneState.scale((1, 1, 1)) on the merged rows, which re-packs the covariance and changes nothing else.

families() are the shapes the GPU tests run.  One of them asserts that its cells collide in the hashed grid, so nb_bucket and the
bucket rule of gsr_neighbours.cpp (256 buckets, doubled while below 2 n) are restated here too."""
import math

import numpy as np

from oracle import oracle as O

NONE = 0xffffffff                        # GSR_CELL_NONE
MAX_CAP = 4095                           # GSR_NEIGHBOUR_MAX_CAP
DEFAULT_BUDGET, MAX_BUDGET = 1 << 34, 1 << 38
CELL_HALF = 1 << 20
M64 = (1 << 64) - 1


# ---- cells ----
def cell_coords(pos, cell):
    """int64[n, 3]: floor((double)x * inv) clamped to [-2^20, 2^20), inv = 1.0 / cell (finite positions only)"""
    inv = 1.0 / float(cell)
    t = np.floor(np.asarray(pos, dtype=np.float32).reshape(-1, 3).astype(np.float64) * inv)
    return np.clip(t, -float(CELL_HALF), float(CELL_HALF - 1)).astype(np.int64)


def cell_key(c):
    return (int(c[0]) + CELL_HALF) | (int(c[1]) + CELL_HALF) << 21 | (int(c[2]) + CELL_HALF) << 42


def nb_bucket(k, mask):
    k ^= k >> 33; k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33; k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k & 0xffffffff & mask


def buckets_of(n):
    b = 256
    while b < 2 * n:
        b <<= 1
    return b


def candidates(pos, rot, scl, mask=None):
    """bool[n]: in scope, and all ten floats finite"""
    pos, rot, scl = (np.asarray(a, dtype=np.float32).reshape(-1, k) for a, k in ((pos, 3), (rot, 4), (scl, 3)))
    ok = np.isfinite(pos).all(axis=1) & np.isfinite(rot).all(axis=1) & np.isfinite(scl).all(axis=1)
    return ok if mask is None else ok & np.asarray(mask, dtype=bool)


def cells_of(pos, rot, scl, cell, mask=None):
    """(cand bool[n], leader uint32[n], members: {leader: ascending member list})"""
    cand = candidates(pos, rot, scl, mask)
    n = cand.size
    leader = np.full(n, NONE, np.uint32)
    members = {}
    idx = np.flatnonzero(cand)
    if idx.size:
        cc = cell_coords(np.asarray(pos, dtype=np.float32).reshape(-1, 3)[idx], cell)
        first = {}
        for i, c in zip(idx.tolist(), map(tuple, cc.tolist())):
            l = first.setdefault(c, i)
            leader[i] = l
            members.setdefault(l, []).append(i)
    return cand, leader, members


def report(pos, rot, scl, cell, cap, mask=None, budget=DEFAULT_BUDGET):
    """(leader, hist uint32[cap + 1], info without pair_bound) of gsr_cells"""
    cand, leader, members = cells_of(pos, rot, scl, cell, mask)
    n = cand.size
    sizes = np.array([len(v) for v in members.values()], dtype=np.int64)
    hist = np.bincount(np.minimum(sizes, cap), minlength=cap + 1).astype(np.uint32) if sizes.size else np.zeros(cap + 1, np.uint32)
    merged = sizes[sizes >= 2]
    info = {"in_scope": int(n if mask is None else np.asarray(mask, dtype=bool).sum()), "candidates": int(cand.sum()), "cells": int(sizes.size),
            "merged_cells": int(merged.size), "merged_members": int(merged.sum()), "largest": int(sizes.max()) if sizes.size else 0,
            "rows_after": int(n - merged.sum() + merged.size), "budget": int(budget)}
    return leader, hist, info


def pair_floor(pos, rot, scl, cell, mask=None):
    """what pair_bound is at least: the sum of m over the candidates"""
    return sum(len(v) ** 2 for v in cells_of(pos, rot, scl, cell, mask)[2].values())


# ---- the merged row ----
def splat_cov(rot, scl):
    """the six sums s0..s5 of the packed covariance, before the `4 *` and the halves: rot = (r0, r1, r2, r3) and scl as stored, in
    the order of operations the covariance words are computed in (Scene.ts:150-176), zero terms included"""
    qx, qy, qz, qw = float(rot[1]), float(rot[2]), float(rot[3]), -float(rot[0])
    b = (1 - 2 * qy * qy - 2 * qz * qz, 2 * qx * qy - 2 * qz * qw, 2 * qx * qz + 2 * qy * qw,
         2 * qx * qy + 2 * qz * qw, 1 - 2 * qx * qx - 2 * qz * qz, 2 * qy * qz - 2 * qx * qw,
         2 * qx * qz - 2 * qy * qw, 2 * qy * qz + 2 * qx * qw, 1 - 2 * qx * qx - 2 * qy * qy)
    a = (float(scl[0]), 0.0, 0.0, 0.0, float(scl[1]), 0.0, 0.0, 0.0, float(scl[2]))
    M = (b[0] * a[0] + b[3] * a[1] + b[6] * a[2], b[1] * a[0] + b[4] * a[1] + b[7] * a[2], b[2] * a[0] + b[5] * a[1] + b[8] * a[2],
         b[0] * a[3] + b[3] * a[4] + b[6] * a[5], b[1] * a[3] + b[4] * a[4] + b[7] * a[5], b[2] * a[3] + b[5] * a[4] + b[8] * a[5],
         b[0] * a[6] + b[3] * a[7] + b[6] * a[8], b[1] * a[6] + b[4] * a[7] + b[7] * a[8], b[2] * a[6] + b[5] * a[7] + b[8] * a[8])
    return (M[0] * M[0] + M[3] * M[3] + M[6] * M[6], M[0] * M[1] + M[3] * M[4] + M[6] * M[7], M[0] * M[2] + M[3] * M[5] + M[6] * M[8],
            M[1] * M[1] + M[4] * M[4] + M[7] * M[7], M[1] * M[2] + M[4] * M[5] + M[7] * M[8], M[2] * M[2] + M[5] * M[5] + M[8] * M[8])


def jacobi(C):
    """steps 6: (lam[3], V[3][3]) of the symmetric matrix given by its six entries 00, 01, 02, 11, 12, 22"""
    A = [[C[0], C[1], C[2]], [C[1], C[3], C[4]], [C[2], C[4], C[5]]]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(6):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            r = 3 - p - q
            apq = A[p][q]
            if apq == 0.0:
                continue
            app, aqq, arp, arq = A[p][p], A[q][q], A[r][p], A[r][q]
            th = (aqq - app) / (2.0 * apq)
            t = 1.0 / (abs(th) + math.sqrt(th * th + 1.0))
            if th < 0:
                t = -t
            cs = 1.0 / math.sqrt(t * t + 1.0)
            sn = t * cs
            A[p][p] = app - t * apq
            A[q][q] = aqq + t * apq
            A[p][q] = A[q][p] = 0.0
            A[r][p] = A[p][r] = cs * arp - sn * arq
            A[r][q] = A[q][r] = sn * arp + cs * arq
            for k in range(3):
                vkp, vkq = V[k][p], V[k][q]
                V[k][p] = cs * vkp - sn * vkq
                V[k][q] = sn * vkp + cs * vkq
    return [A[0][0], A[1][1], A[2][2]], V


def quaternion(V):
    """steps 8 and 9: (x, y, z, w) of R = V^T by Shepperd's four branches"""
    R = [[V[j][k] for j in range(3)] for k in range(3)]
    tr = (R[0][0] + R[1][1]) + R[2][2]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2.0
        return (R[2][1] - R[1][2]) / s, (R[0][2] - R[2][0]) / s, (R[1][0] - R[0][1]) / s, 0.25 * s
    if R[0][0] > R[1][1] and R[0][0] > R[2][2]:
        s = math.sqrt(((1.0 + R[0][0]) - R[1][1]) - R[2][2]) * 2.0
        return 0.25 * s, (R[0][1] + R[1][0]) / s, (R[0][2] + R[2][0]) / s, (R[2][1] - R[1][2]) / s
    if R[1][1] > R[2][2]:
        s = math.sqrt(((1.0 + R[1][1]) - R[0][0]) - R[2][2]) * 2.0
        return (R[0][1] + R[1][0]) / s, 0.25 * s, (R[1][2] + R[2][1]) / s, (R[0][2] - R[2][0]) / s
    s = math.sqrt(((1.0 + R[2][2]) - R[0][0]) - R[1][1]) * 2.0
    return (R[0][2] + R[2][0]) / s, (R[1][2] + R[2][1]) / s, 0.25 * s, (R[1][0] - R[0][1]) / s


def merged_row(pos, rot, scl, rgba, idx):
    """steps 1 to 12 but the covariance words, for the members idx (ascending) of one cell:
    (position f32[3], rotation f32[4], scale f32[3], rgba word, C: the mixture's six entries)"""
    m = len(idx)
    a = [float(int(rgba[i]) >> 24) for i in idx]
    mass = [a[t] * ((abs(float(scl[i][0])) * abs(float(scl[i][1]))) * abs(float(scl[i][2]))) for t, i in enumerate(idx)]
    M = 0.0
    for v in mass:
        M += v
    w, W = (mass, M) if M > 0 else ([1.0] * m, float(m))
    mu = []
    for k in range(3):
        s = 0.0
        for t, i in enumerate(idx):
            s += w[t] * float(pos[i][k])
        mu.append(s / W)
    C = [0.0] * 6
    for t, i in enumerate(idx):
        S = splat_cov(rot[i], scl[i])
        d = [float(pos[i][k]) - mu[k] for k in range(3)]
        for e, (x, y) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            C[e] += w[t] * (S[e] + d[x] * d[y])
    C = [v / W for v in C]
    lam, V = jacobi(C)
    new_scl = np.array([math.sqrt(v if v > 0 else 0.0) for v in lam], dtype=np.float64).astype(np.float32)
    x, y, z, qw = quaternion(V)
    new_rot = np.array([-qw, x, y, z], dtype=np.float64).astype(np.float32)
    word = 0
    for k in range(3):
        s = 0.0
        for t, i in enumerate(idx):
            s += w[t] * float((int(rgba[i]) >> (8 * k)) & 0xff)
        word |= int(math.floor(s / W + 0.5)) << (8 * k)
    vol = (float(new_scl[0]) * float(new_scl[1])) * float(new_scl[2])
    if vol > 0:
        o = M / vol
        alpha = 255 if o >= 255 else int(math.floor(o + 0.5))
    else:
        alpha = int(max(a))
    return np.array(mu, dtype=np.float64).astype(np.float32), new_rot, new_scl, word | alpha << 24, C


def repack(data, pos, rot, scl):
    """the rows with their covariance words packed afresh from rot and scl by the oracle (Scene.scale by one), nothing else changed"""
    st = O.SceneState(np.zeros(0, dtype=np.uint8))
    st.n = int(np.asarray(pos).reshape(-1, 3).shape[0])
    st.data = np.ascontiguousarray(data, dtype=np.uint32).reshape(-1).copy()
    st.positions = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1).copy()
    st.rotations = np.ascontiguousarray(rot, dtype=np.float32).reshape(-1).copy()
    st.scales = np.ascontiguousarray(scl, dtype=np.float32).reshape(-1).copy()
    if st.n:
        st.scale((1.0, 1.0, 1.0))
    assert np.array_equal(st.positions.view(np.uint32), np.ascontiguousarray(pos, dtype=np.float32).reshape(-1).view(np.uint32))
    assert np.array_equal(st.scales.view(np.uint32), np.ascontiguousarray(scl, dtype=np.float32).reshape(-1).view(np.uint32))
    return st.data.reshape(-1, 8)


def merge(data, pos, rot, scl, cell, mask=None, hidden=None):
    """gsr_scene_merge_cells: a dict of the scene that is left -- data uint32[k, 8], positions f32[k, 3], rotations f32[k, 4], scales
    f32[k, 3] -- with `merged` bool[k] (the merged rows: the selection afterwards), `hidden` bool[k] (the carried set), `keep`
    bool[n], `info` (report's) and `C` {new row: the mixture's covariance}.  The inputs are left unchanged."""
    data = np.array(data, dtype=np.uint32).reshape(-1, 8)
    pos = np.array(pos, dtype=np.float32).reshape(-1, 3)
    rot = np.array(rot, dtype=np.float32).reshape(-1, 4)
    scl = np.array(scl, dtype=np.float32).reshape(-1, 3)
    n = pos.shape[0]
    _, _, info = report(pos, rot, scl, cell, 1, mask)
    _, _, members = cells_of(pos, rot, scl, cell, mask)
    keep = np.ones(n, bool)
    merged = np.zeros(n, bool)
    rgba = data[:, 7].copy()
    C = {}
    rows = []
    for l, idx in members.items():
        if len(idx) >= 2:
            rows.append((l, idx, merged_row(pos, rot, scl, rgba, idx)))
    for l, idx, (p, r, s, word, c) in rows:
        pos[l], rot[l], scl[l] = p, r, s
        data[l, 0:3] = p.view(np.uint32)
        data[l, 7] = word
        keep[idx[1:]] = False
        merged[l] = True
        C[l] = c
    lead = np.flatnonzero(merged)
    if lead.size:
        data[lead, 4:7] = repack(data[lead], pos[lead], rot[lead], scl[lead])[:, 4:7]
    new_index = np.cumsum(keep) - 1
    hid = np.zeros(n, bool) if hidden is None else np.asarray(hidden, dtype=bool)
    return {"data": data[keep], "positions": pos[keep], "rotations": rot[keep], "scales": scl[keep], "merged": merged[keep], "hidden": hid[keep],
            "keep": keep, "info": info, "C": {int(new_index[l]): c for l, c in C.items()}}


def cov_of_row(rot, scl):
    """the six sums of a stored row as a symmetric 3 x 3 float64 matrix"""
    s = splat_cov(rot, scl)
    return np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])


def sym(C):
    return np.array([[C[0], C[1], C[2]], [C[1], C[3], C[4]], [C[2], C[4], C[5]]])


# ---- scenes ----
def scene(p, seed=1, scale=(0.01, 0.1)):
    """(data uint32[n, 8], positions f32[n, 3], rotations f32[n, 4], scales f32[n, 3]) around the positions p: random unit rotations,
    scales and colours, data word 3 zero, the covariance words the oracle's"""
    p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    rng = np.random.default_rng(seed)
    rot = rng.normal(0, 1, (n, 4))
    rot = (rot / np.linalg.norm(rot, axis=1, keepdims=True)).astype(np.float32)
    scl = rng.uniform(scale[0], scale[1], (n, 3)).astype(np.float32)
    data = np.zeros((n, 8), np.uint32)
    data[:, 0:3] = p.view(np.uint32)
    data[:, 7] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32) | np.uint32(0x01000000)
    return repack(data, p, rot, scl).copy(), p.copy(), rot, scl


def _ulp_below(v):
    return np.nextafter(np.float32(v), np.float32(-np.inf))


_FAMILIES = None


def families():
    """[(name, (data, positions, rotations, scales), cell)], built once and left unchanged"""
    global _FAMILIES
    if _FAMILIES is not None:
        return _FAMILIES
    rng = np.random.default_rng(20)
    out = []
    out.append(("one splat", scene([[0.1, 0.2, 0.3]]), 0.5))
    out.append(("two splats in one cell", scene([[0.1, 0.2, 0.3], [0.3, 0.1, 0.2]]), 0.5))
    out.append(("two splats in two cells", scene([[0.1, 0.2, 0.3], [0.6, 0.1, 0.2]]), 0.5))
    for k in (63, 64, 65, 255, 256, 257):
        # one cell of k members between two rows of their own cells
        p = np.vstack([[[-5.0, 0.0, 0.0]], rng.uniform(0.0, 1.0, (k, 3)), [[7.0, 0.5, 0.5]]])
        out.append(("%d members in one cell" % k, scene(p, seed=k), 1.0))
    # floor, not truncation, and the two zeros: coordinates exactly on k / 4 and one ulp below, k in -3 .. 3, and -0.0
    axis = [np.float32(k * 0.25) for k in range(-3, 4)] + [_ulp_below(k * 0.25) for k in range(-3, 4)] + [np.float32(-0.0)]
    grid = np.array([[x, y, z] for x in axis for y in axis for z in axis], dtype=np.float32)
    out.append(("lattice on the cell edges", scene(grid[rng.permutation(grid.shape[0])], seed=3, scale=(0.001, 0.01)), 0.25))
    # beyond the clamp: 2^20 cells of 2^-10 end at 1024; everything at or beyond shares the boundary cell
    far = np.array([[1500.0, 0.1, 0.1], [3.0e9, 0.1, 0.1], [1024.0, 0.1, 0.1], [1023.9995, 0.1, 0.1], [-1024.0, 0.1, 0.1], [-2000.0, 0.1, 0.1],
                    [-1023.9995, 0.1, 0.1], [0.1, 5000.0, -7000.0], [0.1, 1.0e8, -1.0e7], [0.1, 0.1, 0.1], [0.1, 0.1, 0.1003]], dtype=np.float32)
    out.append(("rows beyond the clamp", scene(far, seed=4), 2.0 ** -10))
    # 400 cells of two members each: 800 splats in 2048 buckets, so some cells share a bucket
    c = rng.permutation(20 ** 3)[:400]
    corner = np.stack([c % 20, (c // 20) % 20, c // 400], axis=1).astype(np.float64)
    p = np.repeat(corner, 2, axis=0) + rng.uniform(0.05, 0.95, (800, 3))
    out.append(("400 cells of two", scene(p[rng.permutation(800)], seed=5), 1.0))
    # non-finite rows beside mergeable ones
    d, p, r, s = scene(rng.uniform(0.0, 1.0, (12, 3)), seed=6)
    p[2, 1] = np.nan; p[5, 0] = np.inf; s[7, 2] = np.inf; s[8, 0] = np.nan; r[9, 3] = np.nan; r[10, 0] = -np.inf
    d[:, 0:3] = p.view(np.uint32)
    out.append(("non-finite rows", (d, p, r, s), 2.0))
    # a cell of opacity 0: the weights are 1
    d, p, r, s = scene(rng.uniform(0.0, 1.0, (5, 3)), seed=7)
    d[:, 7] &= np.uint32(0x00ffffff)
    out.append(("a cell of opacity 0", (d, p, r, s), 1.0))
    # coincident zero-scale splats: C = 0, no volume
    d, p, r, s = scene(np.tile([[0.25, 0.5, 0.75]], (6, 1)), seed=8)
    s[:] = 0.0
    s[3] = -0.0
    out.append(("coincident zero-scale splats", (repack(d, p, r, s).copy(), p, r, s), 1.0))
    # collinear members (rank one between the centres), and coincident ones
    t = np.linspace(0.1, 0.9, 9)[:, None]
    out.append(("collinear members", scene(np.hstack([t, 0.5 * t, 0.25 + 0.0 * t]), seed=9, scale=(1e-4, 2e-4)), 1.0))
    out.append(("coincident members", scene(np.tile([[0.3, 0.6, 0.1]], (7, 1)), seed=10), 1.0))
    # 8192 clustered splats at about four members per cell
    centres = rng.uniform(-1.0, 1.0, (64, 3))
    p = centres[rng.integers(0, 64, 8192)] + rng.normal(0, 0.05, (8192, 3))
    out.append(("8192 clustered", scene(p, seed=11), 0.08))
    for _, arrays, _ in out:
        for a in arrays:
            a.setflags(write=False)
    _FAMILIES = out
    return out
