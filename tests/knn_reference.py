"""k nearest neighbours, the specification in numpy f64 (include/gsplat_hip.h, "k nearest neighbours"): for every splat in scope
the k nearest OTHER splats in scope within `radius`, ascending by the pair (d2, index); how many were found; the value per splat
(distance to the k-th, or mean distance to those found); the histogram of the lists' lengths; the info block; the range picker;
and the threshold of statistical outlier removal.  Positions arrive as the harness reads them back (f32[3n]); scope masks are
bool[n] (None: every splat).  Nothing here looks at the device code."""
import numpy as np

import neighbour_reference as nr

MAX_K = 32
NONE = 0xffffffff
STATS = {"kth": 0, "mean": 1}
DEFAULT_BUDGET = nr.DEFAULT_BUDGET
MAX_BUDGET = nr.MAX_BUDGET


def _positions(positions):
    return np.asarray(positions, dtype=np.float32).reshape(-1, 3).astype(np.float64)


def _scope(scope_mask, n):
    return np.ones(n, dtype=bool) if scope_mask is None else np.asarray(scope_mask, dtype=bool).reshape(n)


def lists(positions, radius, k, scope_mask=None, block=256):
    """(found uint32[n], idx uint32[n, k], d2 float64[n, k]): blocked O(n^2), f64, d2 = (dx*dx + dy*dy) + dz*dz in the written
    order, near iff d2 <= radius*radius and another splat in S; the near ones ordered by np.lexsort on (j, d2) -- d2 first, equal
    distances to the smaller index -- and cut at k; empty slots hold NONE and +inf.  A NaN or infinite component makes every
    comparison false: such a splat finds nobody and is found by nobody.  Rows outside S: found 0 and empty slots."""
    p = _positions(positions)
    n = p.shape[0]
    s = _scope(scope_mask, n)
    r2 = np.float64(radius) * np.float64(radius)
    members = np.nonzero(s)[0]
    q = p[members]
    found = np.zeros(n, dtype=np.uint32)
    idx = np.full((n, k), NONE, dtype=np.uint32)
    d2 = np.full((n, k), np.inf, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, members.size, block):
            me = q[a:a + block]
            dx = me[:, None, 0] - q[None, :, 0]
            dy = me[:, None, 1] - q[None, :, 1]
            dz = me[:, None, 2] - q[None, :, 2]
            d = (dx * dx + dy * dy) + dz * dz
            near = d <= r2
            rows = np.arange(me.shape[0])
            near[rows, a + rows] = False                 # a splat is not its own neighbour
            for b in rows:
                js = members[near[b]]
                ds = d[b][near[b]]
                order = np.lexsort((js, ds))[:k]         # the last key is the primary one: (d2, j)
                i = members[a + b]
                found[i] = order.size
                idx[i, :order.size] = js[order]
                d2[i, :order.size] = ds[order]
    return found, idx, d2


def values(found, d2, k, stat, scope_mask=None):
    """float64[n].  "kth": found == k ? sqrt(d2[k-1]) : +inf.  "mean": found == 0 ? +inf : (((sqrt(d2[0]) + sqrt(d2[1])) + ..) /
    found -- a sequential sum column by column, s = s + sqrt(col_t) on the rows with t < found, which pins the association.  NaN
    outside S."""
    found = np.asarray(found, dtype=np.uint32)
    d2 = np.asarray(d2, dtype=np.float64).reshape(found.size, k)
    s = _scope(scope_mask, found.size)
    out = np.full(found.size, np.inf, dtype=np.float64)
    if stat == "kth":
        full = found == k
        out[full] = np.sqrt(d2[full, k - 1])
    elif stat == "mean":
        total = np.zeros(found.size, dtype=np.float64)
        for t in range(k):
            live = found > t
            total[live] = total[live] + np.sqrt(d2[live, t])
        some = found > 0
        out[some] = total[some] / found[some].astype(np.float64)
    else:
        raise ValueError(stat)
    out[~s] = np.nan
    return out


def hist(found, k, scope_mask=None):
    """uint32[k + 1]: hist[t] = the splats in S with found == t"""
    f = np.asarray(found, dtype=np.uint32)
    return np.bincount(f[_scope(scope_mask, f.size)], minlength=k + 1).astype(np.uint32)


def info(positions, found, values_, k, scope_mask=None):
    """the exact fields of gsr_knn_info (pair_bound and budget are the index's: neighbour_reference.pair_floor bounds the first)"""
    f = np.asarray(found, dtype=np.uint32)
    s = _scope(scope_mask, f.size)
    v = np.asarray(values_, dtype=np.float64)[s]
    fin = v[np.isfinite(v)]
    return {"in_scope": int(s.sum()), "nonfinite": nr.nonfinite(positions, scope_mask), "complete": int((f[s] == k).sum()), "finite_values": int(fin.size),
            "value_min": float(fin.min()) if fin.size else float("inf"), "value_max": float(fin.max()) if fin.size else float("-inf")}


def select(values_, lo, hi, scope_mask=None):
    """bool[n]: in S and lo <= value and (value < hi or hi == +inf); a NaN is never picked"""
    v = np.asarray(values_, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return _scope(scope_mask, v.size) & (v >= lo) & ((v < hi) | (hi == np.inf))


def outlier_threshold(values_, std_ratio, scope_mask=None):
    """mu + std_ratio * sigma over the finite values in S, sigma the sample standard deviation (n - 1); +inf with fewer than two"""
    v = np.asarray(values_, dtype=np.float64)
    v = v[_scope(scope_mask, v.size)]
    v = v[np.isfinite(v)]
    if v.size < 2:
        return float("inf")
    return float(np.mean(v) + np.float64(std_ratio) * np.std(v, ddof=1))


def brute(positions, radius, k, scope_mask=None):
    """lists() once more as a double loop over python floats, for at most a few dozen splats"""
    p = _positions(positions)
    n = p.shape[0]
    s = _scope(scope_mask, n)
    r2 = float(np.float64(radius) * np.float64(radius))
    found = np.zeros(n, dtype=np.uint32)
    idx = np.full((n, k), NONE, dtype=np.uint32)
    d2 = np.full((n, k), np.inf, dtype=np.float64)
    for i in range(n):
        if not s[i]:
            continue
        pairs = []
        for j in range(n):
            if j == i or not s[j]:
                continue
            dx, dy, dz = float(p[i, 0]) - float(p[j, 0]), float(p[i, 1]) - float(p[j, 1]), float(p[i, 2]) - float(p[j, 2])
            d = (dx * dx + dy * dy) + dz * dz
            if d <= r2:
                pairs.append((d, j))
        pairs.sort()
        pairs = pairs[:k]
        found[i] = len(pairs)
        for t, (d, j) in enumerate(pairs):
            idx[i, t], d2[i, t] = j, d
    return found, idx, d2


# ---- the input families of the GPU tests (tests/test_gpu_knn.py): neighbour_reference.families()' positions, k chosen per family ----
_KS = {"n = 1": (3,), "n = 2 at exactly radius": (3,), "n = 2 one ulp beyond": (3,),
       "n = 63": (1, 8), "n = 64": (1, 8), "n = 65": (1, 8), "n = 257": (1, 8),
       "300 coincident, cap 7": (7, 32),                 # every distance 0: the tie rule, and the full list that rejects a larger index
       "lattice": (6, 32), "lattice 2^19 radii out": (6, 32), "lattice beyond the clamp": (6, 32),   # exact ties at radius
       "non-finite rows": (4,),
       "clusters and floaters": (1, 8, 32)}              # floaters with found < k: padding and +inf values


def families():
    """[(name, positions f32[n, 3], radius, k)]"""
    out = []
    for name, p, radius, _ in nr.families():
        if name not in _KS:
            continue
        base = "300 coincident" if name.startswith("300 coincident") else name
        for k in _KS[name]:
            out.append(("%s, k %d" % (base, k), p, radius, k))
    return out
