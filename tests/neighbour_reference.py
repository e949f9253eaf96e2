"""Neighbours, the specification in numpy f64 (include/gsplat_hip.h, "neighbours"): for every splat in scope the number of OTHER
splats in scope within `radius` of it, capped; the histogram of those counts; the range picker; and two statements about the
index an implementation may build -- the counts once more through the cell construction (grid_counts), and the least any
implementation's pair_bound can be (pair_floor).  Positions arrive as the harness reads them back (f32[3n]); scope masks are
bool[n] (None: every splat).  Nothing here looks at the device code."""
import numpy as np

MAX_CAP = 4095
DEFAULT_BUDGET = 1 << 34
MAX_BUDGET = 1 << 38
CELL_HALF = 1 << 20          # cell coordinates are clamped to [-2^20, 2^20): 21 bits per axis
SLACK = 1.0 + 2.0 ** -10     # cell side = radius * SLACK: strictly larger than the radius


def _positions(positions):
    return np.asarray(positions, dtype=np.float32).reshape(-1, 3).astype(np.float64)


def _scope(scope_mask, n):
    return np.ones(n, dtype=bool) if scope_mask is None else np.asarray(scope_mask, dtype=bool).reshape(n)


def counts(positions, radius, cap, scope_mask=None, block=512):
    """uint32[n]: count_i = min(cap, #{ j in S : i != j and (dx*dx + dy*dy) + dz*dz <= radius*radius }) for i in S, 0 outside S.
    Blocked O(n^2), f64, in the written order; a NaN or infinite component makes every comparison false."""
    p = _positions(positions)
    n = p.shape[0]
    s = _scope(scope_mask, n)
    r2 = np.float64(radius) * np.float64(radius)
    idx = np.nonzero(s)[0]
    q = p[idx]
    out = np.zeros(n, dtype=np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, idx.size, block):
            me = q[a:a + block]
            dx = me[:, None, 0] - q[None, :, 0]
            dy = me[:, None, 1] - q[None, :, 1]
            dz = me[:, None, 2] - q[None, :, 2]
            near = ((dx * dx + dy * dy) + dz * dz) <= r2
            k = np.arange(me.shape[0])
            near[k, a + k] = False                       # a splat does not count itself
            out[idx[a:a + block]] = np.minimum(near.sum(axis=1), cap)
    return out


def hist(counts_, cap, scope_mask=None):
    """uint32[cap + 1]: hist[k] = the splats in S with count == k (the counts are capped: hist[cap] is "cap or more")"""
    c = np.asarray(counts_, dtype=np.uint32)
    s = _scope(scope_mask, c.size)
    return np.bincount(c[s], minlength=cap + 1).astype(np.uint32)


def select(counts_, lo, hi, scope_mask=None):
    """bool[n]: in S and lo <= count < hi"""
    c = np.asarray(counts_, dtype=np.uint32)
    return _scope(scope_mask, c.size) & (c >= lo) & (c < hi)


def nonfinite(positions, scope_mask=None):
    """the splats in S with a NaN or infinite position component"""
    p = _positions(positions)
    return int((~np.isfinite(p).all(axis=1) & _scope(scope_mask, p.shape[0])).sum())


def cells(positions, radius, side=None, trunc=False):
    """(int64[n, 3], bool[n]): the cell of every splat -- floor((double)x * inv_h) with inv_h = 1 / (radius * SLACK) computed once,
    clamped to [-CELL_HALF, CELL_HALF) -- and which splats have one (all components finite).  side / trunc: the constructions
    that do NOT work (tests/test_neighbour_reference.py): another cell side, truncation in place of floor."""
    p = _positions(positions)
    ok = np.isfinite(p).all(axis=1)
    inv_h = np.float64(1.0) / (np.float64(radius) * SLACK if side is None else np.float64(side))
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.where(ok[:, None], p, 0.0) * inv_h
        t = np.trunc(t) if trunc else np.floor(t)
    return np.clip(t, -CELL_HALF, CELL_HALF - 1).astype(np.int64), ok


def _key(c):
    c = c + CELL_HALF
    return c[..., 0] | (c[..., 1] << 21) | (c[..., 2] << 42)


def grid_counts(positions, radius, cap, scope_mask=None, side=None, trunc=False):
    """counts() once more, through the cells: a splat is compared only with the splats in the 27 cells around its own.  Equal to
    counts() because the construction is complete; with side=radius and trunc=True it is not."""
    p = _positions(positions)
    n = p.shape[0]
    s = _scope(scope_mask, n)
    c, ok = cells(positions, radius, side, trunc)
    live = np.nonzero(s & ok)[0]
    out = np.zeros(n, dtype=np.uint32)
    if not live.size:
        return out
    r2 = np.float64(radius) * np.float64(radius)
    keys = _key(c[live])
    order = np.argsort(keys, kind="stable")
    skeys, sidx = keys[order], live[order]
    ukeys, first, pop = np.unique(skeys, return_index=True, return_counts=True)
    members = {int(k): sidx[f:f + m] for k, f, m in zip(ukeys, first, pop)}
    offsets = np.array([(x, y, z) for z in (-1, 0, 1) for y in (-1, 0, 1) for x in (-1, 0, 1)], dtype=np.int64)
    for k, f in zip(ukeys, first):
        mine = members[int(k)]
        around = c[sidx[f]] + offsets
        around = around[((around >= -CELL_HALF) & (around < CELL_HALF)).all(axis=1)]
        others = [members[int(a)] for a in _key(around) if int(a) in members]
        js = np.concatenate(others)
        dx = p[mine, None, 0] - p[None, js, 0]
        dy = p[mine, None, 1] - p[None, js, 1]
        dz = p[mine, None, 2] - p[None, js, 2]
        near = (((dx * dx + dy * dy) + dz * dz) <= r2) & (mine[:, None] != js[None, :])
        out[mine] = np.minimum(near.sum(axis=1), cap)
    return out


def pair_floor(positions, radius, scope_mask=None):
    """For every indexed splat (in S, finite) the population of the 27 exact cells around its own, summed: what a walk that never
    met a hash collision would test.  Every implementation's pair_bound is at least this."""
    p = _positions(positions)
    s = _scope(scope_mask, p.shape[0])
    c, ok = cells(positions, radius)
    live = c[s & ok]
    if not live.shape[0]:
        return 0
    ukeys, inverse, pop = np.unique(_key(live), return_inverse=True, return_counts=True)
    population = dict(zip(ukeys.tolist(), pop.tolist()))
    ucells = np.zeros((ukeys.size, 3), dtype=np.int64)
    ucells[inverse] = live
    total = 0
    for z in (-1, 0, 1):
        for y in (-1, 0, 1):
            for x in (-1, 0, 1):
                around = ucells + np.array([x, y, z], dtype=np.int64)
                inside = ((around >= -CELL_HALF) & (around < CELL_HALF)).all(axis=1)
                there = np.array([population.get(int(a), 0) for a in _key(around)], dtype=np.int64)
                total += int((there * pop * inside).sum())
    return total


# ---- the input families of the GPU tests (tests/test_gpu_neighbours.py) and of the CPU comparison of grid_counts with counts ----
def lattice(radius, side=12, origin=(0.0, 0.0, 0.0)):
    """side^3 splats at exact multiples of `radius` (a power of two keeps every product exact), centred on `origin` given in radii:
    through negative coordinates, and with origin 2^19 far out where a cell coordinate needs 20 bits"""
    k = np.arange(side, dtype=np.float64) - side // 2
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) + np.asarray(origin, dtype=np.float64)
    return (g * radius).astype(np.float32)


def clusters(n=8192, floaters=200, seed=5):
    """three gaussian clusters and `floaters` splats scattered over a box fifty times as wide, shuffled"""
    rng = np.random.default_rng(seed)
    centres = np.array([[0.0, 0.0, 0.0], [2.5, -1.0, 0.5], [-1.5, 2.0, -2.0]])
    body = n - floaters
    which = rng.integers(0, 3, body)
    p = centres[which] + rng.normal(0.0, 0.25, (body, 3))
    f = rng.uniform(-25.0, 25.0, (floaters, 3))
    out = np.concatenate([p, f]).astype(np.float32)
    return out[rng.permutation(n)]


def with_nonfinite(positions):
    """a copy with NaN, +inf, -inf and 3e38 planted in single components of eight rows"""
    p = np.array(positions, dtype=np.float32).reshape(-1, 3)
    n = p.shape[0]
    for k, v in enumerate((np.nan, np.inf, -np.inf, 3e38, -3e38, np.nan, np.inf, 3e38)):
        p[(5 * k + 1) % n, k % 3] = v
    return p


def families():
    """[(name, positions f32[n, 3], radius, cap)]: the shapes both test files run -- the smallest that can still go wrong"""
    rng = np.random.default_rng(11)
    r = 0.375
    beyond = np.nextafter(np.float32(r), np.float32(1.0))
    out = [("n = 1", np.array([[0.25, -1.0, 3.0]], np.float32), r, 8),
           ("n = 2 at exactly radius", np.array([[0.5, 1.0, -2.0], [0.5 + r, 1.0, -2.0]], np.float32), r, 8),
           ("n = 2 one ulp beyond", np.array([[0.0, 1.0, -2.0], [beyond, 1.0, -2.0]], np.float32), r, 8)]
    for n in (63, 64, 65, 257):                        # wave and workgroup edges
        out.append(("n = %d" % n, rng.normal(0.0, 0.5, (n, 3)).astype(np.float32), 0.3, 16))
    same = np.tile(np.array([[1.5, -0.25, 0.75]], np.float32), (300, 1))
    out.append(("300 coincident, cap 7", same, 0.01, 7))              # the early exit
    out.append(("300 coincident, cap 4095", same, 0.01, MAX_CAP))     # the saturated last bin stays empty: 299 each
    out.append(("lattice", lattice(0.25), 0.25, 32))                  # exact multiples of radius, through negative coordinates
    out.append(("lattice 2^19 radii out", lattice(0.25, origin=(2.0 ** 19, -(2.0 ** 19), 2.0 ** 19)), 0.25, 32))
    out.append(("lattice beyond the clamp", lattice(0.25, side=6, origin=(2.0 ** 21, 0.0, -(2.0 ** 22))), 0.25, 32))
    out.append(("non-finite rows", with_nonfinite(rng.normal(0.0, 0.5, (200, 3))), 0.3, 16))
    out.append(("clusters and floaters", clusters(), 0.15, 64))
    return out
