"""Clusters, the specification in numpy f64 (include/gsplat_hip.h, "clusters"): the connected islands of the splats in scope at a
linking radius -- every splat's label and cluster size, the call's info, the size-range picker and the picker of one splat's
cluster.  near(i, j) is neighbour_reference.counts' expression, blocked O(n^2); the closure is a host union-find.  Positions
arrive as the harness reads them back (f32[3n]); scope masks are bool[n] (None: every splat).  Nothing here looks at the device code.

    deg_i   = #{ j in S : near(i, j) }
    core_i  := i in S, finite, deg_i >= min_pts
    i ~ j   := core_i and core_j and near(i, j);  clusters = the classes of the transitive closure of ~ over core splats
    label_i = the smallest index of i's class (core);  min{ label_j : core_j and near(i, j) } (non-core, finite, in S, with such a j:
              border);  NONE otherwise (noise, non-finite, out of scope)
    size_i  = #{ k : label_k == label_i } if label_i != NONE else 0
"""
import numpy as np

import neighbour_reference as nr

NONE = 0xffffffff            # GSR_CLUSTER_NONE: a label
LARGEST = 0xffffffff         # GSR_CLUSTER_LARGEST: a seed
MAX_MIN_PTS = nr.MAX_CAP
MIN_PTS = (0, 1, 3, 6)       # the thresholds both test files run every shape at


def pairs(positions, radius, scope_mask=None, block=512):
    """(deg int64[n], a int64[m], b int64[m], finite bool[n]): deg_i for i in S (0 outside), every near pair of S once with a > b,
    and the splats with finite positions.  The pair test is neighbour_reference.counts', f64 in the written order: a NaN or infinite
    component makes every comparison false."""
    p = nr._positions(positions)
    n = p.shape[0]
    s = nr._scope(scope_mask, n)
    r2 = np.float64(radius) * np.float64(radius)
    idx = np.nonzero(s)[0]
    q = p[idx]
    deg = np.zeros(n, dtype=np.int64)
    aa, bb = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, idx.size, block):
            me = q[a:a + block]
            dx = me[:, None, 0] - q[None, :, 0]
            dy = me[:, None, 1] - q[None, :, 1]
            dz = me[:, None, 2] - q[None, :, 2]
            near = ((dx * dx + dy * dy) + dz * dz) <= r2
            k = np.arange(me.shape[0])
            near[k, a + k] = False                       # a splat is not its own neighbour
            deg[idx[a:a + block]] = near.sum(axis=1)
            rows, cols = np.nonzero(near)
            keep = cols < rows + a
            aa.append(idx[rows[keep] + a])
            bb.append(idx[cols[keep]])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return deg, cat(aa), cat(bb), np.isfinite(p).all(axis=1)


def _roots(n, a, b):
    """int64[n]: the smallest index of every index's class under the pairs (a, b): a host union-find, the larger root hooked onto
    the smaller, so that a root is its class's smallest index"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in zip(a.tolist(), b.tolist()):
        ri, rj = find(i), find(j)
        if ri < rj:
            parent[rj] = ri
        elif rj < ri:
            parent[ri] = rj
    return np.array([find(x) for x in range(n)], dtype=np.int64)


class Clusters:
    """labels uint32[n], sizes uint32[n], core / border bool[n], info: the dict of gsr_cluster_info without pair_bound and budget"""

    def __init__(self, positions, radius, min_pts, scope_mask=None, known_pairs=None):
        deg, a, b, finite = pairs(positions, radius, scope_mask) if known_pairs is None else known_pairs
        n = deg.size
        s = nr._scope(scope_mask, n)
        core = s & finite & (deg >= min_pts)
        both = core[a] & core[b]
        root = _roots(n, a[both], b[both])
        label = np.full(n, NONE, dtype=np.int64)
        label[core] = root[core]
        # border: a non-core finite splat in S takes the smallest label among its near core splats
        best = np.full(n, NONE, dtype=np.int64)
        for x, y in ((a, b), (b, a)):
            take = ~core[x] & core[y]
            np.minimum.at(best, x[take], label[y[take]])
        border = s & finite & ~core & (best != NONE)
        label[border] = best[border]
        self.labels = label.astype(np.uint32)
        self.core, self.border = core, border
        labelled = label != NONE
        per_label = np.bincount(label[labelled], minlength=n) if labelled.any() else np.zeros(n, dtype=np.int64)
        self.sizes = np.where(labelled, per_label[np.where(labelled, label, 0)], 0).astype(np.uint32)
        roots = np.nonzero(per_label)[0]
        largest_label, largest_size = NONE, 0
        if roots.size:
            largest_size = int(per_label[roots].max())
            largest_label = int(roots[per_label[roots] == largest_size].min())      # ties: the smallest label
        in_scope = int(s.sum())
        self.info = {"in_scope": in_scope, "nonfinite": int((s & ~finite).sum()), "core": int(core.sum()), "border": int(border.sum()),
                     "noise": in_scope - int(core.sum()) - int(border.sum()), "clusters": int(roots.size),
                     "largest_label": largest_label, "largest_size": largest_size}
        for arr in (self.labels, self.sizes, self.core, self.border):
            arr.setflags(write=False)


def select(sizes, lo, hi, scope_mask=None):
    """bool[n]: in S and lo <= size < hi"""
    c = np.asarray(sizes, dtype=np.uint32).astype(np.int64)
    return nr._scope(scope_mask, c.size) & (c >= lo) & (c < hi)


def select_at(labels, seed, largest_label=NONE):
    """bool[n]: the splats labelled like `seed` (LARGEST: like largest_label); nobody when that label is NONE"""
    lab = np.asarray(labels, dtype=np.uint32)
    target = largest_label if seed == LARGEST else int(lab[seed])
    return (lab == target) & (target != NONE)


# ---- the shapes of both test files ----
def chain(n=4096, radius=0.25, seed=None):
    """n splats spaced exactly `radius` apart along a line (a power of two: every coordinate and difference exact), in index order
    or in a seeded permutation: deep trees and long hook retries for a union that links neighbours in index order"""
    x = np.arange(n, dtype=np.float64) * radius - 100.0
    p = np.stack([x, np.full(n, 0.5), np.full(n, -1.25)], axis=1).astype(np.float32)
    return p if seed is None else p[np.random.default_rng(seed).permutation(n)]


def coincident_groups(groups=64, each=65):
    """groups * each splats: splat i sits at group i % groups' point, the points a unit apart -- `groups` clusters of equal size, so the
    largest is a tie, and every splat's class is reached through coincident neighbours only"""
    g = np.arange(groups * each) % groups
    return np.stack([g * 1.0, g * 0.0 + 0.25, g * -0.0 - 3.0], axis=1).astype(np.float32)


def shapes():
    """[(name, positions f32[n, 3], radius)]: neighbour_reference.families() and the two shapes a union can go wrong on"""
    seen, out = set(), []
    for name, p, radius, _ in nr.families():
        if name.startswith("300 coincident"):
            if "300 coincident" in seen:
                continue                                    # (the two differ in their cap only)
            name = "300 coincident"
        seen.add(name)
        out.append((name, p, radius))
    out.append(("chain of 4096 in index order", chain(), 0.25))
    out.append(("chain of 4096 permuted", chain(seed=23), 0.25))
    out.append(("64 coincident groups of 65", coincident_groups(), 0.25))
    return out
