"""Clusters without a GPU: tests/cluster_reference.py is the definition it claims to be.  Its partition of the core splats equals
scipy's connected components of the same near matrix (at min_pts = 0 that is the whole statement), its border labels equal a
dense restatement, the hand cases have the labels and sizes written beside them, and the shapes of tests/test_gpu_clusters.py hold
what they are there for: borders, noise, ties, deep chains."""
import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import cluster_reference as cr
import neighbour_reference as nr

SHAPES = cr.shapes()
BY_NAME = {s[0]: s for s in SHAPES}
NONE = cr.NONE
_PAIRS = {}


def _pairs(name, scope_key=None, mask=None):
    key = (name, scope_key)
    if key not in _PAIRS:
        _, p, radius = BY_NAME[name]
        _PAIRS[key] = cr.pairs(p, radius, mask)
    return _PAIRS[key]


def _labels_by_scipy(n, a, b, members):
    """uint32[n]: the smallest index of every member's component of the graph (a, b) restricted to members; NONE for the others"""
    keep = members[a] & members[b]
    g = coo_matrix((np.ones(int(keep.sum()), np.int8), (a[keep], b[keep])), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    smallest = np.full(n, n, dtype=np.int64)
    idx = np.nonzero(members)[0]
    np.minimum.at(smallest, comp[idx], idx)
    out = np.full(n, NONE, dtype=np.int64)
    out[idx] = smallest[comp[idx]]
    return out.astype(np.uint32)


@pytest.mark.parametrize("min_pts", cr.MIN_PTS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_the_partition_is_scipys_and_the_rest_follows_the_definition(shape, min_pts):
    name, p, radius = shape
    n = p.shape[0]
    for scope_key, mask in ((None, None), ("visible", np.arange(n) % 3 != 1)):
        known = _pairs(name, scope_key, mask)
        deg, a, b, finite = known
        c = cr.Clusters(p, radius, min_pts, mask, known)
        s = nr._scope(mask, n)
        # the degrees are the neighbour counts, uncapped
        assert np.array_equal(np.minimum(deg, nr.MAX_CAP), nr.counts(p, radius, nr.MAX_CAP, mask)), name
        core = s & finite & (deg >= min_pts)
        assert np.array_equal(c.core, core)
        if min_pts == 0:
            assert np.array_equal(core, s & finite) and not c.border.any()
        # core labels: scipy's components of the core graph, named by their smallest index
        want = _labels_by_scipy(n, a, b, core)
        assert np.array_equal(c.labels[core], want[core]), name
        # border labels, restated per splat; everything else has none
        others = np.nonzero(s & finite & ~core)[0]
        for i in others[::max(1, others.size // 64)]:        # (every one of them up to 127, a spread of the large shapes')
            near_core = np.concatenate([b[(a == i) & core[b]], a[(b == i) & core[a]]])
            assert int(c.labels[i]) == (int(want[near_core].min()) if near_core.size else NONE), (name, i)
            assert bool(c.border[i]) == bool(near_core.size)
        assert (c.labels[~s | ~finite] == NONE).all()
        # sizes: constant within a label, the label's population; 0 without a label
        labelled = c.labels != NONE
        assert not c.sizes[~labelled].any()
        for lab in np.unique(c.labels[labelled]):
            members = c.labels == lab
            assert (c.sizes[members] == members.sum()).all() and c.labels[lab] == lab and c.core[lab]      # a label is a core splat of its own cluster
            assert np.nonzero(members & c.core)[0].min() == lab                                              # the smallest CORE index: a border splat's may be lower
        info = c.info
        assert info["in_scope"] == int(s.sum()) == info["core"] + info["border"] + info["noise"]
        assert info["nonfinite"] == nr.nonfinite(p, mask) <= info["noise"]
        assert info["clusters"] == np.unique(c.labels[labelled]).size
        if info["clusters"]:
            assert info["largest_size"] == int(c.sizes.max()) and info["largest_label"] == int(c.labels[c.sizes == c.sizes.max()].min())
        else:
            assert info["largest_size"] == 0 and info["largest_label"] == NONE
        # the pickers
        assert int(cr.select(c.sizes, 0, 1, mask).sum()) == info["noise"]
        assert int(cr.select(c.sizes, 1, 2 ** 32 - 1, mask).sum()) == info["core"] + info["border"]
        assert not cr.select(c.sizes, 2, 2, mask).any()
        assert int(cr.select_at(c.labels, cr.LARGEST, info["largest_label"]).sum()) == info["largest_size"]


def test_two_splats_at_the_radius_and_one_ulp_beyond():
    _, p, r = BY_NAME["n = 2 at exactly radius"]
    for min_pts in (0, 1):
        c = cr.Clusters(p, r, min_pts)
        assert c.labels.tolist() == [0, 0] and c.sizes.tolist() == [2, 2] and c.info["clusters"] == 1      # distance exactly radius links
    assert cr.Clusters(p, r, 2).labels.tolist() == [NONE, NONE]
    _, p, r = BY_NAME["n = 2 one ulp beyond"]
    c = cr.Clusters(p, r, 0)
    assert c.labels.tolist() == [0, 1] and c.sizes.tolist() == [1, 1] and c.info["clusters"] == 2 and c.info["largest_label"] == 0
    c = cr.Clusters(p, r, 1)
    assert c.labels.tolist() == [NONE, NONE] and c.sizes.tolist() == [0, 0] and c.info["noise"] == 2 and c.info["largest_label"] == NONE


def _bridge(order):
    """two groups of four splats 0.1 apart and one splat between them that is near the facing end of either group only (radius 1);
    order: the indices of (group A, the bridge, group B)"""
    xs = {"a": [0.0, 0.1, 0.2, 0.3], "bridge": [1.25], "b": [2.2, 2.3, 2.4, 2.5]}
    x = np.concatenate([xs[k] for k in order])
    return np.stack([x, np.zeros(9), np.zeros(9)], axis=1).astype(np.float32)


def test_a_non_core_bridge_does_not_merge_two_groups():
    p = _bridge(("a", "bridge", "b"))
    c = cr.Clusters(p, 1.0, 3)                               # the bridge has two neighbours: not core
    assert c.labels.tolist() == [0, 0, 0, 0, 0, 5, 5, 5, 5] and c.sizes.tolist() == [5] * 5 + [4] * 4
    assert c.info == {"in_scope": 9, "nonfinite": 0, "core": 8, "border": 1, "noise": 0, "clusters": 2, "largest_label": 0, "largest_size": 5}
    c = cr.Clusters(p, 1.0, 2)                               # as a core splat it links them
    assert c.labels.tolist() == [0] * 9 and c.sizes.tolist() == [9] * 9 and c.info["clusters"] == 1
    assert cr.Clusters(p, 1.0, 0).labels.tolist() == [0] * 9


def test_a_border_splat_near_two_clusters_takes_the_smaller_label():
    c = cr.Clusters(_bridge(("bridge", "b", "a")), 1.0, 3)    # the bridge is splat 0; the clusters are 1 (b) and 5 (a)
    assert c.labels.tolist() == [1, 1, 1, 1, 1, 5, 5, 5, 5] and c.sizes.tolist() == [5] * 5 + [4] * 4
    c = cr.Clusters(_bridge(("b", "a", "bridge")), 1.0, 3)    # whichever group comes first in the walk: the smaller label
    assert c.labels.tolist() == [0, 0, 0, 0, 4, 4, 4, 4, 0] and c.border.tolist() == [False] * 8 + [True]


def test_ties_for_the_largest_go_to_the_smallest_label():
    x = np.array([0.0, 0.1, 10.0, 20.0, 10.1, 20.1, 10.2, 20.2])           # {0, 1}, {2, 4, 6}, {3, 5, 7}
    p = np.stack([x, np.zeros(8), np.zeros(8)], axis=1).astype(np.float32)
    c = cr.Clusters(p, 0.5, 0)
    assert c.labels.tolist() == [0, 0, 2, 3, 2, 3, 2, 3] and c.sizes.tolist() == [2, 2, 3, 3, 3, 3, 3, 3]
    assert c.info["clusters"] == 3 and c.info["largest_label"] == 2 and c.info["largest_size"] == 3
    assert cr.select_at(c.labels, cr.LARGEST, 2).tolist() == [False, False, True, False, True, False, True, False]
    assert cr.select_at(c.labels, 7).tolist() == [False, False, False, True, False, True, False, True]
    assert cr.select(c.sizes, 0, 3).tolist() == [True, True] + [False] * 6


def test_the_shapes_hold_what_they_are_there_for():
    _, p, r = BY_NAME["lattice"]
    assert {k: cr.Clusters(p, r, 6).info[k] for k in ("core", "border", "noise", "clusters")} == {"core": 1000, "border": 600, "noise": 128, "clusters": 1}
    for name in ("chain of 4096 in index order", "chain of 4096 permuted"):
        _, p, r = BY_NAME[name]
        for min_pts in (0, 1):
            c = cr.Clusters(p, r, min_pts, known_pairs=_pairs(name))
            assert c.info["clusters"] == 1 and c.info["largest_size"] == 4096 and (c.labels == 0).all()     # one island, every link at exactly radius
        assert cr.Clusters(p, r, 3, known_pairs=_pairs(name)).info["noise"] == 4096                          # nobody has three neighbours
    _, p, r = BY_NAME["64 coincident groups of 65"]
    c = cr.Clusters(p, r, 6, known_pairs=_pairs("64 coincident groups of 65"))
    assert np.array_equal(c.labels, np.arange(64 * 65) % 64) and (c.sizes == 65).all() and c.info["largest_label"] == 0
    _, p, r = BY_NAME["non-finite rows"]
    c = cr.Clusters(p, r, 0)
    bad = ~np.isfinite(p).all(axis=1)
    assert (c.labels[bad] == NONE).all() and c.info["nonfinite"] == 5 and c.info["noise"] == 5    # in scope, never core, nobody's neighbour
    _, p, r = BY_NAME["clusters and floaters"]
    infos = [cr.Clusters(p, r, m, known_pairs=_pairs("clusters and floaters")).info for m in cr.MIN_PTS]
    assert infos[0]["clusters"] > 100 and infos[0]["noise"] == 0             # every floater is an island of its own
    assert all(i["border"] > 0 and i["noise"] > 0 for i in infos[2:])        # thresholds leave borders and noise
