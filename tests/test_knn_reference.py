"""tests/knn_reference.py against itself, without a GPU: the blocked numpy specification equals a brute-force double loop on small
inputs, the hand cases of the definition hold (one splat, two at exactly the radius, two one ulp beyond, the tie that goes to the
smaller index), d2 is symmetric, the histogram sums to the scope, and the values follow the written association."""
import numpy as np
import pytest

import knn_reference as kr
import neighbour_reference as nr

SMALL = [f for f in kr.families() if f[1].shape[0] <= 65]


@pytest.mark.parametrize("case", SMALL, ids=[f[0] for f in SMALL])
def test_lists_equal_the_double_loop(case):
    _, p, radius, k = case
    n = p.shape[0]
    for mask in (None, np.arange(n) % 3 != 1):
        found, idx, d2 = kr.lists(p, radius, k, mask)
        bf, bi, bd = kr.brute(p, radius, k, mask)
        assert np.array_equal(found, bf) and np.array_equal(idx, bi)
        assert np.array_equal(d2.view(np.uint64), bd.view(np.uint64))


def test_the_double_loop_on_random_clouds_with_ties_and_nonfinite_rows():
    rng = np.random.default_rng(3)
    p = (rng.integers(-3, 4, (60, 3)) * 0.25).astype(np.float32)          # a coarse grid: many equal distances and coincident splats
    p = nr.with_nonfinite(p)
    for k in (1, 5, 32):
        found, idx, d2 = kr.lists(p, 0.5, k, block=7)
        bf, bi, bd = kr.brute(p, 0.5, k)
        assert np.array_equal(found, bf) and np.array_equal(idx, bi) and np.array_equal(d2.view(np.uint64), bd.view(np.uint64))
        bad = ~np.isfinite(p).all(axis=1)
        assert bad.sum() == 5 and not found[bad].any()                        # (three of the eight planted values are 3e38: finite) and not np.isin(idx, np.nonzero(bad)[0]).any()
        for stat in kr.STATS:
            assert np.isposinf(kr.values(found, d2, k, stat)[bad]).all()


def test_hand_cases():
    by = {f[0]: f for f in kr.families()}
    _, p, radius, k = by["n = 1, k 3"]
    found, idx, d2 = kr.lists(p, radius, k)
    assert found.tolist() == [0] and (idx == kr.NONE).all() and np.isposinf(d2).all()
    for stat in kr.STATS:
        assert np.isposinf(kr.values(found, d2, k, stat)).all()
    _, p, radius, k = by["n = 2 at exactly radius, k 3"]
    found, idx, d2 = kr.lists(p, radius, k)
    assert found.tolist() == [1, 1] and idx[:, 0].tolist() == [1, 0] and (d2[:, 0] == np.float64(radius) * np.float64(radius)).all()
    assert (idx[:, 1:] == kr.NONE).all() and np.isposinf(d2[:, 1:]).all()
    assert kr.values(found, d2, k, "mean").tolist() == [radius, radius] and np.isposinf(kr.values(found, d2, k, "kth")).all()
    assert kr.values(found, d2[:, :1], 1, "kth").tolist() == [radius, radius]
    _, p, radius, k = by["n = 2 one ulp beyond, k 3"]
    found, idx, d2 = kr.lists(p, radius, k)
    assert found.tolist() == [0, 0] and (idx == kr.NONE).all()
    # three collinear splats with equal gaps: the middle one's two neighbours tie, and the tie goes to the smaller index
    p = np.array([[0.5, 0.0, 0.0], [0.25, 0.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    found, idx, d2 = kr.lists(p, 1.0, 1)
    assert found.tolist() == [1, 1, 1] and idx[:, 0].tolist() == [1, 0, 1]
    found, idx, d2 = kr.lists(p, 1.0, 2)
    assert idx.tolist() == [[1, 2], [0, 2], [1, 0]] and d2[1].tolist() == [0.0625, 0.0625]


def test_d2_is_symmetric_and_lists_are_sorted():
    _, p, radius, _ = [f for f in kr.families() if f[0].startswith("n = 65")][0]
    n = p.shape[0]
    found, idx, d2 = kr.lists(p, radius, 32)
    seen = {}
    for i in range(n):
        pairs = [(d2[i, t], idx[i, t]) for t in range(found[i])]
        assert pairs == sorted(pairs)
        for d, j in pairs:
            seen[(i, int(j))] = d
    both = [(i, j) for (i, j) in seen if (j, i) in seen]
    assert both and all(seen[(i, j)] == seen[(j, i)] for i, j in both)


def test_histogram_info_and_selection():
    _, p, radius, k = [f for f in kr.families() if f[0] == "non-finite rows, k 4"][0]
    n = p.shape[0]
    for mask in (None, np.arange(n) % 3 != 1):
        found, idx, d2 = kr.lists(p, radius, k, mask)
        in_scope = n if mask is None else int(mask.sum())
        h = kr.hist(found, k, mask)
        assert h.shape == (k + 1,) and int(h.sum()) == in_scope
        assert np.array_equal(found, np.minimum(nr.counts(p, radius, nr.MAX_CAP, mask), k))      # found is the neighbour count, cut at k
        for stat in kr.STATS:
            v = kr.values(found, d2, k, stat, mask)
            info = kr.info(p, found, v, k, mask)
            assert info["in_scope"] == in_scope and info["complete"] == int(h[k]) and info["nonfinite"] == nr.nonfinite(p, mask)
            assert np.isnan(v).sum() == n - in_scope
            fin = np.isfinite(v)
            assert info["finite_values"] == int(fin.sum()) and info["value_min"] == v[fin].min() and info["value_max"] == v[fin].max()
            assert info["finite_values"] == (int(h[k]) if stat == "kth" else in_scope - int(h[0]))
            everything = kr.select(v, 0.0, np.inf, mask)
            assert int(everything.sum()) == in_scope                                             # hi = +inf: no upper end, the +inf values included
            assert int(kr.select(v, 0.0, 1e300, mask).sum()) == info["finite_values"]            # a finite hi leaves them out
            assert not kr.select(v, 0.1, 0.1, mask).any()
            assert np.array_equal(kr.select(v, np.inf, np.inf, mask), np.isposinf(v))
    empty = kr.info(p, np.zeros(n, np.uint32), np.full(n, np.inf), k)
    assert empty["finite_values"] == 0 and empty["value_min"] == np.inf and empty["value_max"] == -np.inf


def test_the_mean_is_the_sequential_sum():
    d2 = np.array([[1e-32, 1.0, 4.0, np.inf]], np.float64)
    found = np.array([3], np.uint32)
    want = ((np.sqrt(np.float64(1e-32)) + np.float64(1.0)) + np.float64(2.0)) / np.float64(3.0)
    assert kr.values(found, d2, 4, "mean")[0] == want
    assert np.isposinf(kr.values(found, d2, 4, "kth")[0])


def test_the_outlier_threshold():
    v = np.array([1.0, 2.0, 3.0, np.inf, np.nan, 6.0])
    mu, sigma = 3.0, np.sqrt(14.0 / 3.0)
    assert kr.outlier_threshold(v, 2.0) == pytest.approx(mu + 2.0 * sigma, rel=1e-15)
    assert kr.outlier_threshold(np.array([1.0, np.inf]), 2.0) == np.inf
    assert kr.outlier_threshold(v, 1.0, np.array([1, 1, 0, 1, 1, 0], bool)) == pytest.approx(1.5 + np.sqrt(0.5), rel=1e-15)


def test_families_cover_what_the_gpu_tests_need():
    names = [f[0] for f in kr.families()]
    for name in ("n = 1, k 3", "n = 63, k 1", "n = 257, k 8", "300 coincident, k 7", "300 coincident, k 32", "lattice, k 6", "lattice 2^19 radii out, k 32",
                 "lattice beyond the clamp, k 6", "non-finite rows, k 4", "clusters and floaters, k 1", "clusters and floaters, k 8", "clusters and floaters, k 32"):
        assert name in names, name
    assert all(1 <= f[3] <= kr.MAX_K for f in kr.families())
    _, p, radius, k = [f for f in kr.families() if f[0] == "300 coincident, k 7"][0]
    found, idx, d2 = kr.lists(p, radius, k)
    assert (found == 7).all() and not d2.any()
    assert idx[0].tolist() == [1, 2, 3, 4, 5, 6, 7] and idx[3].tolist() == [0, 1, 2, 4, 5, 6, 7] and idx[299].tolist() == [0, 1, 2, 3, 4, 5, 6]
