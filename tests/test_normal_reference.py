"""tests/normal_reference.py, the specification of "normals", against facts that do not come from it: lattices whose normals and
variations are known by hand, a sphere whose normals are its radii, numpy.linalg.eigh on random neighbourhoods, the splat's own
covariance for the OWN source, and the array form of the specification against its scalar form bit for bit."""
import numpy as np
import pytest

import knn_reference as kr
import merge_reference as mr
import normal_reference as nm


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_plane_lattice_has_exact_normals():
    p, radius, k = nm.plane_lattice()
    normals, variation, found = nm.knn_normals(p, radius, k)
    assert np.array_equal(normals, np.tile(np.float32([0, 0, 1]), (25, 1)))
    assert np.array_equal(_bits(variation), _bits(np.zeros(25)))
    grid = found.reshape(5, 5)
    assert [int(grid[y, x]) for y, x in ((0, 0), (0, 4), (4, 0), (4, 4))] == [2, 2, 2, 2] and grid[2, 2] == 4
    assert nm.info(p, variation) == {"in_scope": 25, "nonfinite": 0, "valid": 25, "variation_min": 0.0, "variation_max": 0.0}


def test_cube_lattice_ties_go_to_column_zero():
    g = (-1.0, 0.0, 1.0)
    p = np.array([[x, y, z] for z in g for y in g for x in g], dtype=np.float32)
    normals, variation, found = nm.knn_normals(p, 1.0, 6)
    centre = 13
    assert found[centre] == 6
    pts = [p[centre].astype(np.float64).tolist()] + [p[j].astype(np.float64).tolist() for j in kr.lists(p, 1.0, 6)[1][centre]]
    _, _, _, lam, _ = nm.one(pts)
    assert lam == [2.0 / 7.0] * 3
    assert normals[centre].tolist() == [1.0, 0.0, 0.0] and variation[centre] == 0.3333333333333333


def test_collinear_coincident_and_single_neighbour():
    normals, variation, found = nm.knn_normals(np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0]]), 5.0, 4)
    assert found.tolist() == [2, 2, 2] and np.array_equal(normals, np.tile(np.float32([0, 1, 0]), (3, 1))) and not variation.any()
    normals, variation, found = nm.knn_normals(np.float32([[0.5, 0.25, 2.0]] * 3), 1.0, 4)
    assert found.tolist() == [2, 2, 2] and np.isnan(normals).all() and np.isnan(variation).all()        # tot == 0
    assert (normals.view(np.uint32) == 0x7fc00000).all() and (variation.view(np.uint64) == 0x7ff8000000000000).all()
    normals, variation, found = nm.knn_normals(np.float32([[0, 0, 0], [0.5, 0, 0], [9, 9, 9]]), 1.0, 4)
    assert found.tolist() == [1, 1, 0] and np.isnan(normals).all() and np.isnan(variation).all()
    assert nm.info(np.float32([[0, 0, 0], [0.5, 0, 0], [9, 9, 9]]), variation)["valid"] == 0


@pytest.fixture(scope="module")
def sphere():
    p, radius, k = nm.sphere()
    lists = kr.lists(p, radius, k)
    return p, radius, k, lists


def test_sphere_normals_are_its_radii(sphere):
    p, radius, k, lists = sphere
    normals, variation, found = nm.knn_normals(p, radius, k, lists=lists)
    assert (found == k).all()
    p64 = p.astype(np.float64)
    radial = p64 / np.linalg.norm(p64, axis=1, keepdims=True)
    cos = np.abs((normals.astype(np.float64) * radial).sum(axis=1))
    print("min |n . p/|p||", cos.min(), "max variation", variation.max())
    assert cos.min() >= 0.999 and variation.max() <= 0.002
    first = np.where(normals[:, 0] != 0, normals[:, 0], np.where(normals[:, 1] != 0, normals[:, 1], normals[:, 2]))
    assert (first > 0).all()
    inward, v2, _ = nm.knn_normals(p, radius, k, toward=(0.0, 0.0, 0.0), lists=lists)
    assert ((inward.astype(np.float64) * p64).sum(axis=1) < 0).all()
    assert np.array_equal(np.abs(inward), np.abs(normals)) and np.array_equal(_bits(v2), _bits(variation))
    outward, _, _ = nm.knn_normals(p, radius, k, toward=(0.0, 0.0, 50.0), lists=lists)
    assert ((outward.astype(np.float64) * (np.float64([0, 0, 50]) - p64)).sum(axis=1) > 0).all()


def test_the_array_form_is_the_scalar_form_bit_for_bit(sphere):
    p, radius, k, lists = sphere
    rng = np.random.default_rng(5)
    q = rng.normal(0, 1, (300, 3)).astype(np.float32)
    for pos, rad, kk, ls, toward in ((p[:256], radius, k, None, None), (q, 0.8, 5, None, (0.3, -2.0, 0.1)), (q, 0.5, 32, None, None)):
        ls = kr.lists(pos, rad, kk)
        normals, variation, found = nm.knn_normals(pos, rad, kk, toward=toward, lists=ls)
        p64 = pos.astype(np.float64)
        for i in range(pos.shape[0]):
            m = int(found[i])
            if m < 2:
                assert np.isnan(variation[i])
                continue
            u, var, tot, _, _ = nm.one([p64[i].tolist()] + [p64[j].tolist() for j in ls[1][i, :m]])
            assert tot > 0
            u = nm.orient_one(u, p64[i].tolist(), toward)
            assert np.array_equal(np.float64(u).astype(np.float32).view(np.uint32), normals[i].view(np.uint32)), i
            assert _bits([var])[0] == _bits(variation[i:i + 1])[0], i


def test_against_eigh_on_random_neighbourhoods():
    rng = np.random.default_rng(11)
    worst_dot = worst_orth = 0.0
    checked = 0
    for _ in range(2000):
        m = int(rng.integers(3, 14))
        basis = np.linalg.qr(rng.normal(0, 1, (3, 3)))[0]
        spread = rng.uniform(0.001, 1.0, 3) * np.float64([1.0, 0.3, 0.05])
        pts = (rng.normal(0, 1, (m, 3)) * spread) @ basis.T + rng.uniform(-2, 2, 3)
        pts = pts.astype(np.float32).astype(np.float64)
        u, var, tot, lam, V = nm.one(pts.tolist())
        V = np.array(V)
        worst_orth = max(worst_orth, float(np.abs(V.T @ V - np.eye(3)).max()))
        C = np.cov(pts.T, bias=True)
        w, E = np.linalg.eigh(C)
        if w[1] - w[0] > 1e-6 * w[2]:
            worst_dot = max(worst_dot, 1.0 - abs(float(np.dot(u, E[:, 0]))))
            checked += 1
        assert abs(var - max(w[0], 0.0) / w.sum()) <= 1e-9
        assert abs(np.linalg.norm(u) - 1.0) <= 1e-14
    print("worst 1 - |dot|", worst_dot, "worst |V^T V - I|", worst_orth, "checked", checked)
    assert checked > 1500 and worst_dot <= 1e-12 and worst_orth <= 1e-14


def test_own_source_is_the_shortest_axis_of_the_splats_covariance():
    rng = np.random.default_rng(3)
    n = 200
    pos = rng.normal(0, 1, (n, 3)).astype(np.float32)
    rot = rng.normal(0, 1, (n, 4))
    rot = (rot / np.linalg.norm(rot, axis=1, keepdims=True)).astype(np.float32)
    scl = rng.uniform(0.01, 0.5, (n, 3)).astype(np.float32)
    scl[::3] *= -1.0                                                  # the sign of a scale does not matter
    scl[7] = [0.2, 0.1, 0.1]                                          # a tie goes to the smallest k
    scl[8] = [0.1, 0.1, 0.1]
    rot[9] = 0.0                                                      # a zero quaternion is no rotation: invalid
    rot[10] = [0.0, 0.0, 0.0, np.nan]
    scl[11] = 0.0                                                     # tot == 0
    scl[12, 1] = np.inf
    pos[13, 2] = np.nan
    normals, variation, found = nm.own_normals(pos, rot, scl)
    assert not found.any()
    bad = [9, 10, 11, 12, 13]
    assert np.isnan(normals[bad]).all() and np.isnan(variation[bad]).all()
    good = np.setdiff1d(np.arange(n), bad)
    assert np.isfinite(normals[good]).all() and np.isfinite(variation[good]).all()
    for i in good:
        C = mr.cov_of_row(rot[i], scl[i])
        a = normals[i].astype(np.float64)
        smin = float(np.abs(scl[i].astype(np.float64)).min())
        assert abs(a @ C @ a - smin * smin) <= 1e-6 * smin * smin, i
        assert abs(variation[i] - smin * smin / float((scl[i].astype(np.float64) ** 2).sum())) <= 1e-15
    R7 = np.array(_rotation(rot[7]))
    assert np.allclose(np.abs(normals[7]), np.abs(R7[1]), atol=1e-7) and np.allclose(np.abs(normals[8]), np.abs(_rotation(rot[8])[0]), atol=1e-7)
    # a scope: rows outside it hold NaN and count nowhere
    mask = np.arange(n) % 2 == 0
    n2, v2, _ = nm.own_normals(pos, rot, scl, mask)
    assert np.isnan(n2[~mask]).all() and np.array_equal(n2[mask].view(np.uint32), normals[mask].view(np.uint32))
    assert nm.info(pos, v2, mask) == {"in_scope": n // 2, "nonfinite": 0, "valid": int(np.isin(good, np.nonzero(mask)[0]).sum()),
                                      "variation_min": float(np.nanmin(v2)), "variation_max": float(np.nanmax(v2))}
    # oriented
    n3, _, _ = nm.own_normals(pos, rot, scl, toward=(5.0, 5.0, 5.0))
    d = (n3[good].astype(np.float64) * (np.float64([5, 5, 5]) - pos[good].astype(np.float64))).sum(axis=1)
    assert (d > 0).all()


def _rotation(rot):
    qx, qy, qz, qw = float(rot[1]), float(rot[2]), float(rot[3]), -float(rot[0])
    return [[1 - 2 * qy * qy - 2 * qz * qz, 2 * qx * qy - 2 * qz * qw, 2 * qx * qz + 2 * qy * qw],
            [2 * qx * qy + 2 * qz * qw, 1 - 2 * qx * qx - 2 * qz * qz, 2 * qy * qz - 2 * qx * qw],
            [2 * qx * qz - 2 * qy * qw, 2 * qy * qz + 2 * qx * qw, 1 - 2 * qx * qx - 2 * qy * qy]]


def test_picker_rule_on_stored_normals():
    normals = np.float32([[0, 0, 1], [0, 1, 0], [0.6, 0, -0.8], [np.nan] * 3, [0, 0, -1]])
    variation = np.float64([0.0, 0.1, 0.25, np.nan, 1.0 / 3.0])
    up = (0.0, 0.0, 2.0)
    assert nm.values(normals, variation, "dot", up)[:3].tolist() == [2.0, 0.0, float(np.float32(-0.8)) * 2.0]
    assert nm.select(normals, variation, "dot", 0.0, 2.0, up).tolist() == [True, True, False, False, False]          # both ends closed
    assert nm.select(normals, variation, "dot", -np.inf, np.inf, up).tolist() == [True, True, True, False, True]      # a NaN row is never picked
    assert nm.select(normals, variation, "abs_dot", 1.5, 2.0, up).tolist() == [True, False, True, False, True]
    assert nm.select(normals, variation, "variation", 0.1, 0.25).tolist() == [False, True, True, False, False]
    assert nm.select(normals, variation, "variation", 0.0, 0.0).tolist() == [True, False, False, False, False]
    assert not nm.select(normals, variation, "variation", -np.inf, np.inf)[3]
    with pytest.raises(ValueError):
        nm.values(normals, variation, "median", up)


def test_families_hold_the_knn_shapes_with_k_of_two_or_more():
    names = [f[0] for f in nm.families()]
    assert all(f[3] >= 2 for f in nm.families()) and len(names) == len(set(names))
    for want in ("n = 1, k 3", "n = 65, k 8", "n = 257, k 8", "300 coincident, k 32", "lattice beyond the clamp, k 6", "non-finite rows, k 4",
                 "clusters and floaters, k 2", "clusters and floaters, k 8", "clusters and floaters, k 32", "plane lattice, k 8", "sphere, k 12"):
        assert want in names, want
