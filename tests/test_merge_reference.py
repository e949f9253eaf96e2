"""tests/merge_reference.py pinned against itself and the definition (include/gsplat_hip.h, "merging cells"), no GPU: the row count
follows the formula, a cell small enough to hold every splat alone leaves every bit, coincident identical splats merge into the
same centre and covariance, opacity x volume is conserved, the stored quaternion is a unit one, the stored row reproduces the
mixture's covariance, and the collision family does collide in the hashed grid.

The covariance bound 2^-20 ||C||_F is f32 storage of three scales and four quaternion components: a relative 2^-24 on each scale
enters s^2 twice (2^-23 on every eigenvalue), and a 2^-24 perturbation of each of four quaternion components (|q_i| <= 1) turns R by
at most 2 * sqrt(4) * 2^-24 = 2^-22, which enters R^T diag(s^2) R twice (2^-21 of the largest eigenvalue); together below
2^-23 + 2^-21 < 2^-20 of ||C||_F, with the f64 steps (1.2e-15) far below.  The quaternion's norm moves by at most
sum |q_i| 2^-24 <= 2 * 2^-24 = 2^-23 < 2^-22."""
import numpy as np
import pytest

import merge_reference as mr

FAMILIES = mr.families()
BY_NAME = {f[0]: f for f in FAMILIES}
_MERGED = {}


def _merged(name):
    """the reference's merge of a family: computed once, shared, left unchanged"""
    if name not in _MERGED:
        _, arrays, cell = BY_NAME[name]
        _MERGED[name] = mr.merge(*arrays, cell)
    return _MERGED[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", [f[0] for f in FAMILIES])
def test_rows_after_equals_the_formula(name):
    _, (data, pos, rot, scl), cell = BY_NAME[name]
    out = _merged(name)
    info = out["info"]
    n = pos.shape[0]
    assert out["positions"].shape[0] == info["rows_after"] == n - info["merged_members"] + info["merged_cells"] == int(out["keep"].sum())
    assert int(out["merged"].sum()) == info["merged_cells"] and info["candidates"] <= info["in_scope"] == n
    leader, hist, info2 = mr.report(pos, rot, scl, cell, 64)
    assert info2 == info and hist[0] == 0 and int(hist.sum()) == info["cells"]
    assert int((leader != mr.NONE).sum()) == info["candidates"] and int((leader == np.arange(n)).sum()) == info["cells"]
    assert mr.pair_floor(pos, rot, scl, cell) >= info["candidates"]


@pytest.mark.parametrize("name", ["lattice on the cell edges", "400 cells of two", "8192 clustered", "non-finite rows"])
def test_a_cell_that_holds_every_splat_alone_leaves_every_bit(name):
    _, (data, pos, rot, scl), _ = BY_NAME[name]
    ok = np.isfinite(pos).all(axis=1)
    p = pos.copy()
    p[ok] = (np.arange(int(ok.sum()))[:, None] * np.array([[3.0, 0.0, 0.0]])).astype(np.float32)   # one splat per cell of side 1
    d = data.copy()
    d[:, 0:3] = p.view(np.uint32)
    out = mr.merge(d, p, rot, scl, 1.0)
    assert out["info"]["merged_cells"] == 0 and out["info"]["rows_after"] == p.shape[0] and not out["merged"].any()
    assert np.array_equal(out["data"], d) and np.array_equal(_bits(out["positions"]), _bits(p))
    assert np.array_equal(_bits(out["rotations"]), _bits(rot)) and np.array_equal(_bits(out["scales"]), _bits(scl))


def test_coincident_identical_splats_keep_centre_and_covariance(capsys):
    worst = 0.0
    for k in (2, 3, 17):
        for seed in range(8):
            d, p, r, s = (a.copy() for a in mr.scene(np.tile([[0.37, -0.21, 0.05]], (k, 1)), seed=seed))
            d[:], r[:], s[:] = d[0], r[0], s[0]
            out = mr.merge(d, p, r, s, 1.0)
            assert out["positions"].shape[0] == 1 and np.array_equal(_bits(out["positions"][0]), _bits(p[0]))
            C = mr.cov_of_row(r[0], s[0])
            got = mr.cov_of_row(out["rotations"][0], out["scales"][0])
            err = float(np.linalg.norm(got - C) / np.linalg.norm(C))
            worst = max(worst, err)
            assert err <= 2.0 ** -20, (k, seed, err)
            assert (out["data"][0, 7] & 0xffffff) == (d[0, 7] & 0xffffff)     # the colour of identical members is theirs
    with capsys.disabled():
        print("coincident identical splats: largest |S' - C|_F / |C|_F = %.3g (bound %.3g)" % (worst, 2.0 ** -20))


def test_opacity_is_k_times_a_when_the_volume_is_the_members():
    # axis-aligned identical members with scales that are exact in f32 through the square and the root: the merged volume IS the member's
    for k, a in ((2, 40), (3, 60), (5, 60), (4, 64)):
        d, p, r, s = (x.copy() for x in mr.scene(np.tile([[0.5, 0.5, 0.5]], (k, 1)), seed=k))
        r[:] = np.array([1.0, 0.0, 0.0, 0.0], np.float32)
        s[:] = np.array([0.5, 0.25, 0.125], np.float32)
        d[:, 7] = np.uint32(a << 24 | 0x102030)
        out = mr.merge(mr.repack(d, p, r, s), p, r, s, 1.0)
        assert np.array_equal(np.sort(out["scales"][0]), np.sort(s[0]))
        assert int(out["data"][0, 7]) >> 24 == min(255, k * a) and int(out["data"][0, 7]) & 0xffffff == 0x102030


@pytest.mark.parametrize("name", [f[0] for f in FAMILIES])
def test_quaternion_is_unit_and_the_stored_row_reproduces_the_mixture(name):
    out = _merged(name)
    rows = np.flatnonzero(out["merged"])
    assert rows.size == out["info"]["merged_cells"] == len(out["C"])
    worst_q = worst_c = 0.0
    for j in rows.tolist():
        q = out["rotations"][j].astype(np.float64)
        worst_q = max(worst_q, abs(float(np.sqrt((q * q).sum())) - 1.0))
        C = mr.sym(out["C"][j])
        norm = float(np.linalg.norm(C))
        if norm > 0:
            worst_c = max(worst_c, float(np.linalg.norm(mr.cov_of_row(out["rotations"][j], out["scales"][j]) - C)) / norm)
        else:
            assert not out["scales"][j].any()
    print(name, "quaternion norm off by", worst_q, "covariance off by", worst_c)
    assert worst_q <= 2.0 ** -22, worst_q
    assert worst_c <= 2.0 ** -20, worst_c


def test_the_collision_family_collides():
    _, (data, pos, rot, scl), cell = BY_NAME["400 cells of two"]
    _, _, members = mr.cells_of(pos, rot, scl, cell)
    assert len(members) == 400 and all(len(v) == 2 for v in members.values())
    mask = mr.buckets_of(pos.shape[0]) - 1
    assert mask == 2047
    cc = mr.cell_coords(pos, cell)
    buckets = [mr.nb_bucket(mr.cell_key(cc[l]), mask) for l in members]
    assert len(set(buckets)) < len(buckets), "no two occupied cells share a bucket"


def test_families_cover_the_edges():
    names = [f[0] for f in FAMILIES]
    for k in (63, 64, 65, 255, 256, 257):
        out = _merged("%d members in one cell" % k)
        assert out["info"]["largest"] == k and out["info"]["merged_cells"] == 1 and out["info"]["rows_after"] == 3
    lat = _merged("lattice on the cell edges")
    assert lat["info"]["cells"] == 8 ** 3 and lat["info"]["largest"] == 27      # k / 4 - ulp joins cell k - 1; -0.0 and +0.0 share cell 0
    far = _merged("rows beyond the clamp")["info"]
    assert far["merged_cells"] == 4 and far["merged_members"] == 11                 # both x ends, the far corner, and the pair at the origin
    nf = _merged("non-finite rows")
    assert nf["info"]["candidates"] == 6 and nf["info"]["in_scope"] == 12 and nf["info"]["rows_after"] == 7
    assert _merged("a cell of opacity 0")["data"][0, 7] >> 24 == 0
    z = _merged("coincident zero-scale splats")
    assert not z["scales"][0].any() and z["rotations"][0].tolist() == [-1.0, 0.0, 0.0, 0.0]
    big = _merged("8192 clustered")["info"]
    assert 3.0 < big["candidates"] / big["cells"] < 6.0 and "two splats in two cells" in names
